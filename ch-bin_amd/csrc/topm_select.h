// The sorted (distance, index) nearest-member list of a lane group, shared by the selection kernels (topm_kernels.hip)
// and the recruit kernel (recruit_kernels.hip).  Device code only, internal linkage.
#pragma once
#include "chb_internal.h"

#include <math.h>

namespace chb {
namespace {

__device__ __forceinline__ bool lex_less(double d0, int i0, double d1, int i1)
{
    return d0 < d1 || (d0 == d1 && i0 < i1);
}

// s-domain (squared distance) admission bound for a list whose m-th entry has distance e:
// sqrt(s) <= e  implies  s <= e*e*(1 + 2^-50)
__device__ __forceinline__ double tau_from(double e) { return e * e * (1.0 + 0x1p-50); }

// Offer the (up to) NC candidates held by every lane of a W-lane group to the group's sorted
// list (lane t of the group holds entry t).  Wave-synchronous; all 64 lanes must call it together.
template <int W, int NC>
__device__ __forceinline__ void select_into(double (&s)[NC], const int (&mid)[NC], double &ld, int &li,
                                            int &lc, double &tau, int m, int tx, int gbase)
{
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (!(s[j] <= tau)) s[j] = kInf;
    for (;;) {
        double bs = s[0];
        int bi = mid[0], bj = 0;
#pragma unroll
        for (int j = 1; j < NC; ++j)
            if (lex_less(s[j], mid[j], bs, bi)) { bs = s[j]; bi = mid[j]; bj = j; }
        double gs = bs;
        int gi = bi;
#pragma unroll
        for (int off = W / 2; off >= 1; off >>= 1) {
            double os = __shfl_xor(gs, off, W);
            int oi = __shfl_xor(gi, off, W);
            if (lex_less(os, oi, gs, gi)) { gs = os; gi = oi; }
        }
        const bool have = gs < kInf;
        if (!__any(have)) break;
        if (have && bs == gs && bi == gi) {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (j == bj) s[j] = kInf;
        }
        const double d = sqrt(gs);
        const bool lt = (tx < lc) && lex_less(ld, li, d, gi);
        const unsigned long long bal = __ballot(lt);
        const int pos = __popcll((bal >> gbase) & ((W == 64) ? ~0ull : ((1ull << (W & 63)) - 1ull)));
        const double ud = __shfl_up(ld, 1, W);
        const int ui = __shfl_up(li, 1, W);
        const bool ins = have && pos < m;
        if (ins) {
            if (tx == pos) { ld = d; li = gi; }
            else if (tx > pos) { ld = ud; li = ui; }
            lc = lc + 1 < m ? lc + 1 : m;
        }
        const double e = __shfl(ld, m - 1, W);
        if (ins && lc >= m) {
            tau = tau_from(e);
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (!(s[j] <= tau)) s[j] = kInf;
        }
    }
}

}  // namespace
}  // namespace chb
