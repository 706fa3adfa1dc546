// The sorted (distance, index) nearest-member list of a 16-lane group with up to 64 entries, for the wide recruit
// kernels (recruit_wide_kernels.hip): select_into's list (topm_select.h) in four slabs.  Device code only, internal
// linkage.
#pragma once
#include "topm_select.h"

namespace chb {
namespace {

constexpr int kWideSlabs = 4;   // 16 entries each: entry e sits on lane e & 15 of the group, in slab e >> 4

// Offer the (up to) NC candidates held by every lane of a 16-lane group to the group's sorted list.  ld / li: my entry of
// every slab ((+inf, INT_MAX) where the list is shorter), lc the list's length, tau the s-domain admission bound (+inf
// while the list is short), ns = ceil(m / 16) the slabs in use (wave-uniform; the others are never touched).  The order
// and the admission rule are select_into's -- (rooted distance, sample index), a candidate enters where it is less than
// an entry or the list is short -- so the list ends as the m least of everything offered, whatever the order of the
// offers.  Wave-synchronous; all 64 lanes must call it together.
template <int NC>
__device__ __forceinline__ void select_wide_into(double (&s)[NC], const int (&mid)[NC], double (&ld)[kWideSlabs],
                                                 int (&li)[kWideSlabs], int &lc, double &tau, int m, int ns, int tx, int gbase)
{
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (!(s[j] <= tau)) s[j] = kInf;
    const int es = (m - 1) >> 4, el = (m - 1) & 15;   // where entry m - 1 sits
    for (;;) {
        double bs = s[0];
        int bi = mid[0], bj = 0;
#pragma unroll
        for (int j = 1; j < NC; ++j)
            if (lex_less(s[j], mid[j], bs, bi)) { bs = s[j]; bi = mid[j]; bj = j; }
        double gs = bs;
        int gi = bi;
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            double os = __shfl_xor(gs, off, 16);
            int oi = __shfl_xor(gi, off, 16);
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
        // the insert position: the entries that precede the candidate, summed over the slabs
        int pos = 0;
#pragma unroll
        for (int r = 0; r < kWideSlabs; ++r) {
            if (r < ns) {
                const bool lt = (16 * r + tx < lc) && lex_less(ld[r], li[r], d, gi);
                const unsigned long long bal = __ballot(lt);
                pos += __popcll((bal >> gbase) & 0xffffull);
            }
        }
        const bool ins = have && pos < m;
        // the shift, last slab first: an entry's predecessor -- lane 15 of slab r - 1 for lane 0 of slab r -- is read before
        // its own slab moves
#pragma unroll
        for (int r = kWideSlabs - 1; r >= 0; --r) {
            if (r < ns) {
                double ud = __shfl_up(ld[r], 1, 16);
                int ui = __shfl_up(li[r], 1, 16);
                if (r > 0) {
                    const double cd = __shfl(ld[r > 0 ? r - 1 : 0], 15, 16);
                    const int ci = __shfl(li[r > 0 ? r - 1 : 0], 15, 16);
                    if (tx == 0) { ud = cd; ui = ci; }
                }
                const int e = 16 * r + tx;
                if (ins && e == pos) { ld[r] = d; li[r] = gi; }
                else if (ins && e > pos) { ld[r] = ud; li[r] = ui; }
            }
        }
        if (ins) lc = lc + 1 < m ? lc + 1 : m;
        double ev = ld[0];
#pragma unroll
        for (int r = 1; r < kWideSlabs; ++r)
            if (r == es) ev = ld[r];
        const double e = __shfl(ev, el, 16);
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
