// The one-wavefront-per-problem backend of active_set_distance2 (hull_solve16.h), shared by hull_generic_kernel
// (qp_kernels.hip) and hull_wide_kernel (recruit_wide_kernels.hip): up to NV <= 64 vertices per problem, lane i owns
// vertex i: row i of the shifted Gram Q and of the inverse H of the lifted support Gram (both in LDS, [NV][NV + 1]
// doubles) and its weight alpha_i.  The same bordering / Schur updates as Inv16, with loops over the vertex count and LDS
// rows where that has 16-entry register arrays and DPP reductions.  Device code only, internal linkage.
//
// NV is the LDS capacity: 64 (66 KiB, dynamic: hull_generic_kernel, hull_wide_kernel<64>) or 32 (17.5 KiB, static:
// hull_wide_kernel<32>).  All 64 lanes of the wavefront take part in every reduction whatever NV is; a lane at or past
// the problem's vertex count n <= NV owns nothing, reads nothing of Q or H and writes only its exchange slots va / vu.
#pragma once
#include "chb_internal.h"
#include "hull_solve16.h"

#include <math.h>

namespace chb {
namespace {

template <int NV>
struct GenLdsT {
    static_assert(NV == 32 || NV == 64, "one wavefront, at most one vertex per lane");
    double Q[NV][NV + 1];
    double H[NV][NV + 1];
    double va[64], vu[64];
};

__device__ __forceinline__ double wave_sum64(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// smallest key, ties to the lowest lane; all keys +inf gives idx = -1
__device__ __forceinline__ void wave_argmin64(double key, int lane, double &kmin, int &idx)
{
    kmin = key;
    idx = key < kInf ? lane : -1;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ok = __shfl_xor(kmin, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (oi >= 0 && (idx < 0 || ok < kmin || (ok == kmin && oi < idx))) { kmin = ok; idx = oi; }
    }
}
__device__ __forceinline__ void gen_sync()
{
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
}

// vertex v enters the support: false (and no change) when it is affinely dependent on it
// (small / reject: as inv16_insert)
template <int NV>
__device__ __forceinline__ bool gen_insert(GenLdsT<NV> &L, int n, double s, unsigned long long &S, int v, int lane, bool &small,
                                           double reject = 1e-13)
{
    const bool in = (S >> lane) & 1ull;
    const double a_own = (lane < n) ? L.Q[v][lane] + s : 0.0;
    const double avv = L.Q[v][v] + s;
    L.va[lane] = in ? a_own : 0.0;
    gen_sync();
    double u = 0.0;
    if (in)
        for (int j = 0; j < n; ++j) u = fma(L.H[lane][j], L.va[j], u);   // (H is zero outside the support)
    double delta = avv - wave_sum64(in ? a_own * u : 0.0);
    if (!(delta > 1e-6 * avv)) {
        // small pivot: one step of iterative refinement against the original rows of Q (see inv16_insert)
        L.vu[lane] = in ? u : 0.0;
        gen_sync();
        double r = a_own;
        if (in)
            for (int j = 0; j < n; ++j)
                if ((S >> j) & 1ull) r = fma(-(L.Q[lane][j] + s), L.vu[j], r);
        gen_sync();
        L.vu[lane] = in ? r : 0.0;
        gen_sync();
        double du = 0.0;
        if (in)
            for (int j = 0; j < n; ++j) du = fma(L.H[lane][j], L.vu[j], du);
        u += du;
        delta = avv - wave_sum64(in ? a_own * u : 0.0);
        gen_sync();
    }
    small = !(delta > kSmallPivot * avv);
    if (!(delta > reject * avv)) return false;
    const double inv = 1.0 / delta;
    L.vu[lane] = in ? u : 0.0;
    gen_sync();
    if (in) {
        const double ui = u * inv;
        for (int j = 0; j < n; ++j)
            if ((S >> j) & 1ull) L.H[lane][j] = fma(ui, L.vu[j], L.H[lane][j]);
        L.H[lane][v] = -ui;
    }
    if (lane == v) {
        for (int j = 0; j < n; ++j) L.H[v][j] = ((S >> j) & 1ull) ? -L.vu[j] * inv : 0.0;
        L.H[v][v] = inv;
    }
    S |= 1ull << v;
    gen_sync();
    return true;
}

// vertex r (in the support) leaves
template <int NV>
__device__ __forceinline__ void gen_remove(GenLdsT<NV> &L, int n, unsigned long long &S, int r, int lane)
{
    const bool in = (S >> lane) & 1ull;
    const double hrr = L.H[r][r];
    if (in && lane != r) {
        const double f = L.H[lane][r] / hrr;
        for (int j = 0; j < n; ++j)
            if (j != r) L.H[lane][j] = fma(-f, L.H[r][j], L.H[lane][j]);
        L.H[lane][r] = 0.0;
    }
    gen_sync();
    if (lane == r)
        for (int j = 0; j < n; ++j) L.H[r][j] = 0.0;
    S &= ~(1ull << r);
    gen_sync();
}

// weight of my vertex in the affine minimiser on the support; false if the weights do not sum > 0
template <int NV>
__device__ __forceinline__ bool gen_beta(GenLdsT<NV> &L, int n, unsigned long long S, int lane, double &beta)
{
    double b = 0.0;
    if ((S >> lane) & 1ull)
        for (int j = 0; j < n; ++j) b += L.H[lane][j];
    const double sum = wave_sum64(b);
    beta = b / sum;
    return sum > 0.0;
}

// The wavefront backend of active_set_distance2: lane i owns vertex i, i.e. row i of L.Q and of L.H.  It works on the
// un-normalised Gram (the lift is s = scale).  gen_sync() stands between a write of L.va and its reads, and after the
// reads before the next write (after the final evaluation that second one has nothing left to order).
template <int NV>
struct Wave64T {
    using Mask = unsigned long long;
    static constexpr int kMajorCap = 3 * NV + 8;
    GenLdsT<NV> &L;
    int n;
    double scale, diag;
    int me;   // (= lane)
    bool mine;
    Mask S;
    __device__ __forceinline__ int cap() const { return n; }
    __device__ __forceinline__ void reset()
    {
        S = 0ull;
        if (NV == 64 || me < NV)   // (a lane past the capacity has no row)
            for (int j = 0; j < NV; ++j) L.H[me][j] = 0.0;
        gen_sync();
    }
    __device__ __forceinline__ bool insert(int v, bool &small, double reject = 1e-13) { return gen_insert(L, n, scale, S, v, me, small, reject); }
    __device__ __forceinline__ void remove(int r) { gen_remove(L, n, S, r, me); }
    __device__ __forceinline__ bool beta(double &b) const { return gen_beta(L, n, S, me, b); }
    __device__ __forceinline__ double value(double alpha, double &gi)
    {
        L.va[me] = alpha;
        gen_sync();
        gi = 0.0;
        if (mine)
            for (int j = 0; j < n; ++j) gi = fma(L.Q[me][j], L.va[j], gi);
        const double val = wave_sum64(alpha * gi);
        gen_sync();
        return val;
    }
    __device__ __forceinline__ double sum(double v) const { return wave_sum64(v); }
    __device__ __forceinline__ void argmin(double key, double &kmin, int &idx) const { wave_argmin64(key, me, kmin, idx); }
    __device__ __forceinline__ bool any(bool p) const { return __ballot(p) != 0ull; }
    __device__ __forceinline__ double renormalise(double alpha, double s1) const { return alpha / s1; }
    __device__ __forceinline__ void stat(int, unsigned long long) const { }
};

}  // namespace
}  // namespace chb
