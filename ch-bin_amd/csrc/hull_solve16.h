// The 16-lane hull solver shared by the hull kernels (qp_kernels.hip) and the recruit kernel (recruit_kernels.hip):
// the reductions of a 16-lane group, the incrementally maintained inverse (Inv16), the Wolfe active-set iteration
// (active_set_distance2, also the driver of hull_generic_kernel), its 16-lane backend (Group16, solve16) and the
// matrix-core Gram tile of 16 shifted rows (gram_tile16).  Device code only, internal linkage: every translation unit
// that includes this header gets its own copy.
#pragma once
#include "chb_internal.h"

#include <math.h>
#include <utility>

namespace chb {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

// Reductions over a 16-lane group = one DPP row: rotations inside the row are VALU moves (row_ror), no LDS
// crossbar and no lgkmcnt wait.  The rotation butterfly (8, 4, 2, 1) adds the same pairs as the xor butterfly at
// every level (the partial results are periodic), so every lane ends with the bit-identical value.
template <int N>
__device__ __forceinline__ int row_ror_i32(int v)
{
    // (every lane of the row is written: no `old` operand to initialise)
    return __builtin_amdgcn_mov_dpp(v, 0x120 + N, 0xF, 0xF, false);
}
template <int N>
__device__ __forceinline__ double row_ror_f64(double v)
{
    const int lo = row_ror_i32<N>(__double2loint(v)), hi = row_ror_i32<N>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// Exchanges with a fixed pattern inside a 16-lane group, as DPP moves as well (a double is two of them; the bits travel
// unchanged, NaN payloads included).  row_xor<K>(v): the value of lane l16 ^ K, K = 8 (a rotation by half a row), 2 and 1
// (quad permutations), 4 (lanes 0-3 and 8-11 take theirs from four lanes up, the others from four lanes down: two moves
// into one register, each writing its own banks).  row_bcast<V>(v): the value of lane V of the row.  Like a shuffle they
// stand outside any condition that splits a row: a disabled lane delivers nothing, and here its reader keeps stale bits.
template <int K>
__device__ __forceinline__ int row_xor_i32(int v)
{
    static_assert(K == 1 || K == 2 || K == 4 || K == 8, "one bit of the lane number inside a row");
    if constexpr (K == 8) return __builtin_amdgcn_mov_dpp(v, 0x128, 0xF, 0xF, false);       // row_ror:8
    else if constexpr (K == 2) return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false);   // quad_perm:[2,3,0,1]
    else if constexpr (K == 1) return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false);   // quad_perm:[1,0,3,2]
    else {
        const int up = __builtin_amdgcn_mov_dpp(v, 0x104, 0xF, 0x5, false);                 // row_shl:4 bank_mask:0x5
        return __builtin_amdgcn_update_dpp(up, v, 0x114, 0xF, 0xA, false);                  // row_shr:4 bank_mask:0xa
    }
}
template <int V>
__device__ __forceinline__ int row_bcast_i32(int v)
{
    static_assert(V >= 0 && V < 16, "a lane of the row");
    return __builtin_amdgcn_mov_dpp(v, 0x150 + V, 0xF, 0xF, false);                         // row_newbcast:V
}
template <int K>
__device__ __forceinline__ double row_xor_f64(double v)
{
    const int lo = row_xor_i32<K>(__double2loint(v)), hi = row_xor_i32<K>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
template <int V>
__device__ __forceinline__ double row_bcast_f64(double v)
{
    const int lo = row_bcast_i32<V>(__double2loint(v)), hi = row_bcast_i32<V>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// f(integral constant 0), ..., f(integral constant N - 1): a loop whose counter can be a DPP control
template <int V>
struct RowLane {
    static constexpr int value = V;
};
template <class F, int... Vs>
__device__ __forceinline__ void for_row_lanes_impl(F &&f, std::integer_sequence<int, Vs...>)
{
    (f(RowLane<Vs>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void for_row_lanes(F &&f)
{
    for_row_lanes_impl(f, std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ double group_sum16(double v)
{
    v += row_ror_f64<8>(v);
    v += row_ror_f64<4>(v);
    v += row_ror_f64<2>(v);
    v += row_ror_f64<1>(v);
    return v;
}
__device__ __forceinline__ double group_max16(double v)
{
    v = fmax(v, row_ror_f64<8>(v));
    v = fmax(v, row_ror_f64<4>(v));
    v = fmax(v, row_ror_f64<2>(v));
    v = fmax(v, row_ror_f64<1>(v));
    return v;
}
__device__ __forceinline__ double group_min16(double v)
{
    v = fmin(v, row_ror_f64<8>(v));
    v = fmin(v, row_ror_f64<4>(v));
    v = fmin(v, row_ror_f64<2>(v));
    v = fmin(v, row_ror_f64<1>(v));
    return v;
}
// smallest key, ties to the lowest lane; key = +inf (or NaN) everywhere gives idx = -1
__device__ __forceinline__ void group_argmin16(double key, int lane, double &kmin, int &idx)
{
    kmin = group_min16(key);
    const unsigned hit = (unsigned)(__ballot(key == kmin && key < kInf) >> (lane & 48)) & 0xFFFFu;
    idx = hit ? __ffs(hit) - 1 : -1;
}

// The affine sub-problem (Q_SS + s 11^T) b = 1, beta = b / sum(b) is solved through the explicit
// inverse H of the lifted support Gram, kept up to date as vertices enter and leave (lane i holds
// row i of H, zeros outside the support).  Entering / leaving is a bordering / Schur update whose
// broadcasts are independent of each other -- a few LDS rounds deep, where an elimination from
// scratch is a 16-step dependent chain.  The pivot of the update is the Schur complement delta, the
// same quantity whose collapse marks an affinely dependent support in solve_affine<M>.
// developer variants (tools/m15_probe.py; tools/build_variant.sh <name> "-DCHB_DEV_QP16_STAT" or "-DCHB_DEV_CLK"):
// CHB_DEV_QP16_STAT = iteration statistics of the 16-lane solver (Group16::stat; its atomics distort timings), CHB_DEV_CLK = cycle
// stamps of the fused 16-lane kernel's phases only
#if defined(CHB_DEV_QP16_STAT) || defined(CHB_DEV_CLK)
__device__ unsigned long long g_qp16_stats[16];
#endif

// 1 / x for normal, well-scaled x (the 16-lane solver works on a Gram normalised to O(1)): hardware estimate + two
// Newton steps, within an ulp or two of the correctly rounded quotient
__device__ __forceinline__ double fast_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

struct Inv16 {
    double H[16];
};

// Every lane of a 16-lane group publishes one value; afterwards out[j] is lane j's.  Through a 16-double LDS row
// of the group (one ds_write_b64 + eight ds_read_b128, broadcast reads) instead of sixteen shuffles of a double
// (32 ds_bpermute_b32): the LDS crossbar is what the 16-lane solver runs on.
__device__ __forceinline__ void group_allgather16(double *sv, int l16, double v, double (&out)[16])
{
    sv[l16] = v;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        const double2 t = *reinterpret_cast<const double2 *>(sv + j);
        out[j] = t.x; out[j + 1] = t.y;
    }
    __builtin_amdgcn_wave_barrier();
}

#ifndef CHB_QP16_OCC
#define CHB_QP16_OCC 3   // wavefronts per SIMD the 16-lane solver is compiled for (168 VGPRs)
#endif
static_assert(kFusedMaxDp <= 16 * 18, "the query row is staged in a 16 x kQ16Ld tile");
constexpr int kQ16Ld = 18;   // row stride of the 16 x 16 Gram tile in LDS (16-byte aligned rows)

// vertex v enters: false (and no change) when it is affinely dependent on the support.
// Qt = the group's LIFTED Gram tile in LDS (Q + s, row stride kQ16Ld), sv = its 16-double exchange row.
// Rows and columns of H outside the support are zero, so the products below need no support mask.
// small (out): the accepted pivot was below kSmallPivot x the vertex's own lifted norm -- the support is ill-conditioned
// (cond ~ 1 / that ratio), see active_set_distance2's rebuild.  reject: the pivot below which the vertex counts as dependent.
constexpr double kSmallPivot = 1e-4;
__device__ __forceinline__ bool inv16_insert(Inv16 &I, const double *Qt, double *sv, unsigned &S, int v, int l16, bool &small,
                                             double reject = 1e-13)
{
    // a = lifted row v (a broadcast read); u = H a
    double u = 0.0;
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        const double2 t = *reinterpret_cast<const double2 *>(Qt + v * kQ16Ld + j);
        u = fma(I.H[j], t.x, u);
        u = fma(I.H[j + 1], t.y, u);
    }
    const double a_own = Qt[v * kQ16Ld + l16], avv = Qt[v * kQ16Ld + v];
    double delta = avv - group_sum16(a_own * u);
    double ug[16];
    if (!(delta > 1e-6 * avv)) {
#ifdef CHB_DEV_QP16_STAT
        if (l16 == 0) atomicAdd(&g_qp16_stats[4], 1ull);
#endif
        // A small pivot is decided after one step of iterative refinement against the ORIGINAL rows
        // of Q: the stored inverse carries an error of eps * cond, which must not leak into the
        // test below (a dependent vertex has to come out at delta ~ eps * avv, as the Schur
        // complement of a factorisation does).
        const bool in = (S >> l16) & 1u;
        group_allgather16(sv, l16, u, ug);
        double r = a_own;
#pragma unroll
        for (int j = 0; j < 16; ++j) r = fma(-Qt[l16 * kQ16Ld + j], ug[j], r);   // u is zero outside the support
        r = in ? r : 0.0;
        group_allgather16(sv, l16, r, ug);
        double du = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) du = fma(I.H[j], ug[j], du);
        u += du;
        delta = avv - group_sum16(a_own * u);
    }
    small = !(delta > kSmallPivot * avv);
    if (!(delta > reject * avv)) return false;
    const double inv = fast_rcp(delta);
    // bordering: H' = H + w w^T / delta with w = (u on the support, -1 at v, 0 elsewhere)
    const double w = l16 == v ? -1.0 : u;
    group_allgather16(sv, l16, w, ug);
    const double f = w * inv;
#pragma unroll
    for (int j = 0; j < 16; ++j) I.H[j] = fma(f, ug[j], I.H[j]);
    S |= 1u << v;
    return true;
}

// vertex r (in S) leaves
__device__ __forceinline__ void inv16_remove(Inv16 &I, double *sv, unsigned &S, int r, int l16)
{
    // row r of H = column r (H is symmetric): every lane contributes its own entry H[l16][r]
    double hrr = 0.0, own = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) own = (j == r) ? I.H[j] : own;
    double hr[16];
    group_allgather16(sv, l16, own, hr);
#pragma unroll
    for (int j = 0; j < 16; ++j) hrr = (j == r) ? hr[j] : hrr;
    const double f = own / hrr;
#pragma unroll
    for (int j = 0; j < 16; ++j) I.H[j] = (l16 == r || j == r) ? 0.0 : fma(-f, hr[j], I.H[j]);
    S &= ~(1u << r);
}

// beta_l16 of the affine minimiser on the current support (0 outside); false if the weights do not sum > 0
__device__ __forceinline__ bool inv16_beta(const Inv16 &I, double &beta)
{
    double b = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) b += I.H[j];
    const double sum = group_sum16(b);
    beta = b * fast_rcp(sum);
    return sum > 0.0;
}

// ---------------------------------------------------------------------------------------------
// The Wolfe active-set iteration of the 16-lane kernels (solve16) and of hull_generic_kernel, written once: the hull
// (metric 0) or affine-hull distance SQUARED of one problem with n > 0 vertices whose largest squared distance is
// `scale`.  Every lane owns one vertex (`me`; `mine`: it exists; `diag`: its squared distance) and returns its weight in
// `alpha`.  Where the Gram and the inverse H of the lifted support Gram live, and how the lanes of a problem talk to each
// other, is the backend G (Group16 below, Wave64 further down), handed over reset (H = 0, support S = 0).  value(alpha, gi)
// publishes the weights: gi = my entry of the gradient Q alpha, the result is alpha^T Q alpha.  cap() bounds the minor
// cycle and rebuild's scan of S: 16 or n, the same scan, since S never has a bit at or above n.
// `dirty` / rebuild: the explicit inverse is only as good as the supports it has been through.  A vertex that enters
// with a pivot of 1e-7 of its norm (four nearly coplanar points in three dimensions: a near-duplicate contig among the
// neighbours) leaves H with entries of 1e7 and a relative error of eps * cond; the Schur update that takes a vertex out
// again cancels all but 1 / cond of that magnitude, so H -- and with it every later weight vector -- is off by
// eps * cond^2 (6e-2 in the case tools/solve16_cases.py found: a distance 1.2 % too large, a corral of eight
// "independent" vertices in three dimensions).  Hence: once a small pivot has been accepted (`dirty`), every removal
// REBUILDS H from the Gram's rows for the vertices that remain -- |S| borderings, error eps * cond of the CURRENT
// support, no history.  Well-conditioned problems (every benchmark configuration) never take that path.
template <class G>
__device__ __forceinline__ double active_set_distance2(G &g, int n, int metric, double scale, double &alpha)
{
    using Mask = typename G::Mask;
    const Mask one = 1;
    double val, gi;
    bool sm;
    if (!(scale > 0.0)) {   // every vertex coincides with the query (or NaN input)
        alpha = g.me == 0 ? 1.0 : 0.0;
        val = scale == 0.0 ? 0.0 : scale;
    } else if (metric == 0) {
        double best;
        int i0;
        g.argmin(g.mine ? g.diag : kInf, best, i0);
        Mask banned = 0;
        (void)g.insert(i0, sm);   // a single vertex is always independent
        alpha = g.me == i0 ? 1.0 : 0.0;
        bool dirty = false;
        // H for the vertices in S from scratch; a vertex whose pivot comes out non-positive now (it was accepted on a
        // corrupted H) is dropped and its weight shared out.  false: nothing usable was left, the solver has been set back
        // to the nearest vertex alone (the caller leaves its minor cycle).
        auto rebuild = [&]() __attribute__((always_inline)) -> bool {
            const Mask S2 = g.S;
            Mask lost = 0;
            g.reset(); dirty = false;
            for (int v = 0; v < g.cap(); ++v) {
                if (!((S2 >> v) & one)) continue;
                bool smv;
                if (g.insert(v, smv, 0.0)) dirty = dirty || smv;
                else lost |= one << v;
            }
            if (lost == 0) return true;
            alpha = ((lost >> g.me) & one) ? 0.0 : alpha;
            const double s1 = g.sum(alpha);
            if (g.S != 0 && s1 > 0.0) { alpha = g.renormalise(alpha, s1); return true; }
            g.reset();
            (void)g.insert(i0, sm);
            alpha = g.me == i0 ? 1.0 : 0.0;
            return false;
        };
        const double tol = 1.4210854715202004e-14 * scale;  // 64 eps * scale
        g.stat(0, 1);
        for (int it = 0; it < G::kMajorCap; ++it) {
            g.stat(1, 1);
            val = g.value(alpha, gi);
            double gmin;
            int jb;
            g.argmin((g.mine && !(((g.S | banned) >> g.me) & one)) ? gi : kInf, gmin, jb);
            if (jb < 0 || !(gmin < val - tol)) break;
            if (!g.insert(jb, sm)) {
                banned |= one << jb;
                continue;
            }
            dirty = dirty || sm;
            for (int mi = 0; mi <= g.cap(); ++mi) {
                double beta;
                if (!g.beta(beta)) {   // (degenerate weights: give the vertex up)
                    if ((g.S >> jb) & one) {
                        g.remove(jb);
                        if (dirty) (void)rebuild();
                    }
                    banned |= one << jb;
                    break;
                }
                const bool in = (g.S >> g.me) & one;
                const bool bad = in && !(beta > 0.0);
                if (!g.any(bad)) {
                    alpha = in ? beta : 0.0;
                    break;
                }
                g.stat(2, 1);
                const double den = alpha - beta;
                double theta;
                int kr;
                g.argmin(bad ? (den > 0.0 ? alpha / den : 0.0) : kInf, theta, kr);
                const double vnew = alpha + theta * (beta - alpha);
                alpha = (in && g.me != kr) ? vnew : 0.0;
                g.remove(kr);
                if (kr == jb) banned |= one << jb;
                if (dirty && !rebuild()) break;
            }
        }
        g.stat(3, __popcll(g.S));
        val = g.value(alpha, gi);
    } else {
        // distance to the AFFINE hull: greedy maximal affinely independent subset (affine_min_norm)
        for (int k = 0; k < n; ++k) (void)g.insert(k, sm);
        double beta = 0.0;
        const bool okb = g.S != 0 && g.beta(beta);
        alpha = (okb && ((g.S >> g.me) & one)) ? beta : 0.0;
        if (!okb) alpha = g.me == 0 ? 1.0 : 0.0;
        val = g.value(alpha, gi);
    }
    return val;
}

// The 16-lane backend: lane l16 of the group owns vertex l16, i.e. row l16 of the plain Gram (Qr) and of H (I), both in
// registers.  Qt = the group's LIFTED Gram tile in LDS (what inv16_insert reads), sv = its exchange row.
struct Group16 {
    using Mask = unsigned;
    static constexpr int kMajorCap = 3 * 16 + 8;
    Inv16 I;
    const double *Qt;
    double *sv;
    double Qr[16], diag;
    int me, lane;   // (me = l16)
    bool mine;
    Mask S;
    __device__ __forceinline__ int cap() const { return 16; }
    __device__ __forceinline__ void reset()
    {
        S = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) I.H[j] = 0.0;
    }
    __device__ __forceinline__ bool insert(int v, bool &small, double reject = 1e-13) { return inv16_insert(I, Qt, sv, S, v, me, small, reject); }
    __device__ __forceinline__ void remove(int r) { inv16_remove(I, sv, S, r, me); }
    __device__ __forceinline__ bool beta(double &b) const { return inv16_beta(I, b); }
    __device__ __forceinline__ double value(double alpha, double &gi)
    {
        double ag[16];   // gathered weights
        group_allgather16(sv, me, alpha, ag);
        gi = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) gi = fma(Qr[j], ag[j], gi);
        return group_sum16(alpha * gi);
    }
    __device__ __forceinline__ double sum(double v) const { return group_sum16(v); }
    __device__ __forceinline__ void argmin(double key, double &kmin, int &idx) const { group_argmin16(key, lane, kmin, idx); }
    __device__ __forceinline__ bool any(bool p) const { return ((__ballot(p) >> (lane & 48)) & 0xFFFFull) != 0ull; }
    __device__ __forceinline__ double renormalise(double alpha, double s1) const { return alpha * fast_rcp(s1); }   // (s1 is O(1))
    __device__ __forceinline__ void stat(int i, unsigned long long v) const
    {
#ifdef CHB_DEV_QP16_STAT
        if (me == 0) atomicAdd(&g_qp16_stats[i], v);
#endif
    }
};

// phase 2 of the 16-lane kernels: the hull (metric 0) or affine-hull distance SQUARED of the group's problem, by
// active_set_distance2 on a Group16.
// Qt = the group's plain shifted Gram tile in LDS (rows / columns >= n finite, e.g. zero), sv = its exchange row;
// lane l16 owns vertex l16 (n <= 16 vertices, n > 0) and returns its weight in `alpha`.
__device__ __forceinline__ double solve16(double *Qt, double *sv, int n, int metric, int lane, double &alpha)
{
    const int l16 = lane & 15;
    Group16 g;
    g.Qt = Qt; g.sv = sv; g.me = l16; g.lane = lane; g.mine = l16 < n;
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        const double2 t = *reinterpret_cast<const double2 *>(Qt + l16 * kQ16Ld + j);
        g.Qr[j] = t.x; g.Qr[j + 1] = t.y;
    }
    alpha = 0.0;
    const double diag = Qt[l16 * kQ16Ld + l16];
    const double scale0 = group_max16(g.mine ? diag : 0.0);
    // The problem is normalised by a power of two (exact): the largest squared distance becomes `scale` in
    // [0.5, 1), so thresholds and reciprocals see O(1) numbers whatever the units of the data.
    int ex = 0;
    if (scale0 > 0.0 && scale0 < kInf) (void)frexp(scale0, &ex);
    ex = ex < -1000 ? -1000 : (ex > 1000 ? 1000 : ex);
    const double dn = ldexp(1.0, -ex);
    const double scale = scale0 * dn;
    g.diag = diag * dn;
#pragma unroll
    for (int j = 0; j < 16; ++j) g.Qr[j] *= dn;
    // the tile in LDS becomes the lifted Gram Q + scale (what inv16_insert reads); Qr keeps the plain rows
#pragma unroll
    for (int j = 0; j < 16; j += 2)
        *reinterpret_cast<double2 *>(Qt + l16 * kQ16Ld + j) = double2{g.Qr[j] + scale, g.Qr[j + 1] + scale};
    __builtin_amdgcn_wave_barrier();
    g.reset();
    return ldexp(active_set_distance2(g, n, metric, scale, alpha), ex);   // back to the data's units (exact)
}

// One k-sweep of the matrix core over the 16 rows `idv` (lane (row, kq): row = lane & 15 supplies the row,
// kq = lane >> 4 its features 4 kq .. 4 kq + 3 of every 16) shifted by the query row q: the 16 x 16 Gram tile,
// lane (row, kq) ends with D[kq + 4 r][row] in acc[r].  TWO: a second row set idw and the tiles
// <rows, rows> (acc), <rows, rows2> (acx: acx[r] = <row kq + 4 r of the first set, row `row` of the second>),
// <rows2, rows2> (acw) from ONE read of every row.
template <bool TWO>
struct RowChunk16 {   // 32 features of the lane's rows: 2 x 4 doubles each
    double2 v[4], x[4], u[TWO ? 4 : 1];
};
// FULL: the whole chunk lies inside the row (no range checks; only a row's last chunk can be partial)
template <bool TWO, bool FULL>
__device__ __forceinline__ void load_chunk16(RowChunk16<TWO> &c, const double *vptr, const double *wptr,
                                             const double *qptr, int k0, int kq, int Dp)
{
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int kk = k0 + 16 * t + 4 * kq;
        const bool in = FULL || kk < Dp;   // Dp % 8 == 0 and kk % 4 == 0: all 4 in range
        c.v[2 * t] = in ? *reinterpret_cast<const double2 *>(vptr + k0 + 16 * t) : double2{0.0, 0.0};
        c.v[2 * t + 1] = in ? *reinterpret_cast<const double2 *>(vptr + k0 + 16 * t + 2) : double2{0.0, 0.0};
        c.x[2 * t] = in ? *reinterpret_cast<const double2 *>(qptr + k0 + 16 * t) : double2{0.0, 0.0};
        c.x[2 * t + 1] = in ? *reinterpret_cast<const double2 *>(qptr + k0 + 16 * t + 2) : double2{0.0, 0.0};
        if (TWO) {
            c.u[2 * t] = in ? *reinterpret_cast<const double2 *>(wptr + k0 + 16 * t) : double2{0.0, 0.0};
            c.u[2 * t + 1] = in ? *reinterpret_cast<const double2 *>(wptr + k0 + 16 * t + 2) : double2{0.0, 0.0};
        }
    }
}
template <bool TWO>
__device__ __forceinline__ void mfma_chunk16(const RowChunk16<TWO> &cur, f64x4 &acc, f64x4 &acx, f64x4 &acw)
{
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double y0 = cur.v[t].x - cur.x[t].x;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(y0, y0, acc, 0, 0, 0);
        if (TWO) {
            const double z0 = cur.u[t].x - cur.x[t].x;
            acx = __builtin_amdgcn_mfma_f64_16x16x4f64(y0, z0, acx, 0, 0, 0);
            acw = __builtin_amdgcn_mfma_f64_16x16x4f64(z0, z0, acw, 0, 0, 0);
        }
        const double y1 = cur.v[t].y - cur.x[t].y;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(y1, y1, acc, 0, 0, 0);
        if (TWO) {
            const double z1 = cur.u[t].y - cur.x[t].y;
            acx = __builtin_amdgcn_mfma_f64_16x16x4f64(y1, z1, acx, 0, 0, 0);
            acw = __builtin_amdgcn_mfma_f64_16x16x4f64(z1, z1, acw, 0, 0, 0);
        }
    }
}
// (pointer form: vptr / wptr / qptr = the lane's rows and the query row, each advanced by 4 kq -- the rows need not share a
//  matrix: the recruit kernel's query rows are not samples.  gram_tile16 below keeps its own copy of the loop: routed
//  through this function the hull kernels' address arithmetic compiles to other instructions, and the counter tables under
//  profiles/ stand for the instructions they were measured on)
template <bool TWO>
__device__ __forceinline__ void gram_tile16_rows(const double *vptr, const double *wptr, const double *qptr, int Dk, int kq,
                                                 f64x4 &acc, f64x4 &acx, f64x4 &acw)
{
    const int Dfull = Dk & ~31;
    int k0 = 0;
    for (; k0 < Dfull; k0 += 32) {
        RowChunk16<TWO> cur;
        load_chunk16<TWO, true>(cur, vptr, wptr, qptr, k0, kq, Dk);
        mfma_chunk16<TWO>(cur, acc, acx, acw);
    }
    if (k0 < Dk) {
        RowChunk16<TWO> cur;
        load_chunk16<TWO, false>(cur, vptr, wptr, qptr, k0, kq, Dk);
        mfma_chunk16<TWO>(cur, acc, acx, acw);
    }
}
template <bool TWO>
__device__ __forceinline__ void gram_tile16(const double *X, int Dp, int Dk, int q, int idv, int idw, int kq, f64x4 &acc,
                                            f64x4 &acx, f64x4 &acw)
{
    const double *vptr = X + (size_t)(idv >= 0 ? idv : q) * Dp + 4 * kq;   // a missing vertex reads the query row: y = 0
    const double *wptr = X + (size_t)(idw >= 0 ? idw : q) * Dp + 4 * kq;
    const double *qptr = X + (size_t)q * Dp + 4 * kq;
    const int Dfull = Dk & ~31;
    int k0 = 0;
    for (; k0 < Dfull; k0 += 32) {
        RowChunk16<TWO> cur;
        load_chunk16<TWO, true>(cur, vptr, wptr, qptr, k0, kq, Dk);
        mfma_chunk16<TWO>(cur, acc, acx, acw);
    }
    if (k0 < Dk) {
        RowChunk16<TWO> cur;
        load_chunk16<TWO, false>(cur, vptr, wptr, qptr, k0, kq, Dk);
        mfma_chunk16<TWO>(cur, acc, acx, acw);
    }
}

}  // namespace
}  // namespace chb
