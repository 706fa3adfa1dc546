// Batched point-to-convex-hull distance for gfx950.
//
// Replaces hull_distance.py:7-35 (convex_hull_distance: P = 2 X X^T, q = -2 X x, sum(alpha) = 1,
// alpha >= 0, ||alpha X - x||) together with solve_qp.py:18-51 / :96-132 (nearest-PD repair,
// quadprog's Goldfarb-Idnani solve, cvxopt fallback) for every (contig, bin) pair of a batch.
//
// The QP min ||sum_a alpha_a x_a - x||^2 over the simplex is the minimum-norm point of
// conv{y_a = x_a - x}.  It is solved in Gram space:
//   phase 1: the shifted Gram Q_ab = <y_a, y_b>.  m <= 8: 16 lanes per problem, fp64 vector FMAs over
//     interleaved feature pairs, one reduce-scatter (hull_qp_kernel).  m > 8: one
//     v_mfma_f64_16x16x4_f64 tile per problem (hull_qp16_kernel).
//   phase 2: Wolfe's minimum-norm-point active-set method.  m <= 8: one problem per lane on the m x m
//     Gram held in registers (fixed-size, mask-driven, fully unrolled so nothing is dynamically
//     indexed); m > 8: one problem per 16 lanes.  Affine sub-problems by LDL^T (or an updated inverse)
//     of the lifted Gram Q_SS + s*11^T, which is positive definite exactly when the support is
//     affinely independent -- so duplicate / collinear vertices (singular 2XX^T, the case the
//     reference repairs with nearest-PD jitter and a cvxopt fallback) need no special handling.
//   distance = sqrt(alpha^T Q alpha).
// The result is the same projection distance the reference's QP defines (unique even when alpha
// is not); agreement with the CPU oracle's Goldfarb-Idnani restatement is ~1e-13 relative.
#include "chb_internal.h"
#include "hull_solve16.h"
#include "hull_solve64.h"
#include <cstdlib>
#include <type_traits>
#include <vector>

#include <math.h>

#include <algorithm>

#ifndef CHB_QP_UNROLL
#define CHB_QP_UNROLL 1
#endif

namespace chb {
namespace {


template <int M>
struct Sym {
    static constexpr int NP = M * (M + 1) / 2;
    __device__ static constexpr int at(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }
};

// Affine minimiser on support S: solve (Q_SS + s 11^T) b = 1, beta = b / sum(b).
// Rows/columns outside S are replaced by identity.  Returns false when a pivot collapses
// (support numerically affinely dependent).
template <int M>
__device__ __forceinline__ bool solve_affine(const double (&Q)[Sym<M>::NP], double s, unsigned S,
                                             double (&beta)[M])
{
    double L[M * (M - 1) / 2 + 1];
    double dg[M];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const bool ink = (S >> k) & 1u;
        const double akk = ink ? Q[Sym<M>::at(k, k)] + s : 1.0;
        double dk = akk;
#pragma unroll
        for (int j = 0; j < k; ++j) dk -= L[k * (k - 1) / 2 + j] * L[k * (k - 1) / 2 + j] * dg[j];
        if (ink && !(dk > 1e-13 * akk)) ok = false;
        dg[k] = dk;
        const double inv = 1.0 / dk;
#pragma unroll
        for (int i = k + 1; i < M; ++i) {
            const bool ini = (S >> i) & 1u;
            double v = (ink && ini) ? Q[Sym<M>::at(i, k)] + s : 0.0;
#pragma unroll
            for (int j = 0; j < k; ++j) v -= L[i * (i - 1) / 2 + j] * L[k * (k - 1) / 2 + j] * dg[j];
            L[i * (i - 1) / 2 + k] = v * inv;
        }
    }
    if (!ok) return false;
    double z[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        double v = ((S >> i) & 1u) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < i; ++j) v -= L[i * (i - 1) / 2 + j] * z[j];
        z[i] = v;
    }
#pragma unroll
    for (int i = 0; i < M; ++i) z[i] = z[i] / dg[i];
    double sum = 0.0;
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
        double v = z[i];
#pragma unroll
        for (int j = i + 1; j < M; ++j) v -= L[j * (j - 1) / 2 + i] * beta[j];
        beta[i] = v;
        sum += v;
    }
    const double inv = 1.0 / sum;
#pragma unroll
    for (int i = 0; i < M; ++i) beta[i] *= inv;
    return sum > 0.0;
}

// Minimum of alpha^T Q alpha over the simplex on the first m (<= M) vertices.  Returns the value
// (squared hull distance) and the weights.
template <int M>
__device__ __forceinline__ double min_norm_point(const double (&Q)[Sym<M>::NP], int m,
                                                 double (&alpha)[M])
{
    double scale = 0.0;
    int i0 = 0;
    double best = kInf;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        alpha[i] = 0.0;
        if (i < m) {
            const double qii = Q[Sym<M>::at(i, i)];
            scale = fmax(scale, qii);
            if (qii < best) { best = qii; i0 = i; }
        }
    }
    if (!(scale > 0.0)) {  // every vertex coincides with the query (or NaN input)
#pragma unroll
        for (int i = 0; i < M; ++i) alpha[i] = (i == 0) ? 1.0 : 0.0;
        return scale == 0.0 ? 0.0 : scale;
    }
    // Full-set start: the first cycle has no entering vertex (jb = -1) -- it solves on all m vertices from the uniform
    // weights.  All beta > 0 (a query inside its neighbours' cloud: the rule, see DESIGN.md section 5, "Solver start") ends
    // the method after this one solve, where growing the support from the nearest vertex takes one solve per vertex of
    // it; some beta <= 0 runs Wolfe's minor cycles down from the full set; a collapsed pivot (an affinely dependent set:
    // duplicates, m > D + 1) starts again from the nearest vertex alone, which adds one vertex per major cycle and bans
    // the dependent ones.
    unsigned S = (1u << m) - 1u, banned = 0u;
    const double uni = 1.0 / (double)m;
#pragma unroll
    for (int i = 0; i < M; ++i) alpha[i] = i < m ? uni : 0.0;
    const double tol = 1.4210854715202004e-14 * scale;  // 64 eps * scale

    for (int it = -1; it < 3 * M + 8; ++it) {
        int jb = -1;
        if (it >= 0) {
            double g[M];
            double val = 0.0;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                double gi = 0.0;
#pragma unroll
                for (int j = 0; j < M; ++j) gi += Q[Sym<M>::at(i, j)] * alpha[j];
                g[i] = gi;
                val += alpha[i] * gi;
            }
            double gmin = kInf;
#pragma unroll
            for (int i = 0; i < M; ++i)
                if (i < m && !(((S | banned) >> i) & 1u) && g[i] < gmin) { gmin = g[i]; jb = i; }
            if (jb < 0 || !(gmin < val - tol)) break;
            S |= 1u << jb;
        }
        for (int mi = 0; mi <= M; ++mi) {
            double beta[M];
            if (!solve_affine<M>(Q, scale, S, beta)) {
                if (jb < 0) {   // the full-set start met a dependent set: the nearest vertex alone
                    S = 1u << i0;
#pragma unroll
                    for (int i = 0; i < M; ++i) alpha[i] = (i == i0) ? 1.0 : 0.0;
                    break;
                }
                S &= ~(1u << jb);
                banned |= 1u << jb;
                break;
            }
            bool allpos = true;
#pragma unroll
            for (int i = 0; i < M; ++i)
                if (((S >> i) & 1u) && !(beta[i] > 0.0)) allpos = false;
            if (allpos) {
                // (the full-set start cut down to one vertex: its weight is 1, as where the method starts from that vertex)
                const bool one = jb < 0 && (S & (S - 1u)) == 0u;
#pragma unroll
                for (int i = 0; i < M; ++i) alpha[i] = ((S >> i) & 1u) ? (one ? 1.0 : beta[i]) : 0.0;
                break;
            }
            double theta = 1.0;
            int kr = -1;
#pragma unroll
            for (int i = 0; i < M; ++i)
                if (((S >> i) & 1u) && !(beta[i] > 0.0)) {
                    const double den = alpha[i] - beta[i];
                    const double r = den > 0.0 ? alpha[i] / den : 0.0;
                    if (kr < 0 || r < theta) { theta = r; kr = i; }
                }
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const double v = alpha[i] + theta * (beta[i] - alpha[i]);
                alpha[i] = (((S >> i) & 1u) && i != kr) ? v : 0.0;
            }
            S &= ~(1u << kr);
            if (kr == jb) banned |= 1u << jb;
        }
    }
    double val = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        double gi = 0.0;
#pragma unroll
        for (int j = 0; j < M; ++j) gi += Q[Sym<M>::at(i, j)] * alpha[j];
        val += alpha[i] * gi;
    }
    return val;
}

// Distance^2 to the AFFINE hull of the first m vertices (hull_distance.py:69-87 affine_hull_distance
// and :38-66 affine_hull_distance_qp: same quantity): the affine minimiser over a maximal affinely
// independent subset, built greedily -- a vertex whose addition collapses a pivot of the lifted
// Gram lies in the affine hull of those already taken and is skipped.
template <int M>
__device__ __forceinline__ double affine_min_norm(const double (&Q)[Sym<M>::NP], int m, double (&alpha)[M])
{
    double scale = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        alpha[i] = 0.0;
        if (i < m) scale = fmax(scale, Q[Sym<M>::at(i, i)]);
    }
    if (!(scale > 0.0)) {
#pragma unroll
        for (int i = 0; i < M; ++i) alpha[i] = (i == 0) ? 1.0 : 0.0;
        return scale == 0.0 ? 0.0 : scale;
    }
    unsigned S = 0u;
    double beta[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
        if (k < m) {
            double trial[M];
            if (solve_affine<M>(Q, scale, S | (1u << k), trial)) {
                S |= 1u << k;
#pragma unroll
                for (int i = 0; i < M; ++i) beta[i] = trial[i];
            }
        }
    }
    if (S == 0u) {   // cannot happen for scale > 0 (a single vertex is always independent)
#pragma unroll
        for (int i = 0; i < M; ++i) alpha[i] = (i == 0) ? 1.0 : 0.0;
        return Q[0];
    }
    double val = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) alpha[i] = ((S >> i) & 1u) ? beta[i] : 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
        double gi = 0.0;
#pragma unroll
        for (int j = 0; j < M; ++j) gi += Q[Sym<M>::at(i, j)] * alpha[j];
        val += alpha[i] * gi;
    }
    return val;
}


// Sum v[e] over the 16 lanes of a group and leave entry e = l16 on lane l16: a reduce-scatter in
// four halving steps (15 exchanges instead of the 64 of sixteen butterfly reductions).  The exchanges are DPP moves
// (row_xor_f64 of hull_solve16.h): a step waits for no LDS round trip.  Every sum is the pair, in the order, of the
// shuffle form this replaces (reduce_scatter16_shfl below, kept for the self-check), so the result has the same bits.
__device__ __forceinline__ double reduce_scatter16(const double (&v)[16], int l16)
{
    double t8[8], t4[4], t2[2];
    const bool b8 = l16 & 8, b4 = l16 & 4, b2 = l16 & 2, b1 = l16 & 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) t8[e] = (b8 ? v[e + 8] : v[e]) + row_xor_f64<8>(b8 ? v[e] : v[e + 8]);
#pragma unroll
    for (int e = 0; e < 4; ++e) t4[e] = (b4 ? t8[e + 4] : t8[e]) + row_xor_f64<4>(b4 ? t8[e] : t8[e + 4]);
#pragma unroll
    for (int e = 0; e < 2; ++e) t2[e] = (b2 ? t4[e + 2] : t4[e]) + row_xor_f64<2>(b2 ? t4[e] : t4[e + 2]);
    return (b1 ? t2[1] : t2[0]) + row_xor_f64<1>(b1 ? t2[0] : t2[1]);
}
__device__ __forceinline__ double reduce_scatter16_shfl(const double (&v)[16], int l16)
{
    double t8[8], t4[4], t2[2];
    const bool b8 = l16 & 8, b4 = l16 & 4, b2 = l16 & 2, b1 = l16 & 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) t8[e] = (b8 ? v[e + 8] : v[e]) + __shfl_xor(b8 ? v[e] : v[e + 8], 8, 64);
#pragma unroll
    for (int e = 0; e < 4; ++e) t4[e] = (b4 ? t8[e + 4] : t8[e]) + __shfl_xor(b4 ? t8[e] : t8[e + 4], 4, 64);
#pragma unroll
    for (int e = 0; e < 2; ++e) t2[e] = (b2 ? t4[e + 2] : t4[e]) + __shfl_xor(b2 ? t4[e] : t4[e + 2], 2, 64);
    return (b1 ? t2[1] : t2[0]) + __shfl_xor(b1 ? t2[0] : t2[1], 1, 64);
}

// INDEXED = false: problems are (batch position, bin) pairs whose vertices come from the top-m
// lists.  INDEXED = true: explicit (query sample, compacted vertex index list, count) problems.
template <int M, int WAVES, bool INDEXED>
__global__ __launch_bounds__(64 * WAVES, (M <= 5 ? 4 : 1)) void hull_qp_kernel(QpArgs a, int nprob, const int *xq,
                                                              const int *xhull, const int *xn,
                                                              int xm, double *xdist, double *xalpha, Gate gate)
{
    CHB_GATE(gate);
    constexpr int NP = Sym<M>::NP;
    static_assert(M <= 8, "m > 8 runs on hull_qp16_kernel");
    __shared__ double sQ[WAVES][NP][65];    // (65: the 16 lanes of a group store 16 entries of ONE problem column -- a stride of 64 doubles would put them all on one bank)
    __shared__ int sN[WAVES][64];

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = INDEXED ? xm : a.m;
    // active mode: the problems are the listed pairs (device-side count), walked grid-stride
    const int *act = INDEXED ? nullptr : a.active;
    if (act != nullptr) nprob = *a.n_active;
    // a listed (usually short) problem set is spread as thinly as possible -- four problems per wavefront,
    // one pass -- because a wavefront's sixteen passes are a serial chain of memory round trips
    const int npass = act != nullptr ? 1 : 16;
    const int ppw = 4 * npass;

    for (int g0 = (blockIdx.x * WAVES + w) * ppw; g0 < nprob; g0 += (int)gridDim.x * WAVES * ppw) {
    {
        // 16 lanes per problem, lane l16 over the features k = l16 (mod 16): every row is read in
        // full 128-byte lines, each lane accumulates all M (M + 1) / 2 products of its features, and
        // a reduce-scatter leaves one finished Gram entry per lane.  For M <= 8 this beats the
        // 16 x 16 matrix-core tile, most of which (the blocks between different problems) is waste.
        const int grp = lane >> 4, l16 = lane & 15;
        for (int pass = 0; pass < npass; ++pass) {
            const int pl = pass * 4 + grp;
            const int g = g0 + pl;
            const bool valid = g < nprob;
            int n = 0, idm = -1, qid = 0;
            size_t slot = 0;
            if (valid) {
                if (INDEXED) {
                    qid = xq[g];
                    n = xn[g];
                    if (l16 < n) idm = xhull[(size_t)g * m + l16];
                } else {
                    const int pr = act ? act[g] : g;
                    const int pos = a.pos_begin + pr / a.B, c = pr - (pr / a.B) * a.B;
                    qid = a.bq[pos];
                    slot = (size_t)c * a.Kcap + pos;
                    n = a.lists.cnt[slot];
                    if (l16 < n) idm = a.lists.idx[slot * m + l16];
                }
            }
            bool changed = valid;
            if (!INDEXED && a.prev.idx != nullptr && act == nullptr && valid)
                changed = a.prev.cnt[slot] != n || (l16 < n && a.prev.idx[slot * m + l16] != idm);
            const bool doit = ((__ballot(changed) >> (16 * grp)) & 0xFFFFull) != 0ull;
            const double *vrow[M];
#pragma unroll
            for (int v = 0; v < M; ++v) {
                const int idv = __shfl(idm, 16 * grp + v, 64);
                // a missing vertex reads the query row: y = 0, its Gram row/column stays 0 (never used)
                vrow[v] = a.X + (size_t)(idv >= 0 ? idv : qid) * a.Dp;
            }
            if (!valid) continue;
            if (!doit) {   // unchanged vertex list: keep the stored distance
                if (l16 == 0) sN[w][pl] = -1;
                continue;
            }
            const double *xrow = a.X + (size_t)qid * a.Dp;
            double acc[NP];
#pragma unroll
            for (int e = 0; e < NP; ++e) acc[e] = 0.0;
            if (n > 0) {
                // 32 features per step as 16-byte loads (lane l16: features 2 l16, 2 l16 + 1), then the
                // remaining < 32 features one double per lane
                const int Dmain = a.Dp & ~31;
#pragma unroll CHB_QP_UNROLL
                for (int k = 2 * l16; k < Dmain; k += 32) {
                    const double2 xk = *reinterpret_cast<const double2 *>(xrow + k);
                    double2 y[M];
#pragma unroll
                    for (int v = 0; v < M; ++v) {
                        const double2 pv = *reinterpret_cast<const double2 *>(vrow[v] + k);
                        y[v] = double2{pv.x - xk.x, pv.y - xk.y};
                    }
#pragma unroll
                    for (int i = 0; i < M; ++i)
#pragma unroll
                        for (int j = 0; j <= i; ++j) {
                            double acc_ij = acc[Sym<M>::at(i, j)];
                            acc_ij = fma(y[i].x, y[j].x, acc_ij);
                            acc[Sym<M>::at(i, j)] = fma(y[i].y, y[j].y, acc_ij);
                        }
                }
                for (int k = Dmain + l16; k < a.Dp; k += 16) {
                    const double xk = xrow[k];
                    double y[M];
#pragma unroll
                    for (int v = 0; v < M; ++v) y[v] = vrow[v][k] - xk;
#pragma unroll
                    for (int i = 0; i < M; ++i)
#pragma unroll
                        for (int j = 0; j <= i; ++j) acc[Sym<M>::at(i, j)] = fma(y[i], y[j], acc[Sym<M>::at(i, j)]);
                }
            }
#pragma unroll
            for (int e0 = 0; e0 < NP; e0 += 16) {
                double v16[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) v16[e] = e0 + e < NP ? acc[e0 + e] : 0.0;
                const double r = reduce_scatter16(v16, l16);
                if (e0 + l16 < NP) sQ[w][e0 + l16][pl] = r;
            }
            if (l16 == 0) sN[w][pl] = n;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes have landed

    const int g = g0 + lane;
    if (lane >= ppw || g >= nprob) continue;
    double Q[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) Q[e] = sQ[w][e][lane];
    const int n = sN[w][lane];
    if (n == -1) continue;   // unchanged vertex list: a.dist already holds this distance
    double alpha[M];
    double dist;
    if (n <= 0) {
        dist = kInf;
#pragma unroll
        for (int v = 0; v < M; ++v) alpha[v] = 0.0;
    } else {
        const double val = a.metric == 0 ? min_norm_point<M>(Q, n, alpha) : affine_min_norm<M>(Q, n, alpha);
        dist = sqrt(fmax(val, 0.0));
    }
    if (INDEXED) {
        xdist[g] = dist;
        if (xalpha) {
#pragma unroll
            for (int v = 0; v < M; ++v)
                if (v < m) xalpha[(size_t)g * m + v] = alpha[v];
        }
    } else {
        const int pr = act ? act[g] : g;
        const int pos = a.pos_begin + pr / a.B, c = pr - (pr / a.B) * a.B;
        a.dist[(size_t)pos * a.B + c] = dist;
    }
    }   // grid-stride loop
}

// ---------------------------------------------------------------------------------------------
// Fused selection + hull distance (FusedArgs in chb_internal.h).  16 lanes per (position, bin) pair as in
// hull_qp_kernel, but over the pair's SHORTLIST (<= C candidates): one sweep over the candidate rows
// accumulates the full C x C shifted Gram.  Its diagonal holds the squared distances of the candidates
// (fp64, fused sums: within ~D eps of the exact value), which rank them; the m x m block of the m
// nearest is the Gram of the hull QP -- no row is read twice.
// Exactness of the selected SET: cdist's (sequentially rounded distance, index) order and this
// kernel's order can only disagree between candidates whose squared distances agree to ~1e-14
// relative; a pair whose m-th and (m+1)-th candidates are closer than kTieRel (1e-11) relative is
// not decided here but handed to the exact path (`slow`).  The ORDER inside the selected set may
// differ from cdist's on such near-ties inside the set; the hull distance does not depend on it
// beyond rounding.
constexpr double kTieRel = 1e-11;

// OFF32: the rows are addressed as 32-bit byte offsets from the (uniform) base of X -- half the registers of
// 64-bit row pointers, which is what keeps the kernel free of spills at 3 wavefronts per SIMD (the launcher picks
// it when the sample matrix is smaller than 4 GiB).
template <int CC, int NR, bool OFF32>
__device__ __forceinline__ void gram_rows(const double *X, int Dp, int Dk, int qid, int idm, int l16, double (&r)[NR])
{   // (Dp: row stride -- whole 128-byte lines; Dk: the columns swept, D rounded up to 8: the padding beyond is never read)
    constexpr int NP = CC * (CC + 1) / 2;
    static_assert(NP <= 16 * NR, "result registers");
    const char *Xb = reinterpret_cast<const char *>(X);
    const double *xrow = X + (size_t)qid * Dp;
    const unsigned xoff = (unsigned)qid * (unsigned)Dp * 8u;
    const double *vrow[OFF32 ? 1 : CC];
    unsigned voff[OFF32 ? CC : 1];
    for_row_lanes<CC>([&](auto lv) {
        constexpr int v = decltype(lv)::value;
        const int idv = row_bcast_i32<v>(idm);
        // a missing candidate reads the query row: y = 0, its Gram row / column stays 0 (never used)
        if (OFF32) voff[OFF32 ? v : 0] = (unsigned)(idv >= 0 ? idv : qid) * (unsigned)Dp * 8u;
        else vrow[OFF32 ? 0 : v] = X + (size_t)(idv >= 0 ? idv : qid) * Dp;
    });
    auto xat = [&](int k) { return OFF32 ? reinterpret_cast<const double *>(Xb + (size_t)(xoff + 8u * (unsigned)k)) : xrow + k; };
    auto vat = [&](int v, int k) {
        return OFF32 ? reinterpret_cast<const double *>(Xb + (size_t)(voff[OFF32 ? v : 0] + 8u * (unsigned)k)) : vrow[OFF32 ? 0 : v] + k;
    };
    double acc[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) acc[e] = 0.0;
    const int Dmain = Dk & ~31;
#pragma unroll 1
    for (int k = 2 * l16; k < Dmain; k += 32) {
        const double2 xk = *reinterpret_cast<const double2 *>(xat(k));
        double2 y[CC];
#pragma unroll
        for (int v = 0; v < CC; ++v) {
            const double2 pv = *reinterpret_cast<const double2 *>(vat(v, k));
            y[v] = double2{pv.x - xk.x, pv.y - xk.y};
        }
#pragma unroll
        for (int i = 0; i < CC; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double t = acc[i * (i + 1) / 2 + j];
                t = fma(y[i].x, y[j].x, t);
                acc[i * (i + 1) / 2 + j] = fma(y[i].y, y[j].y, t);
            }
    }
    for (int k = Dmain + l16; k < Dk; k += 16) {
        const double xk = *xat(k);
        double y[CC];
#pragma unroll
        for (int v = 0; v < CC; ++v) y[v] = *vat(v, k) - xk;
#pragma unroll
        for (int i = 0; i < CC; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) acc[i * (i + 1) / 2 + j] = fma(y[i], y[j], acc[i * (i + 1) / 2 + j]);
    }
#pragma unroll
    for (int t = 0; t < NR; ++t) {
        double v16[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v16[e] = 16 * t + e < NP ? acc[16 * t + e] : 0.0;
        r[t] = 16 * t < NP ? reduce_scatter16(v16, l16) : 0.0;
    }
}

#ifndef CHB_FUSED_C
#define CHB_FUSED_C 7
#endif
#ifndef CHB_FUSED_OCC
#define CHB_FUSED_OCC 3
#endif
#ifndef CHB_FUSED_WIDE
#define CHB_FUSED_WIDE 16
#endif
constexpr int kFusedWide = CHB_FUSED_WIDE;   // widest shortlist the fused kernel takes (one candidate per lane of a group)

// squared distances only: candidate v (v < 8) of every 16-lane group is the one held by lane V0 + v of the group;
// on return lane l16 < 8 holds the squared distance of candidate V0 + l16
template <bool OFF32, int V0>
__device__ __forceinline__ double diag_rows8(const double *X, int Dp, int Dk, int qid, int idm, int l16)
{
    const char *Xb = reinterpret_cast<const char *>(X);
    const double *xrow = X + (size_t)qid * Dp;
    const unsigned xoff = (unsigned)qid * (unsigned)Dp * 8u;
    const double *vrow[OFF32 ? 1 : 8];
    unsigned voff[OFF32 ? 8 : 1];
    for_row_lanes<8>([&](auto lv) {
        constexpr int v = decltype(lv)::value;
        const int idv = row_bcast_i32<V0 + v>(idm);
        if (OFF32) voff[OFF32 ? v : 0] = (unsigned)(idv >= 0 ? idv : qid) * (unsigned)Dp * 8u;
        else vrow[OFF32 ? 0 : v] = X + (size_t)(idv >= 0 ? idv : qid) * Dp;
    });
    auto xat = [&](int k) { return OFF32 ? reinterpret_cast<const double *>(Xb + (size_t)(xoff + 8u * (unsigned)k)) : xrow + k; };
    auto vat = [&](int v, int k) {
        return OFF32 ? reinterpret_cast<const double *>(Xb + (size_t)(voff[OFF32 ? v : 0] + 8u * (unsigned)k)) : vrow[OFF32 ? 0 : v] + k;
    };
    double acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
    const int Dmain = Dk & ~31;
#pragma unroll 1
    for (int k = 2 * l16; k < Dmain; k += 32) {
        const double2 xk = *reinterpret_cast<const double2 *>(xat(k));
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const double2 pv = *reinterpret_cast<const double2 *>(vat(v, k));
            const double dx = pv.x - xk.x, dy = pv.y - xk.y;
            acc[v] = fma(dy, dy, fma(dx, dx, acc[v]));
        }
    }
    for (int k = Dmain + l16; k < Dk; k += 16) {
        const double xk = *xat(k);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const double d = *vat(v, k) - xk;
            acc[v] = fma(d, d, acc[v]);
        }
    }
    return reduce_scatter16(acc, l16);
}

// Trim.  A pair with more than C candidates costs the kernel a distance sweep over up to 16 fp64 rows (or the exact path,
// above 16) although only the m nearest of them enter the hull.  Where the fit has global shadow rows (prefilter_kernels.hip;
// TrimArgs: Gs[p] = fp16((x_p - mu_g) S), gq[p] = {N_p = ||Gs[p]||^2 rounded up, rho_p = ||Gs[p] - (x_p - mu_g) S|| rounded
// up}) such a pair of up to kTrimMax candidates is cut down BEFORE any fp64 row of a candidate is read.  The triangle
// inequality alone gives, for query j and candidate p,
//     sqrt(T) - rho_j - rho_p <= S d(j, p) <= sqrt(T) + rho_j + rho_p,     T = ||Gs[j] - Gs[p]||^2 = N_j + N_p - 2 <Gs[j], Gs[p]>
// -- no bias pieces, no tile terms, no per-bin bounds.  The dot product comes from v_dot2_f32_f16 (fp16 products are exact in
// fp32) summed in fp32 and, over the 16 lanes, in fp64; the computed T is within
//     E = 2 g sqrt(N_j N_p) + 2^-23 (N_j + N_p) + 2^-13 sqrt(D) (sqrt(N_j) + sqrt(N_p)) + D 2^-27
// of the exact one: g = 2.5e-5 bounds the fp32 summation of up to 161 terms in any order (Cauchy-Schwarz on the sum of the
// terms' magnitudes; the constant of prefilter_kernels.hip), the second term the stored norms' rounding, the last two a
// flush of fp16 subnormals to zero, should the instruction do that.  So LB = sqrt(max(T - E, 0)) - rho_j - rho_p and
// UB = sqrt(T + E) + rho_j + rho_p.  tau_u = the m-th smallest UB among the pair's candidates: m of them are provably within
// tau_u, so the m-th distance of the union is at most tau_u / S.  Candidate p is dropped only if LB_p > tau_u (1 + kTrimSlack)
// holds; a NaN or infinite bound anywhere in the pair keeps all of it.
// Guarantee.  Every candidate within 1e-6 relative of the union's m-th distance survives (the fp64 rounding of the bound
// arithmetic, ~1e-15 relative, comes out of that slack).  That covers the m nearest, and any (m+1)-th candidate that the
// kTieRel = 1e-11 test could call a tie of the m-th.  So the selected set, the tie hand-off to the exact path and the hull's
// vertex set are what they are without the trim; only the slot a Gram entry is summed in can differ (its last bit).
// A pair keeps its survivors (at most kTrimKeep, in shortlist order) in the LDS id list and is classed by their number; one
// with more survivors stays as it was.
// The LDS id list (sIds) also takes the ids of every untrimmed pair of at most kTrimKeep candidates: at classification the
// lane that owns the pair loads them (all 64 pairs of the wavefront in one round trip), so that a pass starts on its row
// sweep without a dependent global load of the ids first.  Only pairs of kTrimKeep < n <= 16 candidates fetch theirs in
// the pass.
constexpr int kTrimMax = 32;     // two candidates per lane of a 16-lane group
constexpr int kTrimKeep = 8;     // ids per pair in the LDS list
constexpr int kNbInLds = -1;     // base count of a pair in the passes whose ids come from the LDS list
constexpr double kTrimSlack = 1e-6;
constexpr double kTrimGamma = 2.5e-5;   // fp32 summation of up to 161 terms (kGamma of prefilter_kernels.hip)

// The columns of a lane in a shadow sweep (rows of up to 160 columns): the 8 from 8 * l16 on (one 16-byte load) and the 2
// from 128 + 2 * l16 on (one 4-byte load; clamped to the row's last pair, which the mask then clears).
__device__ __forceinline__ int trim_tail_col(int l16) { return 128 + 2 * l16; }

// <Gs[j], Gs[p]> of the first nmax (uniform) of 16 candidates: candidate v of every 16-lane group is the one its lane v
// holds in `ids` (none: the query's own row is read, the value is not used); qm / qt = the lane's 10 columns of the query's
// row, the halves from column D on cleared (there the rows carry the shortlist kernels' bias constants).  On return lane l16
// holds the product of candidate l16.
__device__ __forceinline__ double shadow_dot16(const unsigned short *Gs, int Dz, int qid, int ids, int nmax, int l16,
                                               const uint4 &qm, unsigned qt)
{
    using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
    auto dot2 = [](unsigned x, unsigned y, float c) {
        return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, x), __builtin_bit_cast(f16x2, y), c, false);
    };
    const int tcol = min(trim_tail_col(l16), Dz - 2);
    double acc[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.0;
    for_row_lanes<4>([&](auto lq) {
        constexpr int v0 = 4 * decltype(lq)::value;
        if (v0 < nmax) {
            for_row_lanes<4>([&](auto lv) {
                constexpr int v = v0 + decltype(lv)::value;
                const int idv = row_bcast_i32<v>(ids);
                const unsigned short *row = Gs + (size_t)(idv >= 0 ? idv : qid) * Dz;
                const uint4 u = *reinterpret_cast<const uint4 *>(row + 8 * l16);   // (8 * l16 + 8 <= 128 < Dz)
                const unsigned ut = *reinterpret_cast<const unsigned *>(row + tcol);
                acc[v] = (double)dot2(ut, qt, dot2(u.w, qm.w, dot2(u.z, qm.z, dot2(u.y, qm.y, dot2(u.x, qm.x, 0.f)))));
            });
        }
    });
    return reduce_scatter16(acc, l16);
}

// Work order of the m <= 5 fused kernel.  STRIPED (a.stripe != 0, B >= 16): consecutive workgroups go round-robin over the
// 8 XCDs, each with its own L2; workgroup b (XCD b % 8) only takes pairs of the bins c = b % 8 (mod 8), walked position-major
// over that bin subset (64 consecutive pairs per wavefront = 64 / nbx positions x the XCD's nbx bins).  The candidate rows an
// XCD gathers then come from an eighth of the bins -- its 4 MiB L2 holds a far larger share of them -- while a query row is
// still shared by the nbx pairs of a position.  Otherwise: position-major over all bins (one position x 64 bins per
// wavefront at B = 64).
__device__ __forceinline__ bool fused_pair_of(const FusedArgs &a, int g0, int lane, int nprob, int &pos, int &c)
{
    if (!a.stripe) {
        const int g = g0 + lane;
        pos = a.pos_begin + g / a.B;
        c = g - (g / a.B) * a.B;
        return g < nprob;
    }
    const int x = (int)(blockIdx.x & 7);
    const int nbx = (a.B - x + 7) >> 3;                    // bins c = x (mod 8)
    const int t = g0 + lane;                               // pair number inside the XCD's list
    const int pq = t / nbx;
    pos = a.pos_begin + pq;
    c = x + 8 * (t - pq * nbx);
    return pq < a.pos_end - a.pos_begin;
}

template <int M, int C, int WAVES, bool OFF32>
__global__ __launch_bounds__(64 * WAVES, CHB_FUSED_OCC) void hull_select_qp_kernel(FusedArgs a, int nprob, Gate gate)
{
    CHB_GATE(gate);
    constexpr int NPM = Sym<M>::NP;            // Gram entries of the hull QP
    constexpr int NPC = C * (C + 1) / 2;       // ... of the candidate Gram
    constexpr int NR = (NPC + 15) / 16;
    constexpr int NCLS = C - M + 1;            // classes of the one-sweep form: widths M, M + 1, ..., C
    static_assert(C <= 8 && M <= C && C - M <= 3, "candidate Gram in registers");
    static_assert(C <= kTrimKeep, "the narrow passes take their ids from the LDS list");
    __shared__ double sQ[WAVES][NPM][65];   // (65: the 16 lanes of a group store 16 entries of ONE problem column -- a stride of 64 doubles would put them all on one bank)
    __shared__ double sT[WAVES][4][NR * 16];   // candidate Gram of the group's pair
    __shared__ double sTh[WAVES][4][2];        // squared distances of ranks m-1 and m
    __shared__ int sSel[WAVES][4][16];         // candidate slot of each rank
    __shared__ int sN[WAVES][64];
    __shared__ int sOrd[WAVES][64];            // problem (lane) of each work position, narrow shortlists first
    __shared__ int sSlowN, sSlowBase;
    __shared__ int sIds[WAVES][64][kTrimKeep];    // candidate ids of a pair with at most kTrimKeep of them (see "Trim" above)
    __shared__ int sTrimN[WAVES][64];             // ... their number; 0: the pair is not trimmed
    __shared__ int sTrimCtr[3];                   // pairs through the trim, their candidates before and after

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int grp = lane >> 4, l16 = lane & 15, gbase = lane & 48;
    const int m = a.m;
    const int Dk = (a.D + 7) & ~7;   // columns swept (the rows are padded to whole 128-byte lines beyond)
    if (threadIdx.x == 0) sSlowN = 0;
    if (threadIdx.x < 3) sTrimCtr[threadIdx.x] = 0;
    __syncthreads();
    // (striped: the wavefront's place in its XCD's own pair list; nprob is then the length of the longest of the 8 lists)
    const int g0 = ((a.stripe ? (int)(blockIdx.x >> 3) : (int)blockIdx.x) * WAVES + w) * 64;
    unsigned long long slowmask = 0ull;        // problems of this wavefront left to the exact path
    int pos = 0, c = 0;
    bool valid = false;

    if (g0 < nprob) {
        // ---- classification, one problem per lane
        valid = fused_pair_of(a, g0, lane, nprob, pos, c);
        int nb = 0, nu = 0, qid = 0;
        size_t slot = 0;
        bool changed = valid;
        if (valid) {
            qid = a.bq[pos];
            slot = (size_t)c * a.Kcap + pos;
            nb = a.cand_cnt[slot];
            if (a.candu != nullptr) nu = a.candu_cnt[slot];
            // unchanged set of batch-entry candidates (the base candidates are fixed during a batch): keep
            if (a.candp != nullptr && a.candp_cnt[slot] == nu) {
                if (nu == 0) changed = false;
                else if (nu <= 8) {
                    bool same = true;
                    for (int i = 0; i < nu; ++i) {
                        const int u = a.candu[slot * kCandCapU + i];
                        bool f = false;
                        for (int j = 0; j < nu; ++j) f = f || a.candp[slot * kCandCapU + j] == u;
                        same = same && f;
                    }
                    changed = !same;
                }
            }
        }
        if (a.short_cnt != nullptr) {
            // the shortlist stage's contract (a short list would be a wrong hull with no error, a wild index a fault)
            bool sh = false;
            if (valid) sh = nb < min(m, a.bin_size != nullptr ? a.bin_size[c] : a.bin_ptr[c + 1] - a.bin_ptr[c]);
            const unsigned long long shm = __ballot(sh);
            if (shm != 0ull && lane == 0) atomicAdd(a.short_cnt, __popcll(shm));
        }
        int n = nb + nu;
        // ---- trim (see "Trim" above): pairs with C < n <= kTrimMax, 16 lanes per pair, four pairs per pass, before any
        // fp64 row of a candidate is read; the classes below then see the survivors.  A loop of its own.
        if (a.trim != nullptr) {
            const bool tr = changed && n > C && n <= kTrimMax;
            const unsigned long long tmask = __ballot(tr);
            const int ntrim = __popcll(tmask);
            if (ntrim > 0) {
                sTrimN[w][lane] = 0;
                if (tr) sOrd[w][__popcll(tmask & ((1ull << lane) - 1ull))] = lane;   // (sOrd: rebuilt below)
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xC07F);
                const TrimArgs ta = *a.trim;
                // (masks by shifts: compares would hold one lane mask each in scalar registers through the loop)
                auto mask32 = [](int nv) { return (unsigned)((1ull << min(max(16 * nv, 0), 32)) - 1ull); };   // nv columns below D
                const int nv = a.D - 8 * l16;
                const uint4 msk{mask32(nv), mask32(nv - 2), mask32(nv - 4), mask32(nv - 6)};
                const unsigned mskt = mask32(a.D - trim_tail_col(l16));
                int c_pairs = 0, c_in = 0, c_kept = 0;
                for (int p0 = 0; p0 < ntrim; p0 += 4) {
                    const int op = p0 + grp;
                    const bool has = op < ntrim;
                    const int pl = has ? sOrd[w][op] : 0;
                    const int n_s = __shfl(n, pl, 64);
                    const int n_g = has ? n_s : 0;
                    const int nb_g = __shfl(nb, pl, 64);
                    const int qid_g = __shfl(qid, pl, 64);
                    const size_t slot_g = (size_t)__shfl(c, pl, 64) * a.Kcap + (size_t)__shfl(pos, pl, 64);
                    // candidates l16 and 16 + l16 of the group's pair
                    int id0 = -1, id1 = -1;
                    if (l16 < n_g)
                        id0 = l16 < nb_g ? a.cand[slot_g * kCandCap + l16] : a.candu[slot_g * kCandCapU + (l16 - nb_g)];
                    if (16 + l16 < n_g)
                        id1 = 16 + l16 < nb_g ? a.cand[slot_g * kCandCap + 16 + l16] : a.candu[slot_g * kCandCapU + (16 + l16 - nb_g)];
                    bool bad = false;   // a wild index: the pair stays as it is (the passes below count it)
                    if ((unsigned)id0 >= (unsigned)a.n_samples && id0 != -1) { bad = true; id0 = -1; }
                    if ((unsigned)id1 >= (unsigned)a.n_samples && id1 != -1) { bad = true; id1 = -1; }
                    int nmax = n_g;
                    nmax = max(nmax, __shfl_xor(nmax, 16, 64));
                    nmax = max(nmax, __shfl_xor(nmax, 32, 64));
                    nmax = __builtin_amdgcn_readfirstlane(nmax);
                    // the lane's columns of the query's own shadow row, its norm and radius
                    const unsigned short *qrow = ta.Gs + (size_t)qid_g * ta.Dz;
                    uint4 qm = *reinterpret_cast<const uint4 *>(qrow + 8 * l16);
                    qm.x &= msk.x; qm.y &= msk.y; qm.z &= msk.z; qm.w &= msk.w;
                    const unsigned qt = *reinterpret_cast<const unsigned *>(qrow + min(trim_tail_col(l16), ta.Dz - 2)) & mskt;
                    const float2 gj = ta.gq[qid_g];
                    const bool in0 = id0 >= 0, in1 = id1 >= 0;
                    const float2 g0 = ta.gq[in0 ? id0 : qid_g], g1 = ta.gq[in1 ? id1 : qid_g];
                    const double dot0 = shadow_dot16(ta.Gs, ta.Dz, qid_g, id0, nmax, l16, qm, qt);
                    double dot1 = 0.0;
                    if (nmax > 16) dot1 = shadow_dot16(ta.Gs, ta.Dz, qid_g, id1, nmax - 16, l16, qm, qt);
                    // the bounds (see "Trim")
                    const double Nj = (double)gj.x, sNj = sqrt(Nj), flush = 0x1p-13 * sqrt((double)a.D);
                    auto bounds = [&](double dot, float2 gp, double &lo, double &hi) {
                        const double Np = (double)gp.x, sNp = sqrt(Np), rho = (double)gj.y + (double)gp.y;
                        const double T = Nj + Np - 2.0 * dot;
                        const double E = 2.0 * kTrimGamma * sNj * sNp + 0x1p-23 * (Nj + Np) + flush * (sNj + sNp) + 0x1p-27 * (double)a.D;
                        lo = sqrt(fmax(T - E, 0.0)) - rho;
                        hi = sqrt(T + E) + rho;
                    };
                    double lo0, lo1, hi0, hi1;
                    bounds(dot0, g0, lo0, hi0);
                    bounds(dot1, g1, lo1, hi1);
                    if (!in0) hi0 = kInf;
                    if (!in1) hi1 = kInf;
                    bad = bad || (in0 && !(hi0 < kInf)) || (in1 && !(hi1 < kInf));   // NaN or infinite: no bound, keep everything
                    // tau_u: the upper bound of rank m - 1 by (bound, slot)
                    int rank0 = 0, rank1 = 0;
                    for_row_lanes<16>([&](auto lu) {
                        constexpr int u = decltype(lu)::value;
                        const double hu = row_bcast_f64<u>(hi0);
                        rank0 += (hu < hi0 || (hu == hi0 && u < l16)) ? 1 : 0;
                        rank1 += hu <= hi1 ? 1 : 0;
                    });
                    if (nmax > 16) {
                        for_row_lanes<16>([&](auto lu) {
                            constexpr int u = decltype(lu)::value;
                            const double hu = row_bcast_f64<u>(hi1);
                            rank0 += hu < hi0 ? 1 : 0;
                            rank1 += (hu < hi1 || (hu == hi1 && u < l16)) ? 1 : 0;
                        });
                    }
                    double tau = (in0 && rank0 == m - 1) ? hi0 : (in1 && rank1 == m - 1) ? hi1 : kInf;
                    tau = fmin(tau, row_xor_f64<1>(tau));
                    tau = fmin(tau, row_xor_f64<2>(tau));
                    tau = fmin(tau, row_xor_f64<4>(tau));
                    tau = fmin(tau, row_xor_f64<8>(tau));
                    const double lim = tau * (1.0 + kTrimSlack);
                    const bool k0 = in0 && !(lo0 > lim), k1 = in1 && !(lo1 > lim);   // (a NaN keeps the candidate)
                    const unsigned badm = (unsigned)(__ballot(bad) >> gbase) & 0xffffu;
                    const unsigned b0 = (unsigned)(__ballot(k0) >> gbase) & 0xffffu, b1 = (unsigned)(__ballot(k1) >> gbase) & 0xffffu;
                    const int nk = badm != 0u ? n_g : __popc(b0) + __popc(b1);
                    if (has && badm == 0u && nk <= kTrimKeep) {
                        if (k0) sIds[w][pl][__popc(b0 & ((1u << l16) - 1u))] = id0;
                        if (k1) sIds[w][pl][__popc(b0) + __popc(b1 & ((1u << l16) - 1u))] = id1;
                        if (l16 == 0) sTrimN[w][pl] = nk;
                    }
                    if (has && l16 == 0) { c_pairs += 1; c_in += n_g; c_kept += nk; }
                }
                c_pairs += __shfl_xor(c_pairs, 16, 64); c_pairs += __shfl_xor(c_pairs, 32, 64);
                c_in += __shfl_xor(c_in, 16, 64); c_in += __shfl_xor(c_in, 32, 64);
                c_kept += __shfl_xor(c_kept, 16, 64); c_kept += __shfl_xor(c_kept, 32, 64);
                if (lane == 0) { atomicAdd(&sTrimCtr[0], c_pairs); atomicAdd(&sTrimCtr[1], c_in); atomicAdd(&sTrimCtr[2], c_kept); }
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xC07F);
                const int nt = sTrimN[w][lane];
                if (nt > 0) { n = nt; nb = kNbInLds; }
            }
        }
        // ---- ids of the untrimmed pairs with at most kTrimKeep candidates: base ids, then the batch-entry ids, loaded by the
        // pair's own lane into the LDS list (the wild-index check stays where a pass reads them)
        if (changed && nb != kNbInLds && n > 0 && n <= kTrimKeep) {
#pragma unroll
            for (int i = 0; i < kTrimKeep; ++i)
                if (i < n) sIds[w][lane][i] = i < nb ? a.cand[slot * kCandCap + i] : a.candu[slot * kCandCapU + (i - nb)];
            nb = kNbInLds;
        }
        // class 0: nothing to compute here.  Classes 1 .. NCLS: ONE sweep over max(n, M) = M + k - 1 candidate
        // rows (full candidate Gram).  Class NCLS + 1 (C < n <= 16): a distance sweep over all candidates,
        // then a second sweep over the m selected rows (just read: they come out of L1 / L2).
        int cls = 0;
        if (changed && n > 0) {
            if (n <= C) cls = n <= M ? 1 : n - M + 1;
            else if (n <= kFusedWide) cls = NCLS + 1;
        }
        slowmask = __ballot(changed && n > kFusedWide);
        sN[w][lane] = (changed && n == 0) ? 0 : -1;   // -1: distance kept / written later
        int before = 0, nwork = 0, nnarrow = 0;
#pragma unroll
        for (int k = 1; k <= NCLS + 1; ++k) {
            const unsigned long long mk = __ballot(cls == k);
            if (cls == k) before = nwork + __popcll(mk & ((1ull << lane) - 1ull));
            nwork += __popcll(mk);
            if (k == NCLS) nnarrow = nwork;
        }
        if (cls > 0) sOrd[w][before] = lane;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);

        // ---- 16 lanes per problem, four problems per pass, narrow shortlists first.
        // (Shuffles stay outside any condition: a lane only delivers data while it is active.)
        for (int p0 = 0; p0 < nnarrow; p0 += 4) {
            const int op = p0 + grp;
            const bool has = op < nnarrow;
            const int pl = has ? sOrd[w][op] : 0;
            const int n_s = __shfl(n, pl, 64);
            const int n_g = has ? n_s : 0;
            const int qid_g = __shfl(qid, pl, 64);
            int idm = -1;
            if (l16 < n_g) idm = sIds[w][pl][l16];   // (n_g <= C <= kTrimKeep: every narrow pair's ids are in the LDS list)
            if ((unsigned)idm >= (unsigned)a.n_samples && idm != -1) {   // never a row address from a wild index
                if (a.short_cnt != nullptr) atomicAdd(a.short_cnt, 1);
                idm = -1;
            }
            // the widest shortlist of the pass (the last problem: they are sorted)
            const int cw = __builtin_amdgcn_readfirstlane(__shfl(n, sOrd[w][min(p0 + 3, nnarrow - 1)], 64));
            double r[NR];
            if (cw <= M) gram_rows<M, NR, OFF32>(a.X, a.Dp, Dk, qid_g, idm, l16, r);
            else if (C >= M + 1 && cw == M + 1) gram_rows<(C >= M + 1 ? M + 1 : M), NR, OFF32>(a.X, a.Dp, Dk, qid_g, idm, l16, r);
            else if (C >= M + 2 && cw == M + 2) gram_rows<(C >= M + 2 ? M + 2 : M), NR, OFF32>(a.X, a.Dp, Dk, qid_g, idm, l16, r);
            else gram_rows<C, NR, OFF32>(a.X, a.Dp, Dk, qid_g, idm, l16, r);
            bool tie = false;
            if (has && n_g <= m) {
                // every candidate is a hull vertex: the candidate Gram is the hull's (any vertex order)
#pragma unroll
                for (int t = 0; t < NR; ++t)
                    if (16 * t + l16 < NPM) sQ[w][16 * t + l16][pl] = r[t];
                if (l16 == 0) sN[w][pl] = n_g;
            } else if (has) {
#pragma unroll
                for (int t = 0; t < NR; ++t) sT[w][grp][16 * t + l16] = r[t];
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xC07F);
                // rank of my candidate by (squared distance, index); the ids come through LDS as well
                // (no shuffle inside a condition)
                if (l16 < C) sSel[w][grp][8 + l16] = idm;
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xC07F);
                const double sv = l16 < n_g ? sT[w][grp][l16 * (l16 + 3) / 2] : kInf;
                int rank = 0;
#pragma unroll
                for (int u = 0; u < C; ++u) {
                    const double su = sT[w][grp][u * (u + 3) / 2];
                    const int iu = sSel[w][grp][8 + u];
                    rank += (u < n_g && u != l16 && (su < sv || (su == sv && iu < idm))) ? 1 : 0;
                }
                if (l16 < n_g) {
                    if (rank < m) sSel[w][grp][rank] = l16;
                    if (rank == m - 1) sTh[w][grp][0] = sv;
                    if (rank == m) sTh[w][grp][1] = sv;
                }
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_s_waitcnt(0xC07F);
                const double t0 = sTh[w][grp][0], t1 = sTh[w][grp][1];
                tie = !(t1 - t0 > kTieRel * t1);   // (also catches NaN)
                if (!tie) {
#pragma unroll
                    for (int t = 0; 16 * t < NPM; ++t) {
                        const int e = 16 * t + l16;   // entry (i, j) of the hull Gram, ranks i >= j
                        int i = 0;
#pragma unroll
                        for (int q = 1; q < M; ++q) i += (q * (q + 1) / 2 <= e) ? 1 : 0;
                        const int j = e - i * (i + 1) / 2;
                        if (e < NPM) {
                            double val = 0.0;
                            if (i < m) {   // (j <= i)
                                const int vi = sSel[w][grp][i], vj = sSel[w][grp][j];
                                const int hi = vi > vj ? vi : vj, lo = vi > vj ? vj : vi;
                                val = sT[w][grp][hi * (hi + 1) / 2 + lo];
                            }
                            sQ[w][e][pl] = val;
                        }
                    }
                    if (l16 == 0) sN[w][pl] = m;
                }
            }
            if (l16 == 0 && tie) slowmask |= 1ull << pl;
        }

        // ---- wide shortlists (C < n <= 16): distances first, then the Gram of the m selected rows
        for (int p0 = nnarrow; p0 < nwork; p0 += 4) {
            const int op = p0 + grp;
            const bool has = op < nwork;
            const int pl = has ? sOrd[w][op] : 0;
            const int n_s = __shfl(n, pl, 64);
            const int n_g = has ? n_s : 0;
            const int nb_g = __shfl(nb, pl, 64);
            const int qid_g = __shfl(qid, pl, 64);
            const size_t slot_g = (size_t)__shfl(c, pl, 64) * a.Kcap + (size_t)__shfl(pos, pl, 64);
            int idm = -1;
            if (l16 < n_g)
                idm = nb_g == kNbInLds ? sIds[w][pl][l16]
                      : l16 < nb_g ? a.cand[slot_g * kCandCap + l16] : a.candu[slot_g * kCandCapU + (l16 - nb_g)];
            if ((unsigned)idm >= (unsigned)a.n_samples && idm != -1) {   // never a row address from a wild index
                if (a.short_cnt != nullptr) atomicAdd(a.short_cnt, 1);
                idm = -1;
            }
            int nmax = n_g;
            nmax = max(nmax, __shfl_xor(nmax, 16, 64));
            nmax = max(nmax, __shfl_xor(nmax, 32, 64));
            nmax = __builtin_amdgcn_readfirstlane(nmax);
            double sv = diag_rows8<OFF32, 0>(a.X, a.Dp, Dk, qid_g, idm, l16);
            if (nmax > 8) {
                const double s_hi = diag_rows8<OFF32, 8>(a.X, a.Dp, Dk, qid_g, idm, l16);
                const double moved = row_xor_f64<8>(s_hi);   // (lanes 8 .. 15 take candidates 8 .. 15 from lanes 0 .. 7)
                sv = l16 < 8 ? sv : moved;
            }
            if (l16 >= n_g) sv = kInf;
            // rank by (squared distance, index) among the group's n_g candidates
            int rank = 0;
            for_row_lanes<16>([&](auto lu) {
                constexpr int u = decltype(lu)::value;
                const double su = row_bcast_f64<u>(sv);
                const int iu = row_bcast_i32<u>(idm);
                rank += (u < n_g && u != l16 && (su < sv || (su == sv && iu < idm))) ? 1 : 0;
            });
            if (has && l16 < n_g) {
                if (rank < m) sSel[w][grp][rank] = idm;
                if (rank == m - 1) sTh[w][grp][0] = sv;
                if (rank == m) sTh[w][grp][1] = sv;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xC07F);
            bool tie = false;
            int idm2 = -1;
            if (has) {   // (n_g > C >= m: both thresholds exist)
                const double t0 = sTh[w][grp][0], t1 = sTh[w][grp][1];
                tie = !(t1 - t0 > kTieRel * t1);
                if (l16 < m) idm2 = sSel[w][grp][l16];
            }
            double r[NR];
            gram_rows<M, NR, OFF32>(a.X, a.Dp, Dk, qid_g, idm2, l16, r);
            if (has && !tie) {
#pragma unroll
                for (int t = 0; t < NR; ++t)
                    if (16 * t + l16 < NPM) sQ[w][16 * t + l16][pl] = r[t];
                if (l16 == 0) sN[w][pl] = m;
            }
            if (l16 == 0 && tie) slowmask |= 1ull << pl;
        }
    }
    unsigned long long sm = slowmask;   // classification bits on every lane, tie bits on lanes 0, 16, 32, 48
    sm |= __shfl_xor(sm, 16, 64);
    sm |= __shfl_xor(sm, 32, 64);
    sm = __shfl(sm, 0, 64);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes have landed

    // ---- phase 2: one problem per lane
    {
        const int n = valid ? sN[w][lane] : -1;
        if (valid && n != -1 && !((sm >> lane) & 1ull)) {   // else: distance kept, or written by the exact path
            double Q[NPM];
#pragma unroll
            for (int e = 0; e < NPM; ++e) Q[e] = sQ[w][e][lane];
            double alpha[M];
            double dist;
            if (n <= 0) {
                dist = kInf;
            } else {
                const double val = a.metric == 0 ? min_norm_point<M>(Q, n, alpha) : affine_min_norm<M>(Q, n, alpha);
                dist = sqrt(fmax(val, 0.0));
            }
            a.dist[(size_t)pos * a.B + c] = dist;
        }
    }

    // ---- the exact path's work list: one device-scope atomic per workgroup (at the very end: the barriers
    // below must not hold a wavefront back between its sweeps and its solver)
    const int nsl = __popcll(sm);
    int wbase = 0;
    if (lane == 0 && nsl > 0) wbase = atomicAdd(&sSlowN, nsl);
    __syncthreads();
    if (threadIdx.x == 0) sSlowBase = sSlowN > 0 ? atomicAdd(a.n_slow, sSlowN) : 0;
    // (the trim's three counters, by three lanes at once)
    if (threadIdx.x < 3 && a.trim != nullptr && sTrimCtr[0] > 0)
        atomicAdd(a.trim->ctr + threadIdx.x, (unsigned long long)sTrimCtr[threadIdx.x]);
    __syncthreads();
    wbase = __shfl(wbase, 0, 64) + sSlowBase;
    if (nsl > 0 && ((sm >> lane) & 1ull)) {
        const int before = __popcll(sm & ((1ull << lane) - 1ull));
        a.slow[wbase + before] = (pos - a.pos_begin) * a.B + c;   // (position-major pair index, whatever the work order)
    }
}

// ---------------------------------------------------------------------------------------------
// m > 8 (the reference's function default is num_neighbors = 15, algorithm.py:17): a 16 x 16 Gram and
// the solver's factor do not fit one lane's registers (the per-lane form above spills ~2 KB), so a
// problem is spread over 16 lanes -- lane i owns vertex i, i.e. row i of Q and its weight alpha_i.
//   phase 1: one v_mfma_f64_16x16x4_f64 tile per problem (16 vertices fill it exactly), four problems
//     per wavefront one after the other, Gram rows handed to their lanes through LDS;
//   phase 2: the same Wolfe iteration as min_norm_point<M>, with the reductions (value, entering
//     vertex, ratio test) as 16-lane butterflies and the affine sub-problem solved through an
//     incrementally maintained inverse with one matrix row per lane (see Inv16).
// Groups follow their own control flow (all branches are uniform within a group of 16 lanes).

#ifdef CHB_DEV_CLK
__device__ unsigned long long g_qp16_clk[131072][8];   // per-wavefront cycle stamps of the last launch (no atomics)
#endif
#ifdef CHB_DEV_CLK
#define QP16_CLK(t) const unsigned long long t = __builtin_readcyclecounter()
#define QP16_CLK_ADD(i, v) do { if (lane == 0) atomicAdd(&g_qp16_stats[i], (unsigned long long)(v)); } while (0)
#define QP16_CLK_ACC(var, v) do { var += (unsigned long long)(v); } while (0)
#else
#define QP16_CLK(t) do { } while (0)
#define QP16_CLK_ADD(i, v) do { } while (0)
#define QP16_CLK_ACC(var, v) do { } while (0)
#endif

constexpr int kExtraMax = 2;   // extra rows beside the tile (3 measured the same: 19 candidates are rare enough)
constexpr int kExtraNP = kExtraMax * (kExtraMax + 1) / 2;
// The sweep of the fused kernel for rows of up to 288 doubles: 16 rows plus NE <= kExtraMax EXTRA rows ide[0..NE)
// (the usual shape of a shortlist at m = 15: 17 or 18 candidates).  The matrix core forms the tile of the 16 rows;
// the few products with and between the extra rows are vector FMAs on the lanes' feature slices: ae[b] = <row `row`,
// extra b>, ee[] = <extra b, extra b'> (b' <= b, packed lower-triangular: ee[b (b + 1) / 2 + b']), complete on every
// lane after the reduction over the four feature slices (lanes row, row + 16, row + 32, row + 48).  The query row
// comes from LDS (xs, zero-padded to a multiple of 16 doubles), which leaves the registers to the candidate rows:
// CH features of every row are in flight per round trip (the whole row for NE = 0 and D <= 160).
// features per round trip for 0 / 1 / 2 extra rows (register budget of the kernel: 168 VGPRs)
#ifndef CHB_SW0
#define CHB_SW0 160
#define CHB_SW1 48
#define CHB_SW2 32
#endif
template <int NE, int CH, bool FULL>
__device__ __forceinline__ void gram_sweep16_chunk(const double *vptr, const double *const (&eptr)[kExtraMax],
                                                   const double *xs, int k0, int kq, int Dp, f64x4 &acc,
                                                   double (&ae)[kExtraMax], double (&ee)[kExtraNP])
{
    constexpr int NG = CH / 16;   // 16-feature groups: the lane holds 4 doubles of each row per group
    double2 v[NG][2], e[NE > 0 ? NE : 1][NG][2];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const bool in = FULL || k0 + 16 * g + 4 * kq < Dp;   // Dp % 8 == 0: all 4 in range
        v[g][0] = in ? *reinterpret_cast<const double2 *>(vptr + k0 + 16 * g) : double2{0.0, 0.0};
        v[g][1] = in ? *reinterpret_cast<const double2 *>(vptr + k0 + 16 * g + 2) : double2{0.0, 0.0};
#pragma unroll
        for (int b = 0; b < NE; ++b) {
            e[b][g][0] = in ? *reinterpret_cast<const double2 *>(eptr[b] + k0 + 16 * g) : double2{0.0, 0.0};
            e[b][g][1] = in ? *reinterpret_cast<const double2 *>(eptr[b] + k0 + 16 * g + 2) : double2{0.0, 0.0};
        }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (FULL || k0 + 16 * g < Dp) {   // (wave-uniform)
            const double2 x0 = *reinterpret_cast<const double2 *>(xs + k0 + 16 * g + 4 * kq);
            const double2 x1 = *reinterpret_cast<const double2 *>(xs + k0 + 16 * g + 4 * kq + 2);
            const double y[4] = {v[g][0].x - x0.x, v[g][0].y - x0.y, v[g][1].x - x1.x, v[g][1].y - x1.y};
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(y[t], y[t], acc, 0, 0, 0);
            double z[NE > 0 ? NE : 1][4];
#pragma unroll
            for (int b = 0; b < NE; ++b) {
                z[b][0] = e[b][g][0].x - x0.x; z[b][1] = e[b][g][0].y - x0.y;
                z[b][2] = e[b][g][1].x - x1.x; z[b][3] = e[b][g][1].y - x1.y;
#pragma unroll
                for (int t = 0; t < 4; ++t) ae[b] = fma(y[t], z[b][t], ae[b]);
#pragma unroll
                for (int b2 = 0; b2 <= b; ++b2)
#pragma unroll
                    for (int t = 0; t < 4; ++t) ee[b * (b + 1) / 2 + b2] = fma(z[b][t], z[b2][t], ee[b * (b + 1) / 2 + b2]);
            }
        }
    }
}
// (rows wider than the LDS tile that stages the query row -- round 5 -- are swept in WINDOWS of up to kFusedMaxDp columns:
//  c0 = first column of the window, Dk = its width, xs = the query row's columns c0 .. c0 + Dk; `first` clears the extra-row
//  sums, `last` reduces them.  The one-window call of the narrow rows is the defaults.)
template <int NE, int CH>
__device__ __forceinline__ void gram_sweep16(const double *X, int Dp, int Dk, int q, int idv, const int (&ide)[kExtraMax], int kq,
                                             const double *xs, f64x4 &acc, double (&ae)[kExtraMax],
                                             double (&ee)[kExtraNP], int c0 = 0, bool first = true, bool last = true)
{
    const double *vptr = X + (size_t)(idv >= 0 ? idv : q) * Dp + 4 * kq + c0;   // a missing vertex reads the query row: y = 0
    const double *eptr[kExtraMax];
#pragma unroll
    for (int b = 0; b < kExtraMax; ++b) eptr[b] = X + (size_t)(b < NE ? ide[b] : q) * Dp + 4 * kq + c0;
    if (first) {
#pragma unroll
        for (int b = 0; b < kExtraMax; ++b) ae[b] = 0.0;
#pragma unroll
        for (int e = 0; e < kExtraNP; ++e) ee[e] = 0.0;
    }
    int k0 = 0;
    for (; k0 + CH <= Dk; k0 += CH) gram_sweep16_chunk<NE, CH, true>(vptr, eptr, xs, k0, kq, Dk, acc, ae, ee);
    if (k0 < Dk) gram_sweep16_chunk<NE, CH, false>(vptr, eptr, xs, k0, kq, Dk, acc, ae, ee);
    if (NE > 0 && last) {
        // sum over the four feature slices
#pragma unroll
        for (int b = 0; b < NE; ++b) {
            ae[b] += __shfl_xor(ae[b], 16, 64);
            ae[b] += __shfl_xor(ae[b], 32, 64);
        }
#pragma unroll
        for (int e = 0; e < NE * (NE + 1) / 2; ++e) {
            ee[e] += __shfl_xor(ee[e], 16, 64);
            ee[e] += __shfl_xor(ee[e], 32, 64);
        }
    }
}

// List-based form: the vertex lists are given (a.lists / explicit problems).  Active mode (a.active): the listed
// pairs only, walked grid-stride.
template <bool INDEXED>
__global__ __launch_bounds__(256, CHB_QP16_OCC) void hull_qp16_kernel(QpArgs a, int nprob, const int *xq, const int *xhull,
                                                        const int *xn, int xm, double *xdist, double *xalpha, Gate gate)
{
    CHB_GATE(gate);
    __shared__ __attribute__((aligned(16))) double sQ[4][4][16][kQ16Ld];   // [wavefront][problem][row][col], padded
    __shared__ __attribute__((aligned(16))) double sV[4][4][16];           // exchange row of each 16-lane group
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int grp = lane >> 4, l16 = lane & 15;
    const int m = INDEXED ? xm : a.m;
    const int *act = INDEXED ? nullptr : a.active;
    if (act != nullptr) nprob = *a.n_active;
    for (int gw = (blockIdx.x * 4 + w) * 4; gw < nprob; gw += (int)gridDim.x * 16) {   // wave-uniform
        const int g = gw + grp;   // my group's problem
        const bool valid = g < nprob;
        int n = 0, idm = -1, qid = 0, pr = 0;
        size_t slot = 0;
        if (valid) {
            if (INDEXED) {
                qid = xq[g];
                n = xn[g];
                if (l16 < n) idm = xhull[(size_t)g * m + l16];
            } else {
                pr = act ? act[g] : g;
                const int pos = a.pos_begin + pr / a.B, c = pr - (pr / a.B) * a.B;
                qid = a.bq[pos];
                slot = (size_t)c * a.Kcap + pos;
                n = a.lists.cnt[slot];
                if (l16 < n) idm = a.lists.idx[slot * m + l16];
            }
        }
        bool changed = valid;
        if (!INDEXED && a.prev.idx != nullptr && act == nullptr && valid)
            changed = a.prev.cnt[slot] != n || (l16 < n && a.prev.idx[slot * m + l16] != idm);
        const bool doit = ((__ballot(changed) >> (16 * grp)) & 0xFFFFull) != 0ull;   // else: keep the stored distance

        // ---- phase 1: Gram of the shifted vertices, one matrix-core tile per problem
        const int row = lane & 15, kq = lane >> 4;
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
            const int np = __shfl(n, 16 * p, 64);
            const bool go = __shfl(doit ? 1 : 0, 16 * p, 64) != 0 && np > 0;
            const int id = __shfl(idm, 16 * p + row, 64);
            const int q = __shfl(qid, 16 * p, 64);
            if (!go) continue;   // wave-uniform
            f64x4 acc = {0.0, 0.0, 0.0, 0.0}, d0 = acc, d1 = acc;
            gram_tile16<false>(a.X, a.Dp, (a.D + 7) & ~7, q, id, -1, kq, acc, d0, d1);
#pragma unroll
            for (int r = 0; r < 4; ++r) sQ[w][p][kq + 4 * r][row] = acc[r];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wavefront's LDS writes have landed
        if (!valid || !doit) continue;

        // ---- phase 2: one problem per 16-lane group
        double alpha = 0.0;
        const double val = n <= 0 ? kInf : solve16(&sQ[w][grp][0][0], &sV[w][grp][0], n, a.metric, lane, alpha);
        const double dist = n <= 0 ? kInf : sqrt(fmax(val, 0.0));
        if (INDEXED) {
            if (l16 == 0) xdist[g] = dist;
            if (xalpha && l16 < m) xalpha[(size_t)g * m + l16] = alpha;
        } else if (l16 == 0) {
            const int pos = a.pos_begin + pr / a.B, c = pr - (pr / a.B) * a.B;
            a.dist[(size_t)pos * a.B + c] = dist;
        }
    }
}

// Fused selection + hull distance for 5 < m <= 16 (the same contract as hull_select_qp_kernel: FusedArgs, tie
// rule kTieRel, pairs it does not decide are appended to `slow`).  One (position, bin) pair per 16-lane group.
// A pair's candidates (base shortlist, then the batch's own entries) are read ONCE:
//   n <= 16: one matrix-core tile (Gram of all candidates);
//   17 .. 20 (the usual excess at m = 15): the tile of candidates 0..15 plus the n - 16 extra rows by vector FMAs;
//   21 .. 32: two tiles and the block between them (ranked and scattered inside the sweep loop);
//   n > 32, or a near-tie between ranks m - 1 and m: exact path.
// The diagonal = the squared distances ranks the candidates; the entries between the m nearest become the hull's
// Gram tile (vertex slot = rank).  For n <= 18 that happens after the sweeps, the four pairs of the wavefront
// side by side (16 lanes each: lane i owns candidate i's row of the raw tile and moves it to its slot).
// WIDEROW: the instantiation for rows wider than kFusedMaxDp columns (its window loop would cost the ordinary one 24 spilled
// registers).
template <int WAVES, bool WIDEROW>
__global__ __launch_bounds__(64 * WAVES, CHB_QP16_OCC) void hull_select_qp16_kernel(FusedArgs a, int nprob, Gate gate)
{
    CHB_GATE(gate);
    __shared__ __attribute__((aligned(16))) double sQ[WAVES][4][16][kQ16Ld];
    __shared__ __attribute__((aligned(16))) double sV[WAVES][4][16];
    __shared__ __attribute__((aligned(16))) double sAE[WAVES][4][kExtraMax][16];   // <candidate i, extra b> of each pair
    __shared__ __attribute__((aligned(16))) double sEE[WAVES][4][kExtraNP];        // <extra b, extra b'>
    __shared__ __attribute__((aligned(16))) double sGD[WAVES][4][20];      // squared distances of a pair's candidates
    __shared__ __attribute__((aligned(16))) int sGI[WAVES][4][20];         // their sample indices
    __shared__ __attribute__((aligned(16))) int sGN[WAVES][4][20];         // their vertex slots (-1: not selected)
    __shared__ double sTh[WAVES][4][2];   // squared distances of ranks m - 1 and m
    __shared__ int sSlowN, sSlowBase;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int grp = lane >> 4, l16 = lane & 15;
    const int m = a.m;
    const int Dk = (a.D + 7) & ~7;   // columns swept (the rows are padded to whole 128-byte lines beyond)
    // rows wider than the tile that stages a pair's query row (kFusedMaxDp = 288 doubles; wide feature vectors, round 5):
    // the sweep of a pair then runs in windows of 288 columns, all 64 lanes staging each window's piece of the query row
    constexpr bool widerow = WIDEROW;   // (the launcher: Dk > kFusedMaxDp)
    // the two-tile form works on one pair at a time inside the sweep loop and borrows the wavefront's group arrays
    // (32 of the 80 entries each), which the groups only use after the loop
    double *sDw = &sGD[w][0][0];
    int *sIdw = &sGI[w][0][0], *sNeww = &sGN[w][0][0];
    if (threadIdx.x == 0) sSlowN = 0;
    __syncthreads();
    // (a.stripe: the work order of the m <= 5 kernel -- workgroup b only takes pairs of the bins c = b (mod 8), so that an
    //  XCD gathers candidate rows of an eighth of the bins; the wavefront's four pairs are four of those bins at one
    //  position while the XCD has that many.  nprob is then the length of the longest of the 8 lists)
    const int gw = ((a.stripe ? (int)(blockIdx.x >> 3) : (int)blockIdx.x) * WAVES + w) * 4;
    int pos = 0, c = 0;
    const bool valid = fused_pair_of(a, gw, grp, nprob, pos, c);
    int nb = 0, nu = 0, qid = 0;
    bool changed = valid;
    const size_t slot = (size_t)c * a.Kcap + pos;
    if (valid) {
        qid = a.bq[pos];
        nb = a.cand_cnt[slot];
        if (a.candu != nullptr) nu = a.candu_cnt[slot];
        // unchanged set of batch-entry candidates (the base candidates are fixed during a batch): keep the distance
        if (a.candp != nullptr && a.candp_cnt[slot] == nu) {
            bool same = true;
            for (int i = l16; i < nu; i += 16) {
                const int u = a.candu[slot * kCandCapU + i];
                bool f = false;
                for (int j = 0; j < nu; ++j) f = f || a.candp[slot * kCandCapU + j] == u;
                same = same && f;
            }
            changed = ((__ballot(!same) >> (lane & 48)) & 0xFFFFull) != 0ull;
        }
    }
    if (a.short_cnt != nullptr && valid && l16 == 0 &&
        nb < min(m, a.bin_size != nullptr ? a.bin_size[c] : a.bin_ptr[c + 1] - a.bin_ptr[c]))
        atomicAdd(a.short_cnt, 1);   // (the shortlist stage's contract, see FusedArgs)
    QP16_CLK(tc0);
#ifdef CHB_DEV_CLK
    unsigned long long c_ids = 0, c_sweep = 0, c_one = 0;
#endif
    const int n = nb + nu;
    const bool work = changed && n > 0 && n <= 32;
    bool slow = changed && n > 32;
    int nsel = n < m ? n : m;   // vertices of the hull problem

    // ---- before the sweeps, every group for its own pair (one round trip for the four pairs): the candidates'
    // sample indices (lane i: candidate i; lanes 0 .. kExtraMax - 1 also the extra candidates 16 + i) and the query
    // row, which goes through LDS -- the pair's own tile is free until its sweep ends and holds rows of up to
    // kFusedMaxDp doubles (the caller checks; the shortlist stage itself needs D <= 160)
    int idm = -1, idx = -1;
    if (work) {
        if (l16 < n) idm = l16 < nb ? a.cand[slot * kCandCap + l16] : a.candu[slot * kCandCapU + (l16 - nb)];
        if (l16 < kExtraMax && 16 + l16 < n)
            idx = 16 + l16 < nb ? a.cand[slot * kCandCap + 16 + l16] : a.candu[slot * kCandCapU + (16 + l16 - nb)];
        if (((unsigned)idm >= (unsigned)a.n_samples && idm != -1) || ((unsigned)idx >= (unsigned)a.n_samples && idx != -1)) {
            if (a.short_cnt != nullptr) atomicAdd(a.short_cnt, 1);   // never a row address from a wild index
            if ((unsigned)idm >= (unsigned)a.n_samples) idm = -1;
            if ((unsigned)idx >= (unsigned)a.n_samples) idx = -1;
        }
        if (!widerow) {
            double *xq = &sQ[w][grp][0][0];
            const int Dp16 = (Dk + 15) & ~15;
            for (int e = 2 * l16; e < Dp16; e += 32)
                *reinterpret_cast<double2 *>(xq + e) =
                    e < Dk ? *reinterpret_cast<const double2 *>(a.X + (size_t)qid * a.Dp + e) : double2{0.0, 0.0};
        }
    }
    __builtin_amdgcn_wave_barrier();

    // ---- phase 1: the wavefront's four pairs one after the other, all 64 lanes on one pair
    const int row = lane & 15, kq = lane >> 4;
#pragma unroll 1
    for (int p = 0; p < 4; ++p) {
        const int np = __shfl(n, 16 * p, 64);
        const int nbp = __shfl(nb, 16 * p, 64);
        const int q = __shfl(qid, 16 * p, 64);
        const bool go = __shfl(work ? 1 : 0, 16 * p, 64) != 0;
        const int idA = __shfl(idm, 16 * p + row, 64);
        int ide[kExtraMax];
#pragma unroll
        for (int b = 0; b < kExtraMax; ++b) ide[b] = __shfl(idx, 16 * p + b, 64);
        if (!go) continue;   // wave-uniform
        QP16_CLK(tp0);
        const size_t slot_p = (size_t)__shfl(c, 16 * p, 64) * a.Kcap + (size_t)__shfl(pos, 16 * p, 64);
        const bool two = np > 16 + kExtraMax;
        const int ne = (np > 16 && !two) ? np - 16 : 0;
        int idB = -1;
        double *Qp = &sQ[w][p][0][0];
        if (!two) {
            f64x4 aa = {0.0, 0.0, 0.0, 0.0};
            double ae[kExtraMax], ee[kExtraNP];
            QP16_CLK(tp1);
            QP16_CLK_ACC(c_ids, tp1 - tp0);
            if (!widerow) {
                if (ne == 0) gram_sweep16<0, CHB_SW0>(a.X, a.Dp, Dk, q, idA, ide, kq, Qp, aa, ae, ee);
                else if (ne == 1) gram_sweep16<1, CHB_SW1>(a.X, a.Dp, Dk, q, idA, ide, kq, Qp, aa, ae, ee);
                else gram_sweep16<2, CHB_SW2>(a.X, a.Dp, Dk, q, idA, ide, kq, Qp, aa, ae, ee);
            } else {
#pragma unroll 1
                for (int c0 = 0; c0 < Dk; c0 += kFusedMaxDp) {
                    const int cw = min(kFusedMaxDp, Dk - c0), cw16 = (cw + 15) & ~15;
                    __builtin_amdgcn_wave_barrier();   // (the previous window's reads of the tile are issued: LDS keeps a wavefront's order)
                    for (int e = 2 * lane; e < cw16; e += 128)
                        *reinterpret_cast<double2 *>(Qp + e) =
                            e < cw ? *reinterpret_cast<const double2 *>(a.X + (size_t)q * a.Dp + c0 + e) : double2{0.0, 0.0};
                    __builtin_amdgcn_wave_barrier();
                    const bool fst = c0 == 0, lst = c0 + kFusedMaxDp >= Dk;
                    if (ne == 0) gram_sweep16<0, CHB_SW1>(a.X, a.Dp, cw, q, idA, ide, kq, Qp, aa, ae, ee, c0, fst, lst);
                    else if (ne == 1) gram_sweep16<1, CHB_SW1>(a.X, a.Dp, cw, q, idA, ide, kq, Qp, aa, ae, ee, c0, fst, lst);
                    else gram_sweep16<2, CHB_SW2>(a.X, a.Dp, cw, q, idA, ide, kq, Qp, aa, ae, ee, c0, fst, lst);
                }
            }
            if (ne > 0) {
                if (kq == 0) {
#pragma unroll
                    for (int b = 0; b < kExtraMax; ++b) sAE[w][p][b][row] = ae[b];
                }
                if (lane == 0) {
#pragma unroll
                    for (int e = 0; e < kExtraNP; ++e) sEE[w][p][e] = ee[e];
                }
            }
            // the raw tile of candidates 0..15; selection (np > m) follows after the loop
#pragma unroll
            for (int r = 0; r < 4; ++r) Qp[(kq + 4 * r) * kQ16Ld + row] = aa[r];
            {
                QP16_CLK(tp2);
                QP16_CLK_ACC(c_sweep, tp2 - tp1);
                QP16_CLK_ACC(c_one, 1);
            }
            continue;
        }
        // ---- two tiles (up to 32 candidates): rank and scatter here, the accumulators are this pair's
        if (16 + row < np)
            idB = 16 + row < nbp ? a.cand[slot_p * kCandCap + 16 + row] : a.candu[slot_p * kCandCapU + (16 + row - nbp)];
        if ((unsigned)idB >= (unsigned)a.n_samples && idB != -1) {   // never a row address from a wild index
            if (a.short_cnt != nullptr) atomicAdd(a.short_cnt, 1);
            idB = -1;
        }
        f64x4 aa = {0.0, 0.0, 0.0, 0.0}, ab = aa, bb = aa;
        gram_tile16<true>(a.X, a.Dp, Dk, q, idA, idB, kq, aa, ab, bb);
        // squared distances = the diagonals (lane (row, kq = row & 3) holds D[row][row] in acc[row >> 2])
        if ((row & 3) == kq) {
            const int rr = row >> 2;
            const double dA = rr == 0 ? aa[0] : rr == 1 ? aa[1] : rr == 2 ? aa[2] : aa[3];
            const double dB = rr == 0 ? bb[0] : rr == 1 ? bb[1] : rr == 2 ? bb[2] : bb[3];
            sDw[row] = dA; sIdw[row] = idA;
            sDw[16 + row] = dB; sIdw[16 + row] = idB;
        }
        __builtin_amdgcn_wave_barrier();
        // rank of candidate lane & 31 by (squared distance, index): each half of the wavefront scans 16 entries
        {
            const int cI = lane & 31, u0 = (lane >> 5) * 16;
            const double dc = cI < np ? sDw[cI] : kInf;
            const int ic = sIdw[cI];
            int rank = 0;
#pragma unroll
            for (int t = 0; t < 16; t += 2) {
                const int u = u0 + t;
                const double2 dd = *reinterpret_cast<const double2 *>(&sDw[u]);
                const int2 ii = *reinterpret_cast<const int2 *>(&sIdw[u]);
                rank += (u < np && u != cI && (dd.x < dc || (dd.x == dc && ii.x < ic))) ? 1 : 0;
                rank += (u + 1 < np && u + 1 != cI && (dd.y < dc || (dd.y == dc && ii.y < ic))) ? 1 : 0;
            }
            rank += __shfl_xor(rank, 32, 64);
            if (lane < 32) {
                sNeww[cI] = (cI < np && rank < m) ? rank : -1;
                if (cI < np && rank == m - 1) sTh[w][p][0] = dc;
                if (cI < np && rank == m) sTh[w][p][1] = dc;
            }
        }
        __builtin_amdgcn_wave_barrier();
        const double t0 = sTh[w][p][0], t1 = sTh[w][p][1];
        const bool tie = !(t1 - t0 > kTieRel * t1);   // (also catches NaN)
        if (tie) {
            if (grp == p) slow = true;
            continue;
        }
        // exactly m candidates are selected: the scatter below writes every entry between vertex slots < m once;
        // rows / columns m .. 15 of the tile are cleared (the solver multiplies them by zero weights)
        for (int v = m; v < 16; ++v)
            if (lane < 16) { Qp[v * kQ16Ld + lane] = 0.0; Qp[lane * kQ16Ld + v] = 0.0; }
        const int njA = sNeww[row], njB = sNeww[16 + row];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int niA = sNeww[kq + 4 * r], niB = sNeww[16 + kq + 4 * r];
            if (niA >= 0 && njA >= 0) Qp[niA * kQ16Ld + njA] = aa[r];
            if (niA >= 0 && njB >= 0) { Qp[niA * kQ16Ld + njB] = ab[r]; Qp[njB * kQ16Ld + niA] = ab[r]; }
            if (niB >= 0 && njB >= 0) Qp[niB * kQ16Ld + njB] = bb[r];
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wavefront's LDS writes have landed

    QP16_CLK(tc1);
    // ---- selection for m < n <= 18, one pair per 16-lane group: lane i owns candidate i (and, i < n - 16, extra i)
    if (work && n > m && n <= 16 + kExtraMax) {
        double *Qt = &sQ[w][grp][0][0];
        const int ne = n > 16 ? n - 16 : 0, nA = n - ne;
        const int ide = l16 < ne ? idx : -1;
        if (l16 >= nA) idm = -1;
        const double dA = l16 < nA ? Qt[l16 * kQ16Ld + l16] : kInf;
        const double dE = l16 < ne ? sEE[w][grp][l16 * (l16 + 1) / 2 + l16] : kInf;
        sGD[w][grp][l16] = dA; sGI[w][grp][l16] = idm;
        if (l16 < 4) { sGD[w][grp][16 + l16] = dE; sGI[w][grp][16 + l16] = ide; }   // (+inf / -1 beyond the extras)
        __builtin_amdgcn_wave_barrier();
        int rA = 0, rE = 0;
#pragma unroll
        for (int u = 0; u < 20; u += 2) {
            const double2 dd = *reinterpret_cast<const double2 *>(&sGD[w][grp][u]);
            const int2 ii = *reinterpret_cast<const int2 *>(&sGI[w][grp][u]);
            // (absent candidates carry +inf: they never precede a real one)
            rA += (u != l16 && (dd.x < dA || (dd.x == dA && ii.x < idm))) ? 1 : 0;
            rA += (u + 1 != l16 && (dd.y < dA || (dd.y == dA && ii.y < idm))) ? 1 : 0;
            rE += (u != 16 + l16 && (dd.x < dE || (dd.x == dE && ii.x < ide))) ? 1 : 0;
            rE += (u + 1 != 16 + l16 && (dd.y < dE || (dd.y == dE && ii.y < ide))) ? 1 : 0;
        }
        const int newA = (l16 < nA && rA < m) ? rA : -1;
        const int newE = (l16 < ne && rE < m) ? rE : -1;
        sGN[w][grp][l16] = newA;
        if (l16 < 4) sGN[w][grp][16 + l16] = newE;
        if (l16 < nA && rA == m - 1) sTh[w][grp][0] = dA;
        if (l16 < nA && rA == m) sTh[w][grp][1] = dA;
        if (l16 < ne && rE == m - 1) sTh[w][grp][0] = dE;
        if (l16 < ne && rE == m) sTh[w][grp][1] = dE;
        // my candidate's row of the raw tile, its products with the extras, and (extra lanes) the extras' own block
        double Qr[16], qe[kExtraMax], qx[kExtraMax];
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
            const double2 t = *reinterpret_cast<const double2 *>(Qt + l16 * kQ16Ld + j);
            Qr[j] = t.x; Qr[j + 1] = t.y;
        }
#pragma unroll
        for (int b = 0; b < kExtraMax; ++b) {
            qe[b] = sAE[w][grp][b][l16];
            const int hi = min(max(l16, b), kExtraMax - 1), lo = min(l16, b);
            qx[b] = sEE[w][grp][hi * (hi + 1) / 2 + lo];   // <extra l16, extra b> (used by lanes < ne)
        }
        __builtin_amdgcn_wave_barrier();
        const double t0 = sTh[w][grp][0], t1 = sTh[w][grp][1];
        if (!(t1 - t0 > kTieRel * t1)) {   // near-tie at the selection boundary (also catches NaN)
            slow = true;
        } else {
            int nj[20];
#pragma unroll
            for (int u = 0; u < 20; u += 4) {
                const int4 t = *reinterpret_cast<const int4 *>(&sGN[w][grp][u]);
                nj[u] = t.x; nj[u + 1] = t.y; nj[u + 2] = t.z; nj[u + 3] = t.w;
            }
            // rows / columns m .. 15 of the tile are cleared (the solver multiplies them by zero weights)
            for (int v = m; v < 16; ++v) { Qt[v * kQ16Ld + l16] = 0.0; Qt[l16 * kQ16Ld + v] = 0.0; }
            if (newA >= 0) {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (nj[j] >= 0) Qt[newA * kQ16Ld + nj[j]] = Qr[j];
#pragma unroll
                for (int b = 0; b < kExtraMax; ++b)
                    if (b < ne && nj[16 + b] >= 0) {
                        Qt[newA * kQ16Ld + nj[16 + b]] = qe[b];
                        Qt[nj[16 + b] * kQ16Ld + newA] = qe[b];
                    }
            }
            if (newE >= 0) {
#pragma unroll
                for (int b = 0; b < kExtraMax; ++b)
                    if (b < ne && nj[16 + b] >= 0) Qt[newE * kQ16Ld + nj[16 + b]] = qx[b];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }

    QP16_CLK(tc2);
    // ---- phase 2: one pair per 16-lane group
    if (valid && changed && !slow) {   // else: distance kept, or written by the exact path
        double alpha = 0.0;
        double dist = kInf;
        if (n > 0) dist = sqrt(fmax(solve16(&sQ[w][grp][0][0], &sV[w][grp][0], nsel, a.metric, lane, alpha), 0.0));
        if (l16 == 0) a.dist[(size_t)pos * a.B + c] = dist;
    }
    QP16_CLK(tc3);

    // ---- the exact path's work list: one device-scope atomic per workgroup (at the very end: the barriers
    // below must not hold a wavefront back between its sweeps and its solver)
    {
        const unsigned long long bal = __ballot(slow && l16 == 0);
        const int nsl = __popcll(bal);
        int wbase = 0;
        if (lane == 0 && nsl > 0) wbase = atomicAdd(&sSlowN, nsl);
        __syncthreads();
        if (threadIdx.x == 0) sSlowBase = sSlowN > 0 ? atomicAdd(a.n_slow, sSlowN) : 0;
        __syncthreads();
        wbase = __shfl(wbase, 0, 64) + sSlowBase;
        if (slow && l16 == 0)   // (position-major pair index, whatever the work order)
            a.slow[wbase + __popcll(bal & ((1ull << lane) - 1ull))] = (pos - a.pos_begin) * a.B + c;
    }
#ifdef CHB_DEV_CLK
    {
        const unsigned wid = blockIdx.x * WAVES + w;
        if (lane == 0 && wid < 131072u) {
            unsigned long long *o = g_qp16_clk[wid];
            o[0] = tc1 - tc0; o[1] = tc2 - tc1; o[2] = tc3 - tc2; o[3] = c_ids; o[4] = c_sweep; o[5] = c_one; o[6] = 1; o[7] = tc0;
        }
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// num_neighbors > 16 (no cap in the reference: algorithm.py:17, cli/clustering.py:118-120): the plain form,
// ONE wavefront per problem, up to 64 vertices.  Lane i owns vertex i: row i of the shifted Gram Q and of the
// inverse H of the lifted support Gram (both in LDS, [64][65] doubles) and its weight alpha_i.  The iteration is
// active_set_distance2 (above, shared with the 16-lane kernels) on the Wave64 backend: the same bordering / Schur
// updates as Inv16, with loops over the vertex count and LDS rows where that has 16-entry register arrays and DPP
// reductions.  Slow by design.
// The backend and its LDS layout live in hull_solve64.h (shared with recruit_wide_kernels.hip); here at its full capacity.
constexpr int kGenN = 64;
using GenLds = GenLdsT<kGenN>;
using Wave64 = Wave64T<kGenN>;

template <bool INDEXED>
__global__ __launch_bounds__(64) void hull_generic_kernel(QpArgs a, int nprob, const int *xq, const int *xhull,
                                                        const int *xn, int xm, double *xdist, double *xalpha, Gate gate)
{
    CHB_GATE(gate);
    extern __shared__ __attribute__((aligned(16))) unsigned char gen_smem[];
    GenLds &L = *reinterpret_cast<GenLds *>(gen_smem);
    const int lane = threadIdx.x;
    const int g = blockIdx.x;
    if (g >= nprob) return;
    const int m = INDEXED ? xm : a.m;
    int n = 0, id = -1, qid = 0, pos = 0, c = 0;
    if (INDEXED) {
        qid = xq[g];
        n = xn[g];
        if (lane < n) id = xhull[(size_t)g * m + lane];
    } else {
        pos = a.pos_begin + g / a.B; c = g - (g / a.B) * a.B;
        qid = a.bq[pos];
        const size_t slot = (size_t)c * a.Kcap + pos;
        n = a.lists.cnt[slot];
        if (lane < n) id = a.lists.idx[slot * m + lane];
        if (a.prev.idx != nullptr) {   // unchanged vertex list: keep the stored distance
            const bool changed = a.prev.cnt[slot] != n || (lane < n && a.prev.idx[slot * m + lane] != id);
            if (__ballot(changed) == 0ull) return;
        }
    }
    const bool mine = lane < n;
    double alpha = 0.0, val = kInf;
    if (n > 0) {
        // ---- shifted Gram: lane i computes row i (its own row against every vertex j <= i, mirrored)
        const double *xrow = a.X + (size_t)qid * a.Dp;
        const double *vi = a.X + (size_t)(mine ? id : qid) * a.Dp;
        for (int j = 0; j < n; ++j) {
            const int idj = __shfl(id, j, 64);
            const double *vj = a.X + (size_t)idj * a.Dp;
            double acc = 0.0;
            for (int k = 0; k < a.Dp; ++k) {
                const double xk = xrow[k];
                acc = fma(vi[k] - xk, vj[k] - xk, acc);
            }
            if (mine) L.Q[lane][j] = acc;
        }
        for (int j = 0; j < kGenN; ++j) L.H[lane][j] = 0.0;
        gen_sync();
        const double diag = mine ? L.Q[lane][lane] : 0.0;
        double scale = diag;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) scale = fmax(scale, __shfl_xor(scale, off, 64));
        Wave64 g{L, n, scale, diag, lane, mine, 0ull};   // (handed over reset: H was zeroed above)
        val = active_set_distance2(g, n, a.metric, scale, alpha);
    }
    const double dist = n <= 0 ? kInf : sqrt(fmax(val, 0.0));
    if (INDEXED) {
        if (lane == 0) xdist[g] = dist;
        if (xalpha && lane < m) xalpha[(size_t)g * m + lane] = alpha;
    } else if (lane == 0) {
        a.dist[(size_t)pos * a.B + c] = dist;
    }
}

template <bool INDEXED>
void launch_generic(const QpArgs &a, int nprob, int m, const int *xq, const int *xhull, const int *xn, double *xdist,
                    double *xalpha, hipStream_t s)
{
    if (nprob <= 0) return;
    // per launch (cheap, and the attribute is per device: a process may hold contexts on several); whether the
    // device grants it at all is asked up front by hull_generic_supported()
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(hull_generic_kernel<INDEXED>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GenLds));
    hipLaunchKernelGGL((hull_generic_kernel<INDEXED>), dim3(nprob), dim3(64), sizeof(GenLds), s, a, nprob, xq, xhull, xn, m,
                       xdist, xalpha, g_gate);
}

template <int M, int WV, bool INDEXED>
void launch_one(const QpArgs &a, int nprob, int m, const int *xq, const int *xhull, const int *xn,
                double *xdist, double *xalpha, hipStream_t s)
{
    constexpr int PPW = 64;
    const int nwaves = (nprob + PPW - 1) / PPW;
    int grid = (nwaves + WV - 1) / WV;
    if (!INDEXED && a.active != nullptr) grid = std::min(16 * grid, 1024);   // listed pairs: grid-stride, 4 per wavefront
    hipLaunchKernelGGL((hull_qp_kernel<M, WV, INDEXED>), dim3(grid), dim3(64 * WV), 0, s, a, nprob,
                       xq, xhull, xn, m, xdist, xalpha, g_gate);
}

template <bool INDEXED>
void dispatch(const QpArgs &a, int nprob, int m, const int *xq, const int *xhull, const int *xn,
              double *xdist, double *xalpha, hipStream_t s)
{
    if (nprob <= 0) return;
    if (m <= 4) launch_one<4, 4, INDEXED>(a, nprob, m, xq, xhull, xn, xdist, xalpha, s);
    else if (m <= 5) launch_one<5, 4, INDEXED>(a, nprob, m, xq, xhull, xn, xdist, xalpha, s);
    else if (m <= 8) launch_one<8, 2, INDEXED>(a, nprob, m, xq, xhull, xn, xdist, xalpha, s);
    else
    {
        int grid = (nprob + 15) / 16;
        if (!INDEXED && a.active != nullptr) grid = std::min(grid, 1024);   // listed pairs (device-side count): grid-stride
        hipLaunchKernelGGL((hull_qp16_kernel<INDEXED>), dim3(grid), dim3(256), 0, s, a, nprob, xq, xhull,
                           xn, m, xdist, xalpha, g_gate);
    }
}

// Self-check of the 16-lane exchanges of hull_solve16.h (the counter "lane_exchange_mismatches"): one workgroup of 256
// threads compares every helper, on ints and on doubles, bit for bit with the shuffle it stands for, and the DPP
// reduce_scatter16 with the shuffle form, and adds the mismatches it sees to *bad.  The values differ from lane to lane
// and from round to round; the doubles run through NaNs with payloads (quiet and signalling), -0.0, denormals of both
// signs, infinities and ordinary numbers from 2^-40 to 2^40.  Every exchange stands outside any condition.
__device__ __forceinline__ unsigned lane_check_hash(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ double lane_check_double(unsigned tid, unsigned round)
{
    const unsigned h = lane_check_hash(tid * 977u + round * 131071u + 12345u);
    const unsigned long long payload = ((unsigned long long)lane_check_hash(h) << 20) ^ h;   // < 2^52
    const double mixed = ldexp((double)((int)(h % 2001u) - 1000), (int)((h >> 11) % 81u) - 40);
    switch ((tid * 7u + round * 3u) & 7u) {
    case 0: return __longlong_as_double((long long)(0x7FF8000000000000ull | (payload & 0x0007FFFFFFFFFFFFull)));   // quiet NaN
    case 1: return __longlong_as_double((long long)(0xFFF0000000000000ull | (payload & 0x0007FFFFFFFFFFFFull) | 1ull));   // signalling NaN, sign set
    case 2: return -0.0;
    case 3: return __longlong_as_double((long long)((payload & 0x000FFFFFFFFFFFFFull) | 1ull));   // denormal
    case 4: return __longlong_as_double((long long)(0x8000000000000000ull | (payload >> 30) | 1ull));   // tiny negative denormal
    case 5: return (h & 1u) ? kInf : -kInf;
    default: return mixed;
    }
}
__global__ __launch_bounds__(256) void lane_exchange_check_kernel(int *bad)
{
    const unsigned tid = threadIdx.x;
    const int lane = (int)(tid & 63u), l16 = lane & 15, gbase = lane & 48;
    int miss = 0;
    auto differ = [](double x, double y) { return __double_as_longlong(x) != __double_as_longlong(y) ? 1 : 0; };
    for (unsigned round = 0; round < 8u; ++round) {
        const int xi = (int)lane_check_hash(tid * 2654435761u + round);
        const double xd = lane_check_double(tid, round);
        miss += row_xor_i32<1>(xi) != __shfl_xor(xi, 1, 64) ? 1 : 0;
        miss += row_xor_i32<2>(xi) != __shfl_xor(xi, 2, 64) ? 1 : 0;
        miss += row_xor_i32<4>(xi) != __shfl_xor(xi, 4, 64) ? 1 : 0;
        miss += row_xor_i32<8>(xi) != __shfl_xor(xi, 8, 64) ? 1 : 0;
        miss += differ(row_xor_f64<1>(xd), __shfl_xor(xd, 1, 64));
        miss += differ(row_xor_f64<2>(xd), __shfl_xor(xd, 2, 64));
        miss += differ(row_xor_f64<4>(xd), __shfl_xor(xd, 4, 64));
        miss += differ(row_xor_f64<8>(xd), __shfl_xor(xd, 8, 64));
        for_row_lanes<16>([&](auto lv) {
            constexpr int v = decltype(lv)::value;
            miss += row_bcast_i32<v>(xi) != __shfl(xi, gbase + v, 64) ? 1 : 0;
            miss += differ(row_bcast_f64<v>(xd), __shfl(xd, gbase + v, 64));
        });
        // sixteen sums of mixed magnitude per lane: both forms add the same pairs in the same order
        double v16[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const unsigned h = lane_check_hash((tid * 16u + (unsigned)e) * 2246822519u + round * 40503u);
            v16[e] = ldexp((double)((int)(h % 2001u) - 1000), (int)((h >> 11) % 81u) - 40);
        }
        miss += differ(reduce_scatter16(v16, l16), reduce_scatter16_shfl(v16, l16));
    }
    if (miss != 0) atomicAdd(bad, miss);
}

}  // namespace

void launch_lane_exchange_check(int *bad, hipStream_t s)
{
    hipLaunchKernelGGL(lane_exchange_check_kernel, dim3(1), dim3(256), 0, s, bad);
}

void launch_hull_qp(const QpArgs &a, hipStream_t s)
{
    const int nprob = (a.pos_end - a.pos_begin) * a.B;
    dispatch<false>(a, nprob, a.m, nullptr, nullptr, nullptr, nullptr, nullptr, s);
}

// (rows of any width: the m <= 5 kernel sweeps them from registers, the 16-lane kernel stages the query row in LDS in
//  windows of kFusedMaxDp columns)
bool fused_supported(int m, int Dp) { (void)Dp; return m >= 1 && m <= 16; }

void launch_hull_select_qp(const FusedArgs &a, bool stripe, bool ptr64, hipStream_t s)
{
    const int nprob = (a.pos_end - a.pos_begin) * a.B;
    if (nprob <= 0) return;
    constexpr int WV = 4;
    FusedArgs as = a;
    as.stripe = (stripe && a.B >= 16) ? 1 : 0;
    if (a.m > 5) {   // 16 lanes per pair, four pairs per wavefront
        int np16 = nprob, grid16 = (nprob + 4 * WV - 1) / (4 * WV);
        if (as.stripe) {
            np16 = (a.pos_end - a.pos_begin) * ((a.B + 7) / 8);
            grid16 = 8 * ((np16 + 4 * WV - 1) / (4 * WV));
        }
        if (((a.D + 7) & ~7) > kFusedMaxDp)
            hipLaunchKernelGGL((hull_select_qp16_kernel<WV, true>), dim3(grid16), dim3(64 * WV), 0, s, as, np16, g_gate);
        else
            hipLaunchKernelGGL((hull_select_qp16_kernel<WV, false>), dim3(grid16), dim3(64 * WV), 0, s, as, np16, g_gate);
        return;
    }
    int np5 = nprob, grid = (nprob + 64 * WV - 1) / (64 * WV);
    if (as.stripe) {
        // the longest of the 8 XCD lists: XCD 0 has ceil(B / 8) bins
        np5 = (a.pos_end - a.pos_begin) * ((a.B + 7) / 8);
        grid = 8 * ((np5 + 64 * WV - 1) / (64 * WV));
    }
    // (rows as 32-bit byte offsets while the sample matrix is smaller than 4 GiB: see gram_rows; ptr64 -- CHB_FUSED_PTR64=1 --
    //  selects the 64-bit-pointer instantiation regardless, for the tests)
    if (!ptr64 && (unsigned long long)a.n_samples * (unsigned long long)a.Dp * 8ull < (1ull << 32))
        hipLaunchKernelGGL((hull_select_qp_kernel<5, CHB_FUSED_C, WV, true>), dim3(grid), dim3(64 * WV), 0, s, as, np5, g_gate);
    else
        hipLaunchKernelGGL((hull_select_qp_kernel<5, CHB_FUSED_C, WV, false>), dim3(grid), dim3(64 * WV), 0, s, as, np5, g_gate);
}

bool hull_generic_supported()
{
    const hipError_t e0 = hipFuncSetAttribute(reinterpret_cast<const void *>(hull_generic_kernel<false>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GenLds));
    const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void *>(hull_generic_kernel<true>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GenLds));
    if (e0 != hipSuccess || e1 != hipSuccess) { (void)hipGetLastError(); return false; }
    return true;
}

void launch_hull_generic(const QpArgs &a, hipStream_t s)
{
    launch_generic<false>(a, (a.pos_end - a.pos_begin) * a.B, a.m, nullptr, nullptr, nullptr, nullptr, nullptr, s);
}

void launch_hull_generic_indexed(const double *X, int D, int Dp, const int *q, const int *hull_idx,
                                 const int *hull_cnt, int P, int m_max, int metric, double *dist,
                                 double *alpha, hipStream_t s)
{
    QpArgs a{};
    a.X = X; a.D = D; a.Dp = Dp; a.m = m_max; a.metric = metric;
    launch_generic<true>(a, P, m_max, q, hull_idx, hull_cnt, dist, alpha, s);
}

void launch_hull_qp_indexed(const double *X, int D, int Dp, const int *q, const int *hull_idx,
                            const int *hull_cnt, int P, int m_max, int metric, double *dist,
                            double *alpha, hipStream_t s)
{
    QpArgs a{};
    a.X = X; a.D = D; a.Dp = Dp; a.m = m_max; a.metric = metric;
    dispatch<true>(a, P, m_max, q, hull_idx, hull_cnt, dist, alpha, s);
}

}  // namespace chb

#if defined(CHB_DEV_QP16_STAT) || defined(CHB_DEV_CLK)
// developer variants only: [0] problems solved, [1] major iterations, [2] ratio-test removals, [3] final support
// sizes (sum), [4] small-pivot refinements of inv16_insert
#ifdef CHB_DEV_CLK
// sums of the per-wavefront stamps of the last launch: [0] sweeps [1] selection [2] slow list + solver [3] id loads
// [4] one-tile sweeps [5] one-tile pairs [6] wavefronts [7] span (last start - first start)
extern "C" int chb_dev_qp16_clk(unsigned long long *out8)
{
    std::vector<unsigned long long> h(131072 * 8);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(chb::g_qp16_clk), h.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
    for (int k = 0; k < 8; ++k) out8[k] = 0;
    unsigned long long lo = ~0ull, hi = 0;
    for (size_t i = 0; i < 131072; ++i) {
        if (!h[i * 8 + 6]) continue;
        for (int k = 0; k < 7; ++k) out8[k] += h[i * 8 + k];
        lo = std::min(lo, h[i * 8 + 7]); hi = std::max(hi, h[i * 8 + 7]);
    }
    out8[7] = hi > lo ? hi - lo : 0;
    const std::vector<unsigned long long> z(131072 * 8, 0ull);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(chb::g_qp16_clk), z.data(), z.size() * sizeof(unsigned long long));
    return 0;
}
#endif
extern "C" int chb_dev_qp16_stats(unsigned long long *out, int reset)
{
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(chb::g_qp16_stats), 16 * sizeof(unsigned long long)) != hipSuccess)
        return -1;
    if (reset) {
        const unsigned long long z[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(chb::g_qp16_stats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
