// Row scoring for 16 < m <= 64 on gfx950 (chb_audit_rows_wide, chb_recruit_rows_wide, chb_*_pairs_wide): what
// recruit_kernel (recruit_kernels.hip) does in one kernel for m <= 16, in two per chunk.
//
// (a) recruit_select_wide_kernel: recruit_kernel's tile loop -- 256 threads own (64 rows) x (one bin) or one tile of at
//     most 64 pairs, the bin's members are streamed in tiles of 64 rows through double-buffered LDS k-chunks, a 4 x 4 fp64
//     micro-tile per thread, work items in XCD-aware order -- with the row's sorted list in four 16-entry slabs
//     (topm_select_wide.h) instead of one.  It withholds the row itself (kResident) and its group (kGrouped) and writes,
//     per (position, bin) or per pair, the list's length and its m sample ids (-1 padded) to a.list: m + 1 int32 per
//     problem.  Nothing else comes out of it; it needs no scratch.
// (b) hull_wide_kernel<NV>, NV = 32 (m <= 32) or 64: one wavefront per problem.  The Gram matrix of the shifted vertices
//     comes from the fp64 matrix core: lane (row, kq) supplies row `row` of every 16-vertex block, only the lower-triangle
//     tiles of the (NV / 16)^2 grid are computed and then mirrored into LDS, every vertex row and the query row are read
//     once in 16-byte loads, a missing vertex reads the query row (y = 0).  Then active_set_distance2 on the Wave64
//     backend (hull_solve64.h), the driver and backend of hull_generic_kernel.
// The list form of (b) (chb_*_rows_multi_wide, dense only) reads the lists (a) left for the list's largest entry: one
// wavefront per (problem, entry of the launch) -- the entries in 17 .. 32 with NV = 32, those in 33 .. 64 with NV = 64 --
// on the first m' ids of the problem's record, one slice of distances per entry.  chb_*_pairs_multi run the same list
// form over a pair chunk behind (a)'s pair form: the arguments say B = 1, so problem g is position g and a slice is the
// chunk's pairs.
// The witness forms of both (chb_*_pairs_witness_wide, pairs only) store m doubles each per pair behind what the plain
// forms do and nothing before it: (a) every list entry's rooted distance, (b) every lane's weight.
//
// Numerics: the selection arithmetic is chb_pairwise_distance's, bit for bit -- sum_k (y_k - p_k)^2 sequentially in k with
// separate multiply and add (fp contraction is off from the pragma below on), a correctly rounded sqrt, members ordered
// by (distance, sample index) -- so a problem's list is what chb_topm_per_bin returns for it.  The distance depends on the
// list alone: the solve kernel reads nothing of the tile, chunk or position a problem came from but its list, so a
// pair's distance has the bits of the dense call's entry.  The Gram arithmetic (matrix core, features in groups of four)
// is not hull_generic_kernel's (one fused multiply-add per feature), so the two agree to rounding, not bit for bit.
#include "chb_internal.h"
#include "hull_solve16.h"
#include "hull_solve64.h"

#include <limits.h>
#include <math.h>

#include <type_traits>

namespace chb {
namespace {

// the lower-triangle tile (bi, bj), bj <= bi, of the block grid
__device__ __forceinline__ constexpr int wide_tile(int bi, int bj) { return bi * (bi + 1) / 2 + bj; }

// the witness forms (chb_*_pairs_witness_wide) take the record buffers behind the plain arguments; the plain forms keep
// the arguments they have
template <bool kWitness, bool kList = false>
using wide_args_t = std::conditional_t<kList, RecruitWideListArgs, std::conditional_t<kWitness, RecruitWideWitnessArgs, RecruitWideArgs>>;

// Problem g of the chunk: its list is a.list[g (m + 1) ..], its distance goes to a.dist[g] -- position g of a pair
// chunk (a.tile set), entry (g / B, g % B) of a dense chunk's [nq][B] table.
// kWitness (pairs only): lane a < m also stores the weight of vertex a as active_set_distance2 returned it, 0 where the
// list has no such vertex, to a.w_alpha[g m + a]: one plain vector store per lane behind the solve, nothing before it.
// The `false` instantiations are unchanged: every place sits behind `if constexpr (kWitness)`.
// kList (chb_*_rows_multi_wide, dense only): block (g, i) is problem g at the launch's entry i, m' = a.mw[i].  The list
// buffer holds records of a.lstride ints, written by the selection at the list's largest entry; the m' nearest are the
// record's first m' ids, so the block does what the single call's does at m = m' -- the same Gram of min(length, m')
// vertices, the same solve -- and stores its distance in slice i: a.dist[i nq B + g].  A launch holds entries of one
// kernel only (NV = 32: 17 .. 32, NV = 64: 33 .. 64; the host launches each group it has), so the bits are
// hull_wide_kernel<NV>'s at m = m'.  (Forming a problem's Gram once and solving its entries in a loop was measured and
// lost: with the solver one loop deeper the compiler no longer unrolls its loops over the LDS rows, and the solve
// alone took 1.4 x the single call's.)
template <int NV, bool kWitness = false, bool kList = false>
__global__ __launch_bounds__(64) void hull_wide_kernel(wide_args_t<kWitness, kList> a, int nprob)
{
    static_assert(!(kWitness && kList), "witnesses travel with the single pair calls: a list has no witness form");
    constexpr int NB = NV / 16, NT = NB * (NB + 1) / 2;
    using Lds = GenLdsT<NV>;
    Lds *Lp;
    if constexpr (NV == 64) {
        extern __shared__ __attribute__((aligned(16))) unsigned char wide_smem[];
        Lp = reinterpret_cast<Lds *>(wide_smem);
    } else {
        __shared__ __attribute__((aligned(16))) Lds wide_lds;
        Lp = &wide_lds;
    }
    Lds &L = *Lp;
    const int lane = threadIdx.x;
    const int g = blockIdx.x;
    if (g >= nprob) return;
    int m = a.m;
    const int *lst;
    double *dst = a.dist;
    if constexpr (kList) {
        m = a.mw[blockIdx.y];
        lst = a.list + (size_t)g * (size_t)a.lstride;
        dst += (size_t)blockIdx.y * ((size_t)a.nq * (size_t)a.B);
    } else lst = a.list + (size_t)g * (size_t)(m + 1);
    const int n = min(lst[0], min(m, NV));   // (never more than the capacity, whatever the buffer holds)
    if (n <= 0) {
        if (lane == 0) dst[g] = kInf;
        if constexpr (kWitness) {
            if (lane < m) a.w_alpha[(size_t)g * (size_t)m + lane] = 0.0;   // (no vertex: the record's padding)
        }
        return;
    }
    const int pos = a.tile ? g : g / a.B;
    const int row = lane & 15, kq = lane >> 4;
    const int nb = (n + 15) >> 4;   // blocks that hold a vertex (wave-uniform)
    const double *qptr = (a.qid ? a.X + (size_t)a.qid[pos] * a.Dp : a.Y + (size_t)pos * a.Dp) + 4 * kq;
    const double *vptr[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int e = 16 * b + row;
        const int id = e < n ? lst[1 + e] : -1;
        vptr[b] = id >= 0 ? a.X + (size_t)id * a.Dp + 4 * kq : qptr;   // a missing vertex reads the query row: y = 0
    }
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int Dk = (a.D + 7) & ~7;
    // 16 features per step: features k0 + 4 kq .. + 3 of the query row and of my vertex in every block, the next step's
    // loads in flight under this step's matrix-core work.  (Dk % 8 == 0 and 4 kq % 4 == 0: a lane's four features are all
    // in range or all out; a block without a vertex is y = 0 without a load)
    double2 cx0, cx1, cv0[NB], cv1[NB], nx0, nx1, nv0[NB], nv1[NB];
    auto load = [&](int k0, double2 &x0, double2 &x1, double2 (&v0)[NB], double2 (&v1)[NB]) {
        const bool in = k0 + 4 * kq < Dk;
        x0 = double2{0.0, 0.0}; x1 = x0;
        if (in) {
            x0 = *reinterpret_cast<const double2 *>(qptr + k0);
            x1 = *reinterpret_cast<const double2 *>(qptr + k0 + 2);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            v0[b] = x0; v1[b] = x1;
            if (in && b < nb) {
                v0[b] = *reinterpret_cast<const double2 *>(vptr[b] + k0);
                v1[b] = *reinterpret_cast<const double2 *>(vptr[b] + k0 + 2);
            }
        }
    };
    load(0, cx0, cx1, cv0, cv1);
    for (int k0 = 0; k0 < Dk; k0 += 16) {
        const bool more = k0 + 16 < Dk;
        if (more) load(k0 + 16, nx0, nx1, nv0, nv1);
        double y[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            y[b][0] = cv0[b].x - cx0.x; y[b][1] = cv0[b].y - cx0.y;
            y[b][2] = cv1[b].x - cx1.x; y[b][3] = cv1[b].y - cx1.y;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int bi = 0; bi < NB; ++bi) {
                if (bi < nb) {
#pragma unroll
                    for (int bj = 0; bj <= bi; ++bj)
                        acc[wide_tile(bi, bj)] =
                            __builtin_amdgcn_mfma_f64_16x16x4f64(y[bi][t], y[bj][t], acc[wide_tile(bi, bj)], 0, 0, 0);
                }
            }
        }
        if (more) {
            cx0 = nx0; cx1 = nx1;
#pragma unroll
            for (int b = 0; b < NB; ++b) { cv0[b] = nv0[b]; cv1[b] = nv1[b]; }
        }
    }
    // lane (row, kq) holds <vertex 16 bi + kq + 4 r, vertex 16 bj + row> in acc[(bi, bj)][r]: into place, and mirrored
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
        if (bi < nb) {
#pragma unroll
            for (int bj = 0; bj <= bi; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[wide_tile(bi, bj)][r];
                    L.Q[16 * bi + kq + 4 * r][16 * bj + row] = v;
                    if (bj != bi) L.Q[16 * bj + row][16 * bi + kq + 4 * r] = v;
                }
        }
    }
    const bool mine = lane < n;
    Wave64T<NV> w{L, n, 0.0, 0.0, lane, mine, 0ull};
    w.reset();   // (H = 0; its gen_sync also stands between the Gram's writes and their reads)
    const double diag = mine ? L.Q[lane][lane] : 0.0;
    double scale = diag;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) scale = fmax(scale, __shfl_xor(scale, off, 64));
    w.scale = scale; w.diag = diag;
    double alpha = 0.0;
    const double val = active_set_distance2(w, n, a.metric, scale, alpha);
    if (lane == 0) dst[g] = sqrt(fmax(val, 0.0));
    if constexpr (kWitness) {
        if (lane < m) a.w_alpha[(size_t)g * (size_t)m + lane] = mine ? alpha : 0.0;
    }
}

}  // namespace
}  // namespace chb

#pragma clang fp contract(off)

#include "topm_select_wide.h"

namespace chb {
namespace {

// LDS of a workgroup: the tile loop's staging buffers (RecruitStage of recruit_kernels.hip)
struct WideStage {
    double q[2][kKChunk][kLdsStride];
    double p[2][kKChunk][kLdsStride];
    int mid[2][kPTile];
    int grp[2][kPTile];
    int own[kQTile], owng[kQTile];   // the tile's own sample ids and group ids: read at a tile's end, not kept in registers
};

// recruit_kernel's tile loop (the template parameters mean what they mean there) around four-slab lists.  Per thread the
// lists of its 4 rows take 4 x 4 (distance, id) entries next to the 4 x 4 micro-tile: 48 + 32 VGPRs.  With the rows' own ids in
// LDS and the slabs shifted last-first (no copy of the list is live) every instantiation fits the 256 registers a wavefront
// has at two workgroups per CU without scratch, so the 64-row tile and the occupancy of recruit_kernel both stay.
// kWitness (chb_*_pairs_witness_wide, pairs only): behind a problem's ids every entry's rooted selection distance -- the
// slab value the lane holds -- goes to a.w_d[problem m ..], +inf past the list's length, by the same lane-per-entry
// vector stores.  The `false` instantiations are unchanged: every place sits behind `if constexpr (kWitness)`.
template <bool kResident, bool kPairs, bool kGrouped, bool kWitness = false>
__global__ __launch_bounds__(256, 2) void recruit_select_wide_kernel(wide_args_t<kWitness> a, int nqt, int total)
{
    static_assert(kResident || !kGrouped, "groups are a property of the resident samples");
    static_assert(kPairs || !kWitness, "witnesses travel with the pair calls: one record per listed pair");
    __shared__ __attribute__((aligned(16))) WideStage lds;

    // XCD-aware order: blocks b and b+8 share an XCD (and its L2), so hand each XCD a contiguous range of work
    // items; consecutive items share a bin, i.e. the same member rows.
    const int per = (total + 7) >> 3;
    const int W = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (W >= total) return;
    int c, qt, nrow = kQTile;
    if constexpr (kPairs) {
        const int4 t = a.tile[W];
        c = t.x; qt = t.y; nrow = t.z;
    } else {
        c = W / nqt; qt = W - c * nqt;
    }

    const int tid = threadIdx.x, lane = tid & 63;
    const int tx = tid & 15, ty = tid >> 4;
    const int gbase = lane & 48;
    const int srow = tid >> 2, skp = tid & 3;

    const int mb = a.bin_ptr[c], nmem = a.bin_ptr[c + 1] - mb;
    const int pos0 = kPairs ? qt : qt * kQTile;
    const int m = a.m, ns = (m + 15) >> 4;

    // list state of my 4 rows: this lane holds entry 16 r + tx of slab r
    double ld[4][kWideSlabs], tau[4];
    int li[4][kWideSlabs], lc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < kWideSlabs; ++r) { ld[i][r] = kInf; li[i][r] = INT_MAX; }
        lc[i] = 0; tau[i] = kInf;
    }

    // staging role: thread (srow, skp) moves feature columns [2*skp, 2*skp+1] of one row per chunk
    int sq = pos0 + srow;
    if (sq >= a.nq) sq = a.nq - 1;
    const double *qrow;
    if constexpr (kResident) qrow = a.X + (size_t)a.qid[sq] * a.Dp + 2 * skp;
    else qrow = a.Y + (size_t)sq * a.Dp + 2 * skp;
    // the sample ids of the tile's rows (a position past the chunk's end scores nothing: any id will do) and their group
    // ids (negative: no group), for the exclusions at every tile's end
    if constexpr (kResident) {
        if (tid < kQTile) {
            const int o = a.qid[min(pos0 + tid, a.nq - 1)];
            lds.own[tid] = o;
            if constexpr (kGrouped) lds.owng[tid] = a.grp[o];
        }
    }
    const double *prow = a.X + 2 * skp;
    const int nch = a.Dp / kKChunk;
    const int ntile = (nmem + kPTile - 1) / kPTile;
    const int nsteps = ntile * nch;

    double2 rq, rp;
    int pmid = -1, pgrp = -1;
    int nt = 0, nc = 0;  // (tile, chunk) of the step being prefetched
    auto prefetch = [&]() {
        if (nc == 0) {
            const int e = nt * kPTile + srow;
            pmid = e < nmem ? a.memb_id[mb + e] : -1;
            if constexpr (kGrouped) pgrp = e < nmem ? a.memb_grp[mb + e] : -1;
            if constexpr (kWitness) {
                // With the record stores behind the loop the grouped form came out three registers short and spilled
                // its copy of a.X + 2 skp, a 64-bit pair that lives across the whole tile loop.  Here the column
                // offset stays 32 bits wide and joins the row's offset once per tile; the empty asm statements keep
                // the compiler from splitting the sum up again.  No scratch, two workgroups per CU as before.
                int col = 2 * skp;
                asm volatile("" : "+v"(col));
                size_t off = (size_t)(pmid < 0 ? 0 : pmid) * a.Dp + (size_t)col;
                asm volatile("" : "+v"(off));
                prow = a.X + off;
            } else prow = a.X + (size_t)(pmid < 0 ? 0 : pmid) * a.Dp + 2 * skp;
        }
        rq = *reinterpret_cast<const double2 *>(qrow + nc * kKChunk);
        rp = *reinterpret_cast<const double2 *>(prow + nc * kKChunk);
    };
    auto stash = [&](int buf) {
        lds.q[buf][2 * skp][srow] = rq.x;
        lds.q[buf][2 * skp + 1][srow] = rq.y;
        lds.p[buf][2 * skp][srow] = rp.x;
        lds.p[buf][2 * skp + 1][srow] = rp.y;
        if (nc == 0 && skp == 0) {
            lds.mid[nt & 1][srow] = pmid;
            if constexpr (kGrouped) lds.grp[nt & 1][srow] = pgrp;
        }
        if (++nc == nch) { nc = 0; ++nt; }
    };

    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

    if (nsteps > 0) { prefetch(); stash(0); }
    __syncthreads();

    int ct = 0, cc = 0;  // (tile, chunk) of the step being computed
    for (int step = 0; step < nsteps; ++step) {
        const int buf = step & 1;
        const bool has_next = step + 1 < nsteps;
        if (has_next) prefetch();
        // keep the global loads of the next chunk in flight across the whole compute block
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < kKChunk; ++k) {
            const double2 qa = *reinterpret_cast<const double2 *>(&lds.q[buf][k][4 * ty]);
            const double2 qb = *reinterpret_cast<const double2 *>(&lds.q[buf][k][4 * ty + 2]);
            const double2 pa = *reinterpret_cast<const double2 *>(&lds.p[buf][k][2 * tx]);
            const double2 pb = *reinterpret_cast<const double2 *>(&lds.p[buf][k][32 + 2 * tx]);
            const double q[4] = {qa.x, qa.y, qb.x, qb.y};
            const double p[4] = {pa.x, pa.y, pb.x, pb.y};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double df = q[i] - p[j];
                    acc[i][j] = acc[i][j] + df * df;
                }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (has_next) stash(buf ^ 1);
        __syncthreads();
        if (++cc == nch) {
            // tile finished: offer its 64 members to the lists
            int mid[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) mid[j] = lds.mid[ct & 1][(j < 2) ? 2 * tx + j : 32 + 2 * tx + (j - 2)];
            int gm[4];
            if constexpr (kGrouped) {
#pragma unroll
                for (int j = 0; j < 4; ++j) gm[j] = lds.grp[ct & 1][(j < 2) ? 2 * tx + j : 32 + 2 * tx + (j - 2)];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bool qvalid;
                if constexpr (kPairs) qvalid = 4 * ty + i < nrow;
                else qvalid = pos0 + 4 * ty + i < a.nq;
                [[maybe_unused]] int own = 0, owng = -1;
                if constexpr (kResident) own = lds.own[4 * ty + i];
                if constexpr (kGrouped) owng = lds.owng[4 * ty + i];
                double s[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bool offer = qvalid && mid[j] >= 0;
                    if constexpr (kResident) offer = offer && mid[j] != own;   // only the row itself: a twin stays
                    if constexpr (kGrouped) offer = offer && !(gm[j] >= 0 && gm[j] == owng);   // ... and its group
                    s[j] = offer ? acc[i][j] : kInf;
                    acc[i][j] = 0.0;
                }
                select_wide_into<4>(s, mid, ld[i], li[i], lc[i], tau[i], m, ns, tx, gbase);
            }
            cc = 0; ++ct;
        }
    }

    // the lists: length, then m ids (-1 past the length); plain vector stores, one record per problem
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int qpos = pos0 + 4 * ty + i;
        bool qvalid;
        if constexpr (kPairs) qvalid = 4 * ty + i < nrow;
        else qvalid = qpos < a.nq;
        if (!qvalid) continue;
        const size_t prob = kPairs ? (size_t)qpos : (size_t)qpos * (size_t)a.B + (size_t)c;
        int *out = a.list + prob * (size_t)(m + 1);
        if (tx == 0) out[0] = lc[i];
#pragma unroll
        for (int r = 0; r < kWideSlabs; ++r) {
            const int e = 16 * r + tx;
            if (r < ns && e < m) out[1 + e] = e < lc[i] ? li[i][r] : -1;
        }
        if constexpr (kWitness) {
            double *wd = a.w_d + prob * (size_t)m;
#pragma unroll
            for (int r = 0; r < kWideSlabs; ++r) {
                const int e = 16 * r + tx;
                if (r < ns && e < m) wd[e] = e < lc[i] ? ld[i][r] : kInf;
            }
        }
    }
}

template <bool kResident, bool kGrouped>
void launch_select_witness(const RecruitWideWitnessArgs &a, hipStream_t s)
{
    if (a.nq <= 0 || a.ntile <= 0) return;
    const int grid = ((a.ntile + 7) / 8) * 8;
    hipLaunchKernelGGL((recruit_select_wide_kernel<kResident, true, kGrouped, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
}

template <bool kResident, bool kGrouped>
void launch_select(const RecruitWideArgs &a, hipStream_t s)
{
    if (a.tile) {
        if (a.nq <= 0 || a.ntile <= 0) return;
        const int grid = ((a.ntile + 7) / 8) * 8;
        hipLaunchKernelGGL((recruit_select_wide_kernel<kResident, true, kGrouped>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
        return;
    }
    if (a.nq <= 0 || a.B <= 0) return;
    const int nqt = (a.nq + kQTile - 1) / kQTile;
    const int total = nqt * a.B;
    const int grid = ((total + 7) / 8) * 8;
    hipLaunchKernelGGL((recruit_select_wide_kernel<kResident, false, kGrouped>), dim3(grid), dim3(256), 0, s, a, nqt, total);
}

}  // namespace

// (a.qid / a.memb_grp / a.tile choose the instantiation)
void launch_recruit_select_wide(const RecruitWideArgs &a, hipStream_t s)
{
    if (!a.qid) launch_select<false, false>(a, s);
    else if (a.memb_grp) launch_select<true, true>(a, s);
    else launch_select<true, false>(a, s);
}

// the witness form: a pair chunk (a.tile set), a.w_d written here
void launch_recruit_select_wide_witness(const RecruitWideWitnessArgs &a, hipStream_t s)
{
    if (!a.qid) launch_select_witness<false, false>(a, s);
    else if (a.memb_grp) launch_select_witness<true, true>(a, s);
    else launch_select_witness<true, false>(a, s);
}

// one wavefront per problem: nq x B of a dense chunk, nq of a pair chunk
void launch_hull_wide(const RecruitWideArgs &a, hipStream_t s)
{
    const long long nprob = a.tile ? (long long)a.nq : (long long)a.nq * (long long)a.B;
    if (nprob <= 0) return;
    if (a.m <= 32) {
        hipLaunchKernelGGL((hull_wide_kernel<32>), dim3((unsigned)nprob), dim3(64), 0, s, a, (int)nprob);
        return;
    }
    // per launch (cheap, and the attribute is per device), as launch_generic does for hull_generic_kernel; whether the
    // device grants it at all is asked up front by the entry points (hull_generic_supported(): the same 66 KiB)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(hull_wide_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)sizeof(GenLdsT<64>));
    hipLaunchKernelGGL((hull_wide_kernel<64>), dim3((unsigned)nprob), dim3(64), sizeof(GenLdsT<64>), s, a, (int)nprob);
}

// the list form: one wavefront per (problem of a dense chunk, entry of the launch), a.nw slices of a.dist written here
// (a pair chunk: a.tile set and a.B = 1, its nq positions are the problems)
void launch_hull_wide_list(const RecruitWideListArgs &a, hipStream_t s)
{
    const long long nprob = (long long)a.nq * (long long)a.B;
    if (nprob <= 0 || a.nw <= 0) return;
    if (a.m <= 32) {
        hipLaunchKernelGGL((hull_wide_kernel<32, false, true>), dim3((unsigned)nprob, (unsigned)a.nw), dim3(64), 0, s, a, (int)nprob);
        return;
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(hull_wide_kernel<64, false, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GenLdsT<64>));
    hipLaunchKernelGGL((hull_wide_kernel<64, false, true>), dim3((unsigned)nprob, (unsigned)a.nw), dim3(64), sizeof(GenLdsT<64>), s, a, (int)nprob);
}

// the witness form: one wavefront per position of a pair chunk, a.w_alpha written here
void launch_hull_wide_witness(const RecruitWideWitnessArgs &a, hipStream_t s)
{
    if (a.nq <= 0) return;
    if (a.m <= 32) {
        hipLaunchKernelGGL((hull_wide_kernel<32, true>), dim3((unsigned)a.nq), dim3(64), 0, s, a, a.nq);
        return;
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(hull_wide_kernel<64, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)sizeof(GenLdsT<64>));
    hipLaunchKernelGGL((hull_wide_kernel<64, true>), dim3((unsigned)a.nq), dim3(64), sizeof(GenLdsT<64>), s, a, a.nq);
}

}  // namespace chb
