// Hull distances of rows to every bin of a frozen labelling for gfx950: NEW rows that are not samples
// (chb_recruit_rows), or resident rows with the row itself left out (chb_audit_rows).
//
// What a fit does for a resident row -- find_nearest_from_cluster (distance_matrix.py:47-62) per bin, then
// calculate_distance (hull_distance.py:90-108) to the hull of those members -- in ONE kernel and without any of the
// fit's state: no member codes, no gate, no flag list, no shortlist stage.  For rows Y that are not part of the resident
// matrix nothing is excluded; for a resident row the only exclusion is the row's own sample index.
//
// One 256-thread workgroup owns (64 rows of Y) x (one bin), tile_kernel's pattern (topm_kernels.hip): the bin's members
// are streamed in tiles of 64 rows, a 64 x 64 tile of squared distances is accumulated with a 4 x 4 register micro-tile
// per thread (fp64 VALU; LDS-staged transposed k-chunks, double buffered), and the 16 lanes that share a row keep its
// sorted (distance, index) list in registers (select_into).  Once the last tile is in, the same 16 lanes solve the
// row's hull problem in place: lane a's list entry is vertex a, the matrix core forms the Gram tile of (p_a - y) from
// the vertex rows (read straight from L2: they were streamed a moment ago) and the 16-lane active-set solver of the
// hull kernels (hull_solve16.h) runs on it.  One store per (row, bin).  The staging buffers and the solver's Gram tiles
// share the workgroup's LDS (the first is dead when the second is written).
//
// Numerics: the selection arithmetic is chb_pairwise_distance's, bit for bit -- every squared distance is
// sum_k (y_k - p_k)^2 accumulated sequentially in k with separate multiply and add (fp contraction is off from the
// pragma below on), then a correctly rounded sqrt; members are ordered by (distance, sample index).  The solver is
// compiled exactly as in qp_kernels.hip (its header is included above the pragma).
//
// A bin is never cut into member ranges: one bin of N members gives ceil(rows / 64) work items that each stream all N
// member rows.  A second small kernel reduces each row of B distances to bin, minimum and margin.
//
// chb_audit_rows runs the same kernel body on RESIDENT rows (template parameter kResident): the rows to score are samples
// named by index, and a row is withheld from its own bin's candidates -- the leave-one-out step of algorithm.py:49-58.
//
// chb_audit_pairs / chb_recruit_pairs run the same kernel body on a LIST of (row, bin) pairs (template parameter kPairs):
// the work items come from a tile table the host cut from the pairs in bin order, and a pair's one distance is stored at
// its position; there is no reduction kernel behind it.  chb_audit_pairs_multi / chb_recruit_pairs_multi serve a list of m
// up to 16 from the same work items (kMulti and kPairs together): one slice of the chunk's positions per entry.
//
// The chb_*_grouped calls run the resident instantiations with one more exclusion (template parameter kGrouped): besides
// the row itself every sample that shares the row's group id -- the sibling pieces of one parent contig -- is withheld.
//
// chb_audit_pairs_witness / chb_recruit_pairs_witness run the pairs' kernel body with one more output (template parameter
// kWitness): per pair the vertices the distance was measured to, their selection distances and their weights.
//
// chb_bin_report runs the audit's two kernels on positions grouped by their own label and a third, bin_report_kernel
// (below), that folds each chunk's distances and bins into B x B tables keyed (own label, bin).
//
// chb_audit_rows_nearest / chb_recruit_rows_nearest run the dense kernel and, in place of the row reduction,
// nearest_bins_kernel (below): each row's k least finite distances with their bins, in (distance, bin) order.
#include "chb_internal.h"
#include "hull_solve16.h"

#include <limits.h>
#include <math.h>

#include <type_traits>

#pragma clang fp contract(off)

#include "topm_select.h"

namespace chb {
namespace {

// LDS of a workgroup: the tile loop's staging buffers, then the solver's Gram tiles and exchange rows
struct RecruitStage {
    double q[2][kKChunk][kLdsStride];
    double p[2][kKChunk][kLdsStride];
    int mid[2][kPTile];
    int grp[2][kPTile];   // (kGrouped: the members' group ids, next to mid; the union's size is RecruitSolve's)
};
struct RecruitSolve {
    double Qt[4][4][16][kQ16Ld];   // [wavefront][16-lane group][row][col], padded
    double sv[4][4][16];
};
union RecruitLds {
    RecruitStage st;
    RecruitSolve so;
};

// (two wavefronts per SIMD, like tile_kernel: at the solver's three the tile loop's lists and micro-tile would spill)
//
// kResident (chb_audit_rows): position q of the chunk is the resident sample a.qid[q] -- its row is read from X, nothing
// is uploaded -- and that sample alone is withheld from its own lists (leave-one-out: algorithm.py:50).  Everything else,
// the arithmetic included, is the same code; the `false` instantiation is chb_recruit_rows' kernel unchanged.
//
// kMulti (chb_audit_rows_multi / chb_recruit_rows_multi): a list of m (the bits of a.mmask) served from one selection
// pass, one [nq][B] slice of dist per entry in ascending order.  a.m is the list's largest entry, so the lists hold the min(members, a.m) nearest in (distance, index)
// order and the m' nearest of any smaller m' are their first m' entries; entry (r, c) of the Gram tile is computed from
// vertices r and c alone, so the m' x m' problem is the tile's leading block.  Per row: phase 1 once, every lane keeps
// its plain row of the tile in registers (the selection state is dead by then), and per list entry the tile is written
// back with everything outside the leading block zeroed -- what a launch with that m alone hands to solve16, where a
// missing vertex reads the query row -- because solve16 overwrites the tile with the lifted, rescaled Gram.  The `false`
// instantiations are the single-m kernels unchanged: everything of the list sits behind `if constexpr (kMulti)`.
//
// kPairs (chb_audit_pairs / chb_recruit_pairs): a list of (row, bin) pairs in place of the dense grid.  The host has put
// the pairs in bin order and cut every bin's run into tiles of at most kQTile positions; work item W is row W of the
// chunk's tile table a.tile = {bin, first position in the chunk, positions}, rows of the tile at or past `positions`
// score nothing, and the one double of a position goes to a.dist[position].  Nothing else differs from the single-m
// kernel -- the staged rows of a short tile's tail are the next tile's (or the chunk's last), read and never offered --
// so a pair's distance has the bits of the dense call's entry.  The `false` instantiations are unchanged: the
// places sit behind `if constexpr (kPairs)`.
//
// kMulti && kPairs (chb_audit_pairs_multi / chb_recruit_pairs_multi, the entries up to 16): the work items of the tile
// table, the list's phase 2 as it is, and one double per (entry, position) -- slice j of a.dist is the chunk's a.nq
// positions, a.dist[j * a.nq + position], stored for the tile's counted rows as in the pair form.  A position's list is
// the single pair launch's at a.m, its first m' entries that launch's at m', so slice j has the bits of the pair kernel at
// the list's j-th smallest entry.
//
// kGrouped (chb_*_grouped, resident rows only): leave-group-out.  Every sample carries a dense int32 group id, negative
// for a sample without a group; besides the row itself every member of the row's group is withheld, whichever bin is
// being scored.  A member's group id travels with its sample index -- a.memb_grp is parallel to a.memb_id, loaded by the
// same thread at the same step and staged next to mid -- and each thread keeps the group ids of its 4 rows (a.grp, read
// once per work item where own[] is read) next to own[].  One more compare per offer, nothing else: a candidate's
// distance does not depend on its tile position, the lists are a total order on (distance, index), and the Gram tile and
// the solve depend on the list alone, so a row's result is what the ungrouped kernel gives on labels from which the
// row's group has been taken out.  The `false` instantiations are unchanged: every place sits behind
// `if constexpr (kGrouped)`.
//
// kWitness (chb_*_pairs_witness, pairs only): what the solve knew and the plain kernels drop.  In phase 2 lane (kq, row)
// holds vertex `row` of its group's problem: its sample id (idv[0]), its selection distance -- select_into keeps the
// ROOTED distance in ld[], entry tx of row 4 ty + i, and tx == row, ty == 4 w + kq: the same lane -- and, behind solve16,
// its weight.  ld[] is kept alive past the tile loop (wdv[], shifted with nn[] / idv[]) and the lanes row < m store the
// three to slot `row` of the position's record (RecruitWitnessArgs), padding where row >= n: plain vector stores, one
// record per pair.  Nothing that the distance depends on differs, so a pair's distance has the plain pair kernel's bits.
// The `false` instantiations are unchanged: every place sits behind `if constexpr (kWitness)`.
template <bool kGrouped, bool kPairs, bool kWitness>
using recruit_args_t = std::conditional_t<kWitness, RecruitWitnessArgs,
    std::conditional_t<kGrouped, RecruitGroupArgs, std::conditional_t<kPairs, RecruitPairArgs, RecruitArgs>>>;

template <bool kResident, bool kMulti, bool kPairs, bool kGrouped = false, bool kWitness = false>
__global__ __launch_bounds__(256, 2) void recruit_kernel(recruit_args_t<kGrouped, kPairs, kWitness> a, int nqt, int total)
{
    static_assert(kResident || !kGrouped, "groups are a property of the resident samples");
    static_assert(kPairs || !kWitness, "witnesses travel with the pair calls: one record per listed pair");
    __shared__ __attribute__((aligned(16))) RecruitLds lds;

    // XCD-aware order: blocks b and b+8 share an XCD (and its L2), so hand each XCD a contiguous range of work
    // items; consecutive items share a bin, i.e. the same member rows.
    const int per = (total + 7) >> 3;
    const int W = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (W >= total) return;
    int c, qt, nrow = kQTile;   // the bin; the tile of 64 positions or (pairs) its first position, and how many of its rows count
    if constexpr (kPairs) {
        const int4 t = a.tile[W];
        c = t.x; qt = t.y; nrow = t.z;
    } else {
        c = W / nqt; qt = W - c * nqt;
    }

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tx = tid & 15, ty = tid >> 4;
    const int gbase = lane & 48;
    const int srow = tid >> 2, skp = tid & 3;

    const int mb = a.bin_ptr[c], nmem = a.bin_ptr[c + 1] - mb;
    const int pos0 = kPairs ? qt : qt * kQTile;
    const int m = a.m;

    // list state of my 4 rows: this lane holds entry #tx
    double ld[4], tau[4];
    int li[4], lc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ld[i] = kInf; li[i] = INT_MAX; lc[i] = 0; tau[i] = kInf; }

    // staging role: thread (srow, skp) moves feature columns [2*skp, 2*skp+1] of one row per chunk
    int sq = pos0 + srow;
    if (sq >= a.nq) sq = a.nq - 1;
    const double *qrow;
    if constexpr (kResident) qrow = a.X + (size_t)a.qid[sq] * a.Dp + 2 * skp;
    else qrow = a.Y + (size_t)sq * a.Dp + 2 * skp;
    // the sample ids of my 4 rows (a position past the chunk's end scores nothing: any id will do)
    int own[4];
    if constexpr (kResident) {
#pragma unroll
        for (int i = 0; i < 4; ++i) own[i] = a.qid[min(pos0 + 4 * ty + i, a.nq - 1)];
    }
    // ... and their group ids (negative: no group)
    int owng[4];
    if constexpr (kGrouped) {
#pragma unroll
        for (int i = 0; i < 4; ++i) owng[i] = a.grp[own[i]];
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
            prow = a.X + (size_t)(pmid < 0 ? 0 : pmid) * a.Dp + 2 * skp;
        }
        rq = *reinterpret_cast<const double2 *>(qrow + nc * kKChunk);
        rp = *reinterpret_cast<const double2 *>(prow + nc * kKChunk);
    };
    auto stash = [&](int buf) {
        lds.st.q[buf][2 * skp][srow] = rq.x;
        lds.st.q[buf][2 * skp + 1][srow] = rq.y;
        lds.st.p[buf][2 * skp][srow] = rp.x;
        lds.st.p[buf][2 * skp + 1][srow] = rp.y;
        if (nc == 0 && skp == 0) {
            lds.st.mid[nt & 1][srow] = pmid;
            if constexpr (kGrouped) lds.st.grp[nt & 1][srow] = pgrp;
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
        // keep the global loads of the next chunk in flight across the whole compute block: the
        // scheduler must neither sink them nor hoist the LDS stores that consume them
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < kKChunk; ++k) {
            const double2 qa = *reinterpret_cast<const double2 *>(&lds.st.q[buf][k][4 * ty]);
            const double2 qb = *reinterpret_cast<const double2 *>(&lds.st.q[buf][k][4 * ty + 2]);
            const double2 pa = *reinterpret_cast<const double2 *>(&lds.st.p[buf][k][2 * tx]);
            const double2 pb = *reinterpret_cast<const double2 *>(&lds.st.p[buf][k][32 + 2 * tx]);
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
            for (int j = 0; j < 4; ++j) mid[j] = lds.st.mid[ct & 1][(j < 2) ? 2 * tx + j : 32 + 2 * tx + (j - 2)];
            int gm[4];
            if constexpr (kGrouped) {
#pragma unroll
                for (int j = 0; j < 4; ++j) gm[j] = lds.st.grp[ct & 1][(j < 2) ? 2 * tx + j : 32 + 2 * tx + (j - 2)];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bool qvalid;
                if constexpr (kPairs) qvalid = 4 * ty + i < nrow;
                else qvalid = pos0 + 4 * ty + i < a.nq;
                double s[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bool offer = qvalid && mid[j] >= 0;
                    if constexpr (kResident) offer = offer && mid[j] != own[i];   // only the row itself: a twin stays
                    if constexpr (kGrouped) offer = offer && !(gm[j] >= 0 && gm[j] == owng[i]);   // ... and its group
                    s[j] = offer ? acc[i][j] : kInf;
                    acc[i][j] = 0.0;
                }
                select_into<16, 4>(s, mid, ld[i], li[i], lc[i], tau[i], m, tx, gbase);
            }
            cc = 0; ++ct;
        }
    }
    __syncthreads();   // the staging buffers (the last tile's member ids among them) become the solver's tiles

    // ---- the hull problems of my wavefront's 16 rows, four at a time (one per 16-lane group): row i of every group
    int nn[4], idv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { nn[i] = lc[i]; idv[i] = tx < lc[i] ? li[i] : -1; }
    [[maybe_unused]] double wdv[4];   // (kWitness: the selection distance of my list entry, next to idv)
    if constexpr (kWitness) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wdv[i] = tx < lc[i] ? ld[i] : kInf;
    }
    const int row = lane & 15, kq = lane >> 4;
    const int Dk = (a.D + 7) & ~7;
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        const int n = nn[0], idm = idv[0];
        // phase 1: Gram of the shifted vertices, one matrix-core tile per problem (lane (row, kq): vertex `row`,
        // features 4 kq .. 4 kq + 3 of every 16); a missing vertex reads the query row: y = 0
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
            const int np = __shfl(n, 16 * p, 64);
            const int id = __shfl(idm, 16 * p + row, 64);
            if (np <= 0) continue;   // wave-uniform
            // (np > 0: a row of the chunk; its sample id sits in the registers of group p, row i of which is own[0] by now)
            const double *qptr;
            if constexpr (kResident) qptr = a.X + (size_t)__shfl(own[0], 16 * p, 64) * a.Dp + 4 * kq;
            else qptr = a.Y + (size_t)(pos0 + 4 * (4 * w + p) + i) * a.Dp + 4 * kq;
            const double *vptr = id >= 0 ? a.X + (size_t)id * a.Dp + 4 * kq : qptr;
            f64x4 g = {0.0, 0.0, 0.0, 0.0}, d0 = g, d1 = g;
            gram_tile16_rows<false>(vptr, vptr, qptr, Dk, kq, g, d0, d1);
#pragma unroll
            for (int r = 0; r < 4; ++r) lds.so.Qt[w][p][kq + 4 * r][row] = g[r];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wavefront's LDS writes have landed
        // phase 2: one problem per 16-lane group
        const int qpos = pos0 + 4 * ty + i;
        if constexpr (kMulti) {
            // my plain row of the group's tile (rows and columns at or past n are zero already)
            double *Qg = &lds.so.Qt[w][kq][0][0];
            double gr[16];
#pragma unroll
            for (int k = 0; k < 16; k += 2) {
                const double2 t = *reinterpret_cast<const double2 *>(Qg + row * kQ16Ld + k);
                gr[k] = t.x; gr[k + 1] = t.y;
            }
            int nlast = -1;       // the n my group solved last, and its distance: a bin with no more members than two
            double dist = kInf;   // list entries asks for the same problem twice
            unsigned left = a.mmask;
#pragma unroll 1
            for (int j = 0; left; ++j) {
                const int nj = min(n, __ffs(left));   // (ascending: once nj has reached n it stays there)
                left &= left - 1;
                if (n > 0 && nj != nlast) {
                    // the leading nj x nj block of the tile, zero around it
#pragma unroll
                    for (int k = 0; k < 16; k += 2)
                        *reinterpret_cast<double2 *>(Qg + row * kQ16Ld + k) =
                            double2{(row < nj && k < nj) ? gr[k] : 0.0, (row < nj && k + 1 < nj) ? gr[k + 1] : 0.0};
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_s_waitcnt(0xC07F);
                    double alpha = 0.0;
                    const double val = solve16(Qg, &lds.so.sv[w][kq][0], nj, a.metric, lane, alpha);
                    dist = sqrt(fmax(val, 0.0));
                    nlast = nj;
                    __builtin_amdgcn_wave_barrier();   // the tile is rewritten for the next list entry
                }
                if constexpr (kPairs) {
                    if (tx == 0 && 4 * ty + i < nrow) a.dist[(size_t)j * a.nq + qpos] = dist;
                } else {
                if (tx == 0 && qpos < a.nq) a.dist[((size_t)j * a.nq + qpos) * a.B + c] = dist;
                }
            }
        } else {
        double dist = kInf;
        [[maybe_unused]] double wal = 0.0;   // (kWitness: my vertex's weight)
        if (n > 0) {
            double alpha = 0.0;
            const double val = solve16(&lds.so.Qt[w][kq][0][0], &lds.so.sv[w][kq][0], n, a.metric, lane, alpha);
            dist = sqrt(fmax(val, 0.0));
            if constexpr (kWitness) wal = alpha;
        }
        if constexpr (kWitness) {
            // slot `row` of the position's record (qpos < a.nq: a tile's counted rows lie inside its chunk)
            if (4 * ty + i < nrow && row < m) {
                const size_t o = (size_t)qpos * kWitnessSlots + row;
                const bool real = row < n;
                a.w_id[o] = real ? idm : -1;
                a.w_d[o] = real ? wdv[0] : kInf;
                a.w_alpha[o] = real ? wal : 0.0;
            }
        }
        if constexpr (kPairs) {
            if (tx == 0 && 4 * ty + i < nrow) a.dist[qpos] = dist;
        } else {
        if (tx == 0 && qpos < a.nq) a.dist[(size_t)qpos * a.B + c] = dist;
        }
        }
        __builtin_amdgcn_wave_barrier();   // the tiles are rewritten by the next row's phase 1
        nn[0] = nn[1]; nn[1] = nn[2]; nn[2] = nn[3];
        idv[0] = idv[1]; idv[1] = idv[2]; idv[2] = idv[3];
        if constexpr (kResident) { own[0] = own[1]; own[1] = own[2]; own[2] = own[3]; }
        if constexpr (kWitness) { wdv[0] = wdv[1]; wdv[1] = wdv[2]; wdv[2] = wdv[3]; }
    }   // (owng[] is dead behind the tile loop: nothing to shift)
}

// strict-'>' scan over each row of B distances (algorithm.py:57: lowest index among equal minima, -1 when every entry
// is +inf), the minimum and the margin = smallest distance of any OTHER bin minus the minimum (+inf without a finite
// runner-up, never inf - inf).  8 lanes per row.
__global__ __launch_bounds__(256) void recruit_reduce_kernel(const double *dist, int nq, int B, int *bin, double *mind,
                                                             double *margin)
{
    const int j = threadIdx.x & 7;
    const int q = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 3);
    const bool valid = q < nq;
    double best = kInf, runner = kInf;
    int bc = -1;
    if (valid) {
        const double *row = dist + (size_t)q * B;
        for (int c = j; c < B; c += 8) {
            const double d = row[c];
            if (best > d) { runner = best; best = d; bc = c; }
            else if (runner > d) runner = d;
        }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
        const double ob = __shfl_xor(best, off, 64), orr = __shfl_xor(runner, off, 64);
        const int oc = __shfl_xor(bc, off, 64);
        // the other side wins on a smaller distance, or on the same (finite) distance with the lower bin
        const bool take = ob < best || (ob == best && oc >= 0 && (bc < 0 || oc < bc));
        const double lose = take ? best : ob;
        runner = fmin(fmin(runner, orr), lose);
        if (take) { best = ob; bc = oc; }
    }
    if (!valid || j != 0) return;
    bin[q] = bc;
    mind[q] = best;
    margin[q] = runner == kInf ? kInf : runner - best;
}

// chb_*_rows_nearest: the k nearest bins of every row of dist[nrows][B], ranked where the table lies.
//
// select_into's insertion scheme on the plain value: the 16 lanes of a group offer up to NC (distance, bin) candidates
// each to the group's list, lane t of which holds entry t; the list is ordered by lex_less on (distance, bin) -- a total
// order, the bins of a row being distinct -- and keeps the k <= 16 least.  +inf is "no candidate": it never enters the
// list.  No sqrt (the table holds distances) and no tau_from slack (what is compared is what is stored).  A sibling of
// select_into, which is compiled as it was.  Wave-synchronous; all 64 lanes must call it together.
template <int NC>
__device__ __forceinline__ void select_near(double (&s)[NC], const int (&cb)[NC], double &ld, int &li, int &lc, double &e,
                                            int &ei, int k, int tx, int gbase)
{
    // (e, ei): the list's k-th entry, kept by the caller from call to call; (+inf, INT_MAX) while the list is short: every
    // finite candidate is less
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (!(s[j] < kInf) || !lex_less(s[j], cb[j], e, ei)) s[j] = kInf;
    for (;;) {
        double bs = s[0];
        int bi = cb[0], bj = 0;
#pragma unroll
        for (int j = 1; j < NC; ++j)
            if (lex_less(s[j], cb[j], bs, bi)) { bs = s[j]; bi = cb[j]; bj = j; }
        if (!__any(bs < kInf)) break;   // (the common round once the lists are full: no lane of the wavefront has a survivor)
        double gs = bs;
        int gi = bi;
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            const double os = __shfl_xor(gs, off, 16);
            const int oi = __shfl_xor(gi, off, 16);
            if (lex_less(os, oi, gs, gi)) { gs = os; gi = oi; }
        }
        const bool have = gs < kInf;   // (false for the groups without a survivor while another group has one)
        if (have && bs == gs && bi == gi) {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (j == bj) s[j] = kInf;
        }
        const bool lt = (tx < lc) && lex_less(ld, li, gs, gi);
        const unsigned long long bal = __ballot(lt);
        const int pos = __popcll((bal >> gbase) & 0xffffull);
        const double ud = __shfl_up(ld, 1, 16);
        const int ui = __shfl_up(li, 1, 16);
        const bool ins = have && pos < k;   // (pos < k: a candidate that is not less than a full list's k-th entry was dropped)
        if (ins) {
            if (tx == pos) { ld = gs; li = gi; }
            else if (tx > pos) { ld = ud; li = ui; }
            lc = lc + 1 < k ? lc + 1 : k;
        }
        e = __shfl(ld, k - 1, 16);
        ei = __shfl(li, k - 1, 16);
        if (ins && lc >= k) {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (!lex_less(s[j], cb[j], e, ei)) s[j] = kInf;
        }
    }
}

// 16 lanes per row, four rows per wavefront, sixteen per workgroup; the list lives in registers, there is no LDS.  A round
// covers kNearPer * 16 consecutive bins of the row: load j of lane t is bin c0 + 16 j + t, so the 16 lanes of a row read 128
// consecutive bytes per load, and the next round's loads are issued ahead of this round's insertions.  A bin at or past B
// is +inf without a load.  Every wavefront runs the same ceil(B / 64) rounds: a row at or past nrows scans the last
// row (all 64 lanes stay in the cross-lane calls) and stores nothing.  Lanes t < k store slot t: plain vector stores, bin
// -1 and +inf at or past the number of finite entries.
constexpr int kNearPer = 4;
__global__ __launch_bounds__(256) void nearest_bins_kernel(const double *dist, int nrows, int B, int k, int *nb_bin,
                                                           double *nb_dist)
{
    const int tx = threadIdx.x & 15, gbase = threadIdx.x & 48;
    const int q = (int)blockIdx.x * 16 + (int)(threadIdx.x >> 4);
    const bool valid = q < nrows;
    const double *row = dist + (size_t)(valid ? q : nrows - 1) * (size_t)B;
    double ld = kInf, e = kInf;   // my list entry; the list's k-th entry
    int li = INT_MAX, lc = 0, ei = INT_MAX;
    double nx[kNearPer];
    auto load = [&](int c0) {
#pragma unroll
        for (int j = 0; j < kNearPer; ++j) {
            const int c = c0 + 16 * j + tx;
            nx[j] = c < B ? row[c] : kInf;
        }
    };
    load(0);
    for (int c0 = 0; c0 < B; c0 += 16 * kNearPer) {
        double s[kNearPer];
        int cb[kNearPer];
#pragma unroll
        for (int j = 0; j < kNearPer; ++j) { s[j] = nx[j]; cb[j] = c0 + 16 * j + tx; }
        if (c0 + 16 * kNearPer < B) load(c0 + 16 * kNearPer);
        select_near<kNearPer>(s, cb, ld, li, lc, e, ei, k, tx, gbase);
    }
    if (!valid || tx >= k) return;
    const size_t o = (size_t)q * (size_t)k + (size_t)tx;
    nb_bin[o] = tx < lc ? li : -1;
    nb_dist[o] = tx < lc ? ld : kInf;
}

// chb_bin_report: one chunk's dist[nq][B] and bin[nq] folded into the B x B tables keyed (the row's own label, bin).
//
// The chunk's positions are grouped by label (the host sorts them), seg names each label's run.  One workgroup owns
// (one run) x (64 consecutive bins), lane = bin: a row's 64 distances are one 512-byte read.  The run is cut into blocks
// of kReportBlock rows; wavefront w sums blocks w, w + 4, ... each in row order in a register (eight rows' loads are
// issued ahead of the eight dependent adds), and after every round of four blocks the first wavefront adds the round's
// block sums, in block order, onto the table's running sum.  So dsum[a][b] is: the finite distances of label a's rows in
// the host's order, blocks of kReportBlock consecutive rows of the label summed in order from 0, the block sums added in
// order from 0 -- whatever the chunks were, since a run starts on a block boundary of its label (BinReportArgs).
// Counts, minima and the confusion counts (rows whose bin[q] is the lane's bin) do not depend on any order.
// A (label, bin) cell is touched by one lane of one workgroup of a launch and the launches of a call follow each other on
// one stream: the tables are updated by plain loads and stores, there is no atomic of any kind.
__global__ __launch_bounds__(256) void bin_report_kernel(BinReportArgs a, int nbt)
{
    __shared__ double part[2][4][64];
    __shared__ double wmin[4][64];
    __shared__ int wcnt[4][64], wconf[4][64], wunp[4];

    const int sg = (int)blockIdx.x / nbt, bt = (int)blockIdx.x - sg * nbt;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int2 s0 = a.seg[sg];
    const int lab = s0.x, r0 = s0.y, r1 = a.seg[sg + 1].y;
    const int b = bt * 64 + lane;
    const bool on = b < a.B;
    const size_t B = (size_t)a.B;
    const double *col = a.dist + (on ? b : a.B - 1);   // (a lane past the last bin reads the last bin and stores nothing)
    const size_t cell = (size_t)lab * B + (size_t)b;
    const int nblk = (r1 - r0 + kReportBlock - 1) / kReportBlock;

    double total = (w == 0 && on) ? a.dsum[cell] : 0.0;
    double mn = kInf;
    int cnt = 0, conf = 0, unp = 0;
    auto fold = [&](double d, int bn, double &s) {
        conf += bn == b;
        unp += bn < 0;
        if (d < kInf) { ++cnt; mn = fmin(mn, d); s = s + d; }
    };
    for (int t0 = 0; t0 < nblk; t0 += 4) {
        const int t = t0 + w;
        double s = 0.0;
        if (t < nblk) {
            const int q1 = min(r0 + (t + 1) * kReportBlock, r1);
            int q = r0 + t * kReportBlock;
            for (; q + 8 <= q1; q += 8) {
                double d[8];
                int bn[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { d[u] = col[(size_t)(q + u) * B]; bn[u] = a.bin[q + u]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) fold(d[u], bn[u], s);
            }
            for (; q < q1; ++q) fold(col[(size_t)q * B], a.bin[q], s);
        }
        const int pb = (t0 >> 2) & 1;   // (two buffers: the first wavefront may still read round r while round r + 1 is written)
        part[pb][w][lane] = s;
        __syncthreads();
        if (w == 0) {
            const int nb = min(4, nblk - t0);
            for (int i = 0; i < nb; ++i) total = total + part[pb][i][lane];
        }
    }
    wmin[w][lane] = mn; wcnt[w][lane] = cnt; wconf[w][lane] = conf;
    if (lane == 0) wunp[w] = unp;
    __syncthreads();
    if (w != 0 || !on) return;
#pragma unroll
    for (int i = 1; i < 4; ++i) { mn = fmin(mn, wmin[i][lane]); cnt += wcnt[i][lane]; conf += wconf[i][lane]; unp += wunp[i]; }
    a.dsum[cell] = total;
    if (cnt) { a.cnt[cell] += cnt; a.dmin[cell] = fmin(a.dmin[cell], mn); }
    if (conf) a.conf[cell] += conf;
    if (b == 0 && unp) a.unplaced[lab] += unp;
}

__global__ __launch_bounds__(256) void fill_f64_kernel(double *p, double v, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace

void launch_bin_report(const BinReportArgs &a, hipStream_t s)
{
    if (a.nseg <= 0 || a.B <= 0) return;
    const int nbt = (a.B + 63) / 64;
    hipLaunchKernelGGL(bin_report_kernel, dim3((unsigned)a.nseg * (unsigned)nbt), dim3(256), 0, s, a, nbt);
}

void launch_fill_f64(double *p, double v, size_t n, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(fill_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, v, n);
}

void launch_recruit(const RecruitArgs &a, hipStream_t s)
{
    if (a.nq <= 0 || a.B <= 0) return;
    const int nqt = (a.nq + kQTile - 1) / kQTile;
    const int total = nqt * a.B;
    const int grid = ((total + 7) / 8) * 8;
    if (a.mmask) {   // a list of m: one slice of dist per entry
        if (a.qid) hipLaunchKernelGGL((recruit_kernel<true, true, false>), dim3(grid), dim3(256), 0, s, a, nqt, total);
        else hipLaunchKernelGGL((recruit_kernel<false, true, false>), dim3(grid), dim3(256), 0, s, a, nqt, total);
        return;
    }
    if (a.qid) hipLaunchKernelGGL((recruit_kernel<true, false, false>), dim3(grid), dim3(256), 0, s, a, nqt, total);
    else hipLaunchKernelGGL((recruit_kernel<false, false, false>), dim3(grid), dim3(256), 0, s, a, nqt, total);
}

// one work item per row of the tile table (a list of m with a.mmask)
void launch_recruit_pairs(const RecruitPairArgs &a, hipStream_t s)
{
    if (a.nq <= 0 || a.ntile <= 0) return;
    const int grid = ((a.ntile + 7) / 8) * 8;
    if (a.mmask) {   // a list of m: one slice of a.nq doubles per entry
        if (a.qid) hipLaunchKernelGGL((recruit_kernel<true, true, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
        else hipLaunchKernelGGL((recruit_kernel<false, true, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
        return;
    }
    if (a.qid) hipLaunchKernelGGL((recruit_kernel<true, false, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
    else hipLaunchKernelGGL((recruit_kernel<false, false, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
}

// the leave-group-out instantiations: the dense grid (a.tile null) or the tile table, either with a list of m (a.mmask)
void launch_recruit_grouped(const RecruitGroupArgs &a, hipStream_t s)
{
    if (a.tile) {
        if (a.nq <= 0 || a.ntile <= 0) return;
        const int grid = ((a.ntile + 7) / 8) * 8;
        if (a.mmask) hipLaunchKernelGGL((recruit_kernel<true, true, true, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
        else hipLaunchKernelGGL((recruit_kernel<true, false, true, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
        return;
    }
    if (a.nq <= 0 || a.B <= 0) return;
    const int nqt = (a.nq + kQTile - 1) / kQTile;
    const int total = nqt * a.B;
    const int grid = ((total + 7) / 8) * 8;
    if (a.mmask) hipLaunchKernelGGL((recruit_kernel<true, true, false, true>), dim3(grid), dim3(256), 0, s, a, nqt, total);
    else hipLaunchKernelGGL((recruit_kernel<true, false, false, true>), dim3(grid), dim3(256), 0, s, a, nqt, total);
}

// the pair kernels that also store every position's witness record
void launch_recruit_witness(const RecruitWitnessArgs &a, hipStream_t s)
{
    if (a.nq <= 0 || a.ntile <= 0) return;
    const int grid = ((a.ntile + 7) / 8) * 8;
    if (!a.qid) hipLaunchKernelGGL((recruit_kernel<false, false, true, false, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
    else if (a.memb_grp) hipLaunchKernelGGL((recruit_kernel<true, false, true, true, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
    else hipLaunchKernelGGL((recruit_kernel<true, false, true, false, true>), dim3(grid), dim3(256), 0, s, a, 0, a.ntile);
}

void launch_recruit_reduce(const double *dist, int nq, int B, int *bin, double *mind, double *margin, hipStream_t s)
{
    if (nq <= 0) return;
    hipLaunchKernelGGL(recruit_reduce_kernel, dim3((nq + 31) / 32), dim3(256), 0, s, dist, nq, B, bin, mind, margin);
}

void launch_nearest_bins(const double *dist, int nq, int B, int k, int *nb_bin, double *nb_dist, hipStream_t s)
{
    if (nq <= 0 || B <= 0 || k <= 0) return;
    hipLaunchKernelGGL(nearest_bins_kernel, dim3((nq + 15) / 16), dim3(256), 0, s, dist, nq, B, k, nb_bin, nb_dist);
}

}  // namespace chb
