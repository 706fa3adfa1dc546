// What the units of the host code of libchbin_hip.so (chb_api.hip, chb_queries.hip, chb_features.hip) share: the buffer
// types, every state struct up to chb_ctx, Timed, and -- at the end -- the functions that one section of the host code
// defines and another calls.  Everything else of a unit stays in its anonymous namespace or static.
#pragma once
#include "chb_internal.h"
#include "../../include/chbin_hip.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <string>
#include <unordered_set>
#include <vector>

using namespace chb;

namespace chb {

// RCCL is resolved at run time (dlopen) so that the library neither forces a second copy of RCCL
// into a process that already has one (PyTorch bundles its own) nor needs it for single-GPU use.
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};

#define NCCLCHK(expr)                                                                      \
    do {                                                                                   \
        ncclResult_t r_ = (expr);                                                          \
        if (r_ != ncclSuccess)                                                             \
            return fail(CHB_EHIP, std::string(#expr) + ": " + rccl()->GetErrorString(r_)); \
    } while (0)

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(CHB_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

// (in a function that returns the hipError_t itself)
#define HIPTRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

struct ProfEntry {
    double ms = 0.0;
    int64_t launches = 0;
    double work = 0.0;
};

struct Pending {
    hipEvent_t a, b;
    std::string name;
    double work;
};

// A buffer that frees itself: device memory (DevBuf), or pinned host staging (PinBuf; labels, permutations: asynchronous
// copies at DMA speed instead of the driver's bounce-buffer path for pageable memory)
template <typename T, bool kPinned>
struct Buf {
    T *p = nullptr; size_t cap = 0;
    hipError_t ensure(size_t n)
    {
        if (n <= cap) return hipSuccess;
        release();
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        hipError_t e = kPinned ? hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) : hipMalloc((void **)&p, bytes);
        if (e == hipSuccess) cap = n;
        return e;
    }
    hipError_t ensure_zeroed(size_t n, hipStream_t s)   // (all of it zeroed on s whenever this allocated or grew it)
    {
        const size_t had = cap;
        const hipError_t e = ensure(n);
        return (e != hipSuccess || cap == had) ? e : hipMemsetAsync(p, 0, sizeof(T) * cap, s);
    }
    void release() { if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
    Buf() = default; Buf(const Buf &) = delete; Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinBuf = Buf<T, true>;

// A device buffer and its pinned twin on the host (the row-scoring calls' chunks: what goes up, what comes down)
template <typename T>
struct Mirror {
    DevBuf<T> d;
    PinBuf<T> h;
    hipError_t ensure(size_t n, bool want_host)   // (the host side only where somebody will read or fill it)
    {
        HIPTRY(d.ensure(n));
        return want_host ? h.ensure(n) : hipSuccess;
    }
    hipError_t up(size_t n, hipStream_t s) { return hipMemcpyAsync(d.p, h.p, sizeof(T) * n, hipMemcpyHostToDevice, s); }
    hipError_t down(size_t n, hipStream_t s) { return hipMemcpyAsync(h.p, d.p, sizeof(T) * n, hipMemcpyDeviceToHost, s); }
};

// device storage behind a MemberPack
struct PackBufs {
    DevBuf<unsigned short> Z;
    DevBuf<float> bias, sn, cs, cb, bb, tsn;   // (bias / sn / cs / cb: the batch-entry pack's per-row columns)
    DevBuf<int> pad_ptr;
    hipError_t ensure(size_t rows, size_t B, size_t Dz)
    {
        hipError_t e;
        if ((e = Z.ensure((rows + 64) * Dz)) != hipSuccess) return e;   // + slack: whole 32-row tiles are read
        DevBuf<float> *f[] = {&bias, &sn, &cs, &cb};
        for (auto *b : f) if ((e = b->ensure(rows + 64)) != hipSuccess) return e;
        if ((e = bb.ensure(4 * B)) != hipSuccess) return e;
        if ((e = tsn.ensure(rows / 32 + B + 68)) != hipSuccess) return e;   // (+ 64: the tile-skipping kernel reads 64 at a time)
        return pad_ptr.ensure(B + 1);
    }
    chb::MemberPack view()
    {
        return chb::MemberPack{Z.p, bias.p, sn.p, cs.p, cb.p, tsn.p, pad_ptr.p, reinterpret_cast<float4 *>(bb.p)};
    }
};

// The product's switches (include/chbin_hip.h; read_switches): each selects a slower, independent formulation of the same
// result for the tests' A/B checks.  (A multi-rank fit may turn speculate, allow_skip, pp_allowed off for itself.)
struct Switches {
    bool use_prefilter = true;    // CHB_PREFILTER=0: brute-force fp64 selection instead of the fp16 shortlist stage
    bool allow_fused = true;      // CHB_FUSED=0: m <= 16 also takes the list-based path (exact rescoring, then the hull kernel)
    bool fused_ptr64 = false;     // CHB_FUSED_PTR64=1: 64-bit row pointers in the m <= 5 fused kernel whatever the size of X
    bool speculate = true;        // CHB_SPECULATE=0: never enqueue the next batch ahead of the convergence test
    bool force_gather = false;    // CHB_FORCE_GATHER=1: run the exchange path even with one rank (tests)
    bool allow_segments = true;   // CHB_SEGMENTS=0: never (A/B tests)
    bool fused_stripe = true;     // CHB_FUSED_STRIPE=0: position-major work order in the fused kernels
    bool fused_trim = true;       // CHB_FUSED_TRIM=0: the m <= 5 fused kernel gathers every candidate of a wide shortlist
    bool pp_allowed = true;       // CHB_PACK_INCR=0: every batch start rebuilds CSR and pack (the form up to round 3; A/B tests)
    bool pool_allowed = true, pool_force = false;   // CHB_POOL_TAU=0: a bin always streamed twice; =2: pools whatever the size
    bool allow_skip = true;       // CHB_TILE_SKIP=0: never (A/B tests)
};

// ---- the context's parts: each feature owns its buffers, host flags, verdict on the running fit, statistics and view for
// the kernels.  fit_reset: what a fit's start resets; fit_scope: what holds inside a chb_fit_cluster_ex call only (FitScope).

// The persistent base pack (prefilter_kernels.hip): the member pack kept across the batches of a fit
struct PersistentPack {
    DevBuf<int> start, cap, fill, live, nt, fill0, start0, memb, row, ctl, ovf, dest;
    int arena_rows = 0;
    int64_t mark = 0;       // rows handed out from which on the host asks for a rebuild (pack_state_build)
    bool fit = false;       // inside chb_fit_cluster (the stepwise entry points and chb_topm_per_bin always rebuild)
    bool valid = false;     // the pack on the device matches the labels
    bool batch = false;     // the open batch was started on it
    bool rebuild = false;   // much of the arena is used up: the next batch start outside a look-ahead window rebuilds
    int64_t stat_batches = 0, stat_builds = 0;
    chb::PackState view() { return chb::PackState{start.p, cap.p, fill.p, live.p, nt.p, fill0.p, start0.p, memb.p, row.p, ctl.p, ovf.p, dest.p, arena_rows}; }
    void fit_reset() { valid = false; batch = false; rebuild = false; }
    void fit_scope(bool in) { fit = in; if (in) { stat_batches = 0; stat_builds = 0; } else valid = false; }
};

// Threshold pools of the shortlist stage (prefilter_kernels.hip, "threshold pools"): for every (bin, home bin) the 32
// base members of the bin nearest to the home bin's centre; built at a fit's start, maintained by every commit
struct ThresholdPools {
    DevBuf<unsigned short> Z;
    DevBuf<int> id, hole, ok, bad;
    DevBuf<float> key, sn, tsn;
    bool fit = false;      // inside chb_fit_cluster (the stepwise entry points and chb_topm_per_bin never use pools)
    bool valid = false;    // the pools on the device match the labels
    bool kept = false;     // ... and did when the last fit ended (what the counter pool_bad_slots looks at)
    bool batch_labelled = true;   // the batch about to be opened may hold labelled samples (the fit loop knows; else: true)
    bool holes = true;     // the open batch may hold labelled samples (their pool slots are holes until the commit)
    int state = 0;         // this fit: 0 undecided = on, 1 kept on, -1 off (its shortlists came out long: overlapping bins;
                           // or tile skipping never loads more than 30 % of the tiles: FitRun::note_verdict has both rules)
    int batches = 0;
    long long cand = 0, pairs = 0;
    long long off_key = -1;   // (bins, neighbours, metric) of the fit that turned them off on these samples
    int64_t stat_batches = 0;
    chb::PoolState view() { return chb::PoolState{Z.p, id.p, key.p, sn.p, hole.p, tsn.p, ok.p}; }
    void release() { Z.release(); id.release(); hole.release(); key.release(); sn.release(); tsn.release(); ok.release(); }
    void fit_reset(bool off) { stat_batches = 0; state = off ? -1 : 0; batches = 0; cand = 0; pairs = 0; }
    void fit_scope(bool in) { fit = in; kept = !in && valid; batch_labelled = true; if (!in) valid = false; }
};

// Tile skipping in the base shortlist launch, and the queries' seats it and the pools need
struct Seating {
    // shells: the CSR of the base members is keyed (bin, shell of the member's distance from the bin's centre), outermost
    // shell first, so that the rows of a 32-row tile have similar norms (tile skipping in the shortlist kernel)
    DevBuf<float> shell_inv;
    int nsh = 1;
    // tile skipping (needs the shells above and queries seated by nearest bin centre): nearest-centre keys, the seating
    // order, and the fit's verdict on whether it pays (0 undecided = on, 1 on, -1 off)
    DevBuf<unsigned long long> ckey;
    DevBuf<int> qord, home;
    // (the fit loop orders the positions of ALL batches of a sweep in one launch; the open batch's part: qord_cur / home_cur)
    DevBuf<int> qord_all, home_all;
    DevBuf<int4> geo_all;
    PinBuf<int4> pin_geo;
    int *qord_cur = nullptr, *home_cur = nullptr;
    int state = 0, batches = 0;
    long long off_key = -1;   // (bins, neighbours, metric) of the fit that found nothing to skip on these samples
    long long skipped = 0, seen = 0, unloaded = 0;
    void fit_reset(bool off) { state = off ? -1 : 0; batches = 0; skipped = 0; seen = 0; unloaded = 0; }
    void unseat() { qord_cur = nullptr; home_cur = nullptr; }   // (no sweep-wide seating: a sweep's start, a fit's end)
};

// Bins far larger than the rest are cut into segments for the shortlist stage (SegPlan, prefilter_kernels.hip): plan
// buffers, and the bin sizes last seen by the host (they come home with the rounds' verdicts)
struct Segments {
    DevBuf<int> nseg, gflag;
    DevBuf<int4> items;
    DevBuf<float> lists;
    int gcap = 0;
    int hint_max_tiles = 0, hint_total_tiles = 0;
    int64_t stat_batches = 0;   // batches of the last fit that ran the segment launches
};

// One half of the row-scoring calls' double buffer: a chunk of the new rows (padded like X) or of sample indices (qid), its
// distances and row reductions, each a Mirror: on the device (.d) and pinned on the host (.h); chb_bin_report's chunks also
// carry seg, each label's run (BinReportArgs), nseg of them; the pair calls' chunks carry tile, the chunk's tile table
// (RecruitPairArgs), ntile rows.
// up / done / down: the upload, the kernels, the download of the chunk in this half are through.
struct ChunkHalf {
    Mirror<double> Y, dist, min, margin;
    Mirror<int> bin, qid;
    Mirror<int2> seg;
    Mirror<int4> tile;
    // the witness calls only (first allocated by the context's first such call): the chunk's witness records, a call-wide
    // number of slots per position (ScoreRun::wslots) -- kWitnessSlots up to 16 neighbours (RecruitWitnessArgs), m beyond
    // (RecruitWideWitnessArgs), where the members' ids are wlist's and wid stays unused
    Mirror<int> wid;
    Mirror<double> wd, walpha;
    // chb_*_rows_nearest only (first allocated by the context's first such call): the chunk's k nearest bins per row and
    // their distances
    Mirror<int> nbin;
    Mirror<double> ndist;
    // the pair calls with more than 16 neighbours only (first allocated by the context's first such call): the chunk's
    // selection lists, m + 1 ints per position (RecruitWideArgs), per half because idx_out copies them down while the next
    // chunk's kernels run
    Mirror<int> wlist;
    hipEvent_t up = nullptr, done = nullptr, down = nullptr;
    int nseg = 0, ntile = 0;
    void destroy_events() { for (hipEvent_t ev : {up, done, down}) if (ev) (void)hipEventDestroy(ev); }
};

// Every row-scoring call (ScoreRun): the calls' own buffers, nothing of a fit.
// While the kernels of chunk k run on the context's stream, copy brings chunk k + 1 up into the other half and chunk
// k - 1 down.  Not per half: the call's CSR over the labels (ptr, memb) and chb_bin_report's B x B tables rep_* (zeroed at
// the call's start), which collect what the chunks' rows say.  The chb_*_grouped calls add the dense group ids: grp of
// every resident sample, mgrp parallel to memb.
struct RowScoring {
    ChunkHalf half[2];
    DevBuf<int> ptr, memb, mgrp, grp;
    PinBuf<int> hptr, hmemb, hmgrp, hgrp;
    DevBuf<long long> rep_conf, rep_unplaced, rep_cnt;
    DevBuf<double> rep_min, rep_sum;
    hipStream_t copy = nullptr;
    int64_t multi_rows = 0;   // rows per launch of the last chb_audit_rows_multi / chb_recruit_rows_multi
    int64_t pair_tiles = 0;   // tiles (work items) of the last chb_audit_pairs / chb_recruit_pairs
    // the dense wide calls (16 < m <= 64): the selection lists of one chunk, rows x B x (m + 1) ints within kWideListBytes
    // (one buffer: a chunk's kernels follow the previous chunk's on the stream and nothing copies it down); first
    // allocated by the context's first such call
    DevBuf<int> wlist;
    int64_t wide_rows = 0;    // rows per launch of the last wide call
};

// Multi-GPU: one context per process per GPU, RCCL communicator over all ranks
struct Exchange {
    ncclComm_t comm = nullptr;
    // host-staged exchange (chb_comm_init_hook): the same sharded loop with the all-gathers done by a
    // caller-supplied function on host buffers -- MPI, gloo, pipes; also how two ranks can share one GPU
    chb_allgather_fn hook = nullptr;
    void *hook_user = nullptr;
    std::vector<char> send, recv;
    DevBuf<int> agree;   // chb_bcast_samples: {status, N, D, root} of every rank; chb_fit_cluster: the fit's agreement table
    // framed exchange of the sharded loop (aux_kernels.hip: xchg_pack / xchg_unpack): every rank's {header, label slice},
    // the number of the fit's next exchange (part of the tag every frame carries), and the device's "a rank was out of
    // step" record {flag, my tag, its tag, rank}
    DevBuf<int> xg, xerr;
    int seq = 0;
};

struct Profile {
    int level = 0;   // 0 off, 1 every kernel, 2 only the two dominant ones (cheap enough for a timed region)
    std::map<std::string, ProfEntry> acc;
    std::vector<Pending> pending;
};

// What describes the open batch on the host.  LookaheadSnap saves and restores it by copy: anything added here is put
// back as it was after a failed look-ahead.
struct BatchState {
    int K = 0, q_lo = 0, q_hi = 0;
    int round_in_batch = 0;     // rounds alternate between the list sets 1 and 2 (the other = previous)
    bool lists_valid = false;   // the open batch was started with need_lists (chb_topm_per_bin)
    bool open = false;
    int *bq_cur = nullptr;      // the open batch's sample indices: bq.p, or a window of perm (no copy)
    int *fc_cur = nullptr;      // slot of the open batch (first_change.p + 0 / kSlotInts), words as SlotWord names them: bin sizes, skip /
                                // pool statistics and the pack's fill mark ride home with the verdict in one copy of kSlotHome ints
    double hint_base_members = 0.0, hint_batch_entries = 0.0;   // work-unit hints for the profile (pairs = queries x members streamed)
};

}  // namespace chb

struct chb_ctx {
    int dev = 0;
    Switches sw;
    hipStream_t stream = nullptr;
    int rank = 0, world = 1;
    PersistentPack pp;
    ThresholdPools pool;
    Seating seat;
    Segments seg;
    RowScoring score;
    Exchange xchg;
    Profile prof;
    BatchState batch;
    // samples
    DevBuf<double> X;
    int64_t N = 0;
    int D = 0, Dp = 0;
    // fit state
    int B = 0, m = 0;
    int metric = 0;   // CHB_METRIC_CONVEX / CHB_METRIC_AFFINE
    bool fit_open = false;
    bool stepwise = false;   // the open fit was begun by chb_fit_begin (the caller drives its batches): chb_recruit_rows / chb_audit_rows refuse
    DevBuf<int> labels, inb;
    // batch buffers (the open batch itself: `batch`)
    int Kcap = 0;
    DevBuf<int> bq, lab_old, lab_prev, lab_new, first_change;
    int *fc_host = nullptr;     // pinned landing places of the two verdict slots (kSlotInts ints each, as on the device)
    hipEvent_t fc_event[2] = {nullptr, nullptr};
    bool argmin_in_place = false;   // chb_fit_cluster without exchange: argmin also stores the label to lab_prev
    DevBuf<double> mind, mind2, dist;   // winning hull distance, runner-up (margin report), all distances
    bool want_margin = false;
    DevBuf<double> l0d, l1d, l2d;
    DevBuf<int> l0i, l1i, l0c, l1c, l2i, l2c;
    int64_t round_active = 0; // `active` of the open batch's last chb_batch_round: may not decrease (include/chbin_hip.h)
    DevBuf<int> cnt, bin_ptr, cursor, memb_id;
    DevBuf<int> cnt2, bin_ptr2, cursor2, memb2_id, memb2_code;
    DevBuf<int> perm;
    PinBuf<int> pin_a, pin_b, pin_c;   // host staging: labels in, labels out, permutation
    // two-stage selection: fp16 shadow copies + shortlists (prefilter_kernels.hip)
    DevBuf<unsigned short> Gs, Zs;     // per sample: query-side row (global centre), member-side row (own bin)
    DevBuf<float> gq, ms;              // per sample: float2 {||qh||^2, rho}, float4 {bias, rho, ||zh||^2, amax}
    DevBuf<double> mu_g, colsum_part;  // global mean, scratch of its two-pass sum
    DevBuf<unsigned int> rmax;
    double shadow_scale = 1.0;         // S
    PackBufs pk, pk2;                  // padded member packs: base members, the batch's own entries
    DevBuf<float> qn;                  // [N][B] float2 exact sample-to-centre norms (per fit)
    DevBuf<double> centers;
    int Dz = 0;
    bool shadow_ok = false, overflow_total_valid = false;
    DevBuf<int> cand, cand_cnt, flags64, flaglist, nflag, overflow;
    DevBuf<int> flaglist2, nflag2;   // what the second-chance launch of a pool batch leaves for the brute-force kernel
    DevBuf<int> active, n_active, act_blk;
    // fused selection + hull distance (m <= 16): batch-entry candidates of this / the previous round,
    // the base stage's tau (bound of the m-th nearest distance), the exact path's work list
    bool fused = false;
    bool pf_fit = false;        // this fit uses the shortlist stage (use_prefilter, D <= 160, m <= 16)
    DevBuf<int> candu[2], candu_cnt[2], slow, n_slow;
    DevBuf<float> tau;
    // the shortlist stage's contract as checked by the fused kernels (FusedArgs::short_cnt): pairs of this fit whose base
    // shortlist held fewer than min(m, bin size) candidates or a wild index -- any is an internal error of the fit
    DevBuf<int> short_cnt;
    // the m <= 5 fused kernel's trim (FusedArgs::trim_ctr): pairs trimmed in this fit, their candidates before and after
    DevBuf<unsigned long long> trim_ctr;
    DevBuf<TrimArgs> trim_args;   // (written with the global shadows: samples_finish)
    // scratch for the indexed / explicit-point entry points
    DevBuf<int> xq, xhull, xcnt;
    DevBuf<double> xdist, xalpha, xpts;
    // the last fit: chb_fit_stats, its speculative batch size, batches whose successor was enqueued ahead of their verdict
    // and kept, ... and discarded (the batch needed further rounds)
    std::array<int64_t, 4> stats{};
    long long last_batch = 0;
    int64_t stats_lookahead = 0, stats_lookahead_failed = 0;
    int64_t kmer_chunks = 0;   // sequence chunks of the last chb_kmer_profiles / chb_set_samples_from_sequences call
#ifdef CHB_DEV_KNOBS
    // developer builds: the switches of the tests and tools/ (read_switches; the Makefile says what each does), their state
    struct DevKnobs {
        bool sl_bounds = false, sl_validate = false;                            // CHB_SL_BOUNDS, CHB_SL_VALIDATE
        int inject_short = 0, sl_bpw = 0, skip_never = 0;                       // CHB_SL_INJECT_SHORT, CHB_SL_BPW, CHB_SKIP_NEVER
        std::string sl_dbg;                                                     // CHB_SL_DBG
        int64_t pack_rebuild_at = -1;                                           // CHB_PACK_REBUILD_AT (-1: unset)
        bool hook_spec = false, local_verdict = false, skip_stats_on = false;   // CHB_DEV_HOOK_SPEC, CHB_DEV_LOCAL_VERDICT,
        int skip_stats[3] = {0, 0, 0};                                          // CHB_DEV_SKIP_STATS
        int batches = 0, launches = 0;   // batch starts (CHB_SL_INJECT_SHORT), base shortlist launches (CHB_SL_DBG) so far
        DevBuf<int> viol, verr;          // first out-of-range access; validation error + per-position counters
        DevBuf<unsigned long long> dbg;  // the timeline
    } dk;
#endif

    Lists L0() { return Lists{l0d.p, l0i.p, l0c.p}; }
    Lists L1() { return Lists{l1d.p, l1i.p, l1c.p}; }
    Lists L2() { return Lists{l2d.p, l2i.p, l2c.p}; }
    Lists Lcur() { return (batch.round_in_batch & 1) ? L2() : L1(); }
    Lists Lprev() { return (batch.round_in_batch & 1) ? L1() : L2(); }

    // The kernels' argument blocks for the positions [lo, hi) of the open batch, with the fields that every launch of a
    // kind shares; a call site adds only what makes it different, and what nobody sets stays zero.
    TopmArgs topm_args(int lo, int hi)
    {
        TopmArgs a{};
        a.X = X.p; a.Dp = Dp; a.bq = batch.bq_cur; a.pos_begin = lo; a.pos_end = hi; a.B = B; a.m = m; a.Kcap = Kcap;
        return a;
    }
    // (query side, geometry, scale, overflow counter, the brute-force kernel's work list -- its counter reset by the CSR kernels)
    ShortlistArgs shortlist_args(int lo, int hi)
    {
        ShortlistArgs a{};
        a.Gs = Gs.p; a.gq = reinterpret_cast<const float2 *>(gq.p); a.qn = reinterpret_cast<const float2 *>(qn.p);
        a.Dz = Dz; a.S = shadow_scale; a.bq = batch.bq_cur; a.pos_begin = lo; a.pos_end = hi; a.B = B; a.m = m; a.Kcap = Kcap;
        a.overflow = overflow.p; a.flaglist = flaglist.p; a.nflag = nflag.p;
        return a;
    }
    RescoreArgs rescore_args(int lo, int hi)   // (candidates: the base shortlists)
    {
        RescoreArgs a{};
        a.X = X.p; a.Dp = Dp; a.bq = batch.bq_cur; a.pos_begin = lo; a.pos_end = hi; a.B = B; a.m = m; a.Kcap = Kcap;
        a.cand = cand.p; a.cand_cnt = cand_cnt.p; a.cand_cap = kCandCap;
        return a;
    }
    QpArgs qp_args(int lo, int hi)
    {
        QpArgs a{};
        a.X = X.p; a.D = D; a.Dp = Dp; a.bq = batch.bq_cur; a.pos_begin = lo; a.pos_end = hi; a.B = B; a.m = m; a.Kcap = Kcap;
        a.dist = dist.p; a.metric = metric;
        return a;
    }
    FusedArgs fused_args(int lo, int hi)
    {
        FusedArgs a{};
        a.X = X.p; a.n_samples = N; a.D = D; a.Dp = Dp; a.bq = batch.bq_cur; a.pos_begin = lo; a.pos_end = hi;
        a.B = B; a.m = m; a.Kcap = Kcap; a.dist = dist.p; a.metric = metric;
        // (the trim sweeps one 160-column slice of the global shadows at the most)
        if (sw.fused_trim && shadow_ok && Dz <= 160 && D + 3 <= 160) a.trim = trim_args.p;
        return a;
    }
};

namespace chb {

struct Timed {
    chb_ctx *h;
    Pending p;
    bool on;
    Timed(chb_ctx *h_, const char *name, double work)
        : h(h_), on(h_->prof.level == 1 || (h_->prof.level == 2 && (!strcmp(name, "prefilter") || !strcmp(name, "hull_qp"))))
    {
        if (!on) return;
        p.name = name; p.work = work;
        (void)hipEventCreate(&p.a);
        (void)hipEventCreate(&p.b);
        (void)hipEventRecord(p.a, h->stream);
    }
    ~Timed()
    {
        if (!on) return;
        (void)hipEventRecord(p.b, h->stream);
        h->prof.pending.push_back(p);
    }
};

// ---- the functions that cross between the sections of the host code (all of them defined in chb_api.hip)
// the context: the thread's error text (fail returns code), the RCCL loader (null: none), what a context owns
int fail(int code, const std::string &msg);
RcclApi *rccl();
int exchange_all_gather(chb_ctx *h, void *buf, size_t count, size_t elem, ncclDataType_t dt);
void drain_profile(chb_ctx *h);
void read_switches(chb_ctx *h);
int set_samples_common(chb_ctx *h, const double *X, int64_t N, int64_t D, bool from_device);
// the batch stages: a fit's start and the three steps of a batch on the device
long long skip_key(const chb_ctx *h);
int ensure_batch_buffers(chb_ctx *h, int Kcap);
int fit_begin_impl(chb_ctx *h, int64_t B, const int64_t *initial, int m, bool sync = true);
int pool_build(chb_ctx *h);
int batch_begin_dev(chb_ctx *h, int K, int q_lo, int q_hi, bool need_lists);
int batch_round_dev(chb_ctx *h, int active);
int batch_commit_dev(chb_ctx *h, const int *final_dev);

}  // namespace chb
