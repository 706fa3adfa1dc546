// Host side of libchbin_hip.so: the C ABI declared in include/chbin_hip.h.
//
// The fit loop reproduces algorithm.py:37-76 exactly -- including the in-place (Gauss-Seidel)
// label updates -- while evaluating K contigs at a time:
//
//   batch = K consecutive positions of the sweep's permutation.
//   T0(j,c): the m nearest members of bin c among samples OUTSIDE the batch (labels frozen at batch
//            start).  One heavy launch per batch (topm_base).
//   round r: every position j takes, for each bin c, T0(j,c) merged with the batch members that
//            belong to c when j is visited: EARLIER positions under their label of round r-1,
//            LATER positions under their pre-batch label (they have not been visited yet).
//            Then hull distances, strict-'>' argmin (algorithm.py:57), giving label_r.
//   Let f = first position with label_r != label_{r-1}.  Positions <= f were computed from labels
//   that can no longer change, hence are final; the next round only re-evaluates positions > f.
//   No change (f = K) means label_r is the unique fixed point = the sequential result.
// In sweep 1 the pre-batch labels of the batch are all -1; in later sweeps they are last sweep's
// labels and a batch typically converges in one round.
#include "chb_host.h"

namespace {

thread_local std::string g_err;

}  // namespace

namespace chb {

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

RcclApi *rccl()
{
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.ok ? &api : nullptr;
    tried = true;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) {
        api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);   // a copy already in the process
        if (api.lib) break;
    }
    if (!api.lib)
        for (const char *n : names) {
            api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (api.lib) break;
        }
    if (!api.lib) return nullptr;
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
    api.AllGather = (decltype(api.AllGather))dlsym(api.lib, "ncclAllGather");
    api.Broadcast = (decltype(api.Broadcast))dlsym(api.lib, "ncclBroadcast");
    api.CommCount = (decltype(api.CommCount))dlsym(api.lib, "ncclCommCount");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather && api.GetErrorString &&
             api.Broadcast && api.CommCount;
    return api.ok ? &api : nullptr;
}

// In-place all-gather of `count` elements per rank inside the device buffer `buf` (rank r's slice sits at
// buf + r * count): RCCL on the context's stream, or the host-staged hook.
int exchange_all_gather(chb_ctx *h, void *buf, size_t count, size_t elem, ncclDataType_t dt)
{
    char *b = static_cast<char *>(buf);
    if (h->xchg.hook != nullptr) {
        const size_t bytes = count * elem;
        h->xchg.send.resize(bytes);
        h->xchg.recv.resize(bytes * (size_t)h->world);
        HIPCHK(hipMemcpyAsync(h->xchg.send.data(), b + (size_t)h->rank * bytes, bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->xchg.hook(h->xchg.hook_user, h->xchg.send.data(), h->xchg.recv.data(), bytes) != 0)
            return fail(CHB_EHIP, "the exchange hook reported a failure");
        HIPCHK(hipMemcpyAsync(b, h->xchg.recv.data(), bytes * (size_t)h->world, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));   // (hook_recv is reused by the next exchange)
        return CHB_OK;
    }
    NCCLCHK(rccl()->AllGather(b + (size_t)h->rank * count * elem, b, count, dt, h->xchg.comm, h->stream));
    return CHB_OK;
}

void drain_profile(chb_ctx *h)
{
    for (auto &p : h->prof.pending) {
        (void)hipEventSynchronize(p.b);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, p.a, p.b);
        auto &e = h->prof.acc[p.name];
        e.ms += ms; e.launches += 1; e.work += p.work;
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    h->prof.pending.clear();
}

long long skip_key(const chb_ctx *h) { return (long long)h->B | ((long long)h->m << 32) | ((long long)h->metric << 40); }

int ensure_batch_buffers(chb_ctx *h, int Kcap)
{
    const size_t B = h->B, m = h->m, K = Kcap;
    const size_t Kpad = K + (size_t)h->world;   // allgather of ceil(K/world)-sized slices
    const size_t flag_tiles = B * ((K + kQTile - 1) / kQTile);   // (bin, query tile) flags of the shortlist stage's overflow
    HIPCHK(h->bq.ensure(K));
    HIPCHK(h->lab_old.ensure(K));
    HIPCHK(h->lab_prev.ensure(Kpad));
    HIPCHK(h->lab_new.ensure(Kpad));
    HIPCHK(h->first_change.ensure(2 * kSlotInts));
    h->batch.fc_cur = h->first_change.p;
    HIPCHK(h->xchg.xg.ensure(Kpad + (size_t)(kXchgHdr + 1) * (size_t)h->world));
    HIPCHK(h->xchg.xerr.ensure_zeroed(4, h->stream));
    HIPCHK(h->mind.ensure(Kpad));
    HIPCHK(h->mind2.ensure(Kpad));
    HIPCHK(h->dist.ensure(K * B));
    HIPCHK(h->l0d.ensure(K * B * m));
    HIPCHK(h->l1d.ensure(K * B * m));
    HIPCHK(h->l2d.ensure(K * B * m));
    HIPCHK(h->l2i.ensure(K * B * m));
    HIPCHK(h->l2c.ensure(K * B));
    HIPCHK(h->l0i.ensure(K * B * m));
    HIPCHK(h->l1i.ensure(K * B * m));
    HIPCHK(h->l0c.ensure(K * B));
    HIPCHK(h->l1c.ensure(K * B));
    HIPCHK(h->cnt.ensure_zeroed(B * (size_t)kShells, h->stream));
    HIPCHK(h->bin_ptr.ensure(B + 1));
    HIPCHK(h->cursor.ensure(B * (size_t)kShells));
    HIPCHK(h->memb_id.ensure((size_t)h->N));
    HIPCHK(h->cnt2.ensure(B));
    HIPCHK(h->bin_ptr2.ensure(B + 1));
    HIPCHK(h->cursor2.ensure(B));
    HIPCHK(h->memb2_id.ensure(2 * K));
    HIPCHK(h->memb2_code.ensure(2 * K));
    if (h->pf_fit) {
        HIPCHK(h->cand.ensure(K * B * (size_t)kCandCap));
        HIPCHK(h->cand_cnt.ensure(K * B));
        HIPCHK(h->active.ensure(K * B));
        HIPCHK(h->n_active.ensure(1));
        HIPCHK(h->act_blk.ensure((K * B + 4095) / 4096 + 1));
        HIPCHK(h->flags64.ensure(flag_tiles));
        HIPCHK(h->flaglist.ensure(flag_tiles));
        HIPCHK(h->nflag.ensure(1));
        HIPCHK(h->flaglist2.ensure(flag_tiles));
        HIPCHK(h->nflag2.ensure(1));
        launch_fill_i32(h->flags64.p, 0, (int)flag_tiles, h->stream);   // kept zero by its consumer
        HIPCHK(h->overflow.ensure(1));
        HIPCHK(h->pk.ensure((size_t)h->N + 32 * B, B, (size_t)h->Dz));
        HIPCHK(h->pk2.ensure(2 * K + 32 * B, B, (size_t)h->Dz));
        h->seg.gcap = (int)std::min<size_t>(64, B / 4 + 1);
        HIPCHK(h->seat.qord.ensure(K));
        HIPCHK(h->seat.home.ensure(B));
        HIPCHK(h->seg.nseg.ensure(1));
        HIPCHK(h->seg.gflag.ensure(B));
        HIPCHK(h->seg.items.ensure(16 * (size_t)h->seg.gcap));
        // (seg_lists -- giant slots x 16 segments x K x list length floats, 0.27 / 0.86 GB at 1M x 200 bins for m = 5 / 15 --
        //  is allocated by the first batch that really runs the segment launches: batch_begin_dev)
        if (h->fused) {
            for (int i = 0; i < 2; ++i) {
                HIPCHK(h->candu[i].ensure(K * B * (size_t)kCandCapU));
                HIPCHK(h->candu_cnt[i].ensure(K * B));
            }
            HIPCHK(h->slow.ensure(K * B));
            HIPCHK(h->n_slow.ensure(1));
            HIPCHK(h->short_cnt.ensure_zeroed(1, h->stream));
            HIPCHK(h->tau.ensure(K * B));
        }
    }
    h->Kcap = Kcap;
    return CHB_OK;
}

// sync = false (chb_fit_cluster): the uploads and kernels of the fit's start are only enqueued -- the caller goes on with
// its own host work (permutation check / conversion) while they run, and the stream orders everything behind them
int fit_begin_impl(chb_ctx *h, int64_t B, const int64_t *initial, int m, bool sync)
{
    if (!h->X.p) return fail(CHB_ESTATE, "chb_set_samples has not been called");
    if (B <= 0) return fail(CHB_EINVAL, "num_clusters must be positive");
    if (B > 8192) return fail(CHB_EUNSUPPORTED, "more than 8192 bins (per-block LDS histograms of the CSR build)");
    if (m < 1 || m > CHB_MAX_NEIGHBORS)
        return fail(CHB_EUNSUPPORTED, "num_neighbors must be in [1, 64]");
    if (m > kMaxM && !hull_generic_supported())
        return fail(CHB_EUNSUPPORTED, "num_neighbors > 16 needs 68 KB of LDS per workgroup, which this device does not grant");
    h->B = (int)B; h->m = m;
    // the fp16 shortlist stage and the tuned kernels hold lists of up to 16 entries; beyond that the plain
    // one-wavefront-per-problem kernels run (brute-force selection, LDS-resident solver)
    h->pf_fit = h->sw.use_prefilter && h->shadow_ok && m <= kMaxM;
    // (a fit that found nothing to skip settles it for later fits over the same samples with the same bin count,
    //  neighbour count and metric -- the verdict depends on all three)
    // (wide rows, Dz > 160: the plain two-sweep builds only -- no tile skipping, pools or segments)
    h->seat.fit_reset(h->seat.off_key == skip_key(h) || h->Dz > 160);
    h->fused = h->sw.allow_fused && h->pf_fit && fused_supported(m, h->Dp);
    HIPCHK(h->pin_a.ensure((size_t)h->N));
    int *lab = h->pin_a.p;
    std::vector<int64_t> bin_size((size_t)B, 0);
    for (int64_t i = 0; i < h->N; ++i) {
        const int64_t v = initial[i];
        if (v >= B) return fail(CHB_EINVAL, "initial_bins contains a label >= num_clusters");
        lab[(size_t)i] = v < 0 ? -1 : (int)v;
        if (v >= 0) ++bin_size[(size_t)v];
    }
    {   // bin sizes as the first batch will see them (later ones come home with the rounds' verdicts)
        int64_t mx = 0, tot = 0;
        for (int64_t c = 0; c < B; ++c) { const int64_t t = (bin_size[(size_t)c] + 31) / 32; mx = std::max(mx, t); tot += t; }
        h->seg.hint_max_tiles = (int)mx; h->seg.hint_total_tiles = (int)std::min<int64_t>(tot, 0x7fffffff);
    }
    HIPCHK(h->labels.ensure((size_t)h->N));
    HIPCHK(h->inb.ensure((size_t)h->N));
    HIPCHK(hipMemcpyAsync(h->labels.p, lab, sizeof(int) * h->N, hipMemcpyHostToDevice, h->stream));
    launch_fill_i32(h->inb.p, -1, (int)h->N, h->stream);
    HIPCHK(h->cnt.ensure((size_t)B * kShells));
    HIPCHK(hipMemsetAsync(h->cnt.p, 0, sizeof(int) * h->cnt.cap, h->stream));   // (kept zero by scan_kernel from here on)
    HIPCHK(h->bin_ptr.ensure((size_t)B + 1));
    HIPCHK(h->cursor.ensure((size_t)B * kShells));
    h->seat.nsh = 1;
    HIPCHK(h->memb_id.ensure((size_t)h->N));
    if (h->pf_fit) {
        // Bin centres for the shortlist stage: the mean of each bin's initially labelled members
        // (the seeds), fixed for the whole fit -- any fixed point keeps the bounds valid, one near
        // the bin keeps them tight.  Then every labelled sample's shadow row against its own bin.
        HIPCHK(h->centers.ensure((size_t)B * h->Dp));
        {
            Timed t(h, "fit_start", (double)h->N);
            launch_bucket_base(h->labels.p, h->inb.p, (int)h->N, h->B, h->cnt.p, h->bin_ptr.p, h->cursor.p,
                               h->memb_id.p, nullptr, nullptr, h->stream);
            launch_bin_centers(h->X.p, h->D, h->Dp, h->memb_id.p, h->bin_ptr.p, h->B, h->centers.p, h->stream);
            launch_sample_shadow(h->X.p, h->D, h->Dp, nullptr, (int)h->N, h->labels.p, h->B, h->centers.p,
                                 h->mu_g.p, h->shadow_scale, h->Zs.p, h->Dz, h->ms.p, nullptr, nullptr, h->stream);
        }
        // every sample's exact norm against every (fixed) centre, and its nearest centre: once per fit, not per batch.
        // N x B x 8 bytes (51 MB at 100k x 64, 1.6 GB at 1M x 200, 65 GB at 1M x 8192): a table that does not fit the
        // device sends the fit to the brute-force selection (as a feature width beyond the shortlist stage's does) instead
        // of failing it
        if (h->qn.ensure((size_t)h->N * (size_t)B * 2) != hipSuccess || h->seat.ckey.ensure((size_t)h->N) != hipSuccess) {
            (void)hipGetLastError();
            h->qn.release(); h->seat.ckey.release();
            h->pf_fit = false; h->fused = false;
        }
    }
    if (h->pf_fit) {
        {
            Timed t(h, "query_norms", (double)h->N * (double)B);
            launch_query_norms(h->X.p, h->D, h->Dp, (int)h->N, h->B, h->centers.p, h->shadow_scale, h->qn.p, h->seat.ckey.p, h->stream);
        }
        // the unit of the CSR's shell key per bin (from the initially labelled members; fixed for the fit)
        int nsh = kShells;
        while (nsh > 1 && (int64_t)B * nsh > kMaxKeys) nsh >>= 1;
        HIPCHK(h->seat.shell_inv.ensure((size_t)B));
        launch_shell_scale(h->ms.p, h->memb_id.p, h->bin_ptr.p, h->B, nsh, h->seat.shell_inv.p, h->stream);
        h->seat.nsh = nsh;
        HIPCHK(hipGetLastError());
    }
    if (sync) HIPCHK(hipStreamSynchronize(h->stream));
    h->fit_open = true; h->batch.open = false; h->Kcap = 0;
    h->overflow_total_valid = false;
    if (h->short_cnt.p) HIPCHK(hipMemsetAsync(h->short_cnt.p, 0, sizeof(int), h->stream));
    if (h->trim_ctr.p) HIPCHK(hipMemsetAsync(h->trim_ctr.p, 0, 3 * sizeof(unsigned long long), h->stream));
    h->pp.fit_reset();
    if (h->pp.ctl.p) HIPCHK(hipMemsetAsync(h->pp.ctl.p, 0, 4 * sizeof(int), h->stream));
    return CHB_OK;
}

}  // namespace chb

namespace {

// The persistent base pack from the labels as they stand (no batch open): compact CSR of all labelled samples, then
// regions with room to grow.  Allocates on first use (12 N + 1024 B rows: the layout takes at most 3.5 N + 128 B, a commit's
// moves at most 3 (N + K) + 96 B, the host rebuilds from 5 N + 512 B on) -- hence only ever called outside a look-ahead window.
int pack_state_build(chb_ctx *h)
{
    const size_t B = h->B;
    // (layout: at most 2 N + 1.5 N + 128 B rows; 2 * row + 1 must fit an int)
    const int arena = (int)std::min<int64_t>(12 * h->N + 1024 * (int64_t)B, 0x3fffff00);
    // The host asks for a rebuild (compaction) once `mark` rows are handed out; the request is honoured up to three commits
    // later (it rides home with a verdict, lags a batch under the look-ahead and waits for a batch start outside a window).
    // What three commits can take: ONE mass move -- every bin's region tripling at once, 3 (N + K) + 96 B rows, after which
    // the regions hold three times their members and cannot move again at once -- plus the appends of the other two (K rows
    // each): 3 N + 5 K + 128 B.  The mark leaves that much room; it always lies above a fresh layout (3.5 N + 128 B) since a
    // batch never holds more than N samples.
    {
        const int64_t K = std::max(h->Kcap, 1);
        h->pp.mark = std::min<int64_t>(5 * h->N + 512 * (int64_t)B, (int64_t)arena - (3 * h->N + 5 * K + 128 * (int64_t)B));
        if (h->pp.mark < 7 * h->N / 2 + 128 * (int64_t)B) { h->pp.valid = false; h->pp.fit = false; return CHB_OK; }   // (capped arena)
    }
    if (h->pp.arena_rows < arena || !h->pp.memb.p) {
        if (h->pk.ensure((size_t)arena, B, (size_t)h->Dz) != hipSuccess || h->pp.memb.ensure((size_t)arena + 64) != hipSuccess) {
            (void)hipGetLastError();   // (no room for the arena: this fit rebuilds its pack per batch)
            h->pp.memb.release();
            HIPCHK(h->pk.ensure((size_t)h->N + 32 * B, B, (size_t)h->Dz));
            h->pp.arena_rows = 0; h->pp.valid = false; h->pp.fit = false;
            return CHB_OK;
        }
        h->pp.arena_rows = arena;
    }
    HIPCHK(h->pp.row.ensure((size_t)h->N));
    DevBuf<int> *pb[] = {&h->pp.start, &h->pp.cap, &h->pp.fill, &h->pp.live, &h->pp.nt, &h->pp.fill0, &h->pp.start0};
    for (auto *b : pb) HIPCHK(b->ensure(B + 1));
    HIPCHK(h->pp.ctl.ensure_zeroed(4, h->stream));
    HIPCHK(h->pp.ovf.ensure((size_t)std::max(h->Kcap, 1)));
    HIPCHK(h->pp.dest.ensure((size_t)std::max(h->Kcap, 1)));
    // (room to grow: were all N samples labelled and spread evenly, a bin would hold N / B rows -- half as much again)
    const int grow = (int)std::min<int64_t>((3 * h->N / 2) / std::max<int64_t>(h->B, 1) + 64, 0x3fffffff);
    {
        Timed t(h, "bucket", (double)h->N);
        launch_bucket_base(h->labels.p, h->inb.p, (int)h->N, h->B, h->cnt.p, h->bin_ptr.p, h->cursor.p, h->memb_id.p, nullptr,
                           nullptr, h->stream);
        launch_pack_state_build(h->pp.view(), h->pk.view(), h->Zs.p, h->ms.p, h->D, h->Dz, h->memb_id.p, h->bin_ptr.p, h->B,
                                (int)h->N, grow, h->stream);
    }
    HIPCHK(hipGetLastError());
    h->pp.valid = true; h->pp.rebuild = false;
    h->pp.stat_builds += 1;
    return CHB_OK;
}

}  // namespace

namespace chb {

// The threshold pools from the labels as they stand at a fit's start (the CSR fit_begin_impl has just made): allocated on
// first use, B x B tiles of 32 shadow rows -- 38 MB at 100k x 136 x 64, 410 MB at 1M x 146 x 200; a fit whose pools would
// take more than kPoolMaxBytes keeps the two-sweep shortlist launch.
constexpr size_t kPoolMaxBytes = (size_t)1 << 30;
int pool_build(chb_ctx *h)
{
    h->pool.valid = false;
    const size_t B = h->B, slots = B * B * (size_t)kPoolRows;
    // (m > 8: the 16-lane hull kernel pays for every candidate beyond 16 with extra rows and second tiles -- with the pools'
    //  17.4 instead of 16.8 candidates per pair at m = 15 it ran 34.4 instead of 28.8 ms per sweep, more than the shortlist
    //  kernel saved (5.1 instead of 5.9): those fits keep the two sweeps)
    if (!h->sw.pool_allowed || !h->fused || !h->pf_fit || h->seat.ckey.p == nullptr || B < 2 || h->m > 8 || h->Dz > 160 ||
        slots * (size_t)h->Dz * sizeof(unsigned short) > kPoolMaxBytes)
        return CHB_OK;
    // (small fits: a bin of a few tiles has no threshold sweep worth replacing, while the pools' build and upkeep are per
    //  fit and per batch -- BASELINE configs[1], 10k x 32 = 10 tiles per bin, went from 1.45 to 1.85 ms per sweep with them.
    //  From 16 tiles per bin on average; CHB_POOL_TAU=2 keeps them whatever the size)
    if (!h->sw.pool_force && (size_t)h->N < 512 * B) return CHB_OK;
    if (h->pool.Z.ensure(slots * (size_t)h->Dz) != hipSuccess || h->pool.id.ensure(slots) != hipSuccess ||
        h->pool.hole.ensure(slots) != hipSuccess || h->pool.key.ensure(slots) != hipSuccess || h->pool.sn.ensure(slots) != hipSuccess ||
        h->pool.tsn.ensure(B * B + 64) != hipSuccess || h->pool.ok.ensure(B * B) != hipSuccess) {
        (void)hipGetLastError();   // (no room: the fit keeps the two-sweep launch)
        h->pool.release();
        return CHB_OK;
    }
    {
        Timed t(h, "pool", (double)h->N);
        launch_pool_build(h->pool.view(), h->Zs.p, h->ms.p, h->qn.p, h->D, h->Dz, h->memb_id.p, h->bin_ptr.p, h->B, h->stream);
    }
    HIPCHK(hipGetLastError());
    h->pool.valid = true;
    return CHB_OK;
}

// chb_create: the environment switches of the new context (unset: the defaults of Switches and chb_ctx::DevKnobs)
void read_switches(chb_ctx *h)
{
    auto flag = [](const char *name, bool &v) { if (const char *e = getenv(name)) v = atoi(e) != 0; };
    Switches &w = h->sw;
    flag("CHB_PREFILTER", w.use_prefilter);
    flag("CHB_FUSED", w.allow_fused);
    flag("CHB_FUSED_PTR64", w.fused_ptr64);
    flag("CHB_SPECULATE", w.speculate);
    flag("CHB_FORCE_GATHER", w.force_gather);
    flag("CHB_SEGMENTS", w.allow_segments);
    flag("CHB_FUSED_STRIPE", w.fused_stripe);
    flag("CHB_FUSED_TRIM", w.fused_trim);
    flag("CHB_PACK_INCR", w.pp_allowed);
    flag("CHB_TILE_SKIP", w.allow_skip);
    if (const char *e = getenv("CHB_POOL_TAU")) { w.pool_allowed = atoi(e) != 0; w.pool_force = atoi(e) == 2; }
#ifdef CHB_DEV_KNOBS
    auto &d = h->dk;
    d.sl_bounds = getenv("CHB_SL_BOUNDS") != nullptr;
    d.sl_validate = getenv("CHB_SL_VALIDATE") != nullptr;
    if (const char *e = getenv("CHB_SL_INJECT_SHORT")) d.inject_short = atoi(e);
    if (const char *e = getenv("CHB_SL_BPW")) d.sl_bpw = atoi(e);
    if (const char *e = getenv("CHB_SKIP_NEVER")) d.skip_never = atoi(e);
    if (const char *e = getenv("CHB_SL_DBG")) d.sl_dbg = e;
    if (const char *e = getenv("CHB_PACK_REBUILD_AT")) d.pack_rebuild_at = atoll(e);
    flag("CHB_DEV_HOOK_SPEC", d.hook_spec);
    flag("CHB_DEV_LOCAL_VERDICT", d.local_verdict);
    if (const char *e = getenv("CHB_DEV_SKIP_STATS"))
        d.skip_stats_on = sscanf(e, "%d,%d,%d", &d.skip_stats[0], &d.skip_stats[1], &d.skip_stats[2]) == 3;
#endif
}

}  // namespace chb

namespace {

// ---- batch_begin_dev's hooks for the developer builds' checks and records of the shortlist stage (product build: none)
#ifdef CHB_DEV_KNOBS
constexpr size_t kDbgWords = (size_t)65536 * 16;   // the timeline: 16 words per workgroup
int sl_bpw(const chb_ctx *h) { return h->dk.sl_bpw; }

// before the base shortlist launch: CHB_SKIP_NEVER's bits; CHB_SL_DBG=<file>: per-wavefront timeline of the context's 10th
// launch (tools/sl_timeline.py); CHB_SL_BOUNDS=1: the launch checks its tile DMA sources and member reads against the
// buffers' extents, skips an access that is out of range and reports the first one (instead of a GPU memory fault)
int dev_shortlist_args(chb_ctx *h, ShortlistArgs &pa, bool skip_on, bool pp_now)
{
    auto &d = h->dk;
    if (skip_on && d.skip_never) pa.skip = 1 | 2 * d.skip_never;
    if (!d.sl_dbg.empty() && ++d.launches == 10) {
        HIPCHK(d.dbg.ensure(kDbgWords));
        HIPCHK(hipMemsetAsync(d.dbg.p, 0, kDbgWords * 8, h->stream));
        pa.dbg = d.dbg.p;
    }
    if (d.sl_bounds) {
        HIPCHK(d.viol.ensure(8));
        HIPCHK(hipMemsetAsync(d.viol.p, 0, 8 * sizeof(int), h->stream));
        pa.viol = d.viol.p;
        pa.viol_rows = pp_now ? (long long)h->pp.arena_rows : (long long)h->N + 32LL * h->B + 64;
        pa.viol_pool_rows = (long long)h->B * h->B * kPoolRows;
        pa.viol_members = pp_now ? (long long)h->pp.arena_rows : (long long)h->N;
    }
    return CHB_OK;
}

// after it (and its second chance): the bounds report, the timeline's dump
int dev_shortlist_report(chb_ctx *h, const ShortlistArgs &pa, bool skip_on, bool pool_on, bool pp_now)
{
    auto &d = h->dk;
    if (pa.viol != nullptr) {
        int hv[8];
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(hv, d.viol.p, sizeof(hv), hipMemcpyDeviceToHost));
        if (hv[0] != 0) {
            fprintf(stderr, "[chb bounds] code %d: %d %d %d %d %d %d (workgroup %d); skip %d pool %d pp %d K %d q %d..%d\n", hv[0], hv[1],
                    hv[2], hv[3], hv[4], hv[5], hv[6], hv[7], (int)skip_on, (int)pool_on, (int)pp_now, h->batch.K, h->batch.q_lo, h->batch.q_hi);
            return fail(CHB_ESTATE, "shortlist bounds check failed");
        }
    }
    if (pa.dbg != nullptr) {
        std::vector<unsigned long long> hostd(kDbgWords);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(hostd.data(), d.dbg.p, kDbgWords * 8, hipMemcpyDeviceToHost));
        if (FILE *fp = fopen(d.sl_dbg.c_str(), "wb")) { fwrite(hostd.data(), 8, kDbgWords, fp); fclose(fp); }
    }
    return CHB_OK;
}

// once a fused batch's base shortlists on a rebuilt CSR are final: CHB_SL_INJECT_SHORT=<n>: the n-th such batch truncates one
// (the product build's check must turn it into an error); CHB_SL_VALIDATE=1: they and the index arrays behind them are
// checked on the device before the hull kernels read them
int dev_shortlist_check(chb_ctx *h, bool skip_on, const int *qord)
{
    auto &d = h->dk;
    const int q_lo = h->batch.q_lo, q_hi = h->batch.q_hi;
    if (d.inject_short > 0 && ++d.batches == d.inject_short)
        launch_inject_short(h->cand_cnt.p, h->B, h->Kcap, q_lo, h->bin_ptr.p, h->m, h->stream);
    if (!d.sl_validate) return CHB_OK;
    HIPCHK(d.verr.ensure(4 + 65536));
    HIPCHK(hipMemsetAsync(d.verr.p, 0, sizeof(int) * (4 + 65536), h->stream));
    launch_validate_batch(h->cand.p, h->cand_cnt.p, h->B, h->Kcap, q_lo, q_hi, kCandCap, (int)h->N, h->bin_ptr.p,
                          h->memb_id.p, skip_on ? qord : nullptr, h->m, d.verr.p, h->stream);
    int herr[4];
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(herr, d.verr.p, sizeof(herr), hipMemcpyDeviceToHost));
    if (herr[0] != 0) {
        fprintf(stderr, "[chb validate] code %d bin %d position %d value %d (batch positions %d..%d, skip %d)\n", herr[0],
                herr[1], herr[2], herr[3], q_lo, q_hi, (int)skip_on);
        if (herr[0] >= 5 && skip_on && q_hi - q_lo <= 256) {
            const int nq = q_hi - q_lo;
            std::vector<int> qo(nq);
            HIPCHK(hipMemcpy(qo.data(), h->seat.qord.p, 4 * (size_t)nq, hipMemcpyDeviceToHost));
            for (int i = 0; i < nq; ++i) fprintf(stderr, "  i %d qord %d\n", i, qo[i]);
        }
        return fail(CHB_ESTATE, "shortlist validation failed");
    }
    return CHB_OK;
}
#else
int sl_bpw(const chb_ctx *) { return 0; }
int dev_shortlist_args(chb_ctx *, ShortlistArgs &, bool, bool) { return CHB_OK; }
int dev_shortlist_report(chb_ctx *, const ShortlistArgs &, bool, bool, bool) { return CHB_OK; }
int dev_shortlist_check(chb_ctx *, bool, const int *) { return CHB_OK; }
#endif

// ---- a batch start (batch_begin_dev): what it will do is decided first -- BatchPlan's constructor from the context alone,
// settle_batch where that allocates, launches or fails -- then its launches follow as stages, in the order they are enqueued
struct BatchPlan {
    bool fusedp;         // the fit loop's fused path (m <= 16) works on the shortlists directly: no exact base lists
    bool pf_base_path;   // the base members go through the shortlist stage
    bool skip_on, pp_now = false, pool_on = false;   // tile skipping, persistent pack, threshold pools serve this batch
    SegPlan sp{};
    int *qord_p, *home_p;   // the queries' seats (read under skip_on / pool_on only)
    BatchPlan(const chb_ctx *h, bool need_lists)   // (a pure function of the context: no HIP call, nothing written)
    {
        fusedp = h->fused && !need_lists;
        pf_base_path = h->pf_fit && h->cand.p;
        // tile skipping: on until the fit's first batches have shown that it skips (next to) nothing
        skip_on = pf_base_path && h->sw.allow_skip && h->seat.nsh > 1 && h->seat.state >= 0 && h->seat.ckey.p != nullptr;
        // segmented bins: the plan is made by the CSR scan on the device, but only if the host will also enqueue the two
        // segment launches -- which it does when the bin sizes it saw last (one or two batches old) say that a bin may
        // have more than kSegMinTiles tiles and four times the average
        if (pf_base_path && h->seg.gflag.p) {
            sp.nseg = h->seg.nseg.p; sp.items = h->seg.items.p; sp.gflag = h->seg.gflag.p; sp.lists = h->seg.lists.p;
            sp.cap = 16 * h->seg.gcap; sp.gcap = h->seg.gcap;
            const long long est = (long long)h->seg.hint_max_tiles * 3 / 2 + 8;
            sp.launch = h->sw.allow_segments && h->Dz <= 160 && est > kSegMinTiles && est * h->B > 3LL * std::max(1, h->seg.hint_total_tiles);
        }
        const bool swept = h->seat.qord_cur != nullptr;   // (seated by the fit loop, for the whole sweep)
        qord_p = swept ? h->seat.qord_cur : h->seat.qord.p; home_p = swept ? h->seat.home_cur : h->seat.home.p;
    }
};

// before the launches: the segment lists' allocation, the pack's (re)build; which of pack and pools serve this batch and stay valid
int settle_batch(chb_ctx *h, BatchPlan &p)
{
    if (p.sp.launch) {
        HIPCHK(h->seg.lists.ensure((size_t)h->seg.gcap * 16 * (size_t)h->Kcap * (size_t)shortlist_list_len(h->m)));
        p.sp.lists = h->seg.lists.p;
    }
    // the persistent base pack serves the fit loop's batches whenever the shortlist launch does not skip tiles (whose
    // shell order needs the rebuild); built / rebuilt only outside a look-ahead window
    if (h->pp.fit && h->sw.pp_allowed && p.fusedp && p.pf_base_path && !p.skip_on) {
        if ((!h->pp.valid || h->pp.rebuild) && g_gate.flag == nullptr) { const int r_ = pack_state_build(h); if (r_) return r_; }
        p.pp_now = h->pp.valid;
    }
    if (!p.pp_now) h->pp.valid = false;   // (this batch's commit will not maintain the pack)
    h->pp.batch = p.pp_now;
    // threshold pools: the base shortlist launch streams a bin once where a pool tile gives the threshold
    if (!(h->pool.fit && p.fusedp && p.pf_base_path)) h->pool.valid = false;   // (this batch will not maintain them)
    if (h->pool.state < 0) h->pool.valid = false;                              // (turned off for this fit: no upkeep either)
    p.pool_on = h->pool.valid && h->pool.state >= 0;
    return CHB_OK;
}

// the batch is opened in the base members' CSR (the pack's, or rebuilt) and in the pools
void open_batch(chb_ctx *h, const BatchPlan &p)
{
    const SegPlan *seg = p.sp.gflag ? &p.sp : nullptr;
    // the pools are opened only for a batch that can hold a labelled sample: no other batch makes a hole, and ok[] is kept
    // right by the build and by every commit (sweep 1 of a fit from seeds -- the benchmark's step -- opens none).  The
    // second-chance launch's overflow counter, which launch_pool_open resets, is then reset by the pack's batch start
    const bool open_pools = h->pool.valid && (h->pool.batch_labelled || !p.pp_now);
    if (p.pp_now) {
        // the batch is opened (its members' rows become holes) and tiles per bin / statistics / segment plan written:
        // one launch instead of count + scan + fill + gather
        Timed t(h, "bucket", (double)h->batch.K);
        launch_pack_state_start(h->pp.view(), h->pk.view(), h->D, h->Dz, h->labels.p, h->inb.p, h->batch.bq_cur, h->batch.K, h->lab_old.p,
                                h->B, seg, h->batch.fc_cur + kSlotMaxTiles, h->nflag.p, h->pool.valid && !open_pools ? h->nflag2.p : nullptr,
                                h->stream);
        h->pp.stat_batches += 1;
    } else {
        // (the batch is opened -- labels remembered, members marked -- inside the CSR count's launch)
        Timed t(h, "bucket", (double)h->N);
        launch_bucket_base(h->labels.p, h->inb.p, (int)h->N, h->B, h->cnt.p, h->bin_ptr.p, h->cursor.p, h->memb_id.p,
                           h->pk.pad_ptr.p, h->nflag.p, h->stream, h->batch.bq_cur, h->batch.K, h->lab_old.p, seg, h->batch.fc_cur + kSlotMaxTiles,
                           p.pf_base_path ? h->ms.p : nullptr, p.skip_on ? h->seat.shell_inv.p : nullptr, p.skip_on ? h->seat.nsh : 1);
    }
    if (open_pools) {
        // (the batch's samples are marked: their slots in the pools are holes while it is open)
        Timed t(h, "pool", (double)h->batch.K);
        launch_pool_open(h->pool.view(), h->inb.p, h->D, h->Dz, h->B, h->nflag2.p, h->stream);
    }
    h->pool.holes = h->pool.batch_labelled;
}

// what the base shortlist launch reads besides the CSR: the fit's overflow counter, a rebuilt CSR's pack, the queries' seats
void shortlist_inputs(chb_ctx *h, const BatchPlan &p)
{
    // (flags64 is all zero here: launch_topm_flagged clears what it serves)
    if (!h->overflow_total_valid) { launch_fill_i32(h->overflow.p, 0, 1, h->stream); h->overflow_total_valid = true; }
    if (!p.pp_now) {
        // the members' shadow rows (relative to their bin's centre) gathered into padded CSR order, and the per-bin
        // bounds: one launch
        Timed t(h, "bucket", 0.0);
        launch_pack_build(h->Zs.p, h->ms.p, h->D, h->Dz, h->memb_id.p, h->bin_ptr.p, h->B, (int)h->N, h->pk.view(), p.skip_on, h->stream);
    }
    if (!(p.skip_on || p.pool_on) || h->seat.qord_cur != nullptr) return;   // (seated by position; done for the whole sweep)
    Timed t(h, "bucket", 0.0);   // (the queries are seated in the order of their nearest bin centre)
    launch_query_order(h->seat.ckey.p, h->batch.bq_cur, h->batch.q_lo, h->batch.q_hi, h->B, h->seat.qord.p, h->seat.home.p, h->stream);
}

int base_shortlist_args(chb_ctx *h, const BatchPlan &p, ShortlistArgs &pa)
{
    pa = h->shortlist_args(h->batch.q_lo, h->batch.q_hi);
    pa.P = h->pk.view(); pa.bin_ptr = h->bin_ptr.p; pa.memb_id = h->memb_id.p;
    if (p.pp_now) {   // (a bin = its region: first row, tiles in use; a row's sample, -1 for a hole)
        pa.P.pad_ptr = h->pp.start.p; pa.P.nt = h->pp.nt.p;
        pa.bin_ptr = h->pp.start.p; pa.memb_id = h->pp.memb.p;
    }
    pa.cand = h->cand.p; pa.cand_cnt = h->cand_cnt.p; pa.cand_cap = kCandCap; pa.seg = p.sp;
    if (p.fusedp) pa.tau_out = h->tau.p;
    if (p.sp.launch) h->seg.stat_batches += 1;
    if (p.skip_on) { pa.qord = p.qord_p; pa.home = p.home_p; pa.skip = 1; pa.skip_stat = h->batch.fc_cur + kSlotSkipped; }
    if (p.pool_on) {
        pa.qord = p.qord_p; pa.home = p.home_p; pa.ckey = h->seat.ckey.p; pa.pool = h->pool.view();
        pa.pool_stat = h->batch.fc_cur + kSlotPoolCand;
        h->pool.stat_batches += 1;
    }
    return dev_shortlist_args(h, pa, p.skip_on, p.pp_now);
}

// two-stage exact selection: fp16 matrix-core shortlist, exact fp64 on the shortlist,
// brute force only for (query tile, bin) pairs whose shortlist overflowed
int base_shortlist(chb_ctx *h, const BatchPlan &p, const ShortlistArgs &pa)
{
    {
        Timed t(h, "prefilter", (double)(h->batch.q_hi - h->batch.q_lo) * h->batch.hint_base_members);
        launch_shortlist(pa, h->flags64.p, sl_bpw(h), h->stream);
    }
    if (p.pool_on) {
        // second chance for the pairs whose pool threshold was too loose for a 128-entry shortlist: the exact two-sweep
        // selection on the overflow list's work items; only what overflows again goes to the brute-force kernel
        Timed t(h, "prefilter_retry", 0.0);
        ShortlistArgs pb = pa;
        pb.worklist = h->flaglist.p; pb.nwork = h->nflag.p; pb.flaglist = h->flaglist2.p; pb.nflag = h->nflag2.p;
        launch_shortlist_worklist(pb, h->flags64.p, h->stream);
    }
    return dev_shortlist_report(h, pa, p.skip_on, p.pool_on, p.pp_now);
}

// (a = the exact selection over the base members, lists to L0: here for the pairs whose shortlist overflowed)
int finish_base_lists(chb_ctx *h, const BatchPlan &p, TopmArgs a)
{
    if (!p.fusedp) {
        RescoreArgs ra = h->rescore_args(h->batch.q_lo, h->batch.q_hi);
        ra.out = h->L0();
        Timed t(h, "rescore", (double)(h->batch.q_hi - h->batch.q_lo) * h->B);
        launch_rescore(ra, h->stream);
    } else {
        // overflowed (query tile, bin) pairs: the brute-force kernel's exact top-m becomes the shortlist
        a.out = Lists{nullptr, nullptr, nullptr};
        a.cand_out = h->cand.p; a.cand_cnt_out = h->cand_cnt.p; a.cand_cap = kCandCap;
        a.tau_out = h->tau.p; a.S = h->shadow_scale;
    }
    {
        Timed t(h, "topm_fallback", 0.0);   // the brute-force kernel's work list: what the second chance left, where it ran
        launch_topm_flagged(a, h->flags64.p, p.pool_on ? h->flaglist2.p : h->flaglist.p, p.pool_on ? h->nflag2.p : h->nflag.p, h->stream);
    }
    return p.fusedp && !p.pp_now ? dev_shortlist_check(h, p.skip_on, p.qord_p) : CHB_OK;
}

// no shortlist stage: the brute-force fp64 selection over all base members
void base_topm_plain(chb_ctx *h, const TopmArgs &a)
{
    Timed t(h, "topm_base", (double)(h->batch.q_hi - h->batch.q_lo) * h->batch.hint_base_members);
    if (h->m > kMaxM) launch_topm_generic(a, h->stream); else launch_topm(a, h->stream);
}

}  // namespace

namespace chb {

// bq already holds the K sample indices (device).  need_lists: the caller wants the exact base lists
// L0 (chb_topm_per_bin); the fit loop of the fused path (m <= 16) works on the shortlists directly.
int batch_begin_dev(chb_ctx *h, int K, int q_lo, int q_hi, bool need_lists)
{
    BatchPlan p(h, need_lists);
    h->batch.lists_valid = !p.fusedp; h->batch.K = K; h->batch.q_lo = q_lo; h->batch.q_hi = q_hi;
    h->batch.round_in_batch = 0; h->round_active = 0;
    { const int r_ = settle_batch(h, p); if (r_) return r_; }
    open_batch(h, p);
    TopmArgs a = h->topm_args(q_lo, q_hi);
    a.bin_ptr = h->bin_ptr.p; a.memb_id = h->memb_id.p; a.out = h->L0();
    if (p.pp_now) { a.bin_ptr = h->pp.start.p; a.bin_cnt = h->pp.fill.p; a.memb_id = h->pp.memb.p; }
    if (p.pf_base_path) {
        ShortlistArgs pa{};
        shortlist_inputs(h, p);
        int r_ = base_shortlist_args(h, p, pa);
        if (!r_) r_ = base_shortlist(h, p, pa);
        if (!r_) r_ = finish_base_lists(h, p, a);
        if (r_) return r_;
    } else base_topm_plain(h, a);
    HIPCHK(hipGetLastError());
    h->batch.open = true;
    return CHB_OK;
}

}  // namespace chb

namespace {

// ---- a round's three formulations (batch_round_dev picks one; a = its exact selection over the batch's own entries)
// the batch's own entries as a padded pack, and the update-mode shortlist launch over it, less its thresholds and candidates
ShortlistArgs batch_entry_shortlist(chb_ctx *h, int lo, int hi)
{
    launch_pack_centered(h->X.p, h->D, h->Dp, h->memb2_id.p, h->memb2_code.p, h->bin_ptr2.p, h->B, 2 * h->batch.K,
                         h->centers.p, h->mu_g.p, h->shadow_scale, h->Dz, h->pk2.view(), h->stream);
    ShortlistArgs pa = h->shortlist_args(lo, hi);
    pa.P = h->pk2.view(); pa.bin_ptr = h->bin_ptr2.p; pa.memb_id = h->memb2_id.p; pa.update = true;
    return pa;
}

// fused (m <= 16, no lists wanted): shortlist of the batch's own entries against the base stage's tau, then selection +
// hull distance straight from the two shortlists
void round_fused(chb_ctx *h, int lo, int hi, TopmArgs a)
{
    hipStream_t s = h->stream;
    const int cur = h->batch.round_in_batch & 1;
    ShortlistArgs pa = batch_entry_shortlist(h, lo, hi);
    pa.tau_in = h->tau.p; pa.cand = h->candu[cur].p; pa.cand_cnt = h->candu_cnt[cur].p; pa.cand_cap = kCandCapU;
    {
        Timed t(h, "prefilter_update", (double)(hi - lo) * h->batch.hint_batch_entries);
        launch_shortlist(pa, h->flags64.p, sl_bpw(h), s);
    }
    {
        // overflowed pairs: exact top-m among the (eligible) batch entries as their shortlist
        a.in = a.out = Lists{nullptr, nullptr, nullptr};
        a.cand_out = h->candu[cur].p; a.cand_cnt_out = h->candu_cnt[cur].p; a.cand_cap = kCandCapU;
        Timed t(h, "topm_fallback", 0.0);
        launch_topm_flagged(a, h->flags64.p, h->flaglist.p, h->nflag.p, s);
    }
    FusedArgs f = h->fused_args(lo, hi);
    f.cand = h->cand.p; f.cand_cnt = h->cand_cnt.p; f.candu = h->candu[cur].p; f.candu_cnt = h->candu_cnt[cur].p;
    if (h->batch.round_in_batch > 0) { f.candp = h->candu[cur ^ 1].p; f.candp_cnt = h->candu_cnt[cur ^ 1].p; }
    f.slow = h->slow.p; f.n_slow = h->n_slow.p; f.bin_ptr = h->bin_ptr.p; f.short_cnt = h->short_cnt.p;
    if (h->pp.batch) f.bin_size = h->pp.live.p;
    {
        Timed t(h, "hull_qp", (double)(hi - lo) * h->B);
        launch_hull_select_qp(f, h->sw.fused_stripe, h->sw.fused_ptr64, s);
    }
    {
        // the exact path for what the fused kernel left: cdist-rounded distances on both shortlists,
        // (distance, index) order, then the list-based hull kernel
        Timed t(h, "slow_path", 0.0);
        RescoreArgs ra = h->rescore_args(lo, hi);
        ra.cand2 = h->candu[cur].p; ra.cand2_cnt = h->candu_cnt[cur].p; ra.cand2_cap = kCandCapU;
        ra.active = h->slow.p; ra.n_active = h->n_slow.p; ra.out = h->L1();
        launch_rescore(ra, s);
        QpArgs q = h->qp_args(lo, hi);
        q.lists = h->L1(); q.active = h->slow.p; q.n_active = h->n_slow.p;
        launch_hull_qp(q, s);
    }
}

// list-based with the shortlist stage: the batch members that can displace an entry of the base list -- fp16 shortlist
// against the exact m-th distance, exact rescoring seeded with the base list
// (fit rounds only produce the "earlier" / "later" eligibility codes, which have the affine form the shortlist kernel
// evaluates; chb_topm_per_bin's "not equal" code stays on launch_topm)
int round_lists_shortlist(chb_ctx *h, int lo, int hi, const TopmArgs &a)
{
    hipStream_t s = h->stream;
    ShortlistArgs pa = batch_entry_shortlist(h, lo, hi);
    pa.seed = h->L0(); pa.cand = h->cand.p; pa.cand_cnt = h->cand_cnt.p; pa.cand_cap = kCandCap;
    {
        Timed t(h, "prefilter_update", (double)(hi - lo) * h->batch.hint_batch_entries);
        launch_shortlist(pa, h->flags64.p, sl_bpw(h), s);
        // the (position, bin) pairs with a non-empty shortlist, for rescore_kernel
        launch_compact_active(h->cand_cnt.p, lo, hi, h->B, h->Kcap, h->act_blk.p, h->active.p, h->n_active.p, s);
    }
    RescoreArgs ra = h->rescore_args(lo, hi);
    ra.active = h->active.p; ra.n_active = h->n_active.p; ra.in = h->L0(); ra.out = h->Lcur();
    // pairs without any candidate keep the base list
    const size_t nl = (size_t)h->Kcap * h->B;
    HIPCHK(hipMemcpyAsync(ra.out.d, h->l0d.p, sizeof(double) * nl * h->m, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ra.out.idx, h->l0i.p, sizeof(int) * nl * h->m, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ra.out.cnt, h->l0c.p, sizeof(int) * nl, hipMemcpyDeviceToDevice, s));
    {
        Timed t(h, "rescore_update", (double)(hi - lo) * h->B);
        launch_rescore(ra, s);
    }
    {
        Timed t(h, "topm_fallback", 0.0);
        launch_topm_flagged(a, h->flags64.p, h->flaglist.p, h->nflag.p, s);
    }
    return CHB_OK;
}

// list-based, brute force: the exact selection over all of the batch's entries
void round_lists_plain(chb_ctx *h, int lo, int hi, const TopmArgs &a)
{
    Timed t(h, "topm_update", (double)(hi - lo) * h->batch.hint_batch_entries);
    if (h->m > kMaxM) launch_topm_generic(a, h->stream); else launch_topm(a, h->stream);
}

}  // namespace

namespace chb {

// lab_prev (device) holds the labels of the previous round.  Evaluates [max(active,q_lo), q_hi).
int batch_round_dev(chb_ctx *h, int active)
{
    hipStream_t s = h->stream;
    const int lo = std::max(active, h->batch.q_lo), hi = h->batch.q_hi;
    if (hi <= lo) launch_fill_i32(h->batch.fc_cur + kSlotFirstChange, h->batch.K, 1, s);
    const bool fusedp = h->fused && h->batch.lists_valid == false;
    if (hi > lo) {
        {
            Timed t(h, "bucket", (double)h->batch.K);
            launch_bucket_batch(h->lab_prev.p, h->lab_old.p, h->batch.bq_cur, h->batch.K, h->B, h->cnt2.p, h->bin_ptr2.p, h->cursor2.p,
                                h->memb2_id.p, h->memb2_code.p, h->pk2.pad_ptr.p, h->batch.fc_cur + kSlotFirstChange,
                                fusedp ? h->n_slow.p : nullptr, h->nflag.p, s, (h->pf_fit && h->pk2.bb.p) ? h->pk2.bb.p : nullptr);
        }
        TopmArgs a = h->topm_args(lo, hi);
        a.bin_ptr = h->bin_ptr2.p; a.memb_id = h->memb2_id.p; a.memb_code = h->memb2_code.p;
        a.in = h->L0(); a.out = h->Lcur();
        if (fusedp) round_fused(h, lo, hi, a);
        else {
            if (h->pf_fit && h->cand.p) { const int r_ = round_lists_shortlist(h, lo, hi, a); if (r_) return r_; }
            else round_lists_plain(h, lo, hi, a);
            QpArgs q = h->qp_args(lo, hi);
            q.lists = h->Lcur();
            // a (position, bin) whose vertex list is the one of the previous round keeps its distance
            q.prev = h->batch.round_in_batch > 0 ? h->Lprev() : Lists{nullptr, nullptr, nullptr};
            Timed t(h, "hull_qp", (double)(hi - lo) * h->B);
            if (h->m > kMaxM) launch_hull_generic(q, s); else launch_hull_qp(q, s);
        }
        {
            Timed t(h, "argmin", (double)(hi - lo));
            launch_argmin(h->dist.p, h->lab_old.p, h->lab_prev.p, lo, hi, h->B, h->lab_new.p, h->mind.p,
                          h->want_margin ? h->mind2.p : nullptr, h->batch.fc_cur + kSlotFirstChange, h->argmin_in_place, s);
        }
        h->stats[2] += (int64_t)(hi - lo) * h->B;
    }
    HIPCHK(hipGetLastError());
    h->stats[1] += 1;
    h->batch.round_in_batch += 1;
    return CHB_OK;
}

int batch_commit_dev(chb_ctx *h, const int *final_dev)
{
    hipStream_t s = h->stream;
    if (h->pp.batch)
        // ... and the rows put back into the persistent pack (in place, or appended to the new bin), then full regions moved
        launch_pack_state_commit(h->pp.view(), h->pk.view(), h->X.p, h->D, h->Dp, h->batch.bq_cur, h->batch.K, h->labels.p, h->B,
                                 h->centers.p, h->mu_g.p, h->shadow_scale, h->Zs.p, h->Dz, h->ms.p, final_dev, h->lab_old.p,
                                 h->inb.p, s);
    else if (h->pf_fit && h->centers.p)
        // final labels out, batch marks cleared, and the members' shadow rows recomputed against their
        // new bin's centre: one launch
        launch_sample_shadow(h->X.p, h->D, h->Dp, h->batch.bq_cur, h->batch.K, h->labels.p, h->B, h->centers.p, h->mu_g.p,
                             h->shadow_scale, h->Zs.p, h->Dz, h->ms.p, final_dev, h->inb.p, s);
    else
        launch_batch_close(h->labels.p, h->inb.p, h->batch.bq_cur, final_dev, h->batch.K, s);
    if (h->pool.valid) {
        // (labels and shadow rows are final: holes resolved, the batch's arrivals offered to their new bins' pools)
        Timed t(h, "pool", (double)h->batch.K);
        // (a batch the persistent pack served: its commit has just put every bin's arrivals at the tail of the bin's region)
        const chb::PackState pack = h->pp.view();
        launch_pool_commit(h->pool.view(), h->Zs.p, h->ms.p, h->qn.p, h->D, h->Dz, h->batch.bq_cur, h->batch.K, final_dev, h->lab_old.p,
                           h->labels.p, h->B, h->pool.holes, h->pp.batch ? &pack : nullptr, s);
    }
    HIPCHK(hipGetLastError());
    h->batch.open = false;
    h->pp.batch = false;
    return CHB_OK;
}

}  // namespace chb

namespace {

// Under an exchange the ranks run ONE fit together: the order of its collectives is a function of the arguments, of the
// context's switches and of the tile-skipping memo -- so before the first batch every rank all-gathers what it was given
// and how it is set up.  Arguments (and the formulation the switches select) must be equal: a difference fails the call on
// EVERY rank with the same message instead of leaving some of them inside a collective.  What may legitimately differ --
// the memo a context keeps from earlier fits, the A/B switches of the look-ahead, the tile skipping and the persistent
// pack -- is settled by taking the most conservative value of all ranks for this fit.
struct FitAgree {
    static constexpr int W = 24, kEq = 16;
    int v[W];
};
const char *const kAgreeNames[FitAgree::kEq] = {
    "library", "num_clusters", "num_neighbors", "n_move", "max_iter", "batch size", "N", "D", "metric", "CHB_FUSED / fused path",
    "CHB_PREFILTER / shortlist stage", "min_dist_out", "perms", "perms", "initial_bins", "initial_bins"};

uint64_t hash_i64(const int64_t *p, int64_t n)
{
    // four independent multiply-xor lanes (the order of the elements matters, which is the point)
    uint64_t a = 0x9e3779b97f4a7c15ull, b = 0xc2b2ae3d27d4eb4full, c = 0x165667b19e3779f9ull, d = 0x27d4eb2f165667c5ull;
    int64_t i = 0;
    for (; i + 4 <= n; i += 4) {
        a = (a ^ (uint64_t)p[i]) * 0x100000001b3ull;     b = (b ^ (uint64_t)p[i + 1]) * 0x100000001b3ull;
        c = (c ^ (uint64_t)p[i + 2]) * 0x100000001b3ull; d = (d ^ (uint64_t)p[i + 3]) * 0x100000001b3ull;
    }
    for (; i < n; ++i) a = (a ^ (uint64_t)p[i]) * 0x100000001b3ull;
    uint64_t x = a ^ (b * 3) ^ (c * 5) ^ (d * 7);
    x ^= x >> 29; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 32;
    return x;
}

// mine: this rank's table; on success `mine` holds the agreed table (equal entries as given, entries >= kEq the minimum
// over the ranks)
int fit_agree(chb_ctx *h, FitAgree *mine)
{
    constexpr int W = FitAgree::W;
    const int world = h->world;
    HIPCHK(h->xchg.agree.ensure((size_t)W * world));
    std::vector<int> all((size_t)W * world, 0);
    memcpy(all.data() + (size_t)W * h->rank, mine->v, sizeof(int) * W);
    HIPCHK(hipMemcpyAsync(h->xchg.agree.p + (size_t)W * h->rank, mine->v, sizeof(int) * W, hipMemcpyHostToDevice, h->stream));
    { const int r_ = exchange_all_gather(h, h->xchg.agree.p, (size_t)W, sizeof(int), ncclInt32); if (r_) return r_; }
    HIPCHK(hipMemcpyAsync(all.data(), h->xchg.agree.p, sizeof(int) * all.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int r = 0; r < world; ++r)
        for (int k = 0; k < FitAgree::kEq; ++k)
            if (all[(size_t)W * r + k] != all[k])   // (against rank 0's: every rank then reports the same pair)
                return fail(CHB_EINVAL, std::string("chb_fit_cluster: rank ") + std::to_string(r) + " and rank 0 differ in `" +
                                        kAgreeNames[k] + "` -- every rank of the communicator must make the same call on the "
                                        "same data with the same switches");
    for (int k = FitAgree::kEq; k < W; ++k) {
        int mn = all[k];
        for (int r = 1; r < world; ++r) mn = std::min(mn, all[(size_t)W * r + k]);
        mine->v[k] = mn;
    }
    return CHB_OK;
}

std::vector<int> to_i32(const int64_t *p, size_t n)
{
    std::vector<int> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (int)p[i];
    return v;
}

// ======== chb_fit_cluster_ex, stage by stage: its arguments are checked (fit_check_args), the fit is started
// (fit_begin_impl) and a FitScope takes over what the call sets on the context; a FitRun then carries the fit through its
// sweeps -- per sweep upload_perm, order_sweep, per batch run_batch and report_batch, then end_sweep.

// null checks, range checks and the up-front scan of the permutations
int fit_check_args(chb_ctx *h, const int64_t *initial_bins, const int64_t *perms, int64_t n_move, int max_iter,
                   const int64_t *labels_out, const double *min_dist_out, const double *margin_out)
{
    if (!h || !initial_bins || !labels_out) return fail(CHB_EINVAL, "null argument");
    if (margin_out && !min_dist_out) return fail(CHB_EINVAL, "margin_out needs min_dist_out");
    if (margin_out && h->world > 1) return fail(CHB_EUNSUPPORTED, "margin report is single-GPU");
    if (n_move > 0 && !perms) return fail(CHB_EINVAL, "perms is null");
    if (max_iter < 0 || n_move < 0 || n_move > h->N) return fail(CHB_EINVAL, "bad n_move/max_iter");
    HIPCHK(hipSetDevice(h->dev));
    if (h->world > 1 && !h->xchg.comm && !h->xchg.hook) return fail(CHB_ESTATE, "world > 1 but chb_comm_init was not called");
    if (!h->X.p) return fail(CHB_ESTATE, "chb_set_samples has not been called");
    // every permutation entry is range-checked BEFORE anything runs (a min / max pass the compiler vectorises), so a
    // bad entry in a late sweep cannot surface after earlier sweeps have already run; duplicates inside a sweep
    // are rejected while that sweep is converted for its upload (bitmap), and any error return closes the fit
    int64_t lo = 0, hi = 0;
    const int64_t tot = (int64_t)max_iter * n_move;
    for (int64_t i = 0; i < tot; ++i) { lo = std::min(lo, perms[i]); hi = std::max(hi, perms[i]); }
    if (lo < 0 || hi >= h->N) return fail(CHB_EINVAL, "perm entry out of range");
    return CHB_OK;
}

// default batch: 8192 positions on one GPU, growing with sqrt(world): the batch-member
// (update) work per rank is ~K^2/world, the per-rank grids ~K/world.  Twice that from 300k contigs to move: every
// batch rebuilds the CSR and the padded pack of ALL labelled contigs (cost ~ N per batch, ~ N^2 / K per sweep), while a
// batch is a smaller share of the sweep and collides with itself no more often (measured: 115 against 124 ms per sweep
// at 500k x 140 x 128, 517 against 538 at 1M x 146 x 200; 100k contigs are best served by 8192)
// (round 5, with the pools' cheaper shortlist launches: four times from 750k contigs -- 1M x 146 x 200: 342 against 361 ms per
//  sweep; 500k x 140 x 128 stays best at twice: 105.5 against 108.5)
int fit_default_batch(const chb_ctx *h, int64_t n_move, int m, int batch)
{
    int Kmax = batch > 0 ? batch : 8192 * std::max(1, (int)std::lround(std::sqrt((double)h->world))) *
                                       ((n_move >= 750000 && h->world == 1) ? 4 : (n_move >= 300000 ? 2 : 1));   // (sharded: as before)
    if (m > kMaxM && batch <= 0) Kmax = std::min(Kmax, 512);   // the plain kernels: one wavefront per (contig, bin)
    if (Kmax > n_move) Kmax = (int)std::max<int64_t>(n_move, 1);
    return Kmax;
}

// What a chb_fit_cluster_ex call sets on a context with a started fit holds for that call only: the margin report, the fit's
// persistent pack and threshold pools, the sweep's seating order, the switches the ranks agreed on, the look-ahead gate
// (error returns inside the window).  An error return must not leave an open fit / batch behind either.
struct FitScope {
    chb_ctx *h;
    bool skip, pack, spec;   // (the agreed switches hold for this fit only)
    bool ok = false;
    FitScope(chb_ctx *h_, bool want_margin) : h(h_), skip(h_->sw.allow_skip), pack(h_->sw.pp_allowed), spec(h_->sw.speculate)
    {
        h->want_margin = want_margin; h->pp.fit_scope(true); h->pool.fit_scope(true);
    }
    ~FitScope()
    {
        g_gate = Gate{};
        h->sw.allow_skip = skip; h->sw.pp_allowed = pack; h->sw.speculate = spec;
        h->pp.fit_scope(false); h->pool.fit_scope(false); h->seat.unseat();
        if (!ok) { (void)hipStreamSynchronize(h->stream); h->fit_open = false; h->batch.open = false; }
        h->want_margin = false;
    }
};

// ---- the fit driver's hooks for the developer builds (product build: none)
#ifdef CHB_DEV_KNOBS
// tests of the exchange schedule (tests/test_gpu_world2.py): CHB_DEV_HOOK_SPEC=1 runs the look-ahead over the host-staged hook
// (no gain, but the RCCL path's ORDER of exchanges); CHB_DEV_SKIP_STATS=<skipped>,<seen>,<unloaded> replaces this rank's
// tile-skipping statistics of every batch; CHB_DEV_LOCAL_VERDICT=1: each rank decides from its OWN ones
struct FitDev {
    static bool hook_spec(const chb_ctx *h) { return h->dk.hook_spec; }
    static bool local_verdict(const chb_ctx *h) { return h->dk.local_verdict; }
    static void skip_stats(chb_ctx *h)
    {
        if (h->dk.skip_stats_on) for (int k = 0; k < 3; ++k) launch_fill_i32(h->batch.fc_cur + kSlotSkipped + k, h->dk.skip_stats[k], 1, h->stream);
    }
    // CHB_PACK_REBUILD_AT=<rows>: rebuild (compact) the pack from that fill mark on -- tests of the rebuild path
    static int64_t rebuild_mark(const chb_ctx *h) { return h->dk.pack_rebuild_at >= 0 ? h->dk.pack_rebuild_at : h->pp.mark; }
    // CHB_DEV_ALL_DIST=<file> (tests/test_gpu_bin_distances.py; read per fit): with min_dist_out on one GPU, every hull distance
    // of each movable contig's last visit -- row perm[t0 + i] of an N x B float64 array (NaN rows for contigs never visited),
    // written raw to <file> when the fit succeeds.  (min_dist_out keeps the look-ahead off: nothing overwrites a batch's dist
    // before it is copied.)
    const char *all_path = nullptr;
    std::vector<double> all;
    void all_begin(const chb_ctx *h, bool wanted)
    {
        all_path = wanted ? getenv("CHB_DEV_ALL_DIST") : nullptr;
        all.assign(all_path ? (size_t)h->N * (size_t)h->B : 0, NAN);
    }
    int all_rows(chb_ctx *h, const int64_t *ids, int K)   // (the batch's K x B distances, each row to its contig's)
    {
        if (!all_path) return CHB_OK;
        std::vector<double> rows((size_t)K * h->B);
        HIPCHK(hipMemcpy(rows.data(), h->dist.p, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < K; ++i)
            memcpy(all.data() + (size_t)ids[i] * h->B, rows.data() + (size_t)i * h->B, sizeof(double) * h->B);
        return CHB_OK;
    }
    int all_write() const
    {
        if (!all_path) return CHB_OK;
        FILE *fp = fopen(all_path, "wb");
        const bool ok = fp && fwrite(all.data(), sizeof(double), all.size(), fp) == all.size();
        if (fp) fclose(fp);
        return ok ? CHB_OK : fail(CHB_EINVAL, std::string("CHB_DEV_ALL_DIST: cannot write ") + all_path);
    }
};
#else
struct FitDev {
    static bool hook_spec(const chb_ctx *) { return false; }
    static bool local_verdict(const chb_ctx *) { return false; }
    static void skip_stats(chb_ctx *) {}
    static int64_t rebuild_mark(const chb_ctx *h) { return h->pp.mark; }
    void all_begin(const chb_ctx *, bool) {}
    int all_rows(chb_ctx *, const int64_t *, int) { return CHB_OK; }
    int all_write() const { return CHB_OK; }
};
#endif

// the positions [t0, t0 + K) of a sweep's permutation as one batch: this rank evaluates [q_lo, q_hi) of it, C per rank
struct Geom { int64_t t0; int K, q_lo, q_hi, C; };

// host-side batch state, saved where a look-ahead window opens (the device side of a gated-off batch never changed)
struct LookaheadSnap {
    BatchState batch; bool pp_batch, pp_valid, pool_valid; std::array<int64_t, 4> stats; size_t n_pending;
    static LookaheadSnap save(const chb_ctx *h)
    {
        return LookaheadSnap{h->batch, h->pp.batch, h->pp.valid, h->pool.valid, h->stats, h->prof.pending.size()};
    }
    void restore(chb_ctx *h) const
    {
        h->batch = batch; h->pp.batch = pp_batch; h->pp.valid = pp_valid; h->pool.valid = pool_valid; h->stats = stats;
        // the launches recorded inside the window were gated off (they returned at once): they are neither
        // launches nor work of the profile
        for (size_t i = n_pending; i < h->prof.pending.size(); ++i) {
            (void)hipEventDestroy(h->prof.pending[i].a);
            (void)hipEventDestroy(h->prof.pending[i].b);
        }
        if (h->prof.pending.size() > n_pending) h->prof.pending.resize(n_pending);
    }
};

struct FitRun {
    // the call's arguments
    chb_ctx *h;
    const int64_t *perms;
    int64_t n_move;
    int max_iter;
    int64_t *labels_out;
    double *min_dist_out, *margin_out;
    // fixed for the fit (can_spec: once the ranks have agreed on the switches)
    int64_t N;
    hipStream_t s;
    int Kmax, world;
    bool xchg;              // the rounds' labels travel through an all-gather: more than one rank, or CHB_FORCE_GATHER
    bool can_spec = false;
    // the sweeps
    int it = 0;
    int64_t assigned0 = 0, labelled = 0;   // labelled samples at the fit's start / after the last sweep
    std::vector<int> prev;                 // labels before the current sweep
    bool sweep_has_labelled = true;
    std::vector<int64_t> batch_t0;         // first position of every batch of the sweep (empty: its batches order themselves)
    std::vector<double> mind_host, mind2_host;
    std::vector<uint64_t> seen_bits;
    // the batches of a sweep
    bool inflight = false;   // the batch's start and first round went out with its predecessor's look-ahead
    bool spec_ok = false;    // (a failed guess switches the look-ahead off until a batch converges in one round again)
    int slot = 0;            // verdict slot of the batch
    FitDev dev;

    FitRun(chb_ctx *h_, const int64_t *perms_, int64_t n_move_, int max_iter_, int Kmax_, int64_t *labels_out_,
           double *min_dist_out_, double *margin_out_)
        : h(h_), perms(perms_), n_move(n_move_), max_iter(max_iter_), labels_out(labels_out_), min_dist_out(min_dist_out_), margin_out(margin_out_), N(h_->N), s(h_->stream), Kmax(Kmax_), world(h_->world),
          xchg((h_->xchg.comm != nullptr || h_->xchg.hook != nullptr) && (h_->world > 1 || h_->sw.force_gather))
    {
    }

    const int64_t *perm() const { return perms + (int64_t)it * n_move; }   // the current sweep's
    // the tag of the fit's next exchange (kind 1: a batch's label guess, 2: a round's labels)
    int next_tag(int kind) { const int t = ((h->xchg.seq & 0x7ffffff) << 4) | kind; h->xchg.seq += 1; return t; }

    // ---- more than one rank: agree on the fit before its first collective (fit_agree)
    int fit_agree_switches(const int64_t *initial_bins)
    {
        h->xchg.seq = 0;
        if (xchg) {
            FitAgree fa{};
            const uint64_t hp = hash_i64(perms, (int64_t)max_iter * n_move), hi_ = hash_i64(initial_bins, N);
            const int eq[FitAgree::kEq] = {0x43480005, h->B, h->m, (int)(n_move & 0x7fffffff), max_iter, Kmax, (int)(N & 0x7fffffff),
                                           h->D, h->metric, h->fused ? 1 : 0, h->pf_fit ? 1 : 0, min_dist_out ? 1 : 0,
                                           (int)(hp & 0x7fffffff), (int)((hp >> 32) & 0x7fffffff), (int)(hi_ & 0x7fffffff),
                                           (int)((hi_ >> 32) & 0x7fffffff)};
            memcpy(fa.v, eq, sizeof(eq));
            fa.v[16] = h->seat.state; fa.v[17] = h->sw.speculate ? 1 : 0; fa.v[18] = h->sw.allow_skip ? 1 : 0; fa.v[19] = h->sw.pp_allowed ? 1 : 0;
            fa.v[20] = h->pool.valid ? h->pool.state : -1;
            const int rc = fit_agree(h, &fa);
            if (rc) return rc;
            h->seat.state = fa.v[16]; h->sw.speculate = fa.v[17] != 0; h->sw.allow_skip = fa.v[18] != 0; h->sw.pp_allowed = fa.v[19] != 0;
            if (fa.v[20] < 0) { h->pool.state = -1; h->pool.valid = false; }
        }
        // (look-ahead under an exchange: the RCCL all-gather sits on the context's stream, so the first-changed position of
        //  a round is computed on the device right behind it and feeds the same gate as on one GPU; every rank sees the same
        //  labels, hence the same verdict, and the all-gathers of a gated-off batch move identical bytes between the ranks'
        //  identical buffers.  The hook transport needs the host between rounds anyway.)
        can_spec = h->sw.speculate && h->fused && (!xchg || (h->xchg.hook == nullptr && h->xchg.comm != nullptr) || FitDev::hook_spec(h)) &&
                   min_dist_out == nullptr;
        return CHB_OK;
    }

    // the labels the fit starts from, the NaN-filled reports
    void begin_outputs()
    {
        dev.all_begin(h, min_dist_out && !xchg);
        // (fit_begin_impl left the converted initial labels in pin_a; their upload and the kernels of the fit's start are
        //  still running -- nothing below touches pin_a again before the sweep's final synchronisation)
        prev.assign(h->pin_a.p, h->pin_a.p + N);
        if (min_dist_out) {
            for (int64_t i = 0; i < N; ++i) min_dist_out[i] = NAN;
            mind_host.resize((size_t)Kmax);
        }
        if (margin_out) {
            for (int64_t i = 0; i < N; ++i) margin_out[i] = NAN;
            mind2_host.resize((size_t)Kmax);
        }
        for (int64_t i = 0; i < N; ++i) assigned0 += prev[(size_t)i] >= 0;
        labelled = assigned0;
    }

    // the sweep's permutation: converted into its pinned staging buffer, checked for duplicates, uploaded
    int upload_perm()
    {
        HIPCHK(h->perm.ensure((size_t)std::max<int64_t>(n_move, 1)));
        HIPCHK(h->pin_c.ensure((size_t)std::max<int64_t>(n_move, 1)));
        if (!n_move) return CHB_OK;
        // (pin_c, the permutations' own staging buffer: the previous sweep's upload from it completed before that
        //  sweep's final synchronisation, and the first sweep's conversion overlaps the kernels of the fit's start)
        const int64_t *pm = perm();
        seen_bits.assign((size_t)(N + 63) / 64, 0);
        uint64_t dup = 0;
        int any_lab = 0;   // does this sweep visit a sample that carries a label?  (sweep 1 normally does not)
        for (int64_t i = 0; i < n_move; ++i) {
            const int64_t v = pm[i];          // (in range: checked up front)
            uint64_t &wd = seen_bits[(size_t)(v >> 6)];
            const uint64_t bit = 1ull << (v & 63);
            dup |= wd & bit;
            wd |= bit;
            h->pin_c.p[i] = (int)v;
            any_lab |= prev[(size_t)v] >= 0;
        }
        sweep_has_labelled = any_lab != 0;
        if (dup) return fail(CHB_EINVAL, "a sweep's permutation lists a sample twice");
        HIPCHK(hipMemcpyAsync(h->perm.p, h->pin_c.p, sizeof(int) * n_move, hipMemcpyHostToDevice, s));
        return CHB_OK;
    }

    Geom geom_at(int64_t t0) const
    {
        // sweep 1 starts from few labelled members: do not let a batch outnumber them by much
        // (measured: a batch of up to 1.5x the labelled members costs no extra rounds and saves a batch)
        int64_t members = (it == 0) ? (assigned0 + t0) * 3 / 2 : N;
        int K = (int)std::min<int64_t>(Kmax, n_move - t0);
        if (members < K) K = (int)std::max<int64_t>(std::min<int64_t>(64, n_move - t0), members);
        K = std::min(K, Kmax);   // (the floor of 64 above must not exceed a caller's smaller batch: buffers hold Kmax)
        // multi-GPU: rank r evaluates positions [r*C, (r+1)*C) of the batch; the label slices
        // are exchanged with one in-place RCCL all-gather per round (KB-sized)
        const int C = (K + world - 1) / world;
        const int q_lo = std::min(K, h->rank * C);
        return Geom{t0, K, q_lo, std::min(K, q_lo + C), C};
    }

    // the seating order of every batch of this sweep (tile skipping / threshold pools), in one launch: the batches are a
    // function of the sweep alone.  (Not for sweeps of thousands of tiny batches: those order theirs one by one.)
    int order_sweep()
    {
        h->seat.unseat();
        batch_t0.clear();
        if (!(h->pf_fit && h->fused && h->seat.ckey.p != nullptr && n_move > 0 && (h->pool.valid || (h->sw.allow_skip && h->seat.state >= 0))))
            return CHB_OK;
        std::vector<int4> geo;
        for (int64_t t = 0; t < n_move && geo.size() <= 4096;) {
            const Geom g = geom_at(t);
            geo.push_back(make_int4((int)g.t0, g.q_lo, g.q_hi, g.K));
            batch_t0.push_back(t);
            t += g.K;
        }
        if (geo.size() > 4096) { batch_t0.clear(); return CHB_OK; }
        HIPCHK(h->seat.geo_all.ensure(geo.size()));
        HIPCHK(h->seat.qord_all.ensure((size_t)n_move));
        HIPCHK(h->seat.home_all.ensure(geo.size() * (size_t)h->B));
        // (pinned staging: the previous sweep's upload from it completed before that sweep's final synchronisation)
        HIPCHK(h->seat.pin_geo.ensure(geo.size()));
        memcpy(h->seat.pin_geo.p, geo.data(), sizeof(int4) * geo.size());
        HIPCHK(hipMemcpyAsync(h->seat.geo_all.p, h->seat.pin_geo.p, sizeof(int4) * geo.size(), hipMemcpyHostToDevice, s));
        Timed t(h, "bucket", (double)n_move);
        launch_query_order_sweep(h->seat.ckey.p, h->perm.p, h->seat.geo_all.p, (int)geo.size(), h->B, h->seat.qord_all.p, h->seat.home_all.p, s);
        return CHB_OK;
    }

    // after a round's kernels: (multi-GPU: exchange) + first-changed position on its way to the host
    int finish_round(const Geom &g, int active, int slot_)
    {
        if (xchg) {
            // this rank's frame {tag, skip and pool statistics of the batch's base shortlist launch, the pack's fill mark, label
            // slice} -> all-gather -> every rank's labels into lab_new / lab_prev, first changed position, statistics summed over
            // the ranks (gated kernels, not memcpys: inside a look-ahead window they must not run; single rank without exchange:
            // the argmin kernel has already written lab_prev).  What comes home in the verdict slot is then the SAME on
            // every rank -- first change, bin sizes (functions of the replicated labels), skip and pool statistics, arena mark --
            // and with it every decision of this loop, in particular whether the next batch is enqueued ahead.
            const int tag = next_tag(2);
            const bool first = active == 0;
            if (first) FitDev::skip_stats(h);
            launch_xchg_pack(h->xchg.xg.p, h->rank, g.C, h->lab_new.p, tag, h->batch.fc_cur, first, first && h->pp.batch, true, g.K, s);
            { const int r_ = exchange_all_gather(h, h->xchg.xg.p, (size_t)(g.C + kXchgHdr), sizeof(int), ncclInt32); if (r_) return r_; }
            launch_xchg_unpack(h->xchg.xg.p, world, g.C, g.K, tag, h->lab_new.p, h->lab_prev.p, active, h->batch.fc_cur,
                               first && !FitDev::local_verdict(h), h->xchg.xerr.p, s);
        }
        HIPCHK(hipMemcpyAsync(h->fc_host + kSlotInts * slot_, h->batch.fc_cur, kSlotHome * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(h->fc_event[slot_], s));
        return CHB_OK;
    }

    // the verdict as it came home (SlotWord); nullptr: the wait failed
    const int *wait_verdict(int slot_)
    {
        const hipError_t e = hipEventSynchronize(h->fc_event[slot_]);
        if (e != hipSuccess) { fail(CHB_EHIP, std::string("hipEventSynchronize(h->fc_event[slot]): ") + hipGetErrorString(e)); return nullptr; }
        return h->fc_host + kSlotInts * slot_;
    }

    // What the host takes from a verdict besides the first change -- no HIP call in here.  The slot's statistics are written
    // by the batch's one base shortlist launch: counted with the batch's first round only (later rounds of the same batch
    // bring the same numbers home again).
    void note_verdict(const int *v, bool first_round)
    {
        // (bin sizes of that batch, for the segment decision of the batches still to be enqueued)
        h->seg.hint_max_tiles = v[kSlotMaxTiles]; h->seg.hint_total_tiles = v[kSlotTotalTiles];
        // (the persistent pack's arena: rows handed out so far, as of that batch's start)
        if (h->pp.valid && v[kSlotMark] > FitDev::rebuild_mark(h)) h->pp.rebuild = true;
        if (!first_round) return;
        // (what the tile skipping of its shortlist launch achieved: a fit whose first batches skip next to nothing turns it off)
        if (v[kSlotSeen] > 0) {
            h->seat.skipped += v[kSlotSkipped]; h->seat.seen += v[kSlotSeen]; h->seat.unloaded += v[kSlotUnloaded];
            if (h->seat.state == 0 && ++h->seat.batches >= 3) {
                // (it pays from a few per cent of the wave-tiles)
                h->seat.state = ((h->seat.skipped + h->seat.unloaded) * 50 >= h->seat.seen + h->seat.unloaded) ? 1 : -1;
                if (h->seat.state < 0) h->seat.off_key = skip_key(h);
            }
        }
        // Where tile skipping never loads a third of a bin's tiles (500k x 140 x 128: 45 %), the threshold sweep is
        // cheap already and the pools' price -- the looser thresholds of the contigs far out in their bins: long
        // shortlists, retries, label guesses that fail -- is higher than what they save (113 against 105 ms per
        // sweep there; 1M x 146 x 200, 19 % never loaded: 366 against 460): such a fit drops them
        // (checked per batch: sweep 1's first batches stream bins of a few tiles, nothing to go by)
        if (h->seat.state == 1 && h->pool.state >= 0 && v[kSlotSeen] > 0) {
            const long long un = v[kSlotUnloaded], sn = v[kSlotSeen];
            if (un * 10 > 3 * (sn + un)) { h->pool.state = -1; h->pool.off_key = skip_key(h); }
        }
        // (threshold pools: candidates per pair of that batch's base shortlist launch, as sampled; a fit whose first
        //  batches admit far more than the exact threshold would -- overlapping bins -- goes back to the two sweeps
        //  -- checked for EVERY batch: the pools of sweep 1's first batches hold whole bins and say nothing yet)
        if (h->pool.state >= 0 && v[kSlotPoolPairs] > 0) {
            const long long pc = v[kSlotPoolCand], pp = v[kSlotPoolPairs];
            h->pool.cand += pc; h->pool.pairs += pp;
            if (++h->pool.batches >= 3 && h->pool.state == 0) h->pool.state = 1;
            // (the benchmark configurations admit m + 0.1 .. m + 0.4 per pair; from m + 3 on the loose thresholds cost the
            //  update stage and the hull kernel more than the threshold sweep did)
            if (pc > (long long)(h->m + 3) * pp) { h->pool.state = -1; h->pool.off_key = skip_key(h); }
        }
    }

    // a round's verdict, waited for and taken note of; *f = its first changed position
    int round_verdict(int slot_, bool first_round, int *f)
    {
        const int *v = wait_verdict(slot_);
        if (!v) return CHB_EHIP;
        *f = v[kSlotFirstChange];
        note_verdict(v, first_round);
        return CHB_OK;
    }

    // batch start + guess + round 0, nothing read back
    int open_batch(const Geom &g, int slot_)
    {
        h->batch.bq_cur = h->perm.p + g.t0;   // the batch's sample indices: a window of the sweep's permutation
        h->batch.fc_cur = h->first_change.p + kSlotInts * slot_;
        if (!batch_t0.empty()) {
            const size_t bi = (size_t)(std::lower_bound(batch_t0.begin(), batch_t0.end(), g.t0) - batch_t0.begin());
            h->seat.qord_cur = h->seat.qord_all.p + g.t0 + g.q_lo; h->seat.home_cur = h->seat.home_all.p + bi * (size_t)h->B;
        }
        h->batch.hint_base_members = (double)((it == 0) ? assigned0 + g.t0 : labelled - g.K);
        h->batch.hint_batch_entries = (double)((it == 0) ? g.K : 2 * g.K);
        h->argmin_in_place = !xchg;
        // (an all-unlabelled batch makes no holes in the pools: nothing to open, nothing for its commit to look for)
        h->pool.batch_labelled = sweep_has_labelled;
        int r = batch_begin_dev(h, g.K, g.q_lo, g.q_hi, false);
        h->pool.batch_labelled = true;
        if (r) return r;
        // starting labels of the rounds: last sweep's label, or for still-unlabelled contigs
        // (sweep 1) the bin whose m-th nearest outside member is closest
        if (h->fused && !h->batch.lists_valid) launch_guess_near(h->tau.p, h->lab_old.p, g.q_lo, g.q_hi, h->B, h->Kcap, h->lab_prev.p, s);
        else launch_guess(h->l0d.p, h->l0c.p, h->lab_old.p, g.q_lo, g.q_hi, h->B, h->m, h->Kcap, h->lab_prev.p, s);
        if (xchg) {
            const int tag = next_tag(1);
            launch_xchg_pack(h->xchg.xg.p, h->rank, g.C, h->lab_prev.p, tag, h->batch.fc_cur, false, false, false, g.K, s);
            { const int r_ = exchange_all_gather(h, h->xchg.xg.p, (size_t)(g.C + kXchgHdr), sizeof(int), ncclInt32); if (r_) return r_; }
            launch_xchg_unpack(h->xchg.xg.p, world, g.C, g.K, tag, h->lab_prev.p, nullptr, 0, h->batch.fc_cur, false, h->xchg.xerr.p, s);
        }
        r = batch_round_dev(h, 0);
        if (r) return r;
        return finish_round(g, 0, slot_);
    }

    // A batch = start (selection against the members outside it), a label guess, then rounds until the first changed
    // position is past its end.  On one GPU the NEXT batch is enqueued while the first round's verdict is still on its way
    // to the host: its kernels (and this batch's commit) carry a gate on that verdict and return at once if the round
    // did not converge, in which case the remaining rounds run and the next batch is enqueued again.
    // The stream never drains while rounds converge at once -- the common case after sweep 1's start;
    // a failed guess switches the look-ahead off until a batch converges in one round again.
    int run_batch(const Geom &g)
    {
        const int K = g.K;
        int rc;
        if (!inflight) { rc = open_batch(g, slot); if (rc) return rc; }
        const int64_t t1 = g.t0 + K;
        // (a batch start that has to build or rebuild the persistent pack stays outside the look-ahead window)
        const bool skip_would = h->sw.allow_skip && h->seat.nsh > 1 && h->seat.state >= 0 && h->seat.ckey.p != nullptr;
        const bool pack_sync = h->pp.fit && h->sw.pp_allowed && h->fused && h->cand.p && !skip_would &&
                               (!h->pp.valid || h->pp.rebuild);
        const bool spec = spec_ok && t1 < n_move && !pack_sync;
        LookaheadSnap snap{};
        if (spec) {
            snap = LookaheadSnap::save(h);
            g_gate = Gate{h->first_change.p + kSlotInts * slot, K};   // "this batch's round 0 changed nothing"
            rc = batch_commit_dev(h, h->lab_prev.p);
            if (rc) return rc;
            rc = open_batch(geom_at(t1), slot ^ 1);
            if (rc) return rc;
            g_gate = Gate{};
        }
        int f = K;
        rc = round_verdict(slot, true, &f);
        if (rc) return rc;
        if (f >= K) {
            inflight = spec;   // the next batch's first round is already running
            if (spec) h->stats_lookahead += 1;
            spec_ok = can_spec;
            return CHB_OK;
        }
        // the guess was off at position f: everything enqueued behind the gate has skipped itself
        if (spec) { snap.restore(h); spec_ok = false; h->stats_lookahead_failed += 1; }
        for (int active = f + 1; active < K; active = f + 1) {
            rc = batch_round_dev(h, active);
            if (rc) return rc;
            rc = finish_round(g, active, slot);
            if (rc) return rc;
            rc = round_verdict(slot, false, &f);
            if (rc) return rc;
            if (f >= K) break;
        }
        inflight = false;
        return CHB_OK;
    }

    // min_dist_out / margin_out of the batch's contigs (the look-ahead is off: nothing has overwritten them)
    int report_batch(const Geom &g)
    {
        if (!min_dist_out) return CHB_OK;
        const int K = g.K;
        const int64_t *ids = perm() + g.t0;
        if (xchg)
            { const int r_ = exchange_all_gather(h, h->mind.p, (size_t)g.C, sizeof(double), ncclFloat64); if (r_) return r_; }
        HIPCHK(hipMemcpyAsync(mind_host.data(), h->mind.p, sizeof(double) * K, hipMemcpyDeviceToHost, s));
        if (margin_out)
            HIPCHK(hipMemcpyAsync(mind2_host.data(), h->mind2.p, sizeof(double) * K, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < K; ++i) min_dist_out[ids[i]] = mind_host[(size_t)i];
        // (runner-up +inf: no other bin has a member -- +inf also when no bin has one, not inf - inf)
        if (margin_out)
            for (int i = 0; i < K; ++i) {
                const double w = mind_host[(size_t)i], r = mind2_host[(size_t)i];
                margin_out[ids[i]] = r == INFINITY ? INFINITY : r - w;
            }
        return dev.all_rows(h, ids, K);
    }

    // ---- the batches of this sweep
    int run_sweep()
    {
        int rc = upload_perm();
        if (rc) return rc;
        rc = order_sweep();
        if (rc) return rc;
        inflight = false; spec_ok = can_spec; slot = 0;
        for (int64_t t0 = 0; t0 < n_move;) {
            const Geom g = geom_at(t0);
            rc = run_batch(g);
            if (rc) return rc;
            rc = report_batch(g);
            if (rc) return rc;
            if (!inflight) {   // (otherwise the commit went out with the look-ahead)
                rc = batch_commit_dev(h, h->lab_prev.p);
                if (rc) return rc;
            } else {
                slot ^= 1;
            }
            h->stats[0] += 1;
            t0 += g.K;
        }
        h->stats[3] += n_move * (int64_t)h->B;
        return CHB_OK;
    }

    // the sweep's labels come home with the device's error words; *diff = labels the sweep changed (algorithm.py:63)
    int end_sweep(int64_t *diff)
    {
        HIPCHK(h->pin_b.ensure((size_t)N));
        HIPCHK(hipMemcpyAsync(h->pin_b.p, h->labels.p, sizeof(int) * N, hipMemcpyDeviceToHost, s));
        if (h->fused && h->short_cnt.p)   // (spare words of the first verdict slot)
            HIPCHK(hipMemcpyAsync(h->fc_host + kSlotShortCnt, h->short_cnt.p, sizeof(int), hipMemcpyDeviceToHost, s));
        h->fc_host[kSlotPackErr] = 0;
        if (h->pp.ctl.p)
            HIPCHK(hipMemcpyAsync(h->fc_host + kSlotPackErr, h->pp.ctl.p + 2, sizeof(int), hipMemcpyDeviceToHost, s));
        std::vector<int> xend;
        if (xchg) {
            // every rank's "a rank was out of step" record: all ranks then leave the sweep with the same status
            xend.assign((size_t)4 * world, 0);
            HIPCHK(hipMemcpyAsync(h->xchg.agree.p + 4 * h->rank, h->xchg.xerr.p, 4 * sizeof(int), hipMemcpyDeviceToDevice, s));
            { const int r_ = exchange_all_gather(h, h->xchg.agree.p, 4, sizeof(int), ncclInt32); if (r_) return r_; }
            HIPCHK(hipMemcpyAsync(xend.data(), h->xchg.agree.p, sizeof(int) * xend.size(), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        for (int r = 0; r < (int)xend.size() / 4; ++r)
            if (xend[(size_t)4 * r] != 0) {
                HIPCHK(hipMemsetAsync(h->xchg.xerr.p, 0, 4 * sizeof(int), s));
                const int *e = xend.data() + 4 * r;
                return fail(CHB_ESTATE, "internal error: the ranks' exchanges fell out of step (rank " + std::to_string(r) + " was at exchange " +
                                        std::to_string(e[1] >> 4) + " kind " + std::to_string(e[1] & 15) + " when rank " + std::to_string(e[3]) +
                                        " sent exchange " + std::to_string(e[2] >> 4) + " kind " + std::to_string(e[2] & 15) +
                                        "); labels not returned");
            }
        if (h->fc_host[kSlotPackErr] != 0)
            return fail(CHB_ESTATE, "internal error: the persistent member pack ran out of rows; labels not returned");
        if (h->fused && h->short_cnt.p && h->fc_host[kSlotShortCnt] != 0)
            return fail(CHB_ESTATE, "internal error: " + std::to_string(h->fc_host[kSlotShortCnt]) + " (position, bin) shortlists of this sweep came "
                        "out short of min(num_neighbors, bin size) candidates or held a wild index; labels not returned");
        // (one pass: change count, label count and the caller's int64 copy -- the last sweep's is what stays)
        const int *pb = h->pin_b.p;
        const int *pv = prev.data();
        *diff = 0;
        labelled = 0;
        for (int64_t i = 0; i < N; ++i) {
            const int v = pb[i];
            *diff += pv[i] != v;
            labelled += v >= 0;
            labels_out[i] = v;
        }
        return CHB_OK;
    }
};

}  // namespace

// the resident copy X[N][Dp] (rows zero-padded to Dp): filled from `X` (host or device), or -- X == nullptr -- left to
// be filled by the caller (chb_bcast_samples on a receiving rank)
static int samples_upload(chb_ctx *h, const double *X, int64_t N, int64_t D, bool from_device)
{
    if (N <= 0 || D <= 0) return fail(CHB_EINVAL, "samples must be a non-empty N x D matrix");
    if (N >= (1LL << 31) - 64 || D > (1 << 20)) return fail(CHB_EUNSUPPORTED, "N or D too large");
    HIPCHK(hipSetDevice(h->dev));
    // rows padded to whole 128-byte lines (16 doubles): a 16-lane group of the hull kernels reads a row in 256-byte pieces
    // from its start, and a row that starts in the middle of a line makes every piece touch three lines instead of two
#ifndef CHB_ROW_PAD
#define CHB_ROW_PAD 16
#endif
    static_assert(CHB_ROW_PAD % kKChunk == 0, "the tile kernels stage kKChunk columns at a time");
    const int Dp = (int)((D + CHB_ROW_PAD - 1) / CHB_ROW_PAD) * CHB_ROW_PAD;
    HIPCHK(h->X.ensure((size_t)N * Dp));
    if (X != nullptr) {
        if (Dp != D) HIPCHK(hipMemsetAsync(h->X.p, 0, sizeof(double) * (size_t)N * Dp, h->stream));
        HIPCHK(hipMemcpy2DAsync(h->X.p, sizeof(double) * Dp, X, sizeof(double) * D, sizeof(double) * D,
                                (size_t)N, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                h->stream));
    }
    h->N = N; h->D = (int)D; h->Dp = Dp;
    h->fit_open = false; h->batch.open = false; h->stepwise = false;
    return CHB_OK;
}

// everything that is a function of the resident X alone (global mean, scale, query-side shadow rows)
static int samples_finish(chb_ctx *h)
{
    h->seat.off_key = -1; h->pool.off_key = -1; h->pool.kept = false;
    const int64_t N = h->N, D = h->D;
    const int Dp = h->Dp;
    // the shortlist stage (prefilter_kernels.hip) keeps its query fragments in registers: D <= 157 in the narrow builds,
    // D <= 573 as two to four 144-column slices in the wide ones (shadow_row_elems)
    h->shadow_ok = false;
    const int Dz = shadow_row_elems((int)D);
    if (h->sw.use_prefilter && Dz > 0) {
        // global mean, the power-of-two scale that puts every centred feature inside +-2^11, and the
        // query-side shadow row of every sample: functions of X alone
        const int part_blocks = 1024;
        HIPCHK(h->mu_g.ensure((size_t)Dp));
        HIPCHK(h->colsum_part.ensure((size_t)part_blocks * Dp));
        HIPCHK(h->rmax.ensure(1));
        HIPCHK(h->Gs.ensure((size_t)N * Dz));
        HIPCHK(h->gq.ensure((size_t)N * 2));
        HIPCHK(h->Zs.ensure((size_t)N * Dz));
        HIPCHK(h->ms.ensure((size_t)N * 4));
        launch_global_center(h->X.p, (int)N, (int)D, Dp, h->colsum_part.p, part_blocks, h->mu_g.p, h->rmax.p,
                             h->stream);
        unsigned int rbits = 0;
        HIPCHK(hipMemcpyAsync(&rbits, h->rmax.p, sizeof(rbits), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        float R;
        memcpy(&R, &rbits, sizeof(R));
        double S = 1.0;
        if (R > 0.f && std::isfinite(R)) {
            int e = 0;
            (void)std::frexp((double)R, &e);   // R < 2^e
            S = std::ldexp(1.0, 10 - e);       // |x - mu_c| S <= 2 R S < 2^11: every member's -bias / 2 then fits the three
                                               // fp16 bias columns of its shadow row (prefilter_kernels.hip, kBiasExp)
            if (Dz > 160) S *= 0.5;            // wide rows (D <= 573): |x - mu_c| S < 2^10, -bias / 2 <= D 2^21 / 2 < 2^29.2
        }
        h->shadow_scale = S;
        launch_global_shadow(h->X.p, (int)N, (int)D, Dp, h->mu_g.p, S, h->Gs.p, Dz, h->gq.p, h->stream);
        HIPCHK(hipGetLastError());
        h->Dz = Dz;
        // the m <= 5 fused kernel's view of these rows (FusedArgs::trim)
        HIPCHK(h->trim_ctr.ensure_zeroed(3, h->stream));
        HIPCHK(h->trim_args.ensure(1));
        const TrimArgs ta{h->Gs.p, reinterpret_cast<const float2 *>(h->gq.p), Dz, h->trim_ctr.p};
        HIPCHK(hipMemcpyAsync(h->trim_args.p, &ta, sizeof(ta), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));   // (ta is a local)
        h->shadow_ok = true;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CHB_OK;
}

namespace chb {

int set_samples_common(chb_ctx *h, const double *X, int64_t N, int64_t D, bool from_device)
{
    if (!h) return fail(CHB_EINVAL, "null context");
    if (!X) return fail(CHB_EINVAL, "samples must be a non-empty N x D matrix");
    const int rc = samples_upload(h, X, N, D, from_device);
    return rc ? rc : samples_finish(h);
}

}  // namespace chb

extern "C" {

const char *chb_last_error(void) { return g_err.c_str(); }
int chb_version(void) { return 1; }

int chb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int chb_create(int device_id, chb_ctx **out)
{
    if (!out) return fail(CHB_EINVAL, "out is null");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(CHB_ENODEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= n) return fail(CHB_EINVAL, "device_id out of range");
    HIPCHK(hipSetDevice(device_id));
    chb_ctx *h = new chb_ctx();
    h->dev = device_id;
    read_switches(h);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->fc_host, 128, hipHostMallocDefault);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->fc_event[i], hipEventDisableTiming);
    if (e != hipSuccess) { delete h; return fail(CHB_EHIP, hipGetErrorString(e)); }
    *out = h;
    return CHB_OK;
}

int chb_destroy(chb_ctx *h)
{
    if (!h) return CHB_OK;
    (void)hipSetDevice(h->dev);
    (void)hipStreamSynchronize(h->stream);
    if (h->score.copy) (void)hipStreamSynchronize(h->score.copy);
    drain_profile(h);
    if (h->xchg.comm && rccl()) { (void)rccl()->CommDestroy(h->xchg.comm); h->xchg.comm = nullptr; }
    // the handles without an owner; the buffers (DevBuf / PinBuf, PackBufs) free themselves when `delete h` destroys them
    for (ChunkHalf &half : h->score.half) half.destroy_events();
    for (hipEvent_t e : h->fc_event) if (e) (void)hipEventDestroy(e);
    if (h->score.copy) (void)hipStreamDestroy(h->score.copy);
    if (h->fc_host) (void)hipHostFree(h->fc_host);
    (void)hipStreamDestroy(h->stream);
    delete h;
    return CHB_OK;
}

int chb_set_samples(chb_ctx *h, const double *X, int64_t N, int64_t D)
{
    return set_samples_common(h, X, N, D, false);
}

int chb_set_samples_device(chb_ctx *h, const double *X, int64_t N, int64_t D)
{
    return set_samples_common(h, X, N, D, true);
}

int chb_bcast_samples(chb_ctx *h, const double *X, int64_t N, int64_t D, int root)
{
    if (!h) return fail(CHB_EINVAL, "null context");
    if (!h->xchg.comm) return fail(CHB_ESTATE, "chb_bcast_samples needs chb_comm_init (RCCL)");
    if (root < 0 || root >= h->world) return fail(CHB_EINVAL, "bad root");
    // Every rank reports {its own status, N, D, root} BEFORE the collective: a rank that returned early (no matrix on the
    // root, an allocation that failed) or ranks that disagree about the shape would otherwise leave the others blocked in
    // ncclBroadcast for good, or broadcast into buffers of the wrong size.
    int rc = (h->rank == root && !X) ? fail(CHB_EINVAL, "the root rank must pass the matrix")
                                     : samples_upload(h, h->rank == root ? X : nullptr, N, D, false);
    {
        const std::string my_err = g_err;
        const int world = h->world;
        HIPCHK(h->xchg.agree.ensure((size_t)4 * world));
        std::vector<int> all((size_t)4 * world, 0);
        int *mine = all.data() + 4 * h->rank;
        mine[0] = rc; mine[1] = (int)(N & 0x7fffffff); mine[2] = (int)(D & 0x7fffffff); mine[3] = root;
        HIPCHK(hipMemcpyAsync(h->xchg.agree.p + 4 * h->rank, mine, 4 * sizeof(int), hipMemcpyHostToDevice, h->stream));
        NCCLCHK(rccl()->AllGather(h->xchg.agree.p + 4 * h->rank, h->xchg.agree.p, 4, ncclInt32, h->xchg.comm, h->stream));
        HIPCHK(hipMemcpyAsync(all.data(), h->xchg.agree.p, sizeof(int) * all.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (rc) return fail(rc, my_err);
        for (int r = 0; r < world; ++r) {
            const int *o = all.data() + 4 * r;
            if (o[0] != 0)
                return fail(CHB_ESTATE, "chb_bcast_samples: rank " + std::to_string(r) + " failed before the broadcast (status " +
                                        std::to_string(o[0]) + ")");
            if (o[1] != mine[1] || o[2] != mine[2] || o[3] != mine[3])
                return fail(CHB_EINVAL, "chb_bcast_samples: rank " + std::to_string(r) + " passed a different N, D or root");
        }
    }
    // the padded resident copy goes out as it lies on the root: one RCCL broadcast over xGMI
    NCCLCHK(rccl()->Broadcast(h->X.p, h->X.p, (size_t)N * (size_t)h->Dp, ncclDouble, root, h->xchg.comm, h->stream));
    return samples_finish(h);
}

int chb_comm_info(chb_ctx *h, int *rank, int *world, int *comm_ranks, int *transport)
{
    if (!h) return fail(CHB_EINVAL, "null context");
    if (rank) *rank = h->rank;
    if (world) *world = h->world;
    int cnt = 0;
    if (h->xchg.comm && rccl()) NCCLCHK(rccl()->CommCount(h->xchg.comm, &cnt));
    if (comm_ranks) *comm_ranks = cnt;
    if (transport) *transport = h->xchg.comm ? 1 : (h->xchg.hook ? 2 : 0);
    return CHB_OK;
}

int chb_fit_begin(chb_ctx *h, int64_t B, const int64_t *initial_bins, int m)
{
    if (!h || !initial_bins) return fail(CHB_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->dev));
    const int rc = fit_begin_impl(h, B, initial_bins, m);
    if (rc == CHB_OK) h->stepwise = true;
    // (the stepwise batches have no loop that reads the skip statistics and could turn the tile-skipping builds off
    //  where they do not pay: they run the ordinary builds)
    if (rc == CHB_OK) h->seat.state = -1;
    return rc;
}

int chb_batch_begin(chb_ctx *h, const int64_t *perm_slice, int64_t K, int64_t q_lo, int64_t q_hi)
{
    if (!h || !perm_slice) return fail(CHB_EINVAL, "null argument");
    if (!h->fit_open) return fail(CHB_ESTATE, "chb_fit_begin has not been called");
    if (h->batch.open) return fail(CHB_ESTATE, "previous batch not committed");
    if (K <= 0 || K > (1 << 24) || q_lo < 0 || q_hi > K || q_lo > q_hi)
        return fail(CHB_EINVAL, "bad batch geometry");
    HIPCHK(hipSetDevice(h->dev));
    {
        // (the batch start counts every labelled sample and subtracts the batch's own entries: a sample listed twice
        //  would be subtracted twice)
        std::vector<uint64_t> seen((size_t)(h->N + 63) / 64, 0);
        for (int64_t i = 0; i < K; ++i) {
            const int64_t v = perm_slice[i];
            if (v < 0 || v >= h->N) return fail(CHB_EINVAL, "perm entry out of range");
            uint64_t &wd = seen[(size_t)(v >> 6)];
            if (wd & (1ull << (v & 63))) return fail(CHB_EINVAL, "a batch lists a sample twice");
            wd |= 1ull << (v & 63);
        }
    }
    if ((int)K > h->Kcap) { int rc = ensure_batch_buffers(h, (int)K); if (rc) return rc; }
    std::vector<int> v = to_i32(perm_slice, (size_t)K);
    h->batch.bq_cur = h->bq.p;
    HIPCHK(hipMemcpyAsync(h->batch.bq_cur, v.data(), sizeof(int) * K, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return batch_begin_dev(h, (int)K, (int)q_lo, (int)q_hi, false);
}

// the labels a caller hands a round or a commit index the per-bin arrays on the device: -1 (unassigned) or a bin
static int check_label_range(const int64_t *lab, int K, int B, const char *what)
{
    for (int i = 0; i < K; ++i)
        if (lab[i] < -1 || lab[i] >= B)
            return fail(CHB_EINVAL, std::string(what) + "[" + std::to_string(i) + "] = " + std::to_string(lab[i]) +
                                    " is outside [-1, num_clusters)");
    return CHB_OK;
}

int chb_batch_round(chb_ctx *h, const int64_t *lab_prev, int64_t active, int64_t *lab_new,
                    double *min_dist)
{
    if (!h || !lab_prev || !lab_new) return fail(CHB_EINVAL, "null argument");
    if (!h->batch.open) return fail(CHB_ESTATE, "no open batch");
    const int K = h->batch.K;
    // (host checks before anything is enqueued: a refused call leaves the batch open and as it was)
    if (active < 0 || active > K) return fail(CHB_EINVAL, "active must be in [0, K]");
    // the rounds keep the distance of a (position, bin) pair whose candidates are those of the previous round: that round
    // must have evaluated the position
    if (active < h->round_active) return fail(CHB_EINVAL, "active must not decrease within a batch");
    { const int rc = check_label_range(lab_prev, K, h->B, "lab_prev"); if (rc) return rc; }
    HIPCHK(hipSetDevice(h->dev));
    h->round_active = active;
    std::vector<int> v = to_i32(lab_prev, (size_t)K);
    HIPCHK(hipMemcpyAsync(h->lab_prev.p, v.data(), sizeof(int) * K, hipMemcpyHostToDevice, h->stream));
    h->argmin_in_place = false;
    int rc = batch_round_dev(h, (int)active);
    if (rc) return rc;
    const int lo = std::max((int)active, h->batch.q_lo), hi = h->batch.q_hi;
    if (hi > lo) {
        std::vector<int> ln((size_t)(hi - lo));
        HIPCHK(hipMemcpyAsync(ln.data(), h->lab_new.p + lo, sizeof(int) * (hi - lo), hipMemcpyDeviceToHost, h->stream));
        if (min_dist)
            HIPCHK(hipMemcpyAsync(min_dist + lo, h->mind.p + lo, sizeof(double) * (hi - lo), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int i = lo; i < hi; ++i) lab_new[i] = ln[(size_t)(i - lo)];
    } else {
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return CHB_OK;
}

int chb_batch_guess(chb_ctx *h, int64_t *guess)
{
    if (!h || !guess) return fail(CHB_EINVAL, "null argument");
    if (!h->batch.open) return fail(CHB_ESTATE, "no open batch");
    HIPCHK(hipSetDevice(h->dev));
    const int lo = h->batch.q_lo, hi = h->batch.q_hi;
    if (hi <= lo) return CHB_OK;
    if (h->fused && !h->batch.lists_valid) launch_guess_near(h->tau.p, h->lab_old.p, lo, hi, h->B, h->Kcap, h->lab_prev.p, h->stream);
    else launch_guess(h->l0d.p, h->l0c.p, h->lab_old.p, lo, hi, h->B, h->m, h->Kcap, h->lab_prev.p, h->stream);
    HIPCHK(hipGetLastError());
    std::vector<int> g((size_t)(hi - lo));
    HIPCHK(hipMemcpyAsync(g.data(), h->lab_prev.p + lo, sizeof(int) * (hi - lo), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = lo; i < hi; ++i) guess[i] = g[(size_t)(i - lo)];
    return CHB_OK;
}

int chb_batch_commit(chb_ctx *h, const int64_t *final_labels)
{
    if (!h || !final_labels) return fail(CHB_EINVAL, "null argument");
    if (!h->batch.open) return fail(CHB_ESTATE, "no open batch");
    { const int rc = check_label_range(final_labels, h->batch.K, h->B, "final_labels"); if (rc) return rc; }
    HIPCHK(hipSetDevice(h->dev));
    std::vector<int> v = to_i32(final_labels, (size_t)h->batch.K);
    HIPCHK(hipMemcpyAsync(h->lab_prev.p, v.data(), sizeof(int) * h->batch.K, hipMemcpyHostToDevice, h->stream));
    int rc = batch_commit_dev(h, h->lab_prev.p);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return CHB_OK;
}

int chb_fit_labels(chb_ctx *h, int64_t *labels_out)
{
    if (!h || !labels_out) return fail(CHB_EINVAL, "null argument");
    if (!h->fit_open) return fail(CHB_ESTATE, "chb_fit_begin has not been called");
    HIPCHK(hipSetDevice(h->dev));
    std::vector<int> v((size_t)h->N);
    HIPCHK(hipMemcpyAsync(v.data(), h->labels.p, sizeof(int) * h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < h->N; ++i) labels_out[i] = v[(size_t)i];
    return CHB_OK;
}

int chb_fit_cluster(chb_ctx *h, int64_t B, const int64_t *initial_bins, const int64_t *perms,
                    int64_t n_move, int m, int max_iter, int batch, int64_t *labels_out,
                    int *iters_run, int64_t *changed_per_iter, double *min_dist_out)
{
    return chb_fit_cluster_ex(h, B, initial_bins, perms, n_move, m, max_iter, batch, labels_out, iters_run,
                              changed_per_iter, min_dist_out, nullptr);
}

int chb_fit_cluster_ex(chb_ctx *h, int64_t B, const int64_t *initial_bins, const int64_t *perms,
                       int64_t n_move, int m, int max_iter, int batch, int64_t *labels_out,
                       int *iters_run, int64_t *changed_per_iter, double *min_dist_out, double *margin_out)
{
    int rc = fit_check_args(h, initial_bins, perms, n_move, max_iter, labels_out, min_dist_out, margin_out);
    if (rc) return rc;
    rc = fit_begin_impl(h, B, initial_bins, m, /*sync=*/false);
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }   // (an upload from pin_a may be in flight: the next call rewrites it)
    h->stepwise = false;
    FitScope scope(h, margin_out != nullptr);
    // threshold pools: built from the initial labels (the CSR of the fit's start is still in place), unless an earlier fit
    // over the same samples, bins and neighbour count found that they do not pay (overlapping bins: long shortlists; or tile
    // skipping that never loads 30 % of the tiles)
    h->pool.fit_reset(h->pool.off_key == skip_key(h));
    if (h->pool.state >= 0) { rc = pool_build(h); if (rc) return rc; }
    const int Kmax = fit_default_batch(h, n_move, m, batch);
    h->last_batch = Kmax;
    rc = ensure_batch_buffers(h, Kmax);
    if (rc) return rc;
    h->stats.fill(0); h->seg.stat_batches = 0; h->stats_lookahead = 0; h->stats_lookahead_failed = 0;

    FitRun run(h, perms, n_move, max_iter, Kmax, labels_out, min_dist_out, margin_out);
    rc = run.fit_agree_switches(initial_bins);
    if (rc) return rc;
    run.begin_outputs();
    bool wrote_out = false;
    for (; run.it < max_iter; ++run.it) {
        int64_t diff = 0;
        rc = run.run_sweep();
        if (rc) return rc;
        rc = run.end_sweep(&diff);
        if (rc) return rc;
        wrote_out = true;
        if (changed_per_iter) changed_per_iter[run.it] = diff;
        if (diff == 0) { ++run.it; break; }  // algorithm.py:64-66
        if (run.it + 1 < max_iter) run.prev.assign(h->pin_b.p, h->pin_b.p + h->N);   // algorithm.py:71-72
    }
    if (!wrote_out)
        for (int64_t i = 0; i < h->N; ++i) labels_out[i] = run.prev[(size_t)i];
    if (iters_run) *iters_run = run.it;
    rc = run.dev.all_write();
    if (rc) return rc;
    scope.ok = true;
    return CHB_OK;
}

int chb_topm_per_bin(chb_ctx *h, const int64_t *labels, int64_t B, int m, const int64_t *query_idx,
                     int64_t Q, int64_t *nbr_idx, double *nbr_dist, int32_t *nbr_cnt)
{
    if (!h || !labels || !query_idx || !nbr_idx || !nbr_cnt) return fail(CHB_EINVAL, "null argument");
    if (Q < 0) return fail(CHB_EINVAL, "Q < 0");
    HIPCHK(hipSetDevice(h->dev));
    std::vector<int64_t> lab((size_t)h->N);
    for (int64_t i = 0; i < h->N; ++i) lab[(size_t)i] = (labels[i] >= 0 && labels[i] < B) ? labels[i] : -1;
    int rc = fit_begin_impl(h, B, lab.data(), m);
    if (rc) return rc;
    h->stepwise = false;
    for (int64_t i = 0; i < Q; ++i)
        if (query_idx[i] < 0 || query_idx[i] >= h->N) return fail(CHB_EINVAL, "query index out of range");
    const int Kmax = (int)std::min<int64_t>(std::max<int64_t>(Q, 1), 4096);
    rc = ensure_batch_buffers(h, Kmax);
    if (rc) return rc;
    hipStream_t s = h->stream;
    std::vector<double> hd;
    std::vector<int> hi, hc;
    int64_t t0 = 0;
    while (t0 < Q) {
        // a chunk must not contain the same sample twice
        std::unordered_set<int64_t> seen;
        int K = 0;
        while (t0 + K < Q && K < Kmax && seen.insert(query_idx[t0 + K]).second) ++K;
        std::vector<int> v = to_i32(query_idx + t0, (size_t)K);
        h->batch.bq_cur = h->bq.p;
        HIPCHK(hipMemcpyAsync(h->batch.bq_cur, v.data(), sizeof(int) * K, hipMemcpyHostToDevice, s));
        rc = batch_begin_dev(h, K, 0, K, true);
        if (rc) return rc;
        // every other query of the chunk is an ordinary member: code "pos != i"
        launch_bucket_batch(h->lab_old.p, nullptr, h->batch.bq_cur, K, h->B, h->cnt2.p, h->bin_ptr2.p,
                            h->cursor2.p, h->memb2_id.p, h->memb2_code.p, nullptr, nullptr, nullptr, nullptr, s);
        TopmArgs a = h->topm_args(0, K);
        a.bin_ptr = h->bin_ptr2.p; a.memb_id = h->memb2_id.p; a.memb_code = h->memb2_code.p;
        a.in = h->L0(); a.out = h->L1();
        {
            Timed t(h, "topm_update", (double)K);
            if (h->m > kMaxM) launch_topm_generic(a, s); else launch_topm(a, s);
        }
        HIPCHK(hipGetLastError());
        const size_t nB = (size_t)h->B, nm = (size_t)m, cap = (size_t)h->Kcap;
        hd.resize(nB * cap * nm); hi.resize(nB * cap * nm); hc.resize(nB * cap);
        HIPCHK(hipMemcpyAsync(hd.data(), h->l1d.p, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hi.data(), h->l1i.p, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hc.data(), h->l1c.p, sizeof(int) * hc.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < K; ++i)
            for (size_t c = 0; c < nB; ++c) {
                const size_t slot = c * cap + (size_t)i;
                const size_t o = ((size_t)(t0 + i) * nB + c);
                nbr_cnt[o] = hc[slot];
                for (size_t e = 0; e < nm; ++e) {
                    nbr_idx[o * nm + e] = hi[slot * nm + e];
                    if (nbr_dist) nbr_dist[o * nm + e] = hd[slot * nm + e];
                }
            }
        rc = batch_commit_dev(h, h->lab_old.p);  // labels unchanged
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(s));
        t0 += K;
    }
    h->fit_open = false;
    return CHB_OK;
}

// ======== row scoring (chb_recruit_rows, chb_audit_rows, chb_*_rows_multi, chb_bin_report, chb_*_pairs, and their _grouped,
// _witness, _nearest and _wide forms): the entry point fills a ScoreRequest by name, the body of its call shape (score_rows,
// bin_report, score_pairs, score_nearest) checks the arguments (score_check_args), a ScoreRun carries it through its stages
namespace {

constexpr int kRecruitPiece = 2048;   // rows per host-to-device copy of a chunk

// chb_bin_report's five tables as the caller wants them (any may be null)
struct ReportOut { int64_t *confusion, *unplaced, *dcnt; double *dmin, *dsum; };

// chb_bin_report's part of a ScoreRun: the scored positions (those whose own label lies in [0, B)) in label order -- a
// stable counting sort, so a label's positions keep the order of row_idx -- and the chunks cut from that order: at most
// kRecruitChunk positions each, cut back to the last kReportBlock-row block boundary of the label a cut would split, so
// that no summation block of dsum (BinReportArgs) lies in two chunks.
// (chb_bin_report_wide with more than 16 neighbours: at most `limit` positions each, the rows a dense wide chunk may hold
// -- a multiple of kReportBlock, so a cut never falls back onto the cut before it.)
struct ReportPlan {
    int64_t B = 0;
    int64_t max_rows = 0;            // of any chunk
    std::vector<int> ord;            // [Qv] sample index of every scored position, grouped by label
    std::vector<int64_t> lab_ptr;    // [B + 1] label a's run is ord[lab_ptr[a] .. lab_ptr[a + 1])
    std::vector<int64_t> cut;        // chunk k is ord[cut[k] .. cut[k + 1])
    // the plan of the positions row_idx[0 .. Q) (nullptr: position = sample); returns Qv, the others are only counted
    int64_t build(const int64_t *labels, int64_t B_, const int64_t *row_idx, int64_t Q, int64_t limit = kRecruitChunk)
    {
        B = B_;
        lab_ptr.assign((size_t)B + 1, 0);
        auto own = [&](int64_t q) { return labels[row_idx ? row_idx[q] : q]; };
        int64_t Qv = 0;
        for (int64_t q = 0; q < Q; ++q) {
            const int64_t l = own(q);
            if (l >= 0 && l < B) { ++lab_ptr[(size_t)l + 1]; ++Qv; }
        }
        if (Qv == 0) return 0;
        for (int64_t c = 0; c < B; ++c) lab_ptr[(size_t)c + 1] += lab_ptr[(size_t)c];
        ord.resize((size_t)Qv);
        std::vector<int64_t> cur(lab_ptr.begin(), lab_ptr.end() - 1);
        for (int64_t q = 0; q < Q; ++q) {
            const int64_t l = own(q);
            if (l >= 0 && l < B) ord[(size_t)cur[(size_t)l]++] = (int)(row_idx ? row_idx[q] : q);
        }
        cut.assign(1, 0);
        while (cut.back() < Qv) {
            int64_t c1 = std::min<int64_t>(Qv, cut.back() + limit);
            if (c1 < Qv) {   // inside (or at the start of) the label whose run holds position c1
                const size_t l = (size_t)(std::upper_bound(lab_ptr.begin(), lab_ptr.end(), c1) - lab_ptr.begin()) - 1;
                c1 -= (c1 - lab_ptr[l]) % kReportBlock;
            }
            max_rows = std::max(max_rows, c1 - cut.back());
            cut.push_back(c1);
        }
        return Qv;
    }
    // nothing to score: the tables of a call without rows
    void empty_tables(const ReportOut &o) const
    {
        const size_t BB = (size_t)B * (size_t)B;
        if (o.confusion) std::fill(o.confusion, o.confusion + BB, (int64_t)0);
        if (o.unplaced) std::fill(o.unplaced, o.unplaced + B, (int64_t)0);
        if (o.dcnt) std::fill(o.dcnt, o.dcnt + BB, (int64_t)0);
        if (o.dmin) std::fill(o.dmin, o.dmin + BB, std::numeric_limits<double>::infinity());
        if (o.dsum) std::fill(o.dsum, o.dsum + BB, 0.0);
    }
    // the context's tables, behind the last chunk
    int copy_tables(chb_ctx *h, const ReportOut &o) const
    {
        const RowScoring &sc = h->score;
        hipStream_t s = h->stream;
        const size_t BB = (size_t)B * (size_t)B;
        static_assert(sizeof(long long) == sizeof(int64_t), "the tables are copied out as they are");
        if (o.confusion) HIPCHK(hipMemcpyAsync(o.confusion, sc.rep_conf.p, sizeof(int64_t) * BB, hipMemcpyDeviceToHost, s));
        if (o.unplaced) HIPCHK(hipMemcpyAsync(o.unplaced, sc.rep_unplaced.p, sizeof(int64_t) * (size_t)B, hipMemcpyDeviceToHost, s));
        if (o.dcnt) HIPCHK(hipMemcpyAsync(o.dcnt, sc.rep_cnt.p, sizeof(int64_t) * BB, hipMemcpyDeviceToHost, s));
        if (o.dmin) HIPCHK(hipMemcpyAsync(o.dmin, sc.rep_min.p, sizeof(double) * BB, hipMemcpyDeviceToHost, s));
        if (o.dsum) HIPCHK(hipMemcpyAsync(o.dsum, sc.rep_sum.p, sizeof(double) * BB, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return CHB_OK;
    }
};

// chb_audit_pairs / chb_recruit_pairs' part of a ScoreRun: the P pairs in bin order -- a stable counting sort, so a bin's
// pairs keep the caller's order --, every bin's run cut into tiles of at most kQTile positions (a tile is a work item of
// the kernel: RecruitPairArgs), and the chunks: runs of whole tiles with at most kRecruitChunk positions.
struct PairPlan {
    const int64_t *row = nullptr;      // [P] the row of input pair p: a sample (row_idx) or a row of Y (row_of)
    std::vector<int64_t> ord;          // [P] the input pair at every position
    std::vector<int4> tile;            // {bin, first position in its chunk, positions, 0}
    std::vector<int64_t> cut, tcut;    // chunk k is the positions cut[k] .. cut[k + 1), the tiles tcut[k] .. tcut[k + 1)
    int64_t max_rows = 0, max_tiles = 0;   // of any chunk
    void build(const int64_t *row_, const int64_t *bin_idx, int64_t P, int64_t B)
    {
        row = row_;
        std::vector<int64_t> ptr((size_t)B + 1, 0);
        for (int64_t p = 0; p < P; ++p) ++ptr[(size_t)bin_idx[p] + 1];
        for (int64_t c = 0; c < B; ++c) ptr[(size_t)c + 1] += ptr[(size_t)c];
        ord.resize((size_t)P);
        std::vector<int64_t> cur(ptr.begin(), ptr.end() - 1);
        for (int64_t p = 0; p < P; ++p) ord[(size_t)cur[(size_t)bin_idx[p]]++] = p;
        cut.assign(1, 0);
        tcut.assign(1, 0);
        int64_t filled = 0;   // positions of the chunk being filled
        auto close = [&](int64_t pos) {
            max_rows = std::max(max_rows, pos - cut.back());
            max_tiles = std::max(max_tiles, (int64_t)tile.size() - tcut.back());
            cut.push_back(pos);
            tcut.push_back((int64_t)tile.size());
            filled = 0;
        };
        for (int64_t c = 0; c < B; ++c)
            for (int64_t t0 = ptr[(size_t)c]; t0 < ptr[(size_t)c + 1]; t0 += kQTile) {
                const int64_t cnt = std::min<int64_t>(kQTile, ptr[(size_t)c + 1] - t0);
                if (filled + cnt > kRecruitChunk) close(t0);
                tile.push_back(make_int4((int)c, (int)filled, (int)cnt, 0));
                filled += cnt;
            }
        close(P);
    }
};

// What a row-scoring call asks for: made by audit() / recruit() below, the rest set by name by its entry point and
// the call body behind it
struct ScoreRequest {
    const int64_t *labels = nullptr; int64_t B = 0;
    // the source, one of four: the new rows Y (recruit); the resident rows row_idx, nullptr meaning all rows (audit);
    // a plan's positions (chb_bin_report: an audit whose chunks are the plan's cuts); a pair plan's positions (below)
    const double *Y = nullptr; const int64_t *row_idx = nullptr; const ReportPlan *plan = nullptr;
    int64_t Q = 0;
    int m = 0; const int *ms = nullptr; int nm = 0;   // neighbours; nm > 0: the list of a chb_*_rows_multi call, m its largest entry
    // (without a destination: neither downloaded nor unpacked)
    int64_t *bin_out = nullptr; double *dist_out = nullptr, *min_dist_out = nullptr, *margin_out = nullptr;
    // chb_*_pairs: Q pairs (row, bin) in place of the grid, the rows resident or (Y set) rows of Y; dist_out is [Q], one
    // double per pair in the caller's order, and there is no row reduction.  With a list (nm > 0: chb_*_pairs_multi)
    // dist_out is [nm][Q], slice j the pair call's answer at ms[j]; the plan and its chunks are the single call's
    const PairPlan *pairs = nullptr;
    // chb_*_grouped: one group id per resident sample, negative = no group; besides the scored row every sample of its
    // group is withheld (leave-group-out).  grouped marks the call, whose groups must not be null
    bool grouped = false;
    const int64_t *groups = nullptr;
    // chb_*_pairs_witness: a pair call that also returns, per pair, the hull's members, their selection distances and
    // their weights ([Q][m] each, in the caller's order; each may be null, not all three); dist_out may then be null
    bool witness = false;
    int64_t *w_idx = nullptr; double *w_dist = nullptr, *w_alpha = nullptr;
    // chb_*_rows_nearest: a dense call whose rows are ranked on the device in place of the row reduction; per row the
    // near_k nearest bins and their distances ([Q][near_k] each, either may be null, not both).  nearest marks the call
    bool nearest = false;
    int near_k = 0;
    int64_t *near_bin = nullptr; double *near_dist = nullptr;
    // chb_*_wide with 16 < m <= 64: the two wide kernels per chunk in place of recruit_kernel; the pair forms may return
    // the selection lists ([Q][m], -1 padded, in the caller's order).  Combines with nearest (the ranking reads the wide
    // chunk's table), plan (cut at wide_chunk_rows) and witness (m slots per pair: the ids are idx_out, w_idx stays null).
    // With a list (nm > 0: chb_*_rows_multi_wide, a dense call with an entry above 16): one selection at the largest entry,
    // the entries up to 16 by recruit_kernel's list launch, those above by the solve kernel's list form
    bool wide = false;
    int64_t *idx_out = nullptr;
    // the two makers: Q resident rows row_idx (or pairs of them), Q new rows Y (or pairs of rows of Y)
    static ScoreRequest audit(const int64_t *labels, int64_t B, int m, const int64_t *row_idx, int64_t Q)
    {
        ScoreRequest rq;
        rq.labels = labels; rq.B = B; rq.m = m; rq.row_idx = row_idx; rq.Q = Q;
        return rq;
    }
    static ScoreRequest recruit(const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q)
    {
        ScoreRequest rq;
        rq.labels = labels; rq.B = B; rq.m = m; rq.Y = Y; rq.Q = Q;
        return rq;
    }
};

// The argument checks of the entry points, for all of them in this order: null context; ranges and a malformed list
// (CHB_EINVAL; a nearest-bins call's k < 1 among them); null arguments (a grouped call's groups, whatever Q, among them);
// outputs; no samples; D; more than 16 neighbours (CHB_EUNSUPPORTED), then a nearest-bins call's k > 16; more than 8192
// bins; an open stepwise fit; Q == 0 (CHB_OK: nothing further is read); the row_idx rules.
// (A wide call, rq.wide: more than 64 neighbours, then more than 32 on a device without the LDS for 64 vertices, in place of
// "more than 16".  wide_rule sets rq.wide only above 16 neighbours, so a _wide symbol never reaches "more than 16".
// A wide list, chb_*_rows_multi_wide with an entry above 16: the same, and its entries are told apart up to 64.)
// who: the name the call goes by in the texts (wide_rule: a _wide symbol's narrow twin up to 16 neighbours).
// D: the rows' number of columns in the calls that take Y, nullptr in the others.  list: the call takes ms / nm, whose
// largest entry becomes rq.m.  no_output: the refusal's text when every output that counts for the call is null, else nullptr.
int score_check_args(chb_ctx *h, const char *who, ScoreRequest &rq, const int64_t *D, bool list, const char *no_output)
{
    if (!h) return fail(CHB_EINVAL, "null context");
    if (list) {
        if (rq.Q < 0 || rq.B < 1) return fail(CHB_EINVAL, "Q < 0 or B < 1");
        if (!rq.ms) return fail(CHB_EINVAL, "ms is null");
        if (rq.nm < 1 || rq.nm > kMaxM) return fail(CHB_EINVAL, "nm must be 1 .. 16");
        // 1 .. 16 distinct entries in 1 .. 16, a wide list's (chb_*_rows_multi_wide) in 1 .. 64 (an entry above that is
        // refused below and sets no bit here)
        const int top = rq.wide ? kMaxMGeneric : kMaxM;
        unsigned long long seen = 0;
        rq.m = 0;
        for (int j = 0; j < rq.nm; ++j) {
            if (rq.ms[j] < 1) return fail(CHB_EINVAL, "an entry of ms is < 1");
            const unsigned long long bit = rq.ms[j] <= top ? 1ull << (rq.ms[j] - 1) : 0;
            if (seen & bit) return fail(CHB_EINVAL, "ms holds a value twice");
            seen |= bit;
            rq.m = std::max(rq.m, rq.ms[j]);
        }
    } else if (rq.Q < 0 || rq.B < 1 || rq.m < 1) {
        return fail(CHB_EINVAL, "Q < 0, B < 1 or m < 1");
    }
    if (rq.nearest && rq.near_k < 1) return fail(CHB_EINVAL, "k < 1");
    if (rq.Q > 0 && (!rq.labels || (D && !rq.Y))) return fail(CHB_EINVAL, "null argument");
    if (rq.grouped && !rq.groups) return fail(CHB_EINVAL, std::string(who) + ": groups is null (the call without groups is the one to use)");
    if (no_output) return fail(CHB_EINVAL, no_output);
    if (!h->X.p) return fail(CHB_ESTATE, "chb_set_samples has not been called");
    if (D && *D != h->D) return fail(CHB_EINVAL, "the rows must have the resident samples' number of columns");
    if (rq.wide) {   // (the wide calls: the limit lifted to 64, and the LDS the 64-vertex solve kernel needs)
        if (rq.m > kMaxMGeneric) return fail(CHB_EUNSUPPORTED, std::string(who) + " supports at most 64 neighbours");
        if (rq.m > 32 && !hull_generic_supported())
            return fail(CHB_EUNSUPPORTED, std::string(who) + ": more than 32 neighbours need 66 KiB of LDS per workgroup, which this device does not grant");
    } else if (rq.m > kMaxM) return fail(CHB_EUNSUPPORTED, std::string(who) + " supports at most 16 neighbours");
    if (rq.nearest && rq.near_k > kMaxNearest) return fail(CHB_EUNSUPPORTED, std::string(who) + " supports at most 16 nearest bins (k)");
    if (rq.B > kRecruitMaxBins) return fail(CHB_EUNSUPPORTED, std::string(who) + " supports at most 8192 bins");
    if (h->batch.open || (h->fit_open && h->stepwise))
        return fail(CHB_ESTATE, "a stepwise fit is open on this context (chb_fit_begin): chb_set_samples ends it");
    if (rq.Q == 0 || D) return CHB_OK;   // (the calls that take Y have no row_idx)
    if (!rq.row_idx && rq.Q != h->N) return fail(CHB_EINVAL, "row_idx is null (all rows): Q must be the number of resident samples");
    for (int64_t q = 0; rq.row_idx && q < rq.Q; ++q)
        if (rq.row_idx[q] < 0 || rq.row_idx[q] >= h->N) return fail(CHB_EINVAL, "row_idx entry outside [0, N)");
    return CHB_OK;
}

// rows of a dense wide chunk: the largest multiple of 64 whose width x (m + 1) int lists fit the list buffer, in [64, 16384]
int64_t wide_chunk_rows(int64_t width, int m)
{
    const int64_t fit = kWideListBytes / (width * (m + 1) * (int64_t)sizeof(int)) / kQTile * kQTile;
    return std::min<int64_t>(kRecruitChunk, std::max<int64_t>(kQTile, fit));
}

// One row-scoring call behind its checks: its stages in call order, then the steps of its pipeline.  The chunks go through
// the two halves of the context's RowScoring: chunk k is staged in pinned memory and copied up on the copy stream, the
// kernels run on the context's stream, the results come down on the copy stream into pinned memory and are unpacked by
// the host.  Everything asynchronous reads and writes context-owned memory.
struct ScoreRun {
    chb_ctx *h;
    const ScoreRequest rq;
    RowScoring &sc = h->score;
    hipStream_t s = h->stream;
    const bool audit = !rq.Y /* the rows are resident */, any_out = rq.bin_out || rq.dist_out || rq.min_dist_out || rq.margin_out || rq.witness || rq.nearest || rq.idx_out;
    const int ns = rq.nm > 0 ? rq.nm : 1;   // result slices per chunk
    const size_t width = rq.pairs ? 1 : (size_t)rq.B;   // distances per result row
    const size_t wslots = rq.wide ? (size_t)rq.m : (size_t)kWitnessSlots;   // slots of a position's witness record
    int slot[kMaxM] = {0};                  // list entry j's slice on the device = the number of smaller entries
    // a wide list (chb_*_rows_multi_wide): its entries up to 16 -- their number and the largest, for recruit_kernel's list
    // launch -- and those above, ascending, for the solve kernel's list form; the slices of the first stand before the others'
    int n_narrow = 0, m_narrow = 0, n_wide = 0;
    unsigned char m_wide[kMaxM] = {0};
    size_t n_memb = 0;
    int64_t chunk = 0, n = 0;               // rows per chunk (a plan: its cuts), chunks
    RecruitWitnessArgs a{};   // (the launchers without witnesses take the part of it that is theirs)
    int64_t start(int64_t k) const { return rq.pairs ? rq.pairs->cut[(size_t)k] : rq.plan ? rq.plan->cut[(size_t)k] : k * chunk; }
    int rows(int64_t k) const { return (int)(std::min<int64_t>(start(k + 1), rq.Q) - start(k)); }
    ChunkHalf &half(int64_t k) { return sc.half[k & 1]; }
    // the copy stream and the halves' events: created by the context's first row-scoring call
    int ensure_copy_stream()
    {
        if (sc.copy) return CHB_OK;
        HIPCHK(hipStreamCreateWithFlags(&sc.copy, hipStreamNonBlocking));
        for (ChunkHalf &b : sc.half)
            for (hipEvent_t *ev : {&b.up, &b.done, &b.down}) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
        return CHB_OK;
    }
    // chb_*_grouped: the caller's group ids (any non-negative int64, not dense) as dense int32 ids in pinned memory, once
    // per call; every sample without a group gets -1, which the kernel never takes for a group
    int dense_groups()
    {
        if (!rq.groups) return CHB_OK;
        const int64_t N = h->N, *groups = rq.groups;
        HIPCHK(sc.hgrp.ensure((size_t)N));
        std::vector<int64_t> ids;
        for (int64_t i = 0; i < N; ++i)
            if (groups[i] >= 0) ids.push_back(groups[i]);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        for (int64_t i = 0; i < N; ++i)
            sc.hgrp.p[i] = groups[i] < 0 ? -1 : (int)(std::lower_bound(ids.begin(), ids.end(), groups[i]) - ids.begin());
        return CHB_OK;
    }
    // CSR over the labels (host counting sort into pinned memory; members of a bin in index order -- the selection does
    // not depend on it); with groups also every member's group id, parallel to the member list
    int label_csr()
    {
        const int64_t N = h->N, B = rq.B, *labels = rq.labels;
        HIPCHK(sc.hptr.ensure((size_t)B + 1));
        int *ptr = sc.hptr.p;
        std::fill(ptr, ptr + B + 1, 0);
        for (int64_t i = 0; i < N; ++i)
            if (labels[i] >= 0 && labels[i] < B) ++ptr[labels[i] + 1];
        for (int64_t c = 0; c < B; ++c) ptr[c + 1] += ptr[c];
        n_memb = (size_t)std::max(ptr[B], 1);
        HIPCHK(sc.hmemb.ensure(n_memb));
        std::vector<int> cur(ptr, ptr + B);
        for (int64_t i = 0; i < N; ++i)
            if (labels[i] >= 0 && labels[i] < B) sc.hmemb.p[cur[(size_t)labels[i]]++] = (int)i;
        if (!rq.groups) return CHB_OK;
        HIPCHK(sc.hmgrp.ensure(n_memb));
        sc.hmgrp.p[0] = -1;   // (without a member: n_memb is 1 and the entry is never read)
        for (int e = 0; e < ptr[B]; ++e) sc.hmgrp.p[e] = sc.hgrp.p[sc.hmemb.p[e]];
        return CHB_OK;
    }
    // a list of m: its mask for the kernel, and where the unpack step finds entry j's slice
    void list_slots()
    {
        for (int j = 0; j < rq.nm; ++j) {
            for (int k = 0; k < rq.nm; ++k) slot[j] += rq.ms[k] < rq.ms[j];
            if (rq.ms[j] <= kMaxM) {
                a.mmask |= 1u << (rq.ms[j] - 1);
                ++n_narrow; m_narrow = std::max(m_narrow, rq.ms[j]);
            } else m_wide[n_wide++] = (unsigned char)rq.ms[j];   // (only a wide list has such entries: at most 64)
        }
        std::sort(m_wide, m_wide + n_wide);
    }
    // chunk length and buffers.  A list's chunks are kRecruitChunk / nm rows, rounded down to whole 64-row tiles, so the
    // nm result slices of a chunk fill no more than a single-m chunk's buffers.
    int size_buffers()
    {
        const int64_t B = rq.B;
        const int64_t list_rows = rq.nm > 0 ? std::max<int64_t>(kQTile, kRecruitChunk / rq.nm / kQTile * kQTile) : 0;
        // (a list of pairs, chb_*_pairs_multi: the pair plan's chunks as they are -- nm doubles per pair are at most 2 MiB --
        // and of the counters only what the single pair call at its largest entry sets)
        if (rq.nm > 0 && !rq.wide && !rq.pairs) sc.multi_rows = list_rows;
        if (rq.wide) sc.wide_rows = wide_chunk_rows((int64_t)width, rq.m);
        // (a wide list: both bounds -- the lists of its largest entry within the list buffer, its nm slices within a chunk's)
        if (rq.wide && rq.nm > 0 && !rq.pairs) sc.wide_rows = std::min(sc.wide_rows, list_rows);
        // (a wide plan: cut at wide_rows by its builder, so its longest chunk is what the buffers must hold)
        chunk = rq.pairs ? rq.pairs->max_rows : rq.plan && rq.wide ? rq.plan->max_rows
              : std::min<int64_t>(rq.Q, rq.wide ? sc.wide_rows : rq.nm > 0 ? sc.multi_rows : kRecruitChunk);
        n = rq.pairs ? (int64_t)rq.pairs->cut.size() - 1 : rq.plan ? (int64_t)rq.plan->cut.size() - 1 : (rq.Q + chunk - 1) / chunk;
        const size_t res = (size_t)chunk * (size_t)ns;   // result rows of a chunk
        const int halves = rq.Q > chunk ? 2 : 1;   // (a plan's or a pair plan's longest chunk is shorter than Q whenever there is a second)
        HIPCHK(sc.ptr.ensure((size_t)B + 1));
        HIPCHK(sc.memb.ensure(n_memb));
        if (rq.groups) {
            HIPCHK(sc.mgrp.ensure(n_memb));
            HIPCHK(sc.grp.ensure((size_t)h->N));
        }
        if (rq.wide && !rq.pairs) HIPCHK(sc.wlist.ensure((size_t)chunk * width * (size_t)(rq.m + 1)));
        for (int i = 0; i < halves; ++i) {
            ChunkHalf &b = sc.half[i];
            HIPCHK(rq.Y ? b.Y.ensure((size_t)chunk * h->Dp, true) : b.qid.ensure((size_t)chunk, true));
            HIPCHK(b.dist.ensure(res * width, rq.dist_out));
            if (rq.pairs) {   // the tile table, and no row reduction
                HIPCHK(b.tile.ensure((size_t)rq.pairs->max_tiles, true));
                if (rq.wide) HIPCHK(b.wlist.ensure((size_t)chunk * (size_t)(rq.m + 1), rq.idx_out));
                if (rq.witness) {   // the records: the kernel writes them all, what the caller wants comes down
                    const size_t slots = (size_t)chunk * wslots;
                    if (!rq.wide) HIPCHK(b.wid.ensure(slots, rq.w_idx));   // (wide: the ids are the lists')
                    HIPCHK(b.wd.ensure(slots, rq.w_dist));
                    HIPCHK(b.walpha.ensure(slots, rq.w_alpha));
                }
                continue;
            }
            if (rq.nearest) {   // the ranked slots in place of the row reduction's three arrays
                const size_t slots = (size_t)chunk * (size_t)rq.near_k;
                HIPCHK(b.nbin.ensure(slots, rq.near_bin));
                HIPCHK(b.ndist.ensure(slots, rq.near_dist));
                continue;
            }
            HIPCHK(b.bin.ensure(res, true));
            HIPCHK(b.min.ensure(res, true));
            HIPCHK(b.margin.ensure(res, true));
            // a chunk holds at most one run per label
            if (rq.plan) HIPCHK(b.seg.ensure((size_t)std::min<int64_t>(B, chunk) + 1, true));
        }
        return CHB_OK;
    }
    // chb_bin_report: the context's tables, zeroed (dmin: +inf) on the stream
    int reset_report_tables()
    {
        if (!rq.plan) return CHB_OK;
        const size_t B = (size_t)rq.B, BB = B * B;
        HIPCHK(sc.rep_conf.ensure(BB));
        HIPCHK(sc.rep_unplaced.ensure(B));
        HIPCHK(sc.rep_cnt.ensure(BB));
        HIPCHK(sc.rep_min.ensure(BB));
        HIPCHK(sc.rep_sum.ensure(BB));
        HIPCHK(hipMemsetAsync(sc.rep_conf.p, 0, sizeof(long long) * BB, s));
        HIPCHK(hipMemsetAsync(sc.rep_unplaced.p, 0, sizeof(long long) * B, s));
        HIPCHK(hipMemsetAsync(sc.rep_cnt.p, 0, sizeof(long long) * BB, s));
        HIPCHK(hipMemsetAsync(sc.rep_sum.p, 0, sizeof(double) * BB, s));
        launch_fill_f64(sc.rep_min.p, std::numeric_limits<double>::infinity(), BB, s);
        return CHB_OK;
    }
    // what every chunk's launch shares, and the CSR it points at on its way up
    int kernel_args()
    {
        HIPCHK(hipMemcpyAsync(sc.ptr.p, sc.hptr.p, sizeof(int) * ((size_t)rq.B + 1), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sc.memb.p, sc.hmemb.p, sizeof(int) * n_memb, hipMemcpyHostToDevice, s));
        a.X = h->X.p; a.D = h->D; a.Dp = h->Dp; a.bin_ptr = sc.ptr.p; a.memb_id = sc.memb.p;
        a.B = (int)rq.B; a.m = rq.m; a.metric = h->metric;
        if (!rq.groups) return CHB_OK;
        HIPCHK(hipMemcpyAsync(sc.mgrp.p, sc.hmgrp.p, sizeof(int) * n_memb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sc.grp.p, sc.hgrp.p, sizeof(int) * (size_t)h->N, hipMemcpyHostToDevice, s));
        a.memb_grp = sc.mgrp.p; a.grp = sc.grp.p;
        return CHB_OK;
    }
    // The order of a step -- kernels of k, upload of k + 1, download of k, unpack of k - 1 -- keeps the copy stream from
    // queueing an upload behind a download that waits for kernels.
    hipError_t pipeline()
    {
        HIPTRY(upload(0));
        for (int64_t k = 0; k < n; ++k) {
            HIPTRY(launch(k));
            if (k + 1 < n) HIPTRY(upload(k + 1));
            if (!any_out) continue;
            HIPTRY(download(k));
            if (k > 0) HIPTRY(unpack(k - 1));
        }
        return any_out ? unpack(n - 1) : hipSuccess;
    }
    int run()
    {
        HIPCHK(hipSetDevice(h->dev));
        int rc;
        if ((rc = ensure_copy_stream()) || (rc = dense_groups()) || (rc = label_csr())) return rc;
        list_slots();
        if ((rc = size_buffers()) || (rc = reset_report_tables()) || (rc = kernel_args())) return rc;
        const hipError_t e = pipeline();
        if (e != hipSuccess) {   // nothing of this call stays in flight behind the error
            (void)hipStreamSynchronize(sc.copy);
            (void)hipStreamSynchronize(s);
            return fail(CHB_EHIP, hipGetErrorString(e));
        }
        return CHB_OK;
    }
    // ---- the pipeline's steps for chunk k
    hipError_t upload(int64_t k)
    {
        ChunkHalf &b = half(k);
        HIPTRY(hipEventSynchronize(b.up));                // the pinned half: its last upload (chunk k - 2) has left it
        HIPTRY(hipStreamWaitEvent(sc.copy, b.done, 0));   // the device half: the kernels of chunk k - 2 have read it
        HIPTRY(rq.pairs ? upload_pairs(b, k) : rq.Y ? upload_rows(b, k) : rq.plan ? upload_plan(b, k) : upload_indices(b, k));
        return hipEventRecord(b.up, sc.copy);
    }
    // packed rows (zero-padded to Dp) in kRecruitPiece pieces, so the copy of a piece runs under the packing of the next;
    // position r of the chunk is row y_of(r) of Y
    hipError_t upload_packed(ChunkHalf &b, int nq, const std::function<int64_t(int)> &y_of)
    {
        const int64_t D = h->D, Dp = h->Dp;
        for (int r0 = 0; r0 < nq; r0 += kRecruitPiece) {
            const int nr = std::min(kRecruitPiece, nq - r0);
            double *dst = b.Y.h.p + (size_t)r0 * Dp;
            for (int r = 0; r < nr; ++r, dst += Dp) {
                memcpy(dst, rq.Y + y_of(r0 + r) * D, sizeof(double) * D);
                for (int64_t j = D; j < Dp; ++j) dst[j] = 0.0;
            }
            HIPTRY(hipMemcpyAsync(b.Y.d.p + (size_t)r0 * Dp, b.Y.h.p + (size_t)r0 * Dp, sizeof(double) * (size_t)nr * Dp,
                                  hipMemcpyHostToDevice, sc.copy));
        }
        return hipSuccess;
    }
    hipError_t upload_rows(ChunkHalf &b, int64_t k)
    {
        const int64_t t0 = start(k);
        return upload_packed(b, rows(k), [t0](int r) { return t0 + r; });
    }
    // a pair plan's chunk: its tile table and, in position order, the pairs' sample indices or their rows of Y (a row
    // named by two pairs is packed twice)
    hipError_t upload_pairs(ChunkHalf &b, int64_t k)
    {
        const PairPlan &pl = *rq.pairs;
        const int nq = rows(k);
        const int64_t *ord = pl.ord.data() + start(k), t0 = pl.tcut[(size_t)k];
        b.ntile = (int)(pl.tcut[(size_t)k + 1] - t0);
        memcpy(b.tile.h.p, pl.tile.data() + t0, sizeof(int4) * (size_t)b.ntile);
        HIPTRY(b.tile.up((size_t)b.ntile, sc.copy));
        if (!audit) return upload_packed(b, nq, [&pl, ord](int r) { return pl.row[ord[r]]; });
        for (int i = 0; i < nq; ++i) b.qid.h.p[i] = (int)pl.row[ord[i]];
        return b.qid.up((size_t)nq, sc.copy);
    }
    // the chunk's sample indices and nothing else: the kernel reads the rows from the resident matrix
    hipError_t upload_indices(ChunkHalf &b, int64_t k)
    {
        const int nq = rows(k);
        const int64_t t0 = start(k);
        for (int i = 0; i < nq; ++i) b.qid.h.p[i] = (int)(rq.row_idx ? rq.row_idx[t0 + i] : t0 + i);
        return b.qid.up((size_t)nq, sc.copy);
    }
    // a plan's indices and the chunk's label runs, for bin_report_kernel behind the two audit kernels
    hipError_t upload_plan(ChunkHalf &b, int64_t k)
    {
        const std::vector<int64_t> &lab_ptr = rq.plan->lab_ptr;
        const int nq = rows(k);
        const int64_t t0 = start(k);
        memcpy(b.qid.h.p, rq.plan->ord.data() + t0, sizeof(int) * nq);
        int2 *sg = b.seg.h.p;   // {label, first position in the chunk} per run, closed by {-1, nq}
        b.nseg = 0;
        size_t l = (size_t)(std::upper_bound(lab_ptr.begin(), lab_ptr.end(), t0) - lab_ptr.begin()) - 1;
        for (; l < (size_t)rq.B && lab_ptr[l] < t0 + nq; ++l)
            if (lab_ptr[l + 1] > lab_ptr[l]) sg[b.nseg++] = make_int2((int)l, (int)(std::max(lab_ptr[l], t0) - t0));
        sg[b.nseg] = make_int2(-1, nq);
        HIPTRY(b.seg.up((size_t)b.nseg + 1, sc.copy));
        return b.qid.up((size_t)nq, sc.copy);
    }
    hipError_t launch(int64_t k)
    {
        ChunkHalf &b = half(k);
        const int nq = rows(k);
        HIPTRY(hipStreamWaitEvent(s, b.up, 0));
        if (any_out) HIPTRY(hipStreamWaitEvent(s, b.down, 0));   // (chunk k - 2 has been copied out of this half's results)
        a.Y = audit ? nullptr : b.Y.d.p; a.qid = audit ? b.qid.d.p : nullptr; a.dist = b.dist.d.p; a.nq = nq;
        // (with groups: the same launches, the leave-group-out instantiation of the kernel)
        if (rq.wide) {   // selection, solve and -- dense -- the row reduction; the work of both is the (row, bin) problems
            RecruitWideWitnessArgs wa{};   // (the launchers without witnesses take the part of it that is theirs)
            static_cast<RecruitGroupArgs &>(wa) = a;
            wa.tile = rq.pairs ? b.tile.d.p : nullptr; wa.ntile = rq.pairs ? b.ntile : 0;
            wa.list = rq.pairs ? b.wlist.d.p : sc.wlist.p;
            if (rq.witness) { wa.w_d = b.wd.d.p; wa.w_alpha = b.walpha.d.p; }   // (a pair chunk: the witness forms)
            const double work = (double)nq * (double)width;
            const bool wlist = rq.nm > 0;   // a wide list: (row, bin, entry) work behind one selection at its largest entry
            if (wlist && n_narrow > 0) {   // the entries up to 16: recruit_kernel's list launch, their slices in front
                RecruitGroupArgs na = a;
                na.m = m_narrow;
                na.tile = wa.tile; na.ntile = wa.ntile;   // (a pair chunk: the tile table's work items)
                Timed t(h, rq.pairs ? (audit ? "audit_pairs_multi" : "recruit_pairs_multi") : (audit ? "audit_multi" : "recruit_multi"),
                        work * (double)n_narrow);
                if (na.memb_grp) launch_recruit_grouped(na, s);
                else if (rq.pairs) launch_recruit_pairs(na, s);
                else launch_recruit(na, s);
            }
            {
                Timed t(h, wlist ? (rq.pairs ? (audit ? "audit_pairs_multi_wide_select" : "recruit_pairs_multi_wide_select")
                                             : (audit ? "audit_multi_wide_select" : "recruit_multi_wide_select"))
                        : rq.pairs ? (audit ? "audit_pairs_wide_select" : "recruit_pairs_wide_select")
                                   : (audit ? "audit_wide_select" : "recruit_wide_select"), work);
                if (rq.witness) launch_recruit_select_wide_witness(wa, s);
                else launch_recruit_select_wide(wa, s);
            }
            if (wlist) {
                // The entries above 16, their slices behind the narrow ones: one wavefront per (problem, entry), those up
                // to 32 by the 32-vertex kernel and those above by the 64-vertex one.  (One launch for both would solve an
                // entry of 24 in 66 KiB of LDS, two wavefronts per CU where the 32-vertex kernel's 17.5 KiB allow nine:
                // measured, it took longer than the single calls together.)
                RecruitWideListArgs la{};
                static_cast<RecruitWideArgs &>(la) = wa;
                la.lstride = rq.m + 1;
                if (rq.pairs) la.B = 1;   // (a pair chunk: nq problems, and a slice is the chunk's pairs)
                const int n32 = (int)(std::upper_bound(m_wide, m_wide + n_wide, (unsigned char)32) - m_wide);
                Timed t(h, rq.pairs ? (audit ? "audit_pairs_multi_wide_solve" : "recruit_pairs_multi_wide_solve")
                                    : (audit ? "audit_multi_wide_solve" : "recruit_multi_wide_solve"), work * (double)n_wide);
                for (int g0 = 0, g1 = n32; g0 < n_wide; g0 = g1, g1 = n_wide) {   // [0, n32), [n32, n_wide)
                    if (g1 == g0) continue;
                    la.m = m_wide[g1 - 1];
                    la.nw = g1 - g0;
                    memset(la.mw, 0, sizeof(la.mw));
                    memcpy(la.mw, m_wide + g0, (size_t)la.nw);
                    la.dist = b.dist.d.p + (size_t)(n_narrow + g0) * (size_t)nq * width;
                    launch_hull_wide_list(la, s);
                }
            } else {
                Timed t(h, rq.pairs ? (audit ? "audit_pairs_wide_solve" : "recruit_pairs_wide_solve")
                                    : (audit ? "audit_wide_solve" : "recruit_wide_solve"), work);
                if (rq.witness) launch_hull_wide_witness(wa, s);
                else launch_hull_wide(wa, s);
            }
            // (a nearest-bins call has no bin / min / margin buffers: the ranking below stands in the reduction's place)
            if (!rq.pairs && !rq.nearest) launch_recruit_reduce(b.dist.d.p, nq * ns, (int)rq.B, b.bin.d.p, b.min.d.p, b.margin.d.p, s);
        } else if (rq.pairs) {   // one launch: the tiles' kernel, no row reduction behind it
            a.tile = b.tile.d.p; a.ntile = b.ntile;
            // (a list, chb_*_pairs_multi without an entry above 16: a.mmask selects the kernel's list form)
            Timed t(h, a.mmask ? (audit ? "audit_pairs_multi" : "recruit_pairs_multi") : (audit ? "audit_pairs" : "recruit_pairs"),
                    (double)nq * (double)ns);
            if (rq.witness) {
                a.w_id = b.wid.d.p; a.w_d = b.wd.d.p; a.w_alpha = b.walpha.d.p;
                launch_recruit_witness(a, s);
            } else if (a.memb_grp) launch_recruit_grouped(a, s);
            else launch_recruit_pairs(a, s);
        } else {
            Timed t(h, a.mmask ? (audit ? "audit_multi" : "recruit_multi") : (audit ? "audit" : "recruit"),
                    (double)nq * (double)rq.B * (double)ns);
            if (a.memb_grp) launch_recruit_grouped(a, s);
            else launch_recruit(a, s);
            if (!rq.nearest) launch_recruit_reduce(b.dist.d.p, nq * ns, (int)rq.B, b.bin.d.p, b.min.d.p, b.margin.d.p, s);
        }
        if (rq.nearest) {   // the same table, ranked in place of the reduction (whose outputs nobody would read)
            Timed t(h, "nearest_bins", (double)nq * (double)rq.B);
            launch_nearest_bins(b.dist.d.p, nq, (int)rq.B, rq.near_k, b.nbin.d.p, b.ndist.d.p, s);
        }
        if (rq.plan) {
            const BinReportArgs r{b.dist.d.p, b.bin.d.p, b.seg.d.p, b.nseg, (int)rq.B,
                                  sc.rep_conf.p, sc.rep_unplaced.p, sc.rep_cnt.p, sc.rep_min.p, sc.rep_sum.p};
            Timed t(h, "bin_report", (double)nq * (double)rq.B);
            launch_bin_report(r, s);
        }
        HIPTRY(hipGetLastError());
        return hipEventRecord(b.done, s);
    }
    hipError_t download(int64_t k)
    {
        ChunkHalf &b = half(k);
        hipStream_t c = sc.copy;
        const size_t nr = (size_t)rows(k) * (size_t)ns;
        HIPTRY(hipStreamWaitEvent(c, b.done, 0));
        if (rq.dist_out) HIPTRY(b.dist.down(nr * width, c));
        if (rq.min_dist_out) HIPTRY(b.min.down(nr, c));
        if (rq.margin_out) HIPTRY(b.margin.down(nr, c));
        if (rq.bin_out) HIPTRY(b.bin.down(nr, c));
        // (pairs: nr positions; a wide witness call has no w_idx, its ids come down as idx_out's lists)
        if (rq.w_idx) HIPTRY(b.wid.down(nr * wslots, c));
        if (rq.w_dist) HIPTRY(b.wd.down(nr * wslots, c));
        if (rq.w_alpha) HIPTRY(b.walpha.down(nr * wslots, c));
        if (rq.idx_out) HIPTRY(b.wlist.down(nr * (size_t)(rq.m + 1), c));
        const size_t near = nr * (size_t)rq.near_k;   // (a nearest-bins call: nr rows)
        if (rq.near_bin) HIPTRY(b.nbin.down(near, c));
        if (rq.near_dist) HIPTRY(b.ndist.down(near, c));
        return hipEventRecord(b.down, c);
    }
    // (a list of m: ns slices of nq rows each, on the device in ascending order of m; slice slot[j] goes to out + j * Q + t0;
    // pairs: the position's double goes to the place of its pair in the caller's order, and so do the first m of the
    // wslots slots of its witness record)
    hipError_t unpack(int64_t k)
    {
        ChunkHalf &b = half(k);
        const int nq = rows(k);
        const int64_t t0 = start(k), B = rq.B;
        HIPTRY(hipEventSynchronize(b.down));
        if (rq.pairs) {
            const int64_t *ord = rq.pairs->ord.data() + t0;
            // (a list: slice slot[j] of the chunk's nq positions goes to the caller's slice j of Q pairs)
            for (int j = 0; j < ns && rq.dist_out; ++j) {
                const double *from = b.dist.h.p + (size_t)slot[j] * (size_t)nq;
                double *to = rq.dist_out + (size_t)j * (size_t)rq.Q;
                for (int i = 0; i < nq; ++i) to[ord[i]] = from[i];
            }
            const size_t m = (size_t)rq.m;
            for (int i = 0; i < nq && rq.idx_out; ++i)   // (the record's first int is the list's length; the ids are padded already)
                for (size_t v = 0; v < m; ++v) rq.idx_out[(size_t)ord[i] * m + v] = b.wlist.h.p[(size_t)i * (m + 1) + 1 + v];
            for (int i = 0; i < nq && rq.witness; ++i) {
                const size_t from = (size_t)i * wslots, to = (size_t)ord[i] * m;
                for (size_t v = 0; v < m && rq.w_idx; ++v) rq.w_idx[to + v] = b.wid.h.p[from + v];
                if (rq.w_dist) memcpy(rq.w_dist + to, b.wd.h.p + from, sizeof(double) * m);
                if (rq.w_alpha) memcpy(rq.w_alpha + to, b.walpha.h.p + from, sizeof(double) * m);
            }
            return hipSuccess;
        }
        if (rq.nearest) {   // near_k slots per row, in the caller's row order already
            const size_t near = (size_t)nq * (size_t)rq.near_k, to = (size_t)t0 * (size_t)rq.near_k;
            for (size_t i = 0; i < near && rq.near_bin; ++i) rq.near_bin[to + i] = b.nbin.h.p[i];
            if (rq.near_dist) memcpy(rq.near_dist + to, b.ndist.h.p, sizeof(double) * near);
            return hipSuccess;
        }
        for (int j = 0; j < ns; ++j) {
            const size_t from = (size_t)slot[j] * (size_t)nq;
            const int64_t to = (int64_t)j * rq.Q + t0;
            if (rq.dist_out) memcpy(rq.dist_out + to * B, b.dist.h.p + from * (size_t)B, sizeof(double) * (size_t)nq * (size_t)B);
            if (rq.min_dist_out) memcpy(rq.min_dist_out + to, b.min.h.p + from, sizeof(double) * nq);
            if (rq.margin_out) memcpy(rq.margin_out + to, b.margin.h.p + from, sizeof(double) * nq);
            if (rq.bin_out)
                for (int i = 0; i < nq; ++i) rq.bin_out[to + i] = b.bin.h.p[from + i];
        }
        return hipSuccess;
    }
};

// ---- the entry points: each makes its request (ScoreRequest::audit / ::recruit), sets what is its own by name and hands it
// to the body of its call shape -- score_rows, bin_report, score_pairs or score_nearest

// The wide calls: one entry point for every m.  A _wide symbol is its narrow twin's request with wide = m > kMaxM: two
// kernels per chunk (recruit_wide_kernels.hip) for 16 < m <= 64, and up to 16 neighbours the twin's call in everything --
// its result, its refusals and its name in their texts.  Returns the name the call goes by.
const char *wide_rule(ScoreRequest &rq, const char *wide_name, const char *narrow_name)
{
    rq.wide = rq.m > kMaxM;
    return rq.wide ? wide_name : narrow_name;
}

// the calls that return rows: the request goes through the checks and, unless Q == 0, through a ScoreRun
int score_rows(chb_ctx *h, const char *who, ScoreRequest &rq, const int64_t *D, bool list, int64_t *bin_out, double *dist_out,
               double *min_dist_out, double *margin_out)
{
    rq.bin_out = bin_out; rq.dist_out = dist_out; rq.min_dist_out = min_dist_out; rq.margin_out = margin_out;
    const int rc = score_check_args(h, who, rq, D, list, bin_out || dist_out ? nullptr : "bin_out and dist_out are both null");
    return rc != CHB_OK || rq.Q == 0 ? rc : ScoreRun{h, rq}.run();
}

// chb_bin_report and its grouped and wide forms behind the request
int bin_report(chb_ctx *h, const char *who, ScoreRequest &rq, int64_t *confusion, int64_t *unplaced, int64_t *dcnt,
               double *dmin, double *dsum, int64_t *n_skipped)
{
    const int64_t *labels = rq.labels, *row_idx = rq.row_idx, B = rq.B, Q = rq.Q;
    const bool any = confusion || unplaced || dcnt || dmin || dsum || n_skipped;
    int rc = score_check_args(h, who, rq, nullptr, false, any ? nullptr : "every output is null");
    if (rc != CHB_OK) return rc;
    const ReportOut out{confusion, unplaced, dcnt, dmin, dsum};
    ReportPlan plan;
    const int64_t Qv = plan.build(labels, B, row_idx, Q, rq.wide ? wide_chunk_rows(B, rq.m) : kRecruitChunk);
    if (n_skipped) *n_skipped = Q - Qv;
    if (Qv == 0) { plan.empty_tables(out); return CHB_OK; }
    rq.row_idx = nullptr; rq.plan = &plan; rq.Q = Qv;   // the plan's positions, already in label order
    rc = ScoreRun{h, rq}.run();
    return rc != CHB_OK ? rc : plan.copy_tables(h, out);
}

// a witness call's outputs: per pair the hull's members, their selection distances and their weights.  (Wide: the members
// are the selection list, so their ids come down as idx_out and w_idx stays null.)
void witness_outputs(ScoreRequest &rq, int64_t *nbr_idx, double *nbr_dist, double *alpha)
{
    rq.witness = true; rq.w_dist = nbr_dist; rq.w_alpha = alpha;
    if (rq.wide) rq.idx_out = nbr_idx;
    else rq.w_idx = nbr_idx;
}

// The pair calls, whole: rq.Q pairs (row, bin_idx), the rows resident (rq.row_idx, which is not "all rows" here: its range
// is checked like chb_audit_rows' list) or, in the recruit forms, rows row_of of the Y_rows rows of Y, D columns each.
// Behind score_check_args the recruit forms' own checks, then the bins' range, the plan and the run.
// list (chb_*_pairs_multi): the call takes ms / nm -- the list calls' checks in score_check_args, the number of rows of Y
// among its ranges -- and dist_out is [nm][P].
int score_pairs(chb_ctx *h, const char *who, ScoreRequest &rq, const int64_t *bin_idx, const int64_t *D = nullptr,
                int64_t Y_rows = 0, const int64_t *row_of = nullptr, bool list = false)
{
    const int64_t P = rq.Q, *row = D ? row_of : rq.row_idx;
    if (h && list && D && Y_rows < 0) return fail(CHB_EINVAL, "Q < 0");
    // null arguments: the lists, then dist_out -- which a witness call may leave out, but not with every witness output
    const char *missing = nullptr;
    if (P > 0 && rq.witness) {
        if (!row || !bin_idx) missing = D ? "row_of or bin_idx is null" : "row_idx or bin_idx is null";
        else if (!rq.w_idx && !rq.idx_out && !rq.w_dist && !rq.w_alpha)
            missing = "nbr_idx, nbr_dist and alpha are all null (the call without witnesses is the one to use)";
    } else if (P > 0 && (!row || !bin_idx || !rq.dist_out)) {
        missing = D ? "row_of, bin_idx or dist_out is null" : "row_idx, bin_idx or dist_out is null";
    }
    const int rc = score_check_args(h, who, rq, D, list, missing);
    if (rc != CHB_OK) return rc;
    if (D) {
        if (Y_rows < 0) return fail(CHB_EINVAL, "Q < 0");
        for (int64_t p = 0; p < P; ++p)
            if (row_of[p] < 0 || row_of[p] >= Y_rows) return fail(CHB_EINVAL, "row_of entry outside [0, Q)");
    }
    if (P == 0) return CHB_OK;
    for (int64_t p = 0; p < P; ++p)
        if (bin_idx[p] < 0 || bin_idx[p] >= rq.B) return fail(CHB_EINVAL, "bin_idx entry outside [0, B)");
    PairPlan plan;
    plan.build(row, bin_idx, P, rq.B);
    h->score.pair_tiles = (int64_t)plan.tile.size();
    rq.row_idx = nullptr; rq.pairs = &plan;
    return ScoreRun{h, rq}.run();
}

// The wide pair calls' idx_out: the selection lists with more than 16 neighbours; up to 16 the narrow witness call's
// nbr_idx -- and with it that call's rule for what may be null -- or, without idx_out, the plain pair call `plain`
const char *wide_pairs_rule(ScoreRequest &rq, int64_t *idx_out, const char *wide_name, const char *witness_name, const char *plain)
{
    const char *who = wide_rule(rq, wide_name, idx_out ? witness_name : plain);
    if (rq.wide) rq.idx_out = idx_out;
    else if (idx_out) witness_outputs(rq, idx_out, nullptr, nullptr);
    return who;
}

// the nearest-bins calls: the dense call's request with the ranked outputs in place of the reduced ones
int score_nearest(chb_ctx *h, const char *who, ScoreRequest &rq, const int64_t *D, int k, int64_t *near_bin, double *near_dist)
{
    rq.nearest = true; rq.near_k = k; rq.near_bin = near_bin; rq.near_dist = near_dist;
    const int rc = score_check_args(h, who, rq, D, false, near_bin || near_dist ? nullptr : "near_bin and near_dist are both null");
    return rc != CHB_OK || rq.Q == 0 ? rc : ScoreRun{h, rq}.run();
}

}  // namespace

int chb_recruit_rows(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q, int64_t D,
                     int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, m, Y, Q);
    return score_rows(h, "chb_recruit_rows", rq, &D, false, bin_out, dist_out, min_dist_out, margin_out);
}

int chb_audit_rows(chb_ctx *h, const int64_t *labels, int64_t B, int m, const int64_t *row_idx, int64_t Q,
                   int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, Q);
    return score_rows(h, "chb_audit_rows", rq, nullptr, false, bin_out, dist_out, min_dist_out, margin_out);
}

int chb_recruit_rows_multi(chb_ctx *h, const int64_t *labels, int64_t B, const int *ms, int nm, const double *Y, int64_t Q,
                           int64_t D, int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, 0, Y, Q);
    rq.ms = ms; rq.nm = nm;
    return score_rows(h, "chb_recruit_rows_multi", rq, &D, true, bin_out, dist_out, min_dist_out, margin_out);
}

int chb_audit_rows_multi(chb_ctx *h, const int64_t *labels, int64_t B, const int *ms, int nm, const int64_t *row_idx,
                         int64_t Q, int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, 0, row_idx, Q);
    rq.ms = ms; rq.nm = nm;
    return score_rows(h, "chb_audit_rows_multi", rq, nullptr, true, bin_out, dist_out, min_dist_out, margin_out);
}

int chb_audit_rows_grouped(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, const int64_t *row_idx,
                           int64_t Q, int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, Q);
    rq.grouped = true; rq.groups = groups;
    return score_rows(h, "chb_audit_rows_grouped", rq, nullptr, false, bin_out, dist_out, min_dist_out, margin_out);
}

int chb_audit_rows_multi_grouped(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, const int *ms, int nm,
                                 const int64_t *row_idx, int64_t Q, int64_t *bin_out, double *dist_out, double *min_dist_out,
                                 double *margin_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, 0, row_idx, Q);
    rq.ms = ms; rq.nm = nm; rq.grouped = true; rq.groups = groups;
    return score_rows(h, "chb_audit_rows_multi_grouped", rq, nullptr, true, bin_out, dist_out, min_dist_out, margin_out);
}

int chb_bin_report(chb_ctx *h, const int64_t *labels, int64_t B, int m, const int64_t *row_idx, int64_t Q,
                   int64_t *confusion, int64_t *unplaced, int64_t *dcnt, double *dmin, double *dsum, int64_t *n_skipped)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, Q);
    return bin_report(h, "chb_bin_report", rq, confusion, unplaced, dcnt, dmin, dsum, n_skipped);
}

int chb_bin_report_grouped(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, const int64_t *row_idx,
                           int64_t Q, int64_t *confusion, int64_t *unplaced, int64_t *dcnt, double *dmin, double *dsum,
                           int64_t *n_skipped)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, Q);
    rq.grouped = true; rq.groups = groups;
    return bin_report(h, "chb_bin_report_grouped", rq, confusion, unplaced, dcnt, dmin, dsum, n_skipped);
}

int chb_audit_pairs(chb_ctx *h, const int64_t *labels, int64_t B, int m, const int64_t *row_idx, const int64_t *bin_idx,
                    int64_t P, double *dist_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, P);
    rq.dist_out = dist_out;
    return score_pairs(h, "chb_audit_pairs", rq, bin_idx);
}

int chb_audit_pairs_grouped(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, const int64_t *row_idx,
                            const int64_t *bin_idx, int64_t P, double *dist_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, P);
    rq.dist_out = dist_out; rq.grouped = true; rq.groups = groups;
    return score_pairs(h, "chb_audit_pairs_grouped", rq, bin_idx);
}

int chb_recruit_pairs(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q, int64_t D,
                      const int64_t *row_of, const int64_t *bin_idx, int64_t P, double *dist_out)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, m, Y, P);
    rq.dist_out = dist_out;
    return score_pairs(h, "chb_recruit_pairs", rq, bin_idx, &D, Q, row_of);
}

int chb_audit_pairs_witness(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, const int64_t *row_idx,
                            const int64_t *bin_idx, int64_t P, double *dist_out, int64_t *nbr_idx, double *nbr_dist,
                            double *alpha)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, P);
    rq.dist_out = dist_out; rq.groups = groups;   // (null: leave-one-out, the ungrouped kernel)
    witness_outputs(rq, nbr_idx, nbr_dist, alpha);
    return score_pairs(h, "chb_audit_pairs_witness", rq, bin_idx);
}

int chb_recruit_pairs_witness(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q, int64_t D,
                              const int64_t *row_of, const int64_t *bin_idx, int64_t P, double *dist_out, int64_t *nbr_idx,
                              double *nbr_dist, double *alpha)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, m, Y, P);
    rq.dist_out = dist_out;
    witness_outputs(rq, nbr_idx, nbr_dist, alpha);
    return score_pairs(h, "chb_recruit_pairs_witness", rq, bin_idx, &D, Q, row_of);
}

int chb_audit_rows_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, const int64_t *row_idx,
                        int64_t Q, int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, Q);
    rq.groups = groups;   // (null: leave-one-out, the ungrouped kernel)
    const char *who = wide_rule(rq, "chb_audit_rows_wide", groups ? "chb_audit_rows_grouped" : "chb_audit_rows");
    return score_rows(h, who, rq, nullptr, false, bin_out, dist_out, min_dist_out, margin_out);
}

int chb_recruit_rows_wide(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q, int64_t D,
                          int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, m, Y, Q);
    const char *who = wide_rule(rq, "chb_recruit_rows_wide", "chb_recruit_rows");
    return score_rows(h, who, rq, &D, false, bin_out, dist_out, min_dist_out, margin_out);
}

namespace {
// wide_rule for a list: wide only with an entry above 16 in a list the narrow list calls would read that far -- every
// other list, those they refuse as a bad argument before that (ms null, nm outside 1 .. 16) among them, is the narrow
// twin's request in everything.  Returns the name the call goes by.
const char *wide_list_rule(ScoreRequest &rq, const char *wide_name, const char *narrow_name)
{
    rq.wide = rq.ms && rq.nm >= 1 && rq.nm <= kMaxM && *std::max_element(rq.ms, rq.ms + rq.nm) > kMaxM;
    return rq.wide ? wide_name : narrow_name;
}
}  // namespace

int chb_audit_rows_multi_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, const int *ms, int nm,
                              const int64_t *row_idx, int64_t Q, int64_t *bin_out, double *dist_out, double *min_dist_out,
                              double *margin_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, 0, row_idx, Q);
    rq.ms = ms; rq.nm = nm;
    rq.groups = groups;   // (null: leave-one-out, the ungrouped kernels)
    const char *who = wide_list_rule(rq, "chb_audit_rows_multi_wide", groups ? "chb_audit_rows_multi_grouped" : "chb_audit_rows_multi");
    return score_rows(h, who, rq, nullptr, true, bin_out, dist_out, min_dist_out, margin_out);
}

int chb_recruit_rows_multi_wide(chb_ctx *h, const int64_t *labels, int64_t B, const int *ms, int nm, const double *Y, int64_t Q,
                                int64_t D, int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, 0, Y, Q);
    rq.ms = ms; rq.nm = nm;
    const char *who = wide_list_rule(rq, "chb_recruit_rows_multi_wide", "chb_recruit_rows_multi");
    return score_rows(h, who, rq, &D, true, bin_out, dist_out, min_dist_out, margin_out);
}

// The pair calls for a list: one symbol for every entry up to 64 and one name in the texts -- there is no narrow twin to
// forward to.  wide_list_rule only says whether an entry above 16 brings the wide kernels in.
int chb_audit_pairs_multi(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, const int *ms, int nm,
                          const int64_t *row_idx, const int64_t *bin_idx, int64_t P, double *dist_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, 0, row_idx, P);
    rq.ms = ms; rq.nm = nm;
    rq.dist_out = dist_out; rq.groups = groups;   // (null: leave-one-out, the ungrouped kernels)
    const char *who = wide_list_rule(rq, "chb_audit_pairs_multi", "chb_audit_pairs_multi");
    return score_pairs(h, who, rq, bin_idx, nullptr, 0, nullptr, true);
}

int chb_recruit_pairs_multi(chb_ctx *h, const int64_t *labels, int64_t B, const int *ms, int nm, const double *Y, int64_t Q,
                            int64_t D, const int64_t *row_of, const int64_t *bin_idx, int64_t P, double *dist_out)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, 0, Y, P);
    rq.ms = ms; rq.nm = nm;
    rq.dist_out = dist_out;
    const char *who = wide_list_rule(rq, "chb_recruit_pairs_multi", "chb_recruit_pairs_multi");
    return score_pairs(h, who, rq, bin_idx, &D, Q, row_of, true);
}

int chb_audit_pairs_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, const int64_t *row_idx,
                         const int64_t *bin_idx, int64_t P, double *dist_out, int64_t *idx_out)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, P);
    rq.dist_out = dist_out; rq.groups = groups;
    const char *who = wide_pairs_rule(rq, idx_out, "chb_audit_pairs_wide", "chb_audit_pairs_witness",
                                      groups ? "chb_audit_pairs_grouped" : "chb_audit_pairs");
    return score_pairs(h, who, rq, bin_idx);
}

int chb_recruit_pairs_wide(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q, int64_t D,
                           const int64_t *row_of, const int64_t *bin_idx, int64_t P, double *dist_out, int64_t *idx_out)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, m, Y, P);
    rq.dist_out = dist_out;
    const char *who = wide_pairs_rule(rq, idx_out, "chb_recruit_pairs_wide", "chb_recruit_pairs_witness", "chb_recruit_pairs");
    return score_pairs(h, who, rq, bin_idx, &D, Q, row_of);
}

int chb_audit_pairs_witness_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m,
                                 const int64_t *row_idx, const int64_t *bin_idx, int64_t P, double *dist_out, int64_t *nbr_idx,
                                 double *nbr_dist, double *alpha)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, P);
    rq.dist_out = dist_out; rq.groups = groups;
    const char *who = wide_rule(rq, "chb_audit_pairs_witness_wide", "chb_audit_pairs_witness");
    witness_outputs(rq, nbr_idx, nbr_dist, alpha);
    return score_pairs(h, who, rq, bin_idx);
}

int chb_recruit_pairs_witness_wide(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q, int64_t D,
                                   const int64_t *row_of, const int64_t *bin_idx, int64_t P, double *dist_out,
                                   int64_t *nbr_idx, double *nbr_dist, double *alpha)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, m, Y, P);
    rq.dist_out = dist_out;
    const char *who = wide_rule(rq, "chb_recruit_pairs_witness_wide", "chb_recruit_pairs_witness");
    witness_outputs(rq, nbr_idx, nbr_dist, alpha);
    return score_pairs(h, who, rq, bin_idx, &D, Q, row_of);
}

int chb_bin_report_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, const int64_t *row_idx,
                        int64_t Q, int64_t *confusion, int64_t *unplaced, int64_t *dcnt, double *dmin, double *dsum,
                        int64_t *n_skipped)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, Q);
    rq.groups = groups;   // (null: leave-one-out, the ungrouped kernel)
    const char *who = wide_rule(rq, "chb_bin_report_wide", groups ? "chb_bin_report_grouped" : "chb_bin_report");
    return bin_report(h, who, rq, confusion, unplaced, dcnt, dmin, dsum, n_skipped);
}

int chb_audit_rows_nearest(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, int k,
                           const int64_t *row_idx, int64_t Q, int64_t *near_bin, double *near_dist)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, Q);
    rq.groups = groups;   // (null: leave-one-out, the ungrouped kernel)
    return score_nearest(h, "chb_audit_rows_nearest", rq, nullptr, k, near_bin, near_dist);
}

int chb_recruit_rows_nearest(chb_ctx *h, const int64_t *labels, int64_t B, int m, int k, const double *Y, int64_t Q, int64_t D,
                             int64_t *near_bin, double *near_dist)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, m, Y, Q);
    return score_nearest(h, "chb_recruit_rows_nearest", rq, &D, k, near_bin, near_dist);
}

int chb_audit_rows_nearest_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m, int k,
                                const int64_t *row_idx, int64_t Q, int64_t *near_bin, double *near_dist)
{
    ScoreRequest rq = ScoreRequest::audit(labels, B, m, row_idx, Q);
    rq.groups = groups;
    const char *who = wide_rule(rq, "chb_audit_rows_nearest_wide", "chb_audit_rows_nearest");
    return score_nearest(h, who, rq, nullptr, k, near_bin, near_dist);
}

int chb_recruit_rows_nearest_wide(chb_ctx *h, const int64_t *labels, int64_t B, int m, int k, const double *Y, int64_t Q,
                                  int64_t D, int64_t *near_bin, double *near_dist)
{
    ScoreRequest rq = ScoreRequest::recruit(labels, B, m, Y, Q);
    const char *who = wide_rule(rq, "chb_recruit_rows_nearest_wide", "chb_recruit_rows_nearest");
    return score_nearest(h, who, rq, &D, k, near_bin, near_dist);
}

int chb_set_metric(chb_ctx *h, int metric)
{
    if (!h) return fail(CHB_EINVAL, "null context");
    if (metric != CHB_METRIC_CONVEX && metric != CHB_METRIC_AFFINE) return fail(CHB_EINVAL, "unknown metric");
    h->metric = metric;
    return CHB_OK;
}

int chb_comm_unique_id(char *out128)
{
    if (!out128) return fail(CHB_EINVAL, "null argument");
    if (!rccl()) return fail(CHB_EUNSUPPORTED, "librccl could not be loaded");
    ncclUniqueId id;
    NCCLCHK(rccl()->GetUniqueId(&id));
    memcpy(out128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return CHB_OK;
}

int chb_comm_init(chb_ctx *h, const char *id128, int rank, int world)
{
    if (!h || !id128) return fail(CHB_EINVAL, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(CHB_EINVAL, "bad rank/world");
    if (!rccl()) return fail(CHB_EUNSUPPORTED, "librccl could not be loaded");
    HIPCHK(hipSetDevice(h->dev));
    if (h->xchg.comm) { (void)rccl()->CommDestroy(h->xchg.comm); h->xchg.comm = nullptr; }
    ncclUniqueId id;
    memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    NCCLCHK(rccl()->CommInitRank(&h->xchg.comm, world, id, rank));
    h->rank = rank; h->world = world;
    h->Kcap = 0;
    return CHB_OK;
}

int chb_comm_init_hook(chb_ctx *h, int rank, int world, chb_allgather_fn fn, void *user)
{
    if (!h || !fn) return fail(CHB_EINVAL, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(CHB_EINVAL, "bad rank/world");
    HIPCHK(hipSetDevice(h->dev));
    if (h->xchg.comm && rccl()) { (void)rccl()->CommDestroy(h->xchg.comm); h->xchg.comm = nullptr; }
    h->xchg.hook = fn; h->xchg.hook_user = user;
    h->rank = rank; h->world = world;
    h->Kcap = 0;
    return CHB_OK;
}

int chb_comm_destroy(chb_ctx *h)
{
    if (!h) return CHB_OK;
    h->xchg.hook = nullptr; h->xchg.hook_user = nullptr;
    if (h->xchg.comm && rccl()) {
        (void)hipSetDevice(h->dev);
        (void)hipStreamSynchronize(h->stream);
        (void)rccl()->CommDestroy(h->xchg.comm);
    }
    h->xchg.comm = nullptr; h->rank = 0; h->world = 1;
    return CHB_OK;
}

int chb_profile_enable(chb_ctx *h, int on)
{
    if (!h) return fail(CHB_EINVAL, "null context");
    drain_profile(h);
    h->prof.level = on < 0 ? 0 : (on > 2 ? 1 : on);
    return CHB_OK;
}

int chb_profile_reset(chb_ctx *h)
{
    if (!h) return fail(CHB_EINVAL, "null context");
    drain_profile(h);
    h->prof.acc.clear();
    return CHB_OK;
}

int chb_profile_get(chb_ctx *h, const char *kernel, double *total_ms, int64_t *launches, double *work_units)
{
    if (!h || !kernel) return fail(CHB_EINVAL, "null argument");
    (void)hipStreamSynchronize(h->stream);
    drain_profile(h);
    ProfEntry e;
    auto it = h->prof.acc.find(kernel);
    if (it != h->prof.acc.end()) e = it->second;
    if (total_ms) *total_ms = e.ms;
    if (launches) *launches = e.launches;
    if (work_units) *work_units = e.work;
    return CHB_OK;
}

// one device int, brought home on the context's stream (p == nullptr: 0)
static int read_device_int(chb_ctx *h, const int *p, int64_t *out)
{
    int v = 0;
    if (p) {
        HIPCHK(hipMemcpyAsync(&v, p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    *out = v;
    return CHB_OK;
}

// the base shortlists' lengths of the last batch, bin by bin (none without the shortlist stage or before the first batch)
static int last_batch_cand_cnt(chb_ctx *h, std::vector<int> *cnt)
{
    if (!h->cand_cnt.p || h->batch.K <= 0) return CHB_OK;
    std::vector<int> v((size_t)h->Kcap * h->B);
    HIPCHK(hipMemcpyAsync(v.data(), h->cand_cnt.p, sizeof(int) * v.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < h->B; ++c) cnt->insert(cnt->end(), v.begin() + (size_t)c * h->Kcap, v.begin() + (size_t)c * h->Kcap + h->batch.K);
    return CHB_OK;
}

// the last fit's threshold pools, as it left them, against what the shortlist kernel relies on (launch_pool_check): slots
// and pools in breach.  For the tests, while no batch is open; 0 where the context has no pools or the fit dropped them
static int pool_bad_slots(chb_ctx *h, int64_t *out)
{
    *out = 0;
    if (!(h->pool.valid || h->pool.kept) || !h->pool.Z.p || !h->labels.p || !h->qn.p || !h->Zs.p) return CHB_OK;
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(h->pool.bad.ensure(1));
    HIPCHK(hipMemsetAsync(h->pool.bad.p, 0, sizeof(int), h->stream));
    launch_pool_check(h->pool.view(), h->Zs.p, h->qn.p, h->labels.p, (int)h->N, h->Dz, h->B, h->pool.bad.p, h->stream);
    HIPCHK(hipGetLastError());
    return read_device_int(h, h->pool.bad.p, out);
}

// the hull kernels' 16-lane exchanges against the shuffles they replace (launch_lane_exchange_check): values that differ
static int lane_exchange_mismatches(chb_ctx *h, int64_t *out)
{
    *out = 0;
    HIPCHK(hipSetDevice(h->dev));
    DevBuf<int> bad;
    HIPCHK(bad.ensure(1));
    HIPCHK(hipMemsetAsync(bad.p, 0, sizeof(int), h->stream));
    launch_lane_exchange_check(bad.p, h->stream);
    HIPCHK(hipGetLastError());
    return read_device_int(h, bad.p, out);   // (synchronises the stream before the buffer goes)
}

// the counters the host keeps
#define CTR(name, expr) {name, [](const chb_ctx *h) -> int64_t { return expr; }}
static const struct { const char *name; int64_t (*get)(const chb_ctx *); } kHostCounters[] = {
    CTR("lookahead_batches", h->stats_lookahead), CTR("lookahead_failed", h->stats_lookahead_failed), CTR("exchanges", h->xchg.seq),
    CTR("pack_incremental_batches", h->pp.stat_batches), CTR("pack_builds", h->pp.stat_builds),
    CTR("pool_batches", h->pool.stat_batches), CTR("pool_state", h->pool.state), CTR("pool_candidates", h->pool.cand),
    CTR("pool_pairs", h->pool.pairs), CTR("fused_enabled", h->fused ? 1 : 0), CTR("segment_batches", h->seg.stat_batches),
    CTR("batch_size", h->last_batch),   // (speculative batch size of the last fit)
    // tile skipping of the last fit: its verdict (0 undecided, 1 kept on, -1 turned off) and the sampled wave-tile counters
    CTR("tile_skip_state", h->seat.state), CTR("tile_skipped", h->seat.skipped), CTR("tile_seen", h->seat.seen),
    CTR("tile_unloaded", h->seat.unloaded), CTR("last_batch_k", h->batch.K),
    CTR("recruit_chunk", kRecruitChunk),   // rows per launch of chb_recruit_rows
    CTR("recruit_multi_rows", h->score.multi_rows),   // ... of the last chb_audit_rows_multi / chb_recruit_rows_multi
    CTR("pair_tiles", h->score.pair_tiles),   // work items of the last chb_audit_pairs / chb_recruit_pairs
    CTR("recruit_wide_rows", h->score.wide_rows),   // rows per launch of the last chb_*_wide call with more than 16 neighbours (a list's: its largest entry)
    // chb_kmer_profiles / chb_set_samples_from_sequences: a chunk's limits, the chunks of the last call
    CTR("kmer_chunk_bytes", kKmerChunkBytes), CTR("kmer_chunk_rows", kKmerChunkRows), CTR("kmer_chunks", h->kmer_chunks),
    CTR("prefilter_enabled", (h->sw.use_prefilter && h->shadow_ok) ? 1 : 0),
};
#undef CTR

int chb_counter(chb_ctx *h, const char *name, int64_t *out)
{
    if (!h || !name || !out) return fail(CHB_EINVAL, "null argument");
    *out = 0;
    if (!strcmp(name, "prefilter_overflow")) return read_device_int(h, h->overflow_total_valid ? h->overflow.p : nullptr, out);
    // pairs of the last fit that broke the shortlist stage's contract (0, or the fit failed)
    if (!strcmp(name, "shortlist_short")) return read_device_int(h, h->short_cnt.p, out);
    if (!strcmp(name, "pool_bad_slots")) return pool_bad_slots(h, out);
    if (!strcmp(name, "lane_exchange_mismatches")) return lane_exchange_mismatches(h, out);
    // regions of the persistent pack that ran full and moved in the last fit (pack_state_fix_kernel)
    if (!strcmp(name, "pack_region_moves")) return read_device_int(h, h->pp.ctl.p ? h->pp.ctl.p + 3 : nullptr, out);
    // pairs the fused kernel left to the exact path
    if (!strcmp(name, "slow_pairs_last_round")) return read_device_int(h, h->fused ? h->n_slow.p : nullptr, out);
    // the m <= 5 fused kernel's trim in the last fit: pairs it swept, their candidates before and after
    for (int i = 0; i < 3; ++i)
        if (!strcmp(name, i == 0 ? "fused_trim_pairs" : i == 1 ? "fused_trim_in" : "fused_trim_kept")) {
            unsigned long long v = 0;
            if (h->fused && h->trim_ctr.p) {
                HIPCHK(hipMemcpyAsync(&v, h->trim_ctr.p + i, sizeof(v), hipMemcpyDeviceToHost, h->stream));
                HIPCHK(hipStreamSynchronize(h->stream));
            }
            *out = (int64_t)v;
            return CHB_OK;
        }
    // "shortlist_le<N>_last_batch": pairs of the last batch with <= N candidates
    const bool sum = !strcmp(name, "shortlist_sum_last_batch"), le = !strncmp(name, "shortlist_le", 12);
    if (sum || le || !strcmp(name, "shortlist_max_last_batch")) {
        std::vector<int> cnt;
        { const int rc = last_batch_cand_cnt(h, &cnt); if (rc) return rc; }
        const int lim = le ? atoi(name + 12) : 0;
        for (const int x : cnt)
            *out = le ? *out + (x <= lim) : sum ? *out + x : std::max<int64_t>(*out, x);
        return CHB_OK;
    }
    for (const auto &c : kHostCounters)
        if (!strcmp(name, c.name)) { *out = c.get(h); return CHB_OK; }
    return fail(CHB_EINVAL, "unknown counter");
}

int chb_fit_stats(chb_ctx *h, int64_t *out4)
{
    if (!h || !out4) return fail(CHB_EINVAL, "null argument");
    for (int i = 0; i < 4; ++i) out4[i] = h->stats[i];
    return CHB_OK;
}

}  // extern "C"
