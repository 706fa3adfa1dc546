/*
 * chbin_hip.h -- C ABI of libchbin_hip.so, the MI355X (gfx950) implementation of CH-Bin's
 * convex-hull binning hot path (ch_bin/core/clustering, AlgoDistanceMetric=convex).
 *
 * The reference (kdsuneraavinash/CH-Bin) is pure Python and has no FFI of its own; its seams are
 * plain Python functions.  Each entry point below names the reference function it replaces
 * (file:line into the reference tree).  The Python host side in ch-bin_amd/ binds these with
 * ctypes and re-exposes the reference's own signatures; INTEGRATION.md shows the stub a CH-Bin
 * maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative CHB_E* code on failure; chb_last_error()
 *     returns a thread-local human-readable message.  No exceptions cross the ABI.
 *   - pointers are caller-owned HOST pointers unless the name says `_device`; C-contiguous;
 *     nothing is retained after return (chb_set_samples_device copies its matrix as well, see below).
 *   - labels / indices are int64 at the ABI (numpy's default, what pandas hands the reference:
 *     cli/clustering.py:52); -1 = unassigned.  Features are float64 (cli/clustering.py:53).
 *   - calls are blocking; a context is not thread-safe (the reference caller is single-threaded).
 *   - there is NO CPU fallback: without a gfx950 device every compute call fails with
 *     CHB_ENODEVICE.
 *   - environment switches read once by chb_create (none is a tuning knob, none touches an error bound: each
 *     selects a slower, independently written formulation of the same exact result, for A/B tests):
 *       CHB_PREFILTER=0     brute-force fp64 selection instead of the fp16 shortlist stage
 *       CHB_FUSED=0         list-based path (exact rescoring + hull kernel) instead of the fused kernels
 *       CHB_FUSED_PTR64=1   64-bit row pointers in the m <= 5 fused kernel (what a matrix >= 4 GiB gets)
 *       CHB_SPECULATE=0     no look-ahead across batches in chb_fit_cluster
 *       CHB_FORCE_GATHER=1  exchange path of the sharded loop even with one rank
 *       CHB_SEGMENTS=0      bins far larger than the rest are never cut into segments for the shortlist stage
 *       CHB_FUSED_STRIPE=0  position-major work order in the fused kernels (default: striped over the XCDs by bin)
 *       CHB_FUSED_TRIM=0    the m <= 5 fused kernel gathers every candidate of a shortlist of more than 7 (default: such a
 *                           shortlist of up to 32 is first cut down by fp16 bounds from the samples' global shadow rows)
 *       CHB_PACK_INCR=0     CSR and member pack of the shortlist stage rebuilt from the labels at every batch start (default:
 *                           kept across the batches of a fit and updated by each commit, where tiles are not skipped)
 *       CHB_POOL_TAU=0      the base shortlist launch always streams a bin twice (threshold sweep + admission sweep); default:
 *                           the threshold comes from a per-(bin, home bin) pool tile where one exists, and the bin is streamed once
 *                           (fits of m <= 8 neighbours, rows of up to 157 columns and at least 512 contigs per bin on average;
 *                           CHB_POOL_TAU=2: whatever the fit's size)
 *       CHB_TILE_SKIP=0     the shortlist stage never skips member tiles (default: on for fits whose first batches
 *                           show that tiles can be skipped -- data with several coverage columns)
 */
#ifndef CHBIN_HIP_H
#define CHBIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHB_OK 0
#define CHB_EINVAL (-1)    /* bad argument */
#define CHB_ENODEVICE (-2) /* no usable HIP device */
#define CHB_EHIP (-3)      /* a HIP runtime call failed */
#define CHB_ESTATE (-4)    /* call sequence violated (e.g. no samples set) */
#define CHB_EUNSUPPORTED (-5)

/* AlgoNumNeighbors supported (default.ini:16 -> 5, function default 15: algorithm.py:17).  The tuned kernels
 * cover 1..16; 17..64 run on plain one-wavefront-per-problem kernels (much slower, same results). */
#define CHB_MAX_NEIGHBORS 64

typedef struct chb_ctx chb_ctx;

const char *chb_last_error(void);
int chb_version(void);
/* number of visible HIP devices (0 when there is none); never fails */
int chb_device_count(void);

/* one context per process per GPU */
int chb_create(int device_id, chb_ctx **out);
int chb_destroy(chb_ctx *h);

/* hull_distance.py:90-108 calculate_distance's metric dispatch (AlgoDistanceMetric): selects what
 * every later hull-distance evaluation of this context computes (chb_fit_cluster,
 * chb_hull_distance_*).  CONVEX = distance to the convex hull ("convex", default.ini:18);
 * AFFINE = distance to the affine hull ("affine" :69-87 and "affine-qp" :38-66, the same quantity).
 * The nearest-member selection is identical for both. */
#define CHB_METRIC_CONVEX 0
#define CHB_METRIC_AFFINE 1
int chb_set_metric(chb_ctx *h, int metric);

/* Feature matrix `samples` of fit_cluster (algorithm.py:13): copied to HBM once and kept resident. */
int chb_set_samples(chb_ctx *h, const double *X, int64_t N, int64_t D);
/* same, from a device buffer (e.g. a torch tensor's data_ptr): copied device-to-device into the context's own resident
 * matrix, nothing is borrowed -- the caller may overwrite or free X_device once the call has returned.  The copy runs on
 * the context's own stream, which knows nothing of the caller's: the caller's writes to X_device must be complete (its
 * stream or device synchronised) before the call. */
int chb_set_samples_device(chb_ctx *h, const double *X_device, int64_t N, int64_t D);

/* distance_matrix.py:33-44 create_in_mem_distance_matrix / :12-30 create_distance_matrix:
 * rows [row_begin,row_end) of the N x N Euclidean matrix, bit-identical to scipy cdist
 * (sqrt of the k-sequential, unfused sum of squared differences).  out: (row_end-row_begin) x N. */
int chb_pairwise_distance(chb_ctx *h, int64_t row_begin, int64_t row_end, double *out);

/* distance_matrix.py:47-62 find_nearest_from_cluster, batched over queries and ALL bins:
 * for query contig query_idx[q] and bin c, the (up to) m members of bin c nearest to the query,
 * ordered by (distance, index); the query itself is never a member (algorithm.py:50).
 * nbr_idx: Q*B*m (-1 padded), nbr_dist: Q*B*m (+inf padded, may be NULL), nbr_cnt: Q*B. */
int chb_topm_per_bin(chb_ctx *h, const int64_t *labels, int64_t B, int m, const int64_t *query_idx,
                     int64_t Q, int64_t *nbr_idx, double *nbr_dist, int32_t *nbr_cnt);

/* Hull distance of NEW rows (not samples) to every bin of a frozen labelling: recruiting contigs that were not part of
 * the fit (the ones cli/features.py:60-64 drops under ContigLengthFilterBp, or a later assembly's) into finished bins.
 * For row q and bin c: among {p : labels[p] == c} the (up to) m members nearest to Y[q] by
 * (distance, index), distance = sqrt of the k-sequential unfused sum of squared differences (the
 * arithmetic of chb_pairwise_distance); dist_out[q*B + c] = distance from Y[q] to their hull under the
 * context's metric (chb_set_metric); +inf for a bin without members.  Nothing is excluded: a row equal
 * to a sample has that sample as a candidate (distance 0).
 * bin_out[q] = the bin the reference's strict-'>' scan (algorithm.py:57) picks over dist_out's row: lowest
 * index among equal minima, -1 when every entry is +inf.  min_dist_out / margin_out as in
 * chb_fit_cluster_ex (margin +inf without a finite runner-up, never inf - inf).
 * labels[N] outside [0, B) count as unassigned (as chb_topm_per_bin).  dist_out, min_dist_out, margin_out
 * may each be NULL; bin_out may be NULL if dist_out is not.  Q = 0 is a no-op.
 *   - limits: m <= 16 and B <= 8192, CHB_EUNSUPPORTED beyond (the plain kernels for up to CHB_MAX_NEIGHBORS do not serve
 *     this call); D must be the resident samples' D (CHB_EINVAL);
 *   - the call reads the resident matrix and `labels` and nothing else: it uses no state of a fit and leaves every counter,
 *     memo and switch of the context as it found it.  While a stepwise fit is open (chb_fit_begin, until the next
 *     chb_set_samples* / chb_fit_cluster* / chb_topm_per_bin) it is refused with CHB_ESTATE and the fit stays usable;
 *   - Y is uploaded and scored in chunks of 16384 rows (chb_counter "recruit_chunk"): the kernels on the context's stream,
 *     the copies of the neighbouring chunks under them on a second stream of the context, through pinned staging buffers
 *     the context keeps (two chunks of rows and of results); Y and the outputs may be ordinary pageable memory;
 *   - one GPU: with a communicator (world > 1) each rank scores the rows it is given, there is no collective. */
int chb_recruit_rows(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q,
                     int64_t D, int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);

/* Audit of a finished labelling: leave-one-out hull distance of RESIDENT rows to every bin of a frozen labelling -- the
 * step of algorithm.py:49-58 for sample r = row_idx[q] against `labels`, with nothing moved.
 * For position q, sample r and bin c: among {p : labels[p] == c, p != r} the (up to) m members nearest to X[r] by
 * (distance, index), distance = sqrt of the k-sequential unfused sum of squared differences (the arithmetic of
 * chb_pairwise_distance, bit for bit); dist_out[q*B + c] = distance from X[r] to their hull under the context's metric
 * (chb_set_metric); +inf for a bin without another member.
 * Only sample r itself is withheld (as chb_topm_per_bin, algorithm.py:50): another sample with the same coordinates
 * stays a candidate, at distance 0.  labels[r] may be anything -- movable, seed, unassigned, out of range; labels
 * outside [0, B) count as unassigned.
 * bin_out / min_dist_out / margin_out as in chb_recruit_rows: the strict-'>' scan over dist_out's row (lowest index among
 * equal minima, -1 when every entry is +inf), its distance, and the margin to the runner-up (+inf without a finite
 * runner-up, never inf - inf).  dist_out, min_dist_out, margin_out may each be NULL; bin_out may be NULL if dist_out is
 * not.
 * row_idx == NULL means all rows 0 .. N-1 in order, and Q must then be N (CHB_EINVAL otherwise).  Otherwise every
 * row_idx[q] must lie in [0, N): checked on the host before anything is enqueued, CHB_EINVAL otherwise; repeats are
 * allowed.  Q = 0 is a no-op, with row_idx == NULL too (the one case in which Q need not be N).
 *   - limits: m <= 16 and B <= 8192, CHB_EUNSUPPORTED beyond; without resident samples CHB_ESTATE;
 *   - like chb_recruit_rows the call reads the resident matrix and `labels` and nothing else: it uses no state of a fit and
 *     leaves every counter, memo and switch of the context as it found it.  While a stepwise fit is open it is refused
 *     with CHB_ESTATE and the fit stays usable;
 *   - no row is uploaded: the positions are scored in chunks of 16384 (chb_counter "recruit_chunk") of which only the
 *     sample indices go to the device, as int32; kernels on the context's stream, the result copies of the neighbouring
 *     chunks under them on the context's second stream, through the pinned buffers chb_recruit_rows uses;
 *   - one GPU: with a communicator (world > 1) each rank scores the positions it is given, there is no collective. */
int chb_audit_rows(chb_ctx *h, const int64_t *labels, int64_t B, int m, const int64_t *row_idx, int64_t Q,
                   int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);

/* Neighbour sweep: chb_audit_rows / chb_recruit_rows for a LIST of m in one pass -- does a finished labelling hold up at
 * other numbers of neighbours?  The calls are defined by the single-m calls: for every j in [0, nm), slice j of each
 * output -- bin_out + j*Q, min_dist_out + j*Q, margin_out + j*Q, dist_out + j*Q*B -- is bit for bit what chb_audit_rows /
 * chb_recruit_rows returns for m = ms[j] on the same other arguments (+inf included).  The outputs are m-major and in the
 * order of ms[], which need not be sorted.
 * How: the members of a bin are ordered by the total order (distance, sample index), so the m' nearest are the first m'
 * entries of the list of the max(ms) nearest, and entry (r, c) of the Gram tile of the shifted vertices depends on vertices
 * r and c alone, so the m' x m' problem is the leading block of the tile of the largest m.  One selection stream (every row
 * against every member of every bin: the dominant cost) and one Gram tile per (row, bin) serve the whole list; only the
 * 16-lane solves repeat, each on exactly the tile the single-m kernel would have formed.
 *   - ms: nm distinct values, 1 <= nm <= 16, each in 1 .. 16.  NULL ms, nm outside 1 .. 16, an entry < 1 or a repeated
 *     entry is CHB_EINVAL; an entry > 16 is CHB_EUNSUPPORTED;
 *   - every other rule is the single-m call's: dist_out, min_dist_out, margin_out may each be NULL, bin_out may be NULL if
 *     dist_out is not; row_idx == NULL means all rows and Q must then be N; every row_idx[q] must lie in [0, N); B <= 8192
 *     (CHB_EUNSUPPORTED beyond); D must be the resident samples' D; CHB_ESTATE without resident samples or while a
 *     stepwise fit is open (the fit stays usable); Q = 0 is a no-op; every check runs on the host before anything is
 *     enqueued; the call uses no state of a fit and leaves every counter (but "recruit_multi_rows"), memo and switch of
 *     the context as it found it; with a communicator each rank scores what it is given, there is no collective;
 *   - chunks: max(64, 16384 / nm rounded down to a multiple of 64) rows per launch (chb_counter "recruit_multi_rows": the
 *     figure of the last such call), through the buffers and the two streams of the single-m calls -- the nm result slices
 *     of a chunk never need more device or pinned memory than the results of a single-m chunk of 16384 rows;
 *   - profile names "audit_multi" / "recruit_multi", work units = (row, bin, m) triples. */
int chb_audit_rows_multi(chb_ctx *h, const int64_t *labels, int64_t B, const int *ms, int nm,
                         const int64_t *row_idx, int64_t Q,
                         int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);
int chb_recruit_rows_multi(chb_ctx *h, const int64_t *labels, int64_t B, const int *ms, int nm,
                           const double *Y, int64_t Q, int64_t D,
                           int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);

/* Bin report: what chb_audit_rows says about a labelling, summed up per (own bin, other bin) pair on the device -- which
 * bins bleed into each other and which are cleanly apart -- without a per-row value crossing the host boundary.
 * The call is defined by chb_audit_rows on the same arguments: for every position q whose own label
 * a = labels[row_idx[q]] lies in [0, B), with d[q][.] the audit's leave-one-out distances and bin[q] its strict-'>' scan:
 *   confusion[a*B + bin[q]] += 1, or unplaced[a] += 1 where bin[q] == -1;
 *   for every bin b with d[q][b] finite: dcnt[a*B + b] += 1, dmin[a*B + b] = min(., d[q][b]), dsum[a*B + b] += d[q][b];
 *   dmin is +inf and dsum 0 where dcnt is 0.
 * Positions whose own label lies outside [0, B) are not scored at all (no kernel work is spent on them); *n_skipped
 * counts them.  Repeats in row_idx count as often as they occur.  confusion, dcnt, dmin, dsum: B*B, unplaced: B.
 * Each output may be NULL; all six NULL is CHB_EINVAL.  Q = 0, or no position with a label in [0, B), gives zero / +inf
 * tables and CHB_OK.
 *   - row_idx == NULL, Q, the limits (m <= 16, B <= 8192: CHB_EUNSUPPORTED beyond), CHB_ESTATE without resident samples or
 *     while a stepwise fit is open (the fit stays usable), and "uses no state of a fit and leaves every counter, memo and
 *     switch of the context as it found it" are chb_audit_rows' rules; every check runs on the host before anything is
 *     enqueued;
 *   - the scored positions are put in label order by a stable counting sort on the host (a label's positions keep the
 *     order of row_idx: ascending sample index for row_idx == NULL) and scored in chunks of at most 16384 cut from that
 *     order; per chunk the int32 sample indices and the int32 {label, first position} of each label's run go up, nothing
 *     comes down before the tables after the last chunk.  The tables live on the device, 32 bytes per (a, b) pair (24 for
 *     dcnt / dmin / dsum, 8 for confusion), allocated by the context and zeroed at the call's start;
 *   - determinism: there is no atomic, floating-point or other.  confusion, unplaced, dcnt and dmin are exact.  dsum[a][b]
 *     is the sum of the finite d[q][b] of label a's positions in this guaranteed order: the label's positions, in the
 *     order above, are taken in blocks of 64 consecutive positions (the last block may be shorter; positions whose
 *     distance is not finite keep their place in a block and add nothing); each block is summed in order starting from
 *     0, and the block sums are added in block order starting from 0.  No chunk boundary splits a block (a chunk that
 *     would is cut up to 63 positions short), so dsum is bit-identical from call to call and does not depend on where the
 *     chunks fall; row_idx == NULL and row_idx = 0 .. N-1 give the same bits;
 *   - one GPU: with a communicator (world > 1) each rank reports on the positions it is given, there is no collective. */
int chb_bin_report(chb_ctx *h, const int64_t *labels, int64_t B, int m, const int64_t *row_idx, int64_t Q,
                   int64_t *confusion, int64_t *unplaced, int64_t *dcnt, double *dmin, double *dsum,
                   int64_t *n_skipped);

/* Pair scoring: the hull distance of a LIST of (row, bin) pairs instead of every row against every bin -- each contig
 * against its own bin, the rows of two confused bins against those two, a second look at a few rows.  Both calls are
 * defined by the dense ones: dist_out[p] of chb_audit_pairs is bit for bit entry [bin_idx[p]] of the dist_out row that
 * chb_audit_rows returns for sample row_idx[p] on the same labels, B, m and metric (+inf included), dist_out[p] of
 * chb_recruit_pairs the same entry of chb_recruit_rows' row for Y[row_of[p]] (Y: Q rows of D columns).  Leave-one-out is
 * the audit's rule: only the sample's own index is withheld, whatever bin the pair names, and a twin with the same
 * coordinates stays a candidate.  Pairs may repeat and come in any order; dist_out (P doubles) is in the caller's order.
 * P = 0 (for chb_recruit_pairs also together with Q = 0) is a no-op and CHB_OK.
 *   - CHB_EINVAL: a null context; P < 0, Q < 0, B < 1 or m < 1; with P > 0 a null labels, bin_idx, row_idx / row_of, Y or
 *     dist_out; a bin_idx entry outside [0, B), a row_idx entry outside [0, N), a row_of entry outside [0, Q); D other
 *     than the resident samples'.  CHB_EUNSUPPORTED: m > 16, B > 8192.  CHB_ESTATE: no resident samples, or a stepwise fit
 *     is open (the fit stays usable).  Every check runs on the host before anything is enqueued, in the order of the
 *     dense calls' checks where they overlap;
 *   - the cost is the members streamed: the pairs are put in bin order by a stable counting sort on the host, each bin's
 *     run is cut into tiles of at most 64 pairs, and a tile streams its bin's members once -- P pairs of one bin cost
 *     ceil(P / 64) passes over that bin and nothing over any other.  chb_counter "pair_tiles": the tiles of the last call;
 *   - chunks: runs of whole tiles with at most 16384 pairs (chb_counter "recruit_chunk"); per chunk the int32 tile table
 *     {bin, first pair, pairs} and the int32 sample indices (chb_audit_pairs) or the pairs' rows of Y (chb_recruit_pairs:
 *     a row named by two pairs travels twice) go up and one double per pair comes down, through the dense calls' pinned
 *     double buffer and second stream.  There is no Q x B table anywhere and no row reduction;
 *   - like the dense calls they use no state of a fit and leave every counter (but "pair_tiles"), memo and switch of the
 *     context as they found it; one GPU: with a communicator (world > 1) there is no collective;
 *   - profile names "audit_pairs" / "recruit_pairs": one launch per chunk, work units = pairs. */
int chb_audit_pairs(chb_ctx *h, const int64_t *labels, int64_t B, int m,
                    const int64_t *row_idx, const int64_t *bin_idx, int64_t P, double *dist_out);
int chb_recruit_pairs(chb_ctx *h, const int64_t *labels, int64_t B, int m,
                      const double *Y, int64_t Q, int64_t D,
                      const int64_t *row_of, const int64_t *bin_idx, int64_t P, double *dist_out);

/* Leave-group-out audit: the four audit-side calls with a row's whole GROUP withheld, not only the row.  CH-Bin cuts long
 * contigs into pieces (preprocess.py:72-101) whose rows are nearly identical; with only the row itself withheld a
 * piece's nearest members are its own siblings and every margin looks sound.  groups[N] holds one int64 per resident
 * sample: any non-negative value is a group id (values up to 2^62, not dense), a negative value means no group.  For a
 * scored sample r the withheld set is
 *     W(r) = {r} + {p : groups[p] >= 0 and groups[p] == groups[r]},
 * removed from the candidates of EVERY bin (siblings may carry different labels).  Everything else is the ungrouped
 * call's definition: the selection arithmetic and the (distance, index) order, a twin with equal coordinates but another
 * group stays a candidate, +inf for a bin with no member left, the strict-'>' scan and the margins.  A row with
 * groups[r] < 0 is scored exactly as the ungrouped call scores it.
 * Each call is defined by its ungrouped form: with labels_g = labels in which every member of group g is set to -1, the
 * result for a row of g is bit for bit what the ungrouped call returns for that row on labels_g (a candidate's distance
 * does not depend on where it sits among the members, the lists are a total order on (distance, index), and the Gram
 * tile and the solve depend on the list alone).  chb_bin_report_grouped keys its tables by the rows' labels in `labels`
 * and sums dsum in chb_bin_report's order.
 *   - the argument list is the ungrouped call's with groups after labels.  groups == NULL is CHB_EINVAL (use the
 *     ungrouped call); every other check is the ungrouped call's, in its order, on the host before anything is enqueued:
 *     m <= 16 and B <= 8192 (CHB_EUNSUPPORTED beyond), CHB_ESTATE without resident samples or while a stepwise fit is
 *     open (the fit stays usable), Q = 0 / P = 0 a no-op, row_idx == NULL all rows;
 *   - one launch per chunk exactly as in the ungrouped call -- the kernel does the withholding with one more compare per
 *     offered member -- through the same chunks, streams and pinned buffers; the profile names ("audit", "audit_multi",
 *     "audit_pairs", "bin_report") and the counters "recruit_chunk", "recruit_multi_rows", "pair_tiles" are the ungrouped
 *     call's.  The group ids are made dense int32 on the host once per call; 4 bytes per resident sample and 4 per
 *     labelled sample go up next to the member list;
 *   - there is no context-level group state and no recruit form (new rows have no siblings among the samples); the calls
 *     use no state of a fit and leave no trace on the context. */
int chb_audit_rows_grouped(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m,
                           const int64_t *row_idx, int64_t Q,
                           int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);
int chb_audit_rows_multi_grouped(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B,
                                 const int *ms, int nm, const int64_t *row_idx, int64_t Q,
                                 int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);
int chb_audit_pairs_grouped(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m,
                            const int64_t *row_idx, const int64_t *bin_idx, int64_t P, double *dist_out);
int chb_bin_report_grouped(chb_ctx *h, const int64_t *labels, const int64_t *groups, int64_t B, int m,
                           const int64_t *row_idx, int64_t Q,
                           int64_t *confusion, int64_t *unplaced, int64_t *dcnt, double *dmin, double *dsum,
                           int64_t *n_skipped);

/* Witnesses for pair scoring: the pair calls' distances together with what each was measured against -- which members of
 * the bin form the hull, how far each is from the row, and with what weights they make the hull's nearest point.  The
 * plain pair calls compute all of it and return one double; these return it, one record of m slots per pair.
 *   - dist_out[p] (P doubles; may be NULL here) is bit for bit what the matching plain call returns for pair p, +inf
 *     included: chb_audit_pairs (groups == NULL), chb_audit_pairs_grouped (groups != NULL: the withheld set W(r) above) or
 *     chb_recruit_pairs, on the same other arguments and metric;
 *   - nbr_idx[p*m + a] is the sample index of vertex a of the hull that distance was measured to: the members the kernel
 *     selected for the pair, in the order of its own list, after the call's withholding (the row itself; with groups also
 *     its group; nothing for chb_recruit_pairs_witness -- a new row equal to a sample has that sample as a vertex at
 *     distance 0).  Slots at or past the number of members left are -1 (chb_topm_per_bin's convention): fewer than m real
 *     slots mean the bin had no more members to offer, and a pair with none has dist_out +inf and every slot padding.
 *     The list's order is (distance, sample index) ascending, where "distance" is the ROOTED value reported in nbr_dist,
 *     not the squared sum under it: two members whose squared sums differ but round to the same square root are ordered
 *     by index.  That is chb_topm_per_bin's order too (both keep their lists with the same code);
 *   - nbr_dist[p*m + a] is that member's Euclidean distance to the row in the selection arithmetic -- the correctly
 *     rounded sqrt of the k-sequential unfused sum of squared differences, chb_pairwise_distance's entry bit for bit.
 *     Padding is +inf;
 *   - alpha[p*m + a] is the weight of vertex a in the nearest point of the hull under the context's metric
 *     (chb_set_metric), exactly as the solver that produced dist_out returned it: the nearest point is
 *     sum_a alpha[p*m + a] X[nbr_idx[p*m + a]] and dist_out[p] its distance from the row, up to the solver's tolerance.
 *     Padding is 0.  Convex metric: the weights are >= 0 and sum to 1; a weight of exactly 0 means the vertex is not in
 *     the solver's support.  Affine metric: they sum to 1 and may be negative (the nearest point of the affine hull need
 *     not lie between the vertices).  Where the vertices are dependent -- twins with equal coordinates, more vertices than
 *     dimensions allow -- the nearest point is unique but the weights are not: any optimal vector is a valid answer and
 *     the one returned is whichever the active-set iteration ended on;
 *   - each of nbr_idx, nbr_dist, alpha may be NULL; with P > 0 all three NULL is CHB_EINVAL (the call without witnesses is
 *     the one to use).  Outputs are in the caller's pair order; pairs may repeat and get equal records;
 *   - every other rule is the plain pair call's, in its order, on the host before anything is enqueued: m <= 16 and
 *     B <= 8192 (CHB_EUNSUPPORTED beyond); CHB_ESTATE without resident samples or while a stepwise fit is open (the fit
 *     stays usable); bin_idx in [0, B), row_idx in [0, N), row_of in [0, Q), D the resident samples' (CHB_EINVAL); P = 0 a
 *     no-op; no state of a fit is used and nothing of the context changes but the counter "pair_tiles"; no collective;
 *   - chunks, tiles and streams are the pair calls' (bin order, tiles of at most 64 pairs, chunks of whole tiles up to 16384
 *     pairs), one launch per chunk under the plain calls' profile names "audit_pairs" / "recruit_pairs".  On the device a
 *     pair's record is 16 slots in each of three arrays (int32 index, double distance, double weight: 320 bytes per pair)
 *     of which the kernel writes the first m; the arrays the caller asked for come down on the copy stream through pinned
 *     buffers of their own and the host unpack compacts 16 slots to m and int32 to int64.  These buffers are allocated by
 *     a context's first witness call: a context that never makes one allocates nothing more than before. */
int chb_audit_pairs_witness(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */,
                            int64_t B, int m, const int64_t *row_idx, const int64_t *bin_idx, int64_t P,
                            double *dist_out, int64_t *nbr_idx, double *nbr_dist, double *alpha);
int chb_recruit_pairs_witness(chb_ctx *h, const int64_t *labels, int64_t B, int m,
                              const double *Y, int64_t Q, int64_t D,
                              const int64_t *row_of, const int64_t *bin_idx, int64_t P,
                              double *dist_out, int64_t *nbr_idx, double *nbr_dist, double *alpha);

/* Nearest bins per row: the k closest bins of every row with their distances, ranked on the device -- "which bin, and
 * which bins come next" without the Q x B table crossing the host boundary (shortlists of (row, bin) pairs for the pair
 * and witness calls, soft membership, recruits whose second choice is as close as their first).
 * Both calls are defined by the dense call on the same arguments and metric: chb_audit_rows (groups == NULL),
 * chb_audit_rows_grouped (groups != NULL: the withheld set W(r) above) or chb_recruit_rows.  With d[.] that call's dist_out
 * row for position q:
 *   - the FINITE entries are ranked by (d[c], c) ascending: a total order, exact ties go to the lower bin;
 *   - near_dist[q*k + j] is the j-th distance, bit for bit, and near_bin[q*k + j] its bin;
 *   - slots at or past the number of finite entries hold bin -1 and distance +inf.  k > B is allowed and pads.  There is
 *     no NaN: every distance is sqrt(fmax(val, 0)).
 * So slot 0 is the dense call's bin_out / min_dist_out, and near_dist[q*k + 1] - near_dist[q*k] is its margin_out bit for
 * bit where slot 1 is real (the margin is +inf where it is not).
 *   - near_bin, near_dist: Q*k each; either may be NULL, both NULL is CHB_EINVAL;
 *   - k < 1 is CHB_EINVAL (with the range checks of Q, B and m); k > 16 is CHB_EUNSUPPORTED, right behind m > 16;
 *   - every other rule is the dense call's, in its order, on the host before anything is enqueued: row_idx == NULL means
 *     all rows and Q must then be N; every row_idx[q] in [0, N); D the resident samples' (CHB_EINVAL); B <= 8192
 *     (CHB_EUNSUPPORTED beyond); CHB_ESTATE without resident samples or while a stepwise fit is open (the fit stays
 *     usable); Q = 0 is a no-op; no collective; the call uses no state of a fit and leaves every counter, memo and switch
 *     of the context as it found it;
 *   - chunks, streams and events are the dense calls' (16384 rows per chunk).  Per chunk the dense call's kernel runs
 *     under its profile name "audit" / "recruit" and leaves the chunk's rows x B table on the device; a second kernel,
 *     profile name "nearest_bins" (work units = (row, bin) pairs), ranks it there in place of the row reduction: 16 lanes
 *     per row keep the row's sorted list in registers.  k int32 bins and k doubles per row come down through pinned
 *     buffers of their own -- 12 k bytes per row instead of 8 B -- and the host unpack widens int32 to int64.  The table
 *     itself is never copied and no pinned memory is held for it.  The buffers are allocated by a context's first such
 *     call: a context that never makes one allocates nothing more than before.
 * There is no list-of-m form, no pair form and no bin-report form. */
int chb_audit_rows_nearest(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */,
                           int64_t B, int m, int k, const int64_t *row_idx, int64_t Q,
                           int64_t *near_bin, double *near_dist);
int chb_recruit_rows_nearest(chb_ctx *h, const int64_t *labels, int64_t B, int m, int k,
                             const double *Y, int64_t Q, int64_t D,
                             int64_t *near_bin, double *near_dist);

/* Row scoring for any number of neighbours up to CHB_MAX_NEIGHBORS = 64: one entry point per family for every m, so a
 * labelling fitted with 16 < num_neighbors <= 64 can be audited at its own m and rows can be recruited into it.
 *   - 1 <= m <= 16 (and every m the existing calls refuse as a bad argument): the call forwards -- chb_audit_rows_wide to
 *     chb_audit_rows (groups == NULL) or chb_audit_rows_grouped; chb_recruit_rows_wide to chb_recruit_rows;
 *     chb_audit_pairs_wide to chb_audit_pairs / chb_audit_pairs_grouped, or with idx_out != NULL to chb_audit_pairs_witness
 *     (nbr_idx = idx_out, no other witness output); chb_recruit_pairs_wide to chb_recruit_pairs or
 *     chb_recruit_pairs_witness.  Results, return codes and error texts are those calls', bit for bit.
 *   - 16 < m <= 64: the definition of those calls with the limit lifted.  Per (row, bin) the up to m members nearest by
 *     (distance, sample index), distances with chb_pairwise_distance's arithmetic; an audit withholds the row itself and,
 *     with groups, every sample of the row's non-negative group (the withheld set W(r) above); the distance to the
 *     selected members' hull under the context's metric, +inf for a bin without a candidate; bin_out / min_dist_out /
 *     margin_out by the dense calls' strict-'>' scan over the row.
 *     BIT-DEFINED: the selection -- idx_out[p*m + a] is entry a of pair p's list, -1 padded, exactly what chb_topm_per_bin
 *     returns for a resident row of the same labelling (with the row, and its group, withheld); a pair's dist_out against
 *     the dense wide call's entry on the same arguments, whatever tile, chunk and list position the pair falls into;
 *     repeated calls; the row reduction against dist_out.
 *     NOT bit-defined: a distance against chb_hull_distance_batch on the same list.  The solver is the same, but the Gram
 *     matrix of the shifted vertices comes from the fp64 matrix core here and from one fused multiply-add per feature
 *     there: the two agree to rounding (relative 1e-13 on well-conditioned sets).  On affinely dependent sets the affine
 *     metric has no unique answer and none is promised, as for m <= 16.
 *   - checks, in the existing calls' order: ranges (Q, B, m: CHB_EINVAL); null arguments; outputs (the dense calls: bin_out
 *     and dist_out both NULL; the pair calls: row_idx / row_of, bin_idx or dist_out NULL with P > 0 -- idx_out may be NULL);
 *     no resident samples (CHB_ESTATE); D; m > 64, then m > 32 on a device that does not grant the 66 KiB of LDS per
 *     workgroup the 64-vertex kernel needs (CHB_EUNSUPPORTED); B > 8192 (CHB_EUNSUPPORTED); an open stepwise fit
 *     (CHB_ESTATE, the fit stays usable); Q = 0 / P = 0 (CHB_OK, nothing further is read); the ranges of row_idx, then
 *     bin_idx / row_of.  A refused call writes nothing.
 *   - the call uses no state of a fit and leaves every counter (but "recruit_wide_rows" and, the pair calls,
 *     "pair_tiles"), memo and switch of the context as it found it; no collective.
 *   - two kernels per chunk on the dense calls' pipeline (streams, pinned staging, label CSR, dense group ids, pair plan
 *     and tile table are theirs): a tiled selection that leaves m + 1 int32 per (row, bin) problem in a device list
 *     buffer, profile names "audit_wide_select" / "recruit_wide_select" / "audit_pairs_wide_select" /
 *     "recruit_pairs_wide_select", and one wavefront per problem for the hull, "..._wide_solve" (work units of both =
 *     (row, bin) problems); the dense calls' row reduction follows.  Rows per chunk: the largest multiple of 64 whose list
 *     buffer rows * width * (m + 1) * 4 bytes stays within 256 MiB (width = B, or 1 for the pair calls), clamped to
 *     [64, 16384]: chb_counter "recruit_wide_rows".  The list buffer and the idx_out staging are allocated by a context's
 *     first wide call with m > 16 and freed with the context. */
int chb_audit_rows_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */, int64_t B, int m,
                        const int64_t *row_idx, int64_t Q,
                        int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);
int chb_recruit_rows_wide(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q, int64_t D,
                          int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);
int chb_audit_pairs_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */, int64_t B, int m,
                         const int64_t *row_idx, const int64_t *bin_idx, int64_t P,
                         double *dist_out, int64_t *idx_out /* may be NULL: [P][m], -1 padded */);
int chb_recruit_pairs_wide(chb_ctx *h, const int64_t *labels, int64_t B, int m, const double *Y, int64_t Q, int64_t D,
                           const int64_t *row_of, const int64_t *bin_idx, int64_t P,
                           double *dist_out, int64_t *idx_out /* may be NULL */);

/* Nearest bins, bin report and pair witnesses for any number of neighbours up to CHB_MAX_NEIGHBORS = 64: what a user turns
 * to after an audit at 16 < m <= 64 -- which bins come next, which bins bleed into each other, which contigs vouch for a
 * pair and with what weights.
 *   - 1 <= m <= 16 (and every m the existing calls refuse as a bad argument): each forwards -- chb_audit_rows_nearest_wide to
 *     chb_audit_rows_nearest, chb_recruit_rows_nearest_wide to chb_recruit_rows_nearest, chb_bin_report_wide to
 *     chb_bin_report (groups == NULL) or chb_bin_report_grouped, chb_audit_pairs_witness_wide to chb_audit_pairs_witness,
 *     chb_recruit_pairs_witness_wide to chb_recruit_pairs_witness.  Results, return codes and error texts are those
 *     calls', bit for bit.
 *   - 16 < m <= 64: each is defined by the wide call above on the same arguments and metric.
 *     NEAREST BINS: the finite entries of the dist_out row of chb_audit_rows_wide / chb_recruit_rows_wide ranked by
 *     (distance, bin) ascending, bit for bit, exact ties to the lower bin, -1 / +inf padding, k > B pads: slot 0 is that
 *     call's bin_out / min_dist_out, slot 1 minus slot 0 its margin_out bit for bit.  The chunk's rows x B table is ranked
 *     on the device in place of the row reduction (profile name "nearest_bins") and never comes down.
 *     BIN REPORT: the tables of chb_bin_report's definition applied to chb_audit_rows_wide's distances (with groups: the
 *     leave-group-out ones).  confusion, unplaced, dcnt and dmin are exact; dsum follows the block order documented for
 *     chb_bin_report (blocks of 64 positions of a label, no chunk boundary inside a block), so it is bit-identical from
 *     call to call and independent of where chunks fall -- the chunks are cut at "recruit_wide_rows" positions (as few as
 *     64 with many bins and large m), then back to the label's block boundary.
 *     WITNESS: dist_out is bit for bit chb_audit_pairs_wide / chb_recruit_pairs_wide; nbr_idx those calls' idx_out (hence
 *     chb_topm_per_bin's list); nbr_dist[p*m + a] the member's rooted selection distance, chb_pairwise_distance's entry
 *     bit for bit, +inf padding; alpha[p*m + a] the weight of vertex a exactly as the one-wavefront solver returned it
 *     for the problem that produced dist_out, 0 padding.  A pair without vertices has +inf, all -1, all +inf, all 0.  The
 *     meaning under the affine metric and the non-uniqueness among dependent vertices are as documented for m <= 16.
 *     Each of nbr_idx, nbr_dist, alpha may be NULL; all three NULL with P > 0 is CHB_EINVAL.
 *   - checks, in the existing calls' order: ranges (Q / P, B, m, and k < 1: CHB_EINVAL); null arguments; outputs; no
 *     resident samples (CHB_ESTATE); D; m > 64, then m > 32 on a device that does not grant the 66 KiB of LDS per workgroup
 *     (CHB_EUNSUPPORTED); k > 16 (CHB_EUNSUPPORTED); B > 8192 (CHB_EUNSUPPORTED); an open stepwise fit (CHB_ESTATE, the fit
 *     stays usable); Q = 0 / P = 0 (CHB_OK, nothing further is read); the ranges of row_idx, then bin_idx / row_of.  A
 *     refused call writes nothing.
 *   - the call uses no state of a fit and leaves every counter (but "recruit_wide_rows" and, the pair forms,
 *     "pair_tiles"), memo and switch of the context as it found it; no collective.
 *   - the wide calls' pipeline and profile names ("..._wide_select", "..._wide_solve"), then "nearest_bins" /
 *     "bin_report" as for m <= 16.  The witness forms of the two kernels add, per pair, m doubles each behind the list's
 *     ids: the selection kernel the entries' distances, the solve kernel the lanes' weights; only what the caller asked
 *     for comes down, through pinned buffers of their own, and the host unpacks it to the caller's pair order.  These
 *     buffers are allocated by a context's first such call with m > 16 and freed with the context. */
int chb_audit_rows_nearest_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */, int64_t B, int m,
                                int k, const int64_t *row_idx, int64_t Q, int64_t *near_bin, double *near_dist);
int chb_recruit_rows_nearest_wide(chb_ctx *h, const int64_t *labels, int64_t B, int m, int k,
                                  const double *Y, int64_t Q, int64_t D, int64_t *near_bin, double *near_dist);
int chb_bin_report_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */, int64_t B, int m,
                        const int64_t *row_idx, int64_t Q,
                        int64_t *confusion, int64_t *unplaced, int64_t *dcnt, double *dmin, double *dsum,
                        int64_t *n_skipped);
int chb_audit_pairs_witness_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */, int64_t B, int m,
                                 const int64_t *row_idx, const int64_t *bin_idx, int64_t P,
                                 double *dist_out, int64_t *nbr_idx, double *nbr_dist, double *alpha);
int chb_recruit_pairs_witness_wide(chb_ctx *h, const int64_t *labels, int64_t B, int m,
                                   const double *Y, int64_t Q, int64_t D,
                                   const int64_t *row_of, const int64_t *bin_idx, int64_t P,
                                   double *dist_out, int64_t *nbr_idx, double *nbr_dist, double *alpha);

/* The neighbour sweep for lists with entries up to CHB_MAX_NEIGHBORS = 64: chb_audit_rows_multi / chb_recruit_rows_multi
 * for a list whose entries need not stop at 16, e.g. (5, 15, 24, 32, 64) around a labelling fitted at m = 24 -- one
 * wide selection pass serves every entry above 16 (and the list calls' one pass those up to 16); only the hull solves
 * repeat.
 *   - outputs: m-major and in the order of ms[], as chb_audit_rows_multi's.  Slice j of each is BIT FOR BIT what
 *     chb_audit_rows_wide(..., groups, ..., ms[j], ...) / chb_recruit_rows_wide(..., ms[j], ...) returns on the same
 *     other arguments and metric, +inf included (and so, for ms[j] <= 16, chb_audit_rows / _grouped / chb_recruit_rows).
 *   - max(ms) <= 16, and every list the existing list calls refuse as a bad argument: the call forwards to
 *     chb_audit_rows_multi (groups == NULL), chb_audit_rows_multi_grouped or chb_recruit_rows_multi.  Result, return
 *     code, error text and counters ("recruit_multi_rows") are those calls'.
 *   - max(ms) > 16: entries up to 16 and above may be mixed, in any order.
 *   - checks, in the list calls' order, all before anything is enqueued: Q < 0 or B < 1; ms NULL; nm outside 1 .. 16; an
 *     entry < 1; a repeated entry (among 1 .. 64) (all CHB_EINVAL); null arguments; outputs (bin_out and dist_out both
 *     NULL); no resident samples (CHB_ESTATE); D; max(ms) > 64, then max(ms) > 32 on a device that does not grant the
 *     66 KiB of LDS per workgroup (CHB_EUNSUPPORTED); B > 8192 (CHB_EUNSUPPORTED); an open stepwise fit (CHB_ESTATE,
 *     the fit stays usable); Q = 0 (CHB_OK); the row_idx rules.  A refused call writes nothing.
 *   - per chunk: the entries up to 16, if any, by the list calls' kernel ("audit_multi" / "recruit_multi", work units =
 *     (row, bin, m) triples over those entries); the wide selection once at max(ms) ("audit_multi_wide_select" /
 *     "recruit_multi_wide_select", work units = (row, bin) problems, max(ms) + 1 int32 per problem in the list buffer);
 *     one wavefront per (row, bin, entry above 16) that reads the first m' ids of the problem's list and does what the
 *     single call's wavefront does at m = m' ("..._multi_wide_solve", work units = those triples; the entries 17 .. 32 on
 *     the 32-vertex kernel and the entries 33 .. 64 on the 64-vertex kernel, one launch for each group the list has, both
 *     booked as one); the row reduction over all nm slices.  (A problem's Gram matrix is formed per entry, not once: the
 *     in-kernel loop over the entries that sharing it needs was measured and cost more than it saved, see DESIGN.md.)
 *   - rows per chunk: min(the wide calls' figure for max(ms), max(64, 16384 / nm rounded down to a multiple of 64)):
 *     chb_counter "recruit_wide_rows".  Otherwise the call uses no state of a fit and leaves every counter, memo and
 *     switch of the context as it found it; no collective. */
int chb_audit_rows_multi_wide(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */, int64_t B,
                              const int *ms, int nm, const int64_t *row_idx, int64_t Q,
                              int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);
int chb_recruit_rows_multi_wide(chb_ctx *h, const int64_t *labels, int64_t B, const int *ms, int nm,
                                const double *Y, int64_t Q, int64_t D,
                                int64_t *bin_out, double *dist_out, double *min_dist_out, double *margin_out);

/* The pair calls for a LIST of neighbour counts: chb_audit_pairs_wide / chb_recruit_pairs_wide for every entry of ms[]
 * from one selection pass per kernel -- the profile of `cohesion` over (1, 3, 5, 10, 15) in one call instead of five that
 * each stream the same members, or the sweep over each row's two or three nearest bins where the dense sweep's table
 * (chb_audit_rows_multi_wide) is B times the work.
 *   - ms holds nm distinct values, 1 <= nm <= 16, each in 1 .. CHB_MAX_NEIGHBORS = 64; entries up to 16 and above may be
 *     mixed, in any order.  One symbol per family for the whole range: these calls have no narrow twin.
 *   - dist_out [nm][P], m-major and in the order of ms[], pairs in the caller's order (they may repeat): dist_out + j * P
 *     is BIT FOR BIT what chb_audit_pairs_wide(h, labels, groups, B, ms[j], row_idx, bin_idx, P, dist, NULL) /
 *     chb_recruit_pairs_wide(h, labels, B, ms[j], Y, Q, D, row_of, bin_idx, P, dist, NULL) returns on the same arguments
 *     and metric, +inf included -- for ms[j] <= 16 that is chb_audit_pairs / _grouped / chb_recruit_pairs, and so the
 *     dense calls' entries.
 *   - why the bits hold: the m' nearest members are a prefix of the max(ms)-nearest list under the total order
 *     (distance, index), so one selection serves every entry.  Up to 16 the m' x m' problem is the leading block of the
 *     one Gram tile, exactly as in chb_audit_rows_multi; above 16 the solve wavefront reads nothing but the list, whose
 *     first m' ids are what the single call's selection leaves at m = m'.
 *   - checks, in the list calls' and pair calls' order, all on the host before anything is enqueued: null context; P < 0,
 *     Q < 0 or B < 1; ms NULL; nm outside 1 .. 16; an entry < 1; a repeated entry among 1 .. 64 (all CHB_EINVAL); with
 *     P > 0 a null labels / row_idx / row_of / bin_idx / Y / dist_out (CHB_EINVAL); no resident samples (CHB_ESTATE); D
 *     other than the resident samples' (CHB_EINVAL); max(ms) > 64, then max(ms) > 32 on a device that does not grant the
 *     66 KiB of LDS per workgroup (CHB_EUNSUPPORTED); B > 8192 (CHB_EUNSUPPORTED); an open stepwise fit (CHB_ESTATE, the
 *     fit stays usable); P = 0 (CHB_OK, nothing further is read); the ranges of row_idx / row_of, then of bin_idx
 *     (CHB_EINVAL).  A refused call writes nothing.
 *   - the plan is the single pair call's, unchanged: stable counting sort by bin, tiles of at most 64 pairs, chunks of whole
 *     tiles up to 16384 pairs -- chb_counter "pair_tiles" is the single call's.  A chunk's nm result slices are nm doubles
 *     per pair (at most 2 MiB: the chunks are not shortened for the list), its list buffer max(ms) + 1 int32 per pair.
 *   - per chunk: the entries up to 16, if any, in one launch of the pair kernel's list form ("audit_pairs_multi" /
 *     "recruit_pairs_multi", work units = (pair, entry up to 16)); with an entry above 16 the wide selection's pair form
 *     once at max(ms) ("audit_pairs_multi_wide_select" / "recruit_...", work units = pairs) and one wavefront per (pair,
 *     entry above 16) on the first m' ids of the pair's list ("..._pairs_multi_wide_solve", work units = those; the
 *     entries 17 .. 32 on the 32-vertex kernel and 33 .. 64 on the 64-vertex kernel, one launch for each group the list
 *     has, both booked as one).  A list with entries on both sides of 16 runs both selections, as the dense wide list
 *     does.
 *   - not offered: an idx_out or a witness form for a list -- the prefix of chb_audit_pairs_wide(..., idx_out) at max(ms)
 *     is every entry's list -- and a recruit form with groups (rows that are not samples have no siblings).
 *   - the call uses no state of a fit and leaves every counter, memo and switch of the context as it found it, except
 *     "pair_tiles" and, with an entry above 16, "recruit_wide_rows" (the single wide pair call's figure); no collective. */
int chb_audit_pairs_multi(chb_ctx *h, const int64_t *labels, const int64_t *groups /* may be NULL */, int64_t B,
                          const int *ms, int nm, const int64_t *row_idx, const int64_t *bin_idx, int64_t P,
                          double *dist_out /* [nm][P] */);
int chb_recruit_pairs_multi(chb_ctx *h, const int64_t *labels, int64_t B, const int *ms, int nm,
                            const double *Y, int64_t Q, int64_t D,
                            const int64_t *row_of, const int64_t *bin_idx, int64_t P, double *dist_out /* [nm][P] */);

/* distance_matrix.py:47-62 find_nearest_from_cluster with the reference's exact signature: the
 * caller supplies one row of a distance matrix (any provenance) and the current labels; selects
 * among {p : labels[p] == c} the (up to) m smallest by (row[p], p).  out_idx[m] (-1 padded). */
int chb_find_nearest_from_row(chb_ctx *h, int64_t c, const int64_t *labels, const double *row,
                              int64_t N, int m, int64_t *out_idx, int32_t *out_cnt);

/* hull_distance.py:7-35 convex_hull_distance (+ solve_qp.py:96-132), batched:
 * problem p = distance from sample query_idx[p] to conv{ samples[hull_idx[p*m_max + a]] }, entries
 * < 0 are padding; an empty hull gives +inf.  alpha (P*m_max, may be NULL) receives the convex
 * weights in hull_idx order (0 at padding). */
int chb_hull_distance_batch(chb_ctx *h, const int64_t *query_idx, int64_t P, const int64_t *hull_idx,
                            int m_max, double *dist, double *alpha);

/* hull_distance.py:90-108 calculate_distance(x, mat_p, qp_solver, "convex") for explicit points:
 * x[D], pts[m][D].  Does not touch the resident samples. */
int chb_hull_distance_points(chb_ctx *h, const double *x, const double *pts, int m, int64_t D,
                             double *dist, double *alpha);

/* algorithm.py:12-76 fit_cluster(samples, num_clusters, initial_bins, distance_matrix,
 * num_neighbors, max_iterations, "convex", qp_solver): the whole reassignment loop with the
 * reference's sequential (Gauss-Seidel) semantics reproduced exactly by speculative batches.
 *   initial_bins[N]      -1 = movable (algorithm.py:38), others are fixed seeds
 *   perms[max_iter*n_move] the permutations algorithm.py:45 would draw, pre-drawn by the caller
 *                        from the legacy numpy RNG so the MT19937 stream matches ch_bin.py:22
 *   batch               speculative batch size (0 = default)
 *   labels_out[N], *iters_run, changed_per_iter[max_iter] (algorithm.py:63-68 counts); on an error return the
 *                        contents of labels_out are undefined (it may hold an earlier sweep's labels),
 *   min_dist_out[N] (may be NULL): winning hull distance of each movable contig's last visit */
int chb_fit_cluster(chb_ctx *h, int64_t B, const int64_t *initial_bins, const int64_t *perms,
                    int64_t n_move, int m, int max_iter, int batch, int64_t *labels_out,
                    int *iters_run, int64_t *changed_per_iter, double *min_dist_out);

/* Same, additionally margin_out[N] (may be NULL; needs min_dist_out; single GPU): the runner-up bin's hull
 * distance minus the winner's at each movable contig's last visit -- how far the argmin of
 * algorithm.py:57 is from flipping (0 on a tie; +inf when no other bin has a member, also when no bin
 * has one and the winning distance is +inf as well; NaN for seeds). */
int chb_fit_cluster_ex(chb_ctx *h, int64_t B, const int64_t *initial_bins, const int64_t *perms,
                       int64_t n_move, int m, int max_iter, int batch, int64_t *labels_out,
                       int *iters_run, int64_t *changed_per_iter, double *min_dist_out, double *margin_out);

/* ---- stepwise form of the same loop (one process per GPU; the host side exchanges labels
 * between ranks with RCCL/gloo between rounds).  Query slice [q_lo,q_hi) of each batch is the
 * part this rank evaluates; labels stay replicated on every rank. */
int chb_fit_begin(chb_ctx *h, int64_t B, const int64_t *initial_bins, int m);
/* open a batch: perm_slice[K] are the contigs visited, in order */
int chb_batch_begin(chb_ctx *h, const int64_t *perm_slice, int64_t K, int64_t q_lo, int64_t q_hi);
/* optional: starting labels for the rounds of this batch, positions [q_lo,q_hi) of guess[K] (other entries untouched).
 * A contig that has a label keeps it.  A still unlabelled one gets a bin by one of two rules, whichever the fit's
 * kernels have the data for: on the list-based paths (CHB_FUSED=0, more than 16 neighbours, rows too wide for the
 * shortlist stage) the bin of its nearest member outside the batch, ties to the lower bin; on the fused path the bin
 * whose num_neighbors-th nearest member outside the batch is nearest by the shortlist stage's single-precision bound.
 * Guaranteed are only: a labelled contig keeps its label, and every value lies in [-1, num_clusters) -- -1 where no bin
 * has a member outside the batch.  Any start gives the same final labels; a good one saves rounds. */
int chb_batch_guess(chb_ctx *h, int64_t *guess);
/* one speculative round: lab_prev[K] in; for positions [max(active,q_lo), q_hi) writes
 * lab_new[pos] and min_dist[pos] (arrays of length K, other entries untouched; min_dist may be NULL).
 *   - every lab_prev[i], i in [0,K), must lie in [-1, num_clusters): CHB_EINVAL otherwise;
 *   - active must lie in [0, K] and must not be smaller than the `active` of the previous round of the same batch
 *     (positions below it are final: a round keeps what the round before it found for a position whose candidates did
 *     not change, so that round must have evaluated the position): CHB_EINVAL otherwise.
 * Both are checked on the host before anything is enqueued; a refused call leaves the batch open and usable. */
int chb_batch_round(chb_ctx *h, const int64_t *lab_prev, int64_t active, int64_t *lab_new,
                    double *min_dist);
/* close the batch: labels[perm_slice[i]] = final[i].  Every final_labels[i] must lie in [-1, num_clusters): CHB_EINVAL
 * otherwise, checked on the host before anything is enqueued, and the batch stays open. */
int chb_batch_commit(chb_ctx *h, const int64_t *final_labels);
int chb_fit_labels(chb_ctx *h, int64_t *labels_out);

/* ---- multi-GPU inside chb_fit_cluster: one process (and one context) per GPU.  Rank 0 obtains a
 * 128-byte RCCL unique id, the host side broadcasts it (torch.distributed / MPI / files), every
 * rank calls chb_comm_init.  chb_fit_cluster then shards each speculative batch's positions over
 * the ranks and exchanges the label slices with RCCL all-gathers over xGMI; every rank must make
 * the same call with the same arguments and receives the same, complete result.  Before the first batch the ranks
 * all-gather {B, m, n_move, max_iter, batch size, N, D, metric, formulation switches, hashes of perms and initial_bins}:
 * a rank that was given something else makes the call fail with CHB_EINVAL on EVERY rank (nobody is left inside a
 * collective); the switches that may differ per context (CHB_SPECULATE, CHB_TILE_SKIP, CHB_PACK_INCR, the tile-skipping
 * memo of earlier fits) take their most conservative value of all ranks for that fit.  Every later exchange carries a
 * {sequence number, kind} tag and the statistics that steer the loop, so that all ranks take the same decisions; ranks
 * found out of step make the fit fail with CHB_ESTATE on every rank at the sweep's end. */
int chb_comm_unique_id(char *out128);
int chb_comm_init(chb_ctx *h, const char *id128, int rank, int world);
int chb_comm_destroy(chb_ctx *h);
/* The same sharded loop with the exchange done by the caller: fn(user, send, recv, bytes) must deliver the
 * `bytes` of every rank's `send` into recv[rank * bytes ..] on every rank (an all-gather on HOST buffers;
 * return 0 on success).  For transports other than RCCL (MPI, gloo, pipes) -- and the way two ranks can
 * share one GPU, which RCCL refuses.  Called from inside chb_fit_cluster, between device synchronisations. */
typedef int (*chb_allgather_fn)(void *user, const void *send, void *recv, size_t bytes);
int chb_comm_init_hook(chb_ctx *h, int rank, int world, chb_allgather_fn fn, void *user);
/* chb_set_samples for every rank of the communicator with ONE crossing of the host boundary: rank `root` passes its host
 * matrix X[N][D] (cli/clustering.py:53), the other ranks pass NULL; the matrix is uploaded on `root`, broadcast to the
 * other GPUs by RCCL over xGMI (109 MB at N = 100k, 1.17 GB at N = 1M) and every rank builds its own resident copy and
 * shadow rows.  N, D and root must agree on all ranks: before the broadcast the ranks exchange {own status, N, D, root}
 * (one small all-gather), and a rank that failed beforehand (no matrix on the root, an allocation) or disagrees makes the
 * call fail on EVERY rank instead of leaving the others blocked in the collective.  Needs chb_comm_init (with the hook
 * transport every rank simply calls chb_set_samples). */
int chb_bcast_samples(chb_ctx *h, const double *X, int64_t N, int64_t D, int root);
/* what the context's communicator really is: *rank / *world as given to chb_comm_init*, *comm_ranks = the rank count
 * RCCL itself reports for the communicator (ncclCommCount; 0 without an RCCL communicator), *transport = 0 none,
 * 1 RCCL, 2 host-staged hook.  Lets a benchmark line carry evidence of the exchange it ran over. */
int chb_comm_info(chb_ctx *h, int *rank, int *world, int *comm_ranks, int *transport);

/* ---- feature assembly: canonical k-mer frequency vectors.
 * Replaces the external seq2vec run of ch_bin/core/features/kmer_count.py:65-107 (and the
 * normalisation of the deprecated kmer-counter path, kmer_count.py:57-59): row i = counts of the
 * canonical k-mers (a k-mer and its reverse complement are one column) of contig i divided by
 * their sum; k = 4 gives the 136 k-mer columns of features.csv (config/default.ini:10).
 * Columns are ordered by the smaller 2-bit code (A<C<G<T) of the k-mer and its reverse complement;
 * windows containing anything but A/C/G/T (either case) are skipped; a contig without a valid
 * window yields a zero row.  seq2vec itself is not part of the reference tree: these two
 * conventions are unpinned (they permute / do not change distances between rows). */
/* number of columns for k (1 <= k <= 7), or a negative error code */
int chb_kmer_dim(int k);
/* seq: the contigs' bases back to back (host), offsets[n+1] their bounds; freq_out[n * dim] doubles;
 * counts_out (optional) [n * dim] raw counts.  Needs a context only for its device and stream. */
int chb_kmer_frequencies(chb_ctx *h, const unsigned char *seq, const int64_t *offsets, int64_t n, int k,
                         double *freq_out, uint32_t *counts_out);
/* The same for a LIST of k values counted in one pass (the reference's KmerK is a comma list, cli/features.py:85-92,128:
 * `4,5` gives 648 columns, `3,4,5` gives 680): the sequence is uploaded once, its bases are staged once per 4096 start
 * positions, and every start position serves all k of the list.  The blocks keep the order of ks[] (not sorted), and
 * every block is bit-identical to what chb_kmer_frequencies returns for that k alone.
 *   - the sequence goes up in chunks of whole contigs, at most 32 MiB of bases (chb_counter "kmer_chunk_bytes") and
 *     16384 contigs (chb_counter "kmer_chunk_rows") each, a longer contig as a chunk of its own, one chunk after the other
 *     on the context's stream (no copy / compute overlap): sequence, offsets, work-item table, row map and counts take
 *     the device memory of ONE chunk however many contigs there are.  What does grow with the call is the output matrix
 *     and, in chb_set_samples_from_sequences, the table `extra` (n_extra x S).  chb_counter "kmer_chunks" = chunks of
 *     the last call;
 *   - every argument check runs on the host before anything is enqueued. */
/* sum of chb_kmer_dim over ks[0..nk); ks distinct, each in [1,7], 1 <= nk <= 7: CHB_EINVAL / CHB_EUNSUPPORTED otherwise */
int chb_kmer_profile_dim(const int *ks, int nk);
/* freq_out[n * dim]: the blocks of ks[0], ks[1], ... side by side, each normalised by its own total (a block without a
 * valid window: zeros); counts_out (optional) the raw counts in the same layout.  seq / offsets as for
 * chb_kmer_frequencies, and the same checks of them; n = 0 is a no-op. */
int chb_kmer_profiles(chb_ctx *h, const unsigned char *seq, const int64_t *offsets, int64_t n,
                      const int *ks, int nk, double *freq_out, uint32_t *counts_out);
/* The same matrix built on the device, widened by S extra columns (coverage): row i = [k-mer blocks | extra[extra_row[i]]],
 * D = dim + S, and made the context's resident samples exactly as chb_set_samples_device(h, that matrix, n, D) would: the
 * matrix is built in a temporary device buffer and handed to the routine behind chb_set_samples_device (one device-to-
 * device copy more than strictly needed, accepted so that padded rows, shadow rows, memos and the end of an open stepwise
 * fit are the same state by construction).  No feature value crosses the host boundary.
 * extra: host [n_extra][S], may be NULL with S = 0; extra_row[n] (NULL = identity, then n_extra == n); every entry in
 * [0, n_extra), checked on the host before anything is enqueued: a refused call (those checks, a repeated or unsupported
 * k, nk outside 1..7, S < 0, n <= 0) leaves the resident samples untouched.  X_out (optional, host, n * D): a copy of the
 * matrix.  With a communicator every rank calls it for itself: there is no collective in it. */
int chb_set_samples_from_sequences(chb_ctx *h, const unsigned char *seq, const int64_t *offsets, int64_t n,
                                   const int *ks, int nk, const double *extra, int64_t n_extra, int64_t S,
                                   const int64_t *extra_row, double *X_out);

/* ---- measurement: HIP-event timing of kernel launches on the context's stream.
 * on = 0 off, 1 every kernel, 2 only "prefilter" and "hull_qp" (the two that dominate a sweep: four
 * event records per batch, cheap enough to leave on inside a timed region) */
int chb_profile_enable(chb_ctx *h, int on);
int chb_profile_reset(chb_ctx *h);
/* kernel: "prefilter" | "prefilter_update" | "rescore" | "rescore_update" | "query_norms" (once per fit) |
 * "fit_start" (bin centres + every labelled sample's shadow row, once per fit) |
 * "topm_fallback" | "topm_base" | "topm_update" | "hull_qp" | "slow_path" | "argmin" | "bucket" |
 * "pool" (upkeep of the shortlist stage's threshold pools: build once per fit, open + commit per batch) |
 * "prefilter_retry" (the exact two-sweep selection for the work items a pool batch's launch left on its overflow list) |
 * "pairwise" | "kmer_count" | "kmer_multi" (chb_kmer_profiles / chb_set_samples_from_sequences: the counting and the
 * finalise launch of one chunk; work units = bases) | "recruit" (chb_recruit_rows: selection + hull kernel and the row reduction of one chunk; work
 * units = (row, bin) pairs) | "audit" (chb_audit_rows: the same pair of launches for one chunk of resident rows; work units
 * = (row, bin) pairs; chb_bin_report books its two audit launches here as well) | "audit_multi" / "recruit_multi"
 * (chb_audit_rows_multi / chb_recruit_rows_multi: the same pair of launches for one chunk and a list of m; work units =
 * (row, bin, m) triples) | "audit_pairs" / "recruit_pairs" (chb_audit_pairs / chb_recruit_pairs: the one launch of a chunk;
 * work units = pairs) | "bin_report" (chb_bin_report: the launch
 * that folds one chunk's distances and bins into the B x B tables; work units = (row, bin) pairs) | "nearest_bins"
 * (chb_audit_rows_nearest / chb_recruit_rows_nearest: the launch that ranks one chunk's rows x B table, behind the dense
 * kernel booked under "audit" / "recruit"; work units = (row, bin) pairs) | "audit_wide_select" / "audit_wide_solve" and their
 * "recruit_" / "_pairs_" counterparts (the chb_*_wide calls with m > 16: a chunk's selection and hull launches; work units =
 * (row, bin) problems) | "audit_multi_wide_select" / "audit_multi_wide_solve" and their "recruit_" counterparts
 * (chb_audit_rows_multi_wide / chb_recruit_rows_multi_wide with an entry above 16: a chunk's one selection launch, work
 * units = (row, bin) problems, and its list solve launch, work units = (row, bin, entry above 16) triples; the entries up
 * to 16 are booked under "audit_multi" / "recruit_multi") | "audit_pairs_multi" / "recruit_pairs_multi"
 * (chb_audit_pairs_multi / chb_recruit_pairs_multi: a chunk's one launch for the entries up to 16; work units = (pair, entry
 * up to 16)) | "audit_pairs_multi_wide_select" / "audit_pairs_multi_wide_solve" and their "recruit_" counterparts (the same
 * calls with an entry above 16: a chunk's one selection launch, work units = pairs, and its list solve launches, work units
 * = (pair, entry above 16)).  For m <= 16 "hull_qp" is the fused selection + hull-distance kernel and
 * "slow_path" the exact path for what it leaves over; "rescore*" then only appear for m > 16 or CHB_FUSED=0. */
int chb_profile_get(chb_ctx *h, const char *kernel, double *total_ms, int64_t *launches,
                    double *work_units);
/* counters of the last chb_fit_cluster call: [0]=batches [1]=rounds [2]=hull distances evaluated
 * (incl. speculative re-evaluation) [3]=hull distances the sequential loop needs (sweeps*n_move*B) */
int chb_fit_stats(chb_ctx *h, int64_t *out4);
/* diagnostic counters: "prefilter_enabled" (1 when the fp16 shortlist stage is active: feature vectors of up to 573
 * columns -- 157 on the narrow builds, two to four 144-column slices beyond, which covers KmerK = 5; wider samples, or the
 * environment variable CHB_PREFILTER=0, select the brute-force selection kernel instead),
 * "prefilter_overflow" (shortlists that overflowed and were recomputed by brute force since the
 * last chb_fit_begin), "fused_enabled" (1 when the fused selection + hull kernels serve the fit), "segment_batches"
 * (batches of the last fit that cut a giant bin into segments), "batch_size" (speculative batch size of the last fit),
 * "tile_skip_state" (tile skipping of the last fit: 0 undecided, 1 kept on, -1 turned off because next to nothing could be
 * skipped), "tile_skipped" / "tile_seen" / "tile_unloaded" (wave-tiles whose compute was skipped / that were met / that
 * were never loaded, as sampled by about 64 workgroups of each base shortlist launch, a batch's launch counted once),
 * "fused_trim_pairs" / "fused_trim_in" / "fused_trim_kept" ((position, bin) pairs of the last fit whose shortlist the
 * m <= 5 fused kernel trimmed, rounds of a batch counted each; their candidates before and after),
 * "shortlist_short" ((position, bin) pairs of the last fit whose base shortlist reached the hull kernels with fewer than
 * min(num_neighbors, members of the bin) candidates or with a wild index: always 0, or chb_fit_cluster has returned
 * CHB_ESTATE at the end of that sweep -- the product build checks the shortlist stage's contract in every fused hull
 * launch), "lookahead_batches" (batches of the last fit whose successor was enqueued ahead of their convergence verdict
 * and kept: on one GPU and, since round 4, under the RCCL exchange), "lookahead_failed" (... and discarded because the
 * batch needed further rounds), "pool_batches" (batches of the last fit whose base shortlist launch took its thresholds
 * from the pools), "pool_state" (0 undecided = on, 1 kept on, -1 turned off because the shortlists came out long),
 * "pool_candidates" / "pool_pairs" (sampled shortlist lengths behind that decision), "pool_bad_slots" (for tests, while no
 * batch is open: slots of the last fit's pools that are not what the shortlist kernel relies on -- a usable slot of pool
 * (bin, home) holds a sample labelled with the bin, that sample's shadow row and key, under the tile's norm bound -- plus pools
 * whose count of usable rows is off; 0 without pools), "pack_region_moves" (regions of the persistent pack that ran full and
 * moved in the last fit), "exchanges" (framed all-gathers of the last fit under an exchange: one per batch for the
 * label guess, one per round), "recruit_chunk" (rows per launch of chb_recruit_rows, chb_audit_rows and -- at most -- chb_bin_report: a constant),
 * "recruit_multi_rows" (rows per launch of the last chb_audit_rows_multi / chb_recruit_rows_multi call: 16384 / nm rounded
 * down to a multiple of 64; 0 before the first), "pair_tiles" (tiles of at most 64 pairs of one bin -- the kernel's work
 * items -- of the last chb_audit_pairs / chb_recruit_pairs call that had pairs, their _wide, _witness and _multi forms among
 * them; 0 before the first),
 * "recruit_wide_rows" (rows per launch of the last chb_*_wide call with m > 16, a chb_*_rows_multi_wide call with an
 * entry above 16 among them: see there; 0 before the first),
 * "kmer_chunk_bytes" / "kmer_chunk_rows" (the most bases / contigs of one sequence chunk of chb_kmer_profiles and
 * chb_set_samples_from_sequences: constants), "kmer_chunks" (chunks of the last such call), "lane_exchange_mismatches" (for
 * tests: one small launch compares the hull kernels' in-register exchanges of a 16-lane group, and the Gram reduction
 * built on them, bit for bit with the shuffles they replace; the number of differences, always 0) */
int chb_counter(chb_ctx *h, const char *name, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* CHBIN_HIP_H */
