"""Mirror of ch_bin/core/clustering/algorithm.py."""
import contextlib
import dataclasses
import logging

import numpy as np

from .._lib import default_context
from .solve_qp import check_solver

logger = logging.getLogger(__name__)


def fit_cluster(
    samples: np.ndarray,
    num_clusters: int,
    initial_bins: np.ndarray,
    distance_matrix: np.ndarray = None,
    num_neighbors: int = 15,
    max_iterations: int = 10,
    metric: str = "convex",
    qp_solver: str = "quadprog",
    batch: int = 0,
) -> np.ndarray:
    """algorithm.py:12-76 with identical semantics and return value.

    `distance_matrix` is accepted for signature compatibility and ignored (may be None): the HIP
    path recomputes the needed distances, with cdist's exact rounding, instead of reading an
    N x N matrix.  The per-sweep permutations come from the same legacy global numpy RNG calls as
    algorithm.py:45, so after `np.random.seed(0)` (ch_bin.py:22) the visiting order -- and the RNG
    state left behind -- are the reference's.
    """
    if metric not in ("convex", "affine", "affine-qp"):
        raise NotImplementedError(f"Metric {metric} not implemented")  # hull_distance.py:108
    check_solver(qp_solver)                                              # solve_qp.py:132

    samples = np.ascontiguousarray(samples, dtype=np.float64)
    initial = np.ascontiguousarray(initial_bins, dtype=np.int64)
    points_to_assign = np.where(initial == -1)[0]                       # algorithm.py:38
    logger.debug("Assigning %s points.", len(points_to_assign))

    # algorithm.py:45 draws one permutation per sweep that actually runs.  Draw them all up front
    # for the kernel, then rewind and replay exactly as many draws as sweeps ran.
    state = np.random.get_state()
    perms = np.stack([np.random.permutation(points_to_assign) for _ in range(max_iterations)]) \
        if max_iterations > 0 else np.zeros((0, len(points_to_assign)), dtype=np.int64)

    ctx = default_context()
    ctx.set_samples_cached(samples)
    with ctx.using_metric(metric):
        labels, iters, changed = ctx.fit_cluster(int(num_clusters), initial, perms.astype(np.int64),
                                                 int(num_neighbors), int(max_iterations), batch=batch)

    np.random.set_state(state)
    for _ in range(iters):
        np.random.permutation(points_to_assign)

    n = len(samples)
    for i_iter in range(iters):                                          # algorithm.py:63-69
        if changed[i_iter] == 0:
            logger.info("Iteration %s: No changes with previous iteration... Stopping...", i_iter + 1)
            break
        logger.info("Iteration %s: Points changed clusters. avg=%s, count=%s", i_iter + 1,
                    changed[i_iter] / n, int(changed[i_iter]))
    else:
        logger.info("Exit due to max iteration limit.")                  # algorithm.py:74-75
    return labels


# audit / recruit / audit_pairs / recruit_pairs / cohesion / bin_report / witness / recruit_witness / nearest_bins /
# recruit_nearest_bins: up to this many neighbours the calls they have always made; beyond it (up to 64; the library
# refuses more) the chb_*_wide calls.  neighbor_sweep keeps refusing entries above 16: those go to neighbor_sweep_wide.
_TILED_MAX_NEIGHBORS = 16


@contextlib.contextmanager
def _resident(samples, metric, qp_solver):
    """How every function below starts: the reference's two refusals, before the context is touched; then the process-wide
    context with `samples` resident and `metric` selected for the length of the with statement."""
    if metric not in ("convex", "affine", "affine-qp"):
        raise NotImplementedError(f"Metric {metric} not implemented")  # hull_distance.py:108
    check_solver(qp_solver)                                              # solve_qp.py:132
    ctx = default_context()
    ctx.set_samples_cached(np.ascontiguousarray(samples, dtype=np.float64))
    with ctx.using_metric(metric):
        yield ctx


def recruit(
    samples: np.ndarray,
    labels: np.ndarray,
    rows: np.ndarray,
    num_clusters: int,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
    return_distances: bool = False,
):
    """Bins for `rows` that were NOT part of the fit (no counterpart in the reference, which drops the contigs under
    ContigLengthFilterBp before the fit: cli/features.py:60-64): for every row the step of algorithm.py:49-58 against
    the finished, frozen `labels` of `samples` -- per bin the `num_neighbors` nearest members, the distance to their
    hull, the strict-'>' argmin over the bins (-1 where no bin has a member).  Neither `samples` nor `labels` change.

    Returns `bins` [len(rows)] or, with return_distances, (bins, distances [len(rows), num_clusters])."""
    with _resident(samples, metric, qp_solver) as ctx:
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        score = ctx.recruit_rows_wide if int(num_neighbors) > _TILED_MAX_NEIGHBORS else ctx.recruit_rows
        bins, dist, _, _ = score(labels, int(num_clusters), int(num_neighbors), rows, want_dist=return_distances)
    return (bins, dist) if return_distances else bins


def audit(
    samples: np.ndarray,
    labels: np.ndarray,
    num_clusters: int,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
    rows: np.ndarray = None,
    return_distances: bool = False,
    groups: np.ndarray = None,
):
    """How well every contig sits in a finished labelling (no counterpart in the reference, which only logs "Exit due to
    max iteration limit": algorithm.py:74-75): for every sample in `rows` (indices into `samples`; None: all of them) the
    step of algorithm.py:49-58 against the frozen `labels` with that sample taken out of its own bin -- per bin the
    `num_neighbors` nearest other members, the distance to their hull, the strict-'>' argmin over the bins.  Seeds,
    unassigned rows and labellings that did not come from fit_cluster are scored alike.  Nothing changes.

    `groups` (one int64 per sample, negative: no group; `parent_groups` makes them from PARENT_NAME) turns leave-one-out
    into leave-group-out: every sample that shares the scored row's group id -- the sibling pieces preprocess.py:72-101
    cut from one parent contig -- is withheld from every bin as well, so a piece is no longer vouched for by its siblings.

    Returns (bins, min_dist, margin) -- the bin the row would choose now (-1 where no bin has another member), its hull
    distance, and the gap to the runner-up bin (+inf without one) -- and with return_distances also
    distances [len(rows), num_clusters]."""
    with _resident(samples, metric, qp_solver) as ctx:
        if int(num_neighbors) > _TILED_MAX_NEIGHBORS:
            bins, dist, mind, margin = ctx.audit_rows_wide(labels, int(num_clusters), int(num_neighbors), rows,
                                                           want_dist=return_distances, groups=groups)
        elif groups is None:
            bins, dist, mind, margin = ctx.audit_rows(labels, int(num_clusters), int(num_neighbors), rows,
                                                      want_dist=return_distances)
        else:
            bins, dist, mind, margin = ctx.audit_rows_grouped(labels, groups, int(num_clusters), int(num_neighbors), rows,
                                                              want_dist=return_distances)
    return (bins, mind, margin, dist) if return_distances else (bins, mind, margin)


def parent_groups(parent_names) -> np.ndarray:
    """Group ids for the `groups` argument of the audit calls from one name per sample -- features.csv's PARENT_NAME, under
    which preprocess.py:72-101 files the pieces `<parent>_S<i>` of a long contig: int64 codes by first occurrence, equal
    names give equal codes.  Every sample gets a group (a contig that was not cut is a group of one, which withholds
    nothing but the row itself)."""
    codes, out = {}, np.empty(len(parent_names), dtype=np.int64)
    for i, name in enumerate(parent_names):
        out[i] = codes.setdefault(name, len(codes))
    return out


@dataclasses.dataclass
class BinReport:
    """What bin_report returns: per (own bin a, bin b) pair of a labelling, over the scored rows of bin a --
    confusion[a, b] rows that would choose bin b now, unplaced[a] rows that would choose none, dcnt / dmin / dsum[a, b]
    count, minimum (+inf without one) and sum of their finite leave-one-out hull distances to bin b; n_skipped rows whose
    own label lies outside [0, num_clusters) and were not scored."""
    confusion: np.ndarray
    unplaced: np.ndarray
    dcnt: np.ndarray
    dmin: np.ndarray
    dsum: np.ndarray
    n_skipped: int

    @property
    def mean(self) -> np.ndarray:
        """dsum / dcnt: mean hull distance of bin a's rows to bin b; NaN where dcnt is 0."""
        out = np.full(self.dsum.shape, np.nan)
        np.divide(self.dsum, self.dcnt, out=out, where=self.dcnt > 0)
        return out

    def confused_pairs(self, min_share: float = 0.05):
        """[(a, b, share)] with a != b and share = confusion[a, b] / (bin a's scored rows, the unplaced ones included)
        >= min_share: bin a's rows that would rather sit in bin b.  Largest share first, then by (a, b)."""
        total = self.confusion.sum(axis=1) + self.unplaced
        pairs = []
        for a, b in zip(*np.nonzero(self.confusion)):
            share = self.confusion[a, b] / total[a]
            if a != b and share >= min_share:
                pairs.append((int(a), int(b), float(share)))
        return sorted(pairs, key=lambda t: (-t[2], t[0], t[1]))


def bin_report(
    samples: np.ndarray,
    labels: np.ndarray,
    num_clusters: int,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
    rows: np.ndarray = None,
    groups: np.ndarray = None,
) -> BinReport:
    """Which bins of a finished labelling bleed into each other (no counterpart in the reference): `audit` for the samples
    in `rows` (None: all of them), reduced on the device by each row's own label -- per bin pair how many rows of bin a
    would choose bin b now, and count / minimum / sum of their hull distances to it.  Only the num_clusters x num_clusters
    tables come back; rows without a label in [0, num_clusters) are not scored.  Nothing changes.
    With `groups` the tables are those of the leave-group-out audit (`audit(..., groups=groups)`)."""
    with _resident(samples, metric, qp_solver) as ctx:
        if int(num_neighbors) > _TILED_MAX_NEIGHBORS:
            return BinReport(*ctx.bin_report_wide(labels, int(num_clusters), int(num_neighbors), rows, groups=groups))
        if groups is None:
            return BinReport(*ctx.bin_report(labels, int(num_clusters), int(num_neighbors), rows))
        return BinReport(*ctx.bin_report_grouped(labels, groups, int(num_clusters), int(num_neighbors), rows))


@dataclasses.dataclass
class NeighborSweep:
    """What neighbor_sweep returns: `audit` of the same rows for every entry of `neighbors` -- bins / min_dist / margin
    [len(neighbors), len(rows)] (row j = audit with num_neighbors = neighbors[j]), `rows` the scored sample indices, `own`
    their labels in the audited labelling, `distances` [len(neighbors), len(rows), num_clusters] if asked for."""
    neighbors: np.ndarray
    rows: np.ndarray
    own: np.ndarray
    bins: np.ndarray
    min_dist: np.ndarray
    margin: np.ndarray
    num_clusters: int
    distances: np.ndarray = None

    @property
    def moved(self) -> np.ndarray:
        """Per entry of `neighbors`: the scored rows with a label in [0, num_clusters) whose audit bin is another one
        (no bin at all, -1, included)."""
        labelled = (self.own >= 0) & (self.own < self.num_clusters)
        return np.count_nonzero((self.bins != self.own[None, :]) & labelled[None, :], axis=1)

    @property
    def agreement(self) -> np.ndarray:
        """[len(neighbors), len(neighbors)]: the share of scored rows on which two entries choose the same bin (both
        choosing none counts as the same); 1 on the diagonal; NaN without a scored row."""
        nm, Q = self.bins.shape
        if Q == 0:
            return np.full((nm, nm), np.nan)
        return (self.bins[:, None, :] == self.bins[None, :, :]).sum(axis=2) / float(Q)

    def stable(self, min_margin: float = 0.0) -> np.ndarray:
        """Boolean per scored row: every entry of `neighbors` chooses the row's own label, with a margin above
        `min_margin` (+inf, no runner-up bin, is above any).  False for rows without a label in [0, num_clusters)."""
        labelled = (self.own >= 0) & (self.own < self.num_clusters)
        return labelled & np.all((self.bins == self.own[None, :]) & (self.margin > min_margin), axis=0)


def neighbor_sweep(
    samples: np.ndarray,
    labels: np.ndarray,
    num_clusters: int,
    neighbors=(1, 3, 5, 10, 15),
    metric: str = "convex",
    qp_solver: str = "quadprog",
    rows: np.ndarray = None,
    return_distances: bool = False,
    groups: np.ndarray = None,
) -> NeighborSweep:
    """Does a finished labelling hold up at other numbers of neighbours (no counterpart in the reference, whose default
    configuration says 5 and whose function default says 15)?  `audit` of the samples in `rows` (None: all of them) for
    every entry of `neighbors` (distinct values in 1 .. 16) at the cost of little more than the audit at the largest: one
    selection pass on the device serves the whole list, and each entry's result is bit for bit what `audit` returns for it.
    Nothing changes.  With `groups` every entry is `audit(..., groups=groups)`: leave-group-out.
    A list with entries above 16 (up to 64) goes to `neighbor_sweep_wide`."""
    with _resident(samples, metric, qp_solver) as ctx:
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        neighbors = np.ascontiguousarray(neighbors, dtype=np.int64)
        if groups is None:
            bins, dist, mind, margin = ctx.audit_rows_multi(labels, int(num_clusters), neighbors, rows,
                                                            want_dist=return_distances)
        else:
            bins, dist, mind, margin = ctx.audit_rows_multi_grouped(labels, groups, int(num_clusters), neighbors, rows,
                                                                    want_dist=return_distances)
    scored = np.arange(np.shape(samples)[0], dtype=np.int64) if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    return NeighborSweep(neighbors, scored, labels[scored], bins, mind, margin, int(num_clusters), dist)


def neighbor_sweep_wide(
    samples: np.ndarray,
    labels: np.ndarray,
    num_clusters: int,
    neighbors=(5, 15, 24, 32, 64),
    metric: str = "convex",
    qp_solver: str = "quadprog",
    rows: np.ndarray = None,
    return_distances: bool = False,
    groups: np.ndarray = None,
) -> NeighborSweep:
    """`neighbor_sweep` for a list whose entries go up to 64 (distinct values, at most 16 of them, any order, entries up to
    16 and above mixed), for a labelling fitted with more than 16 neighbours: one wide selection pass serves every entry
    above 16 and only the active-set solves repeat; each entry's result is bit for bit what `audit` returns for it.  A list
    without an entry above 16 is `neighbor_sweep`'s call.  Nothing changes.  With `groups` every entry is `audit(..., groups=groups)`."""
    with _resident(samples, metric, qp_solver) as ctx:
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        neighbors = np.ascontiguousarray(neighbors, dtype=np.int64)
        bins, dist, mind, margin = ctx.audit_rows_multi_wide(labels, int(num_clusters), neighbors, rows,
                                                             want_dist=return_distances, groups=groups)
    scored = np.arange(np.shape(samples)[0], dtype=np.int64) if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    return NeighborSweep(neighbors, scored, labels[scored], bins, mind, margin, int(num_clusters), dist)


def audit_pairs(
    samples: np.ndarray,
    labels: np.ndarray,
    rows: np.ndarray,
    bins: np.ndarray,
    num_clusters: int,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
    groups: np.ndarray = None,
) -> np.ndarray:
    """`audit`'s leave-one-out hull distances for a list of (row, bin) pairs instead of every bin of every row (no
    counterpart in the reference): entry p is bit for bit `audit(..., rows=rows, return_distances=True)[3][p, bins[p]]`,
    and only the members of the listed bins are streamed -- 64 pairs of a bin share one pass over it.  Pairs may repeat
    and come in any order.  Nothing changes.  With `groups` the entries are those of `audit(..., groups=groups)`.

    Returns distances [len(rows)]."""
    with _resident(samples, metric, qp_solver) as ctx:
        if int(num_neighbors) > _TILED_MAX_NEIGHBORS:
            return ctx.audit_pairs_wide(labels, int(num_clusters), int(num_neighbors), rows, bins, groups=groups)
        if groups is None:
            return ctx.audit_pairs(labels, int(num_clusters), int(num_neighbors), rows, bins)
        return ctx.audit_pairs_grouped(labels, groups, int(num_clusters), int(num_neighbors), rows, bins)


def recruit_pairs(
    samples: np.ndarray,
    labels: np.ndarray,
    new_rows: np.ndarray,
    row_of: np.ndarray,
    bins: np.ndarray,
    num_clusters: int,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
) -> np.ndarray:
    """`audit_pairs` for rows that are NOT samples: entry p is bit for bit
    `recruit(..., new_rows, return_distances=True)[1][row_of[p], bins[p]]`, the hull distance of new_rows[row_of[p]] to
    bin bins[p].  Nothing changes.

    Returns distances [len(row_of)]."""
    with _resident(samples, metric, qp_solver) as ctx:
        new_rows = np.ascontiguousarray(new_rows, dtype=np.float64)
        if int(num_neighbors) > _TILED_MAX_NEIGHBORS:
            return ctx.recruit_pairs_wide(labels, int(num_clusters), int(num_neighbors), new_rows, row_of, bins)
        return ctx.recruit_pairs(labels, int(num_clusters), int(num_neighbors), new_rows, row_of, bins)


def cohesion(
    samples: np.ndarray,
    labels: np.ndarray,
    num_clusters: int,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
    rows: np.ndarray = None,
    groups: np.ndarray = None,
) -> np.ndarray:
    """How well every contig sits in its OWN bin (no counterpart in the reference): for every sample in `rows` (indices
    into `samples`; None: all of them) the leave-one-out hull distance to the bin its label names -- by definition
    `audit(..., rows=rows, return_distances=True)[3][i, labels[rows[i]]]`, at about 1 / num_clusters of that call's cost,
    since only a row's own bin is streamed for it.  NaN where the row's label lies outside [0, num_clusters): such rows
    are not scored.  +inf where the row is its bin's only member.  Nothing changes.
    With `groups` (see `audit`) the row's whole group is withheld: how well a contig sits in its bin WITHOUT the other
    pieces of its own parent -- +inf where the bin holds nothing else.

    Returns distances [len(rows)]."""
    with _resident(samples, metric, qp_solver) as ctx:
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        rows = np.arange(np.shape(samples)[0], dtype=np.int64) if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        own = labels[rows]
        scored = (own >= 0) & (own < int(num_clusters))
        out = np.full(rows.shape[0], np.nan)
        if int(num_neighbors) > _TILED_MAX_NEIGHBORS:
            out[scored] = ctx.audit_pairs_wide(labels, int(num_clusters), int(num_neighbors), rows[scored], own[scored],
                                               groups=groups)
        elif groups is None:
            out[scored] = ctx.audit_pairs(labels, int(num_clusters), int(num_neighbors), rows[scored], own[scored])
        else:
            out[scored] = ctx.audit_pairs_grouped(labels, groups, int(num_clusters), int(num_neighbors), rows[scored],
                                                  own[scored])
    return out


def audit_pairs_sweep(
    samples: np.ndarray,
    labels: np.ndarray,
    rows: np.ndarray,
    bins: np.ndarray,
    num_clusters: int,
    neighbors=(1, 3, 5, 10, 15),
    metric: str = "convex",
    qp_solver: str = "quadprog",
    groups: np.ndarray = None,
) -> np.ndarray:
    """`audit_pairs` for every entry of `neighbors` (distinct values in 1 .. 64, at most 16 of them, any order, entries up
    to 16 and above mixed) at the cost of little more than the call at the largest: the listed bins' members are streamed
    once for the whole list, and row j is bit for bit `audit_pairs(..., num_neighbors=neighbors[j])`.  The sweep over each
    row's nearest bins only (`NearestBins.pairs`), where `neighbor_sweep`'s dense table is num_clusters times the work.
    Nothing changes.  With `groups` every entry is `audit_pairs(..., groups=groups)`.

    Returns distances [len(neighbors), len(rows)]."""
    with _resident(samples, metric, qp_solver) as ctx:
        neighbors = np.ascontiguousarray(neighbors, dtype=np.int64)
        return ctx.audit_pairs_multi(labels, int(num_clusters), neighbors, rows, bins, groups=groups)


def recruit_pairs_sweep(
    samples: np.ndarray,
    labels: np.ndarray,
    new_rows: np.ndarray,
    row_of: np.ndarray,
    bins: np.ndarray,
    num_clusters: int,
    neighbors=(1, 3, 5, 10, 15),
    metric: str = "convex",
    qp_solver: str = "quadprog",
) -> np.ndarray:
    """`audit_pairs_sweep` for rows that are NOT samples: row j is bit for bit
    `recruit_pairs(..., num_neighbors=neighbors[j])`.  Nothing is withheld and nothing changes.

    Returns distances [len(neighbors), len(row_of)]."""
    with _resident(samples, metric, qp_solver) as ctx:
        new_rows = np.ascontiguousarray(new_rows, dtype=np.float64)
        neighbors = np.ascontiguousarray(neighbors, dtype=np.int64)
        return ctx.recruit_pairs_multi(labels, int(num_clusters), neighbors, new_rows, row_of, bins)


def cohesion_sweep(
    samples: np.ndarray,
    labels: np.ndarray,
    num_clusters: int,
    neighbors=(1, 3, 5, 10, 15),
    metric: str = "convex",
    qp_solver: str = "quadprog",
    rows: np.ndarray = None,
    groups: np.ndarray = None,
) -> np.ndarray:
    """`cohesion` for every entry of `neighbors` (distinct values in 1 .. 64, at most 16 of them, any order): how well every
    contig sits in its own bin at each number of neighbours, the cheap instrument for choosing one (the reference's
    configuration says 5, its function default 15) -- one call that streams every bin's members once instead of one
    `cohesion` per entry.  Row j is bit for bit `cohesion(..., num_neighbors=neighbors[j])`; the columns of rows without a
    label in [0, num_clusters) are NaN.  Nothing changes.  With `groups` every entry is leave-group-out.

    Returns distances [len(neighbors), len(rows)]."""
    with _resident(samples, metric, qp_solver) as ctx:
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        neighbors = np.ascontiguousarray(neighbors, dtype=np.int64)
        rows = np.arange(np.shape(samples)[0], dtype=np.int64) if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        own = labels[rows]
        scored = (own >= 0) & (own < int(num_clusters))
        out = np.full((neighbors.shape[0], rows.shape[0]), np.nan)
        out[:, scored] = ctx.audit_pairs_multi(labels, int(num_clusters), neighbors, rows[scored], own[scored], groups=groups)
    return out


@dataclasses.dataclass
class Witness:
    """What `witness` / `recruit_witness` return: per scored (row, bin) pair the hull its distance was measured to.
    Plain numpy, nothing here touches the GPU.

    dist [P]: the pair's hull distance, bit for bit `audit_pairs` / `recruit_pairs`' entry (+inf: the bin had no member
    to offer).  neighbors [P, m]: the sample indices of the hull's vertices -- the bin's members nearest to the row, in
    (distance, index) order, after the call's withholding -- padded with -1 where the bin had fewer than m.
    neighbor_dist [P, m]: each vertex's Euclidean distance to the row (+inf padding).  weights [P, m]: each vertex's
    weight in the nearest point of the hull (0 padding): that point is sum_a weights[p, a] * samples[neighbors[p, a]].

    Under the convex metric the weights are >= 0 and sum to 1, and a zero weight means the vertex does not take part
    in the nearest point.  Under the affine metrics they sum to 1 and MAY BE NEGATIVE: the nearest point of the affine
    hull need not lie between the vertices, so a weight is a coordinate, not a share.  Where vertices are dependent --
    twins with equal coordinates, more vertices than the dimension allows -- the nearest point is unique but the weights
    are not: any optimal vector is a valid answer, and two pieces of software (or two numbers of neighbours) may spread
    the same point differently over the twins."""
    dist: np.ndarray
    neighbors: np.ndarray
    neighbor_dist: np.ndarray
    weights: np.ndarray

    @property
    def count(self) -> np.ndarray:
        """[P]: the number of vertices of each pair's hull (0: an empty bin, dist +inf)."""
        return np.count_nonzero(self.neighbors >= 0, axis=1)

    @property
    def support(self) -> np.ndarray:
        """[P, m] bool: the real vertices with a weight other than 0 -- the ones the nearest point is made of."""
        return (self.neighbors >= 0) & (self.weights != 0)

    def nearest_point(self, samples: np.ndarray) -> np.ndarray:
        """[P, D]: the nearest point of each pair's hull, sum_a weights * samples[neighbors] with padding skipped
        (a row of zeros for a pair without vertices)."""
        samples = np.asarray(samples, dtype=np.float64)
        real = self.neighbors >= 0
        rows = np.where(real[:, :, None], samples[np.where(real, self.neighbors, 0)], 0.0)   # [P, m, D], padding zeroed
        return np.einsum("pa,pad->pd", np.where(real, self.weights, 0.0), rows)

    def residual_by_block(self, samples: np.ndarray, points: np.ndarray, blocks) -> np.ndarray:
        """[P, len(blocks)]: the squared residual ||points - nearest_point||^2 summed over each column range
        (begin, end) of `blocks` -- where a pair's distance comes from: composition (the k-mer blocks of features.csv)
        or abundance (its coverage block).  `points` [P, D] are the scored rows, samples[rows] or new_rows[row_of].
        Over a partition of the columns the blocks sum to dist**2 up to rounding.  NaN for a pair without vertices."""
        points = np.asarray(points, dtype=np.float64)
        r2 = (points - self.nearest_point(samples)) ** 2
        out = np.stack([r2[:, int(b):int(e)].sum(axis=1) for b, e in blocks], axis=1) if len(blocks) \
            else np.zeros((r2.shape[0], 0))
        out[self.count == 0] = np.nan
        return out


def witness(
    samples: np.ndarray,
    labels: np.ndarray,
    rows: np.ndarray,
    bins: np.ndarray,
    num_clusters: int,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
    groups: np.ndarray = None,
) -> Witness:
    """Which contigs vouch for a (row, bin) pair (no counterpart in the reference): `audit_pairs` on the same arguments,
    returning with every distance the members of the bin that form the hull it was measured to, their distances to the
    row and their weights in the hull's nearest point -- see `Witness` for what the weights mean under the affine metric
    and why they are not unique among twins.  With `groups` the hulls are leave-group-out, as in `audit_pairs`.
    Nothing changes."""
    with _resident(samples, metric, qp_solver) as ctx:
        score = ctx.audit_pairs_witness_wide if int(num_neighbors) > _TILED_MAX_NEIGHBORS else ctx.audit_pairs_witness
        return Witness(*score(labels, int(num_clusters), int(num_neighbors), rows, bins, groups=groups))


def recruit_witness(
    samples: np.ndarray,
    labels: np.ndarray,
    new_rows: np.ndarray,
    row_of: np.ndarray,
    bins: np.ndarray,
    num_clusters: int,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
) -> Witness:
    """`witness` for rows that are NOT samples: `recruit_pairs` on the same arguments together with the hull each
    distance was measured to.  Nothing is withheld: a new row equal to a sample has that sample as a vertex at distance
    0.  The weights' meaning under the affine metric and their non-uniqueness among twins are `Witness`'s."""
    with _resident(samples, metric, qp_solver) as ctx:
        new_rows = np.ascontiguousarray(new_rows, dtype=np.float64)
        score = ctx.recruit_pairs_witness_wide if int(num_neighbors) > _TILED_MAX_NEIGHBORS else ctx.recruit_pairs_witness
        return Witness(*score(labels, int(num_clusters), int(num_neighbors), new_rows, row_of, bins))


@dataclasses.dataclass
class NearestBins:
    """What `nearest_bins` / `recruit_nearest_bins` return: per scored row its k nearest bins, nearest first.  Plain numpy,
    nothing here touches the GPU.

    bins [n, k], dist [n, k]: the finite entries of the row's distances to every bin (`audit` / `recruit` with
    return_distances, bit for bit) in (distance, bin) order -- exact ties go to the lower bin.  A row with fewer than k
    bins at a finite distance is padded with bin -1 at distance +inf.  Slot 0 is the bin `audit` / `recruit` choose."""
    bins: np.ndarray
    dist: np.ndarray

    @property
    def count(self) -> np.ndarray:
        """[n]: the real slots of each row (0: no bin has a member to offer)."""
        return np.count_nonzero(self.bins >= 0, axis=1)

    @property
    def margin(self) -> np.ndarray:
        """[n]: dist[:, 1] - dist[:, 0], `audit`'s margin bit for bit; +inf for a row without a runner-up."""
        if self.bins.shape[1] < 2:
            raise ValueError("the margin needs the runner-up: ask for k >= 2")
        out = np.full(self.bins.shape[0], np.inf)
        real = self.bins[:, 1] >= 0
        out[real] = self.dist[real, 1] - self.dist[real, 0]
        return out

    def ambiguous(self, tol: float, relative: bool = False) -> np.ndarray:
        """[n] bool: the rows whose runner-up is within `tol` of their nearest bin (relative: within tol times the nearest
        bin's distance).  A row without a runner-up is never ambiguous."""
        margin = self.margin
        real = self.bins[:, 1] >= 0
        out = np.zeros(self.bins.shape[0], dtype=bool)
        out[real] = margin[real] <= (tol * self.dist[real, 0] if relative else tol)
        return out

    def pairs(self, ranks=(0, 1), mask=None):
        """(positions, bins): the real entries of the slots `ranks` of the rows `mask` selects (bool [n]; None: all), row
        by row -- the two lists `audit_pairs` / `witness` take once positions are turned into sample indices
        (rows[positions]; positions themselves for rows=None), and `recruit_pairs` / `recruit_witness` take as they are
        (row_of = positions).  `audit_pairs_sweep` / `recruit_pairs_sweep` take the same two lists with a list of
        num_neighbors: the way to sweep only a row's nearest bins instead of `neighbor_sweep`'s every bin."""
        ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
        take = self.bins[:, ranks] >= 0
        if mask is not None:
            take &= np.asarray(mask, dtype=bool)[:, None]
        pos, slot = np.nonzero(take)
        return pos.astype(np.int64), self.bins[pos, ranks[slot]].astype(np.int64)


def nearest_bins(
    samples: np.ndarray,
    labels: np.ndarray,
    num_clusters: int,
    k: int = 3,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
    rows: np.ndarray = None,
    groups: np.ndarray = None,
) -> NearestBins:
    """Which bins come next (no counterpart in the reference): `audit` on the same arguments, returning per row the k
    nearest bins with their leave-one-out hull distances instead of the nearest alone -- ranked on the device, so the
    len(rows) x num_clusters table never crosses to the host.  With `groups` the distances are leave-group-out.
    Nothing changes."""
    with _resident(samples, metric, qp_solver) as ctx:
        score = ctx.audit_rows_nearest_wide if int(num_neighbors) > _TILED_MAX_NEIGHBORS else ctx.audit_rows_nearest
        return NearestBins(*score(labels, int(num_clusters), int(num_neighbors), int(k), rows, groups=groups))


def recruit_nearest_bins(
    samples: np.ndarray,
    labels: np.ndarray,
    rows: np.ndarray,
    num_clusters: int,
    k: int = 3,
    num_neighbors: int = 15,
    metric: str = "convex",
    qp_solver: str = "quadprog",
) -> NearestBins:
    """`nearest_bins` for `rows` that are NOT samples: `recruit` on the same arguments, returning per row the k nearest
    bins with their hull distances.  Nothing is withheld and nothing changes."""
    with _resident(samples, metric, qp_solver) as ctx:
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        score = ctx.recruit_rows_nearest_wide if int(num_neighbors) > _TILED_MAX_NEIGHBORS else ctx.recruit_rows_nearest
        return NearestBins(*score(labels, int(num_clusters), int(num_neighbors), int(k), rows))
