"""A stepwise backend (same methods as chbin_amd._lib.Context) implemented with the CPU ORACLE.
Test infrastructure: lets the CPU suite exercise the speculative-batch / multi-rank control flow of
chbin_amd.distributed without a GPU, and states what one round of the stepwise ABI has to return
(tests/test_gpu_stepwise.py).  Never used by the product."""
import numpy as np

from oracle import oracle as O


class OracleBackend:
    def __init__(self, metric="convex", want_all=False, threads=1):
        """metric: what O.sweep evaluates ("convex" / "affine"); want_all: keep every bin's distance of the
        last round in self.all_dist[K, B] (NaN where the round did not evaluate), for the runner-up margin;
        threads: a round's positions are independent of each other by definition, and the oracle library is
        re-entrant and called without the GIL, so they may be evaluated by several host threads."""
        self.metric, self.want_all, self.threads = metric, bool(want_all), int(threads)
        self.all_dist = None

    def set_samples(self, X):
        self.X = np.ascontiguousarray(X, dtype=np.float64)

    def fit_begin(self, B, initial, m):
        self.B, self.m = int(B), int(m)
        self.labels = np.ascontiguousarray(initial, dtype=np.int64).copy()

    def fit_labels(self):
        return self.labels.copy()

    def batch_begin(self, perm_slice, q_lo, q_hi):
        self.sl = np.asarray(perm_slice, dtype=np.int64).copy()
        self.lo, self.hi = int(q_lo), int(q_hi)
        self.lab_old = self.labels[self.sl].copy()

    def batch_guess(self, guess):
        """The header's list rule: a labelled position keeps its label, an unlabelled one gets the bin of its
        nearest member outside the batch (cdist distance, ties to the lower bin), -1 if no bin has one."""
        outside = self.labels.copy()
        outside[self.sl] = -1
        for pos in range(self.lo, self.hi):
            g = self.lab_old[pos]
            if g < 0:
                row = O.cdist_row(self.X, self.sl[pos])
                best = np.inf
                for c in range(self.B):
                    members = np.flatnonzero(outside == c)
                    if members.size and row[members].min() < best:
                        best, g = row[members].min(), c
            guess[pos] = g

    def batch_round(self, lab_prev, active, lab_new, min_dist=None):
        lab_prev = np.asarray(lab_prev, dtype=np.int64)
        if self.want_all:
            self.all_dist = np.full((len(self.sl), self.B), np.nan)

        def visit(pos):
            # the label state the sequential loop would see when it visits position `pos`:
            # earlier batch members carry their (speculative) new label, later ones their old one
            tmp = self.labels.copy()
            tmp[self.sl[:pos]] = lab_prev[:pos]
            tmp[self.sl[pos:]] = self.lab_old[pos:]
            j = self.sl[pos]
            res = O.sweep(self.X, self.B, tmp, np.array([j]), self.m, want_all=self.want_all, metric=self.metric)
            out, md = res[0], res[1]
            lab_new[pos] = out[j]
            if min_dist is not None:
                min_dist[pos] = md[0]
            if self.want_all:
                self.all_dist[pos] = res[2][0]

        todo = range(max(self.lo, int(active)), self.hi)
        if self.threads > 1 and len(todo) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(self.threads) as pool:
                list(pool.map(visit, todo))
        else:
            for pos in todo:
                visit(pos)

    def batch_commit(self, final):
        self.labels[self.sl] = np.asarray(final, dtype=np.int64)


_REPLAY_CACHE = {}


def oracle_fit_replay(O, X, B, initial, perms, m, iters, key=None):
    """The oracle's whole fit as a replay of its own sweeps (algorithm.py:43-76: sweep, count the changed labels, stop
    after the first sweep that changes nothing): one pass gives what `O.fit_cluster` returns AND the winning hull
    distances of the last sweep, which the GPU tests used to obtain by running the fit twice.  `key` caches the result
    for the process (the world-2 and world-3 runs of tests/test_gpu_world2.py share their cases).
    Returns (labels, sweeps run, changed per sweep, winning distances of the last sweep indexed like perms[its - 1])."""
    import numpy as np
    if key is not None and key in _REPLAY_CACHE:
        return _REPLAY_CACHE[key]
    labels = np.asarray(initial, dtype=np.int64).copy()
    changed, md, its = [], None, 0
    for it in range(iters):
        new, md = O.sweep(X, B, labels, perms[it], m)
        diff = int((new != labels).sum())
        changed.append(diff)
        labels = new
        its = it + 1
        if diff == 0:
            break
    out = (labels, its, np.asarray(changed, dtype=np.int64), md)
    if key is not None:
        _REPLAY_CACHE[key] = out
    return out
