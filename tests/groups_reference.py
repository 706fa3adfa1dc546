"""Leave-group-out audit (chb_*_grouped): the numpy statement of the withheld set and the data set of the GPU tests.

For a scored resident row r the grouped calls withhold
    W(r) = {r} + {p : groups[p] >= 0 and groups[p] == groups[r]}
from the candidates of every bin; a negative id means "no group" and never equals anything, itself included.  The calls
are defined by the ungrouped ones: the result for r is what the ungrouped call returns for r on the labels in which W(r)
is set to -1 (labels_without)."""
import functools

import numpy as np

N, D, B = 640, 20, 4
BIG, ALL_OF_BIN, STARVER, TWINS = 2 ** 40 + 3, 2 ** 62, 7, 0   # the ids of the groups with a purpose (group_data)
SMALL_BIN, STARVED_BIN = 3, 2


def withheld(groups, r):
    """W(r): the sorted sample indices withheld when row r is scored."""
    groups = np.asarray(groups)
    w = np.zeros(len(groups), dtype=bool)
    w[r] = True
    if groups[r] >= 0:
        w |= groups == groups[r]
    return np.flatnonzero(w)


def labels_without(labels, groups, r):
    """The labels of the ungrouped call that defines row r's grouped result: W(r) set to -1."""
    out = np.array(labels, dtype=np.int64)
    out[withheld(groups, r)] = -1
    return out


@functools.lru_cache(maxsize=None)
def group_data():
    """(X, labels, groups) of the GPU tests, read-only and deterministic.  N = 640 rows of D = 20 in B = 4 bins:
    bins 0 and 1 hold about 290 members each, bin 2 nine, bin 3 six; about 40 rows carry -1 or an out-of-range label.

    groups, dealt out over a random permutation of the rows so that neighbouring rows -- the four rows of a thread, the
    64 of a query tile, the 64 of a member tile -- mix groups and ungrouped rows:
      BIG (2^40 + 3)     70 members, 40 of bin 0 and 30 of bin 1: more than one member tile, two bins
      ALL_OF_BIN (2^62)  every member of bin 3, and two rows of bin 0: its rows read +inf for bin 3
      STARVER (7)        six of bin 2's nine members: three are left, fewer than m = 5
      TWINS (0)          two rows with equal coordinates (bin 0) and a third row of bin 1; a third twin sits outside in a
                         group of its own (bin 0): it stays a candidate at distance 0
      sizes 1, 2 and 4   eight groups each of sizes 1 and 2, groups of four for the rest; some members carry -1 labels
      negative ids       about a third of the rows: -1, -2, -5, -2^40, which must not be treated as groups"""
    from chbin_amd import synth
    X, _, true = synth.make_synthetic(N, D, B, seed=N + D + B, sigma=6e-3, mix=0.5)
    rng = np.random.default_rng(11)
    labels = true.copy()
    # bins 2 and 3 shrink to nine and six members, the others' rows go to bins 0 and 1
    for b, keep in ((STARVED_BIN, 9), (SMALL_BIN, 6)):
        rest = np.flatnonzero(labels == b)[keep:]
        labels[rest] = np.arange(len(rest)) % 2
    groups = np.full(N, np.iinfo(np.int64).min, dtype=np.int64)   # (every entry is assigned below)
    free = np.ones(N, dtype=bool)

    def take(rows, gid):
        rows = np.asarray(rows)
        assert free[rows].all()
        groups[rows] = gid
        free[rows] = False

    def members(b, n):
        return rng.permutation(np.flatnonzero((labels == b) & free))[:n]

    take(members(SMALL_BIN, 6), ALL_OF_BIN)
    take(members(0, 2), ALL_OF_BIN)
    take(members(STARVED_BIN, 6), STARVER)
    take(np.concatenate([members(0, 40), members(1, 30)]), BIG)
    t = members(0, 3)
    X[t[1]] = X[t[0]]
    X[t[2]] = X[t[0]]
    take(np.concatenate([t[:2], members(1, 1)]), TWINS)
    take(t[2:], 123456789)
    # about 40 rows without a label, with and without a group: -1 and out-of-range values
    wild = rng.permutation(np.flatnonzero(free & (labels < 2)))[:40]
    labels[wild[:20]] = -1
    labels[wild[20:28]] = B
    labels[wild[28:34]] = -7
    labels[wild[34:]] = 2 ** 40
    # the rest: a third without a group, then groups of one, two and four
    rest = rng.permutation(np.flatnonzero(free))
    n_neg = N // 3
    groups[rest[:n_neg]] = np.array([-1, -2, -5, -2 ** 40])[np.arange(n_neg) % 4]
    free[rest[:n_neg]] = False
    rest = rest[n_neg:]
    gid, k = 1000, 0
    for size, count in ((1, 8), (2, 8), (4, len(rest))):
        for _ in range(count):
            if k >= len(rest):
                break
            take(rest[k:k + size], gid)
            k, gid = k + size, gid + 13
    assert not free.any()
    X = np.ascontiguousarray(X)
    for a in (X, labels, groups):
        a.setflags(write=False)
    return X, labels, groups
