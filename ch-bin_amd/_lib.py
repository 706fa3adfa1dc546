"""ctypes binding of libchbin_hip.so (C ABI: include/chbin_hip.h).

Fails loudly: if the shared library has not been built, or no MI355X is visible, every compute
call raises -- there is no CPU fallback in this package.
"""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CHBIN_LIB", os.path.join(_HERE, "libchbin_hip.so"))   # CHBIN_LIB: developer override

CHB_MAX_NEIGHBORS = 64

_lib = None
_lock = threading.Lock()
_ctx_by_device = {}


class ChbError(RuntimeError):
    pass


_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")

# every symbol include/chbin_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "chb_last_error": (C.c_char_p, []),
    "chb_version": (C.c_int, []),
    "chb_device_count": (C.c_int, []),
    "chb_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "chb_destroy": (C.c_int, [C.c_void_p]),
    "chb_set_metric": (C.c_int, [C.c_void_p, C.c_int]),
    "chb_set_samples": (C.c_int, [C.c_void_p, _f64p, C.c_int64, C.c_int64]),
    "chb_set_samples_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "chb_pairwise_distance": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _f64p]),
    "chb_topm_per_bin": (C.c_int, [C.c_void_p, _i64p, C.c_int64, C.c_int, _i64p, C.c_int64, _i64p,
                                   C.c_void_p, _i32p]),
    "chb_recruit_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_audit_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_audit_rows_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_recruit_rows_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_bin_report": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_audit_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_void_p]),
    "chb_recruit_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    # the leave-group-out forms: the ungrouped call's arguments with `groups` after `labels`
    "chb_audit_rows_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_audit_rows_multi_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_audit_pairs_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_void_p]),
    "chb_bin_report_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the pair calls with witnesses: dist_out and the three [P, m] arrays at the end (groups may be NULL)
    "chb_audit_pairs_witness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_recruit_pairs_witness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    # the k nearest bins per row: the dense calls' arguments with k after m and the two [Q, k] arrays (groups may be NULL)
    "chb_audit_rows_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_void_p]),
    "chb_recruit_rows_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                           C.c_int64, C.c_void_p, C.c_void_p]),
    # one entry point for every m up to 64: the dense and pair calls' arguments (groups may be NULL), the pair forms with
    # idx_out [P, m] at the end (may be NULL)
    "chb_audit_rows_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_recruit_rows_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_audit_pairs_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_void_p, C.c_void_p]),
    "chb_recruit_pairs_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    # nearest bins, bin report and witnesses for every m up to 64: the m <= 16 calls' arguments (groups may be NULL)
    "chb_audit_rows_nearest_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                              C.c_int64, C.c_void_p, C.c_void_p]),
    "chb_recruit_rows_nearest_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                                C.c_int64, C.c_void_p, C.c_void_p]),
    "chb_bin_report_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_audit_pairs_witness_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_recruit_pairs_witness_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    # the list calls for entries up to 64: the _multi calls' arguments (the audit with groups, which may be NULL)
    "chb_audit_rows_multi_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "chb_recruit_rows_multi_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the pair calls for a list with entries up to 64: ms / nm in m's place, dist_out [nm, P] (groups may be NULL)
    "chb_audit_pairs_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p]),
    "chb_recruit_pairs_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "chb_find_nearest_from_row": (C.c_int, [C.c_void_p, C.c_int64, _i64p, _f64p, C.c_int64, C.c_int,
                                            _i64p, C.POINTER(C.c_int32)]),
    "chb_hull_distance_batch": (C.c_int, [C.c_void_p, _i64p, C.c_int64, _i64p, C.c_int, _f64p,
                                          C.c_void_p]),
    "chb_hull_distance_points": (C.c_int, [C.c_void_p, _f64p, _f64p, C.c_int, C.c_int64,
                                           C.POINTER(C.c_double), C.c_void_p]),
    "chb_fit_cluster": (C.c_int, [C.c_void_p, C.c_int64, _i64p, _i64p, C.c_int64, C.c_int, C.c_int,
                                  C.c_int, _i64p, C.POINTER(C.c_int), _i64p, C.c_void_p]),
    "chb_fit_cluster_ex": (C.c_int, [C.c_void_p, C.c_int64, _i64p, _i64p, C.c_int64, C.c_int, C.c_int,
                                     C.c_int, _i64p, C.POINTER(C.c_int), _i64p, C.c_void_p, C.c_void_p]),
    "chb_fit_begin": (C.c_int, [C.c_void_p, C.c_int64, _i64p, C.c_int]),
    "chb_batch_begin": (C.c_int, [C.c_void_p, _i64p, C.c_int64, C.c_int64, C.c_int64]),
    "chb_batch_guess": (C.c_int, [C.c_void_p, _i64p]),
    "chb_batch_round": (C.c_int, [C.c_void_p, _i64p, C.c_int64, _i64p, C.c_void_p]),
    "chb_batch_commit": (C.c_int, [C.c_void_p, _i64p]),
    "chb_fit_labels": (C.c_int, [C.c_void_p, _i64p]),
    "chb_comm_unique_id": (C.c_int, [C.c_char_p]),
    "chb_comm_init": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int]),
    "chb_comm_destroy": (C.c_int, [C.c_void_p]),
    "chb_comm_init_hook": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "chb_bcast_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int]),
    "chb_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.POINTER(C.c_int)]),
    "chb_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "chb_profile_reset": (C.c_int, [C.c_void_p]),
    "chb_profile_get": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double),
                                  C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "chb_fit_stats": (C.c_int, [C.c_void_p, _i64p]),
    "chb_counter": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "chb_kmer_dim": (C.c_int, [C.c_int]),
    "chb_kmer_frequencies": (C.c_int, [C.c_void_p, C.c_char_p, _i64p, C.c_int64, C.c_int, _f64p, C.c_void_p]),
    "chb_kmer_profile_dim": (C.c_int, [_i32p, C.c_int]),
    "chb_kmer_profiles": (C.c_int, [C.c_void_p, C.c_char_p, _i64p, C.c_int64, _i32p, C.c_int, _f64p, C.c_void_p]),
    "chb_set_samples_from_sequences": (C.c_int, [C.c_void_p, C.c_char_p, _i64p, C.c_int64, _i32p, C.c_int, C.c_void_p,
                                                 C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
}


def load():
    """dlopen the HIP library and declare every entry point (no GPU needed for this)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ChbError(
                    f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` (or `make -C ch-bin_amd/csrc`). There is no CPU fallback.")
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        msg = load().chb_last_error()
        raise ChbError(f"libchbin_hip error {rc}: {msg.decode() if msg else '?'}")


class Context:
    """One libchbin_hip context (one GPU).  Holds the resident feature matrix."""

    def __init__(self, device=0):
        lib = load()
        if lib.chb_device_count() <= 0:
            raise ChbError("no HIP device visible: chbin_amd needs an MI355X (no CPU fallback)")
        self._h = C.c_void_p()
        check(lib.chb_create(int(device), C.byref(self._h)))
        self._lib = lib
        self.device = int(device)
        self.N = self.D = 0
        self._metric = "convex"

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.chb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    METRICS = {"convex": 0, "affine": 1, "affine-qp": 1}

    def set_metric(self, metric: str):
        if metric not in self.METRICS:
            raise NotImplementedError(f"Metric {metric} not implemented")   # hull_distance.py:108
        check(self._lib.chb_set_metric(self._h, self.METRICS[metric]))
        self._metric = metric

    def get_metric(self) -> str:
        return self._metric

    def using_metric(self, metric: str):
        """with ctx.using_metric("affine"): ... -- selects the metric and puts the caller's back afterwards
        (the mirror functions share one default context)."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            before = self._metric
            self.set_metric(metric)
            try:
                yield self
            finally:
                self.set_metric(before)
        return scope()

    # ---- samples
    def set_samples(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64)  # DataFrame.values may be F-ordered
        if X.ndim != 2:
            raise ValueError("samples must be a 2-D array")
        check(self._lib.chb_set_samples(self._h, X, X.shape[0], X.shape[1]))
        self.N, self.D = X.shape

    def set_samples_cached(self, X):
        """Kept for the callers' sake; it ALWAYS uploads.  (It used to skip the upload when the
        array's address / shape / dtype matched the previous call, but the mirror functions hand it
        `np.ascontiguousarray(...)` temporaries whose address is recycled by the next call, and a
        caller may also change `samples` in place: both made the GPU work on stale data.  An upload
        is milliseconds next to a sweep.)"""
        self.set_samples(X)

    def set_samples_device(self, ptr, N, D):
        check(self._lib.chb_set_samples_device(self._h, C.c_void_p(int(ptr)), int(N), int(D)))
        self.N, self.D = int(N), int(D)

    # ---- entry points
    def pairwise_distance(self, r0=0, r1=None):
        r1 = self.N if r1 is None else r1
        out = np.empty((r1 - r0, self.N), dtype=np.float64)
        check(self._lib.chb_pairwise_distance(self._h, int(r0), int(r1), out))
        return out

    def topm_per_bin(self, labels, B, m, query_idx):
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        q = np.ascontiguousarray(query_idx, dtype=np.int64)
        Q = q.shape[0]
        idx = np.empty((Q, B, m), dtype=np.int64)
        dist = np.empty((Q, B, m), dtype=np.float64)
        cnt = np.empty((Q, B), dtype=np.int32)
        check(self._lib.chb_topm_per_bin(self._h, labels, int(B), int(m), q, Q, idx,
                                         dist.ctypes.data, cnt))
        return idx, dist, cnt

    def _labels(self, labels):
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        if labels.shape != (self.N,):
            raise ValueError("labels must have one entry per resident sample")
        return labels

    def _row_indices(self, rows):
        """(row_idx argument, Q, the array behind it) of rows=None (every resident row in order) or a 1-D list of indices"""
        if rows is None:
            return None, self.N, None
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 1:
            raise ValueError("rows must be a 1-D array of sample indices")
        return rows.ctypes.data, rows.shape[0], rows

    def _groups(self, groups):
        """The int64 group id per resident sample of a leave-group-out call (negative: no group)."""
        groups = np.ascontiguousarray(groups, dtype=np.int64)
        if groups.shape != (self.N,):
            raise ValueError("groups must have one entry per resident sample")
        return groups

    # ---- row scoring: one private method per call shape (_score_rows, _bin_report, _score_pairs), parameterised by the C
    # symbol; the public methods below differ in the symbol they name and in where their arguments go
    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data

    @staticmethod
    def _new_rows(Y):
        """The rows of a recruit call: 2-D float64."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2:
            raise ValueError("rows must be a 2-D array")
        return Y

    def _frozen(self, symbol, labels, groups, slot):
        """(C function, [labels] or [labels, groups]) of a call against a frozen labelling, both checked.  groups go to a
        symbol that has a slot for them (`slot`: the _wide, _witness and _nearest audits, None passing NULL); given to any
        other symbol they select its _grouped form."""
        head = [self._labels(labels)]
        if groups is not None:
            head.append(self._groups(groups))
            if not slot:
                symbol += "_grouped"
        elif slot:
            head.append(None)
        return getattr(self._lib, symbol), head

    @staticmethod
    def _dense_arrays(lead, Q, B, want_dist):
        """bins [*lead, Q], dist [*lead, Q, B] or None, min_dist [*lead, Q], margin [*lead, Q] of a dense call"""
        return (np.empty(lead + (Q,), dtype=np.int64), np.empty(lead + (Q, int(B)), dtype=np.float64) if want_dist else None,
                np.empty(lead + (Q,), dtype=np.float64), np.empty(lead + (Q,), dtype=np.float64))

    @staticmethod
    def _nearest_arrays(Q, k):
        """bins [Q, k] and dist [Q, k] of a nearest-bins call (refused calls write nothing: k as given, at least 0)"""
        k = max(int(k), 0)
        return np.empty((Q, k), dtype=np.int64), np.empty((Q, k), dtype=np.float64)

    def _score_rows(self, symbol, labels, B, want_dist, m=None, ms=None, k=None, rows=None, Y=None, groups=None, slot=False):
        """The dense calls: `symbol` for one m, of the new rows Y or the resident rows `rows`, or with a list `ms` its _multi
        form, whose outputs carry a leading axis of len(ms); with `groups` the audit's leave-group-out form (_frozen).
        Returns (bins, dist or None, min_dist, margin), or with `k`, a _nearest symbol, (bins [Q, k], dist [Q, k])."""
        if groups is not None and Y is not None:
            raise ValueError("groups belong to resident samples: rows that are not samples have no siblings to withhold")
        if ms is not None:
            ms = np.ascontiguousarray(ms, dtype=np.intc)
            if ms.ndim != 1:
                raise ValueError("ms must be a 1-D list of neighbour counts")
        if Y is not None:
            Y = self._new_rows(Y)
        fn, head = self._frozen(symbol, labels, groups, slot)
        if Y is not None:
            source = (Y.ctypes.data, *Y.shape)
        else:
            *source, rows = self._row_indices(rows)
        Q = source[1]
        neighbours = (int(m),) if ms is None else (ms.ctypes.data, ms.shape[0])
        if k is None:
            out = self._dense_arrays(() if ms is None else ms.shape, Q, B, want_dist)
        else:
            neighbours, out = neighbours + (int(k),), self._nearest_arrays(Q, k)
        check(fn(self._h, *map(self._ptr, head), int(B), *neighbours, *source, *map(self._ptr, out)))
        return out

    def recruit_rows(self, labels, B, m, Y, want_dist=True):
        """chb_recruit_rows: hull distance of the NEW rows Y (not samples) to every bin of the frozen `labels`.
        Returns (bins [Q], dist [Q, B] or None, min_dist [Q], margin [Q])."""
        return self._score_rows("chb_recruit_rows", labels, B, want_dist, m=m, Y=Y)

    def audit_rows(self, labels, B, m, rows=None, want_dist=True):
        """chb_audit_rows: leave-one-out hull distance of the RESIDENT rows `rows` (sample indices, repeats allowed; None:
        every row in order) to every bin of the frozen `labels`; a row is withheld from its own bin's candidates.
        Returns (bins [Q], dist [Q, B] or None, min_dist [Q], margin [Q])."""
        return self._score_rows("chb_audit_rows", labels, B, want_dist, m=m, rows=rows)

    def audit_rows_multi(self, labels, B, ms, rows=None, want_dist=True):
        """chb_audit_rows_multi: audit_rows for every m of the list `ms` (distinct values in 1 .. 16, at most 16 of them,
        any order) from one selection pass; slice j of every result is bit for bit audit_rows(labels, B, ms[j], rows).
        Returns (bins [nm, Q], dist [nm, Q, B] or None, min_dist [nm, Q], margin [nm, Q])."""
        return self._score_rows("chb_audit_rows_multi", labels, B, want_dist, ms=ms, rows=rows)

    def audit_rows_grouped(self, labels, groups, B, m, rows=None, want_dist=True):
        """chb_audit_rows_grouped: audit_rows with every sample that shares the scored row's group id withheld as well
        (leave-group-out; `groups` int64 per resident sample, negative: no group) -- for a row of group g bit for bit
        audit_rows on `labels` with g's members set to -1.  Returns what audit_rows returns."""
        return self._score_rows("chb_audit_rows", labels, B, want_dist, m=m, rows=rows, groups=groups)

    def audit_rows_multi_grouped(self, labels, groups, B, ms, rows=None, want_dist=True):
        """chb_audit_rows_multi_grouped: audit_rows_grouped for every m of the list `ms` from one selection pass."""
        return self._score_rows("chb_audit_rows_multi", labels, B, want_dist, ms=ms, rows=rows, groups=groups)

    def recruit_rows_multi(self, labels, B, ms, Y, want_dist=True):
        """chb_recruit_rows_multi: recruit_rows for every m of the list `ms` from one selection pass; slice j of every
        result is bit for bit recruit_rows(labels, B, ms[j], Y).
        Returns (bins [nm, Q], dist [nm, Q, B] or None, min_dist [nm, Q], margin [nm, Q])."""
        return self._score_rows("chb_recruit_rows_multi", labels, B, want_dist, ms=ms, Y=Y)

    def _bin_report(self, symbol, labels, B, m, rows, groups, slot):
        """The report calls: `symbol` (with `groups` its leave-group-out form: _frozen) and its five tables."""
        fn, head = self._frozen(symbol, labels, groups, slot)
        row_idx, Q, rows = self._row_indices(rows)
        B = int(B)
        nb = max(B, 0) if B <= 8192 else 0   # (beyond the limit the call is refused before it writes anything)
        tables = (np.empty((nb, nb), dtype=np.int64), np.empty(nb, dtype=np.int64), np.empty((nb, nb), dtype=np.int64),
                  np.empty((nb, nb), dtype=np.float64), np.empty((nb, nb), dtype=np.float64))
        skipped = C.c_int64(0)
        check(fn(self._h, *map(self._ptr, head), B, int(m), row_idx, Q, *map(self._ptr, tables), C.addressof(skipped)))
        return (*tables, int(skipped.value))

    def bin_report(self, labels, B, m, rows=None, groups=None):
        """chb_bin_report: chb_audit_rows' answer for the RESIDENT rows `rows` (None: every row in order) summed up on the
        device per (own bin a, bin b) pair; rows whose own label lies outside [0, B) are not scored.  With `groups`
        chb_bin_report_grouped: the same tables of chb_audit_rows_grouped's answer.
        Returns (confusion [B, B], unplaced [B], dcnt [B, B], dmin [B, B], dsum [B, B], n_skipped)."""
        return self._bin_report("chb_bin_report", labels, B, m, rows, groups, slot=False)

    def bin_report_grouped(self, labels, groups, B, m, rows=None):
        """chb_bin_report_grouped: bin_report of the leave-group-out distances (audit_rows_grouped)."""
        return self.bin_report(labels, B, m, rows, groups=groups)

    @staticmethod
    def _pair_lists(rows, bins, rows_name):
        """The two int64 lists of a pair call, one entry per pair."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        bins = np.ascontiguousarray(bins, dtype=np.int64)
        if rows.ndim != 1 or bins.ndim != 1:
            raise ValueError(f"{rows_name} and bins must be 1-D arrays")
        if rows.shape != bins.shape:
            raise ValueError(f"{rows_name} and bins must have one entry per pair: {rows.shape[0]} and {bins.shape[0]}")
        return rows, bins

    def _score_pairs(self, symbol, labels, B, m, rows, bins, Y=None, groups=None, slot=False, idx=None, witness=False,
                     ms=None):
        """The pair calls: `symbol` for the pairs (rows[p], bins[p]) of resident rows or, with Y, of rows of Y (`rows` is
        then row_of); with `groups` the audit's leave-group-out form (_frozen).  Returns dist [P]; for a symbol with an
        idx_out (`idx` not None: whether it is wanted, else it is passed NULL) dist or (dist, idx [P, m]); for a `witness`
        symbol (dist, neighbors, neighbor_dist, weights), the last three [P, m]; with a list `ms` in m's place, a _multi
        symbol, dist [len(ms), P].
        (A refused call writes nothing: the [P, m] arrays take m as given, at least 0.)"""
        rows, bins = self._pair_lists(rows, bins, "rows" if Y is None else "row_of")
        if ms is not None:
            ms = np.ascontiguousarray(ms, dtype=np.intc)
            if ms.ndim != 1:
                raise ValueError("ms must be a 1-D list of neighbour counts")
        if Y is not None:
            Y = self._new_rows(Y)
        fn, head = self._frozen(symbol, labels, groups, slot)
        P = rows.shape[0]
        source = () if Y is None else (Y.ctypes.data, *Y.shape)
        if ms is not None:
            out = np.empty(ms.shape + (P,), dtype=np.float64)
            check(fn(self._h, *map(self._ptr, head), int(B), ms.ctypes.data, ms.shape[0], *source, rows.ctypes.data,
                     bins.ctypes.data, P, out.ctypes.data))
            return out
        m_out = max(int(m), 0)
        out = [np.empty(P, dtype=np.float64)]
        if witness:
            out += [np.empty((P, m_out), dtype=np.int64), np.empty((P, m_out), dtype=np.float64),
                    np.empty((P, m_out), dtype=np.float64)]
        elif idx is not None:
            out.append(np.empty((P, m_out), dtype=np.int64) if idx else None)
        check(fn(self._h, *map(self._ptr, head), int(B), int(m), *source, rows.ctypes.data, bins.ctypes.data, P,
                 *map(self._ptr, out)))
        return tuple(out) if witness or idx else out[0]

    def audit_pairs(self, labels, B, m, rows, bins, groups=None):
        """chb_audit_pairs: dist [P], entry p bit for bit audit_rows(labels, B, m, rows)[1][p, bins[p]] -- the leave-one-out
        hull distance of the RESIDENT row rows[p] to bin bins[p] -- at the cost of the listed pairs only.  With `groups`
        chb_audit_pairs_grouped: the same entries of audit_rows_grouped."""
        return self._score_pairs("chb_audit_pairs", labels, B, m, rows, bins, groups=groups)

    def audit_pairs_grouped(self, labels, groups, B, m, rows, bins):
        """chb_audit_pairs_grouped: audit_pairs of the leave-group-out distances (audit_rows_grouped)."""
        return self.audit_pairs(labels, B, m, rows, bins, groups=groups)

    def recruit_pairs(self, labels, B, m, Y, row_of, bins):
        """chb_recruit_pairs: dist [P], entry p bit for bit recruit_rows(labels, B, m, Y)[1][row_of[p], bins[p]] -- the hull
        distance of the NEW row Y[row_of[p]] to bin bins[p]."""
        return self._score_pairs("chb_recruit_pairs", labels, B, m, row_of, bins, Y=Y)

    def audit_pairs_witness(self, labels, B, m, rows, bins, groups=None):
        """chb_audit_pairs_witness: audit_pairs (with `groups` audit_pairs_grouped) together with the hull each distance
        was measured to.  Returns (dist [P], neighbors [P, m], neighbor_dist [P, m], weights [P, m]): dist bit for bit
        the plain call's; per pair the selected members' sample indices in the kernel's list order ((distance, index)
        ascending; -1 padding), their distances to the row (+inf padding) and their weights in the hull's nearest point
        under the context's metric (0 padding; not unique where vertices are dependent)."""
        return self._score_pairs("chb_audit_pairs_witness", labels, B, m, rows, bins, groups=groups, slot=True, witness=True)

    def recruit_pairs_witness(self, labels, B, m, Y, row_of, bins):
        """chb_recruit_pairs_witness: recruit_pairs together with the hull each distance was measured to; returns what
        audit_pairs_witness returns, for the NEW rows Y[row_of[p]] (nothing is withheld)."""
        return self._score_pairs("chb_recruit_pairs_witness", labels, B, m, row_of, bins, Y=Y, witness=True)

    def audit_rows_nearest(self, labels, B, m, k, rows=None, groups=None):
        """chb_audit_rows_nearest: the k nearest bins of every RESIDENT row in `rows` (None: every row in order), ranked on
        the device: the finite entries of audit_rows' (with `groups` audit_rows_grouped's) dist row in (distance, bin)
        order, bit for bit.  Returns (bins [Q, k], dist [Q, k]); slots past the number of finite entries hold -1 / +inf."""
        return self._score_rows("chb_audit_rows_nearest", labels, B, None, m=m, k=k, rows=rows, groups=groups, slot=True)

    def recruit_rows_nearest(self, labels, B, m, k, Y):
        """chb_recruit_rows_nearest: audit_rows_nearest for the NEW rows Y (nothing is withheld), ranked from
        recruit_rows' dist rows.  Returns (bins [Q, k], dist [Q, k])."""
        return self._score_rows("chb_recruit_rows_nearest", labels, B, None, m=m, k=k, Y=Y)

    def audit_rows_wide(self, labels, B, m, rows=None, want_dist=True, groups=None):
        """chb_audit_rows_wide: audit_rows (with `groups` audit_rows_grouped) for any m in 1 .. 64 -- m <= 16 forwards to
        those calls bit for bit, 16 < m <= 64 runs the wide kernels.  Returns what audit_rows returns."""
        return self._score_rows("chb_audit_rows_wide", labels, B, want_dist, m=m, rows=rows, groups=groups, slot=True)

    def recruit_rows_wide(self, labels, B, m, Y, want_dist=True):
        """chb_recruit_rows_wide: recruit_rows for any m in 1 .. 64.  Returns what recruit_rows returns."""
        return self._score_rows("chb_recruit_rows_wide", labels, B, want_dist, m=m, Y=Y)

    def audit_rows_multi_wide(self, labels, B, ms, rows=None, want_dist=True, groups=None):
        """chb_audit_rows_multi_wide: audit_rows_wide for every m of the list `ms` (distinct values in 1 .. 64, at most 16
        of them, any order) from one wide selection pass for all entries above 16; slice j of every result is bit for bit
        audit_rows_wide(labels, B, ms[j], rows, groups=groups).  A list without an entry above 16 forwards to
        audit_rows_multi / audit_rows_multi_grouped.  Returns what audit_rows_multi returns."""
        return self._score_rows("chb_audit_rows_multi_wide", labels, B, want_dist, ms=ms, rows=rows, groups=groups, slot=True)

    def recruit_rows_multi_wide(self, labels, B, ms, Y, want_dist=True):
        """chb_recruit_rows_multi_wide: recruit_rows_wide for every m of the list `ms` (entries up to 64); slice j of every
        result is bit for bit recruit_rows_wide(labels, B, ms[j], Y).  Returns what recruit_rows_multi returns."""
        return self._score_rows("chb_recruit_rows_multi_wide", labels, B, want_dist, ms=ms, Y=Y)

    def audit_pairs_wide(self, labels, B, m, rows, bins, groups=None, want_idx=False):
        """chb_audit_pairs_wide: audit_pairs (with `groups` audit_pairs_grouped) for any m in 1 .. 64; entry p is bit for
        bit audit_rows_wide(labels, B, m, rows, groups=groups)[1][p, bins[p]].  Returns dist [P], or with want_idx
        (dist, idx [P, m]): per pair the selected members' sample indices in (distance, index) order, -1 padded -- what
        topm_per_bin returns for the row."""
        return self._score_pairs("chb_audit_pairs_wide", labels, B, m, rows, bins, groups=groups, slot=True, idx=bool(want_idx))

    def recruit_pairs_wide(self, labels, B, m, Y, row_of, bins, want_idx=False):
        """chb_recruit_pairs_wide: recruit_pairs for any m in 1 .. 64; entry p is bit for bit
        recruit_rows_wide(labels, B, m, Y)[1][row_of[p], bins[p]].  Returns dist [P] or, with want_idx, (dist, idx [P, m])."""
        return self._score_pairs("chb_recruit_pairs_wide", labels, B, m, row_of, bins, Y=Y, idx=bool(want_idx))

    def audit_pairs_multi(self, labels, B, ms, rows, bins, groups=None):
        """chb_audit_pairs_multi: audit_pairs_wide for every m of the list `ms` (distinct values in 1 .. 64, at most 16 of
        them, any order, entries up to 16 and above mixed) from one selection pass per kernel; row j of the result is bit
        for bit audit_pairs_wide(labels, B, ms[j], rows, bins, groups=groups).  Returns dist [nm, P]."""
        return self._score_pairs("chb_audit_pairs_multi", labels, B, None, rows, bins, groups=groups, slot=True, ms=ms)

    def recruit_pairs_multi(self, labels, B, ms, Y, row_of, bins):
        """chb_recruit_pairs_multi: recruit_pairs_wide for every m of the list `ms` (entries up to 64); row j of the result
        is bit for bit recruit_pairs_wide(labels, B, ms[j], Y, row_of, bins).  Returns dist [nm, P]."""
        return self._score_pairs("chb_recruit_pairs_multi", labels, B, None, row_of, bins, Y=Y, ms=ms)

    def audit_rows_nearest_wide(self, labels, B, m, k, rows=None, groups=None):
        """chb_audit_rows_nearest_wide: audit_rows_nearest for any m in 1 .. 64 -- m <= 16 forwards to it bit for bit,
        16 < m <= 64 ranks audit_rows_wide's dist rows on the device.  Returns what audit_rows_nearest returns."""
        return self._score_rows("chb_audit_rows_nearest_wide", labels, B, None, m=m, k=k, rows=rows, groups=groups, slot=True)

    def recruit_rows_nearest_wide(self, labels, B, m, k, Y):
        """chb_recruit_rows_nearest_wide: recruit_rows_nearest for any m in 1 .. 64 (16 < m <= 64: ranked from
        recruit_rows_wide's dist rows).  Returns (bins [Q, k], dist [Q, k])."""
        return self._score_rows("chb_recruit_rows_nearest_wide", labels, B, None, m=m, k=k, Y=Y)

    def bin_report_wide(self, labels, B, m, rows=None, groups=None):
        """chb_bin_report_wide: bin_report (with `groups` bin_report_grouped) for any m in 1 .. 64 -- m <= 16 forwards bit
        for bit, 16 < m <= 64 sums up audit_rows_wide's answer.  Returns what bin_report returns."""
        return self._bin_report("chb_bin_report_wide", labels, B, m, rows, groups, slot=True)

    def audit_pairs_witness_wide(self, labels, B, m, rows, bins, groups=None):
        """chb_audit_pairs_witness_wide: audit_pairs_witness for any m in 1 .. 64 -- m <= 16 forwards bit for bit; at
        16 < m <= 64 dist and neighbors are audit_pairs_wide's dist and idx, neighbor_dist the members' selection
        distances and weights what the wide solve kernel returned.  Returns what audit_pairs_witness returns."""
        return self._score_pairs("chb_audit_pairs_witness_wide", labels, B, m, rows, bins, groups=groups, slot=True,
                                 witness=True)

    def recruit_pairs_witness_wide(self, labels, B, m, Y, row_of, bins):
        """chb_recruit_pairs_witness_wide: recruit_pairs_witness for any m in 1 .. 64.  Returns what it returns."""
        return self._score_pairs("chb_recruit_pairs_witness_wide", labels, B, m, row_of, bins, Y=Y, witness=True)

    def find_nearest_from_row(self, c, labels, row, m):
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        row = np.ascontiguousarray(row, dtype=np.float64)
        out = np.empty(max(int(m), 1), dtype=np.int64)
        cnt = C.c_int32(0)
        check(self._lib.chb_find_nearest_from_row(self._h, int(c), labels, row, labels.shape[0],
                                                  int(m), out, C.byref(cnt)))
        return out[: cnt.value].copy()

    def hull_distance_batch(self, query_idx, hull_idx, want_alpha=False):
        q = np.ascontiguousarray(query_idx, dtype=np.int64)
        hx = np.ascontiguousarray(hull_idx, dtype=np.int64)
        P, m_max = hx.shape
        dist = np.empty(P, dtype=np.float64)
        alpha = np.zeros((P, m_max), dtype=np.float64) if want_alpha else None
        check(self._lib.chb_hull_distance_batch(self._h, q, P, hx, int(m_max), dist,
                                                None if alpha is None else alpha.ctypes.data))
        return (dist, alpha) if want_alpha else dist

    def hull_distance_points(self, x, pts, want_alpha=False):
        x = np.ascontiguousarray(x, dtype=np.float64)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, x.shape[0])
        m = pts.shape[0]
        d = C.c_double(0.0)
        alpha = np.zeros(max(m, 1), dtype=np.float64)
        if m == 0:
            pts = np.zeros((1, x.shape[0]))
        check(self._lib.chb_hull_distance_points(self._h, x, pts, int(m), x.shape[0], C.byref(d),
                                                 alpha.ctypes.data))
        return (d.value, alpha[:m]) if want_alpha else d.value

    def fit_cluster(self, B, initial_bins, perms, m, max_iter, batch=0, want_min_dist=False):
        initial = np.ascontiguousarray(initial_bins, dtype=np.int64)
        perms = np.ascontiguousarray(perms, dtype=np.int64).reshape(max_iter, -1) \
            if max_iter > 0 else np.zeros((0, 0), dtype=np.int64)
        n_move = perms.shape[1] if max_iter > 0 else 0
        out = np.empty(self.N, dtype=np.int64)
        changed = np.zeros(max(max_iter, 1), dtype=np.int64)
        iters = C.c_int(0)
        mind = np.empty(self.N, dtype=np.float64) if want_min_dist else None
        perms_arg = perms if perms.size else np.zeros(1, dtype=np.int64)
        check(self._lib.chb_fit_cluster(self._h, int(B), initial, perms_arg, int(n_move), int(m),
                                        int(max_iter), int(batch), out, C.byref(iters), changed,
                                        None if mind is None else mind.ctypes.data))
        res = (out, iters.value, changed[: iters.value])
        return res + (mind,) if want_min_dist else res

    def fit_cluster_margins(self, B, initial_bins, perms, m, max_iter, batch=0, want_min_dist=False):
        """fit_cluster plus, per movable contig, runner-up minus winning hull distance at its last visit:
        (labels, sweeps, margin), or with want_min_dist (labels, sweeps, changed, min_dist, margin)."""
        initial = np.ascontiguousarray(initial_bins, dtype=np.int64)
        perms = np.ascontiguousarray(perms, dtype=np.int64).reshape(max_iter, -1)
        out = np.empty(self.N, dtype=np.int64)
        changed = np.zeros(max(max_iter, 1), dtype=np.int64)
        iters = C.c_int(0)
        mind = np.empty(self.N, dtype=np.float64)
        margin = np.empty(self.N, dtype=np.float64)
        check(self._lib.chb_fit_cluster_ex(self._h, int(B), initial, perms, int(perms.shape[1]), int(m),
                                           int(max_iter), int(batch), out, C.byref(iters), changed,
                                           mind.ctypes.data, margin.ctypes.data))
        if want_min_dist:
            return out, iters.value, changed[: iters.value], mind, margin
        return out, iters.value, margin

    # stepwise (multi-GPU driver)
    def fit_begin(self, B, initial_bins, m):
        check(self._lib.chb_fit_begin(self._h, int(B), np.ascontiguousarray(initial_bins, dtype=np.int64), int(m)))

    def batch_begin(self, perm_slice, q_lo, q_hi):
        p = np.ascontiguousarray(perm_slice, dtype=np.int64)
        check(self._lib.chb_batch_begin(self._h, p, p.shape[0], int(q_lo), int(q_hi)))

    def batch_guess(self, guess):
        check(self._lib.chb_batch_guess(self._h, guess))

    def batch_round(self, lab_prev, active, lab_new, min_dist=None):
        check(self._lib.chb_batch_round(self._h, np.ascontiguousarray(lab_prev, dtype=np.int64),
                                        int(active), lab_new,
                                        None if min_dist is None else min_dist.ctypes.data))

    def batch_commit(self, final_labels):
        check(self._lib.chb_batch_commit(self._h, np.ascontiguousarray(final_labels, dtype=np.int64)))

    def fit_labels(self):
        out = np.empty(self.N, dtype=np.int64)
        check(self._lib.chb_fit_labels(self._h, out))
        return out

    # multi-GPU (RCCL inside chb_fit_cluster)
    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(128)
        check(load().chb_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        check(self._lib.chb_comm_init(self._h, C.c_char_p(unique_id), int(rank), int(world)))
        self.rank, self.world = int(rank), int(world)

    ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)

    def comm_init_hook(self, rank: int, world: int, allgather):
        """The sharded C++ loop with a host-side exchange: allgather(send: np.uint8[bytes]) ->
        np.uint8[world * bytes] (rank-major)."""
        def _cb(_user, send, recv, nbytes):
            try:
                src = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(nbytes,))
                out = np.ascontiguousarray(allgather(src.copy()), dtype=np.uint8).reshape(-1)
                if out.size != nbytes * world:
                    return 1
                C.memmove(recv, out.ctypes.data, out.size)
                return 0
            except Exception:  # noqa: BLE001
                return 2
        self._hook_cb = self.ALLGATHER_FN(_cb)      # keep the trampoline alive
        check(self._lib.chb_comm_init_hook(self._h, int(rank), int(world), C.cast(self._hook_cb, C.c_void_p), None))
        self.rank, self.world = int(rank), int(world)

    def comm_destroy(self):
        check(self._lib.chb_comm_destroy(self._h))

    def bcast_samples(self, X, N, D, root=0):
        """chb_set_samples for all ranks of the RCCL communicator: the root passes its host matrix, the others None;
        the matrix crosses the host boundary once and reaches the other GPUs by an RCCL broadcast over xGMI."""
        ptr = None
        if X is not None:
            X = np.ascontiguousarray(X, dtype=np.float64)
            if X.shape != (int(N), int(D)):
                raise ValueError("samples must be an N x D matrix")
            ptr = X.ctypes.data_as(C.c_void_p)
        check(self._lib.chb_bcast_samples(self._h, ptr, int(N), int(D), int(root)))
        self.N, self.D = int(N), int(D)

    def comm_info(self):
        """{'rank', 'world', 'comm_ranks' (what RCCL reports for the communicator; 0 without one), 'transport'}"""
        r, w, n, t = C.c_int(0), C.c_int(1), C.c_int(0), C.c_int(0)
        check(self._lib.chb_comm_info(self._h, C.byref(r), C.byref(w), C.byref(n), C.byref(t)))
        return {"rank": r.value, "world": w.value, "comm_ranks": n.value,
                "transport": {0: "none", 1: "rccl", 2: "hook"}[t.value]}

    # measurement
    def profile_enable(self, on=True):
        """on: False / 0 off, True / 1 every kernel, 2 only the two dominant kernels."""
        check(self._lib.chb_profile_enable(self._h, int(on)))

    def profile_reset(self):
        check(self._lib.chb_profile_reset(self._h))

    def profile_get(self, kernel):
        ms, n, w = C.c_double(0), C.c_int64(0), C.c_double(0)
        check(self._lib.chb_profile_get(self._h, kernel.encode(), C.byref(ms), C.byref(n), C.byref(w)))
        return {"ms": ms.value, "launches": n.value, "work": w.value}

    def counter(self, name):
        v = C.c_int64(0)
        check(self._lib.chb_counter(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def kmer_frequencies(self, sequences, k=4, return_counts=False):
        """chb_kmer_frequencies: sequences = list of bytes / str, one per contig."""
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in sequences]
        dim = self._lib.chb_kmer_dim(int(k))
        if dim <= 0:
            raise ChbError(self._lib.chb_last_error().decode())
        offsets = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            offsets[1:] = np.cumsum([len(b) for b in bs])
        freq = np.zeros((len(bs), dim), dtype=np.float64)
        counts = np.zeros((len(bs), dim), dtype=np.uint32) if return_counts else None
        check(self._lib.chb_kmer_frequencies(self._h, b"".join(bs), offsets, len(bs), int(k), freq.reshape(-1),
                                              counts.ctypes.data_as(C.c_void_p) if counts is not None else None))
        return (freq, counts) if return_counts else freq

    @staticmethod
    def _pack_sequences(sequences):
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in sequences]
        offsets = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            offsets[1:] = np.cumsum([len(b) for b in bs])
        return b"".join(bs), offsets, len(bs)

    def _profile_dim(self, ks):
        ks = np.ascontiguousarray(list(ks), dtype=np.int32).reshape(-1)
        dim = self._lib.chb_kmer_profile_dim(ks, len(ks))
        if dim <= 0:
            check(dim)
        return ks, int(dim)

    def kmer_profiles(self, sequences, ks, return_counts=False):
        """chb_kmer_profiles: the k-mer blocks of the list `ks` side by side (list order), all counted in one pass."""
        ks, dim = self._profile_dim(ks)
        seq, offsets, n = self._pack_sequences(sequences)
        freq = np.zeros((n, dim), dtype=np.float64)
        counts = np.zeros((n, dim), dtype=np.uint32) if return_counts else None
        check(self._lib.chb_kmer_profiles(self._h, seq, offsets, n, ks, len(ks), freq.reshape(-1),
                                           counts.ctypes.data_as(C.c_void_p) if counts is not None else None))
        return (freq, counts) if return_counts else freq

    def set_samples_from_sequences(self, sequences, ks, extra=None, extra_row=None, return_matrix=False):
        """chb_set_samples_from_sequences: the resident samples become [k-mer blocks of `ks` | extra[extra_row]], built
        on the device.  extra: [n_extra, S] (coverage), extra_row: [n] rows of it (None: row i of extra for contig i)."""
        ks, dim = self._profile_dim(ks)
        seq, offsets, n = self._pack_sequences(sequences)
        n_extra = S = 0
        if extra is not None:
            extra = np.ascontiguousarray(extra, dtype=np.float64)
            if extra.ndim != 2:
                raise ValueError("extra must be a 2-D array")
            n_extra, S = extra.shape
        if extra_row is not None:
            extra_row = np.ascontiguousarray(extra_row, dtype=np.int64).reshape(-1)
            if len(extra_row) != n:
                raise ValueError("extra_row needs one entry per sequence")
        X = np.empty((n, dim + S), dtype=np.float64) if return_matrix else None
        check(self._lib.chb_set_samples_from_sequences(
            self._h, seq, offsets, n, ks, len(ks), None if extra is None else extra.ctypes.data, n_extra, S,
            None if extra_row is None else extra_row.ctypes.data, None if X is None else X.ctypes.data))
        self.N, self.D = n, dim + S
        return X

    def fit_stats(self):
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.chb_fit_stats(self._h, out))
        return {"batches": int(out[0]), "rounds": int(out[1]), "hull_evaluated": int(out[2]),
                "hull_needed": int(out[3])}


def default_context(device=None):
    """Process-wide context for `device` (default: LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get("CHBIN_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with _lock:
        ctx = _ctx_by_device.get(device)
    if ctx is None:
        ctx = Context(device)
        with _lock:
            _ctx_by_device[device] = ctx
    return ctx
