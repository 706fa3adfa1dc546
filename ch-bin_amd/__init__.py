"""chbin_amd -- MI355X-native convex-hull binning hot path of CH-Bin.

Mirrors the reference's `ch_bin.core.clustering` call surface (fit_cluster, calculate_distance,
find_nearest_from_cluster, create_in_mem_distance_matrix, ...) on top of a C-ABI HIP library
(include/chbin_hip.h, csrc/).  There is no CPU fallback: every compute entry point raises if the
HIP library or a GPU is missing.
"""
from . import synth  # noqa: F401

__all__ = ["synth", "recruit", "audit", "bin_report", "neighbor_sweep", "neighbor_sweep_wide", "audit_pairs", "recruit_pairs",
           "cohesion", "audit_pairs_sweep", "recruit_pairs_sweep", "cohesion_sweep"]


def __getattr__(name):
    # chbin_amd.recruit = clustering.recruit, chbin_amd.audit = clustering.audit, chbin_amd.bin_report =
    # clustering.bin_report, chbin_amd.neighbor_sweep = clustering.neighbor_sweep, and audit_pairs / recruit_pairs /
    # cohesion and their _sweep forms likewise, resolved on first use (importing the package stays free of ctypes work)
    if name == "recruit":
        from .clustering import recruit
        return recruit
    if name == "audit":
        from .clustering import audit
        return audit
    if name == "bin_report":
        from .clustering import bin_report
        return bin_report
    if name == "neighbor_sweep":
        from .clustering import neighbor_sweep
        return neighbor_sweep
    if name in ("audit_pairs", "recruit_pairs", "cohesion", "neighbor_sweep_wide", "audit_pairs_sweep", "recruit_pairs_sweep",
                "cohesion_sweep"):
        from . import clustering
        return getattr(clustering, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
