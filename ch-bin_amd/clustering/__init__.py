"""Host-side mirror of the reference package `ch_bin.core.clustering` (same function names,
argument meaning and error behaviour) on top of libchbin_hip.so."""
from .algorithm import (  # noqa: F401
    BinReport,
    NearestBins,
    NeighborSweep,
    Witness,
    audit,
    audit_pairs,
    audit_pairs_sweep,
    bin_report,
    cohesion,
    cohesion_sweep,
    fit_cluster,
    nearest_bins,
    neighbor_sweep,
    neighbor_sweep_wide,
    parent_groups,
    recruit,
    recruit_nearest_bins,
    recruit_pairs,
    recruit_pairs_sweep,
    recruit_witness,
    witness,
)
from .distance_matrix import (  # noqa: F401
    create_distance_matrix,
    create_in_mem_distance_matrix,
    find_nearest_from_cluster,
)
from .dump_bins import dump_bins  # noqa: F401
from .hull_distance import (  # noqa: F401
    affine_hull_distance,
    affine_hull_distance_qp,
    calculate_distance,
    convex_hull_distance,
)
from .solve_qp import SOLVERS, solve_qp  # noqa: F401
