"""Feature assembly next to the hot path: mirror of ch_bin.core.features for
the parts that need no external bioinformatics tool -- canonical k-mer frequencies (HIP kernel in
place of the seq2vec run), coverage normalisation, contig filtering / splitting -- and, re-exported from cli_features, the
stage driver that strings them together (create_dataset, run_create_dataset, assemble_samples)."""
from .coverage import parse_coverages  # noqa: F401
from .kmer_count import count_kmers, kmer_frequencies, kmer_profiles  # noqa: F401
from .preprocess import filter_short_contigs, get_contig_lengths, split_contigs  # noqa: F401

_STAGE = ("create_dataset", "run_create_dataset", "assemble_samples")


def __getattr__(name):
    # (on first use: cli_features itself imports this package)
    if name in _STAGE:
        from .. import cli_features
        return getattr(cli_features, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
