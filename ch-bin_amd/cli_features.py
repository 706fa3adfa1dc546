"""Mirror of the features stage driver ch_bin/cli/features.py:20-139: contig FASTA, abundance table and seed contigs in,
features.csv (the file cli_clustering.perform_clustering reads) out -- same intermediate files, same columns, same rows
in the same order, same log lines.

Two things differ in how it gets there.  The marker-gene stage (scm_gene.py: FragGeneScan + HMMER, external tools) is out
of scope, so the seed contigs come from the `seed_clusters` argument or, failing that, from `<operating_dir>/scm/seeds.txt`,
the file scm_gene.py:212-213 writes.  And where the reference counts k-mers once per k of `KmerK` and merges one DataFrame
per k, this stage works out the final row list first (names, parents, CLUSTER, the join with the abundance table), orders
the sequences accordingly and makes ONE kmer_profiles call for the whole list of k.

`assemble_samples` goes one step further: it hands sequences, normalised coverage table and parent map to
Context.set_samples_from_sequences, so that the feature matrix is built on the device and becomes the default context's
resident samples without ever crossing the host boundary."""
import collections
import logging
from configparser import SectionProxy
from pathlib import Path
from typing import List, Optional

import numpy as np
import pandas as pd

from . import _lib
from .features import kmer_count
from .features.coverage import parse_coverages
from .features.fasta import read_fasta
from .features.preprocess import filter_short_contigs, get_contig_lengths, split_contigs

logger = logging.getLogger(__name__)


def _read_seeds(scm_dir: Path, seed_clusters) -> List[str]:
    if seed_clusters is not None:
        return [str(s) for s in seed_clusters]
    seeds_file = scm_dir / "seeds.txt"
    seeds = [ln.strip() for ln in open(seeds_file)] if seeds_file.is_file() else []
    seeds = [s for s in seeds if s]
    if not seeds:
        raise Exception("No HMMER seed hits found")   # scm_gene.py:198
    return seeds


def _block_labels(kmer_ks, tool):
    """Column labels of one k block as count_kmers gives them: integers for seq2vec, k-mer strings for kmer_counter."""
    if tool == "seq2vec":
        return [list(range(len(kmer_count.canonical_kmers(k)))) for k in kmer_ks]
    if tool == "kmer_counter":
        return [kmer_count.canonical_kmers(k) for k in kmer_ks]
    raise NotImplementedError(f"Tool {tool} is not implemented")


def _suffix_clashes(left, right, lsuffix, rsuffix):
    """What DataFrame.merge does to the labels of its two sides: a label both sides carry gets the side's suffix."""
    both = set(left) & set(right)
    return ([f"{c}{lsuffix}" if c in both else c for c in left], [f"{c}{rsuffix}" if c in both else c for c in right])


def _feature_header(kmer_ks, tool, coverage_labels):
    """Labels of the feature columns of features.csv: the k blocks merged one after the other with the suffixes
    (x_i, y_i) of cli/features.py:90-92, then the coverage columns merged with pandas' default (_x, _y) (:107)."""
    blocks = _block_labels(kmer_ks, tool)
    merged = list(blocks[0])
    for i, block in enumerate(blocks[1:], start=1):
        left, right = _suffix_clashes(merged, block, f"x_{i}", f"y_{i}")
        merged = left + right
    left, right = _suffix_clashes(merged, list(coverage_labels), "_x", "_y")
    return left + right


# the rows of features.csv before any number is computed: coverage_rows[i] = the row of coverage_values of row i's parent
_Rows = collections.namedtuple("_Rows", "names parents clusters sequences coverage_rows coverage_values coverage_labels")


def _prepare_rows(contig_fasta, coverage_file, operating_dir, kmer_ks, kmer_counter_tool, short_contig_threshold,
                  seed_contig_split_len, seed_clusters) -> _Rows:
    """Steps 01-04 and the row bookkeeping of 06-07 of cli/features.py:47-109."""
    contig_fasta, coverage_file, operating_dir = Path(contig_fasta), Path(coverage_file), Path(operating_dir)
    assert len(kmer_ks) > 0, "No k-mer k values provided"
    _block_labels(kmer_ks, kmer_counter_tool)   # (an unknown tool fails before any file is written)
    filtered_fasta = operating_dir / "filtered-contigs.fasta"
    split_fasta = operating_dir / "split-contigs.fasta"
    scm_operation_dir = operating_dir / "scm"
    operating_dir.mkdir(parents=True, exist_ok=True)
    (operating_dir / "kmers").mkdir(parents=True, exist_ok=True)
    scm_operation_dir.mkdir(parents=True, exist_ok=True)

    logger.info(">> Calculating coverages...")
    df_coverages = parse_coverages(coverage_file)

    logger.info(">> Removing contigs shorter than %s bp.", short_contig_threshold)
    contig_lengths = get_contig_lengths(contig_fasta)
    removed_contigs = filter_short_contigs(contig_fasta, filtered_fasta, threshold=short_contig_threshold)
    logger.info("Removed %s (of %s) short contigs.", len(removed_contigs), len(contig_lengths))

    logger.info(">> Performing single-copy marker gene analysis...")
    seeds = _read_seeds(scm_operation_dir, seed_clusters)
    logger.info("Found %s seeds.", len(seeds))

    logger.info(">> Splitting all contigs to contain %s bp.", seed_contig_split_len)
    sub_contigs = split_contigs(filtered_fasta, split_fasta, seeds, split_len=seed_contig_split_len)
    logger.info("Found %s contigs after splitting.", len(sub_contigs))

    # The outer merge of sub contigs and seeds (cli/features.py:100) sorts by its key PARENT_NAME and keeps the split
    # order within a parent; the inner join with the abundance table (:107) then drops the parents the table lacks.
    cluster_of = {}
    for i, seed in enumerate(seeds):
        cluster_of.setdefault(seed, i)
    coverage_row = {}
    for i, name in enumerate(df_coverages["CONTIG_NAME"].astype(str)):
        coverage_row.setdefault(name, i)
    order = sorted(sub_contigs.items(), key=lambda item: item[1])   # (stable: split order within a parent)
    order = [(name, parent) for name, parent in order if parent in coverage_row]
    sequence_of = {ident: seq for ident, _rest, seq in read_fasta(split_fasta)}
    coverage_labels = [c for c in df_coverages.columns if c != "CONTIG_NAME"]
    return _Rows(names=[name for name, _ in order], parents=[parent for _, parent in order],
                 clusters=np.array([cluster_of.get(parent, -1) for _, parent in order], dtype=np.int64),
                 sequences=[sequence_of[name] for name, _ in order],
                 coverage_rows=np.array([coverage_row[parent] for _, parent in order], dtype=np.int64),
                 coverage_values=np.ascontiguousarray(df_coverages[coverage_labels].to_numpy(dtype=np.float64)),
                 coverage_labels=coverage_labels)


def create_dataset(
    contig_fasta: Path,
    coverage_file: Path,
    operating_dir: Path,
    kmer_ks: List[int],
    kmer_counter_tool: str = "kmer_counter",
    short_contig_threshold: int = 1000,
    coverage_thresh: float = 0.4,
    select_percentile: float = 0.95,
    seed_contig_split_len: int = 10000,
    seed_clusters: Optional[List[str]] = None,
) -> Path:
    """cli/features.py:20-114.  `coverage_thresh` and `select_percentile` steer the marker-gene stage and are accepted for
    the signature's sake; the seed contigs are `seed_clusters` or the lines of `<operating_dir>/scm/seeds.txt`.
    `kmer_counter_tool` decides the k-mer column labels as in count_kmers ("seq2vec": integers, which is where the
    x_i / y_i / _x / _y suffixes of the reference's header come from; "kmer_counter": k-mer strings).  Returns the path
    of features.csv."""
    operating_dir = Path(operating_dir)
    output_dataset_csv = operating_dir / "features.csv"
    rows = _prepare_rows(contig_fasta, coverage_file, operating_dir, kmer_ks, kmer_counter_tool, short_contig_threshold,
                         seed_contig_split_len, seed_clusters)

    logger.info(">> Calculating normalized kmer frequencies using %s ...", kmer_counter_tool)
    header = _feature_header(kmer_ks, kmer_counter_tool, rows.coverage_labels)
    if rows.names:
        profiles = np.asarray(kmer_count.kmer_profiles(rows.sequences, list(kmer_ks)), dtype=np.float64)
    else:
        profiles = np.zeros((0, len(header) - len(rows.coverage_labels)))

    logger.info(">> Creating a dataset with the initial cluster information...")
    logger.info(">> Merging all the features...")
    features = np.hstack([profiles, rows.coverage_values[rows.coverage_rows].reshape(len(rows.names), -1)])
    df_merged = pd.DataFrame(features, columns=pd.Index(header, dtype=object))
    df_merged.insert(0, "CONTIG_NAME", rows.names)
    df_merged.insert(1, "PARENT_NAME", rows.parents)
    df_merged.insert(2, "CLUSTER", rows.clusters)
    df_merged.to_csv(output_dataset_csv, index=False)
    logger.info("Generated csv with shape %s...", df_merged.shape)
    logger.info("Dumped features CSV at %s...", output_dataset_csv)
    return output_dataset_csv


def assemble_samples(
    contig_fasta: Path,
    coverage_file: Path,
    operating_dir: Path,
    kmer_ks: List[int],
    kmer_counter_tool: str = "kmer_counter",
    short_contig_threshold: int = 1000,
    coverage_thresh: float = 0.4,
    select_percentile: float = 0.95,
    seed_contig_split_len: int = 10000,
    seed_clusters: Optional[List[str]] = None,
    device=None,
):
    """The rows of create_dataset as the default context's resident samples, built on the device: row i = [k-mer blocks
    of `kmer_ks` | normalised coverage of the row's parent].  No features.csv is written and no feature value crosses the
    host boundary; the context is ready for fit_cluster.  Returns (names, parents, initial_bins)."""
    rows = _prepare_rows(contig_fasta, coverage_file, Path(operating_dir), kmer_ks, kmer_counter_tool,
                         short_contig_threshold, seed_contig_split_len, seed_clusters)
    logger.info(">> Calculating normalized kmer frequencies into the resident samples ...")
    _lib.default_context(device).set_samples_from_sequences(rows.sequences, list(kmer_ks), extra=rows.coverage_values,
                                                            extra_row=rows.coverage_rows)
    logger.info("Resident samples: %s rows...", len(rows.names))
    return rows.names, rows.parents, rows.clusters


def run_create_dataset(contig_fasta: Path, coverage_file: Path, operating_dir: Path, parameters: SectionProxy) -> Path:
    """cli/features.py:117-139: same INI keys (config/default.ini); KmerK is a comma list."""
    kmer_ks = [int(k) for k in parameters["KmerK"].split(",")]
    return create_dataset(
        contig_fasta=contig_fasta,
        coverage_file=coverage_file,
        operating_dir=operating_dir,
        kmer_ks=kmer_ks,
        kmer_counter_tool=parameters["KmerCounterTool"],
        short_contig_threshold=int(parameters["ContigLengthFilterBp"]),
        coverage_thresh=float(parameters["ScmCoverageThreshold"]),
        select_percentile=float(parameters["ScmSelectPercentile"]),
        seed_contig_split_len=int(parameters["SeedContigSplitLengthBp"]),
    )
