"""The features-stage mirror (ch-bin_amd/cli_features.py), CPU part: create_dataset against tests/golden/create_dataset.npz,
which tests/golden/make_golden_dataset.py wrote by running the reference's own create_dataset (cli/features.py:20-114)
under pandas with stand-ins for the external tools.  The k-mer numbers come from the oracle here (kmer_count.kmer_profiles
is patched: no GPU); what is pinned is everything around them -- header labels incl. pandas' suffix artefacts, row order
(sorted by PARENT_NAME, split order within a parent), CLUSTER, the coverage join and the dropped contigs."""
import configparser
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chbin_amd  # noqa: E402,F401
from chbin_amd import cli_features  # noqa: E402
from chbin_amd.features import fasta, kmer_count  # noqa: E402
from oracle import oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_LISTS = [[4], [4, 5], [3, 4, 5]]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "create_dataset.npz"))


@pytest.fixture
def oracle_profiles(monkeypatch):
    """kmer_count.kmer_profiles answered by the oracle; records the calls."""
    calls = []

    def profiles(sequences, ks, device=None):
        calls.append((list(sequences), list(ks)))
        return np.hstack([O.kmer_frequencies(sequences, k)[0] for k in ks])
    monkeypatch.setattr(kmer_count, "kmer_profiles", profiles)
    return calls


def _write_inputs(gold, tmp_path):
    fa, cov = tmp_path / "contigs.fasta", tmp_path / "abundance.tsv"
    with open(fa, "w") as fh:
        for ident, desc, seq in zip(gold["in_ids"].tolist(), gold["in_desc"].tolist(), gold["in_seq"].tolist()):
            fasta.write_record(fh, ident, seq, description=desc, width=70)
    with open(cov, "w") as fh:
        for name, row in zip(gold["abundance_names"].tolist(), gold["abundance_raw"]):
            fh.write(name + "\t" + "\t".join(repr(float(v)) for v in row) + "\n")
    return fa, cov


def _check_against_fixture(gold, csv, ks, calls):
    tag = "_".join(str(k) for k in ks)
    header = open(csv).readline().rstrip("\r\n").split(",")
    assert header == gold["header_" + tag].tolist()
    df = pd.read_csv(csv, float_precision="round_trip")
    assert df["CONTIG_NAME"].tolist() == gold["contig_" + tag].tolist()
    assert df["PARENT_NAME"].tolist() == gold["parent_" + tag].tolist()
    assert df["PARENT_NAME"].tolist() == sorted(df["PARENT_NAME"].tolist())
    assert df["CLUSTER"].dtype.kind == "i" and np.array_equal(df["CLUSTER"].to_numpy(), gold["cluster_" + tag])
    # the dropped contigs: below the length filter, missing from the abundance table
    assert not {"tiny_1", "beta_9"} & set(df["PARENT_NAME"])
    dk = sum(O.kmer_dim(k) for k in ks)
    assert df.shape == (len(gold["contig_" + tag]), 3 + dk + 2)
    assert np.array_equal(df.iloc[:, 3 + dk:].to_numpy(), gold["coverage_" + tag])   # same pandas operations: bit-exact
    # ONE call for the whole list, the sequences in row order; the blocks side by side in list order
    assert len(calls) == 1 and calls[0][1] == list(ks)
    pieces = dict(zip(df["CONTIG_NAME"], calls[0][0]))
    whole = dict(zip(gold["in_ids"].tolist(), gold["in_seq"].tolist()))
    for parent in set(df["PARENT_NAME"]):
        mine = [pieces[n] for n, p in zip(df["CONTIG_NAME"], df["PARENT_NAME"]) if p == parent]
        assert "".join(mine) == whole[parent]
    want = np.hstack([O.kmer_frequencies(calls[0][0], k)[0] for k in ks])
    assert np.array_equal(df.iloc[:, 3:3 + dk].to_numpy(), want)


@pytest.mark.parametrize("ks", K_LISTS, ids=lambda ks: "-".join(map(str, ks)))
def test_create_dataset_matches_reference_fixture(gold, oracle_profiles, tmp_path, ks):
    fa, cov = _write_inputs(gold, tmp_path)
    work = tmp_path / "work"
    csv = cli_features.create_dataset(fa, cov, work, ks, kmer_counter_tool="seq2vec",
                                      short_contig_threshold=int(gold["threshold"]),
                                      seed_contig_split_len=int(gold["split_len"]), seed_clusters=gold["seeds"].tolist())
    assert csv == work / "features.csv"
    for name in ("filtered-contigs.fasta", "split-contigs.fasta", "kmers", "scm", "features.csv"):
        assert (work / name).exists(), name
    _check_against_fixture(gold, csv, ks, oracle_profiles)
    # a seed shorter than the split length stays one piece; a longer one is cut
    names = pd.read_csv(csv)["CONTIG_NAME"].tolist()
    assert "alpha_3_S0" in names and "alpha_3_S1" not in names and "zeta_7_S2" in names


def test_kmer_counter_tool_gives_kmer_labels(gold, oracle_profiles, tmp_path):
    fa, cov = _write_inputs(gold, tmp_path)
    csv = cli_features.create_dataset(fa, cov, tmp_path / "work", [1, 2], short_contig_threshold=1000,
                                      seed_contig_split_len=1200, seed_clusters=gold["seeds"].tolist())
    header = open(csv).readline().rstrip("\r\n").split(",")
    assert header[3:] == kmer_count.canonical_kmers(1) + kmer_count.canonical_kmers(2) + ["1", "2"]
    with pytest.raises(NotImplementedError):
        cli_features.create_dataset(fa, cov, tmp_path / "w2", [4], kmer_counter_tool="jellyfish", seed_clusters=["zeta_7"])


def test_seeds_come_from_the_marker_stage_file(gold, oracle_profiles, tmp_path):
    fa, cov = _write_inputs(gold, tmp_path)
    work = tmp_path / "work"
    (work / "scm").mkdir(parents=True)
    with open(work / "scm" / "seeds.txt", "w") as fh:
        fh.write("\n".join(gold["seeds"].tolist()))   # (scm_gene.py:212-213: no newline at the end)
    csv = cli_features.create_dataset(fa, cov, work, [4, 5], kmer_counter_tool="seq2vec",
                                      short_contig_threshold=int(gold["threshold"]),
                                      seed_contig_split_len=int(gold["split_len"]))
    _check_against_fixture(gold, csv, [4, 5], oracle_profiles)


def test_missing_seeds_raise_the_reference_exception(gold, oracle_profiles, tmp_path):
    fa, cov = _write_inputs(gold, tmp_path)
    with pytest.raises(Exception, match="No HMMER seed hits found"):
        cli_features.create_dataset(fa, cov, tmp_path / "work", [4], kmer_counter_tool="seq2vec")
    assert not oracle_profiles and not (tmp_path / "work" / "features.csv").exists()


def test_run_create_dataset_parses_the_kmer_list(gold, oracle_profiles, tmp_path):
    fa, cov = _write_inputs(gold, tmp_path)
    work = tmp_path / "work"
    (work / "scm").mkdir(parents=True)
    with open(work / "scm" / "seeds.txt", "w") as fh:
        fh.write("\n".join(gold["seeds"].tolist()))
    cfg = configparser.ConfigParser()
    cfg.read_string("[PARAMETERS]\nKmerK = 4,5\nKmerCounterTool = seq2vec\nContigLengthFilterBp = %d\n"
                    "ScmCoverageThreshold = 0.4\nScmSelectPercentile = 0.95\nSeedContigSplitLengthBp = %d\n"
                    % (int(gold["threshold"]), int(gold["split_len"])))
    csv = cli_features.run_create_dataset(fa, cov, work, cfg["PARAMETERS"])
    _check_against_fixture(gold, csv, [4, 5], oracle_profiles)


def test_stage_is_reexported_from_features():
    from chbin_amd import features
    assert features.create_dataset is cli_features.create_dataset
    assert features.run_create_dataset is cli_features.run_create_dataset
    assert features.assemble_samples is cli_features.assemble_samples
    assert features.kmer_profiles is kmer_count.kmer_profiles
