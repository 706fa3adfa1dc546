"""Fixture for the features-stage mirror (ch-bin_amd/cli_features.py): the reference's own create_dataset
(ch_bin/cli/features.py:20-114) run on a six-contig FASTA with two samples, for KmerK = 4, `4,5` and `3,4,5`.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden_dataset.py
Writes tests/golden/create_dataset.npz.

What runs unchanged is create_dataset itself with the reference's parse_coverages, get_contig_lengths,
filter_short_contigs and split_contigs, under this machine's pandas: the outer merge that orders the rows, the inner joins
that drop rows, the suffixes pandas gives to clashing column labels.  Stand-ins, in this process only:
  * `Bio` (absent here): the reader / recording writer of make_golden_features.py, plus an empty `Bio.SearchIO` with a
    `Hit` name so that scm_gene.py imports;
  * `count_kmers` (an external tool run): one row per record of the split FASTA, a CONTIG_NAME column and the integer column
    labels 0..dim-1 of the seq2vec path (kmer_count.py:99-105); the numbers are 1000 k + column + row / 1000, arbitrary and
    NOT part of what is pinned -- they only let this script check that the blocks come out in list order;
  * `identify_marker_genomes` (FragGeneScan + HMMER): returns the seed list below.
Pinned: header, row order, CONTIG_NAME / PARENT_NAME / CLUSTER, the coverage columns, which contigs are dropped.
"""
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden_features as G  # noqa: E402  (puts the reference on sys.path)

THRESHOLD, SPLIT_LEN = 1000, 1200
K_LISTS = ([4], [4, 5], [3, 4, 5])
SEEDS = ["k141_90", "zeta_7", "alpha_3"]
# FASTA order; not alphabetical.  tiny_1 is below the filter, alpha_3 is a seed shorter than the split length, beta_9 is
# missing from the abundance table (which still lists tiny_1)
LENGTHS = {"zeta_7": 3700, "k141_90": 2600, "tiny_1": 400, "mid_12": 2100, "alpha_3": 1100, "beta_9": 1500}
ABUNDANCE = ["mid_12", "tiny_1", "zeta_7", "alpha_3", "k141_90"]


def _dim(k):
    return (4 ** k + (4 ** (k // 2) if k % 2 == 0 else 0)) // 2


def _install_standins():
    G._install_bio_standin()
    searchio = types.ModuleType("Bio.SearchIO")
    searchio.Hit = type("Hit", (), {})
    sys.modules["Bio"].SearchIO = searchio
    sys.modules["Bio.SearchIO"] = searchio


def _count_kmers(contig_fasta, operating_dir, k=4, tool="kmer_counter"):
    from Bio import SeqIO
    with open(contig_fasta) as fh:
        names = [r.id for r in SeqIO.parse(fh, "fasta")]
    vals = 1000.0 * k + np.arange(_dim(k))[None, :] + np.arange(len(names))[:, None] / 1000.0
    df = pd.DataFrame(vals)
    df["CONTIG_NAME"] = names
    return df


def main():
    _install_standins()
    from ch_bin.cli import features as ref

    ref.count_kmers = _count_kmers
    ref.identify_marker_genomes = lambda *a, **kw: list(SEEDS)

    rng = np.random.default_rng(17)
    recs = [(n, "len=%d" % v, "".join(rng.choice(list("ACGT"), v))) for n, v in LENGTHS.items()]
    raw = rng.lognormal(1.0, 1.0, size=(len(ABUNDANCE), 2))
    out = {"in_ids": np.array([r[0] for r in recs]), "in_desc": np.array([r[1] for r in recs]),
           "in_seq": np.array([r[2] for r in recs]), "abundance_names": np.array(ABUNDANCE), "abundance_raw": raw,
           "seeds": np.array(SEEDS), "threshold": np.int64(THRESHOLD), "split_len": np.int64(SPLIT_LEN)}
    for ks in K_LISTS:
        with tempfile.TemporaryDirectory() as td:
            td = Path(td)
            with open(td / "in.fa", "w") as fh:
                for ident, desc, seq in recs:
                    fh.write(">" + ident + " " + desc + "\n")
                    for i in range(0, len(seq), 70):
                        fh.write(seq[i:i + 70] + "\n")
            with open(td / "abund.tsv", "w") as fh:
                for name, row in zip(ABUNDANCE, raw):
                    fh.write(name + "\t" + "\t".join(repr(float(v)) for v in row) + "\n")
            csv = ref.create_dataset(td / "in.fa", td / "abund.tsv", td / "work", ks, kmer_counter_tool="seq2vec",
                                     short_contig_threshold=THRESHOLD, seed_contig_split_len=SPLIT_LEN)
            header = open(csv).readline().rstrip("\r\n").split(",")
            df = pd.read_csv(csv, float_precision="round_trip")
        dk = sum(_dim(k) for k in ks)
        assert df.shape[1] == 3 + dk + 2, df.shape
        assert header[:3] == ["CONTIG_NAME", "PARENT_NAME", "CLUSTER"]
        # (the stand-in's numbers: the blocks lie side by side in list order, columns ascending, rows = split-FASTA order)
        vals = df.iloc[:, 3:3 + dk].to_numpy()
        want = np.concatenate([1000.0 * k + np.arange(_dim(k)) for k in ks])
        assert np.array_equal(np.floor(vals), np.broadcast_to(want, vals.shape))
        tag = "_".join(str(k) for k in ks)
        out["header_" + tag] = np.array(header)
        out["contig_" + tag] = df["CONTIG_NAME"].to_numpy().astype(str)
        out["parent_" + tag] = df["PARENT_NAME"].to_numpy().astype(str)
        out["cluster_" + tag] = df["CLUSTER"].to_numpy(dtype=np.int64)
        out["coverage_" + tag] = df.iloc[:, 3 + dk:].to_numpy(dtype=np.float64)
        print(tag, df.shape, header[3:6], "...", header[-3:], list(df["CONTIG_NAME"]))
    np.savez_compressed(os.path.join(HERE, "create_dataset.npz"), **out)
    print("written create_dataset.npz")


if __name__ == "__main__":
    main()
