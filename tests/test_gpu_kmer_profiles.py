"""K-mer profiles of a LIST of k values counted in one pass (chb_kmer_profiles), the resident path that builds the feature
matrix on the device (chb_set_samples_from_sequences) and the features-stage mirror on top of them.

References: the oracle restatement, one k at a time and stacked (`np.hstack`), and the existing single-k entry point
chb_kmer_frequencies, which uploads everything in one piece -- the independent formulation for the chunked upload at sizes
where the oracle is too slow to be worth it.  Counts are integers and a frequency is one double division of them: every
comparison is for equality."""
import os

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K_LISTS = [[4], [4, 5], [5, 4], [3, 4, 5], [1, 7], [6, 7], [1, 2, 3, 4, 5, 6, 7]]


@pytest.fixture(scope="module")
def ctx():
    import chbin_amd  # noqa: F401
    from chbin_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _random_bases(rng, n):
    return ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]


def _random_contigs(rng, lengths, dirty=True):
    out = []
    for n in lengths:
        s = _random_bases(rng, n)
        if dirty and n > 20:
            s[rng.integers(0, n, size=max(1, n // 300))] = ord("N")
            lo = rng.integers(0, n - 10)
            s[lo:lo + 10] |= 0x20   # a soft-masked (lower case) run
        out.append(s.tobytes())
    return out


def _oracle_stack(O, seqs, ks):
    parts = [O.kmer_frequencies(seqs, k) for k in ks]
    return np.hstack([p[0] for p in parts]), np.hstack([p[1] for p in parts])


@pytest.mark.parametrize("ks", K_LISTS, ids=lambda ks: "-".join(map(str, ks)))
def test_profiles_match_oracle_and_single_k_calls(ctx, O, ks):
    kmin, kmax = min(ks), max(ks)
    rng = np.random.default_rng(1000 + 10 * kmax + kmin + len(ks))
    lengths = [0, 1, kmin - 1, kmin, kmax - 1, kmax, kmax + 1, 50, 4095, 4096, 4097, 4096 + kmin - 1, 4096 + kmax - 1,
               9000, 40000]
    seqs = _random_contigs(rng, lengths)
    seqs += [b"N" * 500, b"ACGT" * 2000, b"a" * 4100 + b"T" * 4100, b"acgtacgtacgttgca" * 30]
    # a single N at each of the last kmax positions in turn: a small k still has a window in front of it (or behind it),
    # a large one must not count what the prefix of its code would suggest
    for tail in (60, 4096 + kmax):   # (... in the middle of a work item, and where the next item begins)
        for p in range(kmax):
            s = _random_bases(rng, tail)
            s[tail - 1 - p] = ord("N")
            seqs.append(s.tobytes())
    freq, counts = ctx.kmer_profiles(seqs, ks, return_counts=True)
    want_f, want_c = _oracle_stack(O, seqs, ks)
    assert freq.shape == want_f.shape == (len(seqs), sum(O.kmer_dim(k) for k in ks))
    assert np.array_equal(counts.astype(np.int64), want_c)
    assert np.array_equal(freq, want_f)
    assert np.array_equal(freq, np.hstack([ctx.kmer_frequencies(seqs, k) for k in ks]))
    assert np.array_equal(ctx.kmer_profiles(seqs, ks), freq)   # (without the counts)
    assert ctx.counter("kmer_chunks") == 1


def test_many_small_contigs_take_two_chunks(ctx, O):
    rng = np.random.default_rng(21)
    assert ctx.counter("kmer_chunk_rows") == 16384 and ctx.counter("kmer_chunk_bytes") == 32 << 20
    seqs = _random_contigs(rng, rng.integers(30, 61, size=16384 + 5))
    freq, counts = ctx.kmer_profiles(seqs, [3, 4], return_counts=True)
    assert ctx.counter("kmer_chunks") == 2
    want_f, want_c = _oracle_stack(O, seqs, [3, 4])
    assert np.array_equal(counts.astype(np.int64), want_c) and np.array_equal(freq, want_f)


@pytest.mark.parametrize("sizes,chunks", [((12 << 20, 12 << 20, 12 << 20), 2), ((5000, 40 << 20, 7000), 3)],
                         ids=["3x12MiB", "40MiB-between-small"])
def test_large_contigs_are_chunked_like_one_upload(ctx, sizes, chunks):
    rng = np.random.default_rng(sum(sizes) % 1000)
    seqs = []
    for n in sizes:
        s = _random_bases(rng, n)
        s[rng.integers(0, n, size=50)] = ord("N")
        seqs.append(s.tobytes())
    freq, counts = ctx.kmer_profiles(seqs, [4], return_counts=True)
    assert ctx.counter("kmer_chunks") == chunks
    want_f, want_c = ctx.kmer_frequencies(seqs, 4, return_counts=True)   # everything in one upload
    assert np.array_equal(counts, want_c) and np.array_equal(freq, want_f)
    # (every window is there: a contig has L - 3 of them, and each of its 50 N takes at most 4 away)
    assert int(counts.sum()) >= sum(sizes) - 3 * len(sizes) - 4 * 50 * len(sizes)


@pytest.fixture(scope="module")
def resident_case(O):
    """300 contigs of 2-6 kb from four base compositions, two coverage columns of 90 parents, a map that is not the
    identity and gives several rows the same parent; the matrix the oracle says they make for ks = [3, 4]."""
    rng = np.random.default_rng(77)
    comp = np.array([[.40, .10, .10, .40], [.15, .35, .35, .15], [.25, .25, .25, .25], [.10, .40, .20, .30]])
    true = rng.integers(0, 4, size=300)
    seqs = [ACGT[rng.choice(4, size=int(rng.integers(2000, 6001)), p=comp[t])].tobytes() for t in true]
    extra = rng.random((90, 2))
    extra_row = rng.integers(0, 90, size=300)
    assert len(set(extra_row.tolist())) < 300 and not np.array_equal(extra_row[:90], np.arange(90))
    X = np.hstack([_oracle_stack(O, seqs, [3, 4])[0], extra[extra_row]])
    return seqs, extra, extra_row, true, X


def test_resident_matrix_is_the_oracle_stack(ctx, resident_case):
    seqs, extra, extra_row, _true, X = resident_case
    got = ctx.set_samples_from_sequences(seqs, [3, 4], extra=extra, extra_row=extra_row, return_matrix=True)
    assert got.shape == (300, 32 + 136 + 2) and (ctx.N, ctx.D) == got.shape
    assert np.array_equal(got, X)
    d_seq = ctx.pairwise_distance(0, 8)
    ctx.set_samples(X)
    assert np.array_equal(d_seq, ctx.pairwise_distance(0, 8))
    # without a map: row i of extra for contig i; without extra columns: the k-mer blocks alone
    got = ctx.set_samples_from_sequences(seqs[:90], [3, 4], extra=extra, return_matrix=True)
    assert np.array_equal(got, np.hstack([X[:90, :168], extra]))
    got = ctx.set_samples_from_sequences(seqs[:20], [4, 3], return_matrix=True)
    assert np.array_equal(got, np.hstack([X[:20, 32:168], X[:20, :32]])) and ctx.D == 168


def test_fit_on_resident_path_equals_fit_on_uploaded_matrix(ctx, resident_case):
    from chbin_amd import synth
    seqs, extra, extra_row, true, X = resident_case
    B, m, sweeps = 4, 5, 2
    initial = np.full(300, -1, dtype=np.int64)
    for b in range(B):
        initial[np.where(true == b)[0][:10]] = b   # ten seeds per bin
    perms = synth.draw_permutations(initial, sweeps, seed=0)
    assert ctx.set_samples_from_sequences(seqs, [3, 4], extra=extra, extra_row=extra_row) is None
    lab_a, its_a, changed_a = ctx.fit_cluster(B, initial, perms, m, sweeps)
    ctx.set_samples(X)
    lab_b, its_b, changed_b = ctx.fit_cluster(B, initial, perms, m, sweeps)
    assert np.array_equal(lab_a, lab_b) and its_a == its_b and np.array_equal(changed_a, changed_b)
    assert (lab_a >= 0).all() and len(set(lab_a.tolist())) == B


def test_refused_calls(ctx, resident_case):
    from chbin_amd._lib import ChbError
    seqs, extra, extra_row, _true, X = resident_case
    ctx.set_samples(X)
    before = ctx.pairwise_distance(0, 8)
    bad_row = extra_row.copy()
    bad_row[17] = 90
    neg_row = extra_row.copy()
    neg_row[0] = -1
    refused = [dict(ks=[4, 4]), dict(ks=[4, 8]), dict(ks=[]), dict(ks=[0]), dict(ks=[1, 2, 3, 4, 5, 6, 7, 3]),
               dict(ks=[3, 4], extra=extra, extra_row=bad_row), dict(ks=[3, 4], extra=extra, extra_row=neg_row),
               dict(ks=[3, 4], extra=extra[:50])]   # (no map: extra needs one row per contig)
    for kw in refused:
        with pytest.raises(ChbError):
            ctx.set_samples_from_sequences(seqs, **kw)
        assert (ctx.N, ctx.D) == X.shape
    assert np.array_equal(ctx.pairwise_distance(0, 8), before)   # the resident matrix is still the one from before
    for ks in ([4, 4], [8], [], [1, 2, 3, 4, 5, 6, 7, 1]):
        with pytest.raises(ChbError):
            ctx.kmer_profiles(seqs[:3], ks)
    assert ctx.kmer_profiles([], [4, 5]).shape == (0, 648)   # n = 0: nothing to do
    f, c = ctx.kmer_profiles([], [3, 4, 5], return_counts=True)
    assert f.shape == c.shape == (0, 680)


@pytest.mark.parametrize("ks", [[4], [4, 5]], ids=["4", "4-5"])
def test_create_dataset_mirror_on_the_gpu(ctx, O, tmp_path, ks):
    from chbin_amd import cli_clustering, cli_features
    from chbin_amd.features import fasta
    g = np.load(os.path.join(GOLD, "create_dataset.npz"))
    fa, cov = tmp_path / "contigs.fasta", tmp_path / "abundance.tsv"
    with open(fa, "w") as fh:
        for ident, desc, seq in zip(g["in_ids"].tolist(), g["in_desc"].tolist(), g["in_seq"].tolist()):
            fasta.write_record(fh, ident, seq, description=desc, width=70)
    with open(cov, "w") as fh:
        for name, row in zip(g["abundance_names"].tolist(), g["abundance_raw"]):
            fh.write(name + "\t" + "\t".join(repr(float(v)) for v in row) + "\n")
    kw = dict(kmer_counter_tool="seq2vec", short_contig_threshold=int(g["threshold"]),
              seed_contig_split_len=int(g["split_len"]), seed_clusters=g["seeds"].tolist())
    csv = cli_features.create_dataset(fa, cov, tmp_path / "work", ks, **kw)
    tag = "_".join(str(k) for k in ks)
    assert open(csv).readline().rstrip("\r\n").split(",") == g["header_" + tag].tolist()
    df = pd.read_csv(csv, float_precision="round_trip")
    assert df["CONTIG_NAME"].tolist() == g["contig_" + tag].tolist()
    assert df["PARENT_NAME"].tolist() == g["parent_" + tag].tolist()
    assert np.array_equal(df["CLUSTER"].to_numpy(), g["cluster_" + tag])
    dk = sum(O.kmer_dim(k) for k in ks)
    rows = {i: s for i, _d, s in fasta.read_fasta(tmp_path / "work" / "split-contigs.fasta")}
    want = _oracle_stack(O, [rows[n] for n in df["CONTIG_NAME"]], ks)[0]
    assert np.array_equal(df.iloc[:, 3:3 + dk].to_numpy(), want)
    assert np.array_equal(df.iloc[:, 3 + dk:].to_numpy(), g["coverage_" + tag])
    # the same rows as resident samples, built on the device
    names, parents, initial = cli_features.assemble_samples(fa, cov, tmp_path / "work2", ks, **kw)
    assert names == df["CONTIG_NAME"].tolist() and parents == df["PARENT_NAME"].tolist()
    assert np.array_equal(initial, g["cluster_" + tag]) and (ctx.N, ctx.D) == (len(names), dk + 2)
    d_dev = ctx.pairwise_distance()
    ctx.set_samples(df.iloc[:, 3:].to_numpy())
    assert np.array_equal(d_dev, ctx.pairwise_distance())
    # ... and the clustering stage reads the file
    out = cli_clustering.perform_clustering(fa, csv, tmp_path / "bins", num_neighbors=2, max_iterations=2)
    bins = pd.read_csv(out)
    assert bins["CONTIG_NAME"].tolist() == sorted(set(g["parent_" + tag].tolist()))
    assert set(bins["BIN"]) <= {0, 1, 2}
