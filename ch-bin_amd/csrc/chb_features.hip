// The k-mer feature calls: chb_kmer_dim through chb_set_samples_from_sequences.
// Defines none of the shared functions of chb_host.h.
#include "chb_host.h"

extern "C" {

int chb_kmer_dim(int k)
{
    const int n = kmer_canonical_table(k, nullptr);
    return n > 0 ? n : fail(CHB_EUNSUPPORTED, "k must be in [1, 7]");
}

int chb_kmer_frequencies(chb_ctx *h, const unsigned char *seq, const int64_t *offsets, int64_t n, int k,
                         double *freq_out, uint32_t *counts_out)
{
    if (!h || !offsets || !freq_out) return fail(CHB_EINVAL, "null argument");
    if (n < 0 || n >= (1LL << 31)) return fail(CHB_EINVAL, "bad contig count");
    std::vector<unsigned short> table;
    const int dim = kmer_canonical_table(k, &table);
    if (dim <= 0) return fail(CHB_EUNSUPPORTED, "k must be in [1, 7]");
    if (n == 0) return CHB_OK;
    if (offsets[0] != 0) return fail(CHB_EINVAL, "offsets[0] must be 0");
    const int64_t total = offsets[n];
    if (total > 0 && !seq) return fail(CHB_EINVAL, "seq is null");
    HIPCHK(hipSetDevice(h->dev));
    // one work item per kmer_chunk_windows() windows of a contig
    const int cw = kmer_chunk_windows();
    std::vector<int> chunk_ptr((size_t)n + 1);
    std::vector<long long> off64((size_t)n + 1);
    int64_t items = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(CHB_EINVAL, "offsets must be non-decreasing");
        chunk_ptr[(size_t)i] = (int)items;
        const int64_t nwin = offsets[i + 1] - offsets[i] - k + 1;
        if (nwin > 0) items += (nwin + cw - 1) / cw;
        if (items >= (1LL << 31) - 1) return fail(CHB_EUNSUPPORTED, "too many bases for one call");
        off64[(size_t)i] = offsets[i];
    }
    chunk_ptr[(size_t)n] = (int)items;
    off64[(size_t)n] = total;
    DevBuf<unsigned char> dseq;
    DevBuf<long long> doff;
    DevBuf<int> dptr;
    DevBuf<unsigned short> dtab;
    DevBuf<unsigned int> dcnt;
    DevBuf<double> dfreq;
    hipStream_t s = h->stream;
    HIPCHK(dseq.ensure((size_t)std::max<int64_t>(total, 1) + 16));
    HIPCHK(doff.ensure((size_t)n + 1));
    HIPCHK(dptr.ensure((size_t)n + 1));
    HIPCHK(dtab.ensure(table.size()));
    HIPCHK(dcnt.ensure((size_t)n * dim));
    HIPCHK(dfreq.ensure((size_t)n * dim));
    if (total > 0) HIPCHK(hipMemcpyAsync(dseq.p, seq, (size_t)total, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(doff.p, off64.data(), sizeof(long long) * (n + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dptr.p, chunk_ptr.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dtab.p, table.data(), sizeof(unsigned short) * table.size(), hipMemcpyHostToDevice, s));
    {
        Timed t(h, "kmer_count", (double)total);
        launch_kmer_count(dseq.p, doff.p, dptr.p, (int)n, (int)items, k, dim, dtab.p, dcnt.p, dfreq.p, s);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(freq_out, dfreq.p, sizeof(double) * (size_t)n * dim, hipMemcpyDeviceToHost, s));
    if (counts_out)
        HIPCHK(hipMemcpyAsync(counts_out, dcnt.p, sizeof(uint32_t) * (size_t)n * dim, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CHB_OK;
}

// ---- k-mer profiles of a list of k values (kmer_multi_kernels.hip)

static int kmer_list_plan(const int *ks, int nk, KmerMultiPlan *plan, std::vector<unsigned short> *table)
{
    if (!ks) return fail(CHB_EINVAL, "null argument");
    const int dim = kmer_multi_plan(ks, nk, plan, table);
    if (dim == -2) return fail(CHB_EUNSUPPORTED, "k must be in [1, 7]");
    if (dim <= 0) return fail(CHB_EINVAL, "ks must hold 1 to 7 distinct values");
    return dim;
}

int chb_kmer_profile_dim(const int *ks, int nk)
{
    KmerMultiPlan plan;
    return kmer_list_plan(ks, nk, &plan, nullptr);
}

// the checks chb_kmer_frequencies makes of its sequence arguments (n > 0)
static int kmer_check_sequences(const unsigned char *seq, const int64_t *offsets, int64_t n)
{
    if (offsets[0] != 0) return fail(CHB_EINVAL, "offsets[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(CHB_EINVAL, "offsets must be non-decreasing");
    if (offsets[n] > 0 && !seq) return fail(CHB_EINVAL, "seq is null");
    return CHB_OK;
}

// Rows [0, n) of the device matrix out[n][ld]: the k-mer blocks of the plan and, with dextra, S more columns behind them.
// The sequence goes up in chunks of whole contigs -- at most kKmerChunkBytes of bases and kKmerChunkRows contigs, a larger
// contig alone -- one after the other on the context's stream, so that sequence, offsets, work-item table, row map and
// counts take the room of one chunk whatever n is.  counts_out (optional, host): the raw counts, [n][total_dim].
// Arguments are checked by the callers; nothing here refuses a call for its values.
static int kmer_profiles_device(chb_ctx *h, const unsigned char *seq, const int64_t *offsets, int64_t n,
                                const KmerMultiPlan &plan, const std::vector<unsigned short> &table, double *out, int64_t ld,
                                const double *dextra, const int64_t *extra_row, int S, uint32_t *counts_out)
{
    const int dim = plan.total_dim;
    const int cw = kmer_multi_chunk_positions();
    // the chunks: [first contig, one past the last)
    std::vector<std::pair<int64_t, int64_t>> chunks;
    int64_t max_bases = 0, max_rows = 0;
    for (int64_t a = 0; a < n;) {
        int64_t b = a + 1;
        while (b < n && b - a < kKmerChunkRows && offsets[b + 1] - offsets[a] <= kKmerChunkBytes) ++b;
        chunks.emplace_back(a, b);
        max_bases = std::max(max_bases, offsets[b] - offsets[a]);
        max_rows = std::max(max_rows, b - a);
        a = b;
    }
    DevBuf<unsigned char> dseq;
    DevBuf<long long> doff, dxrow;
    DevBuf<int> dptr;
    DevBuf<unsigned short> dtab;
    DevBuf<unsigned int> dcnt;
    hipStream_t s = h->stream;
    HIPCHK(dseq.ensure((size_t)std::max<int64_t>(max_bases, 1)));
    HIPCHK(doff.ensure((size_t)max_rows + 1));
    HIPCHK(dptr.ensure((size_t)max_rows + 1));
    if (dextra && extra_row) HIPCHK(dxrow.ensure((size_t)max_rows));
    HIPCHK(dtab.ensure(table.size()));
    HIPCHK(dcnt.ensure((size_t)max_rows * dim));
    HIPCHK(hipMemcpyAsync(dtab.p, table.data(), sizeof(unsigned short) * table.size(), hipMemcpyHostToDevice, s));
    std::vector<int> item_ptr;
    std::vector<long long> off64, xrow;
    h->kmer_chunks = 0;
    for (const auto &c : chunks) {
        const int64_t a = c.first, rows = c.second - c.first, base0 = offsets[a], bases = offsets[c.second] - base0;
        // one work item per cw start positions of a contig, of the L - kmin + 1 that begin a k-mer of the list
        item_ptr.assign((size_t)rows + 1, 0);
        off64.assign((size_t)rows + 1, 0);
        int64_t items = 0;
        for (int64_t i = 0; i < rows; ++i) {
            item_ptr[(size_t)i] = (int)items;
            off64[(size_t)i] = offsets[a + i] - base0;
            const int64_t nstart = offsets[a + i + 1] - offsets[a + i] - plan.kmin + 1;
            if (nstart > 0) items += (nstart + cw - 1) / cw;
            if (items >= (1LL << 31) - 1) return fail(CHB_EUNSUPPORTED, "a contig is too long for one call");
        }
        item_ptr[(size_t)rows] = (int)items;
        off64[(size_t)rows] = bases;
        if (bases > 0) HIPCHK(hipMemcpyAsync(dseq.p, seq + base0, (size_t)bases, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(doff.p, off64.data(), sizeof(long long) * (rows + 1), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dptr.p, item_ptr.data(), sizeof(int) * (rows + 1), hipMemcpyHostToDevice, s));
        if (dextra && extra_row) {
            xrow.assign(extra_row + a, extra_row + a + rows);
            HIPCHK(hipMemcpyAsync(dxrow.p, xrow.data(), sizeof(long long) * rows, hipMemcpyHostToDevice, s));
        }
        {
            Timed t(h, "kmer_multi", (double)bases);
            launch_kmer_multi(dseq.p, doff.p, dptr.p, (int)rows, (int)items, plan, dtab.p, dcnt.p, out + (size_t)a * ld, ld,
                              dextra, dextra && extra_row ? dxrow.p : nullptr, a, S, s);
        }
        HIPCHK(hipGetLastError());
        if (counts_out)
            HIPCHK(hipMemcpyAsync(counts_out + (size_t)a * dim, dcnt.p, sizeof(uint32_t) * (size_t)rows * dim,
                                  hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));   // (the host tables and the chunk's device buffers are reused by the next chunk)
        ++h->kmer_chunks;
    }
    return CHB_OK;
}

int chb_kmer_profiles(chb_ctx *h, const unsigned char *seq, const int64_t *offsets, int64_t n, const int *ks, int nk,
                      double *freq_out, uint32_t *counts_out)
{
    if (!h || !offsets || !freq_out) return fail(CHB_EINVAL, "null argument");
    if (n < 0 || n >= (1LL << 31)) return fail(CHB_EINVAL, "bad contig count");
    KmerMultiPlan plan;
    std::vector<unsigned short> table;
    const int dim = kmer_list_plan(ks, nk, &plan, &table);
    if (dim <= 0) return dim;
    if (n == 0) return CHB_OK;
    { const int rc = kmer_check_sequences(seq, offsets, n); if (rc) return rc; }
    HIPCHK(hipSetDevice(h->dev));
    DevBuf<double> dfreq;
    HIPCHK(dfreq.ensure((size_t)n * dim));
    { const int rc = kmer_profiles_device(h, seq, offsets, n, plan, table, dfreq.p, dim, nullptr, nullptr, 0, counts_out); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(freq_out, dfreq.p, sizeof(double) * (size_t)n * dim, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CHB_OK;
}

int chb_set_samples_from_sequences(chb_ctx *h, const unsigned char *seq, const int64_t *offsets, int64_t n, const int *ks,
                                   int nk, const double *extra, int64_t n_extra, int64_t S, const int64_t *extra_row,
                                   double *X_out)
{
    // every check before anything is enqueued: a refused call leaves the resident samples as they were
    if (!h || !offsets) return fail(CHB_EINVAL, "null argument");
    if (n <= 0 || n >= (1LL << 31) - 64) return fail(CHB_EINVAL, "bad contig count");
    KmerMultiPlan plan;
    std::vector<unsigned short> table;
    const int dim = kmer_list_plan(ks, nk, &plan, &table);
    if (dim <= 0) return dim;
    { const int rc = kmer_check_sequences(seq, offsets, n); if (rc) return rc; }
    if (S < 0) return fail(CHB_EINVAL, "bad number of extra columns");
    if (S > (1 << 20) - dim) return fail(CHB_EUNSUPPORTED, "N or D too large");
    if (S > 0 && !extra) return fail(CHB_EINVAL, "extra is null");
    if (S == 0 && extra) return fail(CHB_EINVAL, "extra given without columns");
    if (S > 0) {
        if (n_extra <= 0) return fail(CHB_EINVAL, "extra has no rows");
        if (!extra_row && n_extra != n) return fail(CHB_EINVAL, "extra needs one row per contig when there is no extra_row");
        if (extra_row)
            for (int64_t i = 0; i < n; ++i)
                if (extra_row[i] < 0 || extra_row[i] >= n_extra) return fail(CHB_EINVAL, "extra_row out of range");
    }
    const int64_t D = dim + S;
    HIPCHK(hipSetDevice(h->dev));
    DevBuf<double> mat, dextra;
    HIPCHK(mat.ensure((size_t)n * D));
    if (S > 0) {
        HIPCHK(dextra.ensure((size_t)n_extra * S));
        HIPCHK(hipMemcpyAsync(dextra.p, extra, sizeof(double) * (size_t)n_extra * S, hipMemcpyHostToDevice, h->stream));
    }
    { const int rc = kmer_profiles_device(h, seq, offsets, n, plan, table, mat.p, D, S > 0 ? dextra.p : nullptr, extra_row, (int)S, nullptr); if (rc) return rc; }
    if (X_out) {
        HIPCHK(hipMemcpyAsync(X_out, mat.p, sizeof(double) * (size_t)n * D, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    // from here on the matrix is a device matrix like any other: chb_set_samples_device's own routine (padded resident
    // copy, shadow rows, an open stepwise fit ended; it returns with the stream drained, before `mat` is freed)
    return set_samples_common(h, mat.p, n, D, true);
}

}  // extern "C"
