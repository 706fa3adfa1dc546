// Canonical k-mer profiles for a LIST of k values in one counting pass (the reference's KmerK is a comma list,
// cli/features.py:85-92,128: `4,5` gives 648 k-mer columns, `3,4,5` gives 680).
//
// Same conventions as kmer_kernels.hip (column order, base_code's rule for what is a base) and the same shape of work: one
// workgroup per 4096 start positions of a contig, bases -> 2-bit codes staged in LDS once, a histogram in LDS, one global
// atomic per non-zero counter.  What is new is that a start position serves every k of the list: the thread reads the kmax
// codes that follow it once, notes how many of them form an unbroken run of real bases (the run ends at the contig's end or
// at anything but A/C/G/T), and the k-mer of a smaller k is the leading 2k bits of the 2*kmax-bit code.  A k is counted at
// a position iff the run is at least k long -- near a contig's end, or just in front of an N, that holds for the small k of
// a list and not for the large ones.  The histogram covers the columns of all k side by side (block of ks[0], block of
// ks[1], ...: list order, not sorted); the finalise kernel divides every block by its own total, the same double division
// as kmer_normalise_kernel, so a block is bit-identical to what chb_kmer_frequencies returns for that k alone.
#include "chb_internal.h"

#include <algorithm>
#include <vector>

namespace chb {
namespace {

constexpr int kMultiChunk = 4096;          // start positions per workgroup
constexpr int kMultiLdsBytes = 48 * 1024;  // what the histogram copies and the staged codes may take together

__device__ __forceinline__ int base_code(unsigned char ch)
{
    switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return -1;
    }
}

// work item -> (contig, chunk of start positions): item_ptr[i] = first work item of contig i
__global__ __launch_bounds__(256) void kmer_multi_count_kernel(const unsigned char *seq, const long long *offsets,
                                                               const int *item_ptr, int n_contigs, KmerMultiPlan plan,
                                                               const unsigned short *canon, unsigned int *counts)
{
    extern __shared__ unsigned int hist[];   // [copies][total_dim] histograms, then the staged codes
    const int total_dim = plan.total_dim, copies = plan.copies, kmax = plan.kmax;
    signed char *codes = reinterpret_cast<signed char *>(hist + copies * total_dim);   // [kMultiChunk + kmax - 1]
    const int item = blockIdx.x;
    int lo = 0, hi = n_contigs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (item_ptr[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const int ci = lo;
    const long long s0 = offsets[ci], len = offsets[ci + 1] - s0;
    const long long w0 = (long long)(item - item_ptr[ci]) * kMultiChunk;   // first start position of the item
    for (int i = threadIdx.x; i < copies * total_dim; i += 256) hist[i] = 0u;
    // the bases this item can touch; past the contig's end the slot holds "no base", which ends every run there
    const int nslots = kMultiChunk + kmax - 1;
    const int nb = (int)max(0LL, min((long long)nslots, len - w0));
    for (int i = threadIdx.x; i < nslots; i += 256)
        codes[i] = i < nb ? (signed char)base_code(seq[s0 + w0 + i]) : (signed char)-1;
    __syncthreads();
    unsigned int *mine = hist + ((threadIdx.x >> 6) % copies) * total_dim;
    for (int i = threadIdx.x; i < kMultiChunk && i < nb; i += 256) {
        // run = bases of the unbroken run that starts here, capped at kmax; code = their 2-bit codes, first base on top
        int code = 0, run = 0;
        bool ok = true;
        for (int j = 0; j < kmax; ++j) {
            const int b = codes[i + j];
            ok = ok && b >= 0;
            run += ok ? 1 : 0;
            code = (code << 2) | (b & 3);
        }
        for (int q = 0; q < plan.nk; ++q) {
            const int k = plan.k[q];
            if (run >= k) atomicAdd(&mine[plan.col_off[q] + canon[plan.tab_off[q] + (code >> (2 * (kmax - k)))]], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < total_dim; i += 256) {
        unsigned int v = 0;
        for (int c = 0; c < copies; ++c) v += hist[c * total_dim + i];
        if (v) atomicAdd(&counts[(size_t)ci * total_dim + i], v);
    }
}

// out[row][col_off[q] + j] = counts[row][col_off[q] + j] / (sum over the block of ks[q]); a block without a single
// valid window gives zeros.  extra != nullptr: out[row][total_dim + s] = extra[xr][s], xr = extra_row[row] (or, without a
// map, first_row + row).  One wavefront per contig; `out` and `extra_row` begin at the chunk's first row.
__global__ __launch_bounds__(256) void kmer_multi_finalise_kernel(const unsigned int *counts, int n_contigs,
                                                                  KmerMultiPlan plan, double *out, long long ld,
                                                                  const double *extra, const long long *extra_row,
                                                                  long long first_row, int S)
{
    const int lane = threadIdx.x & 63;
    const int ci = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ci >= n_contigs) return;
    const unsigned int *row = counts + (size_t)ci * plan.total_dim;
    double *dst = out + (size_t)ci * (size_t)ld;
    for (int q = 0; q < plan.nk; ++q) {
        const int c0 = plan.col_off[q], dim = plan.dim[q];
        unsigned long long tot = 0;
        for (int j = lane; j < dim; j += 64) tot += row[c0 + j];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) tot += __shfl_xor(tot, off, 64);
        const double t = (double)tot;
        for (int j = lane; j < dim; j += 64) dst[c0 + j] = tot ? (double)row[c0 + j] / t : 0.0;
    }
    if (extra != nullptr) {
        const long long xr = extra_row ? extra_row[ci] : first_row + ci;
        for (int s = lane; s < S; s += 64) dst[plan.total_dim + s] = extra[(size_t)xr * S + s];
    }
}

}  // namespace

int kmer_multi_plan(const int *ks, int nk, KmerMultiPlan *plan, std::vector<unsigned short> *table)
{
    if (!ks || nk < 1 || nk > 7) return -1;
    KmerMultiPlan p{};
    p.nk = nk; p.kmin = 8; p.kmax = 0;
    if (table) table->clear();
    int tab = 0;
    for (int q = 0; q < nk; ++q) {
        for (int r = 0; r < q; ++r) if (ks[r] == ks[q]) return -1;
        std::vector<unsigned short> one;
        const int dim = kmer_canonical_table(ks[q], table ? &one : nullptr);
        if (dim <= 0) return -2;
        p.k[q] = ks[q]; p.dim[q] = dim; p.col_off[q] = p.total_dim; p.tab_off[q] = tab;
        p.total_dim += dim;
        tab += 1 << (2 * ks[q]);
        p.kmin = std::min(p.kmin, ks[q]); p.kmax = std::max(p.kmax, ks[q]);
        if (table) table->insert(table->end(), one.begin(), one.end());
    }
    // one private histogram per wavefront while four of them and the codes fit
    const size_t codes = (size_t)kMultiChunk + p.kmax - 1;
    p.copies = 4 * sizeof(unsigned int) * (size_t)p.total_dim + codes <= (size_t)kMultiLdsBytes ? 4 : 1;
    *plan = p;
    return p.total_dim;
}

int kmer_multi_chunk_positions() { return kMultiChunk; }

void launch_kmer_multi(const unsigned char *seq, const long long *offsets, const int *item_ptr, int n_contigs, int n_items,
                       const KmerMultiPlan &plan, const unsigned short *canon, unsigned int *counts, double *out,
                       long long ld, const double *extra, const long long *extra_row, long long first_row, int S,
                       hipStream_t s)
{
    if (n_contigs <= 0) return;
    (void)hipMemsetAsync(counts, 0, sizeof(unsigned int) * (size_t)n_contigs * plan.total_dim, s);
    const size_t lds = sizeof(unsigned int) * plan.copies * (size_t)plan.total_dim + kMultiChunk + plan.kmax - 1;
    if (n_items > 0)
        hipLaunchKernelGGL(kmer_multi_count_kernel, dim3(n_items), dim3(256), lds, s, seq, offsets, item_ptr, n_contigs,
                           plan, canon, counts);
    hipLaunchKernelGGL(kmer_multi_finalise_kernel, dim3((n_contigs + 3) / 4), dim3(256), 0, s, counts, n_contigs, plan,
                       out, ld, extra, extra_row, first_row, S);
}

}  // namespace chb
