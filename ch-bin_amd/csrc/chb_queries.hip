// The stand-alone queries: chb_pairwise_distance, chb_hull_distance_batch / _points and chb_find_nearest_from_row.
// Defines none of the shared functions of chb_host.h.
#include "chb_host.h"

extern "C" {

int chb_pairwise_distance(chb_ctx *h, int64_t r0, int64_t r1, double *out)
{
    if (!h || !out) return fail(CHB_EINVAL, "null argument");
    if (!h->X.p) return fail(CHB_ESTATE, "chb_set_samples has not been called");
    if (r0 < 0 || r1 > h->N || r0 > r1) return fail(CHB_EINVAL, "row range out of bounds");
    HIPCHK(hipSetDevice(h->dev));
    const int64_t chunk = std::max<int64_t>(64, (int64_t)(1LL << 28) / std::max<int64_t>(h->N, 1));
    DevBuf<double> buf;
    HIPCHK(buf.ensure((size_t)std::min(chunk, r1 - r0) * h->N));
    for (int64_t a = r0; a < r1; a += chunk) {
        const int64_t b = std::min(r1, a + chunk);
        {
            Timed t(h, "pairwise", (double)(b - a) * h->N);
            launch_pairwise(h->X.p, (int)h->N, h->Dp, (int)a, (int)b, buf.p, h->stream);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(out + (a - r0) * h->N, buf.p, sizeof(double) * (b - a) * h->N,
                               hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(CHB_EHIP, hipGetErrorString(e));
    }
    return CHB_OK;
}

static int hull_indexed(chb_ctx *h, const double *Xdev, int D, int Dp, int64_t nrows,
                        const int64_t *query_idx, int64_t P, const int64_t *hull_idx, int m_max,
                        double *dist, double *alpha)
{
    if (m_max < 1 || m_max > CHB_MAX_NEIGHBORS) return fail(CHB_EUNSUPPORTED, "m_max must be in [1, 64]");
    if (P <= 0) return CHB_OK;
    if (m_max > kMaxM && !hull_generic_supported())
        return fail(CHB_EUNSUPPORTED, "more than 16 hull vertices need 68 KB of LDS per workgroup, which this device does not grant");
    hipStream_t s = h->stream;
    // compact each vertex list (padding may sit anywhere at the ABI) and remember the slots
    std::vector<int> q((size_t)P), hx((size_t)P * m_max, -1), slot((size_t)P * m_max, -1), hn((size_t)P, 0);
    for (int64_t p = 0; p < P; ++p) {
        if (query_idx[p] < 0 || query_idx[p] >= nrows) return fail(CHB_EINVAL, "query index out of range");
        q[(size_t)p] = (int)query_idx[p];
        int n = 0;
        for (int a = 0; a < m_max; ++a) {
            const int64_t id = hull_idx[p * m_max + a];
            if (id < 0) continue;
            if (id >= nrows) return fail(CHB_EINVAL, "hull index out of range");
            hx[(size_t)p * m_max + n] = (int)id;
            slot[(size_t)p * m_max + n] = a;
            ++n;
        }
        hn[(size_t)p] = n;
    }
    HIPCHK(h->xq.ensure((size_t)P));
    HIPCHK(h->xhull.ensure((size_t)P * m_max));
    HIPCHK(h->xcnt.ensure((size_t)P));
    HIPCHK(hipMemcpyAsync(h->xcnt.p, hn.data(), sizeof(int) * P, hipMemcpyHostToDevice, s));
    HIPCHK(h->xdist.ensure((size_t)P));
    HIPCHK(h->xalpha.ensure((size_t)P * m_max));
    HIPCHK(hipMemcpyAsync(h->xq.p, q.data(), sizeof(int) * P, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->xhull.p, hx.data(), sizeof(int) * P * m_max, hipMemcpyHostToDevice, s));
    {
        Timed t(h, "hull_qp", (double)P);
        if (m_max > kMaxM)
            launch_hull_generic_indexed(Xdev, D, Dp, h->xq.p, h->xhull.p, h->xcnt.p, (int)P, m_max, h->metric,
                                        h->xdist.p, h->xalpha.p, s);
        else
            launch_hull_qp_indexed(Xdev, D, Dp, h->xq.p, h->xhull.p, h->xcnt.p, (int)P, m_max, h->metric, h->xdist.p,
                                   h->xalpha.p, s);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dist, h->xdist.p, sizeof(double) * P, hipMemcpyDeviceToHost, s));
    std::vector<double> al;
    if (alpha) {
        al.resize((size_t)P * m_max);
        HIPCHK(hipMemcpyAsync(al.data(), h->xalpha.p, sizeof(double) * P * m_max, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (alpha) {
        for (size_t i = 0; i < (size_t)P * m_max; ++i) alpha[i] = 0.0;
        for (int64_t p = 0; p < P; ++p)
            for (int a = 0; a < m_max; ++a) {
                const int sl = slot[(size_t)p * m_max + a];
                if (sl >= 0) alpha[p * m_max + sl] = al[(size_t)p * m_max + a];
            }
    }
    return CHB_OK;
}

int chb_hull_distance_batch(chb_ctx *h, const int64_t *query_idx, int64_t P, const int64_t *hull_idx,
                            int m_max, double *dist, double *alpha)
{
    if (!h || !query_idx || !hull_idx || !dist) return fail(CHB_EINVAL, "null argument");
    if (!h->X.p) return fail(CHB_ESTATE, "chb_set_samples has not been called");
    HIPCHK(hipSetDevice(h->dev));
    return hull_indexed(h, h->X.p, h->D, h->Dp, h->N, query_idx, P, hull_idx, m_max, dist, alpha);
}

int chb_hull_distance_points(chb_ctx *h, const double *x, const double *pts, int m, int64_t D,
                             double *dist, double *alpha)
{
    if (!h || !x || !dist || (m > 0 && !pts)) return fail(CHB_EINVAL, "null argument");
    if (m < 0 || D <= 0) return fail(CHB_EINVAL, "bad m or D");
    if (m == 0) { *dist = INFINITY; return CHB_OK; }
    if (m > CHB_MAX_NEIGHBORS) return fail(CHB_EUNSUPPORTED, "more than 64 hull vertices");
    HIPCHK(hipSetDevice(h->dev));
    const int Dp = (int)((D + kKChunk - 1) / kKChunk) * kKChunk;
    std::vector<double> rows((size_t)(m + 1) * Dp, 0.0);
    memcpy(rows.data(), x, sizeof(double) * D);
    for (int a = 0; a < m; ++a) memcpy(rows.data() + (size_t)(a + 1) * Dp, pts + (size_t)a * D, sizeof(double) * D);
    HIPCHK(h->xpts.ensure(rows.size()));
    HIPCHK(hipMemcpyAsync(h->xpts.p, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, h->stream));
    int64_t q = 0;
    std::vector<int64_t> idx((size_t)m);
    for (int a = 0; a < m; ++a) idx[(size_t)a] = a + 1;
    return hull_indexed(h, h->xpts.p, (int)D, Dp, m + 1, &q, 1, idx.data(), m, dist, alpha);
}

int chb_find_nearest_from_row(chb_ctx *h, int64_t c, const int64_t *labels, const double *row,
                              int64_t N, int m, int64_t *out_idx, int32_t *out_cnt)
{
    if (!h || !labels || !row || !out_idx || !out_cnt) return fail(CHB_EINVAL, "null argument");
    if (N <= 0 || N >= (1LL << 31)) return fail(CHB_EINVAL, "bad N");
    if (m < 1) return fail(CHB_EINVAL, "m must be >= 1");
    HIPCHK(hipSetDevice(h->dev));
    hipStream_t s = h->stream;
    std::vector<int> lab((size_t)N);
    for (int64_t i = 0; i < N; ++i) lab[(size_t)i] = (labels[i] < -1 || labels[i] > 0x7ffffff0) ? -2 : (int)labels[i];
    if (c < 0 || c > 0x7ffffff0) { *out_cnt = 0; for (int i = 0; i < m; ++i) out_idx[i] = -1; return CHB_OK; }
    DevBuf<int> dl, di;
    DevBuf<double> dr;
    hipError_t e = dl.ensure((size_t)N);
    if (e == hipSuccess) e = dr.ensure((size_t)N);
    if (e == hipSuccess) e = di.ensure((size_t)m + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(dl.p, lab.data(), sizeof(int) * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dr.p, row, sizeof(double) * N, hipMemcpyHostToDevice, s);
    std::vector<int> out((size_t)m + 1);
    if (e == hipSuccess) {
        launch_select_row(dl.p, dr.p, (int)N, (int)c, m, di.p, di.p + m, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out.data(), di.p, sizeof(int) * (m + 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(CHB_EHIP, hipGetErrorString(e));
    for (int i = 0; i < m; ++i) out_idx[i] = out[(size_t)i];
    *out_cnt = out[(size_t)m];
    return CHB_OK;
}

}  // extern "C"
