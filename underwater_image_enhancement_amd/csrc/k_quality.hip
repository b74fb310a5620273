// quality_assessment.QualityAssessment (quality_assessment.py:15-286): the eight no-reference scores and their weighted
// sum, as device reductions, so that picking the best of N strategies (main.py:130-146) does not leave the GPU.
//   k_qa_maps    one pass over the quantised frame: gray plane (RGB2GRAY), histograms of gray, HSV saturation and LAB
//                lightness, and the four colourfulness sums: exact integer sums of r - g and r + g - 2b when the frame is
//                u8 / 255, one float64 partial per block from the float image when one is given
//   k_qa_lap     3x3 Laplacian of the gray plane (BORDER_REFLECT_101) as exact integer sums of l and l*l
//   Canny        the quadtree's kernels on one full-frame region per image -> edge count
//   k_qa_finish  scores in float64 from the histograms / sums
// Integer-derived quantities (gray, S, L, Canny, the threshold counts) are exact.  The floating statistics are
// evaluated in float64 from histograms and exact integer sums instead of NumPy's float32 pairwise sums, and the
// Laplacian uses l/255 for the sum of float32(g/255) terms: 2e-3 on the 0..100 scores against the float32 oracle
// (tests/test_gpu_stages.py); the measured distance of that oracle from a float64 evaluation is in DESIGN.md section 2.
// Against the float64 evaluation (tests/quality_ref.py) every score of a u8 frame is held to 1e-9; colourfulness from a
// float image reads float32 values and is held to twice the oracle's own measured distance (tests/test_gpu_quality.py).
// Determinism: every cross-block sum is an integer atomic (exact in any order) or a per-block partial that k_qa_finish
// adds in block order, and the grid depends on the frame size only.  The scores of a frame are therefore the same bits
// in every run, at every position of every batch; for a u8 frame they do not depend on the grid either.  A NaN in the
// float image gives NaN colourfulness and a NaN total, like np.clip and the reference's weighted sum.
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

constexpr int kQaScores = 9;  // contrast, sharpness, entropy, saturation, brightness, edge_density, colorfulness, naturalness, total

struct QaWeights {
    double w[8];
};

// grid (nblk, B), block 256.  hist: [B][3][256] (gray, S, L).  The colourfulness sums (rg, yb, rg^2, yb^2) go to
// cpart: [B][nblk][4] doubles, one row per block, when fimg is given; else to isum: [B][4] int64 of 255 * rg = r - g and
// 510 * yb = r + g - 2b (|sum of squares| <= 510^2 * npx: 64 bits hold any frame the library takes).
__global__ void __launch_bounds__(256) k_qa_maps(const LabTables *__restrict__ T, const uint8_t *__restrict__ in,
                                                 const float *__restrict__ fimg, int npx, int shift,
                                                 uint8_t *__restrict__ gray, uint32_t *__restrict__ hist,
                                                 double *__restrict__ cpart, unsigned long long *__restrict__ isum)
{
    __shared__ uint32_t h[3][256];
    __shared__ int s_sdiv[256];
    __shared__ uint16_t s_gamma[256], s_cbrt[3072];
    __shared__ int s_fwd[3];
    __shared__ double s_red[4][4];
    __shared__ long long s_ired[4][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 768; i += 256) (&h[0][0])[i] = 0;
    s_sdiv[tid] = tid ? __double2int_rn((double)(255 << 12) / (double)tid) : 0;  // RGB2HSV_b's sdiv_table
    s_gamma[tid] = T->gamma[tid];
    for (int i = tid; i < 3072; i += 256) s_cbrt[i] = T->cbrt[i];
    if (tid < 3) s_fwd[tid] = T->fwd[3 + tid];
    __syncthreads();
    const uint8_t *img = in + (size_t)b * npx * 3;
    const float *fi = fimg ? fimg + (size_t)b * npx * 3 : nullptr;
    uint8_t *g = gray + (size_t)b * npx;
    constexpr int Lscale = (116 * 255 + 50) / 100;
    constexpr int Lshift = -((16 * 255 * (1 << 15) + 50) / 100);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    long long i0 = 0, i1 = 0, i2 = 0, i3 = 0;
    for (int p = blockIdx.x * 256 + tid; p < npx; p += gridDim.x * 256) {
        const uint32_t r = img[(size_t)p * 3], gg = img[(size_t)p * 3 + 1], bl = img[(size_t)p * 3 + 2];
        const uint32_t gv = gray_fixed(r, gg, bl, shift);
        g[p] = (uint8_t)gv;
        const int v = max(max(r, gg), bl), vmin = min(min(r, gg), bl);
        const int sat = ((v - vmin) * s_sdiv[v] + (1 << 11)) >> 12;
        const int R = s_gamma[r], G = s_gamma[gg], Bq = s_gamma[bl];
        const int fY = s_cbrt[(R * s_fwd[0] + G * s_fwd[1] + Bq * s_fwd[2] + (1 << 11)) >> 12];
        const int L = min(max((Lscale * fY + Lshift + (1 << 14)) >> 15, 0), 255);
        atomicAdd(&h[0][gv], 1u);
        atomicAdd(&h[1][sat], 1u);
        atomicAdd(&h[2][L], 1u);
        if (fi) {
            const float fr = fi[(size_t)p * 3], fg = fi[(size_t)p * 3 + 1], fb = fi[(size_t)p * 3 + 2];
            const float rg = fr - fg, yb = 0.5f * (fr + fg) - fb;  // quality_assessment.py:158-159
            a0 += (double)rg; a1 += (double)yb; a2 += (double)rg * (double)rg; a3 += (double)yb * (double)yb;
        } else {
            const int rg = (int)r - (int)gg, yb = (int)r + (int)gg - 2 * (int)bl;
            i0 += rg; i1 += yb; i2 += rg * rg; i3 += yb * yb;
        }
    }
    if (fi) {  // thread, wave and block sums in a fixed order; the blocks' rows are added by k_qa_finish
        a0 = wave_sum_f64(a0); a1 = wave_sum_f64(a1); a2 = wave_sum_f64(a2); a3 = wave_sum_f64(a3);
        if ((tid & 63) == 0) {
            s_red[tid >> 6][0] = a0; s_red[tid >> 6][1] = a1; s_red[tid >> 6][2] = a2; s_red[tid >> 6][3] = a3;
        }
        __syncthreads();
        if (tid < 4)
            cpart[((size_t)b * gridDim.x + blockIdx.x) * 4 + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    } else {
        i0 = (long long)wave_sum_u64((uint64_t)i0); i1 = (long long)wave_sum_u64((uint64_t)i1);
        i2 = (long long)wave_sum_u64((uint64_t)i2); i3 = (long long)wave_sum_u64((uint64_t)i3);
        if ((tid & 63) == 0) {
            s_ired[tid >> 6][0] = i0; s_ired[tid >> 6][1] = i1; s_ired[tid >> 6][2] = i2; s_ired[tid >> 6][3] = i3;
        }
        __syncthreads();
        if (tid < 4)
            atomicAdd(&isum[b * 4 + tid], (unsigned long long)(s_ired[0][tid] + s_ired[1][tid] + s_ired[2][tid] + s_ired[3][tid]));
    }
    for (int i = tid; i < 768; i += 256) {
        const uint32_t c = (&h[0][0])[i];
        if (c) atomicAdd(&hist[(size_t)b * 768 + i], c);
    }
}

// cv2.Laplacian(gray, CV_64F), ksize 1: l = up + down + left + right - 4*centre, BORDER_REFLECT_101.  lsum: [B][2] int64.
__global__ void __launch_bounds__(256) k_qa_lap(const uint8_t *__restrict__ gray, int H, int W,
                                                unsigned long long *__restrict__ lsum)
{
    __shared__ long long s_red[4][2];
    const int b = blockIdx.y, tid = threadIdx.x, npx = H * W;
    const uint8_t *g = gray + (size_t)b * npx;
    long long s1 = 0, s2 = 0;
    for (int p = blockIdx.x * 256 + tid; p < npx; p += gridDim.x * 256) {
        const int y = p / W, x = p - y * W;
        const int yu = y > 0 ? y - 1 : (H > 1 ? 1 : 0), yd = y + 1 < H ? y + 1 : (H > 1 ? H - 2 : 0);
        const int xl = x > 0 ? x - 1 : (W > 1 ? 1 : 0), xr = x + 1 < W ? x + 1 : (W > 1 ? W - 2 : 0);
        const int l = (int)g[yu * W + x] + g[yd * W + x] + g[y * W + xl] + g[y * W + xr] - 4 * (int)g[p];
        s1 += l;
        s2 += (long long)l * l;
    }
    s1 = (long long)wave_sum_u64((uint64_t)s1);
    s2 = (long long)wave_sum_u64((uint64_t)s2);
    if ((tid & 63) == 0) { s_red[tid >> 6][0] = s1; s_red[tid >> 6][1] = s2; }
    __syncthreads();
    if (tid < 2)
        atomicAdd(&lsum[b * 2 + tid], (unsigned long long)(s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid]));
}

// np.clip(v, 0, 100): a NaN stays a NaN (fmin / fmax alone would turn it into 0)
__device__ __forceinline__ double clip100(double v) { return v != v ? v : fmin(fmax(v, 0.0), 100.0); }

// grid B, block 64: the wave adds the blocks' colourfulness rows (lane l takes rows l, l + 64, ... in that order, then a
// fixed butterfly), lane 0 evaluates the scores.  nblk == 0: the integer sums of a u8 frame are in isum instead.
__global__ void __launch_bounds__(64) k_qa_finish(const uint32_t *__restrict__ hist, const double *__restrict__ cpart, int nblk,
                                                  const unsigned long long *__restrict__ isum,
                                                  const unsigned long long *__restrict__ lsum, const uint32_t *__restrict__ edges,
                                                  int npx, QaWeights wt, double *__restrict__ out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < nblk; k += 64) {
        const double *row = cpart + ((size_t)b * nblk + k) * 4;
        cs[0] += row[0]; cs[1] += row[1]; cs[2] += row[2]; cs[3] += row[3];
    }
    if (nblk)
        for (int i = 0; i < 4; ++i) cs[i] = wave_sum_f64(cs[i]);
    if (lane) return;
    const uint32_t *hg = hist + (size_t)b * 768, *hs = hg + 256, *hl = hg + 512;
    const double n = (double)npx;
    double mg = 0.0, ms = 0.0, mL = 0.0, ent = 0.0, dark = 0.0, bright = 0.0, oversat = 0.0;
    for (int k = 0; k < 256; ++k) {
        const float xf = px_norm(k);  // the float32 value NumPy holds for this byte
        mg += (double)hg[k] * (double)xf;
        ms += (double)hs[k] * (double)xf;
        mL += (double)hl[k] * (double)k;
        if (hg[k]) {
            const double pk = (double)hg[k] / n;
            ent -= pk * log(pk);
        }
        if (xf < 0.1f) dark += hg[k];
        if (xf > 0.9f) bright += hg[k];
        if (xf > 0.9f) oversat += hs[k];
    }
    mg /= n; ms /= n; mL /= n;
    double vg = 0.0;
    for (int k = 0; k < 256; ++k) {
        const double d = (double)px_norm(k) - mg;
        vg += (double)hg[k] * d * d;
    }
    vg /= n;
    const double l1 = (double)(long long)lsum[b * 2], l2 = (double)(long long)lsum[b * 2 + 1];
    const double vlap = (l2 - l1 * l1 / n) / n / (255.0 * 255.0);
    double mrg, myb, vrg, vyb;
    if (nblk) {
        mrg = cs[0] / n; myb = cs[1] / n;
        vrg = cs[2] / n - mrg * mrg; vyb = cs[3] / n - myb * myb;
        vrg = vrg < 0.0 ? 0.0 : vrg; vyb = vyb < 0.0 ? 0.0 : vyb;  // keeps a NaN
    } else {
        const long long *is = reinterpret_cast<const long long *>(isum) + b * 4;
        mrg = (double)is[0] / (255.0 * n); myb = (double)is[1] / (510.0 * n);
        vrg = int_variance(is[0], is[2], npx) / (255.0 * 255.0); vyb = int_variance(is[1], is[3], npx) / (510.0 * 510.0);
    }
    double sc[8];
    sc[0] = clip100(sqrt(vg) / 0.5 * 100.0);                                        // quality_assessment.py:25-31
    sc[1] = clip100(vlap / 0.5 * 100.0);                                            // :45-52
    sc[2] = clip100((ent / log(2.0) - 4.0) / 4.0 * 100.0);                          // :66-73
    sc[3] = clip100(ms * 100.0);                                                    // :87-94
    sc[4] = 100.0 - clip100(fabs(mL - 128.0) / 128.0 * 100.0);                      // :108-117
    sc[5] = clip100((double)edges[b] / n / 0.2 * 100.0);                            // :131-140
    sc[6] = clip100((sqrt(vrg + vyb) + 0.3 * sqrt(mrg * mrg + myb * myb)) / 0.5 * 100.0);  // :154-175
    sc[7] = 100.0 - clip100((oversat / n + dark / n + bright / n) * 200.0);         // :189-205
    double total = 0.0;
    for (int i = 0; i < 8; ++i) {
        out[(size_t)b * kQaScores + i] = sc[i];
        total += sc[i] * wt.w[i];  // quality_assessment.py:283
    }
    out[(size_t)b * kQaScores + 8] = total;
}

struct QaBufs {
    uint8_t *gray;
    uint32_t *hist, *edges;
    double *cpart;
    unsigned long long *isum, *lsum;
    Region *regs;
    void *canny;
};

// blocks per image of k_qa_maps / k_qa_lap: a function of the frame size alone, so a frame's float partials are summed
// in the same order whatever batch it is part of
int qa_blocks(Shape s) { return grid_for(s.npx(), 1024); }

QaBufs carve_qa(Carver &c, Shape s)
{
    QaBufs q;
    q.gray = c.take<uint8_t>((size_t)s.B * s.npx());
    q.hist = c.take<uint32_t>((size_t)s.B * 768);
    q.edges = c.take<uint32_t>(s.B);
    q.cpart = c.take<double>((size_t)s.B * qa_blocks(s) * 4);
    q.isum = c.take<unsigned long long>((size_t)s.B * 4);
    q.lsum = c.take<unsigned long long>((size_t)s.B * 2);
    q.regs = c.take<Region>(s.B);
    q.canny = c.take<char>(canny_ws_bytes(s));
    return q;
}

// main.py:145: best_strategy = max(strategy_scores, key=strategy_scores.get) -- the first maximum in the strategies' order.
// scores: [n][B][ncols], compared on column col (uwie_select_best_u8: 9 columns, the weighted total is entry 8)
__global__ void k_pick_best(const double *__restrict__ scores, int n, int B, int ncols, int col, int32_t *__restrict__ best)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int k = 0;
    double top = scores[(size_t)b * ncols + col];
    for (int i = 1; i < n; ++i) {
        const double v = scores[((size_t)i * B + b) * ncols + col];
        if (v > top) { top = v; k = i; }
    }
    best[b] = k;
}

// out[b] = all[best[b]][b]: 16 bytes per thread (frames are 3 * npx bytes; the tail goes byte by byte)
__global__ void __launch_bounds__(256) k_gather_best(const uint8_t *__restrict__ all, const int32_t *__restrict__ best, size_t frame_bytes,
                                                     int B, uint8_t *__restrict__ out)
{
    const int b = blockIdx.y;
    const uint8_t *src = all + ((size_t)best[b] * B + b) * frame_bytes;
    uint8_t *dst = out + (size_t)b * frame_bytes;
    const size_t n16 = (((size_t)(src - (const uint8_t *)nullptr) | (size_t)(dst - (uint8_t *)nullptr)) & 15) ? 0 : frame_bytes / 16;
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
        reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
    for (size_t i = n16 * 16 + blockIdx.x * 256 + threadIdx.x; i < frame_bytes; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

}  // namespace

int launch_pick_best(const double *d_scores, int n, Shape s, int ncols, int col, const uint8_t *d_all, int32_t *d_best, uint8_t *d_out,
                     hipStream_t st)
{
    UWIE_LAUNCH(k_pick_best, dim3(cdiv(s.B, 64)), dim3(64), 0, st, d_scores, n, s.B, ncols, col, d_best);
    UWIE_LAUNCH_CHECK();
    if (d_out) {
        UWIE_LAUNCH(k_gather_best, dim3(grid_for(s.npx() * 3 / 16 + 1, 1024), s.B), dim3(256), 0, st, d_all, d_best, s.npx() * 3, s.B, d_out);
        UWIE_LAUNCH_CHECK();
    }
    return UWIE_OK;
}

size_t quality_ws_bytes(Shape s)
{
    Carver c(nullptr);
    carve_qa(c, s);
    return c.total();
}

int launch_quality_scores(uwie_ctx *ctx, const uint8_t *d_u8, const float *d_f32, Shape s, int gray_shift,
                          const double *weights8, double *d_scores, void *ws, hipStream_t st)
{
    Carver c(ws);
    QaBufs q = carve_qa(c, s);
    const int npx = (int)s.npx();
    QaWeights wt;
    for (int i = 0; i < 8; ++i) wt.w[i] = weights8[i];
    UWIE_HIP_CHECK(hipMemsetAsync(q.hist, 0, sizeof(uint32_t) * (size_t)s.B * 768, st));
    UWIE_HIP_CHECK(hipMemsetAsync(q.isum, 0, sizeof(unsigned long long) * (size_t)s.B * 4, st));
    UWIE_HIP_CHECK(hipMemsetAsync(q.lsum, 0, sizeof(unsigned long long) * (size_t)s.B * 2, st));
    const dim3 grid(qa_blocks(s), s.B);
    UWIE_LAUNCH(k_qa_maps, grid, dim3(256), 0, st, ctx->d_lab, d_u8, d_f32, npx, gray_shift, q.gray, q.hist, q.cpart, q.isum);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_qa_lap, grid, dim3(256), 0, st, q.gray, s.H, s.W, q.lsum);
    UWIE_LAUNCH_CHECK();
    int rc = launch_make_full_regions(q.regs, s, st);
    if (rc != UWIE_OK) return rc;
    rc = launch_canny(q.gray, s, q.regs, s.B, s.H, s.W, 50, 150, q.edges, nullptr, q.canny, st);
    if (rc != UWIE_OK) return rc;
    UWIE_LAUNCH(k_qa_finish, dim3(s.B), dim3(64), 0, st, q.hist, q.cpart, d_f32 ? (int)grid.x : 0, q.isum, q.lsum, q.edges, npx, wt,
                d_scores);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
