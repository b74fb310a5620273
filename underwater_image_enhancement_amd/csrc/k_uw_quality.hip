// The two no-reference metrics of the underwater-enhancement literature, UCIQE and UIQM, in the fixed form that
// include/uwie.h states (uwie_underwater_scores_u8: 8 x 8 blocks, plain arithmetic, no PLIP operators), as device reductions,
// so that scoring a folder of results and picking the best of N by them does not leave the GPU.
//   k_uwq_stream  one pass over the frame's bytes: OpenCV's 8-bit LAB per pixel -> the histograms of L8 (256 bins), R - G (511)
//                 and R + G - 2B (1021) as LDS atomics added to the frame's global histograms, and three float64 sums per
//                 block: d, d * d and the saturation term, with d = chroma - (chroma of the frame's first pixel)
//   k_uwq_tiles   64 x 32 tiles staged in LDS with a one-pixel halo (BORDER_REFLECT_101 of the frame, so a batch's frames never
//                 see each other): one lane per pixel column of a block row; q = min(gx^2 + gy^2, 65025) * c^2 of the three
//                 channels (Sobel; q <= 65025^2 < 2^32) and the gray byte, block extrema down the column in registers and
//                 across the eight columns by butterflies, the logarithms once per block, four float64 sums per tile
//   k_uwq_finish  per frame: the blocks' and tiles' rows added in their order, the order statistics of L8 and the trimmed
//                 moments of the two colour planes from the histograms (exact integers, int_variance), the eight scores
// What is exact: con_l, UICM's four moments (integers from histograms until the last divisions), every block's extrema and
// which branch it takes.  The three float64 sums of k_uwq_stream are not: sigma_c comes from sum(d) and sum(d * d) with the
// chroma shifted by a value the frame holds, so a frame of one colour has d = 0 throughout and sigma_c = 0 exactly, and the
// cancellation in sum(d * d) / n - (sum(d) / n)^2 costs at most eps * (sigma^2 + m^2) / (2 sigma) with m = mean - shift; the
// shift being one of the n values, sigma >= |m| / sqrt(n), which keeps that below 1e-12 for any frame the library takes.
// (The unshifted form, exact sum(da^2 + db^2) minus the square of a float mean, loses 1e-8 on a flat coloured frame.)
// Determinism as in k_quality.hip: integer atomics, and per-block / per-tile float64 rows that k_uwq_finish adds in row order; the
// grids depend on H and W only, so a frame's eight numbers are the same bits in every run and at every position of every batch.
// The histograms use plain value-indexed LDS words: lane_hist.h's conflict-free layout (32 columns per value) would need 229 KB
// for these 1788 bins.
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

#define UWQ_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

constexpr int kUwL = 0, kUwRG = 256, kUwYB = 256 + 511, kUwBins = 256 + 511 + 1021;
constexpr int kUwHistStride = 1792;  // words per frame in global memory
constexpr int kUwTileW = 64, kUwTileH = 32;
constexpr int kUwRowStride = 3 * (kUwTileW + 2) + 2;  // bytes per staged row of interleaved RGB (198 used), a multiple of 4

struct LabLds {  // what RGB2LAB reads of LabTables (k_clahe.hip rgb2lab_px), in LDS
    uint16_t gamma[256], cbrt[3072];
    int32_t fwd[9];
};

__device__ __forceinline__ void lab_lds_fill(LabLds &S, const LabTables *__restrict__ T, int tid)
{
    S.gamma[tid] = T->gamma[tid];
    for (int i = tid; i < 3072; i += 256) S.cbrt[i] = T->cbrt[i];
    if (tid < 9) S.fwd[tid] = T->fwd[tid];
}

__device__ __forceinline__ void lab8(const LabLds &S, uint32_t r8, uint32_t g8, uint32_t b8, int &L, int &a, int &b)
{
    const int R = S.gamma[r8], G = S.gamma[g8], B = S.gamma[b8];
    const int fX = S.cbrt[UWQ_DESCALE(R * S.fwd[0] + G * S.fwd[1] + B * S.fwd[2], 12)];
    const int fY = S.cbrt[UWQ_DESCALE(R * S.fwd[3] + G * S.fwd[4] + B * S.fwd[5], 12)];
    const int fZ = S.cbrt[UWQ_DESCALE(R * S.fwd[6] + G * S.fwd[7] + B * S.fwd[8], 12)];
    constexpr int Lscale = (116 * 255 + 50) / 100;
    constexpr int Lshift = -((16 * 255 * (1 << 15) + 50) / 100);
    L = sat_u8(UWQ_DESCALE(Lscale * fY + Lshift, 15));
    a = sat_u8(UWQ_DESCALE(500 * (fX - fY) + 128 * (1 << 15), 15));
    b = sat_u8(UWQ_DESCALE(200 * (fY - fZ) + 128 * (1 << 15), 15));
}

// sqrt(da^2 + db^2) of an 8-bit LAB pixel, in float64 (the square is an integer <= 2 * 128^2)
__device__ __forceinline__ double chroma255(int a, int b)
{
    const int da = a - 128, db = b - 128;
    return sqrt((double)(da * da + db * db));
}

// grid (nblk, B), block 256; four pixels per thread and step.  hist: [B][kUwHistStride] (caller zeroes), spart: [B][nblk][4]
// = sum(d), sum(d * d), sum(saturation), 0.  aligned: every group of four pixels starts at a 4-byte address.
__global__ void __launch_bounds__(256) k_uwq_stream(const LabTables *__restrict__ T, const uint8_t *__restrict__ in, int npx, int aligned,
                                                    uint32_t *__restrict__ hist, double *__restrict__ spart)
{
    __shared__ uint32_t h[kUwBins];
    __shared__ LabLds s_lab;
    __shared__ double s_red[4][3];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < kUwBins; i += 256) h[i] = 0;
    lab_lds_fill(s_lab, T, tid);
    __syncthreads();
    const uint8_t *img = in + (size_t)b * npx * 3;
    int L0, a0, b0;
    lab8(s_lab, img[0], img[1], img[2], L0, a0, b0);
    const double c0 = chroma255(a0, b0);  // the shift of sigma_c's sums: a value of this frame
    double sd = 0.0, sd2 = 0.0, ss = 0.0;
    const int ngrp = (npx + 3) >> 2;
    for (int q = blockIdx.x * 256 + tid; q < ngrp; q += gridDim.x * 256) {
        const int n = min(4, npx - 4 * q);
        const Px4 px = load_px4(img + (size_t)q * 12, n, aligned != 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < n) {
                const int r = (int)px.r[i], g = (int)px.g[i], bl = (int)px.b[i];
                int L, la, lb;
                lab8(s_lab, r, g, bl, L, la, lb);
                atomicAdd(&h[kUwL + L], 1u);
                atomicAdd(&h[kUwRG + (r - g + 255)], 1u);
                atomicAdd(&h[kUwYB + (r + g - 2 * bl + 510)], 1u);
                const double c = chroma255(la, lb), d = c - c0;
                sd += d;
                sd2 += d * d;
                ss += L > 0 ? c / (double)L : 0.0;
            }
        }
    }
    // thread, wave and block sums in a fixed order; the blocks' rows are added by k_uwq_finish
    sd = wave_sum_f64(sd); sd2 = wave_sum_f64(sd2); ss = wave_sum_f64(ss);
    if ((tid & 63) == 0) { s_red[tid >> 6][0] = sd; s_red[tid >> 6][1] = sd2; s_red[tid >> 6][2] = ss; }
    __syncthreads();
    if (tid < 4)
        spart[((size_t)b * gridDim.x + blockIdx.x) * 4 + tid] = tid < 3 ? (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]) : 0.0;
    for (int i = tid; i < kUwBins; i += 256) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hist[(size_t)b * kUwHistStride + i], c);
    }
}

// extrema over each group of eight neighbouring lanes (the eight columns of a block)
__device__ __forceinline__ uint32_t oct_max_u32(uint32_t v)
{
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t oct_min_u32(uint32_t v)
{
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
// one row of one channel at column x of the staged tile (interleaved RGB, the halo column first): left, centre, right bytes
// -> d = right - left (gx sums d over three rows as 1 2 1), s = left + 2 centre + right (gy = s below - s above)
struct RowFeat {
    int d, s, c;
};
__device__ __forceinline__ RowFeat row_feat(const uint8_t *row, int x, int ch)
{
    const int l = row[3 * x + ch], c = row[3 * x + 3 + ch], r = row[3 * x + 6 + ch];
    return RowFeat{r - l, l + 2 * c + r, c};
}

// grid (tiles_x * tiles_y, B), block 256.  Tile (tx, ty) covers pixels [64 tx, 64 tx + 64) x [32 ty, 32 ty + 32) = 8 x 4 blocks of
// 8 x 8 pixels.  Wavefront w takes block row w, lane x one pixel column of it: eight rows top to bottom with the two Sobel
// sums of the rows kept in registers, the running extrema of q and gray per column, then three butterfly steps over the
// eight columns of each block.  The 32 blocks' extrema go through LDS to 128 threads, one per (block, term), which evaluate
// the logarithms once and add them in a fixed butterfly.  Only blocks that lie in the frame whole are counted.
// Staged positions outside the frame hold the frame's REFLECT_101 pixels: the Sobel border rule for the pixels of counted
// blocks, and values nobody counts elsewhere; every staged byte is read from inside this frame.
// tpart: [B][tiles][4] = sum of ln(q_max / q_min) for R, G, B, sum of r ln r for gray.
__global__ void __launch_bounds__(256) k_uwq_tiles(const uint8_t *__restrict__ in, int H, int W, int tiles_x, int shift,
                                                   double *__restrict__ tpart)
{
    constexpr int SH = kUwTileH + 2, SC = kUwTileW + 2, RB = 3 * SC;  // staged rows, pixels and bytes per row
    constexpr int DW = RB / 4, ITEMS = DW + (RB - 4 * DW);            // a row as dwords and tail bytes
    __shared__ __attribute__((aligned(16))) uint8_t s[SH][kUwRowStride];
    __shared__ uint32_t s_ext[(kUwTileW / 8) * (kUwTileH / 8)][8];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kUwTileW, y0 = ty * kUwTileH;
    const uint8_t *img = in + (size_t)b * H * W * 3;
    if (x0 >= 1 && x0 + kUwTileW + 1 <= W) {  // no column mirrored: a staged row is RB consecutive bytes of the frame
        for (int i = tid; i < SH * ITEMS; i += 256) {
            const int ly = i / ITEMS, k = i - ly * ITEMS;
            const uint8_t *row = img + ((size_t)reflect101(y0 - 1 + ly, H) * W + (x0 - 1)) * 3;
            if (k < DW) {
                *reinterpret_cast<uint32_t *>(&s[ly][4 * k]) = *reinterpret_cast<const u32_unaligned *>(row + 4 * k);
            } else {
                const int o = 4 * DW + (k - DW);
                s[ly][o] = row[o];
            }
        }
    } else {
        for (int i = tid; i < SH * SC; i += 256) {
            const int ly = i / SC, lx = i - ly * SC;
            const int gy = reflect101(y0 - 1 + ly, H), gx = reflect101(x0 - 1 + lx, W);
            const uint8_t *p = img + ((size_t)gy * W + gx) * 3;
            s[ly][3 * lx] = p[0]; s[ly][3 * lx + 1] = p[1]; s[ly][3 * lx + 2] = p[2];
        }
    }
    __syncthreads();
    // pixel rows 8 wv .. 8 wv + 7 of the tile are staged rows 8 wv + 1 .. 8 wv + 8
    uint32_t qmax[3] = {0u, 0u, 0u}, qmin[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, gmax = 0u, gmin = 255u;
    RowFeat prev[3], cur[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        prev[c] = row_feat(s[8 * wv], lane, c);
        cur[c] = row_feat(s[8 * wv + 1], lane, c);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const RowFeat nxt = row_feat(s[8 * wv + 2 + i], lane, c);
            const int gx = prev[c].d + 2 * cur[c].d + nxt.d, gy = nxt.s - prev[c].s;
            const uint32_t q = (uint32_t)min(gx * gx + gy * gy, 65025) * (uint32_t)(cur[c].c * cur[c].c);  // <= 65025^2 < 2^32
            qmax[c] = max(qmax[c], q);
            qmin[c] = min(qmin[c], q);
            prev[c] = cur[c];
            cur[c] = nxt;
        }
        const uint32_t g = gray_fixed((uint32_t)prev[0].c, (uint32_t)prev[1].c, (uint32_t)prev[2].c, shift);  // this row's centres
        gmax = max(gmax, g);
        gmin = min(gmin, g);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        qmax[c] = oct_max_u32(qmax[c]);
        qmin[c] = oct_min_u32(qmin[c]);
    }
    gmax = oct_max_u32(gmax);
    gmin = oct_min_u32(gmin);
    if ((lane & 7) == 0) {
        uint32_t *e = s_ext[8 * wv + (lane >> 3)];
        e[0] = qmax[0]; e[1] = qmin[0]; e[2] = qmax[1]; e[3] = qmin[1]; e[4] = qmax[2]; e[5] = qmin[2]; e[6] = gmax; e[7] = gmin;
    }
    __syncthreads();
    if (tid < 128) {  // thread = (term, block): wavefront 0 holds R and G, wavefront 1 B and gray
        const int term = tid >> 5, blk = tid & 31, bx = blk & 7, by = blk >> 3;
        const bool counted = (x0 >> 3) + bx < (W >> 3) && (y0 >> 3) + by < (H >> 3);  // a full block of the frame
        const uint32_t hi = s_ext[blk][2 * term], lo = s_ext[blk][2 * term + 1];
        const bool live = counted && (term < 3 ? lo > 0u : hi > lo);
        double v = 0.0;
        if (live) {
            const double x = term < 3 ? (double)hi / (double)lo : (double)(hi - lo) / (double)(hi + lo);
            const double lg = log(x);
            v = term < 3 ? lg : x * lg;
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(v), o));
        if (blk == 0) tpart[((size_t)b * gridDim.x + blockIdx.x) * 4 + term] = v;
    }
}

// One wavefront over a histogram h[0 .. nbins) of the integer values v0 + k: the sums of v and v * v over the sorted positions
// [lo, hi).  Lane l takes a run of bins, an exclusive scan gives the run's first sorted position; exact integers throughout.
__device__ __forceinline__ void hist_range_sums(const uint32_t *__restrict__ h, int nbins, int v0, long long lo, long long hi,
                                                long long &s1, long long &s2)
{
    const int lane = threadIdx.x & 63, per = (nbins + 63) / 64, k0 = min(lane * per, nbins), k1 = min(k0 + per, nbins);
    uint64_t cnt = 0;
    for (int k = k0; k < k1; ++k) cnt += h[k];
    long long cum = (long long)(wave_incl_scan_u64(cnt) - cnt);
    long long a1 = 0, a2 = 0;
    for (int k = k0; k < k1; ++k) {
        const long long c = h[k], from = max(cum, lo), to = min(cum + c, hi);
        if (to > from) {
            const long long v = v0 + k, kept = to - from;
            a1 += kept * v;
            a2 += kept * v * v;
        }
        cum += c;
    }
    s1 = (long long)wave_sum_u64((uint64_t)a1);
    s2 = (long long)wave_sum_u64((uint64_t)a2);
}
// the value at sorted position idx (0 <= idx < the histogram's total)
__device__ __forceinline__ int hist_order_stat(const uint32_t *__restrict__ h, int nbins, long long idx)
{
    const int lane = threadIdx.x & 63, per = (nbins + 63) / 64, k0 = min(lane * per, nbins), k1 = min(k0 + per, nbins);
    uint64_t cnt = 0;
    for (int k = k0; k < k1; ++k) cnt += h[k];
    long long cum = (long long)(wave_incl_scan_u64(cnt) - cnt);
    uint32_t found = 0;
    for (int k = k0; k < k1; ++k) {
        const long long c = h[k];
        if (idx >= cum && idx < cum + c) found = (uint32_t)k;
        cum += c;
    }
    return (int)wave_sum_u32(found);
}

// grid B, block 64.  The wave adds the blocks' and tiles' rows (lane l takes rows l, l + 64, ... in that order, then a fixed
// butterfly) and walks the histograms; every lane evaluates the scores, lane 0 writes them.
__global__ void __launch_bounds__(64) k_uwq_finish(const uint32_t *__restrict__ hist, const double *__restrict__ spart, int nsblk,
                                                   const double *__restrict__ tpart, int ntiles, int H, int W, double *__restrict__ out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double ss[3] = {0.0, 0.0, 0.0}, ts[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < nsblk; k += 64) {
        const double *row = spart + ((size_t)b * nsblk + k) * 4;
        ss[0] += row[0]; ss[1] += row[1]; ss[2] += row[2];
    }
    for (int k = lane; k < ntiles; k += 64) {
        const double *row = tpart + ((size_t)b * ntiles + k) * 4;
        ts[0] += row[0]; ts[1] += row[1]; ts[2] += row[2]; ts[3] += row[3];
    }
    for (int i = 0; i < 3; ++i) ss[i] = wave_sum_f64(ss[i]);
    for (int i = 0; i < 4; ++i) ts[i] = wave_sum_f64(ts[i]);
    const uint32_t *hf = hist + (size_t)b * kUwHistStride;
    const long long npx = (long long)H * W, t = npx / 10, m = npx - 2 * t;
    const int l_lo = hist_order_stat(hf + kUwL, 256, npx / 100);
    const int l_hi = hist_order_stat(hf + kUwL, 256, min(99 * npx / 100, npx - 1));
    long long rg1, rg2, yb1, yb2;
    hist_range_sums(hf + kUwRG, 511, -255, t, npx - t, rg1, rg2);
    hist_range_sums(hf + kUwYB, 1021, -510, t, npx - t, yb1, yb2);
    const double n = (double)npx, md = ss[0] / n;
    double sc[kUwScores];
    sc[0] = sqrt(fmax(ss[1] / n - md * md, 0.0)) / 255.0;
    sc[1] = (double)(l_hi - l_lo) / 255.0;
    sc[2] = ss[2] / n;
    sc[3] = 0.4680 * sc[0] + 0.2745 * sc[1] + 0.2576 * sc[2];
    const double mu_rg = (double)rg1 / (double)m, mu_yb = (double)yb1 / (double)m / 2.0;
    const double var_rg = int_variance(rg1, rg2, m), var_yb = int_variance(yb1, yb2, m) / 4.0;
    sc[4] = -0.0268 * sqrt(mu_rg * mu_rg + mu_yb * mu_yb) + 0.1586 * sqrt(var_rg + var_yb);
    const long long nblk = (long long)(H >> 3) * (W >> 3);
    const double nb = (double)nblk;
    sc[5] = nblk ? 0.299 * (ts[0] / nb) + 0.587 * (ts[1] / nb) + 0.114 * (ts[2] / nb) : 0.0;
    sc[6] = nblk ? -(ts[3] / nb) : 0.0;
    sc[7] = 0.0282 * sc[4] + 0.2953 * sc[5] + 3.5753 * sc[6];
    if (lane == 0)
        for (int i = 0; i < kUwScores; ++i) out[(size_t)b * kUwScores + i] = sc[i];
}

struct UwBufs {
    uint32_t *hist;
    double *spart, *tpart;
};

// blocks of k_uwq_stream and tiles of k_uwq_tiles per frame: functions of the frame size alone, so a frame's float rows are
// summed in the same order whatever batch it is part of
int uwq_stream_blocks(Shape s) { return grid_for((s.npx() + 3) / 4, 1024); }
int uwq_tiles_x(Shape s) { return cdiv(s.W, kUwTileW); }
int uwq_tiles(Shape s) { return uwq_tiles_x(s) * cdiv(s.H, kUwTileH); }

UwBufs carve_uwq(Carver &c, Shape s)
{
    UwBufs u;
    u.hist = c.take<uint32_t>((size_t)s.B * kUwHistStride);
    u.spart = c.take<double>((size_t)s.B * uwq_stream_blocks(s) * 4);
    u.tpart = c.take<double>((size_t)s.B * uwq_tiles(s) * 4);
    return u;
}

}  // namespace

void underwater_tile(int *tile_w, int *tile_h)
{
    *tile_w = kUwTileW;
    *tile_h = kUwTileH;
}

size_t underwater_ws_bytes(Shape s)
{
    Carver c(nullptr);
    carve_uwq(c, s);
    return c.total();
}

int launch_underwater_scores(uwie_ctx *ctx, const uint8_t *d_u8, Shape s, int gray_shift, double *d_scores, void *ws, hipStream_t st)
{
    Carver c(ws);
    const UwBufs u = carve_uwq(c, s);
    const int npx = (int)s.npx(), nsblk = uwq_stream_blocks(s), ntiles = uwq_tiles(s);
    const int aligned = (npx & 3) == 0 && ((uintptr_t)d_u8 & 3) == 0;
    UWIE_HIP_CHECK(hipMemsetAsync(u.hist, 0, sizeof(uint32_t) * (size_t)s.B * kUwHistStride, st));
    UWIE_LAUNCH(k_uwq_stream, dim3(nsblk, s.B), dim3(256), 0, st, ctx->d_lab, d_u8, npx, aligned, u.hist, u.spart);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_uwq_tiles, dim3(ntiles, s.B), dim3(256), 0, st, d_u8, s.H, s.W, uwq_tiles_x(s), gray_shift, u.tpart);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_uwq_finish, dim3(s.B), dim3(64), 0, st, u.hist, u.spart, nsblk, u.tpart, ntiles, s.H, s.W, d_scores);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
