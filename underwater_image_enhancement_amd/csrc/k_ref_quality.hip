// Full-reference quality of a batch of u8 results against their ground truth (include/uwie.h uwie_reference_scores_u8): mean
// absolute error, mean squared error, PSNR, and SSIM (11 x 11 Gaussian window, sigma 1.5, valid windows only) of the gray plane
// and of the three channels, as device reductions, so that scoring a paired set and picking the best of N by closeness to the
// reference does not leave the GPU.
//   k_rq_stream  one pass over the two frames' bytes: the integer sums of |x - y| and (x - y)^2, one 64-bit pair per block
//   k_rq_tiles   one workgroup per 64 x 92 tile of map points: a 102 x 74 patch of both frames staged in LDS as eight byte
//                planes (gray, R, G, B of x and of y).  Wavefront w owns the band of 23 map rows 23 w .. 23 w + 22, lane l the
//                map column l.  A lane walks down its band's 33 staged rows: per row the five horizontal 11-tap sums (of x, y,
//                x * x, y * y, x * y), then each sum is added with tap k into the accumulator of the map row that started k
//                rows above: eleven rows' accumulators (55 float64) live in registers, rotating; the row loop is unrolled by
//                11 so that every accumulator index is static.  The accumulator that receives tap 10 is complete: s is
//                evaluated and added to the lane's sum.  The first 10 staged rows of a band complete nothing, hence
//                33 = 3 * 11 rows for 23 results.
//                Order of summation: down the column it is the header's (index order); along the row the two values that
//                share a tap (w[k] = w[10 - k]) are added first, as exact integers, which halves the conversions and
//                multiply-adds of the row pass.  Fused multiply-adds throughout.  Both are inside the header's 1e-9.
//   k_rq_finish  per frame: the blocks' and the tiles' rows added in their order, the divisions, the logarithm, NaN where there
//                is no window
// Symmetry: the x and the y side go through the same operations, so identical frames give num == den bit for bit, s = 1.0 and
// sums that are exact integers: every SSIM is exactly 1.0.
// Determinism as in k_uw_quality.hip: integer sums, one row per block and one float64 row per tile, added by k_rq_finish in
// row order; the grids depend on H and W only.  (A first version added the differences with one atomic pair per wave: 8192
// atomics on two addresses per frame took 0.6 ms at 1080p x 8; the ordered rows take 0.02 ms and need no memset.)
// The differences are a pass of their own, not part of the tile pass: tiles overlap by their halo, frames below 11 x 11 have
// no tile at all, and the pass is 3 % of the call (profiles/ref_quality_bench.txt).
// What bounds k_rq_tiles (SQ counters at 4K x 4): vector issue.  24 200 vector instructions per wave, each
// four cycles on a SIMD whether float64 or integer, the vector unit busy 90 % of the time with the two waves per SIMD that
// 217 registers and 62 KB of LDS allow; no LDS bank conflict, 4 % of the wave cycles waiting on LDS.
#include <cmath>

#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

constexpr int kRqTileW = 64, kRqBand = 23, kRqWaves = 4, kRqTileH = kRqBand * kRqWaves;  // map points per workgroup
constexpr int kRqGroups = (kRqBand + 10) / 11;                                             // row groups of 11 per band
static_assert(kRqGroups * 11 == kRqBand + 10, "a band's staged rows are whole groups of 11");
constexpr int kRqRows = kRqTileH + 10, kRqStride = 76;  // staged rows; bytes per staged row (74 used), a multiple of 4
static_assert(kRqStride >= kRqTileW + 10 && kRqStride % 4 == 0, "a staged row holds the tile and its halo");
constexpr double kRqC1 = (0.01 * 255) * (0.01 * 255), kRqC2 = (0.03 * 255) * (0.03 * 255);

struct RefTaps {
    double w[11];
};

// grid (nblk, B), block 256; sixteen bytes per thread and step.  part: [B][nblk][2] = this block's sum |x - y| and sum (x - y)^2
// over its share of the frame's n3 bytes.
__global__ void __launch_bounds__(256) k_rq_stream(const uint8_t *__restrict__ in, const uint8_t *__restrict__ ref, int ref_batch,
                                                   long long n3, unsigned long long *__restrict__ part)
{
    __shared__ uint64_t s_red[4][2];
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint8_t *x = in + (size_t)b * n3, *y = ref + (size_t)(b % ref_batch) * n3;
    const long long items = n3 >> 4;
    uint64_t sa = 0, sq = 0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < items; i += (long long)gridDim.x * 256) {
        const uint4 vx = *reinterpret_cast<const u128_unaligned *>(x + 16 * i), vy = *reinterpret_cast<const u128_unaligned *>(y + 16 * i);
        const uint32_t wx[4] = {vx.x, vx.y, vx.z, vx.w}, wy[4] = {vy.x, vy.y, vy.z, vy.w};
        uint32_t a = 0, q = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int d = (int)((wx[k >> 2] >> (8 * (k & 3))) & 255u) - (int)((wy[k >> 2] >> (8 * (k & 3))) & 255u);
            a += (uint32_t)abs(d);
            q += (uint32_t)(d * d);
        }
        sa += a;
        sq += q;
    }
    if (blockIdx.x == 0 && tid < (int)(n3 & 15)) {  // the bytes behind the last whole item
        const int d = (int)x[16 * items + tid] - (int)y[16 * items + tid];
        sa += (uint32_t)abs(d);
        sq += (uint32_t)(d * d);
    }
    sa = wave_sum_u64(sa);
    sq = wave_sum_u64(sq);
    if ((tid & 63) == 0) { s_red[tid >> 6][0] = sa; s_red[tid >> 6][1] = sq; }
    __syncthreads();
    if (tid < 2) part[((size_t)b * gridDim.x + blockIdx.x) * 2 + tid] = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
}

// an integer below 2^32 as float64: the bits of 2^52 + v, minus 2^52 (one exact float64 addition)
__device__ __forceinline__ double u32_to_f64(uint32_t v) { return __hiloint2double(0x43300000, (int)v) - 4503599627370496.0; }

// s of one map point from its five window sums a = sum w x, sum w y, sum w x^2, sum w y^2, sum w x y
__device__ __forceinline__ double ssim_point(const double *a)
{
    const double mxx = a[0] * a[0], myy = a[1] * a[1], mxy = a[0] * a[1];
    const double vx = a[2] - mxx, vy = a[3] - myy, cv = a[4] - mxy;
    const double num = (2.0 * mxy + kRqC1) * (2.0 * cv + kRqC2);
    const double den = ((mxx + myy) + kRqC1) * ((vx + vy) + kRqC2);
    return num / den;
}

// Eleven staged rows of one lane's column window (sx, sy: the row's bytes at this lane's map column).  acc[(r - k) mod 11] is the
// accumulator of the map row that started k rows above row r.  kFirst: the band's first group, where rows above the band do
// not exist (taps k > r are skipped and only row 10 completes a result).  out0: the band-relative map row that row 0 completes.
template <bool kFirst>
__device__ __forceinline__ void rq_rows11(const uint8_t *sx, const uint8_t *sy, const RefTaps &T, double (&acc)[11][5], int out0,
                                          int nvalid, bool colok, double &sum)
{
#pragma unroll
    for (int r = 0; r < 11; ++r) {
        // the row's five horizontal sums.  The taps are symmetric: the two values that share tap k are added first, as exact
        // integers (<= 2 * 65025), so a row costs 6 conversions and 6 multiply-adds per sum instead of 11
        double h[5];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint32_t xa = sx[r * kRqStride + k], ya = sy[r * kRqStride + k];
            const uint32_t xb = k < 5 ? sx[r * kRqStride + 10 - k] : 0u, yb = k < 5 ? sy[r * kRqStride + 10 - k] : 0u;
            const double v[5] = {u32_to_f64(xa + xb), u32_to_f64(ya + yb), u32_to_f64(xa * xa + xb * xb), u32_to_f64(ya * ya + yb * yb),
                                 u32_to_f64(xa * ya + xb * yb)};
#pragma unroll
            for (int q = 0; q < 5; ++q) h[q] = k == 0 ? T.w[0] * v[q] : fma(T.w[k], v[q], h[q]);
        }
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            if (!kFirst || k <= r) {
                double *a = acc[(r - k + 11) % 11];
#pragma unroll
                for (int q = 0; q < 5; ++q) a[q] = k == 0 ? T.w[0] * h[q] : fma(T.w[k], h[q], a[q]);
            }
        }
        if (!kFirst || r == 10) {
            const double s = ssim_point(acc[(r + 1) % 11]);
            if (colok && out0 + r < nvalid) sum += s;
        }
    }
}

// grid (tiles_x * tiles_y, B), block 256.  Tile (tx, ty) produces map points [64 tx, 64 tx + 64) x [92 ty, 92 ty + 92), which read
// frame rows 92 ty .. 92 ty + 101 and columns 64 tx .. 64 tx + 73.  Staged positions outside the frame hold zeros; only map
// points outside the map read them, and those are not counted.  tpart: [B][tiles][4] = sum of s for gray, R, G, B.
__global__ void __launch_bounds__(256) k_rq_tiles(const uint8_t *__restrict__ in, const uint8_t *__restrict__ ref, int ref_batch, int H,
                                                  int W, int tiles_x, int shift, RefTaps T, double *__restrict__ tpart)
{
    __shared__ __attribute__((aligned(16))) uint8_t s[2][4][kRqRows][kRqStride];
    __shared__ double s_red[kRqWaves][4];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kRqTileW, y0 = ty * kRqTileH;
    const size_t frame = (size_t)H * W * 3;
    const uint8_t *img[2] = {in + (size_t)b * frame, ref + (size_t)(b % ref_batch) * frame};
    constexpr int QUADS = kRqStride / 4;  // a staged row as groups of four pixels
    for (int i = tid; i < kRqRows * QUADS; i += 256) {
        const int ly = i / QUADS, g = i - ly * QUADS, gy = y0 + ly, gx = x0 + 4 * g;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            uint32_t pk[4] = {0u, 0u, 0u, 0u};
            if (gy < H && gx < W) {
                const uint8_t *p = img[f] + ((size_t)gy * W + gx) * 3;
                Px4 px;
                if (gx + 4 <= W) {
                    px = load_px4_any(p);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool in_row = gx + k < W;
                        px.r[k] = in_row ? p[3 * k] : 0u;
                        px.g[k] = in_row ? p[3 * k + 1] : 0u;
                        px.b[k] = in_row ? p[3 * k + 2] : 0u;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    pk[0] |= gray_fixed(px.r[k], px.g[k], px.b[k], shift) << (8 * k);
                    pk[1] |= px.r[k] << (8 * k);
                    pk[2] |= px.g[k] << (8 * k);
                    pk[3] |= px.b[k] << (8 * k);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) *reinterpret_cast<uint32_t *>(&s[f][p][ly][4 * g]) = pk[p];
        }
    }
    __syncthreads();
    const int band0 = wv * kRqBand;
    const int nvalid = min(kRqBand, (H - 10) - (y0 + band0));  // map rows of this band inside the map; <= 0: none
    const bool colok = x0 + lane < W - 10;
#pragma unroll 1
    for (int p = 0; p < 4; ++p) {
        double sum = 0.0;
        if (nvalid > 0) {
            const uint8_t *sx = &s[0][p][band0][lane], *sy = &s[1][p][band0][lane];
            double acc[11][5];
            rq_rows11<true>(sx, sy, T, acc, -10, nvalid, colok, sum);
#pragma unroll 1
            for (int g = 1; g < kRqGroups && 11 * g - 10 < nvalid; ++g)
                rq_rows11<false>(sx + 11 * g * kRqStride, sy + 11 * g * kRqStride, T, acc, 11 * g - 10, nvalid, colok, sum);
        }
        sum = wave_sum_f64(sum);
        if (lane == 0) s_red[wv][p] = sum;
    }
    __syncthreads();
    if (tid < 4) tpart[((size_t)b * gridDim.x + blockIdx.x) * 4 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

// grid B, block 64.  The wave adds the tiles' rows (lane l takes rows l, l + 64, ... in that order, then a fixed butterfly);
// every lane evaluates the scores, lane 0 writes them.  ntiles = 0: no window, the SSIM columns are NaN.
__global__ void __launch_bounds__(64) k_rq_finish(const unsigned long long *__restrict__ part, int nsblk, const double *__restrict__ tpart,
                                                  int ntiles, int H, int W, double *__restrict__ out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double ts[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < ntiles; k += 64) {
        const double *row = tpart + ((size_t)b * ntiles + k) * 4;
        ts[0] += row[0]; ts[1] += row[1]; ts[2] += row[2]; ts[3] += row[3];
    }
    for (int i = 0; i < 4; ++i) ts[i] = wave_sum_f64(ts[i]);
    const double n3 = (double)(3ll * H * W);
    uint64_t sa = 0, sq = 0;
    for (int k = lane; k < nsblk; k += 64) {
        sa += part[((size_t)b * nsblk + k) * 2];
        sq += part[((size_t)b * nsblk + k) * 2 + 1];
    }
    sa = wave_sum_u64(sa);
    sq = wave_sum_u64(sq);
    double sc[kRefScores];
    sc[0] = (double)sa / n3;
    sc[1] = (double)sq / n3;
    sc[2] = sq == 0 ? (double)INFINITY : 10.0 * log10(65025.0 / sc[1]);
    if (ntiles > 0) {
        const double cnt = (double)((long long)(H - 10) * (W - 10));
        for (int i = 0; i < 4; ++i) sc[3 + i] = ts[i] / cnt;
        sc[7] = ((sc[4] + sc[5]) + sc[6]) / 3.0;
    } else {
        for (int i = 3; i < kRefScores; ++i) sc[i] = (double)NAN;
    }
    if (lane == 0)
        for (int i = 0; i < kRefScores; ++i) out[(size_t)b * kRefScores + i] = sc[i];
}

struct RqBufs {
    unsigned long long *part;
    double *tpart;
};

// blocks of k_rq_stream and tiles of k_rq_tiles per frame: functions of the frame size alone
int rq_stream_blocks(Shape s) { return grid_for((3 * s.npx() + 15) / 16, 256); }
int rq_tiles_x(Shape s) { return cdiv(s.W - 10, kRqTileW); }
int rq_tiles(Shape s) { return s.H < 11 || s.W < 11 ? 0 : rq_tiles_x(s) * cdiv(s.H - 10, kRqTileH); }

RqBufs carve_rq(Carver &c, Shape s)
{
    RqBufs u;
    u.part = c.take<unsigned long long>((size_t)s.B * rq_stream_blocks(s) * 2);
    u.tpart = c.take<double>((size_t)s.B * rq_tiles(s) * 4);
    return u;
}

// the 1-D window: exp(-(k - 5)^2 / 4.5) divided by the sum taken in index order
RefTaps ref_taps()
{
    RefTaps t;
    double sum = 0.0;
    for (int k = 0; k < 11; ++k) {
        t.w[k] = std::exp(-(double)((k - 5) * (k - 5)) / 4.5);
        sum += t.w[k];
    }
    for (int k = 0; k < 11; ++k) t.w[k] /= sum;
    return t;
}

}  // namespace

void reference_tile(int *tile_w, int *tile_h)
{
    *tile_w = kRqTileW;
    *tile_h = kRqTileH;
}

size_t reference_ws_bytes(Shape s)
{
    Carver c(nullptr);
    carve_rq(c, s);
    return c.total();
}

int launch_reference_scores(const uint8_t *d_u8, const uint8_t *d_ref_u8, Shape s, int ref_batch, int gray_shift, double *d_scores,
                            void *ws, hipStream_t st)
{
    Carver c(ws);
    const RqBufs u = carve_rq(c, s);
    const int ntiles = rq_tiles(s), nsblk = rq_stream_blocks(s);
    UWIE_LAUNCH(k_rq_stream, dim3(nsblk, s.B), dim3(256), 0, st, d_u8, d_ref_u8, ref_batch, (long long)(3 * s.npx()), u.part);
    UWIE_LAUNCH_CHECK();
    if (ntiles > 0) {
        UWIE_LAUNCH(k_rq_tiles, dim3(ntiles, s.B), dim3(256), 0, st, d_u8, d_ref_u8, ref_batch, s.H, s.W, rq_tiles_x(s), gray_shift,
                    ref_taps(), u.tpart);
        UWIE_LAUNCH_CHECK();
    }
    UWIE_LAUNCH(k_rq_finish, dim3(s.B), dim3(64), 0, st, u.part, nsblk, u.tpart, ntiles, s.H, s.W, d_scores);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
