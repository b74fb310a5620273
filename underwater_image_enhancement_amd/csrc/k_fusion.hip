// Multi-scale fusion of Ancuti et al. 2018 for balanced u8 frames (include/uwie.h uwie_fusion_u8 states the contract): a
// gamma-corrected and a sharpened input, a weight from Laplacian contrast, saliency and saturation, and a blend over a
// Laplacian pyramid -- one weight pyramid and one pyramid of the inputs' difference.  Integer steps are exact, every float64
// step is a single IEEE operation in the contract's order (-ffp-contract=off), so every byte and every weight is that of the
// NumPy restatement (tests/fusion_ref.py), bit for bit.
//   k_fu_inputs    one workgroup per kFuTileW x kFuTileH tile of x staged with a 2-pixel halo: I2 (the unsharp mask over the
//                  5 x 5 binomial blur) goes to memory, the six channel sums of I1 and I2 to one row of 32-bit partials
//   k_fu_means     one wavefront per frame: the rows added as 64-bit integers, mu_c = S_c / n
//   k_fu_level0    the same tile of x and I2 with a 2-pixel halo: I1 through the table, both inputs' 5-tap row sums in LDS,
//                  then per pixel the two weights, Wn (float64) and D = I1 - I2 (three int16 planes)
//   k_fu_reduce    one level of both Gaussian pyramids (GW and the three planes of GD) per launch
//   k_fu_collapse  one level of the collapse per launch, coarse to fine; the last one adds I2 and writes bytes
// Launches: 3 + (L - 1) + L, whatever H and W.  Every index is clamped where it is formed (BORDER_REPLICATE), every store is
// guarded by the plane's size.  No atomics, no memset, no host read; grids come from H, W and L alone.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

constexpr int kFuTileW = 64, kFuTileH = 16;  // the level-0 tile of one workgroup (256 threads, four rows each)
constexpr int kFuHalo = 2;                   // of the 5-tap rule
constexpr int kFuStW = kFuTileW + 2 * kFuHalo, kFuStH = kFuTileH + 2 * kFuHalo;  // the staged tile
constexpr int kFuRow = 8;                    // words per row of partial sums (six used; 32-byte rows)
constexpr int kFuMeans = 8;                  // doubles per frame of means (six used)
static_assert(255u * kFuTileW * kFuTileH < (1u << 24), "a tile's channel sum fits 32 bits with room");
static_assert(kFuTileH % 4 == 0 && kFuTileW == 64, "thread t takes column t & 63 of rows (t >> 6) + 4 i");

struct FuTable {
    uint8_t g[256];
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// T of five values, the contract's order; exact for integers
template <typename V>
__device__ __forceinline__ V taps5(V m2, V m1, V c, V p1, V p2)
{
    return ((m2 + p2) + (V)4 * (m1 + p1)) + (V)6 * c;
}

// stage a (kFuStH x kFuStW x 3)-byte tile of img around tile origin (x0, y0) with clamped indices; f maps a byte
template <class F>
__device__ __forceinline__ void stage_tile(uint8_t (*s)[kFuStW][3], const uint8_t *__restrict__ img, int H, int W, int x0, int y0, F f)
{
    for (int i = threadIdx.x; i < kFuStH * kFuStW; i += 256) {
        const int ty = i / kFuStW, tx = i % kFuStW;
        const int gy = clampi(y0 + ty - kFuHalo, H - 1), gx = clampi(x0 + tx - kFuHalo, W - 1);
        const uint8_t *p = img + ((size_t)gy * W + gx) * 3;
        s[ty][tx][0] = f(p[0]);
        s[ty][tx][1] = f(p[1]);
        s[ty][tx][2] = f(p[2]);
    }
}

// the row pass of B over a staged tile: rs[ty][x][c] = T along the row at tile row ty, tile column x + kFuHalo
__device__ __forceinline__ void row_pass(uint16_t (*rs)[kFuTileW][3], const uint8_t (*s)[kFuStW][3])
{
    for (int i = threadIdx.x; i < kFuStH * kFuTileW; i += 256) {
        const int ty = i / kFuTileW, x = i % kFuTileW;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            rs[ty][x][c] = (uint16_t)taps5<uint32_t>(s[ty][x][c], s[ty][x + 1][c], s[ty][x + 2][c], s[ty][x + 3][c], s[ty][x + 4][c]);
    }
}

// B at tile pixel (x, y): T down the column of the row sums (<= 256 * 255)
__device__ __forceinline__ uint32_t col_pass(const uint16_t (*rs)[kFuTileW][3], int x, int y, int c)
{
    return taps5<uint32_t>(rs[y][x][c], rs[y + 1][x][c], rs[y + 2][x][c], rs[y + 3][x][c], rs[y + 4][x][c]);
}

// grid (cdiv(W, kFuTileW), cdiv(H, kFuTileH), B), block 256.  part: [B][gridDim.y * gridDim.x][kFuRow].
__global__ void __launch_bounds__(256) k_fu_inputs(const uint8_t *__restrict__ in, int H, int W, FuTable tab, uint8_t *__restrict__ in2,
                                                   uint8_t *__restrict__ in1_out, uint32_t *__restrict__ part)
{
    __shared__ uint8_t s_x[kFuStH][kFuStW][3];
    __shared__ uint16_t s_rs[kFuStH][kFuTileW][3];
    __shared__ uint32_t s_red[4][6];
    __shared__ uint8_t s_tab[256];
    const int b = blockIdx.z, tid = threadIdx.x;
    const size_t n = (size_t)H * W;
    const uint8_t *img = in + (size_t)b * 3 * n;
    const int x0 = blockIdx.x * kFuTileW, y0 = blockIdx.y * kFuTileH;
    s_tab[tid] = tab.g[tid];
    stage_tile(s_x, img, H, W, x0, y0, [](uint8_t v) { return v; });
    __syncthreads();
    row_pass(s_rs, s_x);
    __syncthreads();
    uint32_t sum[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    const int x = tid & 63, gx = x0 + x;
#pragma unroll
    for (int i = 0; i < kFuTileH / 4; ++i) {
        const int y = (tid >> 6) + 4 * i, gy = y0 + y;
        if (gx < W && gy < H) {
            const size_t off = (size_t)b * 3 * n + ((size_t)gy * W + gx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int v = s_x[y + kFuHalo][x + kFuHalo][c];
                const int u = (512 * v - (int)col_pass(s_rs, x, y, c) + 128) >> 8;  // arithmetic shift: floor
                const uint32_t i2 = (uint32_t)(u < 0 ? 0 : (u > 255 ? 255 : u)), i1 = s_tab[v];
                in2[off + c] = (uint8_t)i2;
                if (in1_out) in1_out[off + c] = (uint8_t)i1;
                sum[c] += i1;
                sum[3 + c] += i2;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) sum[k] = wave_sum_u32(sum[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_red[tid >> 6][k] = sum[k];
    }
    __syncthreads();
    if (tid < kFuRow) {
        const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.y;
        part[((size_t)b * nblk + blk) * kFuRow + tid] = tid < 6 ? (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]) : 0u;
    }
}

// grid B, block 64.  means: [B][kFuMeans] = mu of I1's r, g, b, then of I2's.
__global__ void __launch_bounds__(64) k_fu_means(const uint32_t *__restrict__ part, int nblk, int H, int W, double *__restrict__ means)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    uint64_t s[6] = {0, 0, 0, 0, 0, 0};
    for (int k = lane; k < nblk; k += 64) {
        const uint32_t *row = part + ((size_t)b * nblk + k) * kFuRow;
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] += row[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] = wave_sum_u64(s[i]);
    const double N = (double)((long long)H * W);
    if (lane < kFuMeans) {
        uint64_t v = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) v = lane == i ? s[i] : v;
        means[(size_t)b * kFuMeans + lane] = lane < 6 ? (double)v / N : 0.0;
    }
}

// W_k of the contract at tile pixel (x, y) of one staged input
__device__ __forceinline__ double fu_weight(const uint8_t (*s)[kFuStW][3], const uint16_t (*rs)[kFuTileW][3], int x, int y, const double *mu,
                                            int gray_shift)
{
    const int sx = x + kFuHalo, sy = y + kFuHalo;
    auto gray = [&](int yy, int xx) { return (int)gray_fixed(s[yy][xx][0], s[yy][xx][1], s[yy][xx][2], gray_shift); };
    const int Y = gray(sy, sx);
    const int l = 4 * Y - gray(sy - 1, sx) - gray(sy + 1, sx) - gray(sy, sx - 1) - gray(sy, sx + 1);
    const double wl = (double)(l < 0 ? -l : l) / 255.0;
    double sal = 0.0;
    int q = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double d = mu[c] - (double)col_pass(rs, x, y, c) * 0x1p-8;
        sal = sal + d * d;
        const int e = (int)s[sy][sx][c] - Y;
        q += e * e;
    }
    const double ws = sal / 65025.0;
    const double wsat = sqrt((double)q / 3.0) / 255.0;
    return (wl + ws) + wsat;
}

// grid as k_fu_inputs.  wn: [B][H][W] float64, dw: the caller's copy of it or nullptr, D: [B][3][H][W] int16.
__global__ void __launch_bounds__(256) k_fu_level0(const uint8_t *__restrict__ in, const uint8_t *__restrict__ in2, int H, int W, FuTable tab,
                                                   const double *__restrict__ means, int gray_shift, double *__restrict__ wn,
                                                   double *__restrict__ dw, int16_t *__restrict__ D)
{
    __shared__ uint8_t s_tab[256];
    __shared__ uint8_t s_1[kFuStH][kFuStW][3], s_2[kFuStH][kFuStW][3];
    __shared__ uint16_t s_r1[kFuStH][kFuTileW][3], s_r2[kFuStH][kFuTileW][3];
    const int b = blockIdx.z, tid = threadIdx.x;
    const size_t n = (size_t)H * W;
    const int x0 = blockIdx.x * kFuTileW, y0 = blockIdx.y * kFuTileH;
    s_tab[tid] = tab.g[tid];
    __syncthreads();
    stage_tile(s_1, in + (size_t)b * 3 * n, H, W, x0, y0, [&](uint8_t v) { return s_tab[v]; });
    stage_tile(s_2, in2 + (size_t)b * 3 * n, H, W, x0, y0, [](uint8_t v) { return v; });
    __syncthreads();
    row_pass(s_r1, s_1);
    row_pass(s_r2, s_2);
    __syncthreads();
    double mu[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) mu[k] = means[(size_t)b * kFuMeans + k];
    const int x = tid & 63, gx = x0 + x;
#pragma unroll
    for (int i = 0; i < kFuTileH / 4; ++i) {
        const int y = (tid >> 6) + 4 * i, gy = y0 + y;
        if (gx < W && gy < H) {
            const double a = fu_weight(s_1, s_r1, x, y, mu, gray_shift) + 0.1;
            const double w = a / (a + (fu_weight(s_2, s_r2, x, y, mu + 3, gray_shift) + 0.1));
            const size_t p = (size_t)gy * W + gx;
            wn[(size_t)b * n + p] = w;
            if (dw) dw[(size_t)b * n + p] = w;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                D[((size_t)b * 3 + c) * n + p] = (int16_t)((int)s_1[y + kFuHalo][x + kFuHalo][c] - (int)s_2[y + kFuHalo][x + kFuHalo][c]);
        }
    }
}

// reduce() of one plane at coarse point (y, x): T along the row at the five clamped rows, T down the column, times 2^-8
template <typename T>
__device__ __forceinline__ double fu_reduce_at(const T *__restrict__ p, int h, int w, int y, int x)
{
    int xs[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) xs[j] = clampi(2 * x + j - 2, w - 1);
    double r[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const T *row = p + (size_t)clampi(2 * y + i - 2, h - 1) * w;
        r[i] = taps5<double>((double)row[xs[0]], (double)row[xs[1]], (double)row[xs[2]], (double)row[xs[3]], (double)row[xs[4]]);
    }
    return taps5<double>(r[0], r[1], r[2], r[3], r[4]) * 0x1p-8;
}

// grid (cdiv(wc, 32), cdiv(hc, 8), B), block 256: level (h, w) -> (hc, wc) = (ceil(h / 2), ceil(w / 2)).
// gw [B][h][w] -> gwc [B][hc][wc]; gd [B][3][h][w] (int16 at level 0, float64 above) -> gdc [B][3][hc][wc].
template <typename T>
__global__ void __launch_bounds__(256) k_fu_reduce(const double *__restrict__ gw, const T *__restrict__ gd, int h, int w, int hc, int wc,
                                                   double *__restrict__ gwc, double *__restrict__ gdc)
{
    const int b = blockIdx.z, x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= wc || y >= hc) return;
    const size_t n = (size_t)h * w, nc = (size_t)hc * wc, pc = (size_t)y * wc + x;
    gwc[(size_t)b * nc + pc] = fu_reduce_at(gw + (size_t)b * n, h, w, y, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) gdc[((size_t)b * 3 + c) * nc + pc] = fu_reduce_at(gd + ((size_t)b * 3 + c) * n, h, w, y, x);
}

// expand() of a coarse plane (hc x wc) at the four fine points (2 ky + j, 2 kx + i) that coarse point (ky, kx) heads: along the
// row at the three clamped coarse rows, then down the column.  The even and the odd rule read the same 3 x 3 neighbourhood, so
// nine loads serve four points and no lane selects by parity.
__device__ __forceinline__ void fu_expand4(const double *__restrict__ p, int hc, int wc, int ky, int kx, double (&e)[2][2])
{
    const int xm = clampi(kx - 1, wc - 1), xp = clampi(kx + 1, wc - 1);
    const int rows[3] = {clampi(ky - 1, hc - 1), ky, clampi(ky + 1, hc - 1)};
    double ev[3], od[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double *row = p + (size_t)rows[i] * wc;
        const double a = row[xm], b = row[kx], c = row[xp];
        ev[i] = ((a + c) + 6.0 * b) * 0.125;
        od[i] = (b + c) * 0.5;
    }
    e[0][0] = ((ev[0] + ev[2]) + 6.0 * ev[1]) * 0.125;
    e[0][1] = ((od[0] + od[2]) + 6.0 * od[1]) * 0.125;
    e[1][0] = (ev[1] + ev[2]) * 0.5;
    e[1][1] = (od[1] + od[2]) * 0.5;
}

// rint(min(max(v, 0), 255)) as a byte: adding 2^52 rounds to an integer by the addition's own round-half-to-even
__device__ __forceinline__ uint8_t fu_byte(double v)
{
    const double lo = v > 0.0 ? v : 0.0, c = lo < 255.0 ? lo : 255.0;
    return (uint8_t)((uint32_t)__double_as_longlong(c + 0x1p52) & 0xffu);
}

// One level of the collapse.  grid (cdiv(ceil(w / 2), 64), cdiv(ceil(h / 2), 4), B), block 256: a thread takes the 2 x 2 points
// of level (h, w) under one point (ky, kx) of the coarser level.  TOP: the coarsest level, acc = GW * GD; else
// acc = GW * (GD - expand(GD')) + expand(acc') with GD', acc' [B][3][hc][wc], (hc, wc) = (ceil(h / 2), ceil(w / 2)).
// FINAL (level 0): out = byte(I2 + acc), else acc goes to acc_out [B][3][h][w].
template <typename T, bool TOP, bool FINAL>
__global__ void __launch_bounds__(256) k_fu_collapse(const double *__restrict__ gw, const T *__restrict__ gd, int h, int w,
                                                     const double *__restrict__ gdc, const double *__restrict__ accc, int hc, int wc,
                                                     double *__restrict__ acc_out, const uint8_t *__restrict__ in2, uint8_t *__restrict__ out)
{
    const int b = blockIdx.z, kx = blockIdx.x * 64 + (threadIdx.x & 63), ky = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int x0 = 2 * kx, y0 = 2 * ky;
    if (x0 >= w || y0 >= h) return;  // (so kx < wc and ky < hc)
    const bool ok[2][2] = {{true, x0 + 1 < w}, {y0 + 1 < h, x0 + 1 < w && y0 + 1 < h}};
    const size_t n = (size_t)h * w, nc = (size_t)hc * wc;
    double wgt[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) wgt[j][i] = ok[j][i] ? gw[(size_t)b * n + (size_t)(y0 + j) * w + x0 + i] : 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t pl = (size_t)b * 3 + c;
        double e1[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, e2[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        if (!TOP) {
            fu_expand4(gdc + pl * nc, hc, wc, ky, kx, e1);
            fu_expand4(accc + pl * nc, hc, wc, ky, kx, e2);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (!ok[j][i]) continue;
                const size_t p = (size_t)(y0 + j) * w + x0 + i;
                const double d = (double)gd[pl * n + p];
                double acc;
                if (TOP) {
                    acc = wgt[j][i] * d;
                } else {
                    const double lap = d - e1[j][i];
                    acc = wgt[j][i] * lap + e2[j][i];
                }
                if (FINAL) {
                    const size_t o = (size_t)b * 3 * n + p * 3 + c;
                    out[o] = fu_byte((double)in2[o] + acc);
                } else {
                    acc_out[pl * n + p] = acc;
                }
            }
    }
}

struct FuLevel {
    int h, w;
    double *gw;   // [B][h][w]           (level 0: Wn)
    double *gd;   // [B][3][h][w]        (levels >= 1; level 0 is the int16 D)
    double *acc;  // [B][3][h][w]        (levels >= 1)
};

struct FuBufs {
    uint32_t *part;  // [B][tiles][kFuRow]
    double *means;   // [B][kFuMeans]
    uint8_t *in2;    // [B][H][W][3]
    int16_t *D;      // [B][3][H][W]
    FuLevel lv[8];
};

int fu_tiles(Shape s) { return cdiv(s.W, kFuTileW) * cdiv(s.H, kFuTileH); }

FuBufs carve_fu(Carver &c, Shape s, int levels)
{
    FuBufs f;
    f.part = c.take<uint32_t>((size_t)s.B * fu_tiles(s) * kFuRow);
    f.means = c.take<double>((size_t)s.B * kFuMeans);
    f.in2 = c.take<uint8_t>((size_t)s.B * s.npx() * 3);
    f.D = c.take<int16_t>((size_t)s.B * s.npx() * 3);
    int h = s.H, w = s.W;
    for (int l = 0; l < 8; ++l) {
        FuLevel &v = f.lv[l];
        v = FuLevel{h, w, nullptr, nullptr, nullptr};
        if (l < levels) {
            const size_t n = (size_t)s.B * h * w;
            v.gw = c.take<double>(n);
            if (l > 0) {
                v.gd = c.take<double>(3 * n);
                v.acc = c.take<double>(3 * n);
            }
        }
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    return f;
}

// profiler rows: the level a launch writes
const char *const kFuReduceRow[8] = {"", "k_fu_reduce<1>", "k_fu_reduce<2>", "k_fu_reduce<3>", "k_fu_reduce<4>", "k_fu_reduce<5>", "k_fu_reduce<6>",
                                     "k_fu_reduce<7>"};
const char *const kFuCollapseRow[8] = {"k_fu_collapse<0>", "k_fu_collapse<1>", "k_fu_collapse<2>", "k_fu_collapse<3>", "k_fu_collapse<4>",
                                       "k_fu_collapse<5>", "k_fu_collapse<6>", "k_fu_collapse<7>"};

template <typename T>
int launch_collapse(const char *row, const double *gw, const T *gd, const FuLevel &v, const FuLevel *coarser, bool final, int B, const uint8_t *in2,
                    uint8_t *out, hipStream_t st)
{
    const dim3 grid(cdiv((v.w + 1) / 2, 64), cdiv((v.h + 1) / 2, 4), B);  // a thread per 2 x 2 points
    const double *gdc = coarser ? coarser->gd : nullptr, *accc = coarser ? coarser->acc : nullptr;
    const int hc = coarser ? coarser->h : 1, wc = coarser ? coarser->w : 1;
#define UWIE_FU_COLLAPSE(TOP, FINAL) \
    UWIE_LAUNCH_AS(row, (k_fu_collapse<T, TOP, FINAL>), grid, dim3(256), 0, st, gw, gd, v.h, v.w, gdc, accc, hc, wc, v.acc, in2, out)
    if (!coarser && final) UWIE_FU_COLLAPSE(true, true);
    else if (!coarser) UWIE_FU_COLLAPSE(true, false);
    else if (final) UWIE_FU_COLLAPSE(false, true);
    else UWIE_FU_COLLAPSE(false, false);
#undef UWIE_FU_COLLAPSE
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace

void fusion_tile(int *tile_w, int *tile_h)
{
    *tile_w = kFuTileW;
    *tile_h = kFuTileH;
}

void fusion_table(double gamma, uint8_t *table256)
{
    for (int v = 0; v < 256; ++v) table256[v] = (uint8_t)std::rint(255.0 * std::pow((double)v / 255.0, gamma));
}

size_t fusion_ws_bytes(Shape s, int levels)
{
    Carver c(nullptr);
    carve_fu(c, s, levels);
    return c.total();
}

int launch_fusion(const uint8_t *d_in, Shape s, double gamma, int levels, int gray_shift, uint8_t *d_out, uint8_t *d_in1, uint8_t *d_in2,
                  double *d_weight, void *ws, hipStream_t st)
{
    Carver c(ws);
    const FuBufs f = carve_fu(c, s, levels);
    FuTable tab;
    fusion_table(gamma, tab.g);
    const dim3 tiles(cdiv(s.W, kFuTileW), cdiv(s.H, kFuTileH), s.B);
    uint8_t *in2 = d_in2 ? d_in2 : f.in2;  // the caller's plane serves as the working one
    UWIE_LAUNCH(k_fu_inputs, tiles, dim3(256), 0, st, d_in, s.H, s.W, tab, in2, d_in1, f.part);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_fu_means, dim3(s.B), dim3(64), 0, st, (const uint32_t *)f.part, fu_tiles(s), s.H, s.W, f.means);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_fu_level0, tiles, dim3(256), 0, st, d_in, (const uint8_t *)in2, s.H, s.W, tab, (const double *)f.means, gray_shift, f.lv[0].gw,
                d_weight, f.D);
    UWIE_LAUNCH_CHECK();
    for (int l = 1; l < levels; ++l) {
        const FuLevel &a = f.lv[l - 1], &b = f.lv[l];
        const dim3 grid(cdiv(b.w, 32), cdiv(b.h, 8), s.B);
        if (l == 1)
            UWIE_LAUNCH_AS(kFuReduceRow[l], k_fu_reduce<int16_t>, grid, dim3(256), 0, st, (const double *)a.gw, (const int16_t *)f.D, a.h, a.w, b.h, b.w, b.gw, b.gd);
        else
            UWIE_LAUNCH_AS(kFuReduceRow[l], k_fu_reduce<double>, grid, dim3(256), 0, st, (const double *)a.gw, (const double *)a.gd, a.h, a.w, b.h, b.w, b.gw, b.gd);
        UWIE_LAUNCH_CHECK();
    }
    for (int l = levels - 1; l >= 0; --l) {
        const FuLevel *coarser = l + 1 < levels ? &f.lv[l + 1] : nullptr;
        const int rc = l == 0 ? launch_collapse<int16_t>(kFuCollapseRow[0], f.lv[0].gw, f.D, f.lv[0], coarser, true, s.B, in2, d_out, st)
                              : launch_collapse<double>(kFuCollapseRow[l], f.lv[l].gw, f.lv[l].gd, f.lv[l], coarser, false, s.B, in2, d_out, st);
        if (rc != UWIE_OK) return rc;
    }
    return UWIE_OK;
}

}  // namespace uwie
