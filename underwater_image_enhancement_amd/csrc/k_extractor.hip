// feature_extraction.FeatureExtractor.extract_all_features (feature_extraction.py:252-295), the classifier input of
// main.py:116,420: 79 values per frame (74 when a dimension is odd and > 1: cv2.dct refuses, the reference drops 57-61).
//   k_fx_maps       one pass over the u8 frame: histograms of R, G, B, L, a, b, H, S, V and gray (cv2 u8 LAB / HSV /
//                   RGB2GRAY), the gray plane, and for a float image per-block float64 sums and the min / max of each channel
//   k_fx_stencil    3x3 stencil over the gray plane: Sobel (exact integer gx, gy; float64 sum of the magnitudes per block),
//                   Laplacian ksize 3 (exact int64 sums), the 10-bin uniform LBP histogram (skimage's float64 bilinear samples)
//   Canny           launch_canny(..., 50, 150), as k_quality.hip
//   k_fx_resize     cv2.resize(gray, (128, 128)) INTER_LINEAR, OpenCV's fixed-point u8 path (INTER_AREA fast path at 2x)
//   k_fx_glcm       one workgroup per (frame, angle): the symmetric 256x256 co-occurrence counts (u16 pairs in 128 KiB of
//                   LDS) and the six graycoprops from exact integer sums, in float64
//   k_fx_dct_rows / k_fx_dct_cols   orthonormal 2-D DCT-II as two f32 MFMA products against the cosine matrix (even / odd
//                   split of DCT-II, entries from a 4N-entry table); the column product reduces its results in the epilogue
//   k_fx_finish     the 79 (74) values in float64 from the histograms, integer sums and per-block partials
// Every floating sum is per-block partials reduced in a fixed order (no float atomics): the same input gives the same bits
// in any batch.  Exactness per index: DESIGN.md section 9.
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

constexpr int kFxHist = 10;        // R, G, B, L, a, b, H, S, V, gray
constexpr int kFxGlcmProps = 6;    // contrast, dissimilarity, homogeneity, energy, correlation, ASM (feature_extraction.py:117)
constexpr int kFxDctSums = 5;      // low, mid, high region energy, total energy, sum |d|
constexpr int kFxMapsCap = 1024;   // blocks per frame of the streaming passes (a function of H, W only)
constexpr int kFxSmall = 128;      // cv2.resize target (feature_extraction.py:107)
constexpr size_t kFxGlcmLds = 256 * 256 * 2 + 256 * 4;  // u16 counts + |i - j| histogram

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define UWIE_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))

__device__ __forceinline__ float key_f32(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// grid (nblk, B), block 256.  hist [B][10][256]; fpart [B][nblk][6] = sum x, sum x^2 per channel; fmm [B][6] = min / max keys
__global__ void __launch_bounds__(256) k_fx_maps(const LabTables *__restrict__ T, const uint8_t *__restrict__ in,
                                                 const float *__restrict__ fimg, int npx, int shift, uint8_t *__restrict__ gray,
                                                 uint32_t *__restrict__ hist, double *__restrict__ fpart, uint32_t *__restrict__ fmm)
{
    __shared__ uint32_t h[kFxHist][256];
    __shared__ int s_sdiv[256], s_hdiv[256];
    __shared__ double s_red[4][6];
    __shared__ uint32_t s_mm[6];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < kFxHist * 256; i += 256) (&h[0][0])[i] = 0;
    // RGB2HSV_b's tables: saturate_cast<int>((255 << 12) / (1. * i)), saturate_cast<int>((180 << 12) / (6. * i))
    s_sdiv[tid] = tid ? __double2int_rn((double)(255 << 12) / (double)tid) : 0;
    s_hdiv[tid] = tid ? __double2int_rn((double)(180 << 12) / (6.0 * tid)) : 0;
    if (tid < 6) s_mm[tid] = (tid & 1) ? 0u : 0xffffffffu;
    __syncthreads();
    const uint8_t *img = in + (size_t)b * npx * 3;
    const float *fi = fimg ? fimg + (size_t)b * npx * 3 : nullptr;
    uint8_t *g = gray + (size_t)b * npx;
    const int *C = T->fwd;
    constexpr int Lscale = (116 * 255 + 50) / 100;
    constexpr int Lshift = -((16 * 255 * (1 << 15) + 50) / 100);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int p = blockIdx.x * 256 + tid; p < npx; p += gridDim.x * 256) {
        const int r = img[(size_t)p * 3], gg = img[(size_t)p * 3 + 1], bl = img[(size_t)p * 3 + 2];
        const uint32_t gv = gray_fixed(r, gg, bl, shift);
        g[p] = (uint8_t)gv;
        // cvtColor(u8, RGB2LAB) (k_clahe.hip rgb2lab_px)
        const int R = T->gamma[r], G = T->gamma[gg], Bq = T->gamma[bl];
        const int fX = T->cbrt[UWIE_DESCALE(R * C[0] + G * C[1] + Bq * C[2], 12)];
        const int fY = T->cbrt[UWIE_DESCALE(R * C[3] + G * C[4] + Bq * C[5], 12)];
        const int fZ = T->cbrt[UWIE_DESCALE(R * C[6] + G * C[7] + Bq * C[8], 12)];
        const int L = sat_u8(UWIE_DESCALE(Lscale * fY + Lshift, 15));
        const int la = sat_u8(UWIE_DESCALE(500 * (fX - fY) + 128 * (1 << 15), 15));
        const int lb = sat_u8(UWIE_DESCALE(200 * (fY - fZ) + 128 * (1 << 15), 15));
        // cvtColor(u8, RGB2HSV), hue range 180 (oracle/cvref.c cvref_rgb2hsv_u8)
        const int v = max(max(r, gg), bl), vmin = min(min(r, gg), bl), diff = v - vmin;
        const int vr = v == r ? -1 : 0, vg = v == gg ? -1 : 0;
        const int sat = (diff * s_sdiv[v] + (1 << 11)) >> 12;
        int hue = (vr & (gg - bl)) + (~vr & ((vg & (bl - r + 2 * diff)) + ((~vg) & (r - gg + 4 * diff))));
        hue = (hue * s_hdiv[diff] + (1 << 11)) >> 12;
        hue += hue < 0 ? 180 : 0;
        atomicAdd(&h[0][r], 1u);
        atomicAdd(&h[1][gg], 1u);
        atomicAdd(&h[2][bl], 1u);
        atomicAdd(&h[3][L], 1u);
        atomicAdd(&h[4][la], 1u);
        atomicAdd(&h[5][lb], 1u);
        atomicAdd(&h[6][hue], 1u);
        atomicAdd(&h[7][sat], 1u);
        atomicAdd(&h[8][v], 1u);
        atomicAdd(&h[9][gv], 1u);
        if (fi) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = fi[(size_t)p * 3 + c];
                acc[2 * c] += (double)x;
                acc[2 * c + 1] += (double)x * (double)x;
                const uint32_t k = f32_key(x);
                mn[c] = min(mn[c], k);
                mx[c] = max(mx[c], k);
            }
        }
    }
    if (fi) {
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[i] = wave_sum_f64(acc[i]);
        if ((tid & 63) == 0)
            for (int i = 0; i < 6; ++i) s_red[tid >> 6][i] = acc[i];
        for (int c = 0; c < 3; ++c) {
            atomicMin(&s_mm[2 * c], mn[c]);
            atomicMax(&s_mm[2 * c + 1], mx[c]);
        }
    }
    __syncthreads();
    if (fi && tid < 6) {
        fpart[((size_t)b * gridDim.x + blockIdx.x) * 6 + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
        if (tid & 1) atomicMax(&fmm[b * 6 + tid], s_mm[tid]);
        else atomicMin(&fmm[b * 6 + tid], s_mm[tid]);
    }
    for (int i = tid; i < kFxHist * 256; i += 256) {
        const uint32_t c = (&h[0][0])[i];
        if (c) atomicAdd(&hist[(size_t)b * kFxHist * 256 + i], c);
    }
}

// skimage.feature.local_binary_pattern's sample at (y + dr, x + dc) for the diagonal offsets +-0.70711 (np.round(sin, 5)):
// bilinear_interpolation in float64 with constant 0 outside, in the library's operation order (-ffp-contract=off: no FMA)
__device__ __forceinline__ double lbp_diag(const uint8_t *g, int H, int W, int y, int x, double offr, double offc)
{
    const double rf = (double)y + offr, cf = (double)x + offc;
    const double minr = floor(rf), minc = floor(cf), maxr = ceil(rf), maxc = ceil(cf);
    const double dr = rf - minr, dc = cf - minc;
    const int r0 = (int)minr, r1 = (int)maxr, c0 = (int)minc, c1 = (int)maxc;
    auto px = [&](int rr, int cc) -> double { return (rr >= 0 && rr < H && cc >= 0 && cc < W) ? (double)g[(size_t)rr * W + cc] : 0.0; };
    const double tl = px(r0, c0), tr = px(r0, c1), bl = px(r1, c0), br = px(r1, c1);
    const double top = (1 - dc) * tl + dc * tr;
    const double bottom = (1 - dc) * bl + dc * br;
    return (1 - dr) * top + dr * bottom;
}

// grid (nblk, B), block 256.  lbp [B][10]; isum [B][4] = sum |l|, sum l, sum l^2, sum (gx^2 + gy^2); gmax [B] = max gx^2 + gy^2;
// mpart [B][nblk] = sum sqrt(gx^2 + gy^2)
__global__ void __launch_bounds__(256) k_fx_stencil(const uint8_t *__restrict__ gray, int H, int W, uint32_t *__restrict__ lbp,
                                                    unsigned long long *__restrict__ isum, uint32_t *__restrict__ gmax,
                                                    double *__restrict__ mpart)
{
    __shared__ uint32_t s_lbp[10];
    __shared__ unsigned long long s_red[4][4];
    __shared__ double s_mag[4];
    __shared__ uint32_t s_max;
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < 10) s_lbp[tid] = 0;
    if (tid == 0) s_max = 0;
    __syncthreads();
    const int npx = H * W;
    const uint8_t *g = gray + (size_t)b * npx;
    constexpr double D = 0.70711;
    long long sabs = 0, s1 = 0, s2 = 0, sm2 = 0;
    uint32_t mmax = 0;
    double smag = 0.0;
    for (int p = blockIdx.x * 256 + tid; p < npx; p += gridDim.x * 256) {
        const int y = p / W, x = p - y * W;
        const int yu = reflect101(y - 1, H), yd = reflect101(y + 1, H), xl = reflect101(x - 1, W), xr = reflect101(x + 1, W);
        const int a00 = g[yu * W + xl], a01 = g[yu * W + x], a02 = g[yu * W + xr];
        const int a10 = g[y * W + xl], a11 = g[p], a12 = g[y * W + xr];
        const int a20 = g[yd * W + xl], a21 = g[yd * W + x], a22 = g[yd * W + xr];
        // cv2.Sobel ksize 3 (BORDER_REFLECT_101) on the bytes: the float32 plane gray/255 differs by the 1/255 factor
        const int gx = (a02 - a00) + 2 * (a12 - a10) + (a22 - a20);
        const int gy = (a20 - a00) + 2 * (a21 - a01) + (a22 - a02);
        const uint32_t m2 = (uint32_t)(gx * gx + gy * gy);
        sm2 += m2;
        mmax = max(mmax, m2);
        smag += sqrt((double)m2);
        // cv2.Laplacian(CV_64F, ksize=3): aperture [[2, 0, 2], [0, -8, 0], [2, 0, 2]]
        const int l = 2 * (a00 + a02 + a20 + a22) - 8 * a11;
        s1 += l;
        sabs += l < 0 ? -l : l;
        s2 += (long long)l * l;
        // LBP (P = 8, R = 1, 'uniform'): points p = 0..7 at (-sin, cos) of 2 pi p / 8; axis points are plain pixels
        const double c = (double)a11;
        auto pix = [&](int rr, int cc) -> double { return (rr >= 0 && rr < H && cc >= 0 && cc < W) ? (double)g[(size_t)rr * W + cc] : 0.0; };
        double sv[8];
        sv[0] = pix(y, x + 1);
        sv[1] = lbp_diag(g, H, W, y, x, -D, D);
        sv[2] = pix(y - 1, x);
        sv[3] = lbp_diag(g, H, W, y, x, -D, -D);
        sv[4] = pix(y, x - 1);
        sv[5] = lbp_diag(g, H, W, y, x, D, -D);
        sv[6] = pix(y + 1, x);
        sv[7] = lbp_diag(g, H, W, y, x, D, D);
        int bits = 0, changes = 0, prev = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int s = (sv[i] - c >= 0) ? 1 : 0;
            bits += s;
            if (i) changes += s != prev;
            prev = s;
        }
        atomicAdd(&s_lbp[changes <= 2 ? bits : 9], 1u);
    }
    unsigned long long v[4] = {(unsigned long long)sabs, (unsigned long long)s1, (unsigned long long)s2, (unsigned long long)sm2};
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = wave_sum_u64(v[i]);
    smag = wave_sum_f64(smag);
    if ((tid & 63) == 0) {
        for (int i = 0; i < 4; ++i) s_red[tid >> 6][i] = v[i];
        s_mag[tid >> 6] = smag;
    }
    atomicMax(&s_max, mmax);
    __syncthreads();
    if (tid < 4) atomicAdd(&isum[b * 4 + tid], s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid]);
    if (tid == 4) mpart[(size_t)b * gridDim.x + blockIdx.x] = (s_mag[0] + s_mag[1]) + (s_mag[2] + s_mag[3]);
    if (tid == 5) atomicMax(&gmax[b], s_max);
    if (tid < 10 && s_lbp[tid]) atomicAdd(&lbp[b * 10 + tid], s_lbp[tid]);
}

// cv2.resize's source taps for one output coordinate (resizeGeneric_, INTER_LINEAR, fixed point): fx = (float)((d + 0.5) *
// scale - 0.5), clamped at the borders, coefficients saturate_cast<short>((1 - fx) * 2048), saturate_cast<short>(fx * 2048)
__device__ __forceinline__ void resize_tap(int d, int src, int &s0, int &s1, int &c0, int &c1)
{
    const double scale = 1.0 / ((double)kFxSmall / (double)src);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= src - 1) { f = 0.0f; s = src - 1; }
    s0 = s;
    s1 = min(s + 1, src - 1);
    c0 = __float2int_rn((1.0f - f) * 2048.0f);
    c1 = __float2int_rn(f * 2048.0f);
}

// grid (B), block 256: small [B][128][128]
__global__ void __launch_bounds__(256) k_fx_resize(const uint8_t *__restrict__ gray, int H, int W, uint8_t *__restrict__ small)
{
    const int b = blockIdx.x;
    const uint8_t *g = gray + (size_t)b * H * W;
    uint8_t *o = small + (size_t)b * kFxSmall * kFxSmall;
    const bool area2 = H == 2 * kFxSmall && W == 2 * kFxSmall;  // is_area_fast, iscale 2 -> INTER_AREA: (a + b + c + d + 2) >> 2
    for (int i = threadIdx.x; i < kFxSmall * kFxSmall; i += 256) {
        const int dy = i / kFxSmall, dx = i % kFxSmall;
        if (area2) {
            const uint8_t *s = g + (size_t)(2 * dy) * W + 2 * dx;
            o[i] = (uint8_t)((s[0] + s[1] + s[W] + s[W + 1] + 2) >> 2);
            continue;
        }
        int x0, x1, a0, a1, y0, y1, b0, b1;
        resize_tap(dx, W, x0, x1, a0, a1);
        resize_tap(dy, H, y0, y1, b0, b1);
        const int S0 = g[(size_t)y0 * W + x0] * a0 + g[(size_t)y0 * W + x1] * a1;  // HResizeLinear
        const int S1 = g[(size_t)y1 * W + x0] * a0 + g[(size_t)y1 * W + x1] * a1;
        // VResizeLinearVec_32s8u: v_mul_hi of (S >> 4) with the 16-bit beta, then a rounding shift by 2 and u8 saturation
        const int v = (((S0 >> 4) * b0) >> 16) + (((S1 >> 4) * b1) >> 16);
        o[i] = sat_u8((v + 2) >> 2);
    }
}

// grid (4, B), block 256, dynamic LDS kFxGlcmLds.  graycomatrix(small, [1], [0, pi/4, pi/2, 3pi/4], 256, symmetric, normed) and
// graycoprops of angle blockIdx.x -> props [B][4][6]
__global__ void __launch_bounds__(256) k_fx_glcm(const uint8_t *__restrict__ small, double *__restrict__ props)
{
    extern __shared__ uint32_t lds[];
    uint32_t *cnt = lds;               // 32768 words: two u16 counts each (a symmetric count is <= 2 * 128 * 127 = 32512)
    uint32_t *dh = lds + 32768;        // |i - j| histogram of the directed pairs
    __shared__ long long s_red[4][5];
    __shared__ unsigned long long s_sq[4];
    const int a = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int orow = a == 0 ? 0 : 1, ocol = a == 0 ? 1 : a == 1 ? 1 : a == 2 ? 0 : -1;  // (round(sin), round(cos)) of the angle
    for (int i = tid; i < 32768 + 256; i += 256) lds[i] = 0;
    __syncthreads();
    const uint8_t *s = small + (size_t)b * kFxSmall * kFxSmall;
    const int r1 = kFxSmall - orow, c0 = max(0, -ocol), c1 = min(kFxSmall, kFxSmall - ocol), wc = c1 - c0;
    long long S1 = 0, S2 = 0, Sij = 0, Sc = 0, Sd = 0;
    for (int e = tid; e < r1 * wc; e += 256) {
        const int r = e / wc, c = c0 + e % wc;
        const int i = s[r * kFxSmall + c], j = s[(r + orow) * kFxSmall + c + ocol];
        const int ij = i * 256 + j, ji = j * 256 + i;
        atomicAdd(&cnt[ij >> 1], 1u << (16 * (ij & 1)));
        atomicAdd(&cnt[ji >> 1], 1u << (16 * (ji & 1)));
        const int d = i > j ? i - j : j - i;
        atomicAdd(&dh[d], 1u);
        S1 += i + j;
        S2 += i * i + j * j;
        Sij += 2 * i * j;
        Sc += 2 * d * d;
        Sd += 2 * d;
    }
    long long v[5] = {S1, S2, Sij, Sc, Sd};
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = (long long)wave_sum_u64((uint64_t)v[k]);
    if ((tid & 63) == 0)
        for (int k = 0; k < 5; ++k) s_red[tid >> 6][k] = v[k];
    __syncthreads();
    unsigned long long sq = 0;  // sum of the squared symmetric counts (ASM)
    for (int w = tid; w < 32768; w += 256) {
        const uint32_t x = cnt[w], lo = x & 0xffffu, hi = x >> 16;
        sq += (unsigned long long)lo * lo + (unsigned long long)hi * hi;
    }
    sq = wave_sum_u64(sq);
    if ((tid & 63) == 0) s_sq[tid >> 6] = sq;
    __syncthreads();
    if (tid != 0) return;
    long long t[5];
    for (int k = 0; k < 5; ++k) t[k] = s_red[0][k] + s_red[1][k] + s_red[2][k] + s_red[3][k];
    const long long T = 2ll * r1 * wc;  // symmetric count total
    const double Td = (double)T;
    double hom = 0.0;
    for (int d = 0; d < 256; ++d) hom += (double)(2ull * dh[d]) / (1.0 + (double)(d * d));
    const double asm_ = (double)(s_sq[0] + s_sq[1] + s_sq[2] + s_sq[3]) / (Td * Td);
    // correlation: with S1 = sum c_ij i (= sum c_ij j), var = (T sum c_ij i^2 - S1^2) / T^2, cov = (T sum c_ij i j - S1^2) / T^2,
    // all exact integers (graycoprops: 1 where a standard deviation is below 1e-15, i.e. var == 0)
    const long long ci = t[0], ci2 = t[1];
    const long long vnum = T * ci2 - ci * ci, cnum = T * t[2] - ci * ci;
    double *o = props + ((size_t)b * 4 + a) * kFxGlcmProps;
    o[0] = (double)t[3] / Td;
    o[1] = (double)t[4] / Td;
    o[2] = hom / Td;
    o[3] = sqrt(asm_);
    o[4] = vnum == 0 ? 1.0 : (double)cnum / (double)vnum;
    o[5] = asm_;
}

// the DCT of one dimension of length N: DCT-II output k is even (k = 2h, h < ne) or odd (k = 2h + 1, h < no); the two halves
// are padded to whole 64-wide blocks (nbe, nbo), so one block of outputs needs only the sums (even) or the differences (odd)
// x_n +- x_{N-1-n}, n < K
struct DctDim {
    int N, ne, no, nbe, K;
    float s0, sk;  // sqrt(1 / N), sqrt(2 / N)
};

__device__ __forceinline__ int dct_out(const DctDim &d, int blk, int pos)  // output index of position pos of block blk, -1: padding
{
    if (blk < d.nbe) {
        const int h = blk * 64 + pos;
        return h < d.ne ? 2 * h : -1;
    }
    const int h = (blk - d.nbe) * 64 + pos;
    return h < d.no ? 2 * h + 1 : -1;
}

// tab [4 W] then [4 H]: cos(pi m / (2 N)), m < 4N
__global__ void __launch_bounds__(256) k_fx_costab(int W, int H, float *__restrict__ tab)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 4 * W) tab[i] = (float)cospi((double)i / (2.0 * W));
    else if (i < 4 * W + 4 * H) tab[i] = (float)cospi((double)(i - 4 * W) / (2.0 * H));
}

// Z = gray . C_W^T, one wave per 64 x 64 block (4 x 4 tiles of v_mfma_f32_16x16x4_f32).  grid (nbe + nbo of W, cdiv(H, 64), B).
// A (16 x 4) = the data, lane l: row l & 15, n = l >> 4;  B (4 x 16) = cosines, lane l: n = l >> 4, output l & 15.
__global__ void __launch_bounds__(64) k_fx_dct_rows(const uint8_t *__restrict__ gray, int H, int W, DctDim dw,
                                                    const float *__restrict__ tab, float *__restrict__ z)
{
    const int b = blockIdx.z, lane = threadIdx.x, qb = blockIdx.x, r0 = blockIdx.y * 64;
    const int kk = lane >> 4, j = lane & 15;
    const bool odd = qb >= dw.nbe;
    const uint8_t *g = gray + (size_t)b * H * W;
    const uint32_t N4 = 4u * (uint32_t)W;
    int kout[4];
    uint32_t idx[4], step[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int k = dct_out(dw, qb, 16 * ni + j);
        kout[ni] = k;
        const uint64_t kk64 = (uint64_t)max(k, 0);
        idx[ni] = (uint32_t)((kk64 * (uint64_t)(2 * kk + 1)) % N4);
        step[ni] = (uint32_t)((8ull * kk64) % N4);
    }
    const uint8_t *rowp[4];
    bool rv[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int r = r0 + 16 * mi + j;
        rv[mi] = r < H;
        rowp[mi] = g + (size_t)min(r, H - 1) * W;
    }
    f32x4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int n0 = 0; n0 < dw.K; n0 += 4) {
        const int n = n0 + kk;
        const bool nv = n < dw.K;
        float av[4], bv[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            float v = 0.0f;
            if (nv && rv[mi]) {
                const float x0 = (float)rowp[mi][n];
                if (W == 1) v = x0;
                else {
                    const float x1 = (float)rowp[mi][W - 1 - n];
                    v = odd ? x0 - x1 : x0 + x1;
                }
            }
            av[mi] = v;
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            bv[ni] = (nv && kout[ni] >= 0) ? tab[idx[ni]] : 0.0f;
            idx[ni] += step[ni];
            if (idx[ni] >= N4) idx[ni] -= N4;
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
    // D: lane l holds rows 4 (l >> 4) + v, column l & 15
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int k = kout[ni];
        if (k < 0) continue;
        const float sc = k ? dw.sk : dw.s0;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = r0 + 16 * mi + 4 * kk + v;
                if (r < H) z[((size_t)b * H + r) * W + k] = acc[mi][ni][v] * sc;
            }
    }
}

// Y = C_H . Z with the reductions fused: grid (cdiv(W, 64), nbe + nbo of H, B).  A (16 x 4) = cosines, lane l: output row
// l & 15, r = l >> 4; B (4 x 16) = Z[r][c] +- Z[H-1-r][c], lane l: r = l >> 4, column l & 15.  part [B][nblk][5] (float64)
__global__ void __launch_bounds__(64) k_fx_dct_cols(const float *__restrict__ z, int H, int W, DctDim dh,
                                                    const float *__restrict__ tab, double *__restrict__ part)
{
    const int b = blockIdx.z, lane = threadIdx.x, pb = blockIdx.y, c0 = blockIdx.x * 64;
    const int kk = lane >> 4, j = lane & 15;
    const bool odd = pb >= dh.nbe;
    const float *zb = z + (size_t)b * H * W;
    const uint32_t N4 = 4u * (uint32_t)H;
    int kin[4];
    uint32_t idx[4], step[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int k = dct_out(dh, pb, 16 * mi + j);
        kin[mi] = k;
        const uint64_t k64 = (uint64_t)max(k, 0);
        idx[mi] = (uint32_t)((k64 * (uint64_t)(2 * kk + 1)) % N4);
        step[mi] = (uint32_t)((8ull * k64) % N4);
    }
    int col[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) col[ni] = c0 + 16 * ni + j;
    f32x4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int q0 = 0; q0 < dh.K; q0 += 4) {
        const int r = q0 + kk;
        const bool rv = r < dh.K;
        float av[4], bv[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            av[mi] = (rv && kin[mi] >= 0) ? tab[idx[mi]] : 0.0f;
            idx[mi] += step[mi];
            if (idx[mi] >= N4) idx[mi] -= N4;
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            float v = 0.0f;
            if (rv && col[ni] < W) {
                const float x0 = zb[(size_t)r * W + col[ni]];
                if (H == 1) v = x0;
                else {
                    const float x1 = zb[(size_t)(H - 1 - r) * W + col[ni]];
                    v = odd ? x0 - x1 : x0 + x1;
                }
            }
            bv[ni] = v;
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
    // feature_extraction.py:143-158: regions [:h//4, :w//4], [h//4:h//2, w//4:w//2], [h//2:, w//2:] of the (k, c) plane
    const int h4 = H / 4, h2 = H / 2, w4 = W / 4, w2 = W / 2;
    double s[kFxDctSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int k = dct_out(dh, pb, 16 * mi + 4 * kk + v);
            if (k < 0) continue;
            const float sc = k ? dh.sk : dh.s0;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int c = col[ni];
                if (c >= W) continue;
                const float y = acc[mi][ni][v] * sc;
                const double e = (double)y * (double)y;
                if (k < h4 && c < w4) s[0] += e;
                if (k >= h4 && k < h2 && c >= w4 && c < w2) s[1] += e;
                if (k >= h2 && c >= w2) s[2] += e;
                s[3] += e;
                s[4] += fabs((double)y);
            }
        }
#pragma unroll
    for (int i = 0; i < kFxDctSums; ++i) s[i] = wave_sum_f64(s[i]);
    if (lane < kFxDctSums) {
        double mine = s[0];
#pragma unroll
        for (int i = 1; i < kFxDctSums; ++i)
            if (lane == i) mine = s[i];
        part[(((size_t)b * gridDim.y + pb) * gridDim.x + blockIdx.x) * kFxDctSums + lane] = mine;
    }
}

struct FxArgs {
    int B, H, W, nA, nB, nD, nf, has_f32;
};

__device__ double hist_moments(const uint32_t *h, double n, double *mean, double *m3, double *m4)
{
    double s = 0.0;
    for (int k = 0; k < 256; ++k) s += (double)h[k] * (double)k;
    const double m = s / n;
    double m2 = 0.0, a3 = 0.0, a4 = 0.0;
    for (int k = 0; k < 256; ++k) {
        if (!h[k]) continue;
        const double d = (double)k - m, d2 = d * d;
        m2 += (double)h[k] * d2;
        a3 += (double)h[k] * d2 * d;
        a4 += (double)h[k] * d2 * d2;
    }
    *mean = m;
    if (m3) *m3 = a3 / n;
    if (m4) *m4 = a4 / n;
    return m2 / n;
}

// mean and variance of x_k = float32(k) / 255 (the float32 values NumPy holds) weighted by the histogram
__device__ double hist_norm_var(const uint32_t *h, double n, double *mean)
{
    double s = 0.0;
    for (int k = 0; k < 256; ++k) s += (double)h[k] * (double)px_norm(k);
    const double m = s / n;
    double v = 0.0;
    for (int k = 0; k < 256; ++k) {
        const double d = (double)px_norm(k) - m;
        v += (double)h[k] * d * d;
    }
    *mean = m;
    return v / n;
}

__device__ int hist_order(const uint32_t *h, long long i)  // byte value of the i-th smallest element
{
    long long c = 0;
    for (int k = 0; k < 256; ++k) {
        c += h[k];
        if (c > i) return k;
    }
    return 255;
}

// np.percentile(float32 x, q), method 'linear', in NumPy 2's float32 arithmetic: q32 = q / float32(100),
// vi = float32(n - 1) * q32, gamma = vi - floor(vi), lerp a + d * g (g < 0.5) or b - d * (1 - g)
__device__ float hist_percentile(const uint32_t *h, long long n, float q)
{
    const float q32 = q / 100.0f;
    const float vi = (float)(n - 1) * q32;
    const float fl = floorf(vi);
    long long lo = (long long)fl, hi = lo + 1;
    if (vi >= (float)(n - 1)) lo = hi = n - 1;
    const float g = vi - fl;
    const float a = px_norm(hist_order(h, lo)), bb = px_norm(hist_order(h, hi));
    const float d = bb - a;
    return g >= 0.5f ? bb - d * (1.0f - g) : a + d * g;
}

// grid (B), block 64: one wave per frame.  The lanes sum the per-block partials (strided, then a butterfly: a fixed order) and
// stage the frame's histograms in LDS; lane 0 evaluates the values.
__global__ void __launch_bounds__(64) k_fx_finish(FxArgs A, const uint32_t *__restrict__ hist, const double *__restrict__ fpart,
                                                  const uint32_t *__restrict__ fmm, const uint32_t *__restrict__ lbp,
                                                  const unsigned long long *__restrict__ isum, const uint32_t *__restrict__ gmax,
                                                  const double *__restrict__ mpart, const uint32_t *__restrict__ edges,
                                                  const double *__restrict__ props, const double *__restrict__ dpart,
                                                  uint32_t *__restrict__ status, double *__restrict__ out)
{
    __shared__ uint32_t s_hist[kFxHist * 256];
    const int b = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < kFxHist * 256; i += 64) s_hist[i] = hist[(size_t)b * kFxHist * 256 + i];
    double fs[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ds[kFxDctSums] = {0.0, 0.0, 0.0, 0.0, 0.0}, sm = 0.0;
    if (A.has_f32)
        for (int i = lane; i < A.nA; i += 64)
            for (int k = 0; k < 6; ++k) fs[k] += fpart[((size_t)b * A.nA + i) * 6 + k];
    for (int i = lane; i < A.nD; i += 64)
        for (int k = 0; k < kFxDctSums; ++k) ds[k] += dpart[((size_t)b * A.nD + i) * kFxDctSums + k];
    for (int i = lane; i < A.nB; i += 64) sm += mpart[(size_t)b * A.nB + i];
    for (int k = 0; k < 6; ++k) fs[k] = wave_sum_f64(fs[k]);
    for (int k = 0; k < kFxDctSums; ++k) ds[k] = wave_sum_f64(ds[k]);
    sm = wave_sum_f64(sm);
    __syncthreads();
    if (lane != 0) return;
    const uint32_t *hb = s_hist;
    const long long npx = (long long)A.H * A.W;
    const double n = (double)npx;
    double *o = out + (size_t)b * A.nf;
    int j = 0;
    // an invariant: every pixel is in each histogram once
    long long tot_g = 0, tot_l = 0;
    for (int k = 0; k < 256; ++k) tot_g += hb[9 * 256 + k];
    for (int k = 0; k < 10; ++k) tot_l += lbp[b * 10 + k];
    if (status && (tot_g != npx || tot_l != npx)) atomicOr(status, (uint32_t)UWIE_STATUS_FEATURE_COUNTS);
    // colour (feature_extraction.py:30-41): L, a, b -> mean, std, skew, kurtosis (SciPy: NaN when m2 <= (eps32 * mean)^2)
    const double eps32 = 1.1920928955078125e-07;
    double mlab[3];
    for (int c = 0; c < 3; ++c) {
        double m, m3, m4;
        const double m2 = hist_moments(hb + (3 + c) * 256, n, &m, &m3, &m4);
        mlab[c] = m;
        const bool zero = m2 <= (eps32 * m) * (eps32 * m);
        o[j++] = m;
        o[j++] = sqrt(m2);
        o[j++] = zero ? __longlong_as_double(0x7ff8000000000000ll) : m3 / (m2 * sqrt(m2));
        o[j++] = zero ? __longlong_as_double(0x7ff8000000000000ll) : m4 / (m2 * m2) - 3.0;
    }
    for (int c = 0; c < 3; ++c) {  // :44-51 HSV
        double m;
        const double m2 = hist_moments(hb + (6 + c) * 256, n, &m, nullptr, nullptr);
        o[j++] = m;
        o[j++] = sqrt(m2);
    }
    {  // :54-66 colour cast factor
        double da = 0.0, db = 0.0;
        for (int k = 0; k < 256; ++k) {
            da += (double)hb[4 * 256 + k] * fabs((double)k - mlab[1]);
            db += (double)hb[5 * 256 + k] * fabs((double)k - mlab[2]);
        }
        da /= n;
        db /= n;
        const double M = sqrt(mlab[1] * mlab[1] + mlab[2] * mlab[2]), Dd = sqrt(da * da + db * db);
        o[j++] = M / (Dd + 1e-10);
        o[j++] = M;
        o[j++] = Dd;
        o[j++] = mlab[1];
        o[j++] = mlab[2];
    }
    for (int c = 0; c < 3; ++c) {  // :69-76 the float image's channels
        if (A.has_f32) {
            const double s = fs[2 * c], q = fs[2 * c + 1];
            const double m = s / n;
            o[j++] = m;
            o[j++] = sqrt(fmax(q / n - m * m, 0.0));
            o[j++] = (double)key_f32(fmm[b * 6 + 2 * c]);
            o[j++] = (double)key_f32(fmm[b * 6 + 2 * c + 1]);
        } else {
            const uint32_t *h = hb + c * 256;
            double m;
            const double v = hist_norm_var(h, n, &m);
            int lo = 0, hi = 255;
            while (!h[lo]) ++lo;
            while (!h[hi]) --hi;
            o[j++] = m;
            o[j++] = sqrt(v);
            o[j++] = (double)px_norm(lo);
            o[j++] = (double)px_norm(hi);
        }
    }
    // texture (:92-124): LBP histogram (density: count / total), GLCM props as mean and std over the 4 angles
    for (int k = 0; k < 10; ++k) o[j++] = (double)lbp[b * 10 + k] / n;
    for (int p = 0; p < kFxGlcmProps; ++p) {
        const double *pv = props + (size_t)b * 4 * kFxGlcmProps + p;
        const double m = (((pv[0] + pv[kFxGlcmProps]) + pv[2 * kFxGlcmProps]) + pv[3 * kFxGlcmProps]) / 4.0;
        double v = 0.0;
        for (int a = 0; a < 4; ++a) v += (pv[a * kFxGlcmProps] - m) * (pv[a * kFxGlcmProps] - m);
        o[j++] = m;
        o[j++] = sqrt(v / 4.0);
    }
    // frequency (:136-163), frames whose dimensions are even or 1
    if (A.nD) {
        const double *s = ds;
        const double ma = s[4] / n;
        o[j++] = s[0] / s[3];
        o[j++] = s[1] / s[3];
        o[j++] = s[2] / s[3];
        o[j++] = ma;
        o[j++] = sqrt(fmax(s[3] / n - ma * ma, 0.0));
    }
    // edges (:174-204): Sobel magnitude of gray / 255, Canny density, Laplacian
    {
        const unsigned long long *is = isum + (size_t)b * 4;
        const double mm = sm / 255.0 / n, q = (double)is[3] / (255.0 * 255.0) / n;
        o[j++] = mm;
        o[j++] = sqrt(fmax(q - mm * mm, 0.0));
        o[j++] = sqrt((double)gmax[b]) / 255.0;
        o[j++] = (double)edges[b] / n;
        const double l1 = (double)(long long)is[1] / n, l2 = (double)(long long)is[2] / n;
        const double var = fmax(l2 - l1 * l1, 0.0);
        o[j++] = (double)(long long)is[0] / n;
        o[j++] = sqrt(var);
        o[j++] = var;
    }
    // quality (:217-248) on gray / 255 and S / 255
    {
        const uint32_t *h = hb + 9 * 256;
        double m;
        const double v = hist_norm_var(h, n, &m);
        double ent = 0.0;
        for (int k = 0; k < 256; ++k)
            if (h[k]) {
                const double pk = (double)h[k] / n;
                ent -= pk * log(pk);
            }
        const float med = (npx & 1) ? px_norm(hist_order(h, npx / 2))
                                    : (px_norm(hist_order(h, npx / 2 - 1)) + px_norm(hist_order(h, npx / 2))) / 2.0f;
        int lo = 0, hi = 255;
        while (!h[lo]) ++lo;
        while (!h[hi]) --hi;
        double ms;
        const double vs = hist_norm_var(hb + 7 * 256, n, &ms);
        o[j++] = sqrt(v);
        o[j++] = ent / log(2.0);
        o[j++] = m;
        o[j++] = (double)med;
        o[j++] = (double)hist_percentile(h, npx, 25.0f);
        o[j++] = (double)hist_percentile(h, npx, 75.0f);
        o[j++] = (double)(px_norm(hi) - px_norm(lo));
        o[j++] = ms;
        o[j++] = sqrt(vs);
        o[j++] = sqrt(v);
    }
}

DctDim dct_dim(int N)
{
    DctDim d;
    d.N = N;
    d.ne = (N + 1) / 2;
    d.no = N / 2;
    d.nbe = cdiv(d.ne, 64);
    d.K = N == 1 ? 1 : N / 2;
    d.s0 = (float)sqrt(1.0 / N);
    d.sk = (float)sqrt(2.0 / N);
    return d;
}

struct FxBufs {
    uint8_t *gray, *small;
    uint32_t *hist, *fmm, *lbp, *gmax, *edges;
    unsigned long long *isum;
    double *fpart, *mpart, *props, *dpart;
    Region *regs;
    void *canny;
    float *z, *tab;
    int nA, nB, nD;
};

FxBufs carve_fx(Carver &c, Shape s)
{
    FxBufs f;
    const DctDim dw = dct_dim(s.W), dh = dct_dim(s.H);
    f.nA = f.nB = grid_for(s.npx(), kFxMapsCap);
    f.nD = feature_extractor_has_dct(s.H, s.W) ? cdiv(s.W, 64) * (dh.nbe + cdiv(dh.no, 64)) : 0;
    (void)dw;
    f.gray = c.take<uint8_t>((size_t)s.B * s.npx());
    f.hist = c.take<uint32_t>((size_t)s.B * kFxHist * 256);
    f.fmm = c.take<uint32_t>((size_t)s.B * 6);
    f.lbp = c.take<uint32_t>((size_t)s.B * 10);
    f.isum = c.take<unsigned long long>((size_t)s.B * 4);
    f.gmax = c.take<uint32_t>(s.B);
    f.edges = c.take<uint32_t>(s.B);
    f.fpart = c.take<double>((size_t)s.B * f.nA * 6);
    f.mpart = c.take<double>((size_t)s.B * f.nB);
    f.props = c.take<double>((size_t)s.B * 4 * kFxGlcmProps);
    f.small = c.take<uint8_t>((size_t)s.B * kFxSmall * kFxSmall);
    f.regs = c.take<Region>(s.B);
    f.canny = c.take<char>(canny_ws_bytes(s));
    f.z = f.nD ? c.take<float>((size_t)s.B * s.npx()) : nullptr;
    f.tab = f.nD ? c.take<float>(4 * ((size_t)s.W + s.H)) : nullptr;
    f.dpart = f.nD ? c.take<double>((size_t)s.B * f.nD * kFxDctSums) : nullptr;
    return f;
}

}  // namespace

bool feature_extractor_has_dct(int H, int W) { return (H == 1 || H % 2 == 0) && (W == 1 || W % 2 == 0); }

int feature_extractor_count(int H, int W) { return feature_extractor_has_dct(H, W) ? 79 : 74; }

size_t feature_extractor_ws_bytes(Shape s)
{
    Carver c(nullptr);
    carve_fx(c, s);
    return c.total();
}

int launch_feature_extractor(uwie_ctx *ctx, const uint8_t *d_u8, const float *d_f32, Shape s, int gray_shift, double *d_out,
                             void *ws, hipStream_t st)
{
    Carver c(ws);
    FxBufs f = carve_fx(c, s);
    const int npx = (int)s.npx();
    UWIE_HIP_CHECK(hipMemsetAsync(f.hist, 0, sizeof(uint32_t) * (size_t)s.B * kFxHist * 256, st));
    UWIE_HIP_CHECK(hipMemsetAsync(f.lbp, 0, sizeof(uint32_t) * (size_t)s.B * 10, st));
    UWIE_HIP_CHECK(hipMemsetAsync(f.isum, 0, sizeof(unsigned long long) * (size_t)s.B * 4, st));
    UWIE_HIP_CHECK(hipMemsetAsync(f.gmax, 0, sizeof(uint32_t) * (size_t)s.B, st));
    if (d_f32) {
        UWIE_HIP_CHECK(hipMemsetAsync(f.fmm, 0, sizeof(uint32_t) * (size_t)s.B * 6, st));  // maxima start at key 0
        for (int i = 0; i < 3; ++i)  // minima start at the largest key
            UWIE_HIP_CHECK(hipMemset2DAsync(f.fmm + 2 * i, 6 * sizeof(uint32_t), 0xff, sizeof(uint32_t), s.B, st));
    }
    UWIE_LAUNCH(k_fx_maps, dim3(f.nA, s.B), dim3(256), 0, st, ctx->d_lab, d_u8, d_f32, npx, gray_shift, f.gray, f.hist, f.fpart, f.fmm);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_fx_stencil, dim3(f.nB, s.B), dim3(256), 0, st, f.gray, s.H, s.W, f.lbp, f.isum, f.gmax, f.mpart);
    UWIE_LAUNCH_CHECK();
    int rc = launch_make_full_regions(f.regs, s, st);
    if (rc != UWIE_OK) return rc;
    rc = launch_canny(f.gray, s, f.regs, s.B, s.H, s.W, 50, 150, f.edges, nullptr, f.canny, st);
    if (rc != UWIE_OK) return rc;
    UWIE_LAUNCH(k_fx_resize, dim3(s.B), dim3(256), 0, st, f.gray, s.H, s.W, f.small);
    UWIE_LAUNCH_CHECK();
    UWIE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fx_glcm), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kFxGlcmLds));
    UWIE_LAUNCH(k_fx_glcm, dim3(4, s.B), dim3(256), kFxGlcmLds, st, f.small, f.props);
    UWIE_LAUNCH_CHECK();
    if (f.nD) {
        const DctDim dw = dct_dim(s.W), dh = dct_dim(s.H);
        UWIE_LAUNCH(k_fx_costab, dim3(cdiv(4ll * (s.W + s.H), 256)), dim3(256), 0, st, s.W, s.H, f.tab);
        UWIE_LAUNCH_CHECK();
        UWIE_LAUNCH(k_fx_dct_rows, dim3(dw.nbe + cdiv(dw.no, 64), cdiv(s.H, 64), s.B), dim3(64), 0, st, f.gray, s.H, s.W, dw, f.tab, f.z);
        UWIE_LAUNCH_CHECK();
        UWIE_LAUNCH(k_fx_dct_cols, dim3(cdiv(s.W, 64), dh.nbe + cdiv(dh.no, 64), s.B), dim3(64), 0, st, f.z, s.H, s.W, dh,
                    f.tab + 4 * (size_t)s.W, f.dpart);
        UWIE_LAUNCH_CHECK();
    }
    const FxArgs A{s.B, s.H, s.W, f.nA, f.nB, f.nD, feature_extractor_count(s.H, s.W), d_f32 != nullptr};
    UWIE_LAUNCH(k_fx_finish, dim3(s.B), dim3(64), 0, st, A, f.hist, f.fpart, f.fmm, f.lbp, f.isum, f.gmax, f.mpart,
                f.edges, f.props, f.dpart, ctx->d_status, d_out);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
