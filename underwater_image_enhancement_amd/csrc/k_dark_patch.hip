// Dark channel over a k x k patch (uwie_params.dark_patch > 1; no reference counterpart: the reference's dark channel is
// the minimum over the three channels of ONE pixel, six_stadigy.py:170-174 / enhancement_strategies.py:221-225).
//
//   k_trans_patch   t0 = 1 - omega * erode_k(min_c(img_c / (A_c + eps))) [clip], float32, one launch for the batch
//
// erode_k is cv2.erode with a k x k rectangle, its default centre anchor a = k / 2 and its default border: the window of
// (y, x) is rows y - a .. y + k - 1 - a and columns x - a .. x + k - 1 - a, clipped to the frame (pixels outside never
// win).  A minimum has no rounding, so every order of taking it gives the same bits, and it commutes with the
// non-decreasing per-channel maps in front of it: the plane equals k_trans_init's of the frame whose channels were eroded
// as bytes ("Dark channel over a patch").
//
// One 256-thread block per kPatchTW x kPatchTH tile of outputs:
//   1. the 768 quotients of k_trans_init (the same IEEE divisions) into LDS;
//   2. the tile's per-pixel dark values with a halo of a rows / columns before it and k - 1 - a behind it into an LDS
//      plane (the halo columns rounded outwards to whole 4-pixel groups), kBig where the frame ends;
//   3. column minimum: a thread takes four output rows of a 4-column group, reads the k + 3 rows they need as float4
//      and shares the minimum of the rows common to all four windows; the results replace the plane's first TH rows;
//   4. row minimum: a thread per output, k neighbouring LDS words (lanes on consecutive words: no bank conflict), then
//      1 - omega * m and the clip; the results go back through LDS so that they leave as float4.
// Nothing but the frame is read from memory and nothing but t0 is written.
#include "common.h"
#include "devutil.h"

namespace uwie {
namespace {

constexpr int kPatchTW = 128, kPatchTH = 32;
constexpr float kBig = 3.0e38f;  // above every quotient (255/255 / 1e-10 at most)

__device__ __forceinline__ float4 min4(const float4 &a, const float4 &b)
{
    return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), fminf(a.w, b.w));
}

// Layout of the LDS plane for patch k: aL / aR halo columns (multiples of 4) left and right of the tile, LW words per row,
// LH rows; s = aL - a is where the window of output column 0 starts.
struct PatchGeom {
    int a, aL, LW, LH, s;
};
__host__ __device__ __forceinline__ PatchGeom patch_geom(int k)
{
    PatchGeom g;
    g.a = k / 2;
    g.aL = (g.a + 3) & ~3;
    const int aR = (k - 1 - g.a + 3) & ~3;
    g.LW = g.aL + kPatchTW + aR;
    g.LH = kPatchTH + k - 1;
    g.s = g.aL - g.a;
    return g;
}

__global__ void __launch_bounds__(256) k_trans_patch(const uint8_t *__restrict__ in, const int32_t *__restrict__ kind,
                                                     const float *__restrict__ A, int H, int W, int k, float omega, float norm_eps,
                                                     int pre_clip, float *__restrict__ t0)
{
    extern __shared__ float4 lds4[];
    float *nrm = reinterpret_cast<float *>(lds4);  // [3][256]
    float *d = nrm + 768;                          // [LH][LW]
    const PatchGeom g = patch_geom(k);
    const int LW = g.LW, LH = g.LH;
    const int b = blockIdx.z, tid = threadIdx.x;
    const int x0 = blockIdx.x * kPatchTW, y0 = blockIdx.y * kPatchTH;
    const int kd = kind ? kind[b] : 0;
    const size_t npx = (size_t)H * W;
    const uint8_t *img = in + (size_t)b * npx * 3;  // this frame only: the border rule is per frame
    for (int i = tid; i < 768; i += 256) {
        const int c = i >> 8;
        nrm[i] = px_val(i & 255, px_atten(kd, c)) / (A[b * 3 + c] + norm_eps);  // S6:170 / ES:221, as k_trans_init
    }
    __syncthreads();
    auto dark = [&](uint32_t r, uint32_t gg, uint32_t bb) { return fminf(fminf(nrm[r], nrm[256 + gg]), nrm[512 + bb]); };

    // ---- 2. dark values of the tile and its halo.  Loads are unconditional, from clamped positions; what lies outside the
    // frame is replaced afterwards.
    const int ytop = y0 - g.a, xleft = x0 - g.aL;
    if ((W & 3) == 0) {
        // whole 4-pixel groups, 12 bytes at a 4-byte aligned address (W and xleft are multiples of 4)
        const int ngx = LW >> 2, n = LH * ngx;
        for (int i = tid; i < n; i += 256) {
            const int j = i / ngx, q = i - j * ngx;
            const int y = ytop + j, x = xleft + 4 * q;
            const bool inside = y >= 0 && y < H && x >= 0 && x < W;
            const int yc = min(max(y, 0), H - 1), xc = min(max(x, 0), W - 4);
            const uint3 w = *reinterpret_cast<const uint3 *>(img + ((size_t)yc * W + xc) * 3);
            float4 v;
            v.x = dark(w.x & 255, (w.x >> 8) & 255, (w.x >> 16) & 255);
            v.y = dark(w.x >> 24, w.y & 255, (w.y >> 8) & 255);
            v.z = dark((w.y >> 16) & 255, w.y >> 24, w.z & 255);
            v.w = dark((w.z >> 8) & 255, (w.z >> 16) & 255, w.z >> 24);
            if (!inside) v = make_float4(kBig, kBig, kBig, kBig);
            *reinterpret_cast<float4 *>(d + j * LW + 4 * q) = v;
        }
    } else {
        // ragged widths: pixel by pixel
        const int n = LH * LW;
        for (int i = tid; i < n; i += 256) {
            const int j = i / LW, c = i - j * LW;
            const int y = ytop + j, x = xleft + c;
            const bool inside = y >= 0 && y < H && x >= 0 && x < W;
            const int yc = min(max(y, 0), H - 1), xc = min(max(x, 0), W - 1);
            const uint8_t *p = img + ((size_t)yc * W + xc) * 3;
            const float v = dark(p[0], p[1], p[2]);
            d[i] = inside ? v : kBig;
        }
    }
    __syncthreads();

    // ---- 3. column minimum: item = (four output rows 4*y4 .. 4*y4 + 3, column group q); row r's window is LDS rows r .. r + k - 1
    const int ngx = LW >> 2, nitems = (kPatchTH / 4) * ngx;  // <= 8 * 40
    float4 col[2][4];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int i = tid + it * 256;
        if (i < nitems) {
            const int y4 = i / ngx, q = i - y4 * ngx;
            const float4 *p = reinterpret_cast<const float4 *>(d + (4 * y4) * LW + 4 * q);
            const int rs = LW >> 2;  // row stride in float4
            float4 o[4];
            if (k >= 4) {
                // rows 3 .. k - 1 are in all four windows
                float4 c = p[3 * rs];
                for (int e = 4; e < k; ++e) c = min4(c, p[e * rs]);
                const float4 h0 = p[0], h1 = p[rs], h2 = p[2 * rs];
                const float4 e0 = p[k * rs], e1 = p[(k + 1) * rs], e2 = p[(k + 2) * rs];
                const float4 h12 = min4(h1, h2), e01 = min4(e0, e1);
                o[0] = min4(c, min4(h0, h12));
                o[1] = min4(c, min4(h12, e0));
                o[2] = min4(c, min4(h2, e01));
                o[3] = min4(c, min4(e01, e2));
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float4 m = p[r * rs];
                    for (int e = 1; e < k; ++e) m = min4(m, p[(r + e) * rs]);
                    o[r] = m;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) col[it][r] = o[r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int i = tid + it * 256;
        if (i < nitems) {
            const int y4 = i / ngx, q = i - y4 * ngx;
#pragma unroll
            for (int r = 0; r < 4; ++r) *reinterpret_cast<float4 *>(d + (4 * y4 + r) * LW + 4 * q) = col[it][r];
        }
    }
    __syncthreads();

    // ---- 4. row minimum: output (y, c) reads LDS columns c + s .. c + s + k - 1 of row y
    constexpr int kPer = kPatchTW * kPatchTH / 256;
    float t[kPer];
#pragma unroll
    for (int it = 0; it < kPer; ++it) {
        const int i = tid + it * 256;
        const int y = i / kPatchTW, c = i - y * kPatchTW;
        const float *p = d + y * LW + c + g.s;
        float m = p[0];
        for (int e = 1; e < k; ++e) m = fminf(m, p[e]);
        float v = 1.0f - omega * m;
        if (pre_clip) v = fminf(fmaxf(v, 0.1f), 1.0f);
        t[it] = v;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kPer; ++it) {
        const int i = tid + it * 256;
        const int y = i / kPatchTW, c = i - y * kPatchTW;
        d[y * LW + c] = t[it];
    }
    __syncthreads();

    // ---- store: four rows of one 4-column group per thread (a wavefront writes two 512-byte row segments per row index)
    float *plane = t0 + (size_t)b * npx;
    const int c4 = tid & 31, y4 = tid >> 5;
    const int x = x0 + 4 * c4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yl = 4 * y4 + r, y = y0 + yl;
        if (y >= H || x >= W) continue;
        const float4 v = *reinterpret_cast<const float4 *>(d + yl * LW + 4 * c4);
        float *o = plane + (size_t)y * W + x;
        if ((W & 3) == 0) {
            *reinterpret_cast<float4 *>(o) = v;  // x + 3 < W, and every row starts on a 16-byte boundary
        } else {
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) o[i] = e[i];
        }
    }
}

}  // namespace

void dark_patch_tile(int *tile_w, int *tile_h)
{
    *tile_w = kPatchTW;
    *tile_h = kPatchTH;
}

int launch_trans_patch(const uint8_t *d_in, const int32_t *d_kind, const float *d_A, Shape s, int k, float omega, float norm_eps,
                       int pre_clip, float *d_t0, hipStream_t st)
{
    UWIE_REQUIRE(k >= 2 && k <= 31, "dark_patch out of range");
    UWIE_REQUIRE(s.B <= 65535 && cdiv(s.H, kPatchTH) <= 65535, "dark_patch: batch or frame height beyond one launch's grid");
    const PatchGeom g = patch_geom(k);
    const size_t lds = (768 + (size_t)g.LH * g.LW) * sizeof(float);  // <= 3 KB + 62 * 160 * 4 = 42.7 KB
    UWIE_LAUNCH(k_trans_patch, dim3(cdiv(s.W, kPatchTW), cdiv(s.H, kPatchTH), s.B), dim3(256), lds, st, d_in, d_kind, d_A, s.H, s.W,
                k, omega, norm_eps, pre_clip, d_t0);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
