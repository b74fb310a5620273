// cv2.resize(frame, dsize) of a ragged batch of RGB u8 frames to the trainer's input:
//   k_resize_rgb   one workgroup per (band of output rows, frame): OpenCV's fixed-point INTER_LINEAR (the INTER_AREA fast
//                  path for an exact 2x reduction, a copy at equal size), an optional fliplr / flipud of the result, and any
//                  of three outputs: u8 [B][oh][ow][3], float32 [B][3][oh][ow] = v / 255, and the same planes normalised
//                  ((v / 255 - mean[c]) / std[c], two float32 operations).
// The frames come from a device table of uwie_frame_desc (pointer, H, W), so a packed upload and separate tensors need no
// copy.  No float reductions and no atomics on results: an output element depends on its frame alone.
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsBand = 4;            // output rows per workgroup when ow <= kRsBandWide
constexpr int kRsBandWide = 1024;     // wider rows: one row per workgroup (bounds the LDS staging of the u8 band)
constexpr int kRsVecBytes = 16;       // OpenCV's baseline SIMD width in VResizeLinearVec_32s8u (see vertical_tail_start)
constexpr int kRsCoefBits = 11;       // INTER_RESIZE_COEF_BITS
constexpr int kRsCoefScale = 1 << kRsCoefBits;

struct RsNorm {
    float mean[3], stdv[3];
};


// one coordinate's float32 source position (float)((d + 0.5) * scale - 0.5), scale = 1 / (dst / src) in double: the floor
// and the fraction
__device__ __forceinline__ void rs_coord(int d, int src, int dst, int &s, float &f)
{
    const double scale = 1.0 / ((double)dst / (double)src);
    f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
}

__device__ __forceinline__ int rs_coef(float c) { return __float2int_rn(c * (float)kRsCoefScale); }

// VResizeLinear's element rule: the vector pass ((S0 >> 4) * b0 >> 16) + ((S1 >> 4) * b1 >> 16), (v + 2) >> 2 for the
// elements before `tail`, FixedPtCast<int, uchar, 22> after it
__device__ __forceinline__ uint8_t rs_vertical(int S0, int S1, int b0, int b1, bool scalar)
{
    if (scalar) return sat_u8((S0 * b0 + S1 * b1 + (1 << (2 * kRsCoefBits - 1))) >> (2 * kRsCoefBits));
    const int v = (((S0 >> 4) * b0) >> 16) + (((S1 >> 4) * b1) >> 16);
    return sat_u8((v + 2) >> 2);
}

// First element of a row of `width` bytes past OpenCV's vector loops: whole kRsVecBytes chunks while x <= width - 16,
// then half chunks while x < width - 8.
__device__ __forceinline__ int rs_tail_start(int width)
{
    int x = (width / kRsVecBytes) * kRsVecBytes;
    while (x < width - kRsVecBytes / 2) x += kRsVecBytes / 2;
    return x;
}

// grid (bands, B), block 256, dynamic LDS ow * 8 + band * ow * 3 bytes.
__global__ void __launch_bounds__(kRsThreads) k_resize_rgb(const uwie_frame_desc *__restrict__ desc, int oh, int ow, int band,
                                                           const uint8_t *__restrict__ flips, uint8_t *__restrict__ out_u8,
                                                           float *__restrict__ out_f32, float *__restrict__ out_norm, RsNorm nm,
                                                           uint32_t *__restrict__ status)
{
    extern __shared__ int rs_lds[];
    int *s_x0 = rs_lds;                                          // [ow] source column of tap 0
    int *s_ab = rs_lds + ow;                                     // [ow] alpha0 | alpha1 << 16
    uint8_t *s_row = reinterpret_cast<uint8_t *>(rs_lds + 2 * ow);  // [band][ow * 3] the u8 band, in output order
    const int b = blockIdx.y, tid = threadIdx.x;
    const uwie_frame_desc d = desc[b];
    const int H = d.H, W = d.W;
    if (!d.data || H < 1 || W < 1 || H > UWIE_RESIZE_MAX_SRC || W > UWIE_RESIZE_MAX_SRC) {
        if (tid == 0 && blockIdx.x == 0) atomicOr(status, (uint32_t)UWIE_STATUS_RESIZE_DESC);
        return;
    }
    const int fl = flips ? flips[b] : 0;
    const bool lr = fl & UWIE_FLIP_LR, ud = fl & UWIE_FLIP_UD;
    const int mode = (H == oh && W == ow) ? 0 : (H == 2 * oh && W == 2 * ow) ? 1 : 2;  // copy, INTER_AREA 2x, linear
    if (mode == 2) {
        for (int x = tid; x < ow; x += kRsThreads) {
            int s;
            float f;
            rs_coord(x, W, ow, s, f);
            if (s < 0) { f = 0.0f; s = 0; }                    // resizeGeneric's xmin / xmax clamps
            if (s >= W - 1) { f = 0.0f; s = W - 1; }
            s_x0[x] = s;
            s_ab[x] = (rs_coef(1.0f - f) & 0xffff) | (rs_coef(f) << 16);
        }
        __syncthreads();
    }
    const int y0 = blockIdx.x * band, y1 = min(y0 + band, oh);
    const int w3 = ow * 3, tail = rs_tail_start(w3);
    const uint8_t *src = d.data;
    const size_t pitch = (size_t)W * 3;
    for (int y = y0; y < y1; ++y) {
        const int ry = ud ? oh - 1 - y : y;  // row of the resized frame
        const uint8_t *r0, *r1;
        int b0 = 0, b1 = 0;
        if (mode == 0) {
            r0 = r1 = src + (size_t)ry * pitch;
        } else if (mode == 1) {
            r0 = src + (size_t)(2 * ry) * pitch;
            r1 = r0 + pitch;
        } else {  // rows: the fraction is kept, the two indices are clipped (resizeGeneric's ibeta and the invoker's clip)
            int s;
            float f;
            rs_coord(ry, H, oh, s, f);
            r0 = src + (size_t)min(max(s, 0), H - 1) * pitch;
            r1 = src + (size_t)min(max(s + 1, 0), H - 1) * pitch;
            b0 = rs_coef(1.0f - f);
            b1 = rs_coef(f);
        }
        for (int x = tid; x < ow; x += kRsThreads) {
            const int rx = lr ? ow - 1 - x : x;  // column of the resized frame
            uint8_t v[3];
            if (mode == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = r0[rx * 3 + c];
            } else if (mode == 1) {
                const int o = 6 * rx;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = (uint8_t)((r0[o + c] + r0[o + 3 + c] + r1[o + c] + r1[o + 3 + c] + 2) >> 2);
            } else {
                const int sx = s_x0[rx], ab = s_ab[rx];
                const int a0 = (int)(short)(ab & 0xffff), a1 = ab >> 16;
                const int o0 = 3 * sx, o1 = 3 * min(sx + 1, W - 1);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int S0 = r0[o0 + c] * a0 + r0[o1 + c] * a1;  // HResizeLinear, exact in int
                    const int S1 = r1[o0 + c] * a0 + r1[o1 + c] * a1;
                    v[c] = rs_vertical(S0, S1, b0, b1, rx * 3 + c >= tail);
                }
            }
            if (out_u8) {
                uint8_t *o = s_row + (size_t)(y - y0) * w3 + 3 * x;
                o[0] = v[0], o[1] = v[1], o[2] = v[2];
            }
            const size_t px = (size_t)y * ow + x, plane = (size_t)oh * ow;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float f = (float)v[c] / 255.0f;  // correctly rounded division (Makefile), as NumPy's / 255.0
                if (out_f32) out_f32[((size_t)b * 3 + c) * plane + px] = f;
                if (out_norm) out_norm[((size_t)b * 3 + c) * plane + px] = (f - nm.mean[c]) / nm.stdv[c];
            }
        }
    }
    if (!out_u8) return;
    __syncthreads();
    // the band is contiguous in the output: byte head up to 4-byte alignment, dwords, byte tail
    uint8_t *dst = out_u8 + ((size_t)b * oh + y0) * w3;
    const int n = (y1 - y0) * w3;
    const int head = min(n, (int)((4u - ((uint32_t)(uintptr_t)dst & 3u)) & 3u));
    for (int i = tid; i < head; i += kRsThreads) dst[i] = s_row[i];
    const int nw = (n - head) >> 2;
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    for (int k = tid; k < nw; k += kRsThreads) {
        const uint8_t *s = s_row + head + 4 * k;
        dw[k] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    }
    for (int i = head + 4 * nw + tid; i < n; i += kRsThreads) dst[i] = s_row[i];
}

}  // namespace

int launch_resize_rgb(const uwie_frame_desc *d_desc, int B, int oh, int ow, const uint8_t *d_flips, uint8_t *d_u8, float *d_f32,
                      float *d_norm, const float *mean3, const float *std3, uint32_t *d_status, hipStream_t st)
{
    RsNorm nm{};
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean3 ? mean3[c] : 0.0f;
        nm.stdv[c] = std3 ? std3[c] : 1.0f;
    }
    const int band = ow <= kRsBandWide ? kRsBand : 1;
    const size_t lds = (size_t)ow * 8 + (d_u8 ? (size_t)band * ow * 3 : 0);
    UWIE_LAUNCH(k_resize_rgb, dim3((oh + band - 1) / band, B), dim3(kRsThreads), lds, st, d_desc, oh, ow, band, d_flips, d_u8,
                d_f32, d_norm, nm, d_status);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
