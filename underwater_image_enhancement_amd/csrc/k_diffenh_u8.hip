// vgg_16_UIE.DifferentiableEnhancement.forward (k_diffenh.hip's module) for u8 frames, in the byte domain: the way
// use_trained_model.EnhancementPredictor.process_single_image goes from a decoded frame to a u8 frame (:113-164).
// x = (float)v / 255.0f is strictly increasing in the byte v, so torch.sort of a channel is the sort of its bytes:
//   count   256-bin histogram per (image, channel): k_frame_hist (k_codes.hip), as it is
//   select  k_du8_select: sorted positions stretch_rank(L_low / L_high, n) -> the bin holding each -> p = (float)code / 255.0f
//   apply   k_du8_apply: the stretch takes at most 256 values per channel, so each block tabulates vgg_stretch for the
//           three channels in LDS (3 KB) and then runs vgg_after_stretch (dehaze, gamma, final clamp: devutil.h, the
//           float32 kernels' source) per pixel; bytes out = (uint8)(v * 255.0f), floats out = v.
// No float image exists anywhere: 3 B/px read twice, 3 B/px (or 12) written.  DESIGN.md section 16.
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

// 16-byte accesses at an address aligned only for its element type: the copy through a local lets the compiler emit one
// global_load / store_dwordx4 (gfx950 takes unaligned addresses) without a cast that promises more alignment than there is
template <typename V, typename T>
__device__ __forceinline__ V load16(const T *p)
{
    V v;
    __builtin_memcpy(&v, p, sizeof(V));
    return v;
}
template <typename V, typename T>
__device__ __forceinline__ void store16(T *p, const V &v)
{
    __builtin_memcpy(p, &v, sizeof(V));
}

// One block per image: per channel an inclusive scan of the 256 bins; the bin with excl <= r < incl holds sorted
// position r (r <= n - 1, so exactly one bin does).  os[b][c] = {p_low, p_high}.
__global__ void __launch_bounds__(256) k_du8_select(const uint32_t *__restrict__ hist, int n, const float *__restrict__ params,
                                                    float *__restrict__ os)
{
    __shared__ uint32_t wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t r_lo = (uint32_t)stretch_rank(params[b * 4 + 0], n), r_hi = (uint32_t)stretch_rank(params[b * 4 + 1], n);
    for (int c = 0; c < 3; ++c) {
        const uint32_t h = hist[((size_t)b * 3 + c) * 256 + tid];
        uint32_t incl = wave_incl_scan_u32(h);
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        for (int w = 0; w < wid; ++w) incl += wsum[w];
        const uint32_t excl = incl - h;
        if (r_lo >= excl && r_lo < incl) os[(b * 3 + c) * 2 + 0] = px_norm(tid);
        if (r_hi >= excl && r_hi < incl) os[(b * 3 + c) * 2 + 1] = px_norm(tid);
        __syncthreads();
    }
}

// three pixels' worth of one quad: the twelve bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
__device__ __forceinline__ uint32_t quad_byte(uint32_t w0, uint32_t w1, uint32_t w2, int i)
{
    const uint32_t w = i < 4 ? w0 : (i < 8 ? w1 : w2);
    return (w >> (8 * (i & 3))) & 0xffu;
}

constexpr int kGroupPx = 16;  // 48 bytes: the period of the channel pattern in 16-byte words

// grid (gx, B).  A thread takes whole groups of 16 pixels (three 16-byte loads, three 16-byte stores of bytes, the floats
// as the compiler groups them: four 12-byte stores per quad); the last n % 16 pixels of a frame go byte by byte.  A frame's base (b * 3 * n bytes) may be unaligned.
__global__ void __launch_bounds__(256) k_du8_apply(const uint8_t *__restrict__ in, int n, const float *__restrict__ params, int flags,
                                                   const float *__restrict__ os, uint8_t *__restrict__ out_u8,
                                                   float *__restrict__ out_f32, float *__restrict__ saved)
{
    __shared__ float lut[3][256];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (saved && blockIdx.x == 0 && tid < 6) saved[b * 6 + tid] = os[b * 6 + tid];  // as uwie_diff_enhance_save_f32 leaves it
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lo = os[(b * 3 + c) * 2], rng = (os[(b * 3 + c) * 2 + 1] - lo) + 1e-8f;
        lut[c][tid] = vgg_stretch(px_norm(tid), lo, rng);
    }
    __syncthreads();
    const float omega = params[b * 4 + 2], gamma = params[b * 4 + 3];
    const size_t base = (size_t)b * 3 * n;
    const int ngroups = n / kGroupPx;
    for (int g = blockIdx.x * 256 + tid; g < ngroups; g += gridDim.x * 256) {
        const size_t off = base + (size_t)g * (3 * kGroupPx);
        const uint4 a0 = load16<uint4>(in + off), a1 = load16<uint4>(in + off + 16), a2 = load16<uint4>(in + off + 32);
        uint32_t d[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        // one quad (four pixels, three words) per turn; the words rotate through d[0..2] / o[9..11] so that the loop body
        // exists once (three pow per pixel: unrolled sixteen times it would not fit the instruction cache)
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            float y[12];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = lut[c][quad_byte(d[0], d[1], d[2], 3 * i + c)];
                vgg_after_stretch(v, omega, gamma, flags);
#pragma unroll
                for (int c = 0; c < 3; ++c) y[3 * i + c] = v[c];
            }
            if (out_f32) {
                float *dst = out_f32 + off + (size_t)q * 12;
#pragma unroll
                for (int j = 0; j < 3; ++j) store16(dst + 4 * j, make_float4(y[4 * j], y[4 * j + 1], y[4 * j + 2], y[4 * j + 3]));
            }
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                d[j] = d[j + 3];
                o[j] = o[j + 3];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j)
                o[9 + j] = quant_u8(y[4 * j]) | (quant_u8(y[4 * j + 1]) << 8) | (quant_u8(y[4 * j + 2]) << 16) | (quant_u8(y[4 * j + 3]) << 24);
        }
        if (out_u8) {
            store16(out_u8 + off, make_uint4(o[0], o[1], o[2], o[3]));
            store16(out_u8 + off + 16, make_uint4(o[4], o[5], o[6], o[7]));
            store16(out_u8 + off + 32, make_uint4(o[8], o[9], o[10], o[11]));
        }
    }
    if (blockIdx.x == 0) {  // the frame's tail: fewer than 16 pixels
        const int p = ngroups * kGroupPx + tid;
        if (p < n) {
            const size_t off = base + (size_t)p * 3;
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = lut[c][in[off + c]];
            vgg_after_stretch(v, omega, gamma, flags);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (out_f32) out_f32[off + c] = v[c];
                if (out_u8) out_u8[off + c] = (uint8_t)quant_u8(v[c]);
            }
        }
    }
}

struct Du8Bufs {
    uint32_t *hist;  // [B][3][256]
    float *os;       // [B][3][2] = p_low, p_high
};
Du8Bufs carve_du8(Carver &c, Shape s)
{
    Du8Bufs d;
    d.hist = c.take<uint32_t>((size_t)s.B * 768);
    d.os = c.take<float>((size_t)s.B * 6);
    return d;
}

}  // namespace

size_t diff_u8_ws_bytes(Shape s)
{
    Carver c(nullptr);
    carve_du8(c, s);
    return c.total();
}

int launch_diff_enhance_u8(const uint8_t *d_in, Shape s, const float *d_params, int flags, uint8_t *d_out_u8, float *d_out_f32,
                           float *d_saved, void *ws, hipStream_t st)
{
    Carver c(ws);
    const Du8Bufs d = carve_du8(c, s);
    const int n = (int)s.npx();
    UWIE_HIP_CHECK(hipMemsetAsync(d.hist, 0, sizeof(uint32_t) * (size_t)s.B * 768, st));
    const int rc = launch_frame_hist(d_in, s, d.hist, st);
    if (rc != UWIE_OK) return rc;
    UWIE_LAUNCH(k_du8_select, dim3(s.B), dim3(256), 0, st, (const uint32_t *)d.hist, n, d_params, d.os);
    UWIE_LAUNCH_CHECK();
    // a few groups per thread at large frames: the 768 table entries of a block stay well below its per-pixel work
    const int gx = std::max(1, std::min(cdiv(n / kGroupPx, 256), 1024));
    UWIE_LAUNCH(k_du8_apply, dim3(gx, s.B), dim3(256), 0, st, d_in, n, d_params, flags, (const float *)d.os, d_out_u8, d_out_f32,
                d_saved);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
