// The two enhancement modules of k_diffenh.hip for u8 frames, in the byte domain.  x = (float)v / 255.0f is strictly
// increasing in the byte v, so torch.sort of a channel is the sort of its bytes.  Both routes share their front:
//   count   256-bin histogram per (image, channel): k_frame_hist (k_codes.hip), as it is
//   bins    two_bins: the module's two sorted positions -> the bin holding each -> p = (float)code / 255.0f
// vgg_16_UIE.DifferentiableEnhancement.forward, the way use_trained_model.EnhancementPredictor.process_single_image goes
// from a decoded frame to a u8 frame (:113-164).  DESIGN.md section 16.
//   select  k_du8_select: sorted positions stretch_rank(L_low / L_high, n) -> p_low, p_high per channel
//   apply   k_du8_apply: the stretch takes at most 256 values per channel, so each block tabulates vgg_stretch for the
//           three channels in LDS (3 KB) and then runs vgg_after_stretch (dehaze, gamma, final clamp: devutil.h, the
//           float32 kernels' source) per pixel; bytes out = (uint8)(v * 255.0f), floats out = v.
// deep_learning_parameters.DifferentiableEnhancement.forward (the gated module), where nothing after the stretch mixes
// channels: per image and channel the whole module is a function of the byte alone.  DESIGN.md section 17.
//   table   k_dg8_table, one block per image: sorted positions gated_rank(L_low / L_high, n) (Python's indexing rules; an
//           unindexable one selects position 0 and sets UWIE_STATUS_DIFF_RANK) -> p_low, p_high, then gated_px (devutil.h,
//           k_diff_gated's source) of the 256 byte values of each channel: 3 x 256 float32 and 3 x 256 bytes
//           (uint8)(v * 255.0f); a flagged image gets NaN and 0
//   apply   k_dg8_apply: out[i] = T[b][i % 3][in[i]], the image's tables in LDS; no per-pixel arithmetic
// No float image exists anywhere: 3 B/px read twice, 3 B/px (or 12) written.
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

// A block of 256 threads, thread = bin, h = its count in one channel's histogram: the inclusive scan of the 256 bins; the
// bin with excl <= r < incl holds sorted position r (r <= n - 1, so exactly one bin does).  os[at], os[at + 1] = p_low, p_high
// (`at` stays an index of its own: folded into the pointer, k_du8_select compiles to other instructions than it had).
__device__ __forceinline__ void two_bins(uint32_t h, uint32_t r_lo, uint32_t r_hi, uint32_t *wsum, float *os, int at)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t incl = wave_incl_scan_u32(h);
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    for (int w = 0; w < wid; ++w) incl += wsum[w];
    const uint32_t excl = incl - h;
    if (r_lo >= excl && r_lo < incl) os[at + 0] = px_norm(tid);
    if (r_hi >= excl && r_hi < incl) os[at + 1] = px_norm(tid);
    __syncthreads();
}

// One block per image.  os[b][c] = {p_low, p_high}.
__global__ void __launch_bounds__(256) k_du8_select(const uint32_t *__restrict__ hist, int n, const float *__restrict__ params,
                                                    float *__restrict__ os)
{
    __shared__ uint32_t wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint32_t r_lo = (uint32_t)stretch_rank(params[b * 4 + 0], n), r_hi = (uint32_t)stretch_rank(params[b * 4 + 1], n);
    for (int c = 0; c < 3; ++c) two_bins(hist[((size_t)b * 3 + c) * 256 + tid], r_lo, r_hi, wsum, os, (b * 3 + c) * 2);
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

__global__ void __launch_bounds__(256) k_dg8_table(const uint32_t *__restrict__ hist, int n, const float *__restrict__ params,
                                                   uint32_t *status, float *__restrict__ tabf, uint8_t *__restrict__ tab8,
                                                   float *__restrict__ saved)
{
    __shared__ uint32_t wsum[4];
    __shared__ float os[3][2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *pr = params + b * 4;
    int k0, k1;
    const bool ok0 = gated_rank(pr[0], n, &k0), ok1 = gated_rank(pr[1], n, &k1);
    const bool ok = ok0 && ok1;
    const uint32_t r_lo = ok ? (uint32_t)k0 : 0u, r_hi = ok ? (uint32_t)k1 : 0u;  // as k_sel_init_gated_ranks
    if (!ok && tid == 0 && status) atomicOr(status, (uint32_t)UWIE_STATUS_DIFF_RANK);
    for (int c = 0; c < 3; ++c) two_bins(hist[((size_t)b * 3 + c) * 256 + tid], r_lo, r_hi, wsum, os[c], 0);
    if (saved && tid < 6) saved[b * 6 + tid] = (&os[0][0])[tid];  // as uwie_diff_gated_save_f32 leaves it
    const float u = pr[2], e = 1.0f / pr[3], om = 1.0f - u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lo = os[c][0], rng = (os[c][1] - lo) + 1e-8f;
        const float v = gated_px(px_norm(tid), lo, rng, u, e, om, ok);
        const size_t at = ((size_t)b * 3 + c) * 256 + tid;
        tabf[at] = v;
        tab8[at] = ok ? (uint8_t)quant_u8(v) : (uint8_t)0;
    }
}

// grid (gx, B): a block stays inside image blockIdx.y, whatever the frame size, and holds that image's tables in LDS.
// A thread takes whole groups of 16 pixels (three 16-byte loads, three 16-byte stores of bytes or twelve of floats); the
// last n % 16 pixels of a frame go byte by byte.  A frame's base (b * 3 * n bytes) may be unaligned.
// OUT: 1 bytes, 2 floats, 3 both.  The byte table is 768 consecutive bytes (bank = byte address / 4 mod 32: a wave's 64
// lookups of one channel fall on that channel's 64 dwords, which cover every bank twice).
template <int OUT>
__global__ void __launch_bounds__(256) k_dg8_apply(const uint8_t *__restrict__ in, int n, const uint8_t *__restrict__ tab8,
                                                   const float *__restrict__ tabf, uint8_t *__restrict__ out_u8,
                                                   float *__restrict__ out_f32)
{
    __shared__ uint32_t lut8w[OUT & 1 ? 192 : 1];
    __shared__ float lutf[OUT & 2 ? 768 : 1];
    const uint8_t *lut8 = reinterpret_cast<const uint8_t *>(lut8w);
    const int b = blockIdx.y, tid = threadIdx.x;
    if constexpr ((OUT & 1) != 0) {
        if (tid < 192) lut8w[tid] = reinterpret_cast<const uint32_t *>(tab8 + (size_t)b * 768)[tid];  // 768-byte rows of a 256-byte aligned buffer
    }
    if constexpr ((OUT & 2) != 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) lutf[c * 256 + tid] = tabf[(size_t)b * 768 + c * 256 + tid];
    }
    __syncthreads();
    const size_t base = (size_t)b * 3 * n;
    const int ngroups = n / kGroupPx;
    for (int g = blockIdx.x * 256 + tid; g < ngroups; g += gridDim.x * 256) {
        const size_t off = base + (size_t)g * (3 * kGroupPx);
        const uint4 a0 = load16<uint4>(in + off), a1 = load16<uint4>(in + off + 16), a2 = load16<uint4>(in + off + 32);
        const uint32_t d[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        if constexpr ((OUT & 1) != 0) {
            uint32_t o[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                uint32_t w = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = (4 * j + i) % 3;
                    w |= (uint32_t)lut8[c * 256 + ((d[j] >> (8 * i)) & 0xffu)] << (8 * i);
                }
                o[j] = w;
            }
            store16(out_u8 + off, make_uint4(o[0], o[1], o[2], o[3]));
            store16(out_u8 + off + 16, make_uint4(o[4], o[5], o[6], o[7]));
            store16(out_u8 + off + 32, make_uint4(o[8], o[9], o[10], o[11]));
        }
        if constexpr ((OUT & 2) != 0) {
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float y[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = (4 * j + i) % 3;
                    y[i] = lutf[c * 256 + ((d[j] >> (8 * i)) & 0xffu)];
                }
                store16(out_f32 + off + 4 * j, make_float4(y[0], y[1], y[2], y[3]));
            }
        }
    }
    if (blockIdx.x == 0) {  // the frame's tail: fewer than 16 pixels
        const int p = ngroups * kGroupPx + tid;
        if (p < n) {
            const size_t off = base + (size_t)p * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t v = in[off + c];
                if constexpr ((OUT & 1) != 0) out_u8[off + c] = lut8[c * 256 + v];
                if constexpr ((OUT & 2) != 0) out_f32[off + c] = lutf[c * 256 + v];
            }
        }
    }
}

// the workspace of either route: the histograms, then what the route's first kernel leaves for its apply kernel
struct U8Bufs {
    uint32_t *hist;  // [B][3][256]
    float *os;       // enhance: [B][3][2] = p_low, p_high
    float *tabf;     // gated: [B][3][256]
    uint8_t *tab8;   // gated: [B][3][256]
};
U8Bufs carve_u8(Carver &c, int B, bool gated)
{
    U8Bufs d{};
    d.hist = c.take<uint32_t>((size_t)B * 768);
    if (!gated) {
        d.os = c.take<float>((size_t)B * 6);
    } else {
        d.tabf = c.take<float>((size_t)B * 768);
        d.tab8 = c.take<uint8_t>((size_t)B * 768);
    }
    return d;
}
size_t u8_ws_bytes(int B, bool gated)
{
    Carver c(nullptr);
    carve_u8(c, B, gated);
    return c.total();
}

// The front of both routes: the carved workspace with its histograms counted, and the apply kernels' grid (up to 1024
// blocks per image: a few groups per thread at large frames, so a block's table stays small beside its pixels).
int u8_front(const uint8_t *d_in, Shape s, bool gated, void *ws, hipStream_t st, U8Bufs *d, dim3 *grid)
{
    Carver c(ws);
    *d = carve_u8(c, s.B, gated);
    UWIE_HIP_CHECK(hipMemsetAsync(d->hist, 0, sizeof(uint32_t) * (size_t)s.B * 768, st));
    *grid = dim3(std::max(1, std::min(cdiv((int)s.npx() / kGroupPx, 256), 1024)), s.B);
    return launch_frame_hist(d_in, s, d->hist, st);
}

}  // namespace

size_t diff_u8_ws_bytes(Shape s) { return u8_ws_bytes(s.B, false); }
size_t diff_gated_u8_ws_bytes(int B) { return u8_ws_bytes(B, true); }

int launch_diff_enhance_u8(const uint8_t *d_in, Shape s, const float *d_params, int flags, uint8_t *d_out_u8, float *d_out_f32,
                           float *d_saved, void *ws, hipStream_t st)
{
    U8Bufs d;
    dim3 grid;
    const int rc = u8_front(d_in, s, false, ws, st, &d, &grid);
    if (rc != UWIE_OK) return rc;
    const int n = (int)s.npx();
    UWIE_LAUNCH(k_du8_select, dim3(s.B), dim3(256), 0, st, (const uint32_t *)d.hist, n, d_params, d.os);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_du8_apply, grid, dim3(256), 0, st, d_in, n, d_params, flags, (const float *)d.os, d_out_u8, d_out_f32, d_saved);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

int launch_diff_gated_u8(const uint8_t *d_in, Shape s, const float *d_params, uint32_t *d_status, uint8_t *d_out_u8,
                         float *d_out_f32, float *d_saved, void *ws, hipStream_t st)
{
    U8Bufs d;
    dim3 grid;
    const int rc = u8_front(d_in, s, true, ws, st, &d, &grid);
    if (rc != UWIE_OK) return rc;
    const int n = (int)s.npx();
    UWIE_LAUNCH(k_dg8_table, dim3(s.B), dim3(256), 0, st, (const uint32_t *)d.hist, n, d_params, d_status, d.tabf, d.tab8, d_saved);
    UWIE_LAUNCH_CHECK();
    const uint8_t *t8 = d.tab8;
    const float *tf = d.tabf;
    if (d_out_u8 && d_out_f32) UWIE_LAUNCH(k_dg8_apply<3>, grid, dim3(256), 0, st, d_in, n, t8, tf, d_out_u8, d_out_f32);
    else if (d_out_u8) UWIE_LAUNCH(k_dg8_apply<1>, grid, dim3(256), 0, st, d_in, n, t8, tf, d_out_u8, d_out_f32);
    else UWIE_LAUNCH(k_dg8_apply<2>, grid, dim3(256), 0, st, d_in, n, t8, tf, d_out_u8, d_out_f32);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
