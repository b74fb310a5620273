// DifferentiableEnhancement.forward (vgg_16_UIE.py:32-128, the `enhance_image` surface of use_trained_model.py:83-111)
// after the order statistics: colour stretch between two sorted positions per channel -> simplified dark-channel
// dehazing with A = 0.6 -> gamma -> clamp.  float32 throughout, one operation per PyTorch operation (torch evaluates
// `tensor op python_scalar` in float32 with the scalar converted to float32).
//   stretch  (channel - p_low) / (p_high - p_low + 1e-8), clamp 0..1                     vgg_16_UIE.py:88-91
//   dehaze   dark = min_c; t = clamp(1 - omega*dark, 0.1, 1); clamp((img - 0.6)/t + 0.6)  vgg_16_UIE.py:103-117
//   gamma    pow(img + 1e-8, gamma)                                                       vgg_16_UIE.py:127
// pow is evaluated in float64 and rounded once; torch's float32 pow (Sleef, 1 ulp) may differ by one ulp: stated
// tolerance of the gamma stage.
//
// Backward (the gradient torch autograd gives the module on the CPU): k_diff_enhance_bwd recomputes
// the forward per pixel from x and the saved order statistics, writes grad_img (optional) and per-block float64 partial
// sums of grad omega, grad gamma, grad p_lo / p_hi plus the counts of x < p and x == p that locate the element torch's
// stable sort routes each order statistic's gradient to; k_diff_enhance_bwd_finish reduces the partials in a fixed order
// (no atomics: bit-identical runs) and scatters the two scalar terms per plane.
//
// Gated gamma (deep_learning_parameters.py:24-90, the module EndToEndTrainer trains through): the same
// stretch with Python's indexing rules for the sorted positions (devutil.h gated_rank), then e = 1.0 / gamma (float32,
// correctly rounded), z = pow(s + 1e-8, e), clamp(use_gamma * z + (1 - use_gamma) * s, 0, 1).  k_diff_gated /
// k_diff_gated_bwd are its forward and backward sweep; the finish kernel is shared (GATED = true).  An image without a
// valid sorted position gets NaN in its output and gradients (the selection set UWIE_STATUS_DIFF_RANK for it).
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

// The per-pixel forwards, shared by the inference kernels and the loss sweep (k_refloss_*): the clamp masks of the loss
// backward recompute these values, so both must see the same bits.
// vgg: v = clamp(stretch -> [dehaze] -> [gamma]) of one pixel's three channels (flags: UWIE_DIFF_OMEGA | UWIE_DIFF_GAMMA);
// the two halves are in devutil.h, where the byte-domain kernels (k_diff_u8.hip) take them from too
__device__ __forceinline__ void vgg_px(const float (&x)[3], const float (&lo)[3], const float (&rng)[3], float omega, float gamma,
                                       int flags, float (&v)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = vgg_stretch(x[c], lo[c], rng[c]);
    vgg_after_stretch(v, omega, gamma, flags);
}

// gated: gated_px (devutil.h), one channel value; the byte-domain table (k_diff_u8.hip) compiles the same source

// planar: img/out [B][3][n];  interleaved: [B][n][3].  os: [B*3][kSelOsStride] floats, entries 0/1 = p_low, p_high.
__global__ void __launch_bounds__(256) k_diff_enhance(const float *__restrict__ img, int planar, int n,
                                                      const float *__restrict__ params, int flags,
                                                      const float *__restrict__ os, float *__restrict__ out,
                                                      float *__restrict__ saved)
{
    const int b = blockIdx.y;
    if (saved && blockIdx.x == 0 && threadIdx.x < 6) {  // {p_lo, p_hi} of the three planes, for the backward
        const int c = threadIdx.x >> 1, q = threadIdx.x & 1;
        saved[(b * 3 + c) * 2 + q] = os[(size_t)(b * 3 + c) * kSelOsStride + q];
    }
    const float *pr = params + b * 4;
    float lo[3], rng[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *o = os + (size_t)(b * 3 + c) * kSelOsStride;
        lo[c] = o[0];
        rng[c] = (o[1] - o[0]) + 1e-8f;
    }
    const float omega = pr[2], gamma = pr[3];
    const size_t base = (size_t)b * 3 * n;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        float x[3], y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = planar ? img[base + (size_t)c * n + p] : img[base + (size_t)p * 3 + c];
        vgg_px(x, lo, rng, omega, gamma, flags, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (planar) out[base + (size_t)c * n + p] = y[c];
            else out[base + (size_t)p * 3 + c] = y[c];
        }
    }
}

// the gated module's forward: params[b] = {L_low, L_high, use_gamma, gamma}; saved as in k_diff_enhance
__global__ void __launch_bounds__(256) k_diff_gated(const float *__restrict__ img, int planar, int n,
                                                    const float *__restrict__ params, const float *__restrict__ os,
                                                    float *__restrict__ out, float *__restrict__ saved)
{
    const int b = blockIdx.y;
    if (saved && blockIdx.x == 0 && threadIdx.x < 6) {
        const int c = threadIdx.x >> 1, q = threadIdx.x & 1;
        saved[(b * 3 + c) * 2 + q] = os[(size_t)(b * 3 + c) * kSelOsStride + q];
    }
    const float *pr = params + b * 4;
    float lo[3], rng[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *o = os + (size_t)(b * 3 + c) * kSelOsStride;
        lo[c] = o[0];
        rng[c] = (o[1] - o[0]) + 1e-8f;
    }
    int k0, k1;
    const bool ok0 = gated_rank(pr[0], n, &k0), ok1 = gated_rank(pr[1], n, &k1);
    const bool ok = ok0 && ok1;
    const float u = pr[2], e = 1.0f / pr[3], om = 1.0f - u;
    const size_t base = (size_t)b * 3 * n;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t i = planar ? base + (size_t)c * n + p : base + (size_t)p * 3 + c;
            out[i] = gated_px(img[i], lo[c], rng[c], u, e, om, ok);
        }
    }
}

// dL/d(out) of w1 * mean|out - ref| + w2 * mean((out - ref)^2) in torch's autograd order, given
// g1 = dL/dl1, g2 = dL/dl2 (device scalars, read by every thread: no host sync):
//   MeanBackward0 -> AbsBackward0: (g1 / N) * sgn(d), sgn(0) = sgn(NaN) = 0;  MseLossBackward0: ((2 / N) * d) * g2;  their sum.
// nf = (float)N and norm = (float)(2.0 / N) as torch converts them; an upstream gradient on out (gout) is added last.
struct LossGrad {
    const float *gl;  // {g1, g2}
    float nf, norm;
};
// the per-thread constants: q1 = g1 / N, norm, g2
struct LossK {
    float q1, norm, g2;
};
__device__ __forceinline__ LossK loss_k(const LossGrad &lg) { return LossK{lg.gl[0] / lg.nf, lg.norm, lg.gl[1]}; }

__device__ __forceinline__ float refloss_grad(const LossK &k, float o, float r, const float *__restrict__ gout, size_t i)
{
    const float d = o - r;
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    const float g = k.q1 * sg + (k.norm * d) * k.g2;
    return gout ? gout[i] + g : g;
}

// Per-block partials: kPartD float64 sums and kPartU counts per (image, block).
//   sums:   0 grad omega (gated: grad use_gamma), 1 grad gamma (gated: grad e, e = 1 / gamma), 2 + c: sum of grad_x over plane c (the stretch's dL/dx before the scatter),
//           5 + c: dL/dr of plane c (r = p_hi - p_lo + 1e-8)
//   counts: c * 4 + {0: x < p_lo, 1: x == p_lo, 2: x < p_hi, 3: x == p_hi}
constexpr int kPartD = 8, kPartU = 12;

// The block's totals of a backward sweep: wave sums, then the four waves in order (fixed order: the same bits every run).
__device__ __forceinline__ void store_partials(const double (&v)[kPartD], const uint32_t (&k)[kPartU], double *__restrict__ part,
                                               uint32_t *__restrict__ cnt)
{
    __shared__ double sd[4][kPartD];
    __shared__ uint32_t su[4][kPartU];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kPartD; ++i) {
        double a = v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) sd[wid][i] = a;
    }
#pragma unroll
    for (int i = 0; i < kPartU; ++i) {
        const uint32_t a = wave_sum_u32(k[i]);
        if (lane == 0) su[wid][i] = a;
    }
    __syncthreads();
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x < kPartD) {
        const int i = threadIdx.x;
        part[slot * kPartD + i] = ((sd[0][i] + sd[1][i]) + sd[2][i]) + sd[3][i];
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + kPartU) {
        const int i = threadIdx.x - 64;
        cnt[slot * kPartU + i] = su[0][i] + su[1][i] + su[2][i] + su[3][i];
    }
}

// One contiguous chunk of `chunk` pixels of one image per block, so that the equal counts of the blocks, in block order,
// are the equal counts of the plane in linear index order (what the finish kernel scans for the stable-sort position).
// Every pointwise term follows torch's backward formulas in operation order (clamp: pass where lo <= v <= hi; a / b:
// grad / b and -grad * ((a / b) / b); min(dim): the first minimal channel; pow: grad * (g * y^(g - 1)) and
// grad * (z * log(y))).  y^(g - 1) is z / y in float64, rounded once (z: the forward's pow, <= 1 ulp).
// LOSS (k_refloss_bwd): g = (gout ? gout[i] : 0) + dL/d(out) of the reference loss, from out recomputed here and ref[i]
// (refloss_grad); otherwise g = gout[i].
template <int FLAGS, bool LOSS>
__device__ __forceinline__ void diff_enhance_bwd_body(const float *__restrict__ img, int planar, int n, int chunk,
                                                      const float *__restrict__ params, const float *__restrict__ saved,
                                                      const float *__restrict__ gout, const float *__restrict__ ref,
                                                      const LossGrad lg, float *__restrict__ gimg, double *__restrict__ part,
                                                      uint32_t *__restrict__ cnt)
{
    const int b = blockIdx.y;
    float lo[3], hi[3], rng[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = saved[(b * 3 + c) * 2];
        hi[c] = saved[(b * 3 + c) * 2 + 1];
        rng[c] = (hi[c] - lo[c]) + 1e-8f;
    }
    const float omega = params[b * 4 + 2], gamma = params[b * 4 + 3];
    const LossK lk = LOSS ? loss_k(lg) : LossK{0.0f, 0.0f, 0.0f};
    double s_om = 0.0, s_ga = 0.0, s_x[3] = {0.0, 0.0, 0.0}, s_r[3] = {0.0, 0.0, 0.0};
    uint32_t k[kPartU];
#pragma unroll
    for (int i = 0; i < kPartU; ++i) k[i] = 0;
    const size_t base = (size_t)b * 3 * n;
    const int p0 = blockIdx.x * chunk;
    const int p1 = min(p0 + chunk, n);
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
        float x[3], g[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t i = planar ? base + (size_t)c * n + p : base + (size_t)p * 3 + c;
            x[c] = img[i];
            if (LOSS) g[c] = ref[i];  // replaced by the loss gradient once out is known
            else g[c] = gout[i];
        }
        float s0[3], s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            k[c * 4 + 0] += x[c] < lo[c];
            k[c * 4 + 1] += x[c] == lo[c];
            k[c * 4 + 2] += x[c] < hi[c];
            k[c * 4 + 3] += x[c] == hi[c];
            s0[c] = (x[c] - lo[c]) / rng[c];
            s[c] = clamp01(s0[c]);
        }
        // forward: dehaze, gamma
        float y[3], d1[3], d2[3], dark = 0.0f, t0 = 1.0f, t = 1.0f;
        int am = 0;
        if (FLAGS & 1) {
            dark = s[0];
            if (s[1] < dark) { dark = s[1]; am = 1; }
            if (s[2] < dark) { dark = s[2]; am = 2; }
            t0 = 1.0f - omega * dark;
            t = fminf(fmaxf(t0, 0.1f), 1.0f);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                d1[c] = (s[c] - 0.6f) / t;
                d2[c] = d1[c] + 0.6f;
                y[c] = clamp01(d2[c]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) y[c] = s[c];
        }
        // backward: final clamp, gamma
        float gy[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (FLAGS & 2) {
                const float ye = y[c] + 1e-8f;
                const float z = pow_f32_fast(ye, gamma);
                if (LOSS) g[c] = refloss_grad(lk, clamp01(z), g[c], gout, planar ? base + (size_t)c * n + p : base + (size_t)p * 3 + c);
                const float gz = (z >= 0.0f && z <= 1.0f) ? g[c] : 0.0f;
                const float dz = gamma * (float)((double)z / (double)ye);
                gy[c] = gamma == 0.0f ? 0.0f : gz * dz;
                s_ga += (double)(gz * (z * logf(ye)));
            } else {
                if (LOSS) g[c] = refloss_grad(lk, clamp01(y[c]), g[c], gout, planar ? base + (size_t)c * n + p : base + (size_t)p * 3 + c);
                gy[c] = (y[c] >= 0.0f && y[c] <= 1.0f) ? g[c] : 0.0f;
            }
        }
        // dehaze: the clamp, (s - 0.6) / t, t = clamp(1 - omega * dark), dark = min_c s
        float gs[3];
        if (FLAGS & 1) {
            float gt = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float gd = (d2[c] >= 0.0f && d2[c] <= 1.0f) ? gy[c] : 0.0f;
                gs[c] = gd / t;
                const float term = -gd * (d1[c] / t);
                gt = c == 0 ? term : gt + term;
            }
            const float gm = -((t0 >= 0.1f && t0 <= 1.0f) ? gt : 0.0f);
            s_om += (double)(gm * dark);
            const float gdark = gm * omega;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c == am) gs[c] = gs[c] + gdark;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) gs[c] = gy[c];
        }
        // stretch: the clamp, (x - p_lo) / r
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g0 = (s0[c] >= 0.0f && s0[c] <= 1.0f) ? gs[c] : 0.0f;
            const float gx = g0 / rng[c];
            s_x[c] += (double)gx;
            s_r[c] += (double)(-g0 * (s0[c] / rng[c]));
            if (gimg) gimg[planar ? base + (size_t)c * n + p : base + (size_t)p * 3 + c] = gx;
        }
    }
    const double v[kPartD] = {s_om, s_ga, s_x[0], s_x[1], s_x[2], s_r[0], s_r[1], s_r[2]};
    store_partials(v, k, part, cnt);
}

template <int FLAGS>
__global__ void __launch_bounds__(256) k_diff_enhance_bwd(const float *__restrict__ img, int planar, int n, int chunk,
                                                          const float *__restrict__ params, const float *__restrict__ saved,
                                                          const float *__restrict__ gout, float *__restrict__ gimg,
                                                          double *__restrict__ part, uint32_t *__restrict__ cnt)
{
    diff_enhance_bwd_body<FLAGS, false>(img, planar, n, chunk, params, saved, gout, nullptr, LossGrad{}, gimg, part, cnt);
}

// The gated module's backward sweep (same chunks, partials and counts as k_diff_enhance_bwd).  torch's graph, with v the
// input of the final clamp and g its gradient after the clamp's mask: d use_gamma = g * z - g * s (MulBackward0 and
// RsubBackward1), dz = g * use_gamma, d e = dz * (z * log(s + 1e-8)), ds = g * (1 - use_gamma) + dz * (e * (s + 1e-8)^(e - 1))
// with (s + 1e-8)^(e - 1) = z / (s + 1e-8) in float64, rounded once.  d gamma = -d e * (r * r) (r = 1 / gamma) is formed
// in the finish kernel.
// LOSS: g as in diff_enhance_bwd_body, with out = the forward's value (gated_px).
template <bool LOSS>
__device__ __forceinline__ void diff_gated_bwd_body(const float *__restrict__ img, int planar, int n, int chunk,
                                                    const float *__restrict__ params, const float *__restrict__ saved,
                                                    const float *__restrict__ gout, const float *__restrict__ ref,
                                                    const LossGrad lg, float *__restrict__ gimg, double *__restrict__ part,
                                                    uint32_t *__restrict__ cnt)
{
    const int b = blockIdx.y;
    float lo[3], hi[3], rng[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = saved[(b * 3 + c) * 2];
        hi[c] = saved[(b * 3 + c) * 2 + 1];
        rng[c] = (hi[c] - lo[c]) + 1e-8f;
    }
    int k0, k1;
    const bool ok0 = gated_rank(params[b * 4 + 0], n, &k0), ok1 = gated_rank(params[b * 4 + 1], n, &k1);
    const bool ok = ok0 && ok1;
    const float u = params[b * 4 + 2], e = 1.0f / params[b * 4 + 3], om = 1.0f - u;
    const LossK lk = LOSS ? loss_k(lg) : LossK{0.0f, 0.0f, 0.0f};
    double s_u = 0.0, s_e = 0.0, s_x[3] = {0.0, 0.0, 0.0}, s_r[3] = {0.0, 0.0, 0.0};
    uint32_t k[kPartU];
#pragma unroll
    for (int i = 0; i < kPartU; ++i) k[i] = 0;
    const size_t base = (size_t)b * 3 * n;
    const int p0 = blockIdx.x * chunk;
    const int p1 = min(p0 + chunk, n);
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t i = planar ? base + (size_t)c * n + p : base + (size_t)p * 3 + c;
            const float x = img[i];
            float g = LOSS ? 0.0f : gout[i];
            k[c * 4 + 0] += x < lo[c];
            k[c * 4 + 1] += x == lo[c];
            k[c * 4 + 2] += x < hi[c];
            k[c * 4 + 3] += x == hi[c];
            const float s0 = (x - lo[c]) / rng[c];
            const float sv = clamp01(s0);
            const float ye = sv + 1e-8f;
            const float z = pow_f32_fast(ye, e);
            const float v = u * z + om * sv;
            // out = gated_px's value; an image without a valid position (!ok) gets NaN gradients below whatever g is
            if (LOSS) g = refloss_grad(lk, clamp01(v), ref[i], gout, i);
            const float gv = (v >= 0.0f && v <= 1.0f) ? g : 0.0f;
            s_u += (double)(gv * z) - (double)(gv * sv);
            const float gz = gv * u;
            s_e += (double)(gz * (z * logf(ye)));
            const float dz = e * (float)((double)z / (double)ye);
            const float gs = gv * om + (e == 0.0f ? 0.0f : gz * dz);
            // stretch: the clamp, (x - p_lo) / r
            const float g0 = (s0 >= 0.0f && s0 <= 1.0f) ? gs : 0.0f;
            const float gx = g0 / rng[c];
            s_x[c] += (double)gx;
            s_r[c] += (double)(-g0 * (s0 / rng[c]));
            if (gimg) gimg[i] = ok ? gx : __builtin_nanf("");
        }
    }
    const double v[kPartD] = {s_u, s_e, s_x[0], s_x[1], s_x[2], s_r[0], s_r[1], s_r[2]};
    store_partials(v, k, part, cnt);
}

__global__ void __launch_bounds__(256) k_diff_gated_bwd(const float *__restrict__ img, int planar, int n, int chunk,
                                                        const float *__restrict__ params, const float *__restrict__ saved,
                                                        const float *__restrict__ gout, float *__restrict__ gimg,
                                                        double *__restrict__ part, uint32_t *__restrict__ cnt)
{
    diff_gated_bwd_body<false>(img, planar, n, chunk, params, saved, gout, nullptr, LossGrad{}, gimg, part, cnt);
}

// The backward sweeps with the reference loss's gradient in place of grad_out (k_refloss_*'s forward values)
template <int FLAGS>
__global__ void __launch_bounds__(256) k_diff_enhance_loss_bwd(const float *__restrict__ img, int planar, int n, int chunk,
                                                               const float *__restrict__ params, const float *__restrict__ saved,
                                                               const float *__restrict__ gout, const float *__restrict__ ref,
                                                               const LossGrad lg, float *__restrict__ gimg,
                                                               double *__restrict__ part, uint32_t *__restrict__ cnt)
{
    diff_enhance_bwd_body<FLAGS, true>(img, planar, n, chunk, params, saved, gout, ref, lg, gimg, part, cnt);
}

__global__ void __launch_bounds__(256) k_diff_gated_loss_bwd(const float *__restrict__ img, int planar, int n, int chunk,
                                                             const float *__restrict__ params, const float *__restrict__ saved,
                                                             const float *__restrict__ gout, const float *__restrict__ ref,
                                                             const LossGrad lg, float *__restrict__ gimg,
                                                             double *__restrict__ part, uint32_t *__restrict__ cnt)
{
    diff_gated_bwd_body<true>(img, planar, n, chunk, params, saved, gout, ref, lg, gimg, part, cnt);
}

// One block per (plane c, image b): the plane's partials in block order, then the element each order statistic's gradient
// goes to.  torch.sort is stable on the CPU, so sorted position k of value p is the (k - #{x < p})-th element equal to p
// in linear index order: the block's equal counts find the chunk, one pass over that chunk finds the element.
// grad_params[b] = {0, 0, grad omega, grad gamma} (plane 0's block).  GATED: the gated module's sorted positions and
// grad_params[b] = {0, 0, grad use_gamma, -grad e * (r * r)} (torch's ReciprocalBackward0, r = 1 / gamma); an image without a
// valid position gets NaN parameter gradients and no scatter (its grad_img is NaN already).
template <bool GATED>
__global__ void __launch_bounds__(256) k_diff_enhance_bwd_finish(const float *__restrict__ img, int planar, int n, int chunk,
                                                                 int gx, const float *__restrict__ params,
                                                                 const float *__restrict__ saved,
                                                                 const double *__restrict__ part,
                                                                 const uint32_t *__restrict__ cnt, float *__restrict__ gimg,
                                                                 float *__restrict__ gparams)
{
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    __shared__ double rd[4][256];
    __shared__ uint32_t ru[4][256];
    double v[4] = {0.0, 0.0, 0.0, 0.0};  // grad omega, grad gamma, sum grad_x, dL/dr
    uint32_t u[4] = {0, 0, 0, 0};        // x < p_lo, x == p_lo, x < p_hi, x == p_hi
    for (int i = tid; i < gx; i += 256) {
        const double *pp = part + ((size_t)b * gx + i) * kPartD;
        const uint32_t *cc = cnt + ((size_t)b * gx + i) * kPartU + c * 4;
        v[0] += pp[0];
        v[1] += pp[1];
        v[2] += pp[2 + c];
        v[3] += pp[5 + c];
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] += cc[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        rd[q][tid] = v[q];
        ru[q][tid] = u[q];
    }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rd[q][tid] += rd[q][tid + w];
                ru[q][tid] += ru[q][tid + w];
            }
        }
        __syncthreads();
    }
    long long k_lo, k_hi;
    bool ok = true;
    if (GATED) {
        int k0, k1;
        const bool ok0 = gated_rank(params[b * 4 + 0], n, &k0), ok1 = gated_rank(params[b * 4 + 1], n, &k1);
        ok = ok0 && ok1;
        k_lo = k0;
        k_hi = k1;
    } else {
        k_lo = stretch_rank(params[b * 4 + 0], n);
        k_hi = stretch_rank(params[b * 4 + 1], n);
    }
    if (c == 0 && tid == 0) {
        gparams[b * 4 + 0] = 0.0f;
        gparams[b * 4 + 1] = 0.0f;
        if (GATED) {
            const float r = 1.0f / params[b * 4 + 3];
            gparams[b * 4 + 2] = ok ? (float)rd[0][0] : __builtin_nanf("");
            gparams[b * 4 + 3] = ok ? (float)rd[1][0] * -(r * r) : __builtin_nanf("");
        } else {
            gparams[b * 4 + 2] = (float)rd[0][0];
            gparams[b * 4 + 3] = (float)rd[1][0];
        }
    }
    if (!gimg || !ok) return;
    // grad p_lo = -sum grad_x - dL/dr, grad p_hi = dL/dr (r = p_hi - p_lo + 1e-8)
    const float g_lo = (float)(-rd[2][0] - rd[3][0]), g_hi = (float)rd[3][0];
    const size_t base = (size_t)b * 3 * n;
    __shared__ int s_blk, s_pos;
    __shared__ long long s_j;
    __shared__ uint32_t s_wave[4];
    int pos[2] = {-1, -1};
    for (int q = 0; q < 2; ++q) {
        if (q == 1 && k_hi == k_lo) {
            pos[1] = pos[0];
            break;
        }
        const float pv = saved[(b * 3 + c) * 2 + q];
        const long long j = (q ? k_hi : k_lo) - (long long)ru[2 * q][0];  // rank among the elements equal to pv
        if (tid == 0) {
            s_blk = -1;
            s_pos = -1;
            long long acc = 0;
            for (int i = 0; i < gx && j >= 0; ++i) {
                const uint32_t e = cnt[((size_t)b * gx + i) * kPartU + c * 4 + 2 * q + 1];
                if (j < acc + e) {
                    s_blk = i;
                    s_j = j - acc;
                    break;
                }
                acc += e;
            }
        }
        __syncthreads();
        const int blk = s_blk;
        if (blk >= 0) {
            const int p0 = blk * chunk, p1 = min(p0 + chunk, n);
            long long left = s_j;  // equal elements still to pass
            for (int t0 = p0; t0 < p1; t0 += 256) {
                const int p = t0 + tid;
                const bool eq = p < p1 && img[planar ? base + (size_t)c * n + p : base + (size_t)p * 3 + c] == pv;
                const uint64_t m = __ballot(eq);
                const uint32_t before = __popcll(m & ((1ull << (tid & 63)) - 1ull));
                if ((tid & 63) == 0) s_wave[tid >> 6] = (uint32_t)__popcll(m);
                __syncthreads();
                uint32_t wbefore = 0, total = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    wbefore += w < (tid >> 6) ? s_wave[w] : 0;
                    total += s_wave[w];
                }
                if (eq && (long long)(wbefore + before) == left) s_pos = p;
                __syncthreads();
                if (s_pos >= 0 || left < (long long)total) break;  // uniform: every thread reads the same values
                left -= total;
            }
        }
        pos[q] = s_pos;
        __syncthreads();
    }
    if (tid == 0) {
        if (k_lo == k_hi) {
            if (pos[0] >= 0) {
                const size_t i = planar ? base + (size_t)c * n + pos[0] : base + (size_t)pos[0] * 3 + c;
                gimg[i] = gimg[i] + (g_lo + g_hi);
            }
        } else {
            for (int q = 0; q < 2; ++q) {
                if (pos[q] < 0) continue;
                const size_t i = planar ? base + (size_t)c * n + pos[q] : base + (size_t)pos[q] * 3 + c;
                gimg[i] = gimg[i] + (q ? g_hi : g_lo);
            }
        }
    }
}

// ------------------------------------------------------------------ ReferenceLoss
// l1 = mean|o - r|, l2 = mean((o - r)^2) of the module's output o and a reference r, fused into the forward (k_refloss_identity / _vgg / _gated): o is formed in
// registers (vgg_px / gated_px, the inference kernels' bits) and written only when asked.  The float32 terms |d| and d * d
// are summed in float64: per thread, then store_partials' fixed wave / block order, then k_refloss_finish.
enum { kMapIdentity = 0, kMapVgg = 1, kMapGated = 2 };  // UWIE_LOSS_*
constexpr int kLossPart = 2;                              // per-block float64 partials: sum |d|, sum d * d

template <int MAP, int FLAGS>
__device__ __forceinline__ void refloss_fwd_body(const float *__restrict__ img, int planar, int n, int chunk,
                                                 const float *__restrict__ params, const float *__restrict__ os,
                                                 const float *__restrict__ ref, float *__restrict__ out, float *__restrict__ saved,
                                                 double *__restrict__ part)
{
    const int b = blockIdx.y;
    float lo[3] = {0.0f, 0.0f, 0.0f}, rng[3] = {1.0f, 1.0f, 1.0f};
    float a0 = 0.0f, a1 = 0.0f, om = 0.0f;  // vgg: omega, gamma; gated: use_gamma, 1 / gamma, 1 - use_gamma
    bool ok = true;
    if (MAP != kMapIdentity) {
        if (saved && blockIdx.x == 0 && threadIdx.x < 6) {  // as the _save_f32 forwards leave it
            const int c = threadIdx.x >> 1, q = threadIdx.x & 1;
            saved[(b * 3 + c) * 2 + q] = os[(size_t)(b * 3 + c) * kSelOsStride + q];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *o = os + (size_t)(b * 3 + c) * kSelOsStride;
            lo[c] = o[0];
            rng[c] = (o[1] - o[0]) + 1e-8f;
        }
        const float *pr = params + b * 4;
        if (MAP == kMapVgg) {
            a0 = pr[2];
            a1 = pr[3];
        } else {
            int k0, k1;
            const bool ok0 = gated_rank(pr[0], n, &k0), ok1 = gated_rank(pr[1], n, &k1);
            ok = ok0 && ok1;
            a0 = pr[2];
            a1 = 1.0f / pr[3];
            om = 1.0f - a0;
        }
    }
    double s1 = 0.0, s2 = 0.0;
    const size_t base = (size_t)b * 3 * n;
    const int p0 = blockIdx.x * chunk;
    const int p1 = min(p0 + chunk, n);
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
        size_t i[3];
        float x[3], o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            i[c] = planar ? base + (size_t)c * n + p : base + (size_t)p * 3 + c;
            x[c] = img[i[c]];
        }
        if (MAP == kMapVgg) {
            vgg_px(x, lo, rng, a0, a1, FLAGS, o);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = MAP == kMapGated ? gated_px(x[c], lo[c], rng[c], a0, a1, om, ok) : x[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = o[c] - ref[i[c]];
            s1 += (double)fabsf(d);
            s2 += (double)(d * d);
            if (MAP != kMapIdentity && out) out[i[c]] = o[c];
        }
    }
    // the block's totals: wave sums, then the four waves in order (store_partials' order)
    __shared__ double sd[4][kLossPart];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
        sd[wid][0] = s1;
        sd[wid][1] = s2;
    }
    __syncthreads();
    if (threadIdx.x < kLossPart) {
        const int q = threadIdx.x;
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kLossPart + q] = ((sd[0][q] + sd[1][q]) + sd[2][q]) + sd[3][q];
    }
}

#define UWIE_REFLOSS_FWD_ARGS                                                                                            \
    const float *__restrict__ img, int planar, int n, int chunk, const float *__restrict__ params, const float *__restrict__ os, \
        const float *__restrict__ ref, float *__restrict__ out, float *__restrict__ saved, double *__restrict__ part
// the three maps: identity (o = img), the vgg module (flags), the gated module
__global__ void __launch_bounds__(256) k_refloss_identity(UWIE_REFLOSS_FWD_ARGS)
{
    refloss_fwd_body<kMapIdentity, 0>(img, planar, n, chunk, params, os, ref, out, saved, part);
}
template <int FLAGS>
__global__ void __launch_bounds__(256) k_refloss_vgg(UWIE_REFLOSS_FWD_ARGS)
{
    refloss_fwd_body<kMapVgg, FLAGS>(img, planar, n, chunk, params, os, ref, out, saved, part);
}
__global__ void __launch_bounds__(256) k_refloss_gated(UWIE_REFLOSS_FWD_ARGS)
{
    refloss_fwd_body<kMapGated, 0>(img, planar, n, chunk, params, os, ref, out, saved, part);
}
#undef UWIE_REFLOSS_FWD_ARGS

// One block: slot j of the nslots per-block partials goes to thread j % 256 (in slot order), then a fixed LDS tree.
// loss[0] = (float)(sum |d| / N), loss[1] = (float)(sum d * d / N): one rounding each.
__global__ void __launch_bounds__(256) k_refloss_finish(const double *__restrict__ part, int nslots, double count,
                                                        float *__restrict__ loss)
{
    __shared__ double rd[kLossPart][256];
    const int tid = threadIdx.x;
    double v0 = 0.0, v1 = 0.0;
    for (int j = tid; j < nslots; j += 256) {
        v0 += part[(size_t)j * kLossPart];
        v1 += part[(size_t)j * kLossPart + 1];
    }
    rd[0][tid] = v0;
    rd[1][tid] = v1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            rd[0][tid] += rd[0][tid + w];
            rd[1][tid] += rd[1][tid + w];
        }
        __syncthreads();
    }
    if (tid < kLossPart) loss[tid] = (float)(rd[tid][0] / count);
}

// The identity map's gradient: grad[i] = (gout ? gout[i] : 0) + dL/do[i], elementwise over all N = B * 3 * n values
__global__ void __launch_bounds__(256) k_refloss_identity_bwd(const float *__restrict__ o, const float *__restrict__ ref,
                                                              const float *__restrict__ gout, const LossGrad lg, size_t total,
                                                              float *__restrict__ grad)
{
    const LossK lk = loss_k(lg);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        grad[i] = refloss_grad(lk, o[i], ref[i], gout, i);
}

// pixels per block of the backward sweep and the cap on blocks per image (the partials' size)
constexpr int kBwdPxPerBlock = 2048, kBwdMaxBlocks = 512;
struct BwdGeom {
    int gx, chunk;
};
BwdGeom bwd_geom(Shape s)
{
    const long long n = (long long)s.npx();
    int gx = cdiv(n, kBwdPxPerBlock);
    if (gx > kBwdMaxBlocks) gx = kBwdMaxBlocks;
    int chunk = cdiv(n, gx);
    chunk = (chunk + 255) & ~255;  // whole 256-pixel tiles
    return {cdiv(n, chunk), chunk};
}

// the backward sweep's per-block partials in the workspace (nullptr: sizing)
struct BwdPart {
    double *part;
    uint32_t *cnt;
};
BwdPart carve_bwd(Carver &c, Shape s, BwdGeom g)
{
    return {c.take<double>((size_t)s.B * g.gx * kPartD), c.take<uint32_t>((size_t)s.B * g.gx * kPartU)};  // (in this order)
}

// LAUNCH(K<flags & 3>) for a launch macro LAUNCH(kernel) and a template <int FLAGS> kernel K
#define UWIE_FOR_FLAGS(LAUNCH, K, flags) \
    switch ((flags) & 3) {               \
    case 0: LAUNCH(K<0>); break;         \
    case 1: LAUNCH(K<1>); break;         \
    case 2: LAUNCH(K<2>); break;         \
    default: LAUNCH(K<3>); break;        \
    }

}  // namespace

int launch_diff_enhance(const float *d_img, int planar, Shape s, const float *d_params, int flags, const float *d_os,
                        float *d_out, hipStream_t st, float *d_saved)
{
    const int n = (int)s.npx();
    UWIE_LAUNCH(k_diff_enhance, dim3(grid_for(n, 4096), s.B), dim3(256), 0, st, d_img, planar, n, d_params, flags, d_os,
                d_out, d_saved);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

int launch_diff_gated(const float *d_img, int planar, Shape s, const float *d_params, const float *d_os, float *d_out,
                      hipStream_t st, float *d_saved)
{
    const int n = (int)s.npx();
    UWIE_LAUNCH(k_diff_gated, dim3(grid_for(n, 4096), s.B), dim3(256), 0, st, d_img, planar, n, d_params, d_os, d_out, d_saved);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

size_t diff_enhance_bwd_ws_bytes(Shape s)
{
    Carver c(nullptr);
    carve_bwd(c, s, bwd_geom(s));
    return c.total();
}

static LossGrad loss_grad_args(Shape s, const float *d_grad_loss)
{
    const long long N = (long long)s.B * 3 * (long long)s.npx();
    return LossGrad{d_grad_loss, (float)N, (float)(2.0 / (double)N)};
}

int launch_module_bwd(int map, const float *d_img, int planar, Shape s, const float *d_params, int flags, const float *d_saved,
                      const float *d_ref, const float *d_grad_out, const float *d_grad_loss, float *d_grad_img,
                      float *d_grad_params, void *ws, hipStream_t st)
{
    const int n = (int)s.npx();
    const BwdGeom g = bwd_geom(s);
    Carver c(ws);
    const BwdPart p = carve_bwd(c, s, g);
    const dim3 grid(g.gx, s.B);
#define UWIE_BWD(K) \
    UWIE_LAUNCH(K, grid, dim3(256), 0, st, d_img, planar, n, g.chunk, d_params, d_saved, d_grad_out, d_grad_img, p.part, p.cnt)
#define UWIE_LOSS_BWD(K) \
    UWIE_LAUNCH(K, grid, dim3(256), 0, st, d_img, planar, n, g.chunk, d_params, d_saved, d_grad_out, d_ref, lg, d_grad_img, p.part, p.cnt)
#define UWIE_BWD_FINISH(K) \
    UWIE_LAUNCH(K, dim3(3, s.B), dim3(256), 0, st, d_img, planar, n, g.chunk, g.gx, d_params, d_saved, p.part, p.cnt, d_grad_img, d_grad_params)
    if (d_grad_loss) {
        const LossGrad lg = loss_grad_args(s, d_grad_loss);
        if (map == kMapGated) UWIE_LOSS_BWD(k_diff_gated_loss_bwd);
        else UWIE_FOR_FLAGS(UWIE_LOSS_BWD, k_diff_enhance_loss_bwd, flags);
    } else {
        if (map == kMapGated) UWIE_BWD(k_diff_gated_bwd);
        else UWIE_FOR_FLAGS(UWIE_BWD, k_diff_enhance_bwd, flags);
    }
    UWIE_LAUNCH_CHECK();
    if (map == kMapGated) UWIE_BWD_FINISH(k_diff_enhance_bwd_finish<true>);
    else UWIE_BWD_FINISH(k_diff_enhance_bwd_finish<false>);
#undef UWIE_BWD
#undef UWIE_LOSS_BWD
#undef UWIE_BWD_FINISH
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

// ------------------------------------------------------------------ ReferenceLoss launchers
size_t refloss_ws_bytes(Shape s)
{
    const BwdGeom g = bwd_geom(s);
    Carver c(nullptr);
    c.take<double>((size_t)s.B * g.gx * kLossPart);
    return c.total();
}

int launch_refloss(int map, const float *d_img, int planar, Shape s, const float *d_params, int flags, const float *d_os,
                   const float *d_ref, float *d_out, float *d_saved, float *d_loss, void *ws, hipStream_t st)
{
    const int n = (int)s.npx();
    const BwdGeom g = bwd_geom(s);
    Carver c(ws);
    double *part = c.take<double>((size_t)s.B * g.gx * kLossPart);
    const dim3 grid(g.gx, s.B);
#define UWIE_REFLOSS_FWD(K) UWIE_LAUNCH(K, grid, dim3(256), 0, st, d_img, planar, n, g.chunk, d_params, d_os, d_ref, d_out, d_saved, part)
    if (map == kMapIdentity) UWIE_REFLOSS_FWD(k_refloss_identity);
    else if (map == kMapGated) UWIE_REFLOSS_FWD(k_refloss_gated);
    else UWIE_FOR_FLAGS(UWIE_REFLOSS_FWD, k_refloss_vgg, flags);
#undef UWIE_REFLOSS_FWD
    UWIE_LAUNCH_CHECK();
    const double count = (double)s.B * 3.0 * (double)s.npx();
    UWIE_LAUNCH(k_refloss_finish, dim3(1), dim3(256), 0, st, (const double *)part, s.B * g.gx, count, d_loss);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

int launch_refloss_bwd(int map, const float *d_img, int planar, Shape s, const float *d_params, int flags, const float *d_saved,
                       const float *d_ref, const float *d_grad_out, const float *d_grad_loss, float *d_grad_img,
                       float *d_grad_params, void *ws, hipStream_t st)
{
    if (map != kMapIdentity)
        return launch_module_bwd(map, d_img, planar, s, d_params, flags, d_saved, d_ref, d_grad_out, d_grad_loss, d_grad_img,
                                 d_grad_params, ws, st);
    const size_t total = (size_t)s.B * 3 * s.npx();
    UWIE_LAUNCH(k_refloss_identity_bwd, dim3(grid_for(total)), dim3(256), 0, st, d_img, d_ref, d_grad_out,
                loss_grad_args(s, d_grad_loss), total, d_grad_img);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
