// EndToEndTrainer.train_epoch's step for ParameterPredictor (deep_learning_parameters.py:265-306):
// the train-mode forward, the backward of the MLP, clip_grad_norm_ and Adam.  float32, one launch per layer, every sum in a
// fixed order (no floating-point atomics), no grid-wide waits.
//
//   k_mt_linear<EPI, X64>   one Linear layer of the train-mode forward: k_pn_linear's arithmetic (one wave per output neuron,
//                           the weight row in registers, the same multiply-adds and butterfly sum, so that p = 0 gives
//                           uwie_mlp_forward's bits) with the dropout sites in the epilogue:
//                           MT_RELU_DROP      relu, then dropout            (input_proj, block.0)
//                           MT_RES_DROP_RELU  (v + aux), dropout, then relu (block.3: the outer Dropout sits before the ReLU)
//                           MT_RELU           relu                          (output_proj)
//                           MT_HEADS          the four heads in the gated order; also keeps the sigmoids for the backward
//                           Dropout is v * (keep ? scale : 0), scale = float32(1 / (1 - p)).  The keep bit of (site, row,
//                           column) is given (uint8 [sites][B][hidden]) or drawn: Philox4x32-10 with the key (seed) and the
//                           counter (column, row, site, step), kept when the first word's top 24 bits / 2^24 >= p.  It depends
//                           on nothing else, so neither the launch shape nor B moves a bit.
//   k_mt_backward<X64>      one Linear layer's backward.  dZ = dY times the derivative of the layer's epilogue, formed as dY is
//                           loaded: a kept, positive output passes dY * scale and every other one 0 (the output is kept from
//                           the forward: it is positive exactly where the mask kept the unit and the ReLU passed it); the
//                           heads pass dY * range * sigmoid', and L_low / L_high pass an exact 0 without reading dY.
//                           The first blocks form dW and db: one wave per neuron n, lane l holds dW[n][l + 64 r], rows of
//                           the batch in ascending order.  The other blocks form dX for 64 columns and 8 rows: each wave walks
//                           a quarter of the neurons in ascending order, the four partial sums are added in wave order.  A
//                           weight is read for dX alone.  block.0 adds the residual branch's dZ to its dX.
//   k_mt_sumsq              per-block partial sums of squares of the gradient, float64, fixed order
//   k_mt_clip_adam          every block re-reduces the partials in the same order, forms clip_grad_norm_'s coefficient in
//                           float32 and applies the clip and torch's Adam update elementwise
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

constexpr int kKR = 18;          // weight registers per lane: K <= 64 * 18 = 1152
constexpr int kLdsRows = 8192;   // floats of batch rows staged in LDS per pass (32 KB), as k_pn_linear
constexpr int kBT = 8;           // batch rows per dX block
constexpr int kMaxN = 1152;
constexpr int kNormBlocks = 256;
enum { MT_RELU_DROP = 0, MT_RES_DROP_RELU = 1, MT_RELU = 2, MT_HEADS = 3 };

// ParameterPredictor's ranges (deep_learning_parameters.py:158-161) in the gated order: L_low, L_high, use_gamma, gamma
__constant__ float kMtScale[4] = {15.0f, 13.0f, 1.0f, 0.5f};
__constant__ float kMtMin[4] = {5.0f, 85.0f, 0.0f, 1.0f};

struct Drop {
    const uint8_t *given;  // [B][N] of this site, or nullptr: drawn
    uint8_t *drawn_out;    // [B][N] of this site, or nullptr
    uint32_t key0, key1, step, site;
    float p, scale;        // p == 0: no dropout at all
};

// Philox4x32-10 (Salmon et al., SC'11): first word of the block for counter (c0, c1, c2, c3) under key (k0, k1)
__device__ __forceinline__ uint32_t philox_first(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ bool keep_bit(const Drop &d, int b, int n, int N)
{
    bool keep;
    if (d.given) keep = d.given[(size_t)b * N + n] != 0;
    else keep = (float)(philox_first((uint32_t)n, (uint32_t)b, d.site, d.step, d.key0, d.key1) >> 8) * 0x1p-24f >= d.p;
    if (d.drawn_out) d.drawn_out[(size_t)b * N + n] = keep ? 1 : 0;
    return keep;
}

struct FwdArgs {
    const float *x;    // [B][K] (X64: float64 values)
    const float *w;    // [N][K]
    const float *b;    // [N]
    const float *aux;  // MT_RES_DROP_RELU: the block's input [B][N]
    float *y;          // [B][N]
    float *sg;         // MT_HEADS: the sigmoids [B][4]
    int B, K, N;
    Drop d;
};

template <int EPI, bool X64>
__global__ void __launch_bounds__(256) k_mt_linear(FwdArgs a)
{
    __shared__ float xs[kLdsRows];
    const int lane = threadIdx.x & 63, n0 = blockIdx.x * 4, n = n0 + (threadIdx.x >> 6);
    const bool live = n < a.N;
    const int span = a.K, rows = max(1, kLdsRows / span);
    float w[kKR], bias = 0.0f;
    if (live) {
        const float *wr = a.w + (size_t)n * a.K;
#pragma unroll
        for (int r = 0; r < kKR; ++r) {
            const int k = lane + 64 * r;
            w[r] = k < a.K ? wr[k] : 0.0f;
        }
        bias = a.b[n];
    }
    for (int b0 = 0; b0 < a.B; b0 += rows) {
        const int nr = min(rows, a.B - b0);
        __syncthreads();  // the previous pass's rows are consumed
        for (int i = threadIdx.x; i < nr * span; i += 256) {
            const size_t at = (size_t)b0 * a.K + i;
            if constexpr (X64) xs[i] = (float)reinterpret_cast<const double *>(a.x)[at];
            else xs[i] = a.x[at];
        }
        __syncthreads();
        if (!live) continue;
        for (int rr = 0; rr < nr; ++rr) {
            const int b = b0 + rr;
            const float *xr = xs + rr * span;
            float s = 0.0f;
#pragma unroll
            for (int r = 0; r < kKR; ++r) {
                const int k = lane + 64 * r;
                if (k < a.K) s = fmaf(w[r], xr[k], s);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane != 0) continue;
            float v = s + bias;
            if constexpr (EPI == MT_RELU_DROP) {
                v = relu_f(v);
                if (a.d.p != 0.0f) v = v * (keep_bit(a.d, b, n, a.N) ? a.d.scale : 0.0f);
            } else if constexpr (EPI == MT_RES_DROP_RELU) {
                v = v + a.aux[(size_t)b * a.N + n];
                if (a.d.p != 0.0f) v = v * (keep_bit(a.d, b, n, a.N) ? a.d.scale : 0.0f);
                v = relu_f(v);
            } else if constexpr (EPI == MT_RELU) {
                v = relu_f(v);
            } else {
                v = sigmoid_f(v);
                a.sg[(size_t)b * 4 + n] = v;
                if (n != 2) v = v * kMtScale[n] + kMtMin[n];  // use_gamma is the sigmoid itself
            }
            a.y[(size_t)b * a.N + n] = v;
        }
    }
}

struct BwdArgs {
    const float *x;      // the layer's input [B][K] (X64: float64 values)
    const float *w;      // [N][K]
    const float *dy;     // dL/d(the layer's output) [B][N]
    const float *y;      // the layer's output [B][N]; heads: the sigmoids [B][4]
    const float *res_dy, *res_y;  // block.0: the block's dL/d(output) and output [B][K], whose dZ is the residual's gradient
    float *dw, *db;      // [N][K], [N]
    float *dx;           // [B][K] or nullptr (input_proj)
    int B, K, N, ndw;    // ndw: the blocks that form dW and db
    int heads;
    float scale;         // the dropout scale of the layer's epilogue (1 where it has no dropout)
};

__device__ __forceinline__ float form_dz(const BwdArgs &a, int b, int n)
{
    if (a.heads) {
        if (n < 2) return 0.0f;  // L_low and L_high reach the loss through int(): no gradient, and dy's columns are not read
        const float sg = a.y[(size_t)b * 4 + n];
        return (a.dy[(size_t)b * 4 + n] * kMtScale[n]) * ((1.0f - sg) * sg);
    }
    const size_t at = (size_t)b * a.N + n;
    return a.y[at] > 0.0f ? a.dy[at] * a.scale : 0.0f;
}

template <bool X64>
__global__ void __launch_bounds__(256) k_mt_backward(BwdArgs a)
{
    __shared__ float dzs[kBT * kMaxN];
    __shared__ float red[4][kBT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < a.ndw) {
        const int n = blockIdx.x * 4 + wave;
        if (n >= a.N) return;
        float acc[kKR], sb = 0.0f;
#pragma unroll
        for (int r = 0; r < kKR; ++r) acc[r] = 0.0f;
        for (int b = 0; b < a.B; ++b) {
            const float dz = form_dz(a, b, n);
            sb += dz;
#pragma unroll
            for (int r = 0; r < kKR; ++r) {
                const int k = lane + 64 * r;
                if (k < a.K) {
                    float xv;
                    if constexpr (X64) xv = (float)reinterpret_cast<const double *>(a.x)[(size_t)b * a.K + k];
                    else xv = a.x[(size_t)b * a.K + k];
                    acc[r] = fmaf(dz, xv, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kKR; ++r) {
            const int k = lane + 64 * r;
            if (k < a.K) a.dw[(size_t)n * a.K + k] = acc[r];
        }
        if (lane == 0) a.db[n] = sb;
        return;
    }
    // dX[b][k] = sum over n of dZ[b][n] * W[n][k] for 64 columns and kBT rows
    const int kblocks = (a.K + 63) / 64, id = blockIdx.x - a.ndw;
    const int k = (id % kblocks) * 64 + lane, b0 = (id / kblocks) * kBT;
    for (int i = threadIdx.x; i < kBT * a.N; i += 256) {
        const int j = i / a.N, n = i - j * a.N;
        dzs[i] = b0 + j < a.B ? form_dz(a, b0 + j, n) : 0.0f;
    }
    __syncthreads();
    const int q = (a.N + 3) / 4, nbeg = wave * q, nend = min(a.N, nbeg + q);
    float acc[kBT];
#pragma unroll
    for (int j = 0; j < kBT; ++j) acc[j] = 0.0f;
    if (k < a.K) {
        for (int n = nbeg; n < nend; ++n) {
            const float wv = a.w[(size_t)n * a.K + k];
#pragma unroll
            for (int j = 0; j < kBT; ++j) acc[j] = fmaf(dzs[j * a.N + n], wv, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < kBT; ++j) red[wave][j][lane] = acc[j];
    __syncthreads();
    if (k >= a.K) return;
    for (int j = wave; j < kBT; j += 4) {
        const int b = b0 + j;
        if (b >= a.B) continue;
        float v = ((red[0][j][lane] + red[1][j][lane]) + red[2][j][lane]) + red[3][j][lane];
        if (a.res_dy) {
            const size_t at = (size_t)b * a.K + k;
            v += a.res_y[at] > 0.0f ? a.res_dy[at] * a.scale : 0.0f;
        }
        a.dx[(size_t)b * a.K + k] = v;
    }
}

struct Skip {
    long long a0, a1, b0, b1;  // [a0, a1) and [b0, b1): the gradient-free heads' weights and biases
    __device__ __forceinline__ bool hit(long long i) const { return (i >= a0 && i < a1) || (i >= b0 && i < b1); }
};

__device__ __forceinline__ double block_sum_f64(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// block i sums the squares of elements [i * per, (i + 1) * per): thread t takes t, t + 256, ..., then a fixed tree
__global__ void __launch_bounds__(256) k_mt_sumsq(const float *__restrict__ g, long long n, long long per, Skip skip,
                                                  double *__restrict__ partial)
{
    __shared__ double red[256];
    const long long beg = (long long)blockIdx.x * per, end = min(n, beg + per);
    double s = 0.0;
    for (long long i = beg + threadIdx.x; i < end; i += 256)
        if (!skip.hit(i)) {
            const double v = (double)g[i];
            s += v * v;
        }
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct AdamArgs {
    float *p, *g, *m, *v;
    long long n;
    const double *partial;
    int nparts;
    double *norm_out;
    float max_norm, w1, beta2, w2, bc2_sqrt, eps, neg_step;
    Skip skip;
};

__global__ void __launch_bounds__(256) k_mt_clip_adam(AdamArgs a)
{
    __shared__ double red[256];
    const double total = block_sum_f64((int)threadIdx.x < a.nparts ? a.partial[threadIdx.x] : 0.0, red);
    const double norm64 = sqrt(total);
    if (a.norm_out && blockIdx.x == 0 && threadIdx.x == 0) *a.norm_out = norm64;
    // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1 (a NaN stays NaN)
    float coef = a.max_norm / ((float)norm64 + 1e-6f);
    coef = coef > 1.0f ? 1.0f : coef;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {
        if (a.skip.hit(i)) continue;
        const float g = a.g[i] * coef;
        float m = a.m[i], v = a.v[i];
        m = m + a.w1 * (g - m);                     // exp_avg.lerp_(grad, 1 - beta1)
        v = v * a.beta2 + (a.w2 * g) * g;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
        a.g[i] = g;
        a.m[i] = m;
        a.v[i] = v;
        a.p[i] = a.p[i] + a.neg_step * (m / denom);  // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
}

struct TrainBufs {
    float *x;      // [nb + 1][B][H]: the inputs of the blocks and of output_proj
    float *t;      // [nb][B][H]: block.0's dropped outputs
    float *f;      // [B][H / 2]
    float *sg;     // [B][4]
    float *ga, *gb, *gt;  // [B][H] gradients
    float *gf;     // [B][H / 2]
};

TrainBufs carve_train(int B, int H, int nb, void *ws, size_t *total = nullptr)
{
    const size_t bh = (size_t)B * H;
    Carver c(ws);
    TrainBufs A;
    A.x = c.take<float>(bh * (nb + 1));
    A.t = c.take<float>(bh * (nb > 0 ? nb : 1));
    A.f = c.take<float>((size_t)B * (H / 2));
    A.sg = c.take<float>((size_t)B * 4);
    A.ga = c.take<float>(bh);
    A.gb = c.take<float>(bh);
    A.gt = c.take<float>(bh);
    A.gf = c.take<float>((size_t)B * (H / 2));
    if (total) *total = c.total();
    return A;
}

template <int EPI, bool X64 = false>
int fwd_layer(const char *name, const float *x, const float *w, const float *b, const float *aux, float *y, float *sg, int B, int K,
              int N, const Drop &d, hipStream_t st)
{
    FwdArgs a{x, w, b, aux, y, sg, B, K, N, d};
    UWIE_PROF(name, st);
    hipLaunchKernelGGL((k_mt_linear<EPI, X64>), dim3(cdiv(N, 4)), dim3(256), 0, st, a);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

int bwd_layer(const char *name, bool x64, BwdArgs a, hipStream_t st)
{
    a.ndw = cdiv(a.N, 4);
    const int ndx = a.dx ? cdiv(a.K, 64) * cdiv(a.B, kBT) : 0;
    UWIE_PROF(name, st);
    if (x64) hipLaunchKernelGGL(k_mt_backward<true>, dim3(a.ndw + ndx), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_mt_backward<false>, dim3(a.ndw + ndx), dim3(256), 0, st, a);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

#define MT_TRY(call)                      \
    do {                                  \
        const int _rc = (call);           \
        if (_rc != UWIE_OK) return _rc;   \
    } while (0)

Skip skip_of(const Mlp &net)
{
    const long long half = net.H / 2, body = (long long)mlp_count(net.F, net.H, net.nb) - 4 * (half + 1);
    // the packed order: ... output_proj, the heads' weights [4][half] in the gated order (L_low, L_high first), their biases [4]
    return Skip{body, body + 2 * half, body + 4 * half, body + 4 * half + 2};
}

}  // namespace

size_t mlp_train_ws_bytes(int B, int hidden, int nb)
{
    size_t n = 0;
    (void)carve_train(B, hidden, nb, nullptr, &n);
    return n;
}

int mlp_train_sites(int nb) { return 1 + 2 * nb; }

int launch_mlp_train_forward(const Mlp &net, const void *feat, bool f64, int B, double p, const uint8_t *given, uint8_t *drawn_out,
                             uint64_t seed, uint32_t step, float *out, void *ws, hipStream_t st)
{
    const TrainBufs A = carve_train(B, net.H, net.nb, ws);
    const int F = net.F, Hd = net.H, half = Hd / 2;
    const size_t bh = (size_t)B * Hd;
    Drop d{nullptr, nullptr, (uint32_t)seed, (uint32_t)(seed >> 32), step, 0, (float)p, (float)(1.0 / (1.0 - p))};
    auto site = [&](int s) {
        Drop r = d;
        r.site = (uint32_t)s;
        r.given = given ? given + (size_t)s * bh : nullptr;
        r.drawn_out = drawn_out ? drawn_out + (size_t)s * bh : nullptr;
        return r;
    };
    const float *q = net.base;
    const float *w = q, *b = q + (size_t)Hd * F;
    q = b + Hd;
    const float *x0 = static_cast<const float *>(feat);
    if (f64) MT_TRY((fwd_layer<MT_RELU_DROP, true>("mlp train input_proj", x0, w, b, nullptr, A.x, nullptr, B, F, Hd, site(0), st)));
    else MT_TRY((fwd_layer<MT_RELU_DROP>("mlp train input_proj", x0, w, b, nullptr, A.x, nullptr, B, F, Hd, site(0), st)));
    for (int k = 0; k < net.nb; ++k) {
        const float *w1 = q, *b1 = w1 + (size_t)Hd * Hd, *w2 = b1 + Hd, *b2 = w2 + (size_t)Hd * Hd;
        q = b2 + Hd;
        float *xin = A.x + (size_t)k * bh, *t = A.t + (size_t)k * bh;
        MT_TRY((fwd_layer<MT_RELU_DROP>("mlp train block.0", xin, w1, b1, nullptr, t, nullptr, B, Hd, Hd, site(1 + 2 * k), st)));
        MT_TRY((fwd_layer<MT_RES_DROP_RELU>("mlp train block.3", t, w2, b2, xin, xin + bh, nullptr, B, Hd, Hd, site(2 + 2 * k), st)));
    }
    const float *xl = A.x + (size_t)net.nb * bh;
    MT_TRY((fwd_layer<MT_RELU>("mlp train output_proj", xl, q, q + (size_t)half * Hd, nullptr, A.f, nullptr, B, Hd, half, d, st)));
    MT_TRY((fwd_layer<MT_HEADS>("mlp train heads", A.f, net.hw, net.hb, nullptr, out, A.sg, B, half, 4, d, st)));
    return UWIE_OK;
}

// grads: the packed order of the parameters (mlp_pack).  scale: the dropout scale of the forward that filled ws.
int launch_mlp_backward(const Mlp &net, float *grads, const void *feat, bool f64, int B, float scale, const float *grad_out, void *ws,
                        hipStream_t st)
{
    const TrainBufs A = carve_train(B, net.H, net.nb, ws);
    const int F = net.F, Hd = net.H, half = Hd / 2;
    const size_t bh = (size_t)B * Hd, hh = (size_t)Hd * Hd;
    const size_t body = mlp_count(F, Hd, net.nb) - 4 * ((size_t)half + 1);
    const size_t o_out = (size_t)Hd * F + Hd + (size_t)net.nb * 2 * (hh + Hd);  // output_proj.0.weight
    const float *P = net.base;
    float *G = grads;
    const float *xl = A.x + (size_t)net.nb * bh;
    BwdArgs h{A.f, net.hw, grad_out, A.sg, nullptr, nullptr, G + body, G + body + 4 * (size_t)half, A.gf, B, half, 4, 0, 1, 1.0f};
    MT_TRY(bwd_layer("mlp bwd heads", false, h, st));
    BwdArgs o{xl, P + o_out, A.gf, A.f, nullptr, nullptr, G + o_out, G + o_out + (size_t)half * Hd, A.ga, B, Hd, half, 0, 0, 1.0f};
    MT_TRY(bwd_layer("mlp bwd output_proj", false, o, st));
    float *gcur = A.ga, *gnext = A.gb;
    for (int k = net.nb - 1; k >= 0; --k) {
        const size_t o1 = (size_t)Hd * F + Hd + (size_t)k * 2 * (hh + Hd), o2 = o1 + hh + Hd;
        const float *xin = A.x + (size_t)k * bh, *t = A.t + (size_t)k * bh, *xout = xin + bh;
        BwdArgs l3{t, P + o2, gcur, xout, nullptr, nullptr, G + o2, G + o2 + hh, A.gt, B, Hd, Hd, 0, 0, scale};
        MT_TRY(bwd_layer("mlp bwd block.3", false, l3, st));
        BwdArgs l0{xin, P + o1, A.gt, t, gcur, xout, G + o1, G + o1 + hh, gnext, B, Hd, Hd, 0, 0, scale};
        MT_TRY(bwd_layer("mlp bwd block.0", false, l0, st));
        std::swap(gcur, gnext);
    }
    BwdArgs in{static_cast<const float *>(feat), P, gcur, A.x, nullptr, nullptr, G, G + (size_t)Hd * F, nullptr, B, F, Hd, 0, 0, scale};
    MT_TRY(bwd_layer("mlp bwd input_proj", f64, in, st));
    return UWIE_OK;
}

size_t mlp_adam_scratch_bytes() { return kNormBlocks * sizeof(double); }

int launch_mlp_adam(const Mlp &net, float *params, float *grads, float *m, float *v, double *partial, const MlpAdam &h, double *norm_out,
                    hipStream_t st)
{
    const long long n = (long long)mlp_count(net.F, net.H, net.nb);
    const int nparts = (int)std::min<long long>(kNormBlocks, (n + 1023) / 1024);
    const long long per = (n + nparts - 1) / nparts;
    const Skip skip = skip_of(net);
    UWIE_LAUNCH(k_mt_sumsq, dim3(nparts), dim3(256), 0, st, grads, n, per, skip, partial);
    UWIE_LAUNCH_CHECK();
    AdamArgs a{params, grads, m, v, n, partial, nparts, norm_out, h.max_norm, h.w1, h.beta2, h.w2, h.bc2_sqrt, h.eps, h.neg_step, skip};
    UWIE_LAUNCH(k_mt_clip_adam, dim3(grid_for((size_t)n, 1024)), dim3(256), 0, st, a);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

// state_dict() order <-> the packed order (mlp_pack's): the body as it is, the four heads gathered in the gated order
int mlp_repack(const float *src, float *dst, int F, int Hd, int nb, bool to_state, hipStream_t st)
{
    const size_t half = (size_t)Hd / 2, body = mlp_count(F, Hd, nb) - 4 * (half + 1);
    UWIE_HIP_CHECK(hipMemcpyAsync(dst, src, body * sizeof(float), hipMemcpyDeviceToDevice, st));
    const int from_state[4] = {1, 2, 3, 0};  // L_low, L_high, use_gamma, gamma
    for (int j = 0; j < 4; ++j) {
        const size_t s_w = body + (size_t)from_state[j] * (half + 1), s_b = s_w + half;  // in state order
        const size_t p_w = body + (size_t)j * half, p_b = body + 4 * half + j;           // packed
        if (to_state) {
            UWIE_HIP_CHECK(hipMemcpyAsync(dst + s_w, src + p_w, half * sizeof(float), hipMemcpyDeviceToDevice, st));
            UWIE_HIP_CHECK(hipMemcpyAsync(dst + s_b, src + p_b, sizeof(float), hipMemcpyDeviceToDevice, st));
        } else {
            UWIE_HIP_CHECK(hipMemcpyAsync(dst + p_w, src + s_w, half * sizeof(float), hipMemcpyDeviceToDevice, st));
            UWIE_HIP_CHECK(hipMemcpyAsync(dst + p_b, src + s_b, sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    }
    return UWIE_OK;
}

}  // namespace uwie
