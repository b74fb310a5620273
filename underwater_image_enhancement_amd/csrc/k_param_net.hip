// ImprovedVGGParameterNet.forward in eval mode (vgg_16_UIE.py:135-255), float32, no autograd.
//
//   launch_param_trunk (k_vgg.hip)  features[:23] -> relu4_3 [B][H/8][W/8][512], channels-last, on k_vgg_conv
//   k_pn_avgpool                    the global average per (image, channel): per-thread partials over a fixed pixel stride,
//                                   finished in a fixed order (no atomics); written at [c] and [512 + c] of the fusion input
//                                   row (avgpool and the reference's "maxpool", both AdaptiveAvgPool2d), then the 79 features
//   k_pn_linear<EPI>                one Linear layer: one wave per output neuron keeps that neuron's weight row in registers
//                                   (each weight read once per call) and forms its dot product with every row of the batch
//                                   (a butterfly sum, fixed order); the block's four neurons share the batch rows, staged
//                                   in LDS 32 KB at a time.  Epilogues:
//                                   LIN_BN_RELU  BatchNorm1d with running statistics, (x - mean) * rsqrt(var + eps) * w + b,
//                                                then ReLU (Dropout is the identity in eval mode)
//                                   LIN_RELU     ReLU
//                                   LIN_ATTN     fused * sigmoid(x): the attention product
//                                   LIN_RANGE    sigmoid(x) * (max - min) + min with the head's param_ranges
//                                   LIN_RES_RELU   relu(x + aux): a residual block's second layer (ParameterPredictor)
//                                   LIN_GATED_RANGE  sigmoid(x) * scale + min with ParameterPredictor's ranges, gated order
//                                   X64: the input rows are float64 and are rounded to float32 as they are staged
//   k_pn_u8_to_f32                  EnhancementPredictor's float image u8 / 255, in the frames' own layout
//
// deep_learning_parameters.ParameterPredictor.forward in eval mode (:97-163) is five kinds of launch of
// the same kernel (launch_mlp): input_proj, per residual block two layers, output_proj, and the four heads as one N = 4 layer.
#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

constexpr int kKR = 18;  // weight registers per lane: K <= 64 * 18 = 1152
constexpr int kFeat = 79, kHalf = 512, kPooled = 1024, kHid = 256, kHead = 128;
enum { LIN_BN_RELU = 0, LIN_RELU = 1, LIN_ATTN = 2, LIN_RANGE = 3, LIN_RES_RELU = 4, LIN_GATED_RANGE = 5 };

// param_ranges (vgg_16_UIE.py:193-198) in ModuleDict order: omega, gamma, L_low, L_high.  torch multiplies the float32
// sigmoid by the Python float (max - min) and adds min, each operand rounded to float32 first.
__constant__ float kRangeScale[4] = {(float)(0.9 - 0.3), (float)(1.5 - 1.0), (float)(15.0 - 2.0), (float)(95.0 - 60.0)};
__constant__ float kRangeMin[4] = {0.3f, 1.0f, 2.0f, 60.0f};
// ParameterPredictor's ranges (deep_learning_parameters.py:158-161) in the gated module's column order: L_low, L_high,
// use_gamma, gamma.  sigmoid * 15 + 5, sigmoid * 13 + 85, sigmoid, sigmoid * 0.5 + 1.0: the Python numbers as float32.
__constant__ float kGatedScale[4] = {15.0f, 13.0f, 1.0f, 0.5f};
__constant__ float kGatedMin[4] = {5.0f, 85.0f, 0.0f, 1.0f};

struct LinArgs {
    const float *x;    // [B][ldx] (X64: float64 values)
    const float *w;    // [N][K]
    const float *b;    // [N]
    const float *bn;   // LIN_BN_RELU: [4][N] = weight, bias, running_mean, running_var
    const float *aux;  // LIN_ATTN: the fused vector [B][N]; LIN_RES_RELU: the block's input [B][N]
    float *y;          // [B][N]
    int B, K, N, ldx;
    int xstep;         // input offset per output neuron (the heads' last layers read their own 128 hidden values)
};

constexpr int kLdsRows = 8192;  // floats of batch rows staged in LDS per pass (32 KB)

template <int EPI, bool X64 = false>
__global__ void __launch_bounds__(256) k_pn_linear(LinArgs a)
{
    __shared__ float xs[kLdsRows];
    const int lane = threadIdx.x & 63, n0 = blockIdx.x * 4, n = n0 + (threadIdx.x >> 6);
    const bool live = n < a.N;
    // the part of each batch row that this block's neurons read: [n0 * xstep, nlast * xstep + K), at most ldx floats
    const int nlast = min(n0 + 3, a.N - 1), span = (nlast - n0) * a.xstep + a.K, rows = max(1, kLdsRows / span);
    const float *xg = a.x + (size_t)n0 * a.xstep;
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
            const int r = i / span;
            const size_t at = (size_t)(b0 + r) * a.ldx + (i - r * span);
            if constexpr (X64) xs[i] = (float)(reinterpret_cast<const double *>(a.x) + (size_t)n0 * a.xstep)[at];
            else xs[i] = xg[at];
        }
        __syncthreads();
        if (!live) continue;
        for (int rr = 0; rr < nr; ++rr) {
            const int b = b0 + rr;
            const float *xr = xs + rr * span + (n - n0) * a.xstep;
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
            if constexpr (EPI == LIN_BN_RELU) {
                const float g = a.bn[n], be = a.bn[a.N + n], mu = a.bn[2 * a.N + n], var = a.bn[3 * a.N + n];
                v = relu_f((v - mu) * (1.0f / sqrtf(var + 1e-5f)) * g + be);
            } else if constexpr (EPI == LIN_RELU) {
                v = relu_f(v);
            } else if constexpr (EPI == LIN_ATTN) {
                v = a.aux[(size_t)b * a.N + n] * sigmoid_f(v);
            } else if constexpr (EPI == LIN_RES_RELU) {
                v = relu_f(v + a.aux[(size_t)b * a.N + n]);
            } else if constexpr (EPI == LIN_GATED_RANGE) {
                v = sigmoid_f(v);
                if (n != 2) v = v * kGatedScale[n] + kGatedMin[n];  // use_gamma is the sigmoid itself
            } else {
                v = sigmoid_f(v) * kRangeScale[n] + kRangeMin[n];
            }
            a.y[(size_t)b * a.N + n] = v;
        }
    }
}

// EnhancementPredictor's image: out[i] = (float)in[i] / 255.0f (NumPy's u8.astype(float32) / 255.0), any layout;
// four bytes per thread, the n % 4 tail by the first threads
__global__ void __launch_bounds__(256) k_pn_u8_to_f32(const uint8_t *__restrict__ in, size_t n, float *__restrict__ out)
{
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const uint32_t v = reinterpret_cast<const uint32_t *>(in)[i];
        float4 f;
        f.x = (float)(v & 0xffu) / 255.0f;
        f.y = (float)((v >> 8) & 0xffu) / 255.0f;
        f.z = (float)((v >> 16) & 0xffu) / 255.0f;
        f.w = (float)(v >> 24) / 255.0f;
        reinterpret_cast<float4 *>(out)[i] = f;
    }
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n - 4 * n4) out[4 * n4 + t] = (float)in[4 * n4 + t] / 255.0f;
}

// grid: 8 blocks per image, each 64 channels of relu4_3 [B][P][512]; thread (c, q) sums pixels q, q + 4, ...
__global__ void __launch_bounds__(256) k_pn_avgpool(const float *__restrict__ act, int P, const float *__restrict__ feat, int din,
                                                    float *__restrict__ comb, float *__restrict__ pooled)
{
    __shared__ float red[256];
    const int tid = threadIdx.x, b = blockIdx.x >> 3, c = (blockIdx.x & 7) * 64 + (tid & 63);
    const float *src = act + (size_t)b * P * kHalf + c;
    float s = 0.0f;
    for (int p = tid >> 6; p < P; p += 4) s += src[(size_t)p * kHalf];
    red[tid] = s;
    __syncthreads();
    if (tid < 64) {
        const float m = (((red[tid] + red[tid + 64]) + red[tid + 128]) + red[tid + 192]) / (float)P;
        float *row = comb + (size_t)b * din;
        row[c] = m;
        row[kHalf + c] = m;
        if (pooled) {
            pooled[(size_t)b * kPooled + c] = m;
            pooled[(size_t)b * kPooled + kHalf + c] = m;
        }
    }
    if ((blockIdx.x & 7) == 0 && din > kPooled)
        for (int i = tid; i < kFeat; i += 256) comb[(size_t)b * din + kPooled + i] = feat[(size_t)b * kFeat + i];
}

struct PnBufs {
    float *X, *Y, *comb, *h1, *h2, *a1, *fused, *hh;
};

PnBufs carve_pn(Shape s, void *ws, size_t *total = nullptr)
{
    const size_t P1 = (size_t)s.B * s.H * s.W, B = (size_t)s.B;
    Carver c(ws);
    PnBufs A;
    A.X = c.take<float>(P1 * 64);  // the trunk's ping-pong: conv1_1's output is the largest activation
    A.Y = c.take<float>(P1 * 64);
    A.comb = c.take<float>(B * (kPooled + kFeat));
    A.h1 = c.take<float>(B * 2 * kHid);
    A.h2 = c.take<float>(B * kHid);
    A.a1 = c.take<float>(B * (kHid / 4));
    A.fused = c.take<float>(B * kHid);
    A.hh = c.take<float>(B * 4 * kHead);
    if (total) *total = c.total();
    return A;
}

template <int EPI, bool X64 = false>
int linear(const char *name, const float *x, int ldx, int xstep, const float *w, const float *b, const float *bn, const float *aux,
           float *y, int B, int K, int N, hipStream_t st)
{
    if (K > 64 * kKR || (size_t)(N - 1) * xstep + K > (size_t)ldx) {
        set_error("param_net: internal Linear shape out of range (K %d, N %d)", K, N);
        return UWIE_E_INVALID;
    }
    LinArgs a{x, w, b, bn, aux, y, B, K, N, ldx, xstep};
    UWIE_PROF(name, st);
    hipLaunchKernelGGL((k_pn_linear<EPI, X64>), dim3(cdiv(N, 4)), dim3(256), 0, st, a);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

#define PN_TRY(call)                      \
    do {                                  \
        const int _rc = (call);           \
        if (_rc != UWIE_OK) return _rc;   \
    } while (0)

constexpr int kConv4Cin[3] = {256, 512, 512};
constexpr size_t kHeadTail = 4 * ((size_t)kHead * kHid + kHead + kHead + 1);  // param_heads.K.0 and .3, K = 0 .. 3

size_t head_count(int din)
{
    return (size_t)2 * kHid * din + 2 * kHid + 4 * 2 * kHid  // feature_fusion.0, .1
           + (size_t)kHid * 2 * kHid + kHid + 4 * kHid       // feature_fusion.4, .5
           + (size_t)(kHid / 4) * kHid + kHid / 4            // attention.0
           + (size_t)kHid * (kHid / 4) + kHid                // attention.2
           + kHeadTail;
}

// blob: [vgg_blob_bytes(UWIE_VGG_F32): conv1_1 ... conv3_3][conv4_l: wf, bias][feature_fusion.0 ... attention.2.bias in
//       d_params' layout][heads.0 weights [4 * 128][256], their biases [512], heads.3 weights [4][128], their biases [4]]
void carve_blob(int din, void *blob, float **wf4, float **b4, float **lin, float **hw, size_t *total)
{
    Carver c(blob ? static_cast<char *>(blob) + vgg_blob_bytes(UWIE_VGG_F32) : nullptr);
    for (int l = 0; l < 3; ++l) {
        wf4[l] = c.take<float>((size_t)512 * 9 * kConv4Cin[l]);
        b4[l] = c.take<float>(512);
    }
    *lin = c.take<float>(head_count(din) - kHeadTail);
    hw[0] = c.take<float>((size_t)4 * kHead * kHid);
    hw[1] = c.take<float>(4 * kHead);
    hw[2] = c.take<float>(4 * kHead);
    hw[3] = c.take<float>(4);
    if (total) *total = vgg_blob_bytes(UWIE_VGG_F32) + c.total();
}

}  // namespace

size_t param_net_count(int use_features)
{
    size_t n = vgg_param_count();
    for (int l = 0; l < 3; ++l) n += (size_t)512 * 9 * kConv4Cin[l] + 512;
    return n + head_count(use_features ? kPooled + kFeat : kPooled);
}

size_t param_net_scratch_floats() { return (size_t)512 * 9 * 512; }

size_t param_net_blob_bytes(int use_features)
{
    float *wf4[3], *b4[3], *lin, *hw[4];
    size_t n = 0;
    carve_blob(use_features ? kPooled + kFeat : kPooled, nullptr, wf4, b4, &lin, hw, &n);
    return n;
}

int param_net_pack(const float *d_params, int use_features, void *blob, float *scratch, ParamNet *net, hipStream_t st)
{
    const int din = use_features ? kPooled + kFeat : kPooled;
    PN_TRY(vgg_pack(d_params, UWIE_VGG_F32, blob, &net->trunk, st));
    float *wf4[3], *b4[3], *lin, *hw[4];
    carve_blob(din, blob, wf4, b4, &lin, hw, nullptr);
    const float *src = d_params + vgg_param_count();
    for (int l = 0; l < 3; ++l) {
        PN_TRY(vgg_pack_conv_f32(src, 512, kConv4Cin[l], wf4[l], scratch, b4[l], st));
        net->wf4[l] = wf4[l];
        net->bias4[l] = b4[l];
        src += (size_t)512 * 9 * kConv4Cin[l] + 512;
    }
    // feature_fusion and attention keep d_params' layout
    const size_t nlin = head_count(din) - kHeadTail;
    UWIE_HIP_CHECK(hipMemcpyAsync(lin, src, nlin * sizeof(float), hipMemcpyDeviceToDevice, st));
    src += nlin;
    const float *p = lin;
    net->din = din;
    net->lw[0] = p, p += (size_t)2 * kHid * din;
    net->lb[0] = p, p += 2 * kHid;
    net->bn[0] = p, p += 4 * 2 * kHid;
    net->lw[1] = p, p += (size_t)kHid * 2 * kHid;
    net->lb[1] = p, p += kHid;
    net->bn[1] = p, p += 4 * kHid;
    net->lw[2] = p, p += (size_t)(kHid / 4) * kHid;
    net->lb[2] = p, p += kHid / 4;
    net->lw[3] = p, p += (size_t)kHid * (kHid / 4);
    net->lb[3] = p;
    // the four heads, gathered so that each of their two layers is one launch
    for (int h = 0; h < 4; ++h) {
        const size_t sizes[4] = {(size_t)kHead * kHid, kHead, kHead, 1};
        float *dst[4] = {hw[0] + (size_t)h * kHead * kHid, hw[1] + h * kHead, hw[2] + h * kHead, hw[3] + h};
        for (int t = 0; t < 4; ++t) {
            UWIE_HIP_CHECK(hipMemcpyAsync(dst[t], src, sizes[t] * sizeof(float), hipMemcpyDeviceToDevice, st));
            src += sizes[t];
        }
    }
    net->lw[4] = hw[0];
    net->lb[4] = hw[1];
    net->lw[5] = hw[2];
    net->lb[5] = hw[3];
    return UWIE_OK;
}

size_t param_net_ws_bytes(Shape s)
{
    size_t n = 0;
    (void)carve_pn(s, nullptr, &n);
    return n;
}

int launch_u8_to_f32(const uint8_t *d_in, size_t n, float *d_out, hipStream_t st)
{
    UWIE_LAUNCH(k_pn_u8_to_f32, dim3(grid_for((n + 3) / 4)), dim3(256), 0, st, d_in, n, d_out);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

int launch_param_net(const ParamNet &net, const float *img, const float *feat, Shape s, float *out, float *pooled, void *ws,
                     hipStream_t st)
{
    const PnBufs A = carve_pn(s, ws);
    const int B = s.B, din = net.din, P = (s.H / 8) * (s.W / 8);
    float *r43 = nullptr;
    PN_TRY(launch_param_trunk(net.trunk, net.wf4, net.bias4, img, s, A.X, A.Y, &r43, st));
    UWIE_LAUNCH(k_pn_avgpool, dim3(8 * B), dim3(256), 0, st, r43, P, feat, din, A.comb, pooled);
    UWIE_LAUNCH_CHECK();
    PN_TRY(linear<LIN_BN_RELU>("pn fusion.0", A.comb, din, 0, net.lw[0], net.lb[0], net.bn[0], nullptr, A.h1, B, din, 2 * kHid, st));
    PN_TRY(linear<LIN_BN_RELU>("pn fusion.4", A.h1, 2 * kHid, 0, net.lw[1], net.lb[1], net.bn[1], nullptr, A.h2, B, 2 * kHid, kHid, st));
    PN_TRY(linear<LIN_RELU>("pn attention.0", A.h2, kHid, 0, net.lw[2], net.lb[2], nullptr, nullptr, A.a1, B, kHid, kHid / 4, st));
    PN_TRY(linear<LIN_ATTN>("pn attention.2", A.a1, kHid / 4, 0, net.lw[3], net.lb[3], nullptr, A.h2, A.fused, B, kHid / 4, kHid, st));
    PN_TRY(linear<LIN_RELU>("pn heads.0", A.fused, kHid, 0, net.lw[4], net.lb[4], nullptr, nullptr, A.hh, B, kHid, 4 * kHead, st));
    PN_TRY(linear<LIN_RANGE>("pn heads.3", A.hh, 4 * kHead, kHead, net.lw[5], net.lb[5], nullptr, nullptr, out, B, kHead, 4, st));
    return UWIE_OK;
}

// ---------------------------------------------------------------- ParameterPredictor
namespace {

struct MlpBufs {
    float *X, *T, *Y, *half;
};
MlpBufs carve_mlp(int B, int hidden, void *ws, size_t *total = nullptr)
{
    Carver c(ws);
    MlpBufs A;
    A.X = c.take<float>((size_t)B * hidden);
    A.T = c.take<float>((size_t)B * hidden);
    A.Y = c.take<float>((size_t)B * hidden);
    A.half = c.take<float>((size_t)B * (hidden / 2));
    if (total) *total = c.total();
    return A;
}

}  // namespace

size_t mlp_count(int F, int Hd, int nb)
{
    const size_t h = (size_t)Hd, half = h / 2;
    return (size_t)F * h + h + (size_t)nb * 2 * (h * h + h) + half * h + half + 4 * (half + 1);
}

// blob = d_params as it is (state_dict() order) up to output_proj; the four heads (state order gamma, L_low, L_high,
// use_gamma, each a weight row and a bias) gathered as one [4][hidden / 2] layer in the gated order
int mlp_pack(const float *d_params, int F, int Hd, int nb, float *blob, Mlp *net, hipStream_t st)
{
    const size_t h = (size_t)Hd, half = h / 2, body = mlp_count(F, Hd, nb) - 4 * (half + 1);
    UWIE_HIP_CHECK(hipMemcpyAsync(blob, d_params, body * sizeof(float), hipMemcpyDeviceToDevice, st));
    float *hw = blob + body, *hb = hw + 4 * half;
    const int from_state[4] = {1, 2, 3, 0};  // L_low, L_high, use_gamma, gamma
    for (int j = 0; j < 4; ++j) {
        const float *src = d_params + body + (size_t)from_state[j] * (half + 1);
        UWIE_HIP_CHECK(hipMemcpyAsync(hw + (size_t)j * half, src, half * sizeof(float), hipMemcpyDeviceToDevice, st));
        UWIE_HIP_CHECK(hipMemcpyAsync(hb + j, src + half, sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    net->F = F, net->H = Hd, net->nb = nb;
    net->base = blob;
    net->hw = hw, net->hb = hb;
    return UWIE_OK;
}

size_t mlp_ws_bytes(int B, int hidden)
{
    size_t n = 0;
    (void)carve_mlp(B, hidden, nullptr, &n);
    return n;
}

int launch_mlp(const Mlp &net, const void *feat, bool f64, int B, float *out, void *ws, hipStream_t st)
{
    MlpBufs A = carve_mlp(B, net.H, ws);
    const int F = net.F, Hd = net.H, half = Hd / 2;
    const float *p = net.base;
    const float *w = p, *b = p + (size_t)Hd * F;
    p = b + Hd;
    if (f64) PN_TRY((linear<LIN_RELU, true>("mlp input_proj", static_cast<const float *>(feat), F, 0, w, b, nullptr, nullptr, A.X, B, F, Hd, st)));
    else PN_TRY(linear<LIN_RELU>("mlp input_proj", static_cast<const float *>(feat), F, 0, w, b, nullptr, nullptr, A.X, B, F, Hd, st));
    for (int k = 0; k < net.nb; ++k) {
        const float *w1 = p, *b1 = w1 + (size_t)Hd * Hd, *w2 = b1 + Hd, *b2 = w2 + (size_t)Hd * Hd;
        p = b2 + Hd;
        PN_TRY(linear<LIN_RELU>("mlp block.0", A.X, Hd, 0, w1, b1, nullptr, nullptr, A.T, B, Hd, Hd, st));
        PN_TRY(linear<LIN_RES_RELU>("mlp block.3", A.T, Hd, 0, w2, b2, nullptr, A.X, A.Y, B, Hd, Hd, st));
        std::swap(A.X, A.Y);
    }
    PN_TRY(linear<LIN_RELU>("mlp output_proj", A.X, Hd, 0, p, p + (size_t)half * Hd, nullptr, nullptr, A.half, B, Hd, half, st));
    PN_TRY(linear<LIN_GATED_RANGE>("mlp heads", A.half, half, 0, net.hw, net.hb, nullptr, nullptr, out, B, half, 4, st));
    return UWIE_OK;
}

}  // namespace uwie
