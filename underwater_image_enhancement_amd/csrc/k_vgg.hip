// PerceptualLoss (vgg_16_UIE.py:257-269): mse_loss(F(pred), F(target)) with F = torchvision vgg16().features[:16], the
// trunk up to relu3_3.  Activations are channels-last ([B][H][W][C]) inside the caller's workspace,
// in the route's element type T: float (the float32 contract) or _Float16 (torch.autocast's float16 contract: every conv
// accumulates in float32 and rounds its output after the bias; ReLU and max-pool run on the rounded values).
//
//   k_vgg_conv0<T>        conv1_1 (3 -> 64, K = 27) + ReLU, direct: NCHW float32 input, too narrow for MFMA tiles
//   k_vgg_conv<T, EPI>    conv1_2 ... conv3_3 and their data-gradients as one implicit GEMM: M = output pixels, N = output
//                         channels, K = 9 * C_in in (tap, channel) order; 64 x 64 tiles, 4 waves of 2 x 2 MFMA tiles
//                         (v_mfma_f32_16x16x4_f32 / v_mfma_f32_16x16x32_f16), A and B staged in LDS.  Epilogues:
//                         EPI_RELU  bias + ReLU
//                         EPI_POOL  bias + ReLU + the 2 x 2 max-pool: M runs over pool windows (4 consecutive rows = one
//                                   window in row-major order), so each lane holds a whole window of its channel
//                         EPI_MASK  data-gradient: threshold_backward against a saved activation
//                         EPI_MSE   the last forward layer on pred: d = f - t against the target's relu3_3, per-block
//                                   float64 sums of d*d, and the ReLU-masked d; f itself is never written
//   k_vgg_unpool<T>       max-pool backward as a gather (every element of the pre-pool grid written once)
//   k_vgg_seed<T>         dL/dF = ((2/N) d) g with g = dL/dloss read on the device
//   k_vgg_conv0_bwd<T>    conv1_1's data-gradient (C_out = 3), direct, float32 NCHW output
//   k_vgg_loss_finish     the loss: the block sums added in a fixed order, one rounding (no atomics)
#include "common.h"

namespace uwie {

namespace {

#define VGG_TRY(call)                     \
    do {                                  \
        const int _rc = (call);           \
        if (_rc != UWIE_OK) return _rc;   \
    } while (0)

// a launch timed under the layer's name (uwie_profile_*: per-conv times, profiles/perceptual_bench.py --layers)
#define VGG_LAUNCH(name, kernel, grid, block, st, ...)                 \
    do {                                                               \
        UWIE_PROF(name, st);                                           \
        hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);   \
    } while (0)

constexpr int kTile = 64;      // BM = BN = 64
constexpr int kRowBytes = 80;  // one LDS row: 64 bytes of K slice + 16 bytes of padding
enum { EPI_RELU = 0, EPI_POOL = 1, EPI_MASK = 2, EPI_MSE = 3 };

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T>
struct VggElem;
template <>
struct VggElem<float> {
    static constexpr int BK = 16;  // 64 bytes of K per step
};
template <>
struct VggElem<_Float16> {
    static constexpr int BK = 32;
};

// torch's relu (clamp_min): NaN stays NaN
template <typename T>
__device__ __forceinline__ T relu_t(T v)
{
    return v <= T(0) ? T(0) : v;
}

struct ConvArgs {
    const void *x;      // input [B][H][W][Cin] (T)
    const void *w;      // [Cout][9][Cin] (T)
    const float *bias;  // [Cout] (forward epilogues)
    void *y;            // output [M][Cout] (EPI_POOL: [B][H/2][W/2][Cout])
    uint8_t *idx;       // EPI_POOL: window position of each maximum (NULL: not kept)
    const void *aux;    // EPI_MASK: the saved activation [M][Cout]; EPI_MSE: the target's relu3_3 [M][Cout]
    float *diff;        // EPI_MSE: masked d [M][Cout]
    double *part;       // EPI_MSE: one float64 sum per block
    int B, H, W, Cin, Cout, M;
};

template <typename T, int EPI>
__global__ void __launch_bounds__(256) k_vgg_conv(ConvArgs a)
{
    constexpr int BK = VggElem<T>::BK, E = 16 / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) char As[kTile * kRowBytes];
    __shared__ __attribute__((aligned(16))) char Bs[kTile * kRowBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.x * kTile, n0 = blockIdx.y * kTile;
    const int K = 9 * a.Cin, cb = a.Cin / BK, steps = 9 * cb;
    // this thread's staging row (a pixel of A, an output channel of B) and 16-byte part of the K slice
    const int row = tid >> 2, part = tid & 3;
    const int m = m0 + row;
    int b = 0, y = 0, x = 0;
    const bool mv = m < a.M;
    if (mv) {
        if (EPI == EPI_POOL) {
            const int PW = a.W >> 1, PH = a.H >> 1, q = m >> 2, w4 = m & 3;
            const int px = q % PW, t = q / PW;
            y = 2 * (t % PH) + (w4 >> 1);
            x = 2 * px + (w4 & 1);
            b = t / PH;
        } else {
            x = m % a.W;
            const int t = m / a.W;
            y = t % a.H;
            b = t / a.H;
        }
    }
    const T *X = static_cast<const T *>(a.x);
    const T *Wt = static_cast<const T *>(a.w) + (size_t)(n0 + row) * K + part * E;
    auto load = [&](int s, uint4 &ra, uint4 &rb) {
        const int tap = s / cb, c0 = (s - tap * cb) * BK;
        const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
        ra = make_uint4(0, 0, 0, 0);
        if (mv && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
            ra = *reinterpret_cast<const uint4 *>(X + ((size_t)(b * a.H + iy) * a.W + ix) * a.Cin + c0 + part * E);
        rb = *reinterpret_cast<const uint4 *>(Wt + tap * a.Cin + c0);
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    uint4 ra, rb;
    load(0, ra, rb);
    const int ar = (wm * 32 + (lane & 15)) * kRowBytes, br = (wn * 32 + (lane & 15)) * kRowBytes;
    for (int s = 0; s < steps; ++s) {
        __syncthreads();
        *reinterpret_cast<uint4 *>(As + row * kRowBytes + part * 16) = ra;
        *reinterpret_cast<uint4 *>(Bs + row * kRowBytes + part * 16) = rb;
        __syncthreads();
        if (s + 1 < steps) load(s + 1, ra, rb);
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ko = (kk * 4 + (lane >> 4)) * 4;
                float av[2], bv[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    av[i] = *reinterpret_cast<const float *>(As + ar + i * 16 * kRowBytes + ko);
                    bv[i] = *reinterpret_cast<const float *>(Bs + br + i * 16 * kRowBytes + ko);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            }
        } else {
            const int ko = (lane >> 4) * 16;
            f16x8 av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                av[i] = *reinterpret_cast<const f16x8 *>(As + ar + i * 16 * kRowBytes + ko);
                bv[i] = *reinterpret_cast<const f16x8 *>(Bs + br + i * 16 * kRowBytes + ko);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    // C/D: lane holds rows 4 (lane >> 4) + v of each 16 x 16 tile, column lane & 15
    T *Y = static_cast<T *>(a.y);
    double sq = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r0 = m0 + wm * 32 + i * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 32 + j * 16 + (lane & 15);
            if constexpr (EPI == EPI_POOL) {
                if (r0 >= a.M) continue;
                const float bn = a.bias[n];
                // max_pool2d_with_indices (CPU): the first maximum in row-major window order; a NaN replaces the maximum
                float best = -__builtin_inff();
                int arg = 0;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float f = (float)relu_t((T)(acc[i][j][v] + bn));
                    if (f > best || f != f) {
                        best = f;
                        arg = v;
                    }
                }
                const size_t o = (size_t)(r0 >> 2) * a.Cout + n;
                Y[o] = (T)best;
                if (a.idx) a.idx[o] = (uint8_t)arg;
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = r0 + v;
                    if (r >= a.M) continue;
                    const size_t o = (size_t)r * a.Cout + n;
                    if constexpr (EPI == EPI_RELU) {
                        Y[o] = relu_t((T)(acc[i][j][v] + a.bias[n]));
                    } else if constexpr (EPI == EPI_MASK) {
                        const T s = static_cast<const T *>(a.aux)[o];
                        Y[o] = s <= T(0) ? T(0) : (T)acc[i][j][v];  // threshold_backward
                    } else {
                        const T f = relu_t((T)(acc[i][j][v] + a.bias[n]));
                        const float d = (float)f - (float)static_cast<const T *>(a.aux)[o];
                        sq += (double)(d * d);
                        a.diff[o] = f <= T(0) ? 0.0f : d;
                    }
                }
            }
        }
    }
    if constexpr (EPI == EPI_MSE) {
        __shared__ double red[256];
        red[tid] = sq;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int k = 0; k < 256; ++k) t += red[k];
            a.part[blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
    }
}

// conv1_1 + ReLU: one thread per pixel, all 64 channels; weights [64][3][3][3] float32 (already rounded to T's values)
template <typename T>
__global__ void __launch_bounds__(256) k_vgg_conv0(const float *__restrict__ img, int B, int H, int W, const float *__restrict__ w,
                                                   const float *__restrict__ bias, T *__restrict__ y)
{
    __shared__ float ws[64 * 27], bs[64];
    for (int i = threadIdx.x; i < 64 * 27; i += 256) ws[i] = w[i];
    if (threadIdx.x < 64) bs[threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)B * H * W) return;
    const int x = (int)(p % W), yy = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
    float in[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int iy = yy + t / 3 - 1, ix = x + t % 3 - 1;
            const float v = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? img[((size_t)(b * 3 + c) * H + iy) * W + ix] : 0.0f;
            in[c * 9 + t] = (float)(T)v;
        }
    T *o = y + p * 64;
    for (int c0 = 0; c0 < 64; c0 += 16 / (int)sizeof(T)) {
        constexpr int E = 16 / (int)sizeof(T);
        union {
            uint4 u;
            T v[E];
        } pk;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 27; ++k) s = fmaf(ws[(c0 + e) * 27 + k], in[k], s);
            pk.v[e] = relu_t((T)(s + bs[c0 + e]));
        }
        *reinterpret_cast<uint4 *>(o + c0) = pk.u;
    }
}

// conv1_1's data-gradient: gx[b][c][y][x] = sum over taps and 64 channels of w[co][c][ky][kx] g[y - ky + 1][x - kx + 1][co]
template <typename T>
__global__ void __launch_bounds__(256) k_vgg_conv0_bwd(const T *__restrict__ g, int B, int H, int W, const float *__restrict__ w,
                                                       float *__restrict__ gx)
{
    __shared__ float ws[64 * 27];
    for (int i = threadIdx.x; i < 64 * 27; i += 256) ws[i] = w[i];
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)B * H * W) return;
    const int x = (int)(p % W), yy = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
    constexpr int E = 16 / (int)sizeof(T);
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (int t = 0; t < 9; ++t) {
        const int sy = yy - t / 3 + 1, sx = x - t % 3 + 1;
        if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
        const T *gp = g + ((size_t)(b * H + sy) * W + sx) * 64;
        for (int c0 = 0; c0 < 64; c0 += E) {
            union {
                uint4 u;
                T v[E];
            } pk;
            pk.u = *reinterpret_cast<const uint4 *>(gp + c0);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const float gv = (float)pk.v[e];
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] = fmaf(ws[(c0 + e) * 27 + c * 9 + t], gv, s[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) gx[((size_t)(b * 3 + c) * H + yy) * W + x] = (float)(T)s[c];
}

// max-pool backward: g[b][y][x][c] = gp of the window when (y, x) is its saved maximum, else 0 (also the floored edge)
template <typename T>
__global__ void __launch_bounds__(256) k_vgg_unpool(const T *__restrict__ gp, const uint8_t *__restrict__ idx, int B, int H, int W,
                                                    int C, T *__restrict__ g)
{
    const size_t n = (size_t)B * H * W * C;
    const int PH = H >> 1, PW = W >> 1;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const size_t pix = i / C;
        const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((size_t)W * H));
        const int py = y >> 1, px = x >> 1;
        T v = T(0);
        if (py < PH && px < PW) {
            const size_t j = ((size_t)(b * PH + py) * PW + px) * C + c;
            if (idx[j] == (y & 1) * 2 + (x & 1)) v = gp[j];
        }
        g[i] = v;
    }
}

// MseLossBackward0: (norm * d) * g, rounded to T (autocast: the backward of the float32 cast)
template <typename T>
__global__ void __launch_bounds__(256) k_vgg_seed(const float *__restrict__ dm, size_t n, float norm, const float *__restrict__ gl,
                                                  T *__restrict__ g)
{
    const float gv = gl[0];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) g[i] = (T)((norm * dm[i]) * gv);
}

__global__ void __launch_bounds__(256) k_vgg_loss_finish(const double *__restrict__ part, int n, double count, float *__restrict__ loss)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t += red[k];
        loss[0] = (float)(t / count);
    }
}

// torchvision's [Cout][Cin][3][3] weights -> wf [Cout][tap][Cin] and the data-gradient's wb [Cin][tap'][Cout] with
// tap' = 8 - tap (180-degree rotation), both rounded to T; bias rounded to T's values in float32
template <typename T>
__global__ void __launch_bounds__(256) k_vgg_pack(const float *__restrict__ src, int Cout, int Cin, T *__restrict__ wf,
                                                  T *__restrict__ wb, float *__restrict__ bias)
{
    const int n = Cout * Cin * 9;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n + Cout; i += gridDim.x * 256) {
        if (i >= n) {
            bias[i - n] = (float)(T)src[i];
            continue;
        }
        const int t = i % 9, ci = (i / 9) % Cin, co = i / (9 * Cin);
        const T v = (T)src[i];
        if (wf) {
            wf[((size_t)co * 9 + t) * Cin + ci] = v;
            wb[((size_t)ci * 9 + (8 - t)) * Cout + co] = v;
        } else {
            reinterpret_cast<float *>(wb)[i] = (float)v;  // conv1_1: the source layout, in float32
        }
    }
}

constexpr int kCin[7] = {3, 64, 64, 128, 128, 256, 256};
const char *const kFwdName[7] = {"vgg conv1_1", "vgg conv1_2", "vgg conv2_1", "vgg conv2_2", "vgg conv3_1", "vgg conv3_2", "vgg conv3_3"};
const char *const kBwdName[7] = {"vgg conv1_1 bwd", "vgg conv1_2 bwd", "vgg conv2_1 bwd", "vgg conv2_2 bwd", "vgg conv3_1 bwd",
                                 "vgg conv3_2 bwd", "vgg conv3_3 bwd"};
constexpr int kCout[7] = {64, 64, 128, 128, 256, 256, 256};

struct Acts {  // one call's buffers (see perceptual_carve)
    void *a1, *p1, *a3, *p2, *a5, *a6, *X, *Y;
    uint8_t *i1, *i2;
    float *dm;
    double *part;
};

template <typename T>
Acts carve(Shape s, void *ws, size_t *total = nullptr)
{
    const size_t P1 = (size_t)s.B * s.H * s.W, P2 = (size_t)s.B * (s.H / 2) * (s.W / 2), P3 = (size_t)s.B * (s.H / 4) * (s.W / 4);
    Carver c(ws);
    Acts A;
    // kept by the forward on pred for the backward
    A.a1 = c.take<T>(P1 * 64);
    A.p1 = c.take<T>(P2 * 64);
    A.i1 = c.take<uint8_t>(P2 * 64);
    A.a3 = c.take<T>(P2 * 128);
    A.p2 = c.take<T>(P3 * 128);
    A.i2 = c.take<uint8_t>(P3 * 128);
    A.a5 = c.take<T>(P3 * 256);
    A.a6 = c.take<T>(P3 * 256);
    A.dm = c.take<float>(P3 * 256);
    A.part = c.take<double>((size_t)cdiv((long long)P3, kTile) * 4);
    // scratch: the forward on target, then the backward's gradients
    A.X = c.take<T>(P1 * 64);
    A.Y = c.take<T>(P1 * 64);
    if (total) *total = c.total();
    return A;
}

template <typename T, int EPI>
int conv(const VggNet &net, int l, bool bwd, const void *x, void *y, int B, int H, int W, hipStream_t st, const void *aux = nullptr,
         uint8_t *idx = nullptr, float *diff = nullptr, double *part = nullptr)
{
    ConvArgs a;
    a.x = x;
    a.w = bwd ? net.wb[l] : net.wf[l];
    a.bias = net.bias[l];
    a.y = y;
    a.idx = idx;
    a.aux = aux;
    a.diff = diff;
    a.part = part;
    a.B = B;
    a.H = H;
    a.W = W;
    a.Cin = bwd ? kCout[l] : kCin[l];
    a.Cout = bwd ? kCin[l] : kCout[l];
    a.M = EPI == EPI_POOL ? B * (H / 2) * (W / 2) * 4 : B * H * W;
    const dim3 grid(cdiv(a.M, kTile), a.Cout / kTile);
    VGG_LAUNCH(bwd ? kBwdName[l] : kFwdName[l], (k_vgg_conv<T, EPI>), grid, dim3(256), st, a);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

// F(img) up to relu3_2 (into the kept buffers, or the X / Y ping-pong when !keep); returns relu3_2's buffer
template <typename T>
int trunk(const VggNet &net, const float *img, Shape s, const Acts &A, bool keep, const void **a6, hipStream_t st)
{
    const int B = s.B, H = s.H, W = s.W, H2 = H / 2, W2 = W / 2, H3 = H2 / 2, W3 = W2 / 2;
    void *a1 = keep ? A.a1 : A.X, *p1 = keep ? A.p1 : A.Y, *a3 = keep ? A.a3 : A.X, *p2 = keep ? A.p2 : A.Y;
    void *a5 = keep ? A.a5 : A.X, *a6v = keep ? A.a6 : A.Y;
    VGG_LAUNCH(kFwdName[0], k_vgg_conv0<T>, dim3(cdiv((long long)B * H * W, 256)), dim3(256), st, img, B, H, W, net.w0, net.bias[0],
               static_cast<T *>(a1));
    UWIE_LAUNCH_CHECK();
    VGG_TRY((conv<T, EPI_POOL>(net, 1, false, a1, p1, B, H, W, st, nullptr, keep ? A.i1 : nullptr)));
    VGG_TRY((conv<T, EPI_RELU>(net, 2, false, p1, a3, B, H2, W2, st)));
    VGG_TRY((conv<T, EPI_POOL>(net, 3, false, a3, p2, B, H2, W2, st, nullptr, keep ? A.i2 : nullptr)));
    VGG_TRY((conv<T, EPI_RELU>(net, 4, false, p2, a5, B, H3, W3, st)));
    VGG_TRY((conv<T, EPI_RELU>(net, 5, false, a5, a6v, B, H3, W3, st)));
    *a6 = a6v;
    return UWIE_OK;
}

template <typename T>
int perceptual(const VggNet &net, const float *pred, const float *target, Shape s, float *loss, void *ws, hipStream_t st)
{
    const Acts A = carve<T>(s, ws);
    const int B = s.B, H3 = s.H / 4, W3 = s.W / 4;
    const void *a6;
    VGG_TRY(trunk<T>(net, target, s, A, false, &a6, st));
    VGG_TRY((conv<T, EPI_RELU>(net, 6, false, a6, A.X, B, H3, W3, st)));  // the target's relu3_3 (X: free from here on)
    VGG_TRY(trunk<T>(net, pred, s, A, true, &a6, st));
    VGG_TRY((conv<T, EPI_MSE>(net, 6, false, a6, nullptr, B, H3, W3, st, A.X, nullptr, A.dm, A.part)));
    const int nblk = cdiv((long long)B * H3 * W3, kTile) * 4;
    UWIE_LAUNCH(k_vgg_loss_finish, dim3(1), dim3(256), 0, st, A.part, nblk, (double)B * H3 * W3 * 256, loss);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

template <typename T>
int perceptual_bwd(const VggNet &net, Shape s, const float *grad_loss, float *grad_pred, void *ws, hipStream_t st)
{
    const Acts A = carve<T>(s, ws);
    const int B = s.B, H = s.H, W = s.W, H2 = H / 2, W2 = W / 2, H3 = H2 / 2, W3 = W2 / 2;
    const size_t n3 = (size_t)B * H3 * W3 * 256;
    UWIE_LAUNCH(k_vgg_seed<T>, dim3(grid_for(n3)), dim3(256), 0, st, A.dm, n3, (float)(2.0 / (double)n3), grad_loss,
                static_cast<T *>(A.X));
    UWIE_LAUNCH_CHECK();
    VGG_TRY((conv<T, EPI_MASK>(net, 6, true, A.X, A.Y, B, H3, W3, st, A.a6)));
    VGG_TRY((conv<T, EPI_MASK>(net, 5, true, A.Y, A.X, B, H3, W3, st, A.a5)));
    VGG_TRY((conv<T, EPI_MASK>(net, 4, true, A.X, A.Y, B, H3, W3, st, A.p2)));
    const size_t n2 = (size_t)B * H2 * W2 * 128;
    UWIE_LAUNCH(k_vgg_unpool<T>, dim3(grid_for(n2)), dim3(256), 0, st, static_cast<const T *>(A.Y), A.i2, B, H2, W2, 128,
                static_cast<T *>(A.X));
    UWIE_LAUNCH_CHECK();
    VGG_TRY((conv<T, EPI_MASK>(net, 3, true, A.X, A.Y, B, H2, W2, st, A.a3)));
    VGG_TRY((conv<T, EPI_MASK>(net, 2, true, A.Y, A.X, B, H2, W2, st, A.p1)));
    const size_t n1 = (size_t)B * H * W * 64;
    UWIE_LAUNCH(k_vgg_unpool<T>, dim3(grid_for(n1)), dim3(256), 0, st, static_cast<const T *>(A.X), A.i1, B, H, W, 64,
                static_cast<T *>(A.Y));
    UWIE_LAUNCH_CHECK();
    VGG_TRY((conv<T, EPI_MASK>(net, 1, true, A.Y, A.X, B, H, W, st, A.a1)));
    VGG_LAUNCH(kBwdName[0], k_vgg_conv0_bwd<T>, dim3(cdiv((long long)B * H * W, 256)), dim3(256), st, static_cast<const T *>(A.X), B,
               H, W, net.w0, grad_pred);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

template <typename T>
size_t pack_bytes()
{
    Carver c(nullptr);
    c.take<float>(64 * 27);
    for (int l = 0; l < 7; ++l) {
        if (l) {
            c.take<T>((size_t)kCout[l] * 9 * kCin[l]);
            c.take<T>((size_t)kCout[l] * 9 * kCin[l]);
        }
        c.take<float>(kCout[l]);
    }
    return c.total();
}

template <typename T>
int pack(const float *d_params, void *blob, VggNet *net, hipStream_t st)
{
    Carver c(blob);
    float *w0 = c.take<float>(64 * 27);
    net->w0 = w0;
    const float *src = d_params;
    for (int l = 0; l < 7; ++l) {
        T *wf = nullptr, *wb = nullptr;
        const size_t nw = (size_t)kCout[l] * 9 * kCin[l];
        if (l) {
            wf = c.take<T>(nw);
            wb = c.take<T>(nw);
        }
        float *bias = c.take<float>(kCout[l]);
        net->wf[l] = wf;
        net->wb[l] = wb;
        net->bias[l] = bias;
        UWIE_LAUNCH(k_vgg_pack<T>, dim3(grid_for(nw + kCout[l], 1024)), dim3(256), 0, st, src, kCout[l], kCin[l], wf,
                    l ? wb : reinterpret_cast<T *>(w0), bias);
        UWIE_LAUNCH_CHECK();
        src += nw + kCout[l];
    }
    return UWIE_OK;
}

}  // namespace

size_t vgg_param_count()
{
    size_t n = 0;
    for (int l = 0; l < 7; ++l) n += (size_t)kCout[l] * 9 * kCin[l] + kCout[l];
    return n;
}

size_t vgg_blob_bytes(int precision) { return precision == UWIE_VGG_F16 ? pack_bytes<_Float16>() : pack_bytes<float>(); }

int vgg_pack(const float *d_params, int precision, void *blob, VggNet *net, hipStream_t st)
{
    net->precision = precision;
    return precision == UWIE_VGG_F16 ? pack<_Float16>(d_params, blob, net, st) : pack<float>(d_params, blob, net, st);
}

size_t perceptual_ws_bytes(Shape s, int precision)
{
    size_t n = 0;
    if (precision == UWIE_VGG_F16) (void)carve<_Float16>(s, nullptr, &n);
    else (void)carve<float>(s, nullptr, &n);
    return n;
}

int launch_perceptual(const VggNet &net, const float *d_pred, const float *d_target, Shape s, float *d_loss, void *ws, hipStream_t st)
{
    return net.precision == UWIE_VGG_F16 ? perceptual<_Float16>(net, d_pred, d_target, s, d_loss, ws, st)
                                         : perceptual<float>(net, d_pred, d_target, s, d_loss, ws, st);
}

int launch_perceptual_bwd(const VggNet &net, Shape s, const float *d_grad_loss, float *d_grad_pred, void *ws, hipStream_t st)
{
    return net.precision == UWIE_VGG_F16 ? perceptual_bwd<_Float16>(net, s, d_grad_loss, d_grad_pred, ws, st)
                                         : perceptual_bwd<float>(net, s, d_grad_loss, d_grad_pred, ws, st);
}

// ---------------------------------------------------------------- ImprovedVGGParameterNet's trunk
int vgg_pack_conv_f32(const float *src, int Cout, int Cin, float *wf, float *wb_scratch, float *bias, hipStream_t st)
{
    const size_t nw = (size_t)Cout * 9 * Cin;
    UWIE_LAUNCH(k_vgg_pack<float>, dim3(grid_for(nw + Cout, 1024)), dim3(256), 0, st, src, Cout, Cin, wf, wb_scratch, bias);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

int launch_param_trunk(const VggNet &net, const float *const wf4[3], const float *const bias4[3], const float *img, Shape s, float *X,
                       float *Y, float **relu43, hipStream_t st)
{
    static const char *const name4[3] = {"vgg conv4_1", "vgg conv4_2", "vgg conv4_3"};
    const int B = s.B, H3 = s.H / 4, W3 = s.W / 4, H4 = H3 / 2, W4 = W3 / 2;
    Acts A{};
    A.X = X;
    A.Y = Y;
    const void *a6;  // relu3_2, in Y
    VGG_TRY(trunk<float>(net, img, s, A, false, &a6, st));
    VGG_TRY((conv<float, EPI_POOL>(net, 6, false, a6, X, B, H3, W3, st)));  // conv3_3 + relu3_3 + pool3 (no indices)
    float *in = X, *out = Y;
    for (int l = 0; l < 3; ++l) {
        ConvArgs a{};
        a.x = in;
        a.w = wf4[l];
        a.bias = bias4[l];
        a.y = out;
        a.B = B;
        a.H = H4;
        a.W = W4;
        a.Cin = l ? 512 : 256;
        a.Cout = 512;
        a.M = B * H4 * W4;
        VGG_LAUNCH(name4[l], (k_vgg_conv<float, EPI_RELU>), dim3(cdiv(a.M, kTile), a.Cout / kTile), dim3(256), st, a);
        UWIE_LAUNCH_CHECK();
        float *t = in;
        in = out;
        out = t;
    }
    *relu43 = in;
    return UWIE_OK;
}

}  // namespace uwie
