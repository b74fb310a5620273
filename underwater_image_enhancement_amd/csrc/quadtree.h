// One step of estimate_atmospheric_light's quadtree (six_stadigy.py:49-157), stated once for the byte route (k_airlight.hip)
// and the float-image route (k_float.hip): the quadrant split and the greedy descent, compute_Q's score and its argmax, the
// trace record, and NumPy's pairwise leaf sum over an element accessor (Elem<VAR> for bytes, ElemF<T, VAR> for floats).
#pragma once
#include "common.h"
#include "devutil.h"
#include "pairwise_tree.h"

namespace uwie {

constexpr int kMaxLevels = 32;

struct TraceRec {  // matches the layout documented in uwie.h
    int32_t y0, x0, rows, cols;
    double score[4];
};

// chunk sums a quadrant of the first level needs (the largest any level has)
inline int max_chunks(Shape s) { return cdiv((long long)((s.H + 1) / 2) * ((s.W + 1) / 2), kNpChunk); }

// ---- the split
__device__ __forceinline__ bool quad_is_leaf(const Region &k, int min_size) { return k.rows <= min_size || k.cols <= min_size; }  // six_stadigy.py:76
// quadrant j of block k of image b: 0 top left, 1 top right, 2 bottom left, 3 bottom right
__device__ __forceinline__ Region quad_region(int b, const Region &k, int j)
{
    const int mr = k.rows / 2, mc = k.cols / 2;  // six_stadigy.py:85-86
    return j == 0   ? Region{b, k.y0, k.x0, mr, mc}
           : j == 1 ? Region{b, k.y0, k.x0 + mc, mr, k.cols - mc}
           : j == 2 ? Region{b, k.y0 + mr, k.x0, k.rows - mr, mc}
                    : Region{b, k.y0 + mr, k.x0 + mc, k.rows - mr, k.cols - mc};
}
// regs[4 b ..] = the four quadrants of k, inactive (rows == 0) when k is a leaf
__device__ __forceinline__ void quad_split(Region *__restrict__ regs, int b, const Region &k, int min_size)
{
    const bool leaf = quad_is_leaf(k, min_size);
    for (int j = 0; j < 4; ++j) {
        Region q = quad_region(b, k, j);
        if (leaf) q.rows = q.cols = 0;
        regs[b * 4 + j] = q;
    }
}
// The greedy step (six_stadigy.py:100-111): quadrant `arg` becomes the block, its quadrants the next level's regions with
// zeroed edge counters.  One lane.
__device__ __forceinline__ void q_descend(Region *__restrict__ blk, Region *__restrict__ regs, uint32_t *__restrict__ edges, int b, int arg,
                                          int min_size)
{
    const Region k = regs[b * 4 + arg];
    blk[b] = k;
    quad_split(regs, b, k, min_size);
    for (int j = 0; j < 4; ++j) edges[b * 4 + j] = 0;
}

// ---- compute_Q's final arithmetic (six_stadigy.py:134-155) in the image's dtype T, every operation rounding once in this
// order: S = the three channel sums, V = the sums of squared deviations, n = pixels, edges = Canny edge pixels
template <class T>
__device__ __forceinline__ double quad_score(const T *S, const T *V, long long n, uint32_t edges)
{
    const T t1 = ((S[0] + S[1]) + S[2]) / (T)(3 * n);
    const T t2 = ((S[2] + S[1]) - (T)2 * S[0]) / (T)n;
    const T v0 = V[0] / (T)n, v1 = V[1] / (T)n, v2 = V[2] / (T)n;
    const T t3 = ((v0 + v1) + v2) / (T)3;
    const double t4 = (double)edges / (double)n;  // int64 / int -> float64
    return (double)((t1 + t2) - t3) - t4;
}
// np.argmax: first maximum
__device__ __forceinline__ int quad_argmax(const double (&score)[4])
{
    int arg = 0;
    for (int q = 1; q < 4; ++q)
        if (score[q] > score[arg]) arg = q;
    return arg;
}
__device__ __forceinline__ void trace_store(TraceRec *__restrict__ trace, int b, int level, const Region &k, const double (&score)[4])
{
    TraceRec &t = trace[b * kMaxLevels + level];
    t.y0 = k.y0; t.x0 = k.x0; t.rows = k.rows; t.cols = k.cols;
    for (int q = 0; q < 4; ++q) t.score[q] = score[q];
}

// ---- leaf sums
// Level 0 of the byte route only (GRAY): the sums pass visits every pixel of the frame exactly once with its normalised,
// colour-corrected value in hand, so it also writes the 8-bit gray plane -- gray = cvtColor((x*255).astype(u8), RGB2GRAY),
// six_stadigy.py:149,177 -- instead of a separate sweep over the frame (k_quant_gray: 1.6 GB read again at 4K x 64).
struct GrayOut {
    uint8_t *plane;  // gray plane of the image (nullptr: none)
    int shift;       // RGB2GRAY fixed point (15 or 14)
};
__device__ __forceinline__ uint32_t gray_of(float v0, float v1, float v2, int shift)
{
    return gray_fixed(quant_u8(v0), quant_u8(v1), quant_u8(v2), shift);
}

// NumPy's pairwise_sum on a block of n <= 128 elements starting at raster element e0 of region r, three channels at once.
// EL: the element accessor -- src_t (what the image holds), val_t (what is summed), img, W, get(p, c) = the value of channel
// c of the pixel at p.
template <class EL, bool GRAY = false>
__device__ void leaf_sum3(const EL &el, const Region &r, int e0, int n, typename EL::val_t out[3], GrayOut go = GrayOut{nullptr, 15})
{
    using V = typename EL::val_t;
    static_assert(!(EL::kVar && GRAY), "the gray plane rides with the plain sums");
    int ly = e0 / r.cols, lx = e0 % r.cols;
    const typename EL::src_t *p = el.img + ((size_t)(r.y0 + ly) * el.W + r.x0 + lx) * 3;
    uint8_t *gp = GRAY ? go.plane + (size_t)(r.y0 + ly) * el.W + r.x0 + lx : nullptr;
    auto step = [&]() {
        ++lx;
        p += 3;
        if (GRAY) ++gp;
        if (lx == r.cols) {
            lx = 0;
            p += (size_t)(el.W - r.cols) * 3;
            if (GRAY) gp += el.W - r.cols;
        }
    };
    // the three values of the pixel at p (and its gray byte on the way)
    auto px3 = [&](V &v0, V &v1, V &v2) {
        v0 = el.get(p, 0);
        v1 = el.get(p, 1);
        v2 = el.get(p, 2);
        if constexpr (GRAY) *gp = (uint8_t)gray_of(v0, v1, v2, go.shift);
    };
    if (n < 8) {
        V a0 = 0, a1 = 0, a2 = 0;
        for (int i = 0; i < n; ++i) {
            V v0, v1, v2;
            px3(v0, v1, v2);
            a0 += v0;
            a1 += v1;
            a2 += v2;
            step();
        }
        out[0] = a0; out[1] = a1; out[2] = a2;
        return;
    }
    V acc[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        px3(acc[0][j], acc[1][j], acc[2][j]);
        step();
    }
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            V v0, v1, v2;
            px3(v0, v1, v2);
            acc[0][j] += v0;
            acc[1][j] += v1;
            acc[2][j] += v2;
            step();
        }
    }
    V res[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) res[c] = tree8<V>(acc[c]);
    for (; i < n; ++i) {
        V v0, v1, v2;
        px3(v0, v1, v2);
        res[0] += v0;
        res[1] += v1;
        res[2] += v2;
        step();
    }
    out[0] = res[0]; out[1] = res[1]; out[2] = res[2];
}

}  // namespace uwie
