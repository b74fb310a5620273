// Gray-world white balance with red-channel compensation for u8 frames (include/uwie.h uwie_gray_world_u8 states the contract;
// Ancuti et al. 2018 eq. 4-5, then Buchsbaum's gray world, in byte units).  Every statistic is an exact integer sum over the
// frame's bytes and every float64 step a single IEEE operation in the contract's order (-ffp-contract=off), so the bytes and
// the twelve stats are those of the NumPy restatement (tests/gray_world_ref.py), bit for bit.
//   k_gw_sums    one pass over the frame's bytes, 3 B/px read: a workgroup takes kGwBlockPx consecutive pixels of one frame in
//                groups of 16 (three 16-byte loads) and leaves one row of five 32-bit sums: S_r, S_g, S_b, S_rg, S_bg
//   k_gw_coeffs  one wavefront per frame: the rows added as 64-bit integers (any order gives the same integer), then the
//                contract's dozen float64 operations; the twelve stats go to the workspace and, if asked for, to d_stats
//   k_gw_apply   3 B/px read, 3 B/px written: 16 pixels per thread (three 16-byte loads, three 16-byte stores); green is a
//                function of one byte and comes from a 256-entry table in LDS, red and blue are evaluated in float64 as the
//                contract writes them.  A thread reads its 48 bytes before it writes them and no other thread touches them,
//                so d_out == d_in is allowed.
// Determinism: integer sums only, no atomics; the grids depend on H and W alone, so a frame's stats and bytes are the same in
// every run and at every position of every batch.  A frame inside a batch starts at b * 3 * n bytes, aligned or not: the
// 16-byte accesses go through load16 / store16 (gfx950 takes unaligned addresses), the last n % 16 pixels byte by byte.
#include <algorithm>

#include "common.h"
#include "devutil.h"

namespace uwie {

namespace {

constexpr int kGwGroupPx = 16;    // pixels per thread and step of both passes: 48 bytes = three 16-byte accesses
// Pixels per workgroup of the sum pass (256 threads x 4 groups).  A workgroup's five sums are 32-bit from the thread to the
// row it writes: the largest is S_rg <= 255 * 255 * px = 65025 * px, and 65025 * px < 2^32 holds up to px = 66051.
constexpr int kGwBlockPx = 16384;
static_assert(65025ull * kGwBlockPx < (1ull << 32), "a workgroup's sum of r * g must fit 32 bits");
static_assert(kGwBlockPx % (256 * kGwGroupPx) == 0, "a workgroup's pixels are whole steps of 256 threads x 16 pixels");
constexpr int kGwRow = 8;  // words per row of partial sums (five used; 32-byte rows)

struct GwSums {
    uint32_t r, g, b, rg, bg;
    __device__ __forceinline__ void add(uint32_t pr, uint32_t pg, uint32_t pb)
    {
        r += pr; g += pg; b += pb;
        rg += pr * pg;
        bg += pb * pg;
    }
};

// byte k of twelve dwords holding 48 consecutive bytes
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&d)[12], int k) { return (d[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// grid (cdiv(n, kGwBlockPx), B), block 256.  part: [B][gridDim.x][kGwRow].
__global__ void __launch_bounds__(256) k_gw_sums(const uint8_t *__restrict__ in, int n, uint32_t *__restrict__ part)
{
    __shared__ uint32_t s_red[4][5];
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint8_t *img = in + (size_t)b * 3 * n;
    const int ngroups = n / kGwGroupPx;                       // whole groups of the frame
    const int g0 = blockIdx.x * (kGwBlockPx / kGwGroupPx);    // this workgroup's first group
    GwSums s{0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kGwBlockPx / (256 * kGwGroupPx); ++i) {
        const int g = g0 + i * 256 + tid;
        if (g < ngroups) {
            const uint8_t *p = img + (size_t)g * (3 * kGwGroupPx);
            const uint4 a0 = load16<uint4>(p), a1 = load16<uint4>(p + 16), a2 = load16<uint4>(p + 32);
            const uint32_t d[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
#pragma unroll
            for (int px = 0; px < kGwGroupPx; ++px) s.add(byte_of(d, 3 * px), byte_of(d, 3 * px + 1), byte_of(d, 3 * px + 2));
        }
    }
    if (blockIdx.x == gridDim.x - 1) {  // the frame's tail: fewer than 16 pixels, in the last workgroup's share
        const int px = ngroups * kGwGroupPx + tid;
        if (px < n) s.add(img[(size_t)px * 3], img[(size_t)px * 3 + 1], img[(size_t)px * 3 + 2]);
    }
    uint32_t v[5] = {s.r, s.g, s.b, s.rg, s.bg};
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = wave_sum_u32(v[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s_red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < kGwRow)
        part[((size_t)b * gridDim.x + blockIdx.x) * kGwRow + tid] = tid < 5 ? (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]) : 0u;
}

// The contract's coefficients from the five sums (all below 2^53: converted exactly); st: the UWIE_GW_STATS values.
__device__ __forceinline__ void gw_coeffs(uint64_t S_r, uint64_t S_g, uint64_t S_b, uint64_t S_rg, uint64_t S_bg, int n, double red, double blue,
                                          double max_gain, double (&st)[UWIE_GW_STATS])
{
    const double N = (double)n;
    const double mr = (double)S_r / N, mg = (double)S_g / N, mb = (double)S_b / N;
    const double dr = mg - mr, db = mg - mb;
    const double kr = (red * (dr > 0.0 ? dr : 0.0)) / 65025.0, kb = (blue * (db > 0.0 ? db : 0.0)) / 65025.0;
    const double cr = ((double)S_r + kr * (double)(255ull * S_g - S_rg)) / N;  // 255 * S_g >= S_rg: one exact integer
    const double cb = ((double)S_b + kb * (double)(255ull * S_g - S_bg)) / N;
    const double cg = mg;
    const double gray = ((cr + cg) + cb) / 3.0;
    double sr = cr > 0.0 ? gray / cr : 1.0, sg = cg > 0.0 ? gray / cg : 1.0, sb = cb > 0.0 ? gray / cb : 1.0;
    if (max_gain > 0.0) {
        sr = sr < max_gain ? sr : max_gain;
        sg = sg < max_gain ? sg : max_gain;
        sb = sb < max_gain ? sb : max_gain;
    }
    st[0] = mr; st[1] = mg; st[2] = mb; st[3] = kr; st[4] = kb; st[5] = cr; st[6] = cg; st[7] = cb; st[8] = gray;
    st[9] = sr; st[10] = sg; st[11] = sb;
}

// grid B, block 64.  stats: [B][UWIE_GW_STATS] in the workspace (k_gw_apply reads it); d_stats: the caller's, or nullptr.
__global__ void __launch_bounds__(64) k_gw_coeffs(const uint32_t *__restrict__ part, int nblk, int n, double red, double blue, double max_gain,
                                                  double *__restrict__ stats, double *__restrict__ d_stats)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    uint64_t s[5] = {0, 0, 0, 0, 0};
    for (int k = lane; k < nblk; k += 64) {
        const uint32_t *row = part + ((size_t)b * nblk + k) * kGwRow;
#pragma unroll
        for (int i = 0; i < 5; ++i) s[i] += row[i];
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) s[i] = wave_sum_u64(s[i]);
    double st[UWIE_GW_STATS];
    gw_coeffs(s[0], s[1], s[2], s[3], s[4], n, red, blue, max_gain, st);
    if (lane < UWIE_GW_STATS) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < UWIE_GW_STATS; ++i) v = lane == i ? st[i] : v;
        stats[(size_t)b * UWIE_GW_STATS + lane] = v;
        if (d_stats) d_stats[(size_t)b * UWIE_GW_STATS + lane] = v;
    }
}

// rint(min(w, 255)) of 0 <= w as a byte: adding 2^52 rounds w to an integer by the addition's own round-half-to-even, and leaves
// that integer in the low bits of the sum
__device__ __forceinline__ uint32_t gw_byte(double w)
{
    const double c = w < 255.0 ? w : 255.0;
    return (uint32_t)__double_as_longlong(c + 0x1p52) & 0xffu;
}
// w_r / w_b of the contract: s * c + cc * ((255 - c) * g), the product an integer, two multiplications and one addition
__device__ __forceinline__ uint32_t gw_comp(uint32_t c, uint32_t g, double s, double cc)
{
    return gw_byte(s * (double)c + cc * (double)((255u - c) * g));
}

// grid (gx, B), block 256; in and out may be the same pointer (no __restrict__ on them).
__global__ void __launch_bounds__(256) k_gw_apply(const uint8_t *in, int n, const double *__restrict__ stats, uint8_t *out)
{
    __shared__ uint8_t s_green[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const double *st = stats + (size_t)b * UWIE_GW_STATS;
    const double sr = st[9], sg = st[10], sb = st[11];
    const double cr = sr * st[3], cb = sb * st[4];
    s_green[tid] = (uint8_t)gw_byte(sg * (double)tid);
    __syncthreads();
    const size_t base = (size_t)b * 3 * n;
    const int ngroups = n / kGwGroupPx;
    for (int g = blockIdx.x * 256 + tid; g < ngroups; g += gridDim.x * 256) {
        const size_t off = base + (size_t)g * (3 * kGwGroupPx);
        const uint4 a0 = load16<uint4>(in + off), a1 = load16<uint4>(in + off + 16), a2 = load16<uint4>(in + off + 32);
        const uint32_t d[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        uint32_t o[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int px = 0; px < kGwGroupPx; ++px) {
            const uint32_t r = byte_of(d, 3 * px), gr = byte_of(d, 3 * px + 1), bl = byte_of(d, 3 * px + 2);
            const uint32_t y[3] = {gw_comp(r, gr, sr, cr), (uint32_t)s_green[gr], gw_comp(bl, gr, sb, cb)};
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(3 * px + c) >> 2] |= y[c] << (8 * ((3 * px + c) & 3));
        }
        store16(out + off, make_uint4(o[0], o[1], o[2], o[3]));
        store16(out + off + 16, make_uint4(o[4], o[5], o[6], o[7]));
        store16(out + off + 32, make_uint4(o[8], o[9], o[10], o[11]));
    }
    if (blockIdx.x == 0) {  // the frame's tail: fewer than 16 pixels
        const int p = ngroups * kGwGroupPx + tid;
        if (p < n) {
            const size_t off = base + (size_t)p * 3;
            const uint32_t r = in[off], gr = in[off + 1], bl = in[off + 2];
            out[off] = (uint8_t)gw_comp(r, gr, sr, cr);
            out[off + 1] = s_green[gr];
            out[off + 2] = (uint8_t)gw_comp(bl, gr, sb, cb);
        }
    }
}

struct GwBufs {
    uint32_t *part;  // [B][blocks][kGwRow]
    double *stats;   // [B][UWIE_GW_STATS]
};

// workgroups of k_gw_sums per frame: a function of the frame size alone
int gw_blocks(Shape s) { return cdiv((long long)s.npx(), kGwBlockPx); }

GwBufs carve_gw(Carver &c, Shape s)
{
    GwBufs g;
    g.part = c.take<uint32_t>((size_t)s.B * gw_blocks(s) * kGwRow);
    g.stats = c.take<double>((size_t)s.B * UWIE_GW_STATS);
    return g;
}

}  // namespace

void gray_world_plan(int *block_px, int *thread_px)
{
    *block_px = kGwBlockPx;
    *thread_px = kGwGroupPx;
}

size_t gray_world_ws_bytes(Shape s)
{
    Carver c(nullptr);
    carve_gw(c, s);
    return c.total();
}

int launch_gray_world(const uint8_t *d_in, Shape s, double red, double blue, double max_gain, uint8_t *d_out, double *d_stats, void *ws,
                      hipStream_t st)
{
    Carver c(ws);
    const GwBufs g = carve_gw(c, s);
    const int n = (int)s.npx(), nblk = gw_blocks(s);
    UWIE_LAUNCH(k_gw_sums, dim3(nblk, s.B), dim3(256), 0, st, d_in, n, g.part);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_gw_coeffs, dim3(s.B), dim3(64), 0, st, (const uint32_t *)g.part, nblk, n, red, blue, max_gain, g.stats, d_stats);
    UWIE_LAUNCH_CHECK();
    if (d_out) {
        // up to 1024 workgroups per frame, a few groups per thread at large frames (as k_dg8_apply)
        const dim3 grid(std::max(1, std::min(cdiv(n / kGwGroupPx, 256), 1024)), s.B);
        UWIE_LAUNCH(k_gw_apply, grid, dim3(256), 0, st, d_in, n, (const double *)g.stats, d_out);
        UWIE_LAUNCH_CHECK();
    }
    return UWIE_OK;
}

}  // namespace uwie
