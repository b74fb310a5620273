// np.percentile(channel, q) (six_stadigy.py:196-197,216-217; enhancement_strategies.py:265-266) for float32
// channels (S6 surface) and float64 channels (ES surface).
//
// NumPy (2.2.6, method "linear") computes, in the dtype of the data:
//     qd = q / dtype(100);  vi = (n - 1) * qd;  prev = floor(vi);  t = vi - prev
//     a = sorted[prev], b = sorted[prev + 1];  r = a + (b - a) * t;  if t >= 0.5: r = b - (b - a) * (1 - t)
// The index arithmetic depends only on (n, q) and is done on the host in that dtype; the two order statistics per
// percentile are found EXACTLY on the device by an MSD radix select on the order-preserving integer image of the
// float bits (float32: 11+11+10 bits, float64: 5x11+9): one launch of k_sel_pass per digit.  Its blocks count slabs of the
// channel plane into LDS and add the counts to the plane's histogram; the block that arrives last at the plane's ticket
// narrows every query to the bucket holding its rank (no block waits for another).  Up to 8 ranks (4 percentiles) per
// channel are resolved in the same passes; queries sharing a prefix share a histogram ("group").  The values come from
// stored planes or are recomputed from the frame and the transmission (restore.h).  A producer kernel may accumulate the
// first digit's histogram itself (k_fused.hip), saving one sweep.  The same passes answer the planes that the linear-digit
// and rank-counting routes below flag.
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "devutil.h"
#include "restore.h"

namespace uwie {

namespace {

constexpr int kMaxRanks = 2 * kMaxPct;
constexpr int kBins = 2048;

template <typename V>
struct Traits;
template <>
struct Traits<float> {
    using K = uint32_t;
    static constexpr int NPASS = 3;
    __host__ __device__ static int shift(int p) { return p == 0 ? 21 : p == 1 ? 10 : 0; }
    __host__ __device__ static int bits(int p) { return p == 2 ? 10 : 11; }
    __device__ static K key(float v) { return f32_key(v); }
    __device__ static float value(K k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
};
template <>
struct Traits<double> {
    using K = uint64_t;
    static constexpr int NPASS = 6;
    __host__ __device__ static int shift(int p) { return p == 5 ? 0 : 53 - 11 * p; }
    __host__ __device__ static int bits(int p) { return p == 5 ? 9 : 11; }
    __device__ static K key(double v) { return f64_key(v); }
    __device__ static double value(K k)
    {
        return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull)));
    }
};

template <typename K>
struct SelState {                 // one per (image, channel)
    K prefix[kMaxRanks];          // key bits resolved so far (right aligned)
    K gprefix[kMaxRanks];         // distinct prefixes
    uint32_t rank[kMaxRanks];     // remaining rank inside the prefix bucket
    uint32_t gid[kMaxRanks];      // histogram group of the query
    uint32_t ngroups;
    uint32_t ticket;              // blocks of the running pass that have added their counts (k_sel_pass)
};
// (carve_select takes the states at this stride for both key widths)
static_assert(sizeof(SelState<uint64_t>) == 200 && sizeof(SelState<uint32_t>) <= 200, "selection state layout");

struct RankList {
    uint32_t r[kMaxRanks];
    int n;
};

template <typename V>
struct FracList {
    V t[kMaxPct];
    int n;
};

// the state before the first pass: every query in group 0 with its whole rank
template <typename K>
__device__ SelState<K> sel_state(const RankList &ranks)
{
    SelState<K> s;
    for (int q = 0; q < kMaxRanks; ++q) {
        s.prefix[q] = 0;
        s.gprefix[q] = 0;
        s.rank[q] = q < ranks.n ? ranks.r[q] : 0;
        s.gid[q] = 0;
    }
    s.ngroups = 1;
    s.ticket = 0;
    return s;
}

template <typename K>
__global__ void k_sel_init(SelState<K> *st, int nbc, RankList ranks)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbc) return;
    st[i] = sel_state<K>(ranks);
}

template <typename V>
__device__ __forceinline__ void sel_count(uint32_t *h, V v, int shift, int bits, uint32_t mask, int first_pass, int ng,
                                          int nbins, const typename Traits<V>::K *gp)
{
    using K = typename Traits<V>::K;
    const K key = Traits<V>::key(v);
    const uint32_t d = (uint32_t)(key >> shift) & mask;
    if (first_pass) {
        atomicAdd(&h[d], 1u);
    } else {
        // prefixes of distinct groups differ, so at most one matches: select its index, then one conditional atomic
        // (gp[g] for g >= ng holds a value no prefix can take, see k_sel_pass)
        const K pre = key >> (shift + bits);
        uint32_t idx = 0xffffffffu;
#pragma unroll
        for (int g = 0; g < 4; ++g) idx = pre == gp[g] ? (uint32_t)g : idx;
        if (ng > 4) {
#pragma unroll
            for (int g = 4; g < kMaxRanks; ++g) idx = pre == gp[g] ? (uint32_t)g : idx;
        }
        if (idx != 0xffffffffu) atomicAdd(&h[idx * nbins + d], 1u);
    }
}

// digit d (0 <= d < nbins, nbins <= 2304) with excl(d) <= rank < incl(d) over the LDS counts h[]; all 256 threads call
__device__ void block_find_digit(const uint32_t *h, int nbins, uint32_t rank, uint32_t *wsum, uint32_t *found,
                                 uint32_t &digit, uint32_t &rrank)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, per = (nbins + 255) / 256;
    uint32_t loc = 0;
    for (int i = 0; i < per; ++i) {
        const int k = tid * per + i;
        if (k < nbins) loc += h[k];
    }
    uint32_t incl = wave_incl_scan_u32(loc);
    __syncthreads();
    if (lane == 63) wsum[w] = incl;
    if (tid == 0) { found[0] = (uint32_t)nbins - 1; found[1] = 0; }
    __syncthreads();
    for (int i = 0; i < w; ++i) incl += wsum[i];
    const uint32_t excl = incl - loc;
    if (excl <= rank && rank < incl) {
        uint32_t acc = excl;
        for (int i = 0; i < per; ++i) {
            const int k = tid * per + i;
            const uint32_t c = k < nbins ? h[k] : 0;
            if (rank < acc + c) {
                found[0] = (uint32_t)k;
                found[1] = rank - acc;
                break;
            }
            acc += c;
        }
    }
    __syncthreads();
    digit = found[0];
    rrank = found[1];
    __syncthreads();
}

// Value sources of k_sel_pass: each(bc, lo, hi, f) calls f(v) for the values of plane bc at the positions lo .. hi - 1 that
// the calling thread owns (lo is a multiple of 4; all 256 threads of the block call).
// Stored values: [B][3][n] planes (planar) or [B][n][3] pixels, with 16-byte loads where the layout allows.
template <typename T>
struct StoredVals {
    using V = T;
    const V *vals;
    size_t img_stride, chan_stride;
    int elem_stride;
    template <class F>
    __device__ __forceinline__ void each(int bc, int lo, int hi, F &&f) const
    {
        constexpr int VEC = 16 / sizeof(V);
        const V *v = vals + (size_t)(bc / 3) * img_stride + (size_t)(bc % 3) * chan_stride;
        if (elem_stride == 1 && ((size_t)v & 15) == 0) {
            const int hiv = lo + ((hi - lo) / VEC) * VEC;
            constexpr int U = 4;  // 16-byte loads in flight per thread: the sweep is latency-bound, not compute-bound
            int i = lo + threadIdx.x * VEC;
            for (; i + (U - 1) * 256 * VEC < hiv; i += U * 256 * VEC) {
                uint4 raw[U];
#pragma unroll
                for (int u = 0; u < U; ++u) raw[u] = *reinterpret_cast<const uint4 *>(v + i + u * 256 * VEC);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    V q[VEC];
                    *reinterpret_cast<uint4 *>(q) = raw[u];
#pragma unroll
                    for (int j = 0; j < VEC; ++j) f(q[j]);
                }
            }
            for (; i < hiv; i += 256 * VEC) {
                V q[VEC];
                *reinterpret_cast<uint4 *>(q) = *reinterpret_cast<const uint4 *>(v + i);
#pragma unroll
                for (int j = 0; j < VEC; ++j) f(q[j]);
            }
            for (int i = hiv + threadIdx.x; i < hi; i += 256) f(v[i]);
        } else {
            for (int i = lo + threadIdx.x; i < hi; i += 256) f(v[(size_t)i * elem_stride]);
        }
    }
};
// Values recomputed from the frame and the transmission, by the expressions of the producers that histogram them
// (k_fused.hip k_restore_planar_hist): float32 restore (UWIE_INTER_F32T: restore.h one32_raw), or the ES surface's float64
// image (restore.h four64's expression, on the same groups of four pixels, for the plane's channel only).  The channel is a template argument: a[c] / att[c] with a
// runtime c would keep the restore's registers in scratch memory.
template <typename T>
struct RestoredVals {
    using V = T;
    RestoreSrc S;
    int npx;
    template <int C, class F>
    __device__ __forceinline__ void channel(int b, int lo, int hi, F &f) const
    {
        if constexpr (sizeof(V) == 8) {  // four64's sequence for channel C alone: the same groups, the same branch per group
            RestoreImg R;
            R.init(S, b, (size_t)npx);
            for (int p = lo + threadIdx.x * 4; p < hi; p += 1024) {
                const int m = min(4, hi - p);
                uint32_t u[4];
                double tv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    u[i] = i < m ? R.img[(size_t)(p + i) * 3 + C] : 0u;
                    tv[i] = i < m ? R.t[p + i] : 1.0;
                }
                const bool fast = R.recip_ok(tv[0]) && R.recip_ok(tv[1]) && R.recip_ok(tv[2]) && R.recip_ok(tv[3]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < m) f(fast ? R.one64_fast(u[i], C, tv[i], R.recip(tv[i])) : R.one64(u[i], C, tv[i]));
            }
        } else if (S.t32) {
            RestoreImg32 R;
            R.init(S, b, (size_t)npx);
            for (int p = lo + threadIdx.x; p < hi; p += 256)
                f(fminf(fmaxf(R.one32_raw(R.img[(size_t)p * 3 + C], C, R.recip32(R.tf()[p])), 0.0f), 1.0f));
        } else {
            RestoreImg R;
            R.init(S, b, (size_t)npx);
            for (int p = lo + threadIdx.x; p < hi; p += 256) {
                const uint32_t u = R.img[(size_t)p * 3 + C];
                const double tv = R.t[p];
                f(R.recip_ok(tv) ? R.one_fast(u, C, tv, R.recip(tv)) : R.one(u, C, tv));
            }
        }
    }
    template <class F>
    __device__ __forceinline__ void each(int bc, int lo, int hi, F &&f) const
    {
        const int b = bc / 3, c = bc % 3;
        if (c == 0) channel<0>(b, lo, hi, f);
        else if (c == 1) channel<1>(b, lo, hi, f);
        else channel<2>(b, lo, hi, f);
    }
};

// One digit of the select: grid (blocks, B*3), dynamic LDS = (pass ? nq : 1) * nbins * 4 bytes.  Each block counts a
// contiguous slab of the plane (sweep = 0: nothing, the producer has counted the first digit), counting only the elements
// whose resolved prefix matches a query group, and adds its counts to the plane's histogram.  Then it takes a ticket; the
// block that arrives last narrows each query by the digit, regroups the prefixes, writes the order statistics after the last
// digit, and leaves the histogram counters and the ticket at zero for the next pass.  No block waits for another, so the
// result does not depend on how the blocks are dispatched.  only != nullptr: planes with only[bc] == 0 return at once.
template <class Src>
__global__ void __launch_bounds__(256) k_sel_pass(Src src, int n, SelState<typename Traits<typename Src::V>::K> *__restrict__ st,
                                                  int pass, int nq, int sweep, uint32_t *__restrict__ ghist,
                                                  typename Src::V *__restrict__ os, const uint32_t *__restrict__ only)
{
    using V = typename Src::V;
    using K = typename Traits<V>::K;
    extern __shared__ uint32_t h[];
    __shared__ uint32_t wsum[4], found[2];
    __shared__ SelState<K> ss;  // the last arriver's copy of the plane's state
    constexpr int kStateWords = sizeof(SelState<K>) / 4;
    const int bc = blockIdx.y, tid = threadIdx.x;
    if (only && !only[bc]) return;
    SelState<K> *s = st + bc;
    const int shift = Traits<V>::shift(pass), bits = Traits<V>::bits(pass), nbins = 1 << bits;
    const int ng = pass == 0 ? 1 : min((int)s->ngroups, nq);
    uint32_t *gh = ghist + (size_t)bc * kSelGroupStride;
    if (sweep) {
        K gp[kMaxRanks];
#pragma unroll
        for (int g = 0; g < kMaxRanks; ++g) gp[g] = g < ng ? s->gprefix[g] : ~K(0);  // ~0 >> (shift + bits) is not a prefix
        for (int i = tid; i < ng * nbins; i += 256) h[i] = 0;
        __syncthreads();
        const uint32_t mask = (uint32_t)nbins - 1;
        const int per = (((n + 3) / 4 + gridDim.x - 1) / gridDim.x) * 4;  // slab, multiple of 4 elements
        const int lo = min(n, blockIdx.x * per), hi = min(n, lo + per);  // lo == hi for surplus blocks
        src.each(bc, lo, hi, [&](V v) { sel_count<V>(h, v, shift, bits, mask, pass == 0, ng, nbins, gp); });
        __syncthreads();
        for (int i = tid; i < ng * nbins; i += 256) {
            const uint32_t c = h[i];
            if (c) atomicAdd(&gh[(i / nbins) * kBins + (i % nbins)], c);
        }
    }
    // arrival: the counts are device-scope atomics, released at agent scope before the ticket; the last arriver acquires
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t arrived = __hip_atomic_fetch_add(&s->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        found[0] = arrived == gridDim.x - 1;
        if (found[0]) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!found[0]) return;  // block-uniform
    // behind the acquire, plain loads: the plane's state, and its counts eight loads in flight per thread
    if (tid < kStateWords) reinterpret_cast<uint32_t *>(&ss)[tid] = reinterpret_cast<const uint32_t *>(s)[tid];
    for (int i0 = 0; i0 < ng * nbins; i0 += 8 * 256) {
        uint32_t c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 256 + tid;
            c[u] = i < ng * nbins ? gh[(i / nbins) * kBins + (i % nbins)] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u * 256 + tid < ng * nbins) h[i0 + u * 256 + tid] = c[u];
    }
    __syncthreads();
    for (int i = tid; i < ng * nbins; i += 256) gh[(i / nbins) * kBins + (i % nbins)] = 0;  // (for the next pass)
    for (int q = 0; q < nq; ++q) {
        uint32_t d, rr;
        block_find_digit(h + ss.gid[q] * nbins, nbins, ss.rank[q], wsum, found, d, rr);
        if (tid == 0) {
            ss.prefix[q] = (ss.prefix[q] << bits) | (K)d;
            ss.rank[q] = rr;
        }
    }
    if (tid == 0) {
        uint32_t ngr = 0;
        for (int q = 0; q < nq; ++q) {
            uint32_t g = 0;
            for (; g < ngr; ++g)
                if (ss.gprefix[g] == ss.prefix[q]) break;
            if (g == ngr) ss.gprefix[ngr++] = ss.prefix[q];
            ss.gid[q] = g;
        }
        ss.ngroups = ngr;
        ss.ticket = 0;
        if (pass == Traits<V>::NPASS - 1)
            for (int q = 0; q < nq; ++q) os[bc * kMaxRanks + q] = Traits<V>::value(ss.prefix[q]);
    }
    __syncthreads();
    if (tid < kStateWords) reinterpret_cast<uint32_t *>(s)[tid] = reinterpret_cast<const uint32_t *>(&ss)[tid];
}

// All digits of the select for the planes of `only` (every plane: nullptr).  The state (k_sel_init, or the scan kernels of the
// routes below) and the counters (zero, or the first digit's when pass1_done) are ready.
template <class Src>
int sel_passes(const SelectPlan &plan, const Src &src, int n, int nbc, int blocks, bool pass1_done, const uint32_t *only,
               hipStream_t st)
{
    using V = typename Src::V;
    using K = typename Traits<V>::K;
    const int nq = 2 * plan.nq;
    for (int p = 0; p < Traits<V>::NPASS; ++p) {
        const int sweep = p > 0 || !pass1_done;
        const size_t lds = (size_t)(p == 0 ? 1 : nq) * (1u << Traits<V>::bits(p)) * sizeof(uint32_t);
        UWIE_LAUNCH(k_sel_pass<Src>, dim3(sweep ? blocks : 1, nbc), dim3(256), lds, st, src, n, (SelState<K> *)plan.state, p, nq,
                    sweep, plan.ghist, (V *)plan.os, only);
        UWIE_LAUNCH_CHECK();
    }
    return UWIE_OK;
}

// blocks per plane of a pass.  Stored values: few, fat blocks (the LDS histogram is zeroed and flushed once per block, and every
// block pays an agent-scope release on the pass's critical path), at least 256 in all: with the 1024 of the former sweep kernel
// the DifferentiableEnhancement forward took 1.27 instead of 1.21 ms at 8 x 4K and 96 instead of 84 us at 32 x 224^2.
// Recomputed values (the flagged planes of the linear-digit and rank routes): 96 per plane, the grid of the round-4 fallback
// (11 bytes per value, three planes per frame: 24 took 2.8 ms for two flagged 4K planes), whatever the batch.
int pass_blocks(long long n, int nbc, bool recomputed)
{
    if (recomputed) return 96;
    int blocks = (int)((n + 262143) / 262144);
    if (blocks * nbc < 256) blocks = cdiv(256, nbc);
    return std::max(1, std::min(blocks, 256));
}
// NumPy's _lerp (numpy/lib/_function_base_impl.py), in the data's dtype
template <typename V>
__device__ __forceinline__ V np_lerp(V a, V b, V t)
{
    const V diff = b - a;
    V r = a + diff * t;
    if (t >= (V)0.5) r = b - diff * ((V)1 - t);
    return r;
}

template <typename V>
__global__ void k_pct_finish(const V *__restrict__ os, int nbc, FracList<V> fr, V *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbc * fr.n) return;
    const int bc = i / fr.n, j = i % fr.n;
    out[i] = np_lerp<V>(os[bc * kMaxRanks + 2 * j], os[bc * kMaxRanks + 2 * j + 1], fr.t[j]);
}

// Percentiles of a stretch of a stretch from ONE selection: the first stretch f1(x) = clip((x - lo1)/(hi1 - lo1 + eps))
// is monotone non-decreasing in floating point (rounding, division by a positive constant and clip all are), so the
// k-th order statistic of f1(img) is f1 of the k-th order statistic of img.  Percentiles 0,1 are the first
// stretch's (six_stadigy.py:196-197); 2,3 are the second's (white_balance, six_stadigy.py:216-217), taken on
// f1(img).  out[bc][4] = lo1, hi1, lo2, hi2.
__global__ void k_pct_finish_chain(const float *__restrict__ os, int nbc, FracList<float> fr, float eps,
                                   float *__restrict__ out)
{
    const int bc = blockIdx.x * blockDim.x + threadIdx.x;
    if (bc >= nbc) return;
    const float *o = os + bc * kMaxRanks;
    const float lo1 = np_lerp<float>(o[0], o[1], fr.t[0]), hi1 = np_lerp<float>(o[2], o[3], fr.t[1]);
    const float den = (hi1 - lo1) + eps;
    float m[4];
    for (int i = 0; i < 4; ++i) m[i] = fminf(fmaxf((o[4 + i] - lo1) / den, 0.0f), 1.0f);
    out[bc * 4 + 0] = lo1;
    out[bc * 4 + 1] = hi1;
    out[bc * 4 + 2] = np_lerp<float>(m[0], m[1], fr.t[2]);
    out[bc * 4 + 3] = np_lerp<float>(m[2], m[3], fr.t[3]);
}

// Host side of np.percentile's index arithmetic ("linear" method), in the data's dtype V.
template <typename V>
void percentile_indices(long long n, double q_percent, uint32_t *prev, uint32_t *next, double *t)
{
    const V q = (V)q_percent / (V)100;
    const V nm1 = (V)(n - 1);
    const V vi = nm1 * q;
    const V p = std::floor(vi);
    if (vi >= nm1) {  // above bounds: both neighbours are the maximum
        *prev = *next = (uint32_t)(n - 1);
        *t = 0.0;
        return;
    }
    *prev = (uint32_t)p;
    *next = *prev + 1;
    *t = (double)(vi - p);
}

// list capacity per (image, channel, group); UWIE_LIN_CAP overrides it (tests force the overflow / fallback path)
uint32_t lin_cap(Shape s)
{
    const uint32_t dflt = (uint32_t)std::max<size_t>(65536, s.npx() / 64);
    const long v = tune().lin_cap;  // (0 outside an entry point: the workspace is sized for the default)
    return v > 0 && v < (long)dflt ? (uint32_t)v : dflt;
}

// The selection's workspace, the one place that lays it out: every begin carves its plan here and select_ws_bytes is this
// carve on a null base.  lin: the buffers of the linear-digit and rank routes behind the three every route uses.
void carve_select(Carver &c, Shape s, bool lin, SelectPlan *plan)
{
    const size_t nbc = (size_t)s.B * 3;
    plan->state = c.take<SelState<uint64_t>>(nbc);  // sized for the wider key
    plan->ghist = c.take<uint32_t>(nbc * kMaxRanks * kBins);
    plan->os = c.take<double>(nbc * kMaxRanks);
    if (!lin) return;
    plan->lin = c.take<LinState>(nbc);
    plan->flags = c.take<uint32_t>(nbc);
    plan->cap = lin_cap(s);
    plan->lists = c.take<double>(nbc * kLinLists * plan->cap);  // (sized for the float64 surface)
}

int zero_ghist(const SelectPlan &plan, Shape s, hipStream_t st)
{
    UWIE_HIP_CHECK(hipMemsetAsync(plan.ghist, 0, sizeof(uint32_t) * (size_t)s.B * 3 * kMaxRanks * kBins, st));
    return UWIE_OK;
}

RankList rank_list(const SelectPlan &plan)
{
    RankList ranks;
    ranks.n = 2 * plan.nq;
    for (int j = 0; j < ranks.n; ++j) ranks.r[j] = plan.ranks[j];
    return ranks;
}

// What the percentile begins share: the checks, the carve, and np.percentile's ranks and weights in the data's dtype V.
template <typename V>
int plan_percentiles(Shape s, const double *q_percent, int nq, void *ws, bool lin, SelectPlan *plan)
{
    UWIE_REQUIRE(nq >= 1 && nq <= kMaxPct, "percentiles: 1..4 percentiles per call");
    const long long n = (long long)s.npx();
    UWIE_REQUIRE(n >= 1 && n < (1ll << 31), "percentiles: plane size out of range");
    Carver c(ws);
    carve_select(c, s, lin, plan);
    plan->nq = nq;
    plan->is64 = sizeof(V) == 8;
    for (int j = 0; j < nq; ++j)
        percentile_indices<V>(n, q_percent[j], &plan->ranks[2 * j], &plan->ranks[2 * j + 1], &plan->t[j]);
    return UWIE_OK;
}

// DifferentiableEnhancement.color_stretch_batch (vgg_16_UIE.py:78-82): per image, the sorted positions
// int((L/100.0) * n) clamped to [0, n-1] of L_low and L_high, evaluated in float64 like the Python expression
// (L is the float32 parameter's value).  params[b*stride + 0/1] = L_low, L_high.
__global__ void k_sel_init_stretch_ranks(SelState<uint32_t> *st, int nbc, const float *__restrict__ params, int stride,
                                         int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbc) return;
    const float *pr = params + (size_t)(i / 3) * stride;
    RankList ranks;
    ranks.n = 2;
    for (int q = 0; q < 2; ++q) {
        const double pos = ((double)pr[q] / 100.0) * (double)n;
        long long idx = (long long)pos;  // int(): truncation toward zero
        idx = idx < 0 ? 0 : idx > n - 1 ? n - 1 : idx;
        ranks.r[q] = (uint32_t)idx;
    }
    st[i] = sel_state<uint32_t>(ranks);
}

// deep_learning_parameters.DifferentiableEnhancement.color_stretch (:73-77): the same two sorted positions per image, by
// Python's indexing rules instead of a clamp (gated_rank).  An image without a valid position selects position 0 (a safe
// substitute) and sets UWIE_STATUS_DIFF_RANK; the gated kernels write NaN for it.
__global__ void k_sel_init_gated_ranks(SelState<uint32_t> *st, int nbc, const float *__restrict__ params, int stride, int n,
                                       uint32_t *status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbc) return;
    const float *pr = params + (size_t)(i / 3) * stride;
    int k[2];
    const bool ok0 = gated_rank(pr[0], n, &k[0]), ok1 = gated_rank(pr[1], n, &k[1]);
    const bool ok = ok0 && ok1;
    RankList ranks;
    ranks.n = 2;
    ranks.r[0] = ok ? (uint32_t)k[0] : 0u;
    ranks.r[1] = ok ? (uint32_t)k[1] : 0u;
    if (!ok && status) atomicOr(status, (uint32_t)UWIE_STATUS_DIFF_RANK);
    st[i] = sel_state<uint32_t>(ranks);
}

// The rank begins of the two DifferentiableEnhancement modules: init(state, nbc, n) launches the kernel that writes every
// plane's two ranks.
template <class Init>
int begin_ranks(Shape s, const char *range_msg, void *ws, hipStream_t st, SelectPlan *plan, Init &&init)
{
    const long long n = (long long)s.npx();
    UWIE_REQUIRE(n >= 1 && n < (1ll << 31), range_msg);
    Carver c(ws);
    carve_select(c, s, false, plan);
    plan->nq = 1;  // two ranks
    plan->is64 = false;
    plan->t[0] = 0.0;
    init((SelState<uint32_t> *)plan->state, s.B * 3, (int)n);
    UWIE_LAUNCH_CHECK();
    return zero_ghist(*plan, s, st);
}

}  // namespace

// ===================================================================================== linear-digit selection
namespace {

constexpr uint32_t kLinDone = 0xffffffffu;
constexpr int kLinSampleOff = 4096;  // the sample histogram of a plane lives behind the producer's in its ghist group

// grid (blocks, B): linear-digit histogram of the restored image on every stride-th group of four pixels (ngs groups;
// the frame as one flat array, so the sample is spread over rows and columns alike)
template <typename V>
__global__ void __launch_bounds__(256) k_lin_sample(RestoreSrc S, int npx, int stride, int ngs, uint32_t *__restrict__ ghist)
{
    __shared__ uint32_t h[3][kLinBins];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 3 * kLinBins; i += 256) (&h[0][0])[i] = 0;
    __syncthreads();
    RestoreImg R;
    RestoreImg32 R32;  // UWIE_INTER_F32T (float32 planes only)
    if (S.t32) R32.init(S, b, (size_t)npx);
    else R.init(S, b, (size_t)npx);
    for (int i = blockIdx.x * 256 + tid; i < ngs; i += gridDim.x * 256) {
        V r[3][4];
        if constexpr (sizeof(V) == 8) R.four64((i * stride + stride / 2) * 4, 4, r);  // (ES surface: the float64 image)
        else if (S.t32) R32.four((i * stride + stride / 2) * 4, 4, r);
        else R.four((i * stride + stride / 2) * 4, 4, r);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) atomicAdd(&h[c][lin_digit(r[c][j])], 1u);
    }
    __syncthreads();
    for (int i = tid; i < 3 * kLinBins; i += 256) {
        const uint32_t c = (&h[0][0])[i];
        if (c) atomicAdd(&ghist[(size_t)(b * 3 + i / kLinBins) * kSelGroupStride + kLinSampleOff + (i % kLinBins)], c);
    }
}

// one block per (image, channel): clears the state; with a sample (ns > 0) the window of percentile j spans the bins
// that hold the sample ranks r_j*ns/n -+ delta, delta = 4 binomial standard deviations of the sample rank (+2); windows
// that touch are merged.  shift: test knob, moves the windows up by that many bins.
__global__ void __launch_bounds__(256) k_lin_predict(LinState *__restrict__ st, uint32_t *__restrict__ ghist,
                                                     RankList ranks, uint32_t n, uint32_t ns, int shift)
{
    __shared__ uint32_t h[kLinBins], wsum[4], found[2], wl[kMaxPct], wh[kMaxPct];
    const int bc = blockIdx.x, tid = threadIdx.x;
    if (tid < kMaxPct) { wl[tid] = kLinNoWin; wh[tid] = 0; }
    if (ns > 0) {
        uint32_t *gh = ghist + (size_t)bc * kSelGroupStride + kLinSampleOff;
        for (int i = tid; i < kLinBins; i += 256) {
            h[i] = gh[i];
            gh[i] = 0;  // (the plane's counters are zero again for the key-digit passes of a flagged plane)
        }
        __syncthreads();
        for (int j = 0; j < ranks.n / 2 && j < kMaxPct; ++j) {
            const double p = (double)ranks.r[2 * j] / (double)n, sd = sqrt((double)ns * p * (1.0 - p));
            const double c0 = (double)ranks.r[2 * j] * ns / n, c1 = (double)ranks.r[2 * j + 1] * ns / n, delta = 4.0 * sd + 2.0;
            const uint32_t rlo = (uint32_t)fmax(c0 - delta, 0.0), rhi = (uint32_t)fmin(c1 + delta, (double)ns - 1.0);
            uint32_t dlo, dhi, rr;
            block_find_digit(h, kLinBins, rlo, wsum, found, dlo, rr);
            block_find_digit(h, kLinBins, rhi, wsum, found, dhi, rr);
            if (tid == 0) {  // interior bins only: the scan answers the bins of exact 0 and exact 1 by itself
                wl[j] = (uint32_t)min(max((int)dlo + shift, 1), kLinBins - 2);
                wh[j] = (uint32_t)min(max((int)dhi + shift, (int)wl[j]), kLinBins - 2);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        LinState s;
        for (int q = 0; q < kMaxRanks; ++q) { s.rr[q] = 0; s.qbin[q] = 0; s.gid[q] = kLinDone; s.gbin[q] = kLinDone; }
        for (int g = 0; g < kLinLists; ++g) s.gcount[g] = 0;
        s.ngroups = 0;
        // windows that touch or overlap become one (the producer files a value under one window only)
        for (bool again = true; again;) {
            again = false;
            for (int i = 0; i < kMaxPct; ++i)
                for (int j = i + 1; j < kMaxPct; ++j)
                    if (wl[i] != kLinNoWin && wl[j] != kLinNoWin && wl[j] <= wh[i] + 1 && wl[i] <= wh[j] + 1) {
                        wl[i] = min(wl[i], wl[j]);
                        wh[i] = max(wh[i], wh[j]);
                        wl[j] = kLinNoWin;
                        again = true;
                    }
        }
        for (int w = 0; w < kMaxPct; ++w) {
            s.wlo[w] = wl[w];
            s.wspan[w] = wl[w] == kLinNoWin ? 0 : wh[w] - wl[w];
            s.below[w] = 0;
        }
        st[bc] = s;
    }
}

// one block per (image, channel): the bin of every rank from the producer's histogram; ranks in the bins of exact
// 0 / exact 1 are answered here.  A plane all of whose other queries fall into the predicted windows is done with
// collecting (ngroups = 0, gid = the window's list); otherwise its queries are grouped by bin for the collecting sweep.
// The plane's key-digit state is set and its histogram counters are left at zero, for the passes if the plane is flagged.
template <typename V>
__global__ void __launch_bounds__(256) k_lin_scan(LinState *__restrict__ st, uint32_t *__restrict__ ghist, RankList ranks,
                                                  V *__restrict__ os, uint32_t *__restrict__ flags, uint32_t cap,
                                                  SelState<typename Traits<V>::K> *__restrict__ sel)
{
    __shared__ uint32_t h[kLinBins], wsum[4], found[2], qbin[kMaxRanks], qrr[kMaxRanks];
    const int bc = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) sel[bc] = sel_state<typename Traits<V>::K>(ranks);
    uint32_t *gh = ghist + (size_t)bc * kSelGroupStride;
    for (int i = tid; i < kLinBins; i += 256) {
        h[i] = gh[i];
        gh[i] = 0;
    }
    __syncthreads();
    for (int q = 0; q < ranks.n; ++q) {
        uint32_t d, rr;
        block_find_digit(h, kLinBins, ranks.r[q], wsum, found, d, rr);
        if (tid == 0) { qbin[q] = d; qrr[q] = rr; }
    }
    __syncthreads();
    if (tid == 0) {
        LinState s = st[bc];
        bool covered = true;
        for (int q = 0; q < kMaxRanks; ++q) { s.rr[q] = 0; s.qbin[q] = 0; s.gid[q] = kLinDone; s.gbin[q] = kLinDone; }
        for (int q = 0; q < ranks.n; ++q) {
            s.rr[q] = qrr[q];
            s.qbin[q] = qbin[q];
            if (qbin[q] == 0 || qbin[q] == kLinBins - 1) {  // every element of these bins is 0 resp. 1
                os[bc * kMaxRanks + q] = qbin[q] == 0 ? (V)0 : (V)1;
                continue;
            }
            int w = -1;
            for (int i = kMaxPct - 1; i >= 0; --i)
                if (qbin[q] - s.wlo[i] <= s.wspan[i]) w = i;
            if (w >= 0 && s.gcount[w] > cap) w = -1;  // the window met a heavy bin: the target bin alone may still fit
            if (w >= 0) s.gid[q] = (uint32_t)w;
            else covered = false;
        }
        uint32_t ng = 0;
        if (!covered) {
            for (int g = 0; g < kLinLists; ++g) s.gcount[g] = 0;
            for (int q = 0; q < ranks.n; ++q) {
                s.gid[q] = kLinDone;
                if (qbin[q] == 0 || qbin[q] == kLinBins - 1) continue;
                uint32_t g = 0;
                for (; g < ng; ++g)
                    if (s.gbin[g] == qbin[q]) break;
                if (g == ng) s.gbin[ng++] = qbin[q];
                s.gid[q] = g;
            }
        }
        s.ngroups = ng;
        st[bc] = s;
        flags[bc] = 0;
    }
}

// After the rank-counting sweep (k_restore_rank): one thread per (image, channel).  Window w holds the elements of bins
// wlo .. wlo + wspan in its list (gcount of them) and `below` elements lie in the bins under it, so rank r belongs to the
// window with below <= r < below + gcount, at position r - below of its list.  Bins 0 and kLinBins - 1 hold exact zeros and
// exact ones only: a rank under a window that starts at bin 1 is 0, one above a window that ends at bin 2048 is 1.  Anything
// else -- the prediction missed, or the list overflowed -- flags the plane for the key-digit passes (whose state is set here).
__global__ void k_rank_scan(LinState *__restrict__ st, RankList ranks, float *__restrict__ os, uint32_t *__restrict__ flags,
                            uint32_t cap, int nbc, SelState<uint32_t> *__restrict__ sel)
{
    const int bc = blockIdx.x * blockDim.x + threadIdx.x;
    if (bc >= nbc) return;
    sel[bc] = sel_state<uint32_t>(ranks);
    LinState s = st[bc];
    bool miss = false;
    for (int q = 0; q < kMaxRanks; ++q) { s.rr[q] = 0; s.qbin[q] = 0; s.gid[q] = kLinDone; s.gbin[q] = kLinDone; }
    for (int q = 0; q < ranks.n; ++q) {
        const uint32_t r = ranks.r[q];
        bool done = false;
        for (int w = 0; w < kMaxPct && !done; ++w) {
            if (s.wlo[w] == kLinNoWin) continue;
            const uint32_t below = s.below[w], cnt = s.gcount[w];
            if (r >= below && r - below < cnt) {
                if (cnt <= cap) {
                    s.gid[q] = (uint32_t)w;
                    s.rr[q] = r - below;
                    s.qbin[q] = kLinAnyBin;
                } else {
                    miss = true;
                }
                done = true;
            } else if (r < below && s.wlo[w] == 1u) {
                os[bc * kMaxRanks + q] = 0.0f;
                done = true;
            } else if (r >= below && s.wlo[w] + s.wspan[w] == (uint32_t)kLinBins - 2u) {
                os[bc * kMaxRanks + q] = 1.0f;
                done = true;
            }
        }
        miss = miss || !done;
    }
    s.ngroups = 0;
    st[bc] = s;
    flags[bc] = miss ? 1u : 0u;
}

// grid (blocks, B*3): one sweep over the plane; elements whose bin is a target bin go to that group's list.  A block
// stages its candidates in LDS (they are ~0.5 % of the elements) and reserves list space for a batch at a time.
template <typename V>
__global__ void __launch_bounds__(256) k_lin_collect(const V *__restrict__ vals, int n, LinState *__restrict__ st,
                                                     V *__restrict__ lists, uint32_t cap)
{
    constexpr int kStage = sizeof(V) == 8 ? 256 : 512;  // 16 KB of LDS either way
    __shared__ V stg[kMaxRanks][kStage];
    __shared__ uint32_t scount[kMaxRanks], sbase[kMaxRanks];
    const int bc = blockIdx.y, tid = threadIdx.x;
    LinState *s = st + bc;
    const int ng = (int)s->ngroups;
    if (ng == 0) return;
    // Target bins are interior (1..2048: the scan answers bins 0 and 2049 itself), so with d = (uint32)(x * 2048):
    // x is in bin tb  <=>  d == tb - 1, except that x = 0 also gives d = 0: zeros are mapped to a d nobody asks for.
    uint32_t gd[kMaxRanks];
#pragma unroll
    for (int g = 0; g < kMaxRanks; ++g) gd[g] = g < ng ? s->gbin[g] - 1 : kLinDone;
    if (tid < kMaxRanks) scount[tid] = 0;
    __syncthreads();
    V *L = lists + (size_t)bc * kLinLists * cap;
    const V *v = vals + (size_t)bc * n;
    const int per = (((n + 3) / 4 + gridDim.x - 1) / gridDim.x) * 4;
    const int lo = min(n, blockIdx.x * per), hi = min(n, lo + per);
    auto take = [&](V x, bool live) {
        const uint32_t d = (live && x > (V)0) ? (uint32_t)(x * (V)2048) : 0xfffffffeu;
        uint32_t idx = kLinDone;
#pragma unroll
        for (int g = 0; g < 4; ++g) idx = d == gd[g] ? (uint32_t)g : idx;
        if (ng > 4) {
#pragma unroll
            for (int g = 4; g < kMaxRanks; ++g) idx = d == gd[g] ? (uint32_t)g : idx;
        }
        if (idx != kLinDone) {
            const uint32_t pos = atomicAdd(&scount[idx], 1u);
            if (pos < (uint32_t)kStage) {
                stg[idx][pos] = x;
            } else {  // a burst (a smooth region at the percentile's level): straight to the list
                const uint32_t at = atomicAdd(&s->gcount[idx], 1u);
                if (at < cap) L[(size_t)idx * cap + at] = x;
            }
        }
    };
    // all threads of the block call: move the staged candidates to the lists when a stage is three quarters full
    auto flush = [&](bool force) {
        __syncthreads();
        bool need = force;
        for (int g = 0; g < ng; ++g) need = need || scount[g] > (uint32_t)(kStage * 3 / 4);
        if (!need) return;  // block-uniform
        if (tid < ng) sbase[tid] = atomicAdd(&s->gcount[tid], min(scount[tid], (uint32_t)kStage));
        __syncthreads();
        for (int g = 0; g < ng; ++g) {
            const uint32_t c = min(scount[g], (uint32_t)kStage), base = sbase[g];
            for (uint32_t i = tid; i < c; i += 256)
                if (base + i < cap) L[(size_t)g * cap + base + i] = stg[g][i];
        }
        __syncthreads();
        if (tid < kMaxRanks) scount[tid] = 0;
        __syncthreads();
    };
    const bool vec = ((size_t)v & 15) == 0;
    const int hiv = vec ? lo + ((hi - lo) / 4) * 4 : lo;
    constexpr int U = sizeof(V) == 8 ? 2 : 4;  // 16-byte loads: four floats, two doubles (two per group of four)
    for (int base = lo; base < hiv; base += U * 1024) {  // block-uniform trip count
        const int i = base + tid * 4;
        V raw[U][4];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = i + u * 1024 < hiv;
            if constexpr (sizeof(V) == 8) {
                const double2 lo2 = ok[u] ? *reinterpret_cast<const double2 *>(v + i + u * 1024) : make_double2(0, 0);
                const double2 hi2 = ok[u] ? *reinterpret_cast<const double2 *>(v + i + u * 1024 + 2) : make_double2(0, 0);
                raw[u][0] = lo2.x; raw[u][1] = lo2.y; raw[u][2] = hi2.x; raw[u][3] = hi2.y;
            } else {
                const float4 q = ok[u] ? *reinterpret_cast<const float4 *>(v + i + u * 1024) : make_float4(0, 0, 0, 0);
                raw[u][0] = q.x; raw[u][1] = q.y; raw[u][2] = q.z; raw[u][3] = q.w;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) take(raw[u][e], ok[u]);
        }
        flush(false);
    }
    for (int t0 = hiv; t0 < hi; t0 += 256) {
        const int j = t0 + tid;
        take(j < hi ? v[j] : (V)0, j < hi);
        flush(false);
    }
    flush(true);
}

// The same sweep when the planes are not stored: grid (blocks, B), the block recomputes its pixels' three restored
// values from the frame and the transmission (restore.h, 11 instead of 12 bytes per pixel and no stored copy) and
// files each under its own channel's groups.  NG: most groups per channel (ranks of the call).
template <typename V, int NG>
__global__ void __launch_bounds__(256) k_lin_collect_src(RestoreSrc S, int n, LinState *__restrict__ st,
                                                         V *__restrict__ lists, uint32_t cap)
{
    constexpr int kStage = sizeof(V) == 8 ? 256 : 512;  // 24 KB of LDS either way (V = double: the ES surface's float64 image)
    __shared__ V stg[3 * NG][kStage];
    __shared__ uint32_t scount[3 * NG], sbase[3 * NG];
    const int b = blockIdx.y, tid = threadIdx.x;
    LinState *s = st + 3 * b;
    int ngc[3];
    uint32_t gd[3][NG];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ngc[c] = min((int)s[c].ngroups, NG);
#pragma unroll
        for (int g = 0; g < NG; ++g) gd[c][g] = g < ngc[c] ? s[c].gbin[g] - 1 : kLinDone;
    }
    if (ngc[0] + ngc[1] + ngc[2] == 0) return;
    if (tid < 3 * NG) scount[tid] = 0;
    __syncthreads();
    RestoreImg R;
    RestoreImg32 R32;  // UWIE_INTER_F32T (float32 planes only)
    if (S.t32) R32.init(S, b, (size_t)n);
    else R.init(S, b, (size_t)n);
    const int per = (((n + 3) / 4 + gridDim.x - 1) / gridDim.x) * 4;
    const int lo = min(n, blockIdx.x * per), hi = min(n, lo + per);
    auto take = [&](int c, V x, bool live) {
        const uint32_t d = (live && x > (V)0) ? (uint32_t)(x * (V)2048) : 0xfffffffeu;  // see k_lin_collect
        uint32_t idx = kLinDone;
#pragma unroll
        for (int g = 0; g < NG; ++g) idx = d == gd[c][g] ? (uint32_t)g : idx;
        if (idx != kLinDone) {
            const uint32_t pos = atomicAdd(&scount[c * NG + idx], 1u);
            if (pos < (uint32_t)kStage) {
                stg[c * NG + idx][pos] = x;
            } else {  // a burst: straight to the list
                const uint32_t at = atomicAdd(&s[c].gcount[idx], 1u);
                if (at < cap) lists[((size_t)(3 * b + c) * kLinLists + idx) * cap + at] = x;
            }
        }
    };
    auto flush = [&](bool force) {  // all threads of the block call
        __syncthreads();
        bool need = force;
        for (int j = 0; j < 3 * NG; ++j) need = need || scount[j] > (uint32_t)(kStage * 3 / 4);
        if (!need) return;  // block-uniform
        if (tid < 3 * NG) {
            const uint32_t c = min(scount[tid], (uint32_t)kStage);
            if (c) sbase[tid] = atomicAdd(&s[tid / NG].gcount[tid % NG], c);
        }
        __syncthreads();
        for (int j = 0; j < 3 * NG; ++j) {
            const uint32_t c = min(scount[j], (uint32_t)kStage), base = sbase[j];
            V *L = lists + ((size_t)(3 * b + j / NG) * kLinLists + (j % NG)) * cap;
            for (uint32_t i = tid; i < c; i += 256)
                if (base + i < cap) L[base + i] = stg[j][i];
        }
        __syncthreads();
        if (tid < 3 * NG) scount[tid] = 0;
        __syncthreads();
    };
    constexpr int U = 2;
    for (int base = lo; base < hi; base += U * 1024) {  // block-uniform trip count
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = base + u * 1024 + tid * 4, m = min(4, hi - p);
            if (m > 0) {
                V r[3][4];
                if constexpr (sizeof(V) == 8) R.four64(p, m, r);
                else if (S.t32) R32.four(p, m, r);
                else R.four(p, m, r);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    take(0, r[0][i], i < m);
                    take(1, r[1][i], i < m);
                    take(2, r[2][i], i < m);
                }
            }
        }
        flush(false);
    }
    flush(true);
}

// One block of 1024 per (image, channel, query): the query is finished on its list by a radix select among the list's
// elements of the query's bin (a window's list holds neighbouring bins too).
// The elements of one linear bin span 1/2048 of [0, 1], so their keys share most of their high bits: fixed key digits
// would put thousands of increments on a handful of LDS counters (same-address atomics serialise; that was 0.28 ms at
// 4K x 64).  The first sweep therefore only copies the bin's elements into LDS (if they fit) and takes the minimum and
// maximum key; the select then runs over the bits in which those two differ, eleven at a time from the top, where the
// elements spread evenly.
template <typename V>
__global__ void __launch_bounds__(1024) k_lin_finish(const LinState *__restrict__ st, const V *__restrict__ lists,
                                                     uint32_t cap, V *__restrict__ os, uint32_t *__restrict__ flags, int pair,
                                                     int nlists)
{
    using K = typename Traits<V>::K;
    constexpr int kBuf = 49152 / (int)sizeof(V);
    __shared__ uint32_t h[2048], wsum[16], found[2], s_nloc;
    __shared__ unsigned long long s_kmin, s_kmax;
    __shared__ V s_buf[kBuf];
    const int bc = blockIdx.x, tid = threadIdx.x, lane = tid & 63;  // grid (B*3, ranks)
    const LinState *s = st + bc;
    // pair: blocks 0 .. ranks/2 - 1 take the even queries (and their successor when it is the next element of the same list),
    // blocks ranks/2 .. the odd queries that are not such successors
    int q = blockIdx.y;
    if (pair) {
        const int half = (int)gridDim.y / 2;
        if (q < half) {
            q = 2 * q;
        } else {
            q = 2 * (q - half) + 1;
            if (s->gid[q] != kLinDone && s->gid[q] == s->gid[q - 1] && s->qbin[q] == s->qbin[q - 1] && s->rr[q] - s->rr[q - 1] <= 1u)
                return;  // its predecessor's block answers it
        }
    }
    const bool with_next = pair && !(q & 1);
    const uint32_t g = s->gid[q];
    if (g == kLinDone) return;  // block-uniform: answered by the scan
    const uint32_t cnt = s->gcount[g];
    if (cnt > cap) {
        if (tid == 0) flags[bc] = 1;
        return;
    }
    const V *L = lists + ((size_t)bc * nlists + g) * cap;  // (nlists lists of `cap` elements per plane: kLinLists, or 2 four times as long)
    uint32_t r = s->rr[q];
    const uint32_t tb = s->qbin[q];
    // A whole window's list (tb == kLinAnyBin, the rank-counting sweep: several bins, ~1 % of the plane, 100 K elements at 4K)
    // does not fit the LDS buffer, and every further pass over it in global memory is a dozen dependent round trips of a
    // lone block (0.27 ms at 4K x 64).  So ONE pass bins its elements 2048 ways across the window's value range and finds the
    // rank's sub-bin; from then on "mine" is that sub-bin's few dozen elements and everything else runs in LDS.
    bool sub = false;
    float sub_lo = 0.0f, sub_scale = 0.0f;
    uint32_t sub_d = 0;
    auto subbin = [&](V x) -> uint32_t {
        const float f = ((float)x - sub_lo) * sub_scale;  // monotone in x: the same expression in every pass
        return (uint32_t)fminf(fmaxf(f, 0.0f), 2047.0f);
    };
    if (tb == kLinAnyBin && cnt > (uint32_t)kBuf) {  // block-uniform
        sub = true;
        sub_lo = (float)(s->wlo[g] - 1u) * (1.0f / 2048.0f);
        sub_scale = 2048.0f * 2048.0f / (float)(s->wspan[g] + 1u);
        for (int i = tid; i < 2048; i += 1024) h[i] = 0;
        __syncthreads();
        constexpr int kFly = sizeof(V) == 4 ? 16 : 8;  // loads in flight per thread (a lone block: latency is all there is)
        for (uint32_t base = 0; base < cnt; base += kFly * 1024) {
            V x[kFly];
#pragma unroll
            for (int u = 0; u < kFly; ++u) {
                const uint32_t i = min(base + u * 1024 + tid, cnt - 1);  // (clamped, not predicated: no wait per load)
                x[u] = L[i];
            }
#pragma unroll
            for (int u = 0; u < kFly; ++u)
                if (base + u * 1024 + tid < cnt) atomicAdd(&h[subbin(x[u])], 1u);
        }
        __syncthreads();
        uint32_t d, rr;
        block_find_digit(h, 2048, r, wsum, found, d, rr);
        sub_d = d;
        r = rr;
    }
    const uint32_t r_mine = r;  // the query's rank among "mine"
    auto is_mine = [&](V x, uint32_t i) -> bool {
        if (tb != kLinAnyBin) return lin_digit(x) == tb;
        return i < cnt && (!sub || subbin(x) == sub_d);
    };
    if (tid == 0) {
        s_nloc = 0;
        s_kmin = ~0ull;
        s_kmax = 0ull;
    }
    __syncthreads();
    {
        unsigned long long kmin = ~0ull, kmax = 0ull;
        constexpr int kFly = sizeof(V) == 4 ? 16 : 8;
        for (uint32_t base = 0; base < cnt; base += kFly * 1024) {  // kFly loads in flight per thread
            V x[kFly];
#pragma unroll
            for (int u = 0; u < kFly; ++u) {
                const uint32_t i = base + u * 1024 + tid;
                const V v = L[min(i, cnt - 1)];  // (clamped load, then the select: no wait per load)
                x[u] = i < cnt ? v : (V)-1;  // (bin 0, never a list's target)
            }
#pragma unroll
            for (int u = 0; u < kFly; ++u) {
                const bool mine = is_mine(x[u], base + u * 1024 + tid);
                const uint64_t m = __ballot(mine);
                if (m) {  // wavefront-aggregated append
                    const int leader = (int)__builtin_ctzll(m);
                    uint32_t at = 0;
                    if (lane == leader) at = atomicAdd(&s_nloc, (uint32_t)__popcll(m));
                    at = __shfl(at, leader) + (uint32_t)__popcll(m & ((1ull << lane) - 1));
                    if (mine) {
                        const unsigned long long key = (unsigned long long)Traits<V>::key(x[u]);
                        kmin = key < kmin ? key : kmin;
                        kmax = key > kmax ? key : kmax;
                        if (at < (uint32_t)kBuf) s_buf[at] = x[u];
                    }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long a = shfl_u64(kmin, lane ^ o), b = shfl_u64(kmax, lane ^ o);
            kmin = a < kmin ? a : kmin;
            kmax = b > kmax ? b : kmax;
        }
        if (lane == 0) {
            atomicMin(&s_kmin, kmin);
            atomicMax(&s_kmax, kmax);
        }
    }
    __syncthreads();
    const uint32_t nloc = s_nloc;
    const bool local = nloc <= (uint32_t)kBuf;
    const unsigned long long kmin = s_kmin, kmax = s_kmax;
    int lo = kmin == kmax ? 0 : 64 - __clzll((long long)(kmin ^ kmax));  // the keys differ in their low `lo` bits only
    unsigned long long prefix = lo >= 64 ? 0ull : kmin >> lo;
    while (lo > 0) {  // block-uniform
        const int bits = min(11, lo), shift = lo - bits, nbins = 1 << bits;
        for (int i = tid; i < nbins; i += 1024) h[i] = 0;
        __syncthreads();
        auto take = [&](V x, bool ok) {
            const unsigned long long key = (unsigned long long)Traits<V>::key(x);
            if (ok && (lo >= 64 || (key >> lo) == prefix)) atomicAdd(&h[(uint32_t)(key >> shift) & (uint32_t)(nbins - 1)], 1u);
        };
        if (local) {
            for (uint32_t i = tid; i < nloc; i += 1024) take(s_buf[i], true);
        } else {
            for (uint32_t base = 0; base < cnt; base += 8192) {
                V x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t i = base + u * 1024 + tid;
                    x[u] = i < cnt ? L[i] : (V)-1;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) take(x[u], is_mine(x[u], base + u * 1024 + tid));
            }
        }
        __syncthreads();
        uint32_t d, rr;
        block_find_digit(h, nbins, r, wsum, found, d, rr);  // (threads 256.. hold no bins there)
        prefix = (prefix << bits) | d;
        r = rr;
        lo = shift;
    }
    if (tid == 0) os[bc * kMaxRanks + q] = Traits<V>::value((K)prefix);
    // pair != 0 (grid.y = queries / 2): the block also answers query q + 1 when it is the NEXT order statistic of the same
    // list (np.percentile's two neighbours, S6:196-197): one more pass -- how many elements are <= x_r, and the smallest one
    // above it -- instead of a second block repeating the whole select.
    if (!with_next) return;
    const int q1 = q + 1;
    if (s->gid[q1] != g || s->qbin[q1] != tb || s->rr[q1] - s->rr[q] > 1u) return;  // (answered by its own block: see the launch)
    if (s->rr[q1] == s->rr[q]) {
        if (tid == 0) os[bc * kMaxRanks + q1] = Traits<V>::value((K)prefix);
        return;
    }
    __syncthreads();
    if (tid == 0) {
        s_nloc = 0;      // elements <= x_r
        s_kmin = ~0ull;  // smallest key above x_r's
    }
    __syncthreads();
    {
        uint32_t cle = 0;
        unsigned long long kgt = ~0ull;
        auto look = [&](V x, bool ok) {
            const unsigned long long key = (unsigned long long)Traits<V>::key(x);
            if (ok) {
                if (key <= prefix) ++cle;
                else kgt = key < kgt ? key : kgt;
            }
        };
        if (local) {
            for (uint32_t i = tid; i < nloc; i += 1024) look(s_buf[i], true);
        } else {
            for (uint32_t base = 0; base < cnt; base += 1024) {
                const uint32_t i = base + tid;
                const V x = i < cnt ? L[i] : (V)-1;
                look(x, is_mine(x, i));
            }
        }
        cle = wave_sum_u32(cle);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long a = shfl_u64(kgt, lane ^ o);
            kgt = a < kgt ? a : kgt;
        }
        if (lane == 0) {
            atomicAdd(&s_nloc, cle);
            atomicMin(&s_kmin, kgt);
        }
    }
    __syncthreads();
    // x_r has rank r_mine among "mine": the next order statistic is x_r again if more than r_mine + 1 of them are <= x_r,
    // else the smallest element above it -- of the sub-bin, or (none left there) of the rest of the list: one more pass
    if (sub && s_nloc <= r_mine + 1u && s_kmin == ~0ull) {  // block-uniform
        unsigned long long kgt = ~0ull;
        for (uint32_t base = 0; base < cnt; base += 1024) {
            const uint32_t i = base + tid;
            if (i < cnt) {
                const unsigned long long key = (unsigned long long)Traits<V>::key(L[i]);
                if (key > prefix && key < kgt) kgt = key;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long a = shfl_u64(kgt, lane ^ o);
            kgt = a < kgt ? a : kgt;
        }
        if (lane == 0) atomicMin(&s_kmin, kgt);
        __syncthreads();
    }
    if (tid == 0) os[bc * kMaxRanks + q1] = Traits<V>::value((K)(s_nloc > r_mine + 1u ? prefix : s_kmin));
}

// profiler rows of the launches below that name V (the rows are matched by name: bench.py, profiles/f32t_stats.py)
template <typename V>
struct LinRows;
template <>
struct LinRows<float> {
    static constexpr const char *sample = "k_lin_sample<float>", *scan = "k_lin_scan<float>", *collect = "k_lin_collect<float>",
                                *collect_src = "(k_lin_collect_src<float, 4>)", *finish = "k_lin_finish<float>";
};
template <>
struct LinRows<double> {
    static constexpr const char *sample = "k_lin_sample<double>", *scan = "k_lin_scan<double>", *collect = "k_lin_collect<double>",
                                *collect_src = "k_lin_collect_src64", *finish = "k_lin_finish<double>";
};

}  // namespace

size_t select_ws_bytes(Shape s)
{
    Carver c(nullptr);
    SelectPlan plan;
    carve_select(c, s, true, &plan);
    return c.total();
}

// Before the producer: the plan, zeroed counters and (predict) the windows of bins predicted from a sample of *predict.
template <typename V>
int select_lin_begin(Shape s, const double *q_percent, int nq, void *ws, hipStream_t st, SelectPlan *plan, const RestoreSrc *predict)
{
    constexpr bool f64 = sizeof(V) == 8;
    int rc = plan_percentiles<V>(s, q_percent, nq, ws, true, plan);
    // only the first kLinBins counters of every (image, channel) are used by the producer (and kLinBins more by the sample)
    if (rc == UWIE_OK) rc = zero_ghist(*plan, s, st);
    if (rc != UWIE_OK) return rc;
    const int n = (int)s.npx(), nbc = s.B * 3;
    // ~128 K sample pixels per frame in evenly spaced groups of four (odd stride: no column is favoured): the
    // sampling error of a 1 % rank is ~0.03 % of the frame, half a bin where the 2048 bins are equally full
    const int ngroups = n / 4;
    // tuning (tests): lin_no_predict switches the prediction off, lin_predict_shift = k moves the predicted windows k bins
    // up (a large shift makes every prediction miss: collecting-sweep fallback).
    // The float64 terms.  nq <= 2 has to be there: the float64 producer files two windows at most (launch_recover64_planar_hist
    // refuses a larger plan) where the float32 one has a four-window variant.  ngroups > 0 need not differ: a plane of fewer
    // than four pixels gets no sample and so no window on either surface, every query takes the collecting sweep, and
    // `predicted` then only picks that sweep's grid (select_lin_run) and, in float32, opens the rank route, which asks for
    // four pixels itself.  Float32 has always said true there and float64 false; both are kept as they were.
    plan->predicted = predict && !tune().lin_no_predict && (!f64 || (nq <= 2 && ngroups > 0));
    uint32_t ns = 0;
    if (plan->predicted && ngroups > 0) {
        int stride = std::max(1, ngroups / 32768);
        if (stride > 1) stride |= 1;
        const int ngs = ngroups / stride;
        ns = 4u * (uint32_t)ngs;
        UWIE_LAUNCH_AS(LinRows<V>::sample, k_lin_sample<V>, dim3(std::max(1, std::min(8, cdiv(ngs, 512))), s.B), dim3(256), 0, st,
                       *predict, n, stride, ngs, plan->ghist);
        UWIE_LAUNCH_CHECK();
    }
    UWIE_LAUNCH(k_lin_predict, dim3(nbc), dim3(256), 0, st, plan->lin, plan->ghist, rank_list(*plan), (uint32_t)n, ns,
                tune().lin_predict_shift);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

// After the producer has filled the linear-digit histogram: scan -> one collecting sweep -> finish on the lists;
// planes whose list overflowed (a heavy bin, e.g. a constant image) take the key-digit passes.
template <typename V>
int select_lin_run(const SelectPlan &plan, const V *d_planar, Shape s, hipStream_t st, const RestoreSrc *src)
{
    using Rows = LinRows<V>;
    const int n = (int)s.npx(), nbc = s.B * 3;
    const RankList ranks = rank_list(plan);
    UWIE_REQUIRE(!src || ranks.n <= 4, "select_lin_run: the recomputing sweep handles at most two percentiles");
    V *lists = plan.lists_as<V>(), *os = (V *)plan.os;
    UWIE_LAUNCH_AS(Rows::scan, k_lin_scan<V>, dim3(nbc), dim3(256), 0, st, plan.lin, plan.ghist, ranks, os, plan.flags, plan.cap,
                   (SelState<typename Traits<V>::K> *)plan.state);
    UWIE_LAUNCH_CHECK();
    int blocks = (int)(((long long)n + 131071) / 131072);
    if (blocks * nbc < 1024) blocks = cdiv(1024, nbc);
    blocks = blocks < 1 ? 1 : blocks > 256 ? 256 : blocks;
    // after a prediction the sweep only serves the few planes it missed (a heavy bin next to the target made the
    // window's list overflow, or the sample was off); its blocks return at once for the others, and the ones that work
    // are alone on the chip: more, smaller blocks (4K x 64 with 4 such planes: 32 per plane 0.29 ms, 128: 0.12 ms)
    if (plan.predicted) blocks = std::max(1, std::min(2 * blocks, cdiv(24576, nbc)));
    if (src) {
        const int per_image = std::min(3 * blocks, std::max(1, cdiv(n, 2048)));
        UWIE_LAUNCH_AS(Rows::collect_src, (k_lin_collect_src<V, 4>), dim3(per_image, s.B), dim3(256), 0, st, *src, n, plan.lin, lists,
                       plan.cap);
    } else {
        UWIE_LAUNCH_AS(Rows::collect, k_lin_collect<V>, dim3(blocks, nbc), dim3(256), 0, st, d_planar, n, plan.lin, lists, plan.cap);
    }
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH_AS(Rows::finish, k_lin_finish<V>, dim3(nbc, ranks.n), dim3(1024), 0, st, plan.lin, lists, plan.cap, os,
                   plan.flags, 0, kLinLists);
    UWIE_LAUNCH_CHECK();
    // the flagged planes: the key-digit passes over their recomputed or stored values (they return at once for the others)
    if (src) return sel_passes(plan, RestoredVals<V>{*src, n}, n, nbc, pass_blocks(n, nbc, true), false, plan.flags, st);
    const StoredVals<V> vals{d_planar, (size_t)n * 3, (size_t)n, 1};
    return sel_passes(plan, vals, n, nbc, pass_blocks(n, nbc, false), false, plan.flags, st);
}

template int select_lin_begin<float>(Shape, const double *, int, void *, hipStream_t, SelectPlan *, const RestoreSrc *);
template int select_lin_run<float>(const SelectPlan &, const float *, Shape, hipStream_t, const RestoreSrc *);
template int select_lin_begin<double>(Shape, const double *, int, void *, hipStream_t, SelectPlan *, const RestoreSrc *);
template int select_lin_run<double>(const SelectPlan &, const double *, Shape, hipStream_t, const RestoreSrc *);

// After launch_restore_rank: scan -> finish on the window lists; flagged planes take the key-digit passes.
int select_rank_run(const SelectPlan &plan, Shape s, hipStream_t st, const RestoreSrc &src)
{
    const int n = (int)s.npx(), nbc = s.B * 3;
    const RankList ranks = rank_list(plan);
    UWIE_LAUNCH(k_rank_scan, dim3(cdiv(nbc, 64)), dim3(64), 0, st, plan.lin, ranks, (float *)plan.os, plan.flags, kRankCapMul * plan.cap,
                nbc, (SelState<uint32_t> *)plan.state);
    UWIE_LAUNCH_CHECK();
    UWIE_LAUNCH(k_lin_finish<float>, dim3(nbc, ranks.n), dim3(1024), 0, st, plan.lin, plan.lists_as<float>(),
                kRankCapMul * plan.cap, (float *)plan.os, plan.flags, 1, kLinLists / kRankCapMul);
    UWIE_LAUNCH_CHECK();
    return sel_passes(plan, RestoredVals<float>{src, n}, n, nbc, pass_blocks(n, nbc, true), false, plan.flags, st);
}

int select_begin_stretch_ranks(Shape s, const float *d_params, int stride, void *ws, hipStream_t st, SelectPlan *plan)
{
    return begin_ranks(s, "stretch ranks: plane size out of range", ws, st, plan, [&](SelState<uint32_t> *state, int nbc, int n) {
        UWIE_LAUNCH(k_sel_init_stretch_ranks, dim3(cdiv(nbc, 64)), dim3(64), 0, st, state, nbc, d_params, stride, n);
    });
}

int select_begin_gated_ranks(Shape s, const float *d_params, int stride, uint32_t *d_status, void *ws, hipStream_t st,
                             SelectPlan *plan)
{
    return begin_ranks(s, "gated ranks: plane size out of range", ws, st, plan, [&](SelState<uint32_t> *state, int nbc, int n) {
        UWIE_LAUNCH(k_sel_init_gated_ranks, dim3(cdiv(nbc, 64)), dim3(64), 0, st, state, nbc, d_params, stride, n, d_status);
    });
}

int select_lerp_chain(const SelectPlan &plan, Shape s, float eps, float *d_pct4, hipStream_t st)
{
    UWIE_REQUIRE(plan.nq == 4 && !plan.is64, "chained stretch needs 4 float32 percentiles");
    FracList<float> fr;
    fr.n = 4;
    for (int j = 0; j < 4; ++j) fr.t[j] = (float)plan.t[j];
    const int nbc = s.B * 3;
    UWIE_LAUNCH(k_pct_finish_chain, dim3(cdiv(nbc, 64)), dim3(64), 0, st, (const float *)plan.os, nbc, fr, eps, d_pct4);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

// ===================================================================================== the key-digit route on stored values
template <typename V>
int select_begin(Shape s, const double *q_percent, int nq, void *ws, hipStream_t st, SelectPlan *plan)
{
    using K = typename Traits<V>::K;
    const int rc = plan_percentiles<V>(s, q_percent, nq, ws, false, plan);
    if (rc != UWIE_OK) return rc;
    const int nbc = s.B * 3;
    UWIE_LAUNCH(k_sel_init<K>, dim3(cdiv(nbc, 64)), dim3(64), 0, st, (SelState<K> *)plan->state, nbc, rank_list(*plan));
    UWIE_LAUNCH_CHECK();
    return zero_ghist(*plan, s, st);
}

template <typename V>
int select_run(const SelectPlan &plan, const V *d_vals, int planar, Shape s, bool pass1_done, hipStream_t st)
{
    const int n = (int)s.npx(), nbc = s.B * 3;
    const StoredVals<V> src{d_vals, (size_t)n * 3, planar ? (size_t)n : (size_t)1, planar ? 1 : 3};
    return sel_passes(plan, src, n, nbc, pass_blocks(n, nbc, false), pass1_done, nullptr, st);
}

template <typename V>
int select_lerp(const SelectPlan &plan, Shape s, V *d_out, hipStream_t st)
{
    FracList<V> fr;
    fr.n = plan.nq;
    for (int j = 0; j < plan.nq; ++j) fr.t[j] = (V)plan.t[j];
    const int nbc = s.B * 3;
    UWIE_LAUNCH(k_pct_finish<V>, dim3(cdiv(nbc * plan.nq, 64)), dim3(64), 0, st, (const V *)plan.os, nbc, fr, d_out);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

template <typename V>
int launch_percentiles(const V *d_vals, int planar, Shape s, const double *q_percent, int nq, V *d_out, void *ws, hipStream_t st)
{
    SelectPlan plan;
    int rc = select_begin<V>(s, q_percent, nq, ws, st, &plan);
    if (rc != UWIE_OK) return rc;
    rc = select_run(plan, d_vals, planar, s, false, st);
    if (rc != UWIE_OK) return rc;
    return select_lerp(plan, s, d_out, st);
}

template int select_begin<float>(Shape, const double *, int, void *, hipStream_t, SelectPlan *);
template int select_begin<double>(Shape, const double *, int, void *, hipStream_t, SelectPlan *);
template int select_run<float>(const SelectPlan &, const float *, int, Shape, bool, hipStream_t);
template int select_run<double>(const SelectPlan &, const double *, int, Shape, bool, hipStream_t);
template int select_lerp<float>(const SelectPlan &, Shape, float *, hipStream_t);
template int select_lerp<double>(const SelectPlan &, Shape, double *, hipStream_t);
template int launch_percentiles<float>(const float *, int, Shape, const double *, int, float *, void *, hipStream_t);
template int launch_percentiles<double>(const double *, int, Shape, const double *, int, double *, void *, hipStream_t);

namespace {
__global__ void k_widen_f32(const float *__restrict__ in, double *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}
}  // namespace

int launch_widen_f32(const float *d_in, double *d_out, size_t n, hipStream_t st)
{
    if (n == 0) return UWIE_OK;
    UWIE_LAUNCH(k_widen_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_in, d_out, n);
    UWIE_LAUNCH_CHECK();
    return UWIE_OK;
}

}  // namespace uwie
