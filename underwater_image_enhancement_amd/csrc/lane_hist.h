// The lane-column byte histogram: a 3 x 256 histogram of RGB bytes taken by a block of 256 threads with LDS atomics that
// never conflict, whatever the picture (k_chunk_hist, k_chunk_hist_quad, k_q_hist, k_hist_strong).
//
// One 32-bit word per (byte value, lane column), the three channels' counters in 10-bit fields of that word: R in bits 0-9,
// G in 10-19, B in 20-29.  Word (value, column) sits at byte value * 128 + column * 4 of the 32 KB array, so the LDS bank of
// an atomic is the lane's column (lane & 31 -- `ds_add_u32` is serviced in the two 32-lane halves, banks (a / 4) mod 32),
// never the pixel's value: no bank conflicts, where value-indexed copies spent 72 % of their LDS cycles on conflicts
// (neighbouring pixels share their values).
//
// A field holds 1023, so a column (eight of the block's 256 threads) may receive at most 1023 pixels between two folds:
// every user states that bound for its own loop in a static_assert next to it.  A fold adds the 32 columns of a value into
// three 32-bit counts, thread v taking value v, and starts at a rotated column so that neighbouring lanes read different
// banks.
#pragma once
#include "devutil.h"

namespace uwie {

constexpr int kLaneHistCols = 32;
constexpr int kLaneHistWords = 256 * kLaneHistCols;  // the LDS array: __shared__ __attribute__((aligned(16))) uint32_t h[kLaneHistWords]
constexpr int kLaneHistField = 1023;                 // largest count of a field

struct LaneHist {
    uint32_t (&h)[kLaneHistWords];  // the LDS array
    uint32_t colb;  // byte offset of this lane's column inside a value's 128 bytes

    __device__ __forceinline__ LaneHist(uint32_t (&h)[kLaneHistWords], int tid) : h(h), colb((uint32_t)(tid & (kLaneHistCols - 1)) * 4u) {}

    // all threads, before the first use (no barrier: the caller's)
    static __device__ __forceinline__ void zero(uint32_t (&h)[kLaneHistWords], int tid)
    {
        for (int i = tid; i < kLaneHistWords / 4; i += 256) reinterpret_cast<uint4 *>(h)[i] = make_uint4(0, 0, 0, 0);
    }
    // byte address of (value, column): value * 128 + column * 4; the caller shifts the value's byte to bit 7 of `moved`
    __device__ __forceinline__ void bump(uint32_t moved, uint32_t inc) const
    {
        atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(h) + ((moved & 0x7f80u) | colb)), inc);
    }
    static constexpr uint32_t kR = 1u, kG = 1u << 10, kB = 1u << 20;
    // four pixels from three dwords: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
    __device__ __forceinline__ void add4(uint32_t c0, uint32_t c1, uint32_t c2) const
    {
        bump(c0 << 7, kR); bump(c0 >> 1, kG); bump(c0 >> 9, kB);
        bump(c0 >> 17, kR); bump(c1 << 7, kG); bump(c1 >> 1, kB);
        bump(c1 >> 9, kR); bump(c1 >> 17, kG); bump(c2 << 7, kB);
        bump(c2 >> 1, kR); bump(c2 >> 9, kG); bump(c2 >> 17, kB);
    }
    // one pixel at p (R, G, B bytes)
    __device__ __forceinline__ void add1(const uint8_t *p) const
    {
        bump((uint32_t)p[0] << 7, kR); bump((uint32_t)p[1] << 7, kG); bump((uint32_t)p[2] << 7, kB);
    }
    // Thread v = tid adds the 32 columns of value v (after a barrier of the caller's) -> (R, G, B) counts.  One column per LDS
    // instruction, lane l starting at bank l; the words stay.  (The folds return their counts: written through reference
    // parameters, the b128 one cost k_chunk_hist_quad and k_hist_strong 40 more VGPRs and a wavefront of occupancy.)
    static __device__ __forceinline__ uint3 fold_b32(uint32_t (&h)[kLaneHistWords], int tid)
    {
        uint32_t r = 0, g = 0, b = 0;
#pragma unroll 8
        for (int k = 0; k < kLaneHistCols; ++k) {
            const uint32_t w = h[tid * kLaneHistCols + ((tid + k) & (kLaneHistCols - 1))];
            r += w & 1023u;
            g += (w >> 10) & 1023u;
            b += w >> 20;
        }
        return make_uint3(r, g, b);
    }
    // The same with four columns per LDS instruction, cleared on the way; the quads are taken in a rotated order (eight
    // neighbouring lanes cover the 32 banks).  A quarter of the LDS instructions of the b32 form, which made the two folds of a
    // chunk cost as much as a third of its atomics.
    static __device__ __forceinline__ uint3 fold_b128(uint32_t (&h)[kLaneHistWords], int tid)
    {
        uint32_t r = 0, g = 0, b = 0;
#pragma unroll
        for (int k = 0; k < kLaneHistCols / 4; ++k) {
            uint4 *wq = reinterpret_cast<uint4 *>(&h[tid * kLaneHistCols + 4 * ((tid + k) & (kLaneHistCols / 4 - 1))]);
            const uint4 w = *wq;
            *wq = make_uint4(0, 0, 0, 0);
            r += (w.x & 1023u) + (w.y & 1023u) + (w.z & 1023u) + (w.w & 1023u);
            g += ((w.x >> 10) & 1023u) + ((w.y >> 10) & 1023u) + ((w.z >> 10) & 1023u) + ((w.w >> 10) & 1023u);
            b += (w.x >> 20) + (w.y >> 20) + (w.z >> 20) + (w.w >> 20);
        }
        return make_uint3(r, g, b);
    }
    // All threads, between batches: fold_b128 into the block's 32-bit totals cnt[3][256] (LDS), barriers included
    static __device__ __forceinline__ void fold_totals(uint32_t (&h)[kLaneHistWords], int tid, uint32_t (&cnt)[768])
    {
        __syncthreads();
        const uint3 f = fold_b128(h, tid);
        cnt[tid] += f.x; cnt[256 + tid] += f.y; cnt[512 + tid] += f.z;
        __syncthreads();
    }
    // the block's 768 totals added to histogram `slot` of hist[][3][256] in global memory (after fold_totals)
    static __device__ __forceinline__ void flush(int tid, const uint32_t *cnt, uint32_t *hist, size_t slot)
    {
        for (int i = tid; i < 768; i += 256)
            if (cnt[i]) atomicAdd(&hist[slot * 768 + i], cnt[i]);
    }
};

}  // namespace uwie
