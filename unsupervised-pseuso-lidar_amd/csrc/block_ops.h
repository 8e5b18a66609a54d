// Workgroup primitives of the kernels: sum, scan, ballot count and rank, the one-workgroup scan of per-block counts, the radix-select step.
// Device only: the .hip files include it, the *_math.h headers that the host checks compile never do.  WAVES is the workgroup's size in
// wavefronts (4 for 256 threads, 16 for 1024); s is WAVES entries of LDS.
#pragma once
#include "mcav_common.h"

namespace mcav {

// Sum over the 64 lanes of a wavefront; every lane gets the total.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sum over the workgroup in a fixed order -- the butterfly inside each wave, then the wave totals from left to right; every thread gets
// the total.  Safe to call again with the same s: the first barrier ends the previous call's reads.
template <typename T, int WAVES>
__device__ __forceinline__ T block_sum(T v, T* s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = s[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t += s[w];
    return t;
}

// Exclusive scan over the workgroup's threads; total: the workgroup's sum, in every thread.  The barriers sit as in block_sum (before s
// is written, and between the write and the reads), so it is safe to call again with the same s.
template <typename T, int WAVES>
__device__ __forceinline__ T block_scan(T v, T* s, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T a = __shfl_up(inc, off, 64);
        if (lane >= off) inc += a;
    }
    __syncthreads();
    if (lane == 63) s[wave] = inc;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before += s[w];
        total += s[w];
    }
    return before + inc - v;
}

// s[0] + ... + s[N - 1] as a tree, (s0 + s1) + (s2 + s3), N a power of two
template <int N>
__device__ __forceinline__ unsigned pairwise_sum(const unsigned* s) {
    if constexpr (N == 1) return s[0];
    else return pairwise_sum<N / 2>(s) + pairwise_sum<N / 2>(s + N / 2);
}

// The flags of a workgroup: how many are set, and how many are set in the threads before this one.  One barrier, after s is written: a
// second call with the same s needs a barrier of the caller's in front of it.
template <int WAVES>
__device__ __forceinline__ unsigned block_count(bool flag, unsigned* s) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    return pairwise_sum<WAVES>(s);
}
template <int WAVES>
__device__ __forceinline__ unsigned block_rank(bool flag, unsigned* s) {
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += s[w];
    return before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// ONE workgroup scans n entries, WAVES * 64 per pass, the carry in a register: store(i, the sum of load(0 .. i - 1)) for every i < n;
// returns the total in every thread.  load and store may name the same array.
template <typename T, int WAVES, class Load, class Store>
__device__ __forceinline__ T chunked_scan(int n, T* s, Load load, Store store) {
    T carry = 0;
    for (int base = 0; base < n; base += WAVES * 64) {
        const int i = base + (int)threadIdx.x;
        T total;
        const T ex = block_scan<T, WAVES>(i < n ? load(i) : T(0), s, total);
        if (i < n) store(i, carry + ex);
        carry += total;
    }
    return carry;
}

// ---------------------------------------------------------------------------------------------- radix select
// The element of rank k among 32-bit keys, exactly, in three passes over 2048-bin histograms: 11 + 11 + 10 bits from the top.  Pass p
// counts digit (key >> shift) & dmask of the keys whose earlier digits (key & pmask) match the prefix found so far.
constexpr int RADIX_PASSES = 3, RADIX_BINS = 2048;
__constant__ const int radix_shift[RADIX_PASSES] = {21, 10, 0};
__constant__ const int radix_width[RADIX_PASSES] = {11, 11, 10};

struct RadixPass {
    int shift;
    unsigned dmask, pmask;
};
__device__ __forceinline__ RadixPass radix_pass(int p) {
    const int shift = radix_shift[p], top = shift + radix_width[p];
    return RadixPass{shift, (1u << radix_width[p]) - 1u, top >= 32 ? 0u : ~0u << top};
}

// The bin that holds rank k.  Thread t holds the counts c of bins t * PER ... t * PER + PER - 1; true in the one thread that holds the
// bin (none if k is not below the sum of all bins), with pick = the bin and left = the rank inside it.
template <int PER, int WAVES>
__device__ __forceinline__ bool pick_bin(const unsigned (&c)[PER], unsigned k, unsigned* s, unsigned& pick, unsigned& left) {
    unsigned sum = 0, total;
#pragma unroll
    for (int j = 0; j < PER; ++j) sum += c[j];
    unsigned before = block_scan<unsigned, WAVES>(sum, s, total);
    if (k < before || k >= before + sum) return false;
    unsigned j = 0;
#pragma unroll
    for (int e = 0; e < PER - 1; ++e)
        if (j == (unsigned)e && before + c[e] <= k) { before += c[e]; ++j; }
    pick = threadIdx.x * PER + j;
    left = k - before;
    return true;
}

}  // namespace mcav
