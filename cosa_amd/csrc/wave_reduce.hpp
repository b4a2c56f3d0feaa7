// wave_reduce.hpp -- the order-independent wave-level pieces of the monitor and check kernels, once: integer sums, maxima and ORs over a
// wavefront, the floating-point maximum, the wave-aggregated count, the non-finite bit test and the closing step that sends a workgroup's
// LDS counters to global memory.  Every result is the same bits whatever the order of the lanes and of the wavefronts.  Floating-point SUMS
// are not here: their order is part of their bits, and each stays with the kernel that defines it.
#pragma once
#include "common.hpp"

namespace cosa {
namespace {

__device__ __forceinline__ bool nonfinite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the butterflies: every lane of the wavefront must make the call, every lane holds the result
__device__ __forceinline__ unsigned wave_sum32(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, d), hi = __shfl_xor((unsigned)(v >> 32), d);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_max32(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_or32(unsigned v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d);
    return v;
}

// fmax drops a NaN: none leaves a maximum that something else entered
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

// ctr[slot] += 1 for every lane with `valid`, one atomic per distinct slot of the wavefront (a crop holds a handful of labels: a
// plain atomic per lane would serialise 64 deep on one address).  `todo` is wave-uniform, so every lane leaves the loop together.
// T: unsigned long long or unsigned int counters, in LDS or in global memory.  Every lane of the wavefront must make the call.
template <typename T>
__device__ __forceinline__ void wave_count(T *ctr, int slot, bool valid)
{
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const int s = __builtin_amdgcn_readlane(slot, leader);
        const unsigned long long same = __ballot(valid && slot == s);
        if ((int)__lane_id() == leader) atomicAdd(&ctr[s], (T)__popcll(same));
        todo &= ~same;
    }
}

// wave_count for slots that may be many per wavefront (a [K][K] matrix under a speckled map): the two most wanted slots -- the leaders' --
// leave aggregated as above, what is left after them adds one by one, where few lanes share an address.  The same sums.
template <typename T>
__device__ __forceinline__ void wave_count_mixed(T *ctr, int slot, bool valid)
{
    unsigned long long todo = __ballot(valid);
    for (int round = 0; round < 2 && todo; round++) {
        const int leader = __ffsll(todo) - 1;
        const int s = __builtin_amdgcn_readlane(slot, leader);
        const unsigned long long same = __ballot(valid && slot == s);
        if ((int)__lane_id() == leader) atomicAdd(&ctr[s], (T)__popcll(same));
        valid = valid && slot != s;
        todo &= ~same;
    }
    if (valid) atomicAdd(&ctr[slot], (T)1);
}

struct NeverMax {
    __device__ __forceinline__ bool operator()(int) const { return false; }
};

// The closing step of a monitor kernel, after the barrier behind the last LDS update: the workgroup's `threads` threads send the LDS words
// lds[0 .. words) to out[0 .. words), word i by atomicMax where is_max(i) and by atomicAdd elsewhere.  A zero word is skipped: it changes
// neither a sum nor a maximum.
template <typename L, typename IsMax = NeverMax>
__device__ __forceinline__ void flush_counters(const L *lds, unsigned long long *out, int words, int threads, IsMax is_max = IsMax())
{
    for (int i = threadIdx.x; i < words; i += threads) {
        const unsigned long long v = lds[i];
        if (!v) continue;
        if (is_max(i)) atomicMax(&out[i], v); else atomicAdd(&out[i], v);
    }
}

}  // namespace
}  // namespace cosa
