// act_stats_kernels.hip -- the --act_stats_iters monitor: what the activations of an fp32 no-grad pass look like to
// an fp16 split (range) and how sharp its attention is (logit magnitude, row entropy).  Two reductions over the plain fp32 buffers of the
// "f32" operand family (csrc/f32_kernels.hip), accumulated on the device into int64 words (include/cosa_hip.h: the layouts).
//
//   cosa_range_stats_f32   one streaming pass over a column window of an fp32 matrix: finite / over 65504 / over 32768 / below 2^-14 /
//                          non-finite counts and the largest finite |x|
//   cosa_attn_stats_f32    the QK^T half of attn_fwd_f32_kernel (f32_attn_tile.hpp: the same code) without the PV product: per head
//                          the mean normalised row entropy, the mean top-1 probability, the peaked rows, the largest |logit|
//
// Everything that is added is an integer: counts, and per-row terms in 64-bit fixed point (rint of the term times 2^32 in double, once per
// row).  Every maximum is an integer maximum of the bit pattern of a finite non-negative fp32 value.  So the words do not depend on the order
// in which the wavefronts arrive: the same inputs give the same bytes on every run, and a second call on a table that was not zeroed
// doubles counts and sums and keeps maxima.  Built with -ffp-contract=off: what is an fma here is written fmaf / fma.
#include "wave_reduce.hpp"
#include "f32_attn_tile.hpp"

namespace cosa {
namespace {

typedef unsigned long long u64;

constexpr unsigned kAbsMask = 0x7fffffffu, kInfBits = 0x7f800000u;
constexpr unsigned kF16MaxBits = 0x477fe000u;        // 65504.0f: the largest finite fp16
constexpr unsigned kF16HalfBits = 0x47000000u;       // 32768.0f: one bit of headroom left
constexpr unsigned kF16MinNormalBits = 0x38800000u;  // 2^-14: below it the fp16 hi half is subnormal

// ---- range -------------------------------------------------------------------------------------------------------------------------------
enum { rFinite = 0, rAbsMax, rOver, rNear, rTiny, rNonFinite, rWords };

struct RangeAcc {
    unsigned finite = 0, over = 0, near = 0, tiny = 0, bad = 0, amax = 0;          // (a thread sees far fewer than 2^32 elements)

    __device__ __forceinline__ void add(float x)
    {
        const unsigned a = __float_as_uint(x) & kAbsMask;          // |x| as bits: ordered like the values for everything finite
        const bool fin = a < kInfBits;                             // (branch-free: one counter per class, no indexed pair)
        finite += fin ? 1u : 0u;
        bad += fin ? 0u : 1u;
        amax = (fin && a > amax) ? a : amax;
        over += (fin && a > kF16MaxBits) ? 1u : 0u;
        near += (fin && a > kF16HalfBits) ? 1u : 0u;
        tiny += (a != 0u && a < kF16MinNormalBits) ? 1u : 0u;
    }
};

// the elements [c0, c0 + W * per_row) of rows r0 .. r1 - 1, W floats per load: the threads walk (row, slot) pairs in steps of the block size
template <int W>
__device__ __forceinline__ void range_scan(RangeAcc &acc, const float *__restrict__ x, long long r0, long long r1, long long ld, int c0, int per_row)
{
    if (per_row < 1) return;
    long long row = r0;
    int v = threadIdx.x;
    while (v >= per_row) {
        v -= per_row;
        row++;
    }
    while (row < r1) {
        const float *p = x + row * ld + c0 + (long long)v * W;
        if (W == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(p);
            acc.add(q.x); acc.add(q.y); acc.add(q.z); acc.add(q.w);
        } else {
            acc.add(*p);
        }
        v += blockDim.x;
        while (v >= per_row) {
            v -= per_row;
            row++;
        }
    }
}

__global__ __launch_bounds__(256) void range_stats_f32_kernel(const float *__restrict__ x, long long rows, int cols, long long ld, long long chunk,
                                                              int vec, u64 *__restrict__ out)
{
    __shared__ u64 red[rWords];
    if (threadIdx.x < rWords) red[threadIdx.x] = 0;
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    RangeAcc acc;
    if (vec) {                                   // 16-byte aligned row starts: float4 over the whole quads, the last cols % 4 columns alone
        range_scan<4>(acc, x, r0, r1, ld, 0, cols >> 2);
        range_scan<1>(acc, x, r0, r1, ld, cols & ~3, cols & 3);
    } else {
        range_scan<1>(acc, x, r0, r1, ld, 0, cols);
    }
    const u64 n_fin = wave_sum64(acc.finite), n_over = wave_sum64(acc.over), n_near = wave_sum64(acc.near), n_tiny = wave_sum64(acc.tiny),
              n_bad = wave_sum64(acc.bad), amax = wave_max32(acc.amax);
    if ((threadIdx.x & 63) == 0) {
        if (n_fin) atomicAdd(&red[rFinite], n_fin);
        if (amax) atomicMax(&red[rAbsMax], amax);
        if (n_over) atomicAdd(&red[rOver], n_over);
        if (n_near) atomicAdd(&red[rNear], n_near);
        if (n_tiny) atomicAdd(&red[rTiny], n_tiny);
        if (n_bad) atomicAdd(&red[rNonFinite], n_bad);
    }
    __syncthreads();
    flush_counters(red, out, rWords, 256, [](int i) { return i == rAbsMax; });
}

// ---- attention -----------------------------------------------------------------------------------------------------------------------------
// As attn_fwd_f32_kernel (csrc/f32_kernels.hip), through the calls of f32_attn_tile.hpp:
// one block = 128 queries of one (batch, head) slice, 4 waves of 32 queries, key tiles of 32
// through LDS, S^T[key][query] = K[key][d] Q^T[d][query] on the f32-input MFMA with Q held in 32 VGPRs, the chain over d ascending.  A
// lane's column is its query; the two lane halves hold different keys of the same query and share one maximum per tile.  Per query the
// kernel carries the running maximum m (fp32, as the softmax sees it) and, in double so that no summation order shows,
//     l = sum e^(s - m),   t = sum e^(s - m) (s - m)            (e^ is expf of the fp32 difference, as in the forward kernel)
// with l <- alpha l, t <- alpha (t + (m - m') l), alpha = e^(m - m'), when m rises to m'.  A row ends as H = log l - t / l.
enum { aRows = 0, aEntFix, aTop1Fix, aPeaked, aSmax, aSharp, aNonFiniteRows, aWords };

__global__ __launch_bounds__(256) void attn_stats_f32_kernel(const float *__restrict__ qkv, u64 *__restrict__ out, int N, int H, float scale,
                                                             long long ldq)
{
    __shared__ float Ks[AK][K_LD];
    __shared__ u64 red[aWords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    if (tid < aWords) red[tid] = 0;                // (ordered before its first use by the barriers of the tile loop)
    const float *base = qkv + (size_t)b * N * ldq;
    const float *qp = base + (size_t)head * HD, *kp = base + (size_t)(H + head) * HD;
    const int query = blockIdx.x * AQ + wave * 32 + (lane & 31);

    float qreg[HD / 2];
    attn_load_q(qp, query, N, ldq, half, qreg);

    float m = -INFINITY;
    double l = 0.0, t = 0.0;
    unsigned smax = 0, bad = 0;

    float4 rk[2];          // staging: keys past N are zeros and are masked below

    const int tiles = (N + AK - 1) / AK;
    attn_load_rows(kp, 0, N, ldq, tid, rk);
    attn_store_k(Ks, tid, rk);
    __syncthreads();
    for (int kt = 0; kt < tiles; kt++) {
        if (kt + 1 < tiles) attn_load_rows(kp, (kt + 1) * AK, N, ldq, tid, rk);
        f32x16 s = attn_scores(Ks, qreg, lane);
        const float mx = attn_mask_max(s, kt * AK, N, scale, lane, [&](float v, bool live) {
            const unsigned a = __float_as_uint(v) & kAbsMask;
            if (live) {
                if (a >= kInfBits) bad = 1; else smax = a > smax ? a : smax;
            }
        });
        const float m_new = fmaxf(m, mx);                                    // finite from the first tile on: key 0 exists
        const float alpha = expf(m - m_new);                                 // (first tile: expf(-inf) = 0 on l = 0, t = 0)
        const float dm = m == -INFINITY ? 0.f : m - m_new;                   // (... whose -inf must not meet that 0)
        double psum = 0.0, tsum = 0.0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const bool live = kt * AK + cd_row(r, lane) < N;
            const float d = live ? s[r] - m_new : 0.f, p = live ? expf(d) : 0.f;
            psum += (double)p;
            tsum = fma((double)p, (double)d, tsum);
        }
        t = fma((double)alpha, fma((double)dm, l, t), tsum);
        l = fma(l, (double)alpha, psum);
        m = m_new;
        __syncthreads();
        if (kt + 1 < tiles) {
            attn_store_k(Ks, tid, rk);
            __syncthreads();
        }
    }
    // the two halves of a query meet: its sums, its largest logit, whether any of its logits was non-finite
    l += __shfl_xor(l, 32, 64);
    t += __shfl_xor(t, 32, 64);
    const unsigned smax2 = __shfl_xor(smax, 32, 64), bad2 = __shfl_xor(bad, 32, 64);
    smax = smax2 > smax ? smax2 : smax;
    bad |= bad2;

    const bool mine = half == 0 && query < N, good = mine && !bad;         // one lane per query counts it
    u64 ent = 0, top = 0;
    unsigned peaked = 0, sharp = 0;
    if (good) {
        double hn = N > 1 ? (log(l) - t / l) / log((double)N) : 0.0;
        hn = hn < 0.0 ? 0.0 : hn > 1.0 ? 1.0 : hn;                       // (rounding may leave a one-hot row at -1e-17)
        const double top1 = 1.0 / l;                                        // (l >= 1: the maximum's own term)
        ent = (u64)llrint(ldexp(hn, 32));
        top = (u64)llrint(ldexp(top1, 32));
        peaked = top1 > 0.5 ? 1u : 0u;
        sharp = __float_as_uint((float)(1.0 - hn));
    }
    const u64 w[aWords] = {wave_sum64(good ? 1u : 0u), wave_sum64(ent), wave_sum64(top), wave_sum64(peaked), wave_max32(good ? smax : 0u),
                           wave_max32(sharp), wave_sum64(mine && bad ? 1u : 0u)};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < aWords; i++) {
            if (!w[i]) continue;
            if (i == aSmax || i == aSharp) atomicMax(&red[i], w[i]); else atomicAdd(&red[i], w[i]);
        }
    }
    __syncthreads();
    flush_counters(red, out + (size_t)head * aWords, aWords, 256, [](int i) { return i == aSmax || i == aSharp; });
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_range_stats_f32(const float *x, long long rows, int cols, long long ld, int64_t *out6, void *stream)
{
    COSA_REQUIRE(x && out6, "cosa_range_stats_f32: null operand");
    COSA_REQUIRE(rows >= 1 && cols >= 1 && ld >= cols, "cosa_range_stats_f32: rows >= 1, cols >= 1, ld >= cols (got rows=%lld cols=%d ld=%lld)", rows,
                 cols, ld);
    COSA_REQUIRE((reinterpret_cast<uintptr_t>(out6) & 7) == 0, "cosa_range_stats_f32: the output words must be 8-byte aligned");
    const long long want = rows < 2048 ? rows : 2048, chunk = (rows + want - 1) / want, blocks = (rows + chunk - 1) / chunk;
    const int vec = aligned16(x) && ld % 4 == 0 && cols >= 4;
    hipLaunchKernelGGL(range_stats_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, rows, cols, ld, chunk, vec,
                       reinterpret_cast<u64 *>(out6));
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_attn_stats_f32(const float *qkv, int B, int N, int H, int head_dim, float scale, long long ldq, int64_t *out, void *stream)
{
    COSA_REQUIRE(qkv && out, "cosa_attn_stats_f32: null operand");
    COSA_REQUIRE(B >= 1 && N >= 1 && H >= 1 && head_dim == HD, "cosa_attn_stats_f32: head_dim must be 64 (got B=%d N=%d H=%d d=%d)", B, N, H, head_dim);
    COSA_REQUIRE(ldq >= 3ll * H * HD && ldq % 4 == 0 && aligned16(qkv),
                 "cosa_attn_stats_f32: token rows of stride ldq >= 3*H*64 in multiples of 4, 16-byte aligned base");
    COSA_REQUIRE(H <= 65535 && B <= 65535, "cosa_attn_stats_f32: too many heads / images for one launch");
    COSA_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0, "cosa_attn_stats_f32: the output words must be 8-byte aligned");
    hipLaunchKernelGGL(attn_stats_f32_kernel, dim3((N + AQ - 1) / AQ, H, B), dim3(256), 0, as_stream(stream), qkv, reinterpret_cast<u64 *>(out), N, H,
                       scale, ldq);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
