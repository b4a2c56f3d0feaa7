// optim_kernels.hip -- one pass over the parameters per training step (gfx950, HBM-bound).
//
// Reference: utils/torch_helper.py:261-293 (PolyWarmupAdamW = torch AdamW with a scheduled LR), main.py:250-252 (EMA of
// the teacher, a Python loop over ~150 tensors).  Here AdamW, the EMA update and the refresh of the bf16 shadow copies that
// the forward passes read are ONE multi-tensor kernel: per parameter 20 B read (p, g, m, v, teacher) and 20 B written
// (p, m, v, teacher, 2 x bf16) instead of four separate sweeps (~72 B).  Frozen tensors (grad == NULL) only take the EMA.
#include "kernels.hpp"

#include <cmath>
#include <cstddef>
#include <mutex>
#include <vector>

namespace cosa {
namespace {

typedef __bf16 bf16;

struct TensorRec {          // one record per parameter tensor (device table)
    float *p;               // student master
    const float *g;         // gradient or NULL (frozen)
    float *m, *v;           // AdamW moments
    float *tp;              // teacher master
    bf16 *p16, *t16;        // bf16 shadows or NULL
    float lr, wd;           // per-group hyper-parameters (already scheduled)
    long long n;
    int t16_f16, p16_f16;   // the shadow's 16-bit type: 0 bf16, 1 IEEE fp16 (fp16-operand teacher passes)
};

struct ChunkRec { int tensor; int chunk; };

__device__ __forceinline__ uint2 pack16x4(const float (&v)[4], int f16)
{
    if (f16) {
        _Float16 o[4] = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        return *reinterpret_cast<uint2 *>(o);
    }
    bf16 o[4] = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    return *reinterpret_cast<uint2 *>(o);
}
__device__ __forceinline__ void store16(bf16 *dst, float v, int f16)
{
    if (f16) *reinterpret_cast<_Float16 *>(dst) = (_Float16)v;
    else *dst = (bf16)v;
}
constexpr int kChunk = 65536;            // elements per block

// The gradient guard: what grad_norm_finalize_kernel leaves for the guarded optimizer kernel, and the running
// counters of a run.  40 bytes, 8-byte aligned (include/cosa_hip.h).
struct GuardRec {
    float norm;             // global L2 norm of all gradients of the step (non-finite exactly when some gradient element is)
    float coef;             // min(1, max_norm / (norm + 1e-6)); 1 when clipping is off
    int skip;               // 1: the step is refused (skip_nonfinite and a non-finite norm)
    int pad;
    long long applied, skipped, clipped;
};

// GUARDED: every gradient element is multiplied by `coef` first (exact for coef == 1: same bits as the unguarded kernel)
template <bool GUARDED>
__device__ __forceinline__ void adamw_ema_body(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks, float beta1, float beta2,
                                               float eps, float bc1, float bc2_sqrt, float ema, float coef)
{
    const ChunkRec c = chunks[blockIdx.x];
    const TensorRec t = recs[c.tensor];
    const long long base = (long long)c.chunk * kChunk;
    long long end = base + kChunk;
    end = end < t.n ? end : t.n;
    const float step_size = t.lr / bc1;
    const float decay = 1.0f - t.lr * t.wd;
    const bool vec = ((t.n & 3) == 0);
    if (vec) {
        for (long long i = base + threadIdx.x * 4; i < end; i += 1024) {
            float4 p = *reinterpret_cast<const float4 *>(t.p + i);
            float4 tp = *reinterpret_cast<const float4 *>(t.tp + i);
            float pv[4] = {p.x, p.y, p.z, p.w}, tv[4] = {tp.x, tp.y, tp.z, tp.w};
            if (t.g) {
                const float4 g = *reinterpret_cast<const float4 *>(t.g + i);
                float4 m = *reinterpret_cast<const float4 *>(t.m + i), v = *reinterpret_cast<const float4 *>(t.v + i);
                float gv[4] = {g.x, g.y, g.z, g.w}, mv[4] = {m.x, m.y, m.z, m.w}, vv[4] = {v.x, v.y, v.z, v.w};
                if (GUARDED) {
#pragma unroll
                    for (int e = 0; e < 4; e++) gv[e] *= coef;
                }
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    pv[e] *= decay;
                    mv[e] = beta1 * mv[e] + (1.0f - beta1) * gv[e];
                    vv[e] = beta2 * vv[e] + (1.0f - beta2) * gv[e] * gv[e];
                    const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
                    pv[e] -= step_size * (mv[e] / denom);
                }
                *reinterpret_cast<float4 *>(t.m + i) = make_float4(mv[0], mv[1], mv[2], mv[3]);
                *reinterpret_cast<float4 *>(t.v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                *reinterpret_cast<float4 *>(t.p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            }
#pragma unroll
            for (int e = 0; e < 4; e++) tv[e] = ema * tv[e] + (1.0f - ema) * pv[e];
            *reinterpret_cast<float4 *>(t.tp + i) = make_float4(tv[0], tv[1], tv[2], tv[3]);
            if (t.p16 && t.g) *reinterpret_cast<uint2 *>(t.p16 + i) = pack16x4(pv, t.p16_f16);
            if (t.t16) *reinterpret_cast<uint2 *>(t.t16 + i) = pack16x4(tv, t.t16_f16);
        }
    } else {
        for (long long i = base + threadIdx.x; i < end; i += 256) {
            float p = t.p[i], tp = t.tp[i];
            if (t.g) {
                const float g = GUARDED ? t.g[i] * coef : t.g[i];
                p *= decay;
                const float m = beta1 * t.m[i] + (1.0f - beta1) * g;
                const float v = beta2 * t.v[i] + (1.0f - beta2) * g * g;
                p -= step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
                t.m[i] = m; t.v[i] = v; t.p[i] = p;
                if (t.p16) store16(t.p16 + i, p, t.p16_f16);
            }
            tp = ema * tp + (1.0f - ema) * p;
            t.tp[i] = tp;
            if (t.t16) store16(t.t16 + i, tp, t.t16_f16);
        }
    }
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                       float beta1, float beta2, float eps, float bc1, float bc2_sqrt, float ema)
{
    adamw_ema_body<false>(recs, chunks, beta1, beta2, eps, bc1, bc2_sqrt, ema, 1.0f);
}

// The same step behind the guard record of this iteration: refused as a whole (no block stores anything: masters, moments, teacher and
// all 16-bit shadows keep their bytes, the EMA is not applied) or taken on g * coef.  The gradient buffers are only read.
__global__ __launch_bounds__(256) void adamw_ema_guarded_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                               float beta1, float beta2, float eps, float bc1, float bc2_sqrt, float ema,
                                                               const GuardRec *__restrict__ guard)
{
    if (guard->skip) return;
    adamw_ema_body<true>(recs, chunks, beta1, beta2, eps, bc1, bc2_sqrt, ema, guard->coef);
}

// ---- gradient accumulation over micro-batches -------------------------------------------------------------------
// One block per chunk of the optimizer's own record table and chunk list, its loop shape (a pure stream: 8 B read + 4 B written per element,
// mode 0: 4 + 4).  MODE 0: acc = g (the first micro-step: the accumulator is not read, so it needs no clear); 1: acc = acc + g;
// 2: acc = (acc + g) * scale (the closing micro-step).  fp32, one rounding per operation (this file is built with -ffp-contract=off: the
// closing add and multiply are not fused), non-finite values propagate.  A tensor with g == NULL, or without an accumulator, is skipped;
// the gradient buffers are only read.
template <int MODE>
__device__ __forceinline__ float accum_one(float a, float g, float scale)
{
    if (MODE == 0) return g;
    if (MODE == 1) return a + g;
    return (a + g) * scale;
}

template <int MODE>
__global__ __launch_bounds__(256) void grad_accumulate_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                             float *const *__restrict__ accs, float scale)
{
    const ChunkRec c = chunks[blockIdx.x];
    const TensorRec t = recs[c.tensor];
    float *acc = accs[c.tensor];
    if (!t.g || !acc) return;
    const long long base = (long long)c.chunk * kChunk;
    long long end = base + kChunk;
    end = end < t.n ? end : t.n;
    if ((t.n & 3) == 0) {
        for (long long i = base + threadIdx.x * 4; i < end; i += 1024) {
            const float4 g = *reinterpret_cast<const float4 *>(t.g + i);
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (MODE != 0) a = *reinterpret_cast<const float4 *>(acc + i);
            a.x = accum_one<MODE>(a.x, g.x, scale);
            a.y = accum_one<MODE>(a.y, g.y, scale);
            a.z = accum_one<MODE>(a.z, g.z, scale);
            a.w = accum_one<MODE>(a.w, g.w, scale);
            *reinterpret_cast<float4 *>(acc + i) = a;
        }
    } else {
        for (long long i = base + threadIdx.x; i < end; i += 256) acc[i] = accum_one<MODE>(MODE != 0 ? acc[i] : 0.0f, t.g[i], scale);
    }
}

// ---- global gradient norm ---------------------------------------------------------------------------------------
// One block per chunk of the optimizer's own record table and chunk list; sum of g^2 in double (a finite fp32 squared and summed in double
// cannot overflow: the norm is non-finite exactly when some gradient element is), one partial per chunk, every addition in a fixed order.
__device__ __forceinline__ double block_sum_256(double s, double *red)
{
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void grad_norm_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                       double *__restrict__ partials)
{
    __shared__ double red[256];
    const ChunkRec c = chunks[blockIdx.x];
    const TensorRec t = recs[c.tensor];
    if (!t.g) {                                             // frozen: contributes nothing (its chunk's partial is still written)
        if (threadIdx.x == 0) partials[blockIdx.x] = 0.0;
        return;
    }
    const long long base = (long long)c.chunk * kChunk;
    long long end = base + kChunk;
    end = end < t.n ? end : t.n;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if ((t.n & 3) == 0) {
        for (long long i = base + threadIdx.x * 4; i < end; i += 1024) {
            const float4 g = *reinterpret_cast<const float4 *>(t.g + i);
            s0 += (double)g.x * (double)g.x;
            s1 += (double)g.y * (double)g.y;
            s2 += (double)g.z * (double)g.z;
            s3 += (double)g.w * (double)g.w;
        }
    } else {
        for (long long i = base + threadIdx.x; i < end; i += 256) {
            const double g = (double)t.g[i];
            s0 += g * g;
        }
    }
    const double s = block_sum_256((s0 + s1) + (s2 + s3), red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One block: thread k adds its contiguous run of partials in index order, the 256 runs are combined by the fixed tree above (no atomics:
// the same bits from run to run); thread 0 writes this iteration's decision and advances the counters with ordinary stores.
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double *__restrict__ partials, int n_chunks, float max_norm,
                                                                int skip_nonfinite, GuardRec *__restrict__ guard)
{
    __shared__ double red[256];
    const int per = (n_chunks + 255) / 256;
    const int lo = (int)threadIdx.x * per;
    int hi = lo + per;
    hi = hi < n_chunks ? hi : n_chunks;
    double s = 0.0;
    for (int i = lo; i < hi; i++) s += partials[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        float coef = 1.0f;
        if (max_norm > 0.0f) {                              // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1), NaN stays NaN
            const float c = max_norm / (norm + 1e-6f);
            coef = c > 1.0f ? 1.0f : c;
        }
        const int skip = (skip_nonfinite && !isfinite(s)) ? 1 : 0;    // on the double sum: an fp32 norm can round to inf from finite gradients
        guard->norm = norm;
        guard->coef = coef;
        guard->skip = skip;
        guard->pad = 0;
        if (skip) {
            guard->skipped += 1;
        } else {
            guard->applied += 1;
            if (coef < 1.0f) guard->clipped += 1;
        }
    }
}

// ---- per-tensor diagnostics -------------------------------------------------------------------------------------
// The reduction above keeps one number; these keep the per-tensor structure.  One row per tensor (cosa_tensor_stats_layout): three sums in
// double, the largest finite |g|, two counts of non-finite elements.  Everything the record table points at is only read.
struct StatsRow {
    double g_sq, w_sq, gap_sq, g_absmax;
    unsigned long long g_nonfinite, w_nonfinite;
};
static_assert(sizeof(StatsRow) == 8 * COSA_TENSOR_STATS_SLOTS, "a row is six 8-byte slots");
constexpr int kStatsMaxDevices = 64;      // read-back streams of cosa_tensor_stats, one per device

__device__ __forceinline__ bool nonfinite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

struct StatsLane {          // one thread's running values
    double g[4], w[4], d[4];
    float gmax;
    unsigned gbad, wbad;
};

template <int L>
__device__ __forceinline__ void stats_grad(StatsLane &a, float g)
{
    const bool bad = nonfinite_f32(g);
    a.g[L] += bad ? 0.0 : (double)g * (double)g;           // grad_norm_kernel's term, or 0 in place of a non-finite square
    a.gmax = bad ? a.gmax : fmaxf(a.gmax, fabsf(g));
    a.gbad += bad ? 1u : 0u;
}

template <int L>
__device__ __forceinline__ void stats_weight(StatsLane &a, float p, float tp)
{
    const bool pbad = nonfinite_f32(p), bad = pbad || nonfinite_f32(tp);
    const double d = (double)tp - (double)p;
    a.w[L] += pbad ? 0.0 : (double)p * (double)p;
    a.d[L] += bad ? 0.0 : d * d;
    a.wbad += bad ? 1u : 0u;
}

__global__ __launch_bounds__(256) void tensor_stats_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                          StatsRow *__restrict__ partials)
{
    __shared__ double red_g[256], red_w[256], red_d[256];
    __shared__ float red_m[256];
    __shared__ unsigned red_c[2][256];
    const ChunkRec c = chunks[blockIdx.x];
    const TensorRec t = recs[c.tensor];
    const long long base = (long long)c.chunk * kChunk;
    long long end = base + kChunk;
    end = end < t.n ? end : t.n;
    StatsLane a;
#pragma unroll
    for (int e = 0; e < 4; e++) a.g[e] = a.w[e] = a.d[e] = 0.0;
    a.gmax = 0.0f;
    a.gbad = a.wbad = 0u;
    if ((t.n & 3) == 0) {
        for (long long i = base + threadIdx.x * 4; i < end; i += 1024) {
            const float4 p = *reinterpret_cast<const float4 *>(t.p + i);
            const float4 tp = *reinterpret_cast<const float4 *>(t.tp + i);
            if (t.g) {
                const float4 g = *reinterpret_cast<const float4 *>(t.g + i);
                stats_grad<0>(a, g.x);
                stats_grad<1>(a, g.y);
                stats_grad<2>(a, g.z);
                stats_grad<3>(a, g.w);
            }
            stats_weight<0>(a, p.x, tp.x);
            stats_weight<1>(a, p.y, tp.y);
            stats_weight<2>(a, p.z, tp.z);
            stats_weight<3>(a, p.w, tp.w);
        }
    } else {
        for (long long i = base + threadIdx.x; i < end; i += 256) {
            if (t.g) stats_grad<0>(a, t.g[i]);
            stats_weight<0>(a, t.p[i], t.tp[i]);
        }
    }
    // the three sums through the guard's own tree (g_sq: the bits of grad_norm_kernel's partial on an all-finite chunk), each in its own array
    const double g_sq = block_sum_256((a.g[0] + a.g[1]) + (a.g[2] + a.g[3]), red_g);
    const double w_sq = block_sum_256((a.w[0] + a.w[1]) + (a.w[2] + a.w[3]), red_w);
    const double gap_sq = block_sum_256((a.d[0] + a.d[1]) + (a.d[2] + a.d[3]), red_d);
    red_m[threadIdx.x] = a.gmax;
    red_c[0][threadIdx.x] = a.gbad;                         // at most 65536 per block
    red_c[1][threadIdx.x] = a.wbad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red_m[threadIdx.x] = fmaxf(red_m[threadIdx.x], red_m[threadIdx.x + w]);
            red_c[0][threadIdx.x] += red_c[0][threadIdx.x + w];
            red_c[1][threadIdx.x] += red_c[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        StatsRow r;
        r.g_sq = g_sq; r.w_sq = w_sq; r.gap_sq = gap_sq;
        r.g_absmax = (double)red_m[0];
        r.g_nonfinite = red_c[0][0];
        r.w_nonfinite = red_c[1][0];
        partials[blockIdx.x] = r;
    }
}

// tensor t's chunks, clamped to the list: a table the host did not check (cosa_grad_blame) cannot send a thread outside the partials
__device__ __forceinline__ void chunk_range(const int *__restrict__ first_chunk, int t, int n_chunks, int &lo, int &hi)
{
    lo = first_chunk[t];
    hi = first_chunk[t + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_chunks ? n_chunks : hi;
}

// One thread per tensor: its chunks' partial rows in index order (sums added in that order, counts as integers, maxima as maxima); a tensor
// without chunks gets a zero row.
__global__ __launch_bounds__(256) void tensor_stats_finalize_kernel(const StatsRow *__restrict__ partials, const int *__restrict__ first_chunk,
                                                                   int n_tensors, int n_chunks, StatsRow *__restrict__ out)
{
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= n_tensors) return;
    int lo, hi;
    chunk_range(first_chunk, t, n_chunks, lo, hi);
    StatsRow r;
    r.g_sq = r.w_sq = r.gap_sq = r.g_absmax = 0.0;
    r.g_nonfinite = r.w_nonfinite = 0ull;
    for (int i = lo; i < hi; i++) {
        const StatsRow q = partials[i];
        r.g_sq += q.g_sq;
        r.w_sq += q.w_sq;
        r.gap_sq += q.gap_sq;
        r.g_absmax = q.g_absmax > r.g_absmax ? q.g_absmax : r.g_absmax;
        r.g_nonfinite += q.g_nonfinite;
        r.w_nonfinite += q.w_nonfinite;
    }
    out[t] = r;
}

// Which tensor made the guard's sum non-finite: over the partials grad_norm_kernel has just written (a double sum of squared fp32 values is
// non-finite exactly when an element is), one thread per tensor, ordinary loads and stores.
__global__ __launch_bounds__(256) void grad_blame_kernel(const double *__restrict__ partials, const int *__restrict__ first_chunk, int n_tensors,
                                                        int n_chunks, unsigned long long *__restrict__ blame)
{
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= n_tensors) return;
    int lo, hi;
    chunk_range(first_chunk, t, n_chunks, lo, hi);
    bool bad = false;
    for (int i = lo; i < hi; i++) bad = bad || !isfinite(partials[i]);
    if (bad) blame[t] += 1ull;
}

// ---- training-state snapshot / restore ---------------------------------------------------------------------
// The same record-table + chunk-list pattern as above, over BYTES: every tensor that defines the future of a run (any dtype, contiguous)
// is copied into its 16-byte-aligned, zero-padded slot of one contiguous arena (or back), and two 64-bit checksums per tensor are formed
// over the slot's little-endian 32-bit words w_i: s0 = sum w_i, s1 = sum (i+1) w_i, both mod 2^64.  Integer addition commutes, so the
// workgroup reduction + one atomicAdd pair per chunk gives the same bits in any order.
// A tensor whose address is a multiple of 16 moves in 16-byte units, one that is only 4-byte aligned in 4-byte ones; any other address takes
// sixteen single-byte accesses per unit for the WHOLE tensor.  Allocator-made tensors are always 16-byte aligned, so that path serves odd
// views only; it is correct (tests/test_resume_gpu.py) and its throughput has not been measured.
struct StateRec {
    unsigned char *ptr;              // the tensor's bytes
    unsigned long long nbytes;       // its size (slot = nbytes rounded up to 16, tail zero)
    unsigned long long off;          // slot offset in the arena (cosa_state_layout)
};

constexpr unsigned long long kStateChunk = 262144;         // slot bytes per block
constexpr int kStateMaxTensors = 4096;
constexpr unsigned long long kStateMaxBytes = 1ull << 40;

// MODE 0: tensor -> arena (snapshot); 1: arena -> checksums only (verify); 2: arena -> tensor (scatter)
template <int MODE>
__global__ __launch_bounds__(256) void state_kernel(const StateRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                    unsigned char *__restrict__ arena, unsigned long long *__restrict__ sums)
{
    const ChunkRec c = chunks[blockIdx.x];
    const StateRec t = recs[c.tensor];
    const unsigned long long slot = (t.nbytes + 15ull) & ~15ull;
    const unsigned long long base = (unsigned long long)c.chunk * kStateChunk;
    unsigned long long end = base + kStateChunk;
    end = end < slot ? end : slot;
    unsigned char *a = arena + t.off;                      // 16-byte aligned: the arena's base and every offset are
    const unsigned mis = (unsigned)(reinterpret_cast<unsigned long long>(t.ptr) & 15ull);
    unsigned long long s0 = 0, s1 = 0;
    for (unsigned long long o = base + threadIdx.x * 16ull; o < end; o += 4096ull) {
        const bool full = o + 16ull <= t.nbytes;
        uint4 v;
        if (MODE == 0) {
            if (full && mis == 0) {
                v = *reinterpret_cast<const uint4 *>(t.ptr + o);
            } else if (full && (mis & 3u) == 0) {
                const unsigned *s = reinterpret_cast<const unsigned *>(t.ptr + o);
                v = make_uint4(s[0], s[1], s[2], s[3]);
            } else {                                       // unaligned source or the slot's last, partly padded unit
                unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 16; j++)
                    if (o + j < t.nbytes) w[j >> 2] |= (unsigned)t.ptr[o + j] << (8 * (j & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4 *>(a + o) = v;
        } else {
            v = *reinterpret_cast<const uint4 *>(a + o);
            if (MODE == 2) {
                if (full && mis == 0) {
                    *reinterpret_cast<uint4 *>(t.ptr + o) = v;
                } else if (full && (mis & 3u) == 0) {
                    unsigned *d = reinterpret_cast<unsigned *>(t.ptr + o);
                    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                } else {
                    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 16; j++)
                        if (o + j < t.nbytes) t.ptr[o + j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
                }
            }
        }
        const unsigned long long i1 = (o >> 2) + 1ull;     // (index + 1) of the unit's first word
        s0 += (unsigned long long)v.x + v.y + v.z + v.w;
        s1 += i1 * v.x + (i1 + 1ull) * v.y + (i1 + 2ull) * v.z + (i1 + 3ull) * v.w;
    }
    __shared__ unsigned long long red[2][256];
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicAdd(&sums[2 * c.tensor], red[0][0]);
        atomicAdd(&sums[2 * c.tensor + 1], red[1][0]);
    }
}

template <int MODE>
int launch_state(const void *records, const void *chunks, int n_tensors, int n_chunks, void *arena, void *sums, void *stream, const char *who)
{
    COSA_REQUIRE(n_tensors >= 0 && n_tensors <= kStateMaxTensors, "%s: %d tensors (at most %d)", who, n_tensors, kStateMaxTensors);
    COSA_REQUIRE(n_chunks >= 0, "%s: negative chunk count", who);
    if (n_tensors == 0) {
        COSA_REQUIRE(n_chunks == 0, "%s: chunks without tensors", who);
        return COSA_OK;
    }
    COSA_REQUIRE(records && sums, "%s: null record table or checksum buffer", who);
    COSA_REQUIRE((reinterpret_cast<unsigned long long>(sums) & 7ull) == 0, "%s: the checksum buffer must be 8-byte aligned", who);
    COSA_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)n_tensors * 16, as_stream(stream)));
    if (n_chunks == 0) return COSA_OK;                      // zero-length tensors only
    COSA_REQUIRE(chunks && arena, "%s: null chunk list or arena", who);
    COSA_REQUIRE((reinterpret_cast<unsigned long long>(arena) & 15ull) == 0, "%s: the arena must be 16-byte aligned", who);
    hipLaunchKernelGGL(state_kernel<MODE>, dim3(n_chunks), dim3(256), 0, as_stream(stream), static_cast<const StateRec *>(records),
                       static_cast<const ChunkRec *>(chunks), static_cast<unsigned char *>(arena), static_cast<unsigned long long *>(sums));
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" size_t cosa_optim_record_bytes(void) { return sizeof(TensorRec); }
extern "C" int cosa_optim_chunk_elems(void) { return kChunk; }

/* records: device array of n_tensors TensorRec (layout: 7 pointers, float lr, float wd, int64 n, int32 t16_f16, int32 p16_f16); chunks: device array of
 * n_chunks {int tensor, int chunk}.  step >= 1 is the AdamW step count used for bias correction.                       */
extern "C" int cosa_fused_adamw_ema(const void *records, const void *chunks, int n_chunks, float beta1, float beta2, float eps,
                                    int step, float ema_momentum, void *stream)
{
    COSA_REQUIRE(records && chunks && n_chunks > 0 && step >= 1, "cosa_fused_adamw_ema: bad arguments");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_ema_kernel, dim3(n_chunks), dim3(256), 0, as_stream(stream), static_cast<const TensorRec *>(records),
                       static_cast<const ChunkRec *>(chunks), beta1, beta2, eps, bc1, bc2_sqrt, ema_momentum);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

/* ---- gradient accumulation (include/cosa_hip.h) ---- */
extern "C" int cosa_grad_accumulate(const void *records, const void *chunks, int n_chunks, const void *acc_ptrs, int mode, float scale,
                                    void *stream)
{
    COSA_REQUIRE(records && chunks && acc_ptrs, "cosa_grad_accumulate: null record table, chunk list or accumulator pointer array");
    COSA_REQUIRE(n_chunks > 0, "cosa_grad_accumulate: %d chunks (must be positive)", n_chunks);
    COSA_REQUIRE(mode >= 0 && mode <= 2, "cosa_grad_accumulate: mode %d (0: acc = g, 1: acc += g, 2: acc = (acc + g) * scale)", mode);
    COSA_REQUIRE(std::isfinite(scale), "cosa_grad_accumulate: scale %g is not finite", (double)scale);
    const TensorRec *recs = static_cast<const TensorRec *>(records);
    const ChunkRec *ch = static_cast<const ChunkRec *>(chunks);
    float *const *accs = static_cast<float *const *>(acc_ptrs);
    if (mode == 0)
        hipLaunchKernelGGL(grad_accumulate_kernel<0>, dim3(n_chunks), dim3(256), 0, as_stream(stream), recs, ch, accs, scale);
    else if (mode == 1)
        hipLaunchKernelGGL(grad_accumulate_kernel<1>, dim3(n_chunks), dim3(256), 0, as_stream(stream), recs, ch, accs, scale);
    else
        hipLaunchKernelGGL(grad_accumulate_kernel<2>, dim3(n_chunks), dim3(256), 0, as_stream(stream), recs, ch, accs, scale);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

/* ---- the gradient guard (include/cosa_hip.h) ---- */
extern "C" size_t cosa_grad_guard_bytes(void) { return sizeof(GuardRec); }
extern "C" size_t cosa_grad_norm_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(double) : 0; }

extern "C" int cosa_grad_norm(const void *records, const void *chunks, int n_chunks, float max_norm, int skip_nonfinite, void *workspace,
                              size_t workspace_bytes, void *guard, void *stream)
{
    COSA_REQUIRE(records && chunks && n_chunks > 0, "cosa_grad_norm: null record table or chunk list, or no chunks");
    COSA_REQUIRE(guard, "cosa_grad_norm: null guard record");
    COSA_REQUIRE((reinterpret_cast<unsigned long long>(guard) & 7ull) == 0, "cosa_grad_norm: the guard record must be 8-byte aligned");
    COSA_REQUIRE(max_norm >= 0.0f, "cosa_grad_norm: max_norm %g (0 = no clipping, or a positive bound)", (double)max_norm);
    const size_t need = cosa_grad_norm_workspace_bytes(n_chunks);
    COSA_REQUIRE(workspace && workspace_bytes >= need, "cosa_grad_norm: workspace of %zu bytes (%zu needed)", workspace ? workspace_bytes : (size_t)0,
                 need);
    COSA_REQUIRE((reinterpret_cast<unsigned long long>(workspace) & 7ull) == 0, "cosa_grad_norm: the workspace must be 8-byte aligned");
    double *partials = static_cast<double *>(workspace);
    hipLaunchKernelGGL(grad_norm_kernel, dim3(n_chunks), dim3(256), 0, as_stream(stream), static_cast<const TensorRec *>(records),
                       static_cast<const ChunkRec *>(chunks), partials);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, n_chunks, max_norm, skip_nonfinite ? 1 : 0,
                       static_cast<GuardRec *>(guard));
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_fused_adamw_ema_guarded(const void *records, const void *chunks, int n_chunks, float beta1, float beta2, float eps,
                                            int step, float ema_momentum, const void *guard, void *stream)
{
    COSA_REQUIRE(records && chunks && n_chunks > 0 && step >= 1, "cosa_fused_adamw_ema_guarded: bad arguments");
    COSA_REQUIRE(guard, "cosa_fused_adamw_ema_guarded: null guard record");
    COSA_REQUIRE((reinterpret_cast<unsigned long long>(guard) & 7ull) == 0, "cosa_fused_adamw_ema_guarded: the guard record must be 8-byte aligned");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_ema_guarded_kernel, dim3(n_chunks), dim3(256), 0, as_stream(stream), static_cast<const TensorRec *>(records),
                       static_cast<const ChunkRec *>(chunks), beta1, beta2, eps, bc1, bc2_sqrt, ema_momentum, static_cast<const GuardRec *>(guard));
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

/* ---- per-tensor diagnostics (include/cosa_hip.h) ---- */
extern "C" size_t cosa_tensor_stats_layout(size_t *offsets)
{
    if (!offsets) {
        set_error("cosa_tensor_stats_layout: offsets must be non-null");
        return 0;
    }
    offsets[0] = offsetof(StatsRow, g_sq);
    offsets[1] = offsetof(StatsRow, w_sq);
    offsets[2] = offsetof(StatsRow, gap_sq);
    offsets[3] = offsetof(StatsRow, g_absmax);
    offsets[4] = offsetof(StatsRow, g_nonfinite);
    offsets[5] = offsetof(StatsRow, w_nonfinite);
    return sizeof(StatsRow);
}

extern "C" size_t cosa_tensor_stats_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(StatsRow) : 0; }

extern "C" int cosa_tensor_stats(const void *records, const void *chunks, const int *first_chunk, int n_tensors, int n_chunks, void *workspace,
                                 size_t workspace_bytes, void *out, void *stream)
{
    COSA_REQUIRE(records && chunks && first_chunk && out, "cosa_tensor_stats: null record table, chunk list, first_chunk or out");
    COSA_REQUIRE(n_tensors > 0 && n_chunks > 0, "cosa_tensor_stats: %d tensors, %d chunks (both must be positive)", n_tensors, n_chunks);
    const size_t need = cosa_tensor_stats_workspace_bytes(n_chunks);
    COSA_REQUIRE(workspace && workspace_bytes >= need, "cosa_tensor_stats: workspace of %zu bytes (%zu needed)", workspace ? workspace_bytes : (size_t)0,
                 need);
    COSA_REQUIRE(((reinterpret_cast<unsigned long long>(workspace) | reinterpret_cast<unsigned long long>(out)) & 7ull) == 0,
                 "cosa_tensor_stats: workspace and out must be 8-byte aligned");
    // first_chunk decides which partials a tensor's thread reads: checked on the host before anything is launched.  The n_tensors + 1 ints
    // come back on a stream of our own (non-blocking: the caller's stream, and the step in flight on it, are not waited for).
    // The host does wait for that copy (tens of microseconds, once per sample; DESIGN.md section 12 has the measured figure).  One stream per
    // device, created on first use under a lock and kept for the life of the process, like the library's other per-process state.
    static std::mutex side_lock;
    static hipStream_t side_of[kStatsMaxDevices] = {};
    int device = -1;
    COSA_HIP_CHECK(hipGetDevice(&device));
    COSA_REQUIRE(device >= 0 && device < kStatsMaxDevices, "cosa_tensor_stats: device %d (at most %d devices per process)", device, kStatsMaxDevices);
    std::vector<int> fc((size_t)n_tensors + 1);
    {
        std::lock_guard<std::mutex> hold(side_lock);       // (also serialises two threads' read-backs on the one stream)
        if (!side_of[device]) COSA_HIP_CHECK(hipStreamCreateWithFlags(&side_of[device], hipStreamNonBlocking));
        COSA_HIP_CHECK(hipMemcpyAsync(fc.data(), first_chunk, fc.size() * sizeof(int), hipMemcpyDeviceToHost, side_of[device]));
        COSA_HIP_CHECK(hipStreamSynchronize(side_of[device]));
    }
    COSA_REQUIRE(fc[0] == 0, "cosa_tensor_stats: first_chunk[0] is %d (must be 0)", fc[0]);
    for (int t = 0; t < n_tensors; t++)
        COSA_REQUIRE(fc[t + 1] >= fc[t], "cosa_tensor_stats: first_chunk is not monotone at tensor %d (%d after %d)", t, fc[t + 1], fc[t]);
    COSA_REQUIRE(fc[n_tensors] == n_chunks, "cosa_tensor_stats: first_chunk ends at %d, the chunk list has %d", fc[n_tensors], n_chunks);
    StatsRow *partials = static_cast<StatsRow *>(workspace);
    hipLaunchKernelGGL(tensor_stats_kernel, dim3(n_chunks), dim3(256), 0, as_stream(stream), static_cast<const TensorRec *>(records),
                       static_cast<const ChunkRec *>(chunks), partials);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(tensor_stats_finalize_kernel, dim3((n_tensors + 255) / 256), dim3(256), 0, as_stream(stream), partials, first_chunk, n_tensors,
                       n_chunks, static_cast<StatsRow *>(out));
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_grad_blame(const void *partials, const int *first_chunk, int n_tensors, int n_chunks, unsigned long long *blame, void *stream)
{
    COSA_REQUIRE(partials && first_chunk && blame, "cosa_grad_blame: null partials, first_chunk or blame");
    COSA_REQUIRE(n_tensors > 0 && n_chunks > 0, "cosa_grad_blame: %d tensors, %d chunks (both must be positive)", n_tensors, n_chunks);
    COSA_REQUIRE(((reinterpret_cast<unsigned long long>(partials) | reinterpret_cast<unsigned long long>(blame)) & 7ull) == 0,
                 "cosa_grad_blame: partials and blame must be 8-byte aligned");
    hipLaunchKernelGGL(grad_blame_kernel, dim3((n_tensors + 255) / 256), dim3(256), 0, as_stream(stream), static_cast<const double *>(partials),
                       first_chunk, n_tensors, n_chunks, blame);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

/* ---- training-state arena (include/cosa_hip.h) ---- */
extern "C" size_t cosa_state_record_bytes(void) { return sizeof(StateRec); }
extern "C" size_t cosa_state_chunk_bytes(void) { return (size_t)kStateChunk; }

extern "C" size_t cosa_state_layout(int n, const unsigned long long *nbytes, unsigned long long *offsets_out)
{
    if (n < 0 || n > kStateMaxTensors || (n > 0 && (!nbytes || !offsets_out))) {
        set_error("cosa_state_layout: %d tensors (0..%d, with size and offset arrays)", n, kStateMaxTensors);
        return (size_t)-1;
    }
    unsigned long long off = 0;
    for (int i = 0; i < n; i++) {
        if (nbytes[i] > kStateMaxBytes) {
            set_error("cosa_state_layout: tensor %d has %llu bytes (at most 2^40)", i, nbytes[i]);
            return (size_t)-1;
        }
        offsets_out[i] = off;
        off += (nbytes[i] + 15ull) & ~15ull;
    }
    return (size_t)off;
}

extern "C" int cosa_state_snapshot(const void *records, const void *chunks, int n_tensors, int n_chunks, void *arena, void *sums, void *stream)
{
    return launch_state<0>(records, chunks, n_tensors, n_chunks, arena, sums, stream, "cosa_state_snapshot");
}

extern "C" int cosa_state_restore(const void *records, const void *chunks, int n_tensors, int n_chunks, const void *arena, void *sums,
                                  int scatter, void *stream)
{
    if (scatter)
        return launch_state<2>(records, chunks, n_tensors, n_chunks, const_cast<void *>(arena), sums, stream, "cosa_state_restore");
    return launch_state<1>(records, chunks, n_tensors, n_chunks, const_cast<void *>(arena), sums, stream, "cosa_state_restore");
}
