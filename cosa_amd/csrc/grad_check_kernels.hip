// grad_check_kernels.hip -- the --grad_check_iters check: the two streams over the parameters that a finite-difference
// check of the step's gradient needs, on a record table of the check's own (include/cosa_hip.h: the layout).
//
//   cosa_grad_check_norms    per direction G2 = sum g^2, W2 = sum w^2 and the counts of non-finite g / w elements, then the step length
//                            s = float(rho sqrt(W2 / G2)) -- 0, and the record flagged, where the direction has no usable gradient
//   cosa_grad_check_perturb  dst = w + fl32(fl32(c s) g) inside direction `dir` (s read from the record on the device: no sync), dst = w
//                            outside it, and the realised step t_c = sum (dst - w) g
//
// Every sum is a double: each thread adds its strided elements in index order, a wavefront's 64 sums meet in an xor butterfly, the four
// wavefronts are added in wave order, one partial per chunk is written, and a finalize launch adds the partials of a direction lane-strided
// in chunk order and closes with the same butterfly.  No atomics: the same bytes on every run.  Plain vector loads and stores only: dwordx4
// where w, g and dst of a tensor are 16-byte aligned, single elements otherwise and for a tensor's last n % 4 elements.
#include "wave_reduce.hpp"

namespace cosa {
namespace {

constexpr int kChunk = COSA_GRAD_CHECK_CHUNK;
constexpr int kRecord = COSA_GRAD_CHECK_RECORD;
constexpr int kThreads = 256;
static_assert(kChunk % (4 * kThreads) == 0, "a chunk is whole rounds of dwordx4 per thread");

struct TensorRec {                 // COSA_GRAD_CHECK_RECORD_BYTES each
    const float *w;                // the fp32 master
    const float *g;                // its raw gradient (NULL: none, dir must be -1)
    float *dst;                    // the check network's copy
    long long n;
    int dir;                       // -1: in no direction (copied)
    int pad;
};
static_assert(sizeof(TensorRec) == COSA_GRAD_CHECK_RECORD_BYTES, "the table's layout is part of the ABI");

struct ChunkRec { int tensor; int chunk; };

// a double over the wavefront: the xor butterfly (fixed order: the same bits on every run); every lane holds the result
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the workgroup's sum on thread 0: butterfly per wavefront, then the wavefronts in wave order
__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum_f64(v);
    const int wave = threadIdx.x >> 6;
    if (__lane_id() == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kThreads / 64; i++) s += red[i];
    __syncthreads();
    return s;
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// partials [n_chunks][4]: g2, w2, non-finite g, non-finite w (counts below 2^53: exact in a double)
__global__ __launch_bounds__(kThreads) void norms_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                         double *__restrict__ partials)
{
    __shared__ double red[kThreads / 64];
    const ChunkRec c = chunks[blockIdx.x];
    const TensorRec t = recs[c.tensor];
    double *out = partials + 4 * (size_t)blockIdx.x;
    if (t.dir < 0 || !t.g) {                                           // (block-uniform) in no direction: the partial is still written
        if (threadIdx.x == 0) out[0] = out[1] = out[2] = out[3] = 0.0;
        return;
    }
    const long long base = (long long)c.chunk * kChunk;
    long long end = base + kChunk;
    end = end < t.n ? end : t.n;
    double g2 = 0.0, w2 = 0.0;
    unsigned bad_g = 0, bad_w = 0;
    auto one = [&](float g, float w) {
        g2 += (double)g * (double)g;
        w2 += (double)w * (double)w;
        bad_g += nonfinite_bits(g) ? 1u : 0u;
        bad_w += nonfinite_bits(w) ? 1u : 0u;
    };
    long long i = base;
    if (aligned16(t.w) && aligned16(t.g)) {
        const long long end4 = base + ((end - base) & ~3ll);
        for (long long j = base + threadIdx.x * 4; j < end4; j += kThreads * 4) {
            const float4 g = *reinterpret_cast<const float4 *>(t.g + j), w = *reinterpret_cast<const float4 *>(t.w + j);
            one(g.x, w.x);
            one(g.y, w.y);
            one(g.z, w.z);
            one(g.w, w.w);
        }
        i = end4;
    }
    for (long long j = i + threadIdx.x; j < end; j += kThreads) one(t.g[j], t.w[j]);
    const double s0 = block_sum(g2, red), s1 = block_sum(w2, red), s2 = block_sum((double)bad_g, red), s3 = block_sum((double)bad_w, red);
    if (threadIdx.x == 0) {
        out[0] = s0;
        out[1] = s1;
        out[2] = s2;
        out[3] = s3;
    }
}

// the partials of direction `d` over the chunk list: lane l takes chunks l, l + 64, ... in that order, then the butterfly
template <int STRIDE>
__device__ __forceinline__ double dir_sum(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks, const double *__restrict__ partials,
                                          int n_chunks, int d, int field)
{
    double s = 0.0;
    for (int i = __lane_id(); i < n_chunks; i += 64)
        if (recs[chunks[i].tensor].dir == d) s += partials[(size_t)i * STRIDE + field];
    return wave_sum_f64(s);
}

// one wavefront per direction
__global__ __launch_bounds__(64) void norms_finalize_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                           const double *__restrict__ partials, int n_chunks, double rho,
                                                           double *__restrict__ record)
{
    const int d = blockIdx.x;
    const double G2 = dir_sum<4>(recs, chunks, partials, n_chunks, d, 0), W2 = dir_sum<4>(recs, chunks, partials, n_chunks, d, 1),
                 bad_g = dir_sum<4>(recs, chunks, partials, n_chunks, d, 2), bad_w = dir_sum<4>(recs, chunks, partials, n_chunks, d, 3);
    if (__lane_id() != 0) return;
    unsigned flags = 0;
    if (G2 == 0.0) flags |= COSA_GRAD_CHECK_FLAG_ZERO_GRAD;
    if (!isfinite(G2) || bad_g > 0.0) flags |= COSA_GRAD_CHECK_FLAG_BAD_GRAD;
    if (!isfinite(W2) || bad_w > 0.0) flags |= COSA_GRAD_CHECK_FLAG_BAD_WEIGHT;
    float s = 0.0f;
    if (!flags) {
        s = (float)(rho * sqrt(W2 / G2));
        if (!isfinite(s) || s == 0.0f) {                               // (W2 = 0, or a ratio outside fp32)
            s = 0.0f;
            flags |= COSA_GRAD_CHECK_FLAG_NO_STEP;
        }
    }
    double *r = record + (size_t)d * kRecord;
    r[COSA_GRAD_CHECK_G2] = G2;
    r[COSA_GRAD_CHECK_W2] = W2;
    r[COSA_GRAD_CHECK_S] = (double)s;
    r[COSA_GRAD_CHECK_FLAGS] = (double)flags;
    r[COSA_GRAD_CHECK_BAD_G] = bad_g;
    r[COSA_GRAD_CHECK_BAD_W] = bad_w;
}

// partials [n_chunks]: sum (dst - w) g
__global__ __launch_bounds__(kThreads) void perturb_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks, int dir, float c,
                                                           const double *__restrict__ record, double *__restrict__ partials)
{
    __shared__ double red[kThreads / 64];
    const ChunkRec ck = chunks[blockIdx.x];
    const TensorRec t = recs[ck.tensor];
    const float s = (float)record[(size_t)dir * kRecord + COSA_GRAD_CHECK_S];
    const float cs = __fmul_rn(c, s);
    const bool moved = t.dir == dir && t.g && s != 0.0f;               // (block-uniform)
    const long long base = (long long)ck.chunk * kChunk;
    long long end = base + kChunk;
    end = end < t.n ? end : t.n;
    double tc = 0.0;
    auto one = [&](float w, float g) -> float {
        const float wp = __fadd_rn(w, __fmul_rn(cs, g));               // two roundings, no contraction
        tc += ((double)wp - (double)w) * (double)g;
        return wp;
    };
    long long i = base;
    if (aligned16(t.w) && aligned16(t.dst) && (!moved || aligned16(t.g))) {
        const long long end4 = base + ((end - base) & ~3ll);
        for (long long j = base + threadIdx.x * 4; j < end4; j += kThreads * 4) {
            float4 w = *reinterpret_cast<const float4 *>(t.w + j);
            if (moved) {
                const float4 g = *reinterpret_cast<const float4 *>(t.g + j);
                w.x = one(w.x, g.x);
                w.y = one(w.y, g.y);
                w.z = one(w.z, g.z);
                w.w = one(w.w, g.w);
            }
            *reinterpret_cast<float4 *>(t.dst + j) = w;
        }
        i = end4;
    }
    for (long long j = i + threadIdx.x; j < end; j += kThreads) {
        const float w = t.w[j];
        t.dst[j] = moved ? one(w, t.g[j]) : w;
    }
    const double sum = block_sum(tc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(64) void perturb_finalize_kernel(const TensorRec *__restrict__ recs, const ChunkRec *__restrict__ chunks,
                                                             const double *__restrict__ partials, int n_chunks, int dir, int slot,
                                                             double *__restrict__ record)
{
    const double t = dir_sum<1>(recs, chunks, partials, n_chunks, dir, 0);
    if (__lane_id() == 0) record[(size_t)dir * kRecord + COSA_GRAD_CHECK_T + slot] = t;
}

// the envelope of both entry points, on the host copy of the table the device one was uploaded from
int check_table(const char *who, const void *table_host, const void *table_dev, int n_tensors, int n_chunks, int n_dirs, const double *record,
                const void *workspace, size_t workspace_bytes, size_t need)
{
    COSA_REQUIRE(table_host && table_dev && record && workspace, "%s: null argument (the table on the host and on the device, the record and the "
                 "workspace are required)", who);
    COSA_REQUIRE(n_tensors > 0 && n_chunks > 0 && n_dirs > 0, "%s: n_tensors %d, n_chunks %d and n_dirs %d must be positive", who, n_tensors,
                 n_chunks, n_dirs);
    COSA_REQUIRE(((uintptr_t)table_dev & 7) == 0 && ((uintptr_t)record & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
                 "%s: the table, the record and the workspace must be 8-byte aligned", who);
    COSA_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu bytes, %zu needed)", who, workspace_bytes, need);
    const TensorRec *recs = static_cast<const TensorRec *>(table_host);
    const ChunkRec *chunks = reinterpret_cast<const ChunkRec *>(recs + n_tensors);
    long long covered = 0, total = 0;
    for (int i = 0; i < n_tensors; i++) {
        const TensorRec &t = recs[i];
        COSA_REQUIRE(t.n >= 0, "%s: tensor %d has n %lld", who, i, t.n);
        COSA_REQUIRE(t.dir >= -1 && t.dir < n_dirs, "%s: tensor %d has dir %d outside [-1, %d)", who, i, t.dir, n_dirs);
        COSA_REQUIRE(t.n == 0 || (t.w && t.dst), "%s: tensor %d has a null w or dst", who, i);
        COSA_REQUIRE(t.n == 0 || t.dir < 0 || t.g, "%s: tensor %d is in direction %d and has no gradient", who, i, t.dir);
        COSA_REQUIRE((((uintptr_t)t.w | (uintptr_t)t.g | (uintptr_t)t.dst) & 3) == 0, "%s: tensor %d is not 4-byte aligned", who, i);
        total += (t.n + kChunk - 1) / kChunk;
    }
    for (int i = 0; i < n_chunks; i++) {
        const ChunkRec &c = chunks[i];
        COSA_REQUIRE(c.tensor >= 0 && c.tensor < n_tensors && c.chunk >= 0 && (long long)c.chunk * kChunk < recs[c.tensor].n,
                     "%s: chunk %d (tensor %d, chunk %d) lies outside the table", who, i, c.tensor, c.chunk);
        // in table order, every chunk once: a tensor's chunks follow each other from 0
        const bool first = i == 0 || chunks[i - 1].tensor != c.tensor;
        COSA_REQUIRE(first ? (c.chunk == 0 && (i == 0 || chunks[i - 1].tensor < c.tensor)) : c.chunk == chunks[i - 1].chunk + 1,
                     "%s: chunk %d is out of order", who, i);
        covered++;
    }
    COSA_REQUIRE(covered == total, "%s: the chunk list has %lld chunks, the tensors %lld", who, covered, total);
    return COSA_OK;
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" size_t cosa_grad_check_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * 4 * sizeof(double) : 0; }

extern "C" int cosa_grad_check_norms(const void *table_host, const void *table_dev, int n_tensors, int n_chunks, int n_dirs, double rho,
                                     double *record, void *workspace, size_t workspace_bytes, void *stream)
{
    const int rc = check_table("cosa_grad_check_norms", table_host, table_dev, n_tensors, n_chunks, n_dirs, record, workspace, workspace_bytes,
                               cosa_grad_check_workspace_bytes(n_chunks));
    if (rc != COSA_OK) return rc;
    COSA_REQUIRE(rho == rho && rho - rho == 0.0 && rho > 0.0, "cosa_grad_check_norms: rho must be finite and positive (got %g)", rho);
    const TensorRec *recs = static_cast<const TensorRec *>(table_dev);
    const ChunkRec *chunks = reinterpret_cast<const ChunkRec *>(recs + n_tensors);
    double *partials = static_cast<double *>(workspace);
    hipLaunchKernelGGL(norms_kernel, dim3(n_chunks), dim3(kThreads), 0, as_stream(stream), recs, chunks, partials);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(norms_finalize_kernel, dim3(n_dirs), dim3(64), 0, as_stream(stream), recs, chunks, partials, n_chunks, rho, record);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_grad_check_perturb(const void *table_host, const void *table_dev, int n_tensors, int n_chunks, int n_dirs, int dir, float c,
                                       int slot, double *record, void *workspace, size_t workspace_bytes, void *stream)
{
    const int rc = check_table("cosa_grad_check_perturb", table_host, table_dev, n_tensors, n_chunks, n_dirs, record, workspace, workspace_bytes,
                               (size_t)(n_chunks > 0 ? n_chunks : 0) * sizeof(double));
    if (rc != COSA_OK) return rc;
    COSA_REQUIRE(dir >= 0 && dir < n_dirs, "cosa_grad_check_perturb: dir %d outside [0, %d)", dir, n_dirs);
    COSA_REQUIRE(slot >= 0 && slot < COSA_GRAD_CHECK_STEPS, "cosa_grad_check_perturb: slot %d outside [0, %d)", slot, COSA_GRAD_CHECK_STEPS);
    COSA_REQUIRE(c == c && c - c == 0.0f, "cosa_grad_check_perturb: c must be finite (got %g)", (double)c);
    const TensorRec *recs = static_cast<const TensorRec *>(table_dev);
    const ChunkRec *chunks = reinterpret_cast<const ChunkRec *>(recs + n_tensors);
    double *partials = static_cast<double *>(workspace);
    hipLaunchKernelGGL(perturb_kernel, dim3(n_chunks), dim3(kThreads), 0, as_stream(stream), recs, chunks, dir, c, record, partials);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(perturb_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), recs, chunks, partials, n_chunks, dir, slot, record);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
