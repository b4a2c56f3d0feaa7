// teacher_check_kernels.hip -- the --teacher_check monitor: one reduction that scores two teacher passes (the same
// weights and images on two operand modes) against each other, accumulated on the device in a vector of uint64 counters.
//
// Everything that is added is an integer; the per-plane figure max |a - b| is a float maximum of exactly computed fp32 differences (no
// NaN ever enters it), kept as its bit pattern and combined with integer atomic maxima: the same bits in any order, on every run.
#include "student_label.hpp"      // label_slot, load_f32x4; wave_reduce.hpp: wave_sum32, wave_max, wave_count, nonfinite_bits

namespace cosa {
namespace {

constexpr int kSets = 3;                   // map sets: cam, aux, tgt
constexpr int kPairs = 2;                  // label pairs: main, aux
constexpr int kBins = COSA_TEACHER_CHECK_BINS;
constexpr int kMaxK = 256;                 // K = C + 1, C <= 255
constexpr int kPairSlots = 4 + 3 * kMaxK;  // pix, agree, ign_a, ign_b, cnt_a[K], cnt_b[K], inter[K]
constexpr unsigned kChunk = 4096;          // elements of a plane per workgroup of the map pass: 256 threads x 4 items x 4 elements
constexpr unsigned kInfBits = 0x7f800000u;

// THE definition of the counter vector (uint64 elements) for the device and the host: off[] of, in order, checks; then for each map
// set (cam, aux, tgt): planes, over, worst, hist[8], nonfinite_a, nonfinite_b; then for each label pair (main, aux): pix, agree,
// ign_a, ign_b, cnt_a[K], cnt_b[K], inter[K]; -> the number of elements (48 + 6K)
__host__ __device__ inline int teacher_check_offsets(int K, int (&off)[COSA_TEACHER_CHECK_SLOTS])
{
    int i = 0, o = 0;
    off[i++] = o; o += 1;                                  // checks
    for (int s = 0; s < kSets; s++) {
        off[i++] = o; o += 1;                              // planes
        off[i++] = o; o += 1;                              // over
        off[i++] = o; o += 1;                              // worst
        off[i++] = o; o += kBins;                          // hist
        off[i++] = o; o += 1;                              // nonfinite_a
        off[i++] = o; o += 1;                              // nonfinite_b
    }
    for (int p = 0; p < kPairs; p++) {
        off[i++] = o; o += 1;                              // pix
        off[i++] = o; o += 1;                              // agree
        off[i++] = o; o += 1;                              // ign_a
        off[i++] = o; o += 1;                              // ign_b
        off[i++] = o; o += K;                              // cnt_a
        off[i++] = o; o += K;                              // cnt_b
        off[i++] = o; o += K;                              // inter
    }
    return o;
}

struct TeacherCheckArgs {
    const float *a[kSets], *b[kSets];      // the two passes of a map set; both NULL: the set is absent
    unsigned n[kSets];                     // elements of a plane
    unsigned chunks[kSets];                // workgroups per plane
    unsigned first[kSets + 1];             // first workgroup of a set; first[kSets]: first workgroup of the label pass
    int vec[kSets];                        // a plane may be read as float4
    const float *la[kPairs], *lb[kPairs];  // the label maps of a pair; both NULL: the pair is absent
    const float *cls;                      // [B,C] or NULL: every plane is active
    const int32_t *boxes;
    unsigned long long *counters;
    unsigned int *fig;                     // workspace: [kSets][B*C] bit patterns of the planes' figures, zeroed by the call
    int B, C, K, S, lvec;
    float ignore;
};

// the map pass of one workgroup: kChunk elements of ONE plane of one set.  A plane of an absent class is left before its first load.
__device__ __forceinline__ void map_chunk(const TeacherCheckArgs &a, int set, unsigned wg, const int (&off)[COSA_TEACHER_CHECK_SLOTS])
{
    const unsigned plane = wg / a.chunks[set], chunk = wg - plane * a.chunks[set];          // plane < B*C (grid size)
    if (a.cls && a.cls[plane] == 0.0f) return;                                              // (workgroup-uniform)
    const unsigned n = a.n[set];
    const float *pa = a.a[set] + (size_t)plane * n, *pb = a.b[set] + (size_t)plane * n;
    float fig = 0.0f;
    unsigned bad_a = 0, bad_b = 0;
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const unsigned e = chunk * kChunk + (it * 256u + threadIdx.x) * 4u;
        if (e >= n) continue;
        float va[4], vb[4];
        load_f32x4(pa + e, (int)e, (int)n, a.vec[set], va);          // (vec: n % 4 == 0, so e + 3 < n; n < 2^31: entry point)
        load_f32x4(pb + e, (int)e, (int)n, a.vec[set], vb);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool na = nonfinite_bits(va[k]), nb = nonfinite_bits(vb[k]);
            bad_a += na ? 1u : 0u;
            bad_b += nb ? 1u : 0u;
            // a non-finite element in either pass makes the plane's figure +inf; a - b of two finite values is finite or +-inf, never NaN
            fig = fmaxf(fig, (na || nb) ? __uint_as_float(kInfBits) : fabsf(va[k] - vb[k]));
        }
    }
    fig = wave_max(fig);
    bad_a = wave_sum32(bad_a);
    bad_b = wave_sum32(bad_b);
    if (__lane_id() == 0) {
        // non-negative floats order as their bit patterns: an integer maximum, exact in any order
        if (fig > 0.0f) atomicMax(&a.fig[(size_t)set * a.B * a.C + plane], __float_as_uint(fig));
        if (bad_a) atomicAdd(&a.counters[off[1 + 6 * set + 4]], (unsigned long long)bad_a);
        if (bad_b) atomicAdd(&a.counters[off[1 + 6 * set + 5]], (unsigned long long)bad_b);
    }
}

// the label pass of one workgroup: 256 items of four adjacent pixels of a row, both pairs
__device__ __forceinline__ void label_chunk(const TeacherCheckArgs &a, unsigned wg, unsigned long long *ctr)
{
    const int S = a.S, K = a.K, S4 = (S + 3) >> 2;
    const unsigned per_img = (unsigned)S * S4, total = per_img * a.B;                        // < 2^31 (entry point)
    const unsigned item = wg * 256u + threadIdx.x;
    bool in[4] = {false, false, false, false};
    int b = 0, Y = 0, X = 0;
    if (item < total) {
        b = item / per_img;
        const unsigned r = item - b * per_img;
        Y = r / S4;
        X = (r - Y * S4) * 4;
        const int32_t *bx = a.boxes + 4 * b;
        const bool row_in = Y >= bx[0] && Y < bx[1];
#pragma unroll
        for (int k = 0; k < 4; k++) in[k] = row_in && X + k >= bx[2] && X + k < bx[3] && X + k < S;
    }
    const bool any = in[0] || in[1] || in[2] || in[3];
    const size_t o = ((size_t)b * S + Y) * S + X;
    unsigned n_pix = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) n_pix += in[k] ? 1u : 0u;
    n_pix = wave_sum32(n_pix);
    for (int p = 0; p < kPairs; p++) {
        if (!a.la[p]) continue;                                                              // (uniform)
        float va[4] = {0.0f, 0.0f, 0.0f, 0.0f}, vb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (any) {
            if (a.lvec) {                                    // (both maps under ONE branch: two load_f32x4 calls cost 7 SGPRs)
                const float4 ta = *reinterpret_cast<const float4 *>(a.la[p] + o), tb = *reinterpret_cast<const float4 *>(a.lb[p] + o);
                va[0] = ta.x; va[1] = ta.y; va[2] = ta.z; va[3] = ta.w;
                vb[0] = tb.x; vb[1] = tb.y; vb[2] = tb.z; vb[3] = tb.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    va[k] = X + k < S ? a.la[p][o + k] : 0.0f;
                    vb[k] = X + k < S ? a.lb[p][o + k] : 0.0f;
                }
            }
        }
        unsigned long long *c = ctr + p * kPairSlots;
        unsigned n_agree = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int sa = label_slot(va[k], K, a.ignore), sb = label_slot(vb[k], K, a.ignore);
            n_agree += (in[k] && va[k] == vb[k]) ? 1u : 0u;
            // slots of a pair in LDS: [pix, agree, ign_a, ign_b, cnt_a[K], cnt_b[K], inter[K]]
            wave_count(c, sa == K ? 2 : 4 + sa, in[k] && sa >= 0);
            wave_count(c, sb == K ? 3 : 4 + K + sb, in[k] && sb >= 0);
            wave_count(c, 4 + 2 * K + sa, in[k] && sa >= 0 && sa < K && sa == sb);
        }
        n_agree = wave_sum32(n_agree);
        if (__lane_id() == 0) {
            if (n_pix) atomicAdd(&c[0], (unsigned long long)n_pix);
            if (n_agree) atomicAdd(&c[1], (unsigned long long)n_agree);
        }
    }
}

// Workgroups [first[s], first[s+1]) own set s's planes, chunks[s] each; the rest own the label maps.  Counts of the label pass meet in
// workgroup-private LDS counters and leave with one global integer atomic per non-zero slot.
__global__ __launch_bounds__(256) void teacher_check_kernel(const TeacherCheckArgs a)
{
    __shared__ unsigned long long ctr[kPairs * kPairSlots];
    int off[COSA_TEACHER_CHECK_SLOTS];
    teacher_check_offsets(a.K, off);
    const unsigned wg = blockIdx.x;
    if (wg < a.first[kSets]) {
        const int set = wg >= a.first[2] ? 2 : (wg >= a.first[1] ? 1 : 0);
        map_chunk(a, set, wg - a.first[set], off);
        return;
    }
    const int per = 4 + 3 * a.K;
    for (int p = 0; p < kPairs; p++)
        for (int i = threadIdx.x; i < per; i += 256) ctr[p * kPairSlots + i] = 0;
    __syncthreads();
    label_chunk(a, wg - a.first[kSets], ctr);
    __syncthreads();
    for (int p = 0; p < kPairs; p++) {
        if (!a.la[p]) continue;
        const int base = off[1 + 6 * kSets + 7 * p];                                       // the pair's slots are contiguous from `pix` on
        for (int i = threadIdx.x; i < per; i += 256)          // (flush_counters' loop written out: the helper moves this kernel's register count)
            if (ctr[p * kPairSlots + i]) atomicAdd(&a.counters[base + i], ctr[p * kPairSlots + i]);
    }
}

// after teacher_check_kernel on the same stream: one thread per (set, plane) bins the plane's figure; thread 0 counts the check
__global__ __launch_bounds__(256) void teacher_check_finish_kernel(const TeacherCheckArgs a, float bar)
{
    __shared__ unsigned int cnt[kSets][2 + kBins];          // planes, over, hist
    __shared__ unsigned int worst[kSets];
    for (int i = threadIdx.x; i < kSets * (2 + kBins); i += 256) (&cnt[0][0])[i] = 0;
    if (threadIdx.x < kSets) worst[threadIdx.x] = 0;
    __syncthreads();
    int off[COSA_TEACHER_CHECK_SLOTS];
    teacher_check_offsets(a.K, off);
    const unsigned planes = (unsigned)a.B * a.C, t = blockIdx.x * 256u + threadIdx.x;
    if (t < kSets * planes) {
        const unsigned set = t / planes, plane = t - set * planes;
        if (a.a[set] && (!a.cls || a.cls[plane] != 0.0f)) {
            const unsigned bits = a.fig[t];
            const float fig = __uint_as_float(bits);
            const float edge[kBins] = {1e-6f, 1e-5f, 1e-4f, 3e-4f, 1e-3f, 3e-3f, 1e-2f, __uint_as_float(kInfBits)};
            int bin = 0;
            while (bin < kBins - 1 && !(fig <= edge[bin])) bin++;
            atomicAdd(&cnt[set][0], 1u);
            if (fig > bar) atomicAdd(&cnt[set][1], 1u);
            atomicAdd(&cnt[set][2 + bin], 1u);
            atomicMax(&worst[set], bits);
        }
    }
    __syncthreads();
    if (threadIdx.x < kSets * (2 + kBins)) {
        const int set = threadIdx.x / (2 + kBins), i = threadIdx.x % (2 + kBins);
        // planes, over | hist: `worst` sits between over and hist in the vector
        const int slot = i < 2 ? off[1 + 6 * set + i] : off[1 + 6 * set + 3] + (i - 2);
        if (cnt[set][i]) atomicAdd(&a.counters[slot], (unsigned long long)cnt[set][i]);
    }
    if (threadIdx.x < kSets && worst[threadIdx.x]) atomicMax(&a.counters[off[1 + 6 * threadIdx.x + 2]], (unsigned long long)worst[threadIdx.x]);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counters[off[0]], 1ull);
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" size_t cosa_teacher_check_layout(int K, size_t *offsets)
{
    if (!offsets || K < 2 || K > kMaxK) {
        set_error("cosa_teacher_check_layout: K must be in 2..%d (got %d) and offsets non-null", kMaxK, K);
        return 0;
    }
    int off[COSA_TEACHER_CHECK_SLOTS];
    const int n = teacher_check_offsets(K, off);
    for (int i = 0; i < COSA_TEACHER_CHECK_SLOTS; i++) offsets[i] = (size_t)off[i];
    return (size_t)n;
}

extern "C" size_t cosa_teacher_check_workspace_bytes(int B, int C)
{
    if (B <= 0 || C <= 0 || C > kMaxK - 1) return 0;
    return (size_t)kSets * B * C * sizeof(unsigned int);
}

extern "C" int cosa_teacher_check(const float *camA, const float *camB, const float *auxA, const float *auxB, const float *tgtA,
                                  const float *tgtB, const float *mainA, const float *mainB, const float *lauxA, const float *lauxB,
                                  const float *cls_label, const int32_t *boxes, int B, int C, int K, int S, int h, int w, int ignore_index,
                                  float bar, unsigned long long *counters, void *workspace, size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(camA && camB && auxA && auxB && mainA && mainB && boxes && counters && workspace,
                 "cosa_teacher_check: null argument (only the tgt pair, the auxiliary label pair and cls_label may be NULL)");
    COSA_REQUIRE((tgtA == nullptr) == (tgtB == nullptr) && (lauxA == nullptr) == (lauxB == nullptr),
                 "cosa_teacher_check: a pair is given whole or not at all");
    COSA_REQUIRE(C >= 1 && C <= kMaxK - 1 && K == C + 1, "cosa_teacher_check: C must be in 1..%d and K == C + 1 (got C %d, K %d)", kMaxK - 1, C, K);
    COSA_REQUIRE(B > 0 && S > 0 && (!tgtA || (h > 0 && w > 0 && h <= S && w <= S)),
                 "cosa_teacher_check: sizes outside the envelope (B %d, S %d, h %d, w %d: all > 0, h and w <= S)", B, S, h, w);
    COSA_REQUIRE(ignore_index < 0 || ignore_index >= K, "cosa_teacher_check: ignore_index %d is a class index (K %d)", ignore_index, K);
    COSA_REQUIRE(bar >= 0.0f, "cosa_teacher_check: the bar must be a non-negative number");
    COSA_REQUIRE((size_t)S * S < 0x7fffffffull && (size_t)B * S * ((S + 3) / 4) < 0x7fffffffull, "cosa_teacher_check: maps too large (B %d, S %d)", B, S);
    COSA_REQUIRE((((size_t)counters | (size_t)workspace) & 7) == 0, "cosa_teacher_check: counters and workspace must be 8-byte aligned");
    const size_t need = cosa_teacher_check_workspace_bytes(B, C);
    COSA_REQUIRE(workspace_bytes >= need, "cosa_teacher_check: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    TeacherCheckArgs a;
    a.a[0] = camA; a.b[0] = camB; a.a[1] = auxA; a.b[1] = auxB; a.a[2] = tgtA; a.b[2] = tgtB;
    a.la[0] = mainA; a.lb[0] = mainB; a.la[1] = lauxA; a.lb[1] = lauxB;
    a.cls = cls_label; a.boxes = boxes; a.counters = counters; a.fig = (unsigned int *)workspace;
    a.B = B; a.C = C; a.K = K; a.S = S; a.ignore = (float)ignore_index;
    const size_t planes = (size_t)B * C;
    size_t wgs = 0;
    for (int s = 0; s < kSets; s++) {
        const bool on = a.a[s] != nullptr;
        const int width = s < 2 ? S : w;
        a.n[s] = s < 2 ? (unsigned)S * S : (on ? (unsigned)h * w : 0u);
        a.chunks[s] = on ? (a.n[s] + kChunk - 1) / kChunk : 0u;
        // float4 where a row is a whole number of them (then so is a plane) and the bases are 16-byte aligned
        a.vec[s] = on && (width & 3) == 0 && ((((size_t)a.a[s] | (size_t)a.b[s]) & 15) == 0);
        a.first[s] = (unsigned)wgs;
        wgs += planes * a.chunks[s];
    }
    a.first[kSets] = (unsigned)wgs;
    a.lvec = (S & 3) == 0 && ((((size_t)mainA | (size_t)mainB | (size_t)lauxA | (size_t)lauxB) & 15) == 0);
    wgs += ((size_t)B * S * ((S + 3) / 4) + 255) / 256;
    COSA_REQUIRE(wgs < 0x7fffffffull, "cosa_teacher_check: too many workgroups (B %d, C %d, S %d)", B, C, S);
    hipStream_t st = as_stream(stream);
    COSA_HIP_CHECK(hipMemsetAsync(workspace, 0, need, st));
    hipLaunchKernelGGL(teacher_check_kernel, dim3((unsigned)wgs), dim3(256), 0, st, a);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(teacher_check_finish_kernel, dim3((unsigned)((kSets * planes + 255) / 256)), dim3(256), 0, st, a, bar);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
