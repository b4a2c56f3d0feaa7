// student_check_kernels.hip -- the --student_check monitor: one reduction that scores the student's training forward
// (a) against a second forward of the same weights on the same images (b: the fp32 family by default), accumulated on the device in a
// vector of uint64 counters (include/cosa_hip.h: the layout).
//
// Everything that is added is an integer: counts, and sums of exactly computed fp32 terms converted to 64-bit fixed point (rint of the
// term times a power of two in double: exact, then rounded half-to-even once per term).  Every maximum is an integer maximum of the bit
// pattern of a finite non-negative fp32 value, the flag word an integer OR.  So the counters do not depend on the order in which the
// wavefronts arrive: the same inputs give the same bytes on every run.
//
// Layout of the work: one wavefront per cell (b, y, x) with the class on the lane (lane l owns channels l, l + 64, l + 128, l + 192: K <=
// 256), four wavefronts per workgroup, kCellsPerWave cells per wavefront.  The two [B,K-1] logit matrices and the loss vectors are tiny:
// workgroup 0 takes them after its cells.  Counts meet in workgroup-private LDS counters and leave with one global atomic per touched slot.
#include "wave_reduce.hpp"

namespace cosa {
namespace {

constexpr int kMaxK = COSA_STUDENT_CHECK_MAX_K;
constexpr int kPerLane = kMaxK / 64;
constexpr int kCellsPerWave = 4;
constexpr int kWaves = 4;
constexpr int kHead = COSA_STUDENT_CHECK_HEAD;             // slots in front of the two per-class vectors
constexpr unsigned kInfBits = 0x7f800000u;

// slots (include/cosa_hip.h)
constexpr int kChecks = 0, kFlags = 1, kTensor0 = 2, kTensorFields = 7, kCells = 37, kDiffer = 38, kFlipHist = 39, kSignFlips = 43,
              kClsCols = 45, kLoss0 = 46, kLossFields = 4;         // (kSignFlips: cls, then clsaux)
// fields of a tensor: n, nonfinite_a, nonfinite_b, max |a-b| bits, max |b| bits, sum (a-b)^2, sum b^2
enum { fN = 0, fBadA, fBadB, fMaxD, fMaxB, fSumD2, fSumB2 };

__host__ __device__ inline bool slot_is_max(int s)
{
    if (s >= kTensor0 && s < kTensor0 + 5 * kTensorFields) {
        const int f = (s - kTensor0) % kTensorFields;
        return f == fMaxD || f == fMaxB;
    }
    return s >= kLoss0 && s < kLoss0 + 4 * kLossFields && (s - kLoss0) % kLossFields == 2;
}

// a term t >= 0 in fixed point with `frac` fractional bits, or "not representable": t >= 2^int_bits (NaN and +inf land here too).  frac +
// int_bits = 42 for every sum (include/cosa_hip.h), so 2^22 terms fit in 64 bits whatever their values
__device__ __forceinline__ bool to_fixed(float t, int frac, int int_bits, unsigned long long &out)
{
    if (!(t < ldexpf(1.0f, int_bits))) return false;
    out = (unsigned long long)llrint(ldexp((double)t, frac));
    return true;
}

// the element statistics of one tensor, per lane
struct Acc {
    unsigned n = 0, bad_a = 0, bad_b = 0, max_d = 0, max_b = 0, flag = 0;
    unsigned long long sd2 = 0, sb2 = 0;

    __device__ __forceinline__ void add(float a, float b)
    {
        const bool fa = finite_bits(a), fb = finite_bits(b);
        n++;
        bad_a += fa ? 0u : 1u;
        bad_b += fb ? 0u : 1u;
        if (fb) {
            const unsigned mb = __float_as_uint(fabsf(b));
            max_b = mb > max_b ? mb : max_b;
        }
        if (!(fa && fb)) {
            flag = 1;
            return;
        }
        const float d = __fsub_rn(a, b);
        if (finite_bits(d)) {
            const unsigned md = __float_as_uint(fabsf(d));
            max_d = md > max_d ? md : max_d;
        }
        unsigned long long t;
        if (to_fixed(__fmul_rn(d, d), COSA_STUDENT_CHECK_D2_FRAC, COSA_STUDENT_CHECK_D2_INT, t)) sd2 += t; else flag = 1;
        if (to_fixed(__fmul_rn(b, b), COSA_STUDENT_CHECK_B2_FRAC, COSA_STUDENT_CHECK_B2_INT, t)) sb2 += t; else flag = 1;
    }

    // the wavefront's totals into the workgroup's LDS counters (all lanes call)
    __device__ __forceinline__ void flush(unsigned long long *ctr, int tensor)
    {
        const unsigned n_ = wave_sum32(n), ba = wave_sum32(bad_a), bb = wave_sum32(bad_b), md = wave_max32(max_d), mb = wave_max32(max_b),
                       fl = wave_or32(flag);
        const unsigned long long s1 = wave_sum64(sd2), s2 = wave_sum64(sb2);
        if (__lane_id() == 0) {
            unsigned long long *c = ctr + kTensor0 + tensor * kTensorFields;
            if (n_) atomicAdd(&c[fN], (unsigned long long)n_);
            if (ba) atomicAdd(&c[fBadA], (unsigned long long)ba);
            if (bb) atomicAdd(&c[fBadB], (unsigned long long)bb);
            if (md) atomicMax(&c[fMaxD], (unsigned long long)md);
            if (mb) atomicMax(&c[fMaxB], (unsigned long long)mb);
            if (s1) atomicAdd(&c[fSumD2], s1);
            if (s2) atomicAdd(&c[fSumB2], s2);
            if (fl) atomicOr(&ctr[kFlags], 1ull << tensor);
        }
    }
};

struct StudentCheckArgs {
    const float *a[5], *b[5];              // seg [B,K,h,w]; cam, aux [B,K-1,h,w]; cls, clsaux [B,K-1]
    const float *loss_a, *loss_b;          // [4]
    const float *cls_label;                // [B,K-1]
    unsigned long long *counters;
    int B, K, hw;
    unsigned cells;
};

// the better of two (value, channel) candidates of an argmax: the larger value, the lower channel among equals
__device__ __forceinline__ void arg_better(float &v, int &i, float v2, int i2)
{
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}

__device__ __forceinline__ void wave_argmax(float &v, int &i)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float v2 = __shfl_xor(v, d);
        const int i2 = __shfl_xor(i, d);
        arg_better(v, i, v2, i2);
    }
}

__device__ __forceinline__ float wave_maxf(float v)        // (no NaN enters: the callers replace it by -inf)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(64 * kWaves) void student_check_kernel(const StudentCheckArgs g)
{
    __shared__ unsigned long long ctr[kHead + 2 * kMaxK];
    const int K = g.K, C = K - 1, hw = g.hw, n_slots = kHead + 2 * K;
    for (int i = threadIdx.x; i < n_slots; i += blockDim.x) ctr[i] = 0;
    __syncthreads();
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const float ninf = -__uint_as_float(kInfBits);
    Acc acc[3];
    unsigned n_cells = 0, n_differ = 0;
    const unsigned cell0 = (blockIdx.x * kWaves + wave) * kCellsPerWave;
    for (int it = 0; it < kCellsPerWave; it++) {
        const unsigned cell = cell0 + it;
        if (cell >= g.cells) break;                                                // (wave-uniform)
        const int b = cell / hw, p = cell - b * hw;
        const float *lab = g.cls_label + (size_t)b * C;
        float va[kPerLane], vb[kPerLane];                                          // seg logits as the argmax reads them: -inf where not allowed / NaN
        float best_a = ninf, best_b = ninf;
        int idx_a = 0x7fffffff, idx_b = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const int c = lane + 64 * j;
            va[j] = vb[j] = ninf;
            bool allowed = false;
            if (c < K) {
                allowed = c == 0 || lab[c - 1] != 0.0f;
                if (allowed) {
                    const size_t o = ((size_t)b * K + c) * hw + p;
                    const float xa = g.a[0][o], xb = g.b[0][o];
                    acc[0].add(xa, xb);
                    va[j] = xa != xa ? ninf : xa;
                    vb[j] = xb != xb ? ninf : xb;
                    arg_better(best_a, idx_a, va[j], c);
                    arg_better(best_b, idx_b, vb[j], c);
                }
                if (c >= 1 && allowed) {                                           // the CAM planes of the present classes
                    const size_t o = ((size_t)b * C + (c - 1)) * hw + p;
                    acc[1].add(g.a[1][o], g.b[1][o]);
                    acc[2].add(g.a[2][o], g.b[2][o]);
                }
            }
        }
        wave_argmax(best_a, idx_a);                                                // (channel 0 is always allowed: idx < K)
        wave_argmax(best_b, idx_b);
        // the check pass's top-2: the largest allowed value outside its argmax channel
        float second = ninf;
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const int c = lane + 64 * j;
            const bool allowed = c < K && (c == 0 || lab[c - 1] != 0.0f);
            if (allowed && c != idx_b && vb[j] > second) second = vb[j];
        }
        second = wave_maxf(second);
        n_cells++;
        if (lane == 0) {
            atomicAdd(&ctr[kHead + idx_b], 1ull);                                  // labelled[class of the check pass]
            if (idx_a == idx_b) {
                atomicAdd(&ctr[kHead + K + idx_b], 1ull);                          // agree[class]
            } else {
                n_differ++;
                const float m = __fsub_rn(best_b, second);                         // (+inf with a single allowed channel; NaN: the last bin)
                const int bin = m < 1e-3f ? 0 : m < 1e-2f ? 1 : m < 1e-1f ? 2 : 3;
                atomicAdd(&ctr[kFlipHist + bin], 1ull);
            }
        }
    }
    if (lane == 0) {
        if (n_cells) atomicAdd(&ctr[kCells], (unsigned long long)n_cells);
        if (n_differ) atomicAdd(&ctr[kDiffer], (unsigned long long)n_differ);
    }
    for (int t = 0; t < 3; t++) acc[t].flush(ctr, t);

    if (blockIdx.x == 0) {
        // the classification logits: statistics over the present classes' columns, sign flips over every column
        Acc cl[2];
        unsigned flips[2] = {0, 0}, cols = 0;
        const int total = g.B * C;
        for (int i = threadIdx.x; i < total; i += blockDim.x) {
            const bool present = g.cls_label[i] != 0.0f;
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const float xa = g.a[3 + t][i], xb = g.b[3 + t][i];
                if (present) cl[t].add(xa, xb);
                const int sa = (xa > 0.0f) - (xa < 0.0f), sb = (xb > 0.0f) - (xb < 0.0f);
                flips[t] += sa != sb ? 1u : 0u;
            }
            cols++;
        }
        for (int t = 0; t < 2; t++) cl[t].flush(ctr, 3 + t);
        flips[0] = wave_sum32(flips[0]);
        flips[1] = wave_sum32(flips[1]);
        cols = wave_sum32(cols);
        if (lane == 0) {
            if (flips[0]) atomicAdd(&ctr[kSignFlips], (unsigned long long)flips[0]);
            if (flips[1]) atomicAdd(&ctr[kSignFlips + 1], (unsigned long long)flips[1]);
            if (cols) atomicAdd(&ctr[kClsCols], (unsigned long long)cols);
        }
        if (threadIdx.x < 4) {
            // the loss terms: sum |a - b|, sum |b|, max |a - b| bits, checks
            const int j = threadIdx.x;
            const float xa = g.loss_a[j], xb = g.loss_b[j];
            unsigned long long *c = ctr + kLoss0 + j * kLossFields;
            unsigned long long t1, t2;
            const float d = fabsf(__fsub_rn(xa, xb));
            if (finite_bits(xa) && finite_bits(xb) && to_fixed(d, COSA_STUDENT_CHECK_LOSS_FRAC, COSA_STUDENT_CHECK_LOSS_INT, t1) &&
                to_fixed(fabsf(xb), COSA_STUDENT_CHECK_LOSS_FRAC, COSA_STUDENT_CHECK_LOSS_INT, t2)) {
                c[0] = t1;                                                          // (this thread owns the term's slots in this workgroup)
                c[1] = t2;
                c[2] = __float_as_uint(d);
            } else {
                atomicOr(&ctr[kFlags], 1ull << (8 + j));
            }
            c[3] = 1;
        }
        if (threadIdx.x == 0) ctr[kChecks] = 1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_slots; i += blockDim.x) {
        const unsigned long long v = ctr[i];
        if (!v) continue;
        if (i == kFlags) atomicOr(&g.counters[i], v);
        else if (slot_is_max(i)) atomicMax(&g.counters[i], v);
        else atomicAdd(&g.counters[i], v);
    }
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" size_t cosa_student_check_counters(int K)
{
    if (K < 2 || K > kMaxK) {
        set_error("cosa_student_check_counters: K must be in 2..%d (got %d)", kMaxK, K);
        return 0;
    }
    return (size_t)kHead + 2 * (size_t)K;
}

extern "C" int cosa_student_check(const float *seg_a, const float *seg_b, const float *cam_a, const float *cam_b, const float *aux_a,
                                  const float *aux_b, const float *cls_a, const float *cls_b, const float *clsaux_a, const float *clsaux_b,
                                  const float *loss_a, const float *loss_b, const float *cls_label, long long *counters, int B, int K, int h,
                                  int w, void *stream)
{
    COSA_REQUIRE(seg_a && seg_b && cam_a && cam_b && aux_a && aux_b && cls_a && cls_b && clsaux_a && clsaux_b && loss_a && loss_b && cls_label &&
                     counters, "cosa_student_check: null argument (every tensor pair, the loss vectors, cls_label and the counters are required)");
    COSA_REQUIRE(B > 0 && h > 0 && w > 0, "cosa_student_check: B, h and w must be positive (got B %d, h %d, w %d)", B, h, w);
    COSA_REQUIRE(K >= 2 && K <= kMaxK, "cosa_student_check: K must be in 2..%d (got %d)", kMaxK, K);
    COSA_REQUIRE((size_t)B * K * h * w < 0x7fffffffull, "cosa_student_check: tensors too large (B %d, K %d, h %d, w %d)", B, K, h, w);
    COSA_REQUIRE(((size_t)counters & 7) == 0, "cosa_student_check: counters must be 8-byte aligned");
    StudentCheckArgs g;
    g.a[0] = seg_a; g.b[0] = seg_b; g.a[1] = cam_a; g.b[1] = cam_b; g.a[2] = aux_a; g.b[2] = aux_b;
    g.a[3] = cls_a; g.b[3] = cls_b; g.a[4] = clsaux_a; g.b[4] = clsaux_b;
    g.loss_a = loss_a; g.loss_b = loss_b; g.cls_label = cls_label;
    g.counters = reinterpret_cast<unsigned long long *>(counters);
    g.B = B; g.K = K; g.hw = h * w;
    g.cells = (unsigned)B * (unsigned)(h * w);
    const unsigned per_wg = kWaves * kCellsPerWave, wgs = (g.cells + per_wg - 1) / per_wg;
    hipLaunchKernelGGL(student_check_kernel, dim3(wgs), dim3(64 * kWaves), 0, as_stream(stream), g);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
