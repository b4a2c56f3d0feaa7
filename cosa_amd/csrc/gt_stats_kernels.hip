// gt_stats_kernels.hip -- --gt_stats: the confusion matrices of the main pseudo-label map, the auxiliary one and the
// student's prediction against the ground truth of the training crops, one reduction per step over tensors the step already holds.
//
// The ground truth is monitoring data only: nothing here writes anything the training step reads.  Compiled with -ffp-contract=off: the
// student's label is student_label.hpp's, the one cosa_label_stats counts, evaluated by the same calls.
#include "kernels.hpp"
#include "student_label.hpp"

namespace cosa {
namespace {

// LDS the histogram of one workgroup may take: a quarter of a CU's 160 KiB, so that the four workgroups per CU of the grid stay resident.
// 2K(K+1) + K^2 u32 counters: K <= 58 fits (VOC's 21: 5.3 KiB), COCO's 81 (78 KiB) counts in global memory.
constexpr size_t kGtStatsLdsBytes = 40 * 1024;

// THE definition of the counter vector (uint64 elements) for the device and the host: off[i] of steps, pix, valid, gt_other, main[K][K+1],
// aux[K][K+1], student[K][K]; -> the number of elements
__host__ __device__ inline int gt_stats_offsets(int K, int (&off)[COSA_GT_STATS_SLOTS])
{
    off[0] = 0;                        // steps
    off[1] = 1;                        // pix
    off[2] = 2;                        // valid
    off[3] = 3;                        // gt_other
    off[4] = 4;                        // main[K][K+1]
    off[5] = off[4] + K * (K + 1);     // aux[K][K+1]
    off[6] = off[5] + K * (K + 1);     // student[K][K]
    return off[6] + K * K;
}

struct GtStatsArgs {
    const uint8_t *gt;
    const float *mask_main, *mask_aux, *seg, *cls;
    const int32_t *boxes;
    unsigned long long *counters;
    int B, K, S, h, w;
    int vec, vec_gt;                        // every row of the masks may be read as float4 / of gt as one dword
    float sy, sx, ignore;
};

// The iteration of label_stats_kernel: a thread owns four adjacent pixels of a row, a wavefront's 64 items lie in one image (two or more
// only across an image boundary or at tiny S).  gt is read first: a thread none of whose pixels is inside the box with a class as ground
// truth reads neither mask nor logits.  kLds: the three matrices meet in workgroup-private u32 LDS counters (a workgroup counts fewer
// than 2^31 pixels) and leave with one 64-bit global atomic per non-zero entry; otherwise the counts go to the global counters
// directly.  Either way through wave_count_mixed: a crop of real ground truth shows a wavefront a handful of (class, label) pairs, which leave
// aggregated; a speckled map costs one more atomic per lane instead of a round per pair.  Integer atomics only: the same bytes in any order.
template <bool kLds>
__global__ __launch_bounds__(256) void gt_stats_kernel(const GtStatsArgs a)
{
    extern __shared__ unsigned int hist[];                  // kLds: main | aux | student, the layout's order
    __shared__ unsigned int scal[3];                        // pix, valid, gt_other
    const int S = a.S, K = a.K, S4 = (S + 3) >> 2;
    const int nm = K * (K + 1), T = 2 * nm + K * K;
    if (kLds)
        for (int i = threadIdx.x; i < T; i += 256) hist[i] = 0;
    if (threadIdx.x < 3) scal[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long *gmat = a.counters + 4;
    const unsigned per_img = (unsigned)S * S4, total = per_img * a.B;          // < 2^31 (entry point)
    const size_t hw = (size_t)a.h * a.w;
    const int lane = (int)__lane_id();
    const unsigned wave_off = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    unsigned n_pix = 0, n_valid = 0, n_other = 0;
    for (unsigned base = blockIdx.x * 256u + wave_off; base < total; base += gridDim.x * 256u) {          // (wave-uniform)
        const unsigned item = base + lane;
        const unsigned last = base + 63 < total - 1 ? base + 63 : total - 1;
        const int b_lo = base / per_img, b_hi = last / per_img;
        bool ok[4] = {false, false, false, false};          // inside the box, ground truth a class
        int g[4] = {0, 0, 0, 0}, iv[4] = {0, 0, 0, 0};
        float mv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, av[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int b = -1, Y = 0, X = 0;
        bool any = false;
        if (item < total) {
            b = item / per_img;
            const unsigned r = item - b * per_img;
            Y = r / S4;
            X = (r - Y * S4) * 4;
            const int32_t *bx = a.boxes + 4 * b;
            const bool row_in = Y >= bx[0] && Y < bx[1];
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; k++) in[k] = row_in && X + k >= bx[2] && X + k < bx[3] && X + k < S;
            if (in[0] || in[1] || in[2] || in[3]) {
                const size_t o = ((size_t)b * S + Y) * S + X;
                if (a.vec_gt) {
                    const unsigned int v = *reinterpret_cast<const unsigned int *>(a.gt + o);
#pragma unroll
                    for (int k = 0; k < 4; k++) g[k] = (int)((v >> (8 * k)) & 0xffu);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) g[k] = X + k < S ? (int)a.gt[o + k] : 255;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    ok[k] = in[k] && g[k] < K;
                    n_pix += in[k] ? 1u : 0u;
                    n_valid += ok[k] ? 1u : 0u;
                    n_other += (in[k] && g[k] >= K && g[k] != 255) ? 1u : 0u;
                }
                any = ok[0] || ok[1] || ok[2] || ok[3];
                if (any) {
                    load_f32x4(a.mask_main + o, X, S, a.vec, mv);
                    if (a.mask_aux) load_f32x4(a.mask_aux + o, X, S, a.vec, av);
                }
            }
        }
        for (int bb = b_lo; bb <= b_hi; bb++) {
            unsigned long long present[2];
            present_classes(a.cls, bb, K, lane, present);
            if (any && b == bb) student_label4(a.seg + (size_t)bb * K * hw, K, a.h, a.w, a.sy, a.sx, S, Y, X, present, iv);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int gk = ok[k] ? g[k] : 0;
            const int m = label_slot(mv[k], K, a.ignore), x = label_slot(av[k], K, a.ignore);
            if (kLds) {
                wave_count_mixed(hist, gk * (K + 1) + m, ok[k] && m >= 0);
                if (a.mask_aux) wave_count_mixed(hist + nm, gk * (K + 1) + x, ok[k] && x >= 0);
                wave_count_mixed(hist + 2 * nm, gk * K + iv[k], ok[k]);
            } else {
                wave_count_mixed(gmat, gk * (K + 1) + m, ok[k] && m >= 0);
                if (a.mask_aux) wave_count_mixed(gmat + nm, gk * (K + 1) + x, ok[k] && x >= 0);
                wave_count_mixed(gmat + 2 * nm, gk * K + iv[k], ok[k]);
            }
        }
    }
    if (n_pix) atomicAdd(&scal[0], n_pix);
    if (n_valid) atomicAdd(&scal[1], n_valid);
    if (n_other) atomicAdd(&scal[2], n_other);
    __syncthreads();
    flush_counters(scal, a.counters + 1, 3, 256);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&a.counters[0], 1ull);          // steps
    if (kLds) flush_counters(hist, gmat, T, 256);
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" size_t cosa_gt_stats_layout(int K, size_t *offsets)
{
    if (!offsets || K < 2 || K > kStatsMaxK) {
        set_error("cosa_gt_stats_layout: K must be in 2..%d (got %d) and offsets non-null", kStatsMaxK, K);
        return 0;
    }
    int off[COSA_GT_STATS_SLOTS];
    const int n = gt_stats_offsets(K, off);
    for (int i = 0; i < COSA_GT_STATS_SLOTS; i++) offsets[i] = (size_t)off[i];
    return (size_t)n;
}

extern "C" int cosa_gt_stats(const uint8_t *gt, const float *mask_main, const float *mask_aux, const float *seg_logits, const float *cls_label,
                             const int32_t *boxes, int B, int K, int S, int h, int w, int ignore_index, unsigned long long *counters,
                             void *stream)
{
    COSA_REQUIRE(gt && mask_main && seg_logits && cls_label && boxes && counters, "cosa_gt_stats: null argument (only mask_aux may be NULL)");
    COSA_REQUIRE(K >= 2 && K <= kStatsMaxK, "cosa_gt_stats: K must be in 2..%d (got %d)", kStatsMaxK, K);
    COSA_REQUIRE(B > 0 && S > 0 && h > 0 && w > 0 && h <= S && w <= S,
                 "cosa_gt_stats: sizes outside the envelope (B %d, S %d, h %d, w %d: all > 0, h and w <= S)", B, S, h, w);
    COSA_REQUIRE(ignore_index < 0 || ignore_index >= K, "cosa_gt_stats: ignore_index %d is a class index (K %d)", ignore_index, K);
    COSA_REQUIRE((size_t)B * S * ((S + 3) / 4) < 0x7fffffffull, "cosa_gt_stats: maps too large (B %d, S %d)", B, S);
    COSA_REQUIRE(((size_t)counters & 7) == 0, "cosa_gt_stats: counters must be 8-byte aligned");
    COSA_REQUIRE(((((size_t)mask_main | (size_t)mask_aux | (size_t)seg_logits | (size_t)cls_label | (size_t)boxes)) & 3) == 0,
                 "cosa_gt_stats: masks, logits, labels and boxes must be 4-byte aligned");
    GtStatsArgs a;
    a.gt = gt; a.mask_main = mask_main; a.mask_aux = mask_aux; a.seg = seg_logits; a.cls = cls_label; a.boxes = boxes; a.counters = counters;
    a.B = B; a.K = K; a.S = S; a.h = h; a.w = w;
    a.sy = (float)h / (float)S; a.sx = (float)w / (float)S; a.ignore = (float)ignore_index;
    a.vec = (S & 3) == 0 && ((((size_t)mask_main | (size_t)mask_aux) & 15) == 0);
    a.vec_gt = (S & 3) == 0 && (((size_t)gt & 3) == 0);
    const unsigned groups = ((unsigned)B * S * ((S + 3) / 4) + 255u) / 256u;          // label_stats' grid
    const unsigned rounds = (groups + kStatsMaxGroups - 1) / kStatsMaxGroups;
    const unsigned grid = (groups + rounds - 1) / rounds;
    const size_t lds = ((size_t)2 * K * (K + 1) + (size_t)K * K) * sizeof(unsigned int);
    if (lds <= kGtStatsLdsBytes)
        hipLaunchKernelGGL(gt_stats_kernel<true>, dim3(grid), dim3(256), lds, as_stream(stream), a);
    else
        hipLaunchKernelGGL(gt_stats_kernel<false>, dim3(grid), dim3(256), 0, as_stream(stream), a);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

// which path a K takes (1: the LDS histogram, 0: global atomics; -1 on bad K): for tests and tools
extern "C" int cosa_gt_stats_uses_lds(int K)
{
    if (K < 2 || K > kStatsMaxK) return -1;
    return ((size_t)2 * K * (K + 1) + (size_t)K * K) * sizeof(unsigned int) <= kGtStatsLdsBytes ? 1 : 0;
}
