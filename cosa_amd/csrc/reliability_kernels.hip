// reliability_kernels.hip -- the per-pixel weight of the reliability-weighted seg loss: how far the CAM that gave a
// pseudo label lies from the threshold it passed.  This project's own weighting; the reference keeps only the loss that takes such a map
// (utils/seg_helper.py:823-835, seg_weightloss) and the flag --camweight_beta.
//
//   cosa_label_reliability   G CAM sets [B,C,S,S], their label maps [B,S,S] and thresholds -> G weight maps [B,S,S] in [0, 1], one launch
//
// Per pixel, all fp32 in this order (l = (int)mask, y = the image's class row):
//   l == 0        m = max_c (y[c] * cam[c]),  r = (lo - m) / lo
//   1 <= l <= C   v = y[l-1] * cam[l-1],      r = (v - hi) / (1 - hi)
//   otherwise     w = 0, and the pixel enters no statistic
//   r = (r != r) ? 0 : min(max(r, 0), 1)
//   u = 1 (beta == 0) | r (beta == 1) | (r == 0 ? 0 : exp2f(beta * log2f(r)))
//   w = floor + (1 - floor) * u, 1 - floor formed once on the host
// The plane of a class that is absent from y is never read: its product counts as 0, so the maximum starts at 0 exactly when a class is
// absent.  A NaN in a plane that is read stays a NaN through the maximum (as torch.amax keeps it) and ends as r = 0.
// Statistics: Sum rint(w 2^32) and the pixel count per set and group (background / foreground), wave butterflies and 64-bit integer atomics:
// the same input gives the same bytes on every run.  Built with -ffp-contract=off.
#include "kernels.hpp"
#include "wave_reduce.hpp"

namespace cosa {
namespace {

constexpr int RG = 4;              // CAM sets per launch
constexpr int RPX = 4;             // pixels per thread
constexpr int RMAXC = 255;

struct RelSets {
    const float *cam[RG], *mask[RG];
    float *rel[RG];
    float hi[RG], lo[RG];
};

__device__ __forceinline__ float nan_max(float m, float v) { return (m != m) ? m : ((v != v || v > m) ? v : m); }

struct RelSums { unsigned long long s_bg, s_fg; unsigned n_bg, n_fg; };       // a thread's share of the statistics
struct RelParams { float hi, lo, beta, floor, one_minus_floor; };

// the four pixels p0 .. p0 + 3 of one image and set: their weights written, their statistics added to `sums`.  VEC: S*S % 4 == 0 and every base
// pointer 16-byte aligned -- the four pixels are one float4; otherwise four bounded scalar accesses (the image's base is then not 16-byte
// aligned, and the last thread's pixels may end early).  yv / present / np: the image's class row and present-class list, in LDS.
template <bool VEC>
__device__ __forceinline__ void weigh_pixels(const float *__restrict__ cam, const float *__restrict__ mask, float *__restrict__ rel, long long p0,
                                             long long SS, int C, const float *yv, const unsigned char *present, int np, const RelParams &pr,
                                             RelSums &sums)
{
    const int live = p0 >= SS ? 0 : (SS - p0 < RPX ? (int)(SS - p0) : RPX);        // pixels of this thread inside the map
    float lab[RPX] = {255.f, 255.f, 255.f, 255.f};
    if (VEC) {
        if (live) {
            const float4 q = *reinterpret_cast<const float4 *>(mask + p0);
            lab[0] = q.x; lab[1] = q.y; lab[2] = q.z; lab[3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < RPX; j++)
            if (j < live) lab[j] = mask[p0 + j];
    }
    int l[RPX];
    bool any = false;
#pragma unroll
    for (int j = 0; j < RPX; j++) {
        const int v = (int)lab[j];
        l[j] = (j < live && v >= 0 && v <= C) ? v : -1;           // -1: ignored (255, outside the classes, outside the map)
        any = any || l[j] >= 0;
    }
    float m[RPX], own[RPX];
#pragma unroll
    for (int j = 0; j < RPX; j++) {
        m[j] = np < C ? 0.f : -INFINITY;
        own[j] = 0.f;
    }
    if (any) {
        for (int i = 0; i < np; i++) {
            const int c = present[i];
            const float y = yv[c];
            const float *pl = cam + (size_t)c * SS + p0;
            float x[RPX] = {0.f, 0.f, 0.f, 0.f};
            if (VEC) {
                const float4 q = *reinterpret_cast<const float4 *>(pl);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < RPX; j++)
                    if (j < live) x[j] = pl[j];
            }
#pragma unroll
            for (int j = 0; j < RPX; j++) {
                const float v = y * x[j];
                m[j] = nan_max(m[j], v);
                if (l[j] - 1 == c) own[j] = v;
            }
        }
    }
    float w[RPX];
#pragma unroll
    for (int j = 0; j < RPX; j++) {
        w[j] = 0.f;
        if (l[j] < 0) continue;
        float r = l[j] == 0 ? (pr.lo - m[j]) / pr.lo : (own[j] - pr.hi) / (1.0f - pr.hi);
        r = (r != r) ? 0.f : fminf(fmaxf(r, 0.f), 1.f);
        const float u = pr.beta == 0.f ? 1.f : (pr.beta == 1.f ? r : (r == 0.f ? 0.f : exp2f(pr.beta * log2f(r))));
        w[j] = pr.floor + pr.one_minus_floor * u;
        const unsigned long long q = (unsigned long long)__builtin_rint((double)w[j] * 4294967296.0);
        if (l[j] == 0) { sums.s_bg += q; sums.n_bg++; } else { sums.s_fg += q; sums.n_fg++; }
    }
    if (VEC) {
        if (live) *reinterpret_cast<float4 *>(rel + p0) = make_float4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < RPX; j++)
            if (j < live) rel[p0 + j] = w[j];
    }
}

constexpr int RBLOCKS = 32;        // workgroups per image and set, at most

// grid (min(pixel chunks, RBLOCKS), B, G): a workgroup builds its image's class list once and walks chunks of 256 x RPX pixels with the
// grid's stride -- the four statistics of a set meet in four addresses, and a workgroup per chunk (3136 per set at b = 16 x 448^2) spent
// most of the launch queueing its atomics there.
template <bool VEC>
__global__ __launch_bounds__(256) void label_reliability_kernel(RelSets sets, const float *__restrict__ labels, const float *__restrict__ thr_dev, int C,
                                                               long long SS, float beta, float floor, float one_minus_floor,
                                                               unsigned long long *__restrict__ stats)
{
    __shared__ float yv[RMAXC];                 // the image's class row
    __shared__ unsigned char present[RMAXC];    // its present classes in ascending order
    __shared__ int npres;
    __shared__ unsigned long long red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, g = blockIdx.z;
    for (int c = tid; c < C; c += 256) yv[c] = labels[(size_t)b * C + c];
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int c = 0; c < C; c++)
            if (yv[c] != 0.f) present[n++] = (unsigned char)c;
        npres = n;
    }
    __syncthreads();
    const int np = npres;
    const RelParams pr = {thr_dev ? thr_dev[2 * g] : sets.hi[g], thr_dev ? thr_dev[2 * g + 1] : sets.lo[g], beta, floor, one_minus_floor};
    const float *__restrict__ cam = sets.cam[g] + (size_t)b * C * SS;
    const float *__restrict__ mask = sets.mask[g] + (size_t)b * SS;
    float *__restrict__ rel = sets.rel[g] + (size_t)b * SS;
    RelSums sums = {0ull, 0ull, 0u, 0u};
    const long long chunks = (SS + 256 * RPX - 1) / (256 * RPX);
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x)
        weigh_pixels<VEC>(cam, mask, rel, (chunk * 256 + tid) * RPX, SS, C, yv, present, np, pr, sums);
    if (!stats) return;                                             // (uniform over the launch)
    const unsigned long long s_bg = wave_sum64(sums.s_bg), s_fg = wave_sum64(sums.s_fg);
    const unsigned n_bg = wave_sum32(sums.n_bg), n_fg = wave_sum32(sums.n_fg);
    if (lane == 0) { red[wave][0] = s_bg; red[wave][1] = n_bg; red[wave][2] = s_fg; red[wave][3] = n_fg; }
    __syncthreads();
    if (tid < 4) {
        const unsigned long long t = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        if (t) atomicAdd(&stats[g * 4 + tid], t);
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_label_reliability(const float *const *cams, const float *labels, const float *const *masks, float *const *rel,
                                      const float *thr_hi, const float *thr_lo, const float *thr_dev, int G, int B, int C, int S, float beta,
                                      float floor, long long *stats, void *stream)
{
    COSA_REQUIRE(cams && labels && masks && rel, "cosa_label_reliability: null pointer");
    COSA_REQUIRE(thr_dev || (thr_hi && thr_lo), "cosa_label_reliability: thresholds on the host (thr_hi, thr_lo) or on the device (thr_dev)");
    COSA_REQUIRE(G >= 1 && G <= RG, "cosa_label_reliability: 1 to %d CAM sets (got %d)", RG, G);
    COSA_REQUIRE(C >= 1 && C <= RMAXC, "cosa_label_reliability: 1 to %d classes (got %d)", RMAXC, C);
    COSA_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && S <= 32768, "cosa_label_reliability: bad shape (B=%d S=%d)", B, S);
    // (a NaN fails every comparison: refused here as well)
    COSA_REQUIRE(beta >= 0.f && beta <= 8.f, "cosa_label_reliability: beta must lie in [0, 8] (got %g)", (double)beta);
    COSA_REQUIRE(floor >= 0.f && floor < 1.f, "cosa_label_reliability: floor must lie in [0, 1) (got %g)", (double)floor);
    RelSets sets = {};
    const long long SS = (long long)S * S;
    bool vec = SS % RPX == 0;
    for (int g = 0; g < G; g++) {
        COSA_REQUIRE(cams[g] && masks[g] && rel[g], "cosa_label_reliability: null CAM set / label map / weight map %d", g);
        sets.cam[g] = cams[g]; sets.mask[g] = masks[g]; sets.rel[g] = rel[g];
        sets.hi[g] = thr_dev ? 0.f : thr_hi[g];
        sets.lo[g] = thr_dev ? 0.f : thr_lo[g];
        vec = vec && aligned16(cams[g]) && aligned16(masks[g]) && aligned16(rel[g]);
    }
    const float one_minus_floor = 1.0f - floor;
    const long long chunks = (SS + 256 * RPX - 1) / (256 * RPX);
    const dim3 grid((unsigned)(chunks < RBLOCKS ? chunks : RBLOCKS), B, G);
    const auto kern = vec ? label_reliability_kernel<true> : label_reliability_kernel<false>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, as_stream(stream), sets, labels, thr_dev, C, SS, beta, floor, one_minus_floor,
                       reinterpret_cast<unsigned long long *>(stats));
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
