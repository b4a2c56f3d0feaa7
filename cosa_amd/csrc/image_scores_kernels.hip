// image_scores_kernels.hip -- per-image evaluation counters: ONE image's ground truth against up to eight label maps
// of it in one launch, into one row of uint64 words
//   row = [ n, n_valid, then for map m, class c: I, P, G, A ]
// (what the reference's assist_seg, evaluation_engine.py:311-329, needs of a prediction, and what the confusion matrix of the same maps
// sums to: diagonal I, column sums P, row sums G).  Byte work: a thread owns 16 consecutive pixels, reads gt once (one dwordx4) and each
// map once, and counts into workgroup-private 32-bit LDS counters; label maps are made of runs, so a thread adds a run of equal slots
// with one LDS atomic.  Per map and class the LDS holds four DISJOINT counts
//   I  = counted, gt == c and pred == c        Gx = counted, gt == c and pred != c
//   Px = counted, pred == c and gt != c        X  = pred == c, gt not a class (ignored truth)
// so a correctly labelled pixel costs one update; P = I + Px, G = I + Gx and A = I + Px + X are formed at the flush, which sends the
// non-zero words out with 64-bit integer atomics: the same bytes on every run and for every grid.  No float, no workspace, no host sync.
#include "common.hpp"
#include "wave_reduce.hpp"

namespace cosa {
namespace {

constexpr int kScoreLds = COSA_IMAGE_SCORES_MAX_MAPS * 255 * 4;          // 8160 words, 32640 bytes

struct ImageScoresArgs {
    const uint8_t *gt;
    const uint8_t *pred[COSA_IMAGE_SCORES_MAX_MAPS];
    unsigned long long *row;
    size_t n, chunks;                       // chunks: 16-byte items of the body [head, head + 16 chunks)
    int head;                               // pixels in front of the body: gt + head is 16-byte aligned (or head == n)
    int n_maps, nc;
    unsigned aligned;                       // bit m: pred[m] + head is 16-byte aligned too
};

// a run of equal LDS slots, added with one atomic when it ends; slot < 0: nothing to count
struct Run {
    int slot = -1;
    unsigned cnt = 0;
    __device__ __forceinline__ void push(unsigned *ctr, int s)
    {
        if (s == slot) { cnt++; return; }
        if (slot >= 0) atomicAdd(&ctr[slot], cnt);
        slot = s;
        cnt = 1;
    }
    __device__ __forceinline__ void end(unsigned *ctr)
    {
        if (slot >= 0) atomicAdd(&ctr[slot], cnt);
    }
};

// The counting rule of confusion_kernel (eval_kernels.hip) for one pixel of one map: counted iff t < nc and p < nc -- a prediction that
// is no class, 255 included, drops the pixel from I / P / G whatever the map's pseudo flag says.  base = 4 nc m.
__device__ __forceinline__ void score_pixel(unsigned *ctr, int base, int nc, int t, int p, Run &a, Run &b)
{
    int s1 = -1, s2 = -1;
    if (p < nc) {
        if (t >= nc) {
            s1 = base + 4 * p + 3;                      // X
        } else if (t == p) {
            s1 = base + 4 * t;                          // I
        } else {
            s1 = base + 4 * t + 2;                      // Gx
            s2 = base + 4 * p + 1;                      // Px
        }
    }
    a.push(ctr, s1);
    b.push(ctr, s2);
}

__global__ __launch_bounds__(256) void image_scores_kernel(const ImageScoresArgs a)
{
    __shared__ unsigned int ctr[kScoreLds];
    __shared__ unsigned int valid_lds;
    const int nc = a.nc, cells = a.n_maps * nc;
    for (int i = threadIdx.x; i < 4 * cells; i += 256) ctr[i] = 0;
    if (threadIdx.x == 0) valid_lds = 0;
    __syncthreads();
    unsigned n_valid = 0;
    for (size_t ch = (size_t)blockIdx.x * 256 + threadIdx.x; ch < a.chunks; ch += (size_t)gridDim.x * 256) {
        const size_t o = (size_t)a.head + ch * 16;
        const uint4 g4 = *reinterpret_cast<const uint4 *>(a.gt + o);
        const unsigned gw[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int k = 0; k < 16; k++) n_valid += (int)((gw[k >> 2] >> (8 * (k & 3))) & 255) < nc ? 1u : 0u;
        for (int m = 0; m < a.n_maps; m++) {
            uint4 p4;
            if ((a.aligned >> m) & 1)
                p4 = *reinterpret_cast<const uint4 *>(a.pred[m] + o);
            else
                __builtin_memcpy(&p4, a.pred[m] + o, 16);          // a view at any byte offset: a load the target takes unaligned
            const unsigned pw[4] = {p4.x, p4.y, p4.z, p4.w};
            Run r1, r2;
#pragma unroll
            for (int k = 0; k < 16; k++)
                score_pixel(ctr, 4 * nc * m, nc, (gw[k >> 2] >> (8 * (k & 3))) & 255, (pw[k >> 2] >> (8 * (k & 3))) & 255, r1, r2);
            r1.end(ctr);
            r2.end(ctr);
        }
    }
    // the scalar head and tail, fewer than 32 pixels: one pixel per thread of workgroup 0
    const size_t body_end = (size_t)a.head + a.chunks * 16;
    const size_t loose = (size_t)a.head + (a.n - body_end);
    if (blockIdx.x == 0 && threadIdx.x < loose) {
        const size_t i = (int)threadIdx.x < a.head ? threadIdx.x : body_end + (threadIdx.x - a.head);
        const int t = a.gt[i];
        n_valid += t < nc ? 1u : 0u;
        for (int m = 0; m < a.n_maps; m++) {
            Run r1, r2;
            score_pixel(ctr, 4 * nc * m, nc, t, a.pred[m][i], r1, r2);
            r1.end(ctr);
            r2.end(ctr);
        }
    }
    n_valid = wave_sum32(n_valid);
    if (__lane_id() == 0 && n_valid) atomicAdd(&valid_lds, n_valid);
    __syncthreads();
    unsigned long long *out = a.row + 2;
    for (int i = threadIdx.x; i < cells; i += 256) {
        const unsigned long long I = ctr[4 * i], Px = ctr[4 * i + 1], Gx = ctr[4 * i + 2], X = ctr[4 * i + 3];
        if (I) atomicAdd(&out[4 * i], I);
        if (I + Px) atomicAdd(&out[4 * i + 1], I + Px);
        if (I + Gx) atomicAdd(&out[4 * i + 2], I + Gx);
        if (I + Px + X) atomicAdd(&out[4 * i + 3], I + Px + X);
    }
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) atomicAdd(&a.row[0], (unsigned long long)a.n);
        if (valid_lds) atomicAdd(&a.row[1], (unsigned long long)valid_lds);
    }
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" size_t cosa_image_scores_words(int num_classes, int n_maps)
{
    if (num_classes < 1 || num_classes > 255 || n_maps < 1 || n_maps > COSA_IMAGE_SCORES_MAX_MAPS) {
        set_error("cosa_image_scores_words: num_classes must be in 1..255 and n_maps in 1..%d (got %d, %d)", COSA_IMAGE_SCORES_MAX_MAPS,
                  num_classes, n_maps);
        return 0;
    }
    return 2 + (size_t)n_maps * num_classes * 4;
}

extern "C" int cosa_image_scores(const uint8_t *gt, const uint8_t *const *preds, const int *pseudo, int n_maps, size_t n, int num_classes,
                                 unsigned long long *row, void *stream)
{
    COSA_REQUIRE(gt && preds && pseudo && row, "cosa_image_scores: null argument");
    COSA_REQUIRE(num_classes >= 1 && num_classes <= 255, "cosa_image_scores: num_classes must be in 1..255 (got %d)", num_classes);
    COSA_REQUIRE(n_maps >= 1 && n_maps <= COSA_IMAGE_SCORES_MAX_MAPS, "cosa_image_scores: n_maps must be in 1..%d (got %d)",
                 COSA_IMAGE_SCORES_MAX_MAPS, n_maps);
    COSA_REQUIRE(n >= 1 && n <= 0xffffffffull, "cosa_image_scores: n must be in 1..2^32-1 (got %zu)", n);
    COSA_REQUIRE(((size_t)row & 7) == 0, "cosa_image_scores: the row must be 8-byte aligned");
    ImageScoresArgs a;
    a.gt = gt; a.row = row; a.n = n; a.n_maps = n_maps; a.nc = num_classes;
    const size_t head = (size_t)(-(intptr_t)gt) & 15;
    a.head = (int)(head < n ? head : n);
    a.chunks = (n - a.head) / 16;
    a.aligned = 0;
    for (int m = 0; m < COSA_IMAGE_SCORES_MAX_MAPS; m++) {
        a.pred[m] = m < n_maps ? preds[m] : nullptr;
        COSA_REQUIRE(m >= n_maps || preds[m], "cosa_image_scores: map %d is null", m);
        if (m < n_maps && (((size_t)preds[m] + a.head) & 15) == 0) a.aligned |= 1u << m;
    }
    size_t blocks = (a.chunks + 255) / 256;          // one 16-pixel item per thread, by grid stride past 1024 workgroups
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(image_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
