// student_label.hpp -- what the per-step monitors of the label maps share (eval_kernels.hip: cosa_label_stats; gt_stats_kernels.hip:
// cosa_gt_stats) and --teacher_check's label pass (teacher_check_kernels.hip): spec R's source index and bilinear sample, the student's label
// of four adjacent pixels, the four-pixel load and a label's histogram slot; the wave-aggregated count comes with wave_reduce.hpp.
// Include from a translation unit compiled with -ffp-contract=off (build.py: EXACT): what is an fma here is written as one.
#pragma once
#include "kernels.hpp"
#include "wave_reduce.hpp"

namespace cosa {
namespace {

// spec R: scale = (float)in / (float)out;  src = max(fmaf(scale, dst + 0.5f, -0.5f), 0);  i0 = min((int)src, in-1)
__device__ __forceinline__ void src_index_r(int dst, int in, float scale, int &i0, int &i1, float &l0, float &l1)
{
    float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    src = src < 0.0f ? 0.0f : src;
    int i = (int)src;
    i = i > in - 1 ? in - 1 : i;
    float lam = src - (float)i;
    lam = lam < 0.0f ? 0.0f : (lam > 1.0f ? 1.0f : lam);
    i0 = i;
    i1 = i < in - 1 ? i + 1 : i;
    l1 = lam;
    l0 = 1.0f - lam;
}

__device__ __forceinline__ float bilerp(const float *__restrict__ pl, int w, int y0, int y1, int x0, int x1, float ly0, float ly1,
                                        float lx0, float lx1)
{
    const float r0 = __builtin_fmaf(pl[(size_t)y0 * w + x0], lx0, pl[(size_t)y0 * w + x1] * lx1);
    const float r1 = __builtin_fmaf(pl[(size_t)y1 * w + x0], lx0, pl[(size_t)y1 * w + x1] * lx1);
    return __builtin_fmaf(r0, ly0, r1 * ly1);
}

// image b's label row cls[b][K-1] as a wave-uniform bit mask, with two loads and two ballots: present[0] bit i: class i + 1 is in the row
// (i < 64); present[1]: classes 65..128.  Every lane of the wavefront must make the call.
__device__ __forceinline__ void present_classes(const float *__restrict__ cls, int b, int K, int lane, unsigned long long (&present)[2])
{
    const float *cl = cls + (size_t)b * (K - 1);
    present[0] = __ballot(lane < K - 1 && cl[lane < K - 1 ? lane : 0] != 0.0f);
    present[1] = __ballot(lane + 64 < K - 1 && cl[lane + 64 < K - 1 ? lane + 64 : 0] != 0.0f);
}

// THE student label of the monitors, for the four pixels X..X+3 of row Y of an (S,S) map: the K low-resolution logit planes sb[K][h][w]
// (L2-resident) resized by spec R through the same src_index_r / bilerp calls as eval_labels_kernel's lab_vd, a class absent from the label
// row at -1e5 with its plane unread (seg_validation; background always live; a scalar branch: `present` is wave-uniform), first maximum in
// class order.  A pixel past the row's end takes the last column's label.
__device__ __forceinline__ void student_label4(const float *__restrict__ sb, int K, int h, int w, float sy, float sx, int S, int Y, int X,
                                               const unsigned long long (&present)[2], int (&iv)[4])
{
    const size_t hw = (size_t)h * w;
    int y0, y1, x0[4], x1[4];
    float ly0, ly1, lx0[4], lx1[4];
    src_index_r(Y, h, sy, y0, y1, ly0, ly1);
#pragma unroll
    for (int k = 0; k < 4; k++) src_index_r(X + k < S ? X + k : S - 1, w, sx, x0[k], x1[k], lx0[k], lx1[k]);
    float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < K; c++) {
        const bool live = c == 0 || ((present[(c - 1) >> 6] >> ((c - 1) & 63)) & 1ull);
        const float *pl = sb + (size_t)c * hw;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float v = live ? bilerp(pl, w, y0, y1, x0[k], x1[k], ly0, ly1, lx0[k], lx1[k]) : -1e5f;
            if (c == 0 || v > bv[k]) { bv[k] = v; iv[k] = c; }
        }
    }
}

__device__ __forceinline__ void load_f32x4(const float *__restrict__ p, int X, int S, int vec, float (&v)[4])
{
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = X + k < S ? p[k] : 0.0f;
    }
}

// a label map's value as a slot of a [K+1] histogram: 0..K-1 for a class (a label is an integer), K for ignore, -1 for anything else
__device__ __forceinline__ int label_slot(float v, int K, float ignore)
{
    if (v == ignore) return K;
    return (v >= 0.0f && v < (float)K && v == (float)(int)v) ? (int)v : -1;
}

}  // namespace
}  // namespace cosa
