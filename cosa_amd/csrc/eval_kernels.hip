// eval_kernels.hip -- evaluation path (SURVEY f-1): label maps at the ground truth's resolution and the confusion matrix.
//
//   evaluation_engine.py:96-126,198-200   F.interpolate(cam / seg, size=labels.shape) -> cam_to_label / seg_validation -> argmax
//   utils/seg_helper.py:515-546           cam_to_label
//   utils/evaluation.py:10-70             _fast_hist / scores / pseudo_scores
//
// HBM-bound byte work.  The reference materialises the resized [1,C,H,W] and [1,C+1,H,W] tensors (and clones of them) and takes
// three argmaxes over them; here one thread per output pixel samples the (S,S) maps (L2-resident: 448^2 x 4 B x (2C+1)) and writes
// three bytes.  Arithmetic spec R (this file is compiled with -ffp-contract=off):
//   scale = (float)in / (float)out;  src = max(fmaf(scale, dst + 0.5f, -0.5f), 0);  i0 = min((int)src, in-1);  l1 = src - i0
//   r0 = fma(p00, lx0, p01*lx1);  r1 = fma(p10, lx0, p11*lx1);  v = fma(r0, ly0, r1*ly1)
// which is how ATen's CPU kernel evaluates F.interpolate(bilinear, align_corners=False) at image sizes: the label maps are
// bit-identical to the reference's on the golden vectors (tests/golden/eval.npz).
#include "kernels.hpp"
#include "spec_math.hpp"
#include "student_label.hpp"      // src_index_r, bilerp, student_label4; wave_reduce.hpp: wave_count, nonfinite_bits, flush_counters

namespace cosa {
namespace {

// cam [B,C,S,S], seg [B,C+1,S,S], cls [B,C] -> three uint8 maps [B,H,W]
__global__ __launch_bounds__(256) void eval_labels_kernel(const float *__restrict__ cam, const float *__restrict__ seg,
                                                         const float *__restrict__ cls, int C, int S, int H, int W, float sy, float sx,
                                                         float bkg_thre, uint8_t *__restrict__ lab_cam, uint8_t *__restrict__ lab_ps,
                                                         uint8_t *__restrict__ lab_vd)
{
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int b = blockIdx.y;
    const int Y = pix / W, X = pix - Y * W;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index_r(Y, S, sy, y0, y1, ly0, ly1);
    src_index_r(X, S, sx, x0, x1, lx0, lx1);
    const size_t ss = (size_t)S * S;
    const float *cl = cls + (size_t)b * C;
    const size_t o = (size_t)b * H * W + pix;
    if (cam) {
        const float *cb = cam + (size_t)b * C * ss;
        float best = 0.0f;
        int bi = 0;
        for (int c = 0; c < C; c++) {
            const float l = cl[c];
            // an absent class contributes l * v = 0 exactly (CAMs are finite): skip its four taps
            const float v = l != 0.0f ? l * bilerp(cb + c * ss, S, y0, y1, x0, x1, ly0, ly1, lx0, lx1) : 0.0f;
            if (c == 0 || v > best) { best = v; bi = c; }
        }
        lab_cam[o] = best <= bkg_thre ? 0 : (uint8_t)(bi + 1);
    }
    if (seg) {
        const float *sb = seg + (size_t)b * (C + 1) * ss;
        float bp = 0.0f, bv = 0.0f;
        int ip = 0, iv = 0;
        for (int c = 0; c <= C; c++) {
            const float v = bilerp(sb + c * ss, S, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
            if (c == 0 || v > bp) { bp = v; ip = c; }
            const float vv = (c == 0 || cl[c - 1] != 0.0f) ? v : -1e5f;
            if (c == 0 || vv > bv) { bv = vv; iv = c; }
        }
        lab_ps[o] = (uint8_t)ip;
        lab_vd[o] = (uint8_t)iv;
    }
}

// cam_to_label on an already sized CAM [B,C,H,W]
__global__ __launch_bounds__(256) void cam_to_label_kernel(const float *__restrict__ cam, const float *__restrict__ cls, int C, int H, int W,
                                                          float bkg_thre, const int32_t *__restrict__ boxes, int ignore_mid, float high_thre,
                                                          float low_thre, long long ignore_index, long long *__restrict__ label,
                                                          float *__restrict__ valid_cam)
{
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int b = blockIdx.y;
    const size_t hw = (size_t)H * W;
    const float *cb = cam + (size_t)b * C * hw;
    float best = 0.0f;
    int bi = 0;
    for (int c = 0; c < C; c++) {
        float v = cb[c * hw + pix];
        if (cls) v = cls[(size_t)b * C + c] * v;
        if (valid_cam) valid_cam[((size_t)b * C + c) * hw + pix] = v;
        if (c == 0 || v > best) { best = v; bi = c; }
    }
    long long l = bi + 1;
    if (best <= bkg_thre) l = 0;
    if (boxes) {
        if (ignore_mid) {
            if (best <= high_thre) l = ignore_index;
            if (best <= low_thre) l = 0;
        }
        const int Y = pix / W, X = pix - Y * W;
        const int32_t *bx = boxes + 4 * b;
        if (!(Y >= bx[0] && Y < bx[1] && X >= bx[2] && X < bx[3])) l = ignore_index;
    }
    label[(size_t)b * hw + pix] = l;
}

// hist[nc*t + p] += 1 over pixels with t < nc.  Workgroup-private LDS counters (nc^2 <= 8192), flushed with one global atomic per
// non-zero bin: the 81 x 81 COCO matrix costs 26 KB of LDS.
constexpr int kHistLds = 8192;
__global__ __launch_bounds__(256) void confusion_kernel(const uint8_t *__restrict__ gt, const uint8_t *__restrict__ pred, size_t n, int nc,
                                                       int pseudo, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned int h[kHistLds];
    const int bins = nc * nc;
    for (int i = threadIdx.x; i < bins; i += 256) h[i] = 0;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256 * 16;
    for (size_t base = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16; base < n; base += stride) {
        if (base + 16 <= n && (((size_t)(gt + base) | (size_t)(pred + base)) & 15) == 0) {
            const uint4 g4 = *reinterpret_cast<const uint4 *>(gt + base), p4 = *reinterpret_cast<const uint4 *>(pred + base);
            const unsigned gw[4] = {g4.x, g4.y, g4.z, g4.w}, pw[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int t = (gw[k >> 2] >> (8 * (k & 3))) & 255, p = (pw[k >> 2] >> (8 * (k & 3))) & 255;
                if (pseudo && p == 255) continue;
                if (t < nc && p < nc) atomicAdd(&h[nc * t + p], 1u);
            }
        } else {
            for (size_t i = base; i < n && i < base + 16; i++) {
                const int t = gt[i], p = pred[i];
                if (pseudo && p == 255) continue;
                if (t < nc && p < nc) atomicAdd(&h[nc * t + p], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256)
        if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// ---- export: every file product of ONE image in one packed record at the image's own H x W -----------------
// A thread owns four consecutive pixels of one row (one dword of each uint8 product); the source rows and their weights are computed
// once per thread, the source columns and weights once per pixel, and reused for every plane of every product.  seg calls the same
// src_index_r / bilerp in the same order as eval_labels_kernel, so it holds that kernel's lab_vd (lab_ps without a label row) bits.
struct ExportArgs {
    const float *cam, *cam_aux, *seg, *cls;
    uint8_t *seg_out, *pseudo[2];           // [H,W]
    float *raw[2];                          // [K_live,H,W]
    int32_t *raw_idx[2];                    // [K_live]
    int C, S, H, W, K_live;
    float sy, sx, hi, lo;
    int ignore;
};

__device__ __forceinline__ void store_u8x4(uint8_t *__restrict__ row, int X, int W, const uint8_t (&v)[4], bool dword_ok)
{
    if (dword_ok && X + 4 <= W) {
        *reinterpret_cast<uint32_t *>(row + X) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
        for (int k = 0; k < 4 && X + k < W; k++) row[X + k] = v[k];
    }
}

__global__ __launch_bounds__(256) void export_maps_kernel(const ExportArgs a)
{
    const int W4 = (a.W + 3) >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.H * W4) return;
    const int Y = t / W4, X = (t - Y * W4) * 4;
    const int S = a.S, C = a.C, W = a.W;
    const size_t ss = (size_t)S * S, hw = (size_t)a.H * W;
    const bool dword_ok = (W & 3) == 0;     // rows start dword-aligned (the products are 16-byte aligned in the record)
    int y0, y1, x0[4], x1[4];
    float ly0, ly1, lx0[4], lx1[4];
    src_index_r(Y, S, a.sy, y0, y1, ly0, ly1);
#pragma unroll
    for (int k = 0; k < 4; k++) src_index_r(X + k < W ? X + k : W - 1, S, a.sx, x0[k], x1[k], lx0[k], lx1[k]);
    if (a.seg_out) {
        float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint8_t iv[4] = {0, 0, 0, 0};
        for (int c = 0; c <= C; c++) {
            const bool present = c == 0 || !a.cls || a.cls[c - 1] != 0.0f;      // seg_validation: an absent class is -1e5, its plane unread
            const float *pl = a.seg + c * ss;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float v = present ? bilerp(pl, S, y0, y1, x0[k], x1[k], ly0, ly1, lx0[k], lx1[k]) : -1e5f;
                if (c == 0 || v > bv[k]) { bv[k] = v; iv[k] = (uint8_t)c; }
            }
        }
        store_u8x4(a.seg_out + (size_t)Y * W, X, W, iv, dword_ok);
    }
    for (int g = 0; g < 2; g++) {
        const float *cams = g ? a.cam_aux : a.cam;
        if (!a.pseudo[g] && !a.raw[g]) continue;
        float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int bi[4] = {-1, -1, -1, -1};
        int live = 0;
        for (int c = 0; c < C; c++) {
            const float l = a.cls[c];
            if (l == 0.0f) continue;         // planes of absent classes are never read
            const float *pl = cams + c * ss;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                v[k] = l * bilerp(pl, S, y0, y1, x0[k], x1[k], ly0, ly1, lx0[k], lx1[k]);      // cam_validation
                if (bi[k] < 0 || v[k] > best[k]) { best[k] = v[k]; bi[k] = c; }
            }
            if (a.raw[g] && live < a.K_live) {
                float *o = a.raw[g] + (size_t)live * hw + (size_t)Y * W + X;
                if (dword_ok) {
                    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    for (int k = 0; k < 4 && X + k < W; k++) o[k] = v[k];
                }
                if (t == 0) a.raw_idx[g][live] = c;
            }
            live++;
        }
        if (a.pseudo[g]) {
            // cam2mask without a refine model, per pixel: the threshold plane is key 0 and wins ties (first maximum), so the "high" map
            // names the class iff its value exceeds hi, likewise "low"; mask = class | ignore where only "low" names one | 0
            uint8_t m[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                m[k] = (bi[k] >= 0 && best[k] > a.hi) ? (uint8_t)(bi[k] + 1) : ((bi[k] >= 0 && best[k] > a.lo) ? (uint8_t)a.ignore : (uint8_t)0);
            store_u8x4(a.pseudo[g] + (size_t)Y * W, X, W, m, dword_ok);
        }
    }
}

// ---- PAR-refined pseudo labels at the image's own H x W (pseudo_par / pseudo_aux_par) ----------------------------
// cam2mask (utils/seg_helper.py:721-797) read literally at h != w, every resize by spec R:
//   v = cls * resize(CAM, (H, W));  [thr | v] -> resize to (h, w) = (H / 2, W / 2)  (downscale 0: h = H, w = W, no resize)
//   -> softmax over threshold plane + present classes (hi and lo thresholds) -> PAR on the (h, w) image -> resize to (H, W)
//   -> first-max argmax -> key -> m = hi; m[hi == 0] = ignore; m[hi + lo == 0] = 0
// Stack layout P[2 * set + {hi, lo}][K1][h * w], K1 = K_live + 1 (plane 0: the threshold), sets = the CAM sets asked for.
struct RefineArgs {
    const float *cams[2];                   // the CAM sets asked for, [C,S,S] each
    const float *cls;                       // [C]
    uint8_t *out[2];                        // [H,W] per set
    float *P;
    int sets, C, S, H, W, h, w, K1;
    float cy, cx;                           // S / H, S / W: CAM -> image
    float dy, dx;                           // H / h, W / w: image -> PAR grid
    float uy, ux;                           // h / H, w / W: PAR grid -> image
    float hi, lo;
    int ignore;
};

__device__ __forceinline__ float blend4(float p00, float p01, float p10, float p11, float ly0, float ly1, float lx0, float lx1)
{
    const float r0 = __builtin_fmaf(p00, lx0, p01 * lx1);
    const float r1 = __builtin_fmaf(p10, lx0, p11 * lx1);
    return __builtin_fmaf(r0, ly0, r1 * ly1);
}

// One thread per PAR-grid pixel and CAM set.  DS = 2 composes the two resamplings: the four image-grid taps of the pixel, each four
// taps of the (S,S) CAM times the label -- the [C+1,H,W] tensors are never written.  The values of the present classes are parked in
// their hi planes (each thread re-reads only what it wrote itself), then both softmaxes are written over them, sums in class order.
template <int DS>
__global__ __launch_bounds__(256) void refine_softmax_kernel(const RefineArgs a)
{
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int hw = a.h * a.w;
    if (pix >= hw) return;
    const int g = blockIdx.y;
    const int y = pix / a.w, x = pix - y * a.w;
    const int S = a.S, nk = a.K1 - 1;
    const size_t ss = (size_t)S * S;
    float *Phi = a.P + (size_t)(2 * g) * a.K1 * hw + pix;
    float *Plo = Phi + (size_t)a.K1 * hw;
    constexpr int NT = DS ? 2 : 1;          // image-grid taps per axis
    int Yi[2] = {y, y}, Xi[2] = {x, x};
    float wy[2] = {1.0f, 0.0f}, wx[2] = {1.0f, 0.0f};
    float thi = a.hi, tlo = a.lo;
    if (DS) {
        src_index_r(y, a.H, a.dy, Yi[0], Yi[1], wy[0], wy[1]);
        src_index_r(x, a.W, a.dx, Xi[0], Xi[1], wx[0], wx[1]);
        thi = blend4(thi, thi, thi, thi, wy[0], wy[1], wx[0], wx[1]);       // the constant plane goes through the same resize
        tlo = blend4(tlo, tlo, tlo, tlo, wy[0], wy[1], wx[0], wx[1]);
    }
    int cy0[2], cy1[2], cx0[2], cx1[2];
    float ly0[2], ly1[2], lx0[2], lx1[2];
#pragma unroll
    for (int i = 0; i < NT; i++) {
        src_index_r(Yi[i], S, a.cy, cy0[i], cy1[i], ly0[i], ly1[i]);
        src_index_r(Xi[i], S, a.cx, cx0[i], cx1[i], lx0[i], lx1[i]);
    }
    float mc = -INFINITY;
    int live = 0;
    for (int c = 0; c < a.C && live < nk; c++) {
        const float l = a.cls[c];
        if (l == 0.0f) continue;
        const float *pl = a.cams[g] + c * ss;
        float v;
        if (DS) {
            float u[2][2];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) u[i][j] = l * bilerp(pl, S, cy0[i], cy1[i], cx0[j], cx1[j], ly0[i], ly1[i], lx0[j], lx1[j]);
            v = blend4(u[0][0], u[0][1], u[1][0], u[1][1], wy[0], wy[1], wx[0], wx[1]);
        } else {
            v = l * bilerp(pl, S, cy0[0], cy1[0], cx0[0], cx1[0], ly0[0], ly1[0], lx0[0], lx1[0]);
        }
        live++;
        Phi[(size_t)live * hw] = v;
        mc = v > mc ? v : mc;
    }
    const float mhi = mc > thi ? mc : thi, mlo = mc > tlo ? mc : tlo;
    const float ehi0 = spec_expf(thi - mhi), elo0 = spec_expf(tlo - mlo);
    float shi = 0.0f + ehi0, slo = 0.0f + elo0;
    for (int k = 1; k <= live; k++) {
        const float v = Phi[(size_t)k * hw];
        shi = shi + spec_expf(v - mhi);
        slo = slo + spec_expf(v - mlo);
    }
    Phi[0] = ehi0 / shi;
    Plo[0] = elo0 / slo;
    for (int k = 1; k <= live; k++) {
        const float v = Phi[(size_t)k * hw];
        Phi[(size_t)k * hw] = spec_expf(v - mhi) / shi;
        Plo[(size_t)k * hw] = spec_expf(v - mlo) / slo;
    }
    for (int k = live + 1; k <= nk; k++) {          // K_live above the label row's count: planes that can never win the argmax
        Phi[(size_t)k * hw] = 0.0f;
        Plo[(size_t)k * hw] = 0.0f;
    }
}

// planes [n,H,W] -> [n,h,w] by spec R (the [0,1] image onto the PAR grid)
__global__ __launch_bounds__(256) void resize_planes_r_kernel(const float *__restrict__ src, float *__restrict__ dst, int planes, int H, int W,
                                                             int h, int w, float sy, float sx)
{
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= h * w) return;
    const int y = pix / w, x = pix - y * w;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index_r(y, H, sy, y0, y1, ly0, ly1);
    src_index_r(x, W, sx, x0, x1, lx0, lx1);
    for (int p = 0; p < planes; p++)
        dst[(size_t)p * h * w + pix] = bilerp(src + (size_t)p * H * W, W, y0, y1, x0, x1, ly0, ly1, lx0, lx1);
}

// Refined stacks -> label bytes.  A thread owns four pixels of a row (one dword of each map), as export_maps_kernel; the key of a plane
// is found by walking the label row in the order the softmax kernel numbered the planes.  P == nullptr: no present class, all zero.
__global__ __launch_bounds__(256) void refine_merge_kernel(const RefineArgs a, const float *__restrict__ P)
{
    const int W4 = (a.W + 3) >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.H * W4) return;
    const int Y = t / W4, X = (t - Y * W4) * 4;
    const int W = a.W, w = a.w, nk = a.K1 - 1;
    const size_t hw = (size_t)a.h * w;
    const bool dword_ok = (W & 3) == 0;
    if (!P) {
        const uint8_t z[4] = {0, 0, 0, 0};
        for (int g = 0; g < a.sets; g++) store_u8x4(a.out[g] + (size_t)Y * W, X, W, z, dword_ok);
        return;
    }
    int y0, y1, x0[4], x1[4];
    float ly0, ly1, lx0[4], lx1[4];
    src_index_r(Y, a.h, a.uy, y0, y1, ly0, ly1);
#pragma unroll
    for (int k = 0; k < 4; k++) src_index_r(X + k < W ? X + k : W - 1, w, a.ux, x0[k], x1[k], lx0[k], lx1[k]);
    for (int g = 0; g < a.sets; g++) {
        int key[2][4];
        for (int half = 0; half < 2; half++) {
            const float *Pb = P + (size_t)(2 * g + half) * a.K1 * hw;
            float best[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                best[k] = bilerp(Pb, w, y0, y1, x0[k], x1[k], ly0, ly1, lx0[k], lx1[k]);
                key[half][k] = 0;
            }
            int live = 0;
            for (int c = 0; c < a.C && live < nk; c++) {
                if (a.cls[c] == 0.0f) continue;
                live++;
                const float *pl = Pb + (size_t)live * hw;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float v = bilerp(pl, w, y0, y1, x0[k], x1[k], ly0, ly1, lx0[k], lx1[k]);
                    if (v > best[k]) { best[k] = v; key[half][k] = c + 1; }          // first maximum wins
                }
            }
        }
        uint8_t m[4];
#pragma unroll
        for (int k = 0; k < 4; k++) m[k] = key[0][k] ? (uint8_t)key[0][k] : (key[1][k] ? (uint8_t)a.ignore : (uint8_t)0);
        store_u8x4(a.out[g] + (size_t)Y * W, X, W, m, dword_ok);
    }
}

// ---- per-step pseudo-label statistics and the teacher finite check -----------------------------------------------
// THE definition of the counter vector (uint64 elements) for the device and the host: off[i] of steps, pix, main[K+1], aux[K+1], agree,
// inter[K], pred[K], bad_cam, bad_cam_aux; -> the number of elements
constexpr int kStatsSlots = 4 * kStatsMaxK + 7;
__host__ __device__ inline int label_stats_offsets(int K, int (&off)[COSA_LABEL_STATS_SLOTS])
{
    off[0] = 0;                  // steps
    off[1] = 1;                  // pix
    off[2] = 2;                  // main[K+1]
    off[3] = off[2] + K + 1;     // aux[K+1]
    off[4] = off[3] + K + 1;     // agree
    off[5] = off[4] + 1;         // inter[K]
    off[6] = off[5] + K;         // pred[K]
    off[7] = off[6] + K;         // bad_cam
    off[8] = off[7] + 1;         // bad_cam_aux
    return off[8] + 1;
}

struct LabelStatsArgs {
    const float *mask_main, *mask_aux, *seg, *cls, *cam, *cam_aux;
    const int32_t *boxes;
    unsigned long long *counters;
    unsigned int *flag;                     // step-local: set when this call meets a non-finite CAM element
    int B, K, S, h, w, vec;                 // vec: every full-resolution row may be read as float4 (S % 4 == 0, 16-byte aligned bases)
    float sy, sx, ignore;
};

// A thread owns four adjacent pixels of a row: the source rows and their weights once per thread, the source columns once per pixel,
// the K low-resolution logit planes (L2-resident) through the same src_index_r / bilerp calls as eval_labels_kernel's lab_vd.  The two
// masks and the CAM planes of the present classes are the only full-resolution streams, read once as float4.  A wavefront's 64 items
// lie in one image (two or more only across an image boundary or at tiny S): the image's label row becomes a wave-uniform bit mask with
// two loads and two ballots, so the class loops branch on scalars and an absent class costs no load at all.  Counts meet in
// workgroup-private LDS counters and leave with one global integer atomic per non-zero slot: the same bits in any order.
__global__ __launch_bounds__(256) void label_stats_kernel(const LabelStatsArgs a)
{
    __shared__ unsigned long long ctr[kStatsSlots];
    int off[COSA_LABEL_STATS_SLOTS];
    const int n = label_stats_offsets(a.K, off);
    for (int i = threadIdx.x; i < n; i += 256) ctr[i] = 0;
    __syncthreads();
    const int S = a.S, K = a.K, S4 = (S + 3) >> 2;
    const unsigned per_img = (unsigned)S * S4, total = per_img * a.B;          // < 2^31 (entry point)
    const size_t ss = (size_t)S * S, hw = (size_t)a.h * a.w;
    const int lane = (int)__lane_id();
    const unsigned wave_off = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    unsigned n_pix = 0, n_agree = 0, n_bad[2] = {0, 0};
    for (unsigned base = blockIdx.x * 256u + wave_off; base < total; base += gridDim.x * 256u) {          // (wave-uniform)
        const unsigned item = base + lane;
        const unsigned last = base + 63 < total - 1 ? base + 63 : total - 1;
        const int b_lo = base / per_img, b_hi = last / per_img;
        bool in[4] = {false, false, false, false};
        float mv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, av[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int iv[4] = {0, 0, 0, 0};
        int b = -1, Y = 0, X = 0;
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
        if (any) {
            const size_t o = ((size_t)b * S + Y) * S + X;
            load_f32x4(a.mask_main + o, X, S, a.vec, mv);
            if (a.mask_aux) load_f32x4(a.mask_aux + o, X, S, a.vec, av);
        }
        for (int bb = b_lo; bb <= b_hi; bb++) {
            unsigned long long present[2];
            present_classes(a.cls, bb, K, lane, present);
            if (!(any && b == bb)) continue;
            student_label4(a.seg + (size_t)bb * K * hw, K, a.h, a.w, a.sy, a.sx, S, Y, X, present, iv);
            for (int g = 0; g < 2; g++) {
                const float *cams = g ? a.cam_aux : a.cam;
                if (!cams) continue;
                const float *cb = cams + (size_t)bb * (K - 1) * ss + (size_t)Y * S + X;
                for (int half = 0; half < 2; half++) {
                    for (unsigned long long m = present[half]; m; m &= m - 1) {          // planes of absent classes are never read
                        const int c = 64 * half + __ffsll(m) - 1;
                        float v[4];
                        load_f32x4(cb + (size_t)c * ss, X, S, a.vec, v);
#pragma unroll
                        for (int k = 0; k < 4; k++) n_bad[g] += (in[k] && nonfinite_bits(v[k])) ? 1u : 0u;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool m_ign = mv[k] == a.ignore, m_cls = mv[k] >= 0.0f && mv[k] < (float)K && mv[k] == (float)(int)mv[k];          // a label is an integer
            const int m = m_ign ? K : (int)mv[k];
            n_pix += in[k] ? 1u : 0u;
            wave_count(ctr + off[2], m, in[k] && (m_ign || m_cls));
            if (a.mask_aux) {
                const bool a_ign = av[k] == a.ignore, a_cls = av[k] >= 0.0f && av[k] < (float)K && av[k] == (float)(int)av[k];
                wave_count(ctr + off[3], a_ign ? K : (int)av[k], in[k] && (a_ign || a_cls));
                n_agree += (in[k] && mv[k] == av[k]) ? 1u : 0u;
            }
            wave_count(ctr + off[6], iv[k], in[k] && m_cls && !m_ign);
            wave_count(ctr + off[5], iv[k], in[k] && m_cls && !m_ign && iv[k] == m);
        }
    }
    if (n_pix) atomicAdd(&ctr[off[1]], (unsigned long long)n_pix);
    if (n_agree) atomicAdd(&ctr[off[4]], (unsigned long long)n_agree);
    if (n_bad[0]) atomicAdd(&ctr[off[7]], (unsigned long long)n_bad[0]);
    if (n_bad[1]) atomicAdd(&ctr[off[8]], (unsigned long long)n_bad[1]);
    __syncthreads();
    flush_counters(ctr, a.counters, n, 256);
    if (threadIdx.x == 0 && (ctr[off[7]] | ctr[off[8]])) atomicOr(a.flag, 1u);
}

// after label_stats_kernel on the same stream: the step count, and the factor the trainer multiplies its loss with
__global__ void label_stats_finish_kernel(unsigned long long *__restrict__ counters, const unsigned int *__restrict__ flag,
                                          float *__restrict__ step_scale)
{
    if (threadIdx.x == 0) {
        counters[0] += 1;
        *step_scale = *flag ? __uint_as_float(0x7fc00000u) : 1.0f;
    }
}

__global__ __launch_bounds__(256) void spec_expf_kernel(const float *__restrict__ x, float *__restrict__ y, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = spec_expf(x[i]);
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_eval_labels(const float *cam, const float *seg, const float *cls_label, int B, int C, int S, int H, int W,
                                float bkg_thre, uint8_t *lab_cam, uint8_t *lab_ps, uint8_t *lab_vd, void *stream)
{
    COSA_REQUIRE(cls_label && (cam || seg) && B > 0 && C > 0 && C < 255 && S > 0 && H > 0 && W > 0, "cosa_eval_labels: bad arguments");
    COSA_REQUIRE((!cam || lab_cam) && (!seg || (lab_ps && lab_vd)), "cosa_eval_labels: missing output map");
    COSA_REQUIRE((size_t)H * W < 0x7fffffffull && B <= 65535, "cosa_eval_labels: map too large");
    const float sy = (float)S / (float)H, sx = (float)S / (float)W;
    hipLaunchKernelGGL(eval_labels_kernel, dim3((H * W + 255) / 256, B), dim3(256), 0, as_stream(stream), cam, seg, cls_label, C, S, H, W,
                       sy, sx, bkg_thre, lab_cam, lab_ps, lab_vd);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_cam_to_label(const float *cam, const float *cls_label, int B, int C, int H, int W, float bkg_thre,
                                 const int32_t *boxes, int ignore_mid, float high_thre, float low_thre, long long ignore_index,
                                 long long *label, float *valid_cam, void *stream)
{
    COSA_REQUIRE(cam && label && B > 0 && C > 0 && H > 0 && W > 0, "cosa_cam_to_label: bad arguments");
    COSA_REQUIRE((size_t)H * W < 0x7fffffffull && B <= 65535, "cosa_cam_to_label: map too large");
    hipLaunchKernelGGL(cam_to_label_kernel, dim3((H * W + 255) / 256, B), dim3(256), 0, as_stream(stream), cam, cls_label, C, H, W, bkg_thre,
                       boxes, ignore_mid, high_thre, low_thre, ignore_index, label, valid_cam);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_confusion_hist(const uint8_t *gt, const uint8_t *pred, size_t n, int num_classes, int pseudo,
                                   unsigned long long *hist, void *stream)
{
    COSA_REQUIRE(gt && pred && hist && num_classes > 0, "cosa_confusion_hist: bad arguments");
    COSA_REQUIRE(num_classes * num_classes <= kHistLds, "cosa_confusion_hist: at most 90 classes (got %d)", num_classes);
    if (n == 0) return COSA_OK;
    size_t blocks = (n + 256 * 16 * 8 - 1) / (256 * 16 * 8);          // >= 8 chunks of 16 bytes per thread: amortises the flush
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), gt, pred, n, num_classes, pseudo, hist);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

// One definition of the record for the device and the host: offsets[i] (bytes, 16-byte aligned) of product i in the order seg, pseudo,
// pseudo_aux, rawcam, rawcam_aux, rawcam_idx, rawcam_aux_idx, pseudo_par, pseudo_aux_par; (size_t)-1 for a product not asked for.  The
// PAR products come last, so a record without them is laid out as before they existed.  Returns the record's size, or 0 on bad arguments.
extern "C" size_t cosa_export_record_layout(int C, int H, int W, int K_live, unsigned what, size_t *offsets)
{
    if (!offsets || C < 1 || C >= 255 || H < 1 || W < 1 || K_live < 0 || K_live > C || (what & ~(unsigned)COSA_EXPORT_EVERY) || !what) {
        set_error("cosa_export_record_layout: bad arguments (C %d, H %d, W %d, K_live %d, what 0x%x)", C, H, W, K_live, what);
        return 0;
    }
    const size_t hw = (size_t)H * W;
    const size_t sizes[COSA_EXPORT_SLOTS] = {hw, hw, hw, hw * K_live * 4, hw * K_live * 4, (size_t)K_live * 4, (size_t)K_live * 4, hw, hw};
    const unsigned bits[COSA_EXPORT_SLOTS] = {COSA_EXPORT_SEG, COSA_EXPORT_PSEUDO, COSA_EXPORT_PSEUDO_AUX, COSA_EXPORT_RAWCAM,
                                              COSA_EXPORT_RAWCAM_AUX, COSA_EXPORT_RAWCAM, COSA_EXPORT_RAWCAM_AUX,
                                              COSA_EXPORT_PSEUDO_PAR, COSA_EXPORT_PSEUDO_AUX_PAR};
    size_t off = 0;
    for (int i = 0; i < COSA_EXPORT_SLOTS; i++) {
        if (what & bits[i]) {
            offsets[i] = off;
            off += (sizes[i] + 15) & ~(size_t)15;
        } else {
            offsets[i] = (size_t)-1;
        }
    }
    return off < 16 ? 16 : off;
}

extern "C" int cosa_export_maps(const float *cam, const float *cam_aux, const float *seg, const float *cls_label, int C, int S, int H, int W,
                                int K_live, unsigned what, float high_thre, float low_thre, int ignore_index, void *record,
                                size_t record_bytes, void *stream)
{
    COSA_REQUIRE(record && what && !(what & ~(unsigned)COSA_EXPORT_ALL), "cosa_export_maps: bad arguments (what 0x%x)", what);
    COSA_REQUIRE(C > 0 && C < 255 && S > 0, "cosa_export_maps: C must be in 1..254 and S >= 1 (got C %d, S %d)", C, S);
    COSA_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W < 0x7fffffffull, "cosa_export_maps: bad size %d x %d", H, W);
    COSA_REQUIRE(ignore_index >= 0 && ignore_index <= 255, "cosa_export_maps: ignore_index %d does not fit a byte", ignore_index);
    const unsigned cam_bits = what & ~(unsigned)COSA_EXPORT_SEG;
    COSA_REQUIRE(!cam_bits || cls_label, "cosa_export_maps: pseudo / rawcam products need the image-level label row");
    COSA_REQUIRE(!(what & COSA_EXPORT_SEG) || seg, "cosa_export_maps: seg asked for without logits");
    COSA_REQUIRE(!(what & (COSA_EXPORT_PSEUDO | COSA_EXPORT_RAWCAM)) || cam, "cosa_export_maps: main-CAM product without the main CAM");
    COSA_REQUIRE(!(what & (COSA_EXPORT_PSEUDO_AUX | COSA_EXPORT_RAWCAM_AUX)) || cam_aux, "cosa_export_maps: auxiliary-CAM product without the auxiliary CAM");
    COSA_REQUIRE(K_live >= 0 && K_live <= C, "cosa_export_maps: K_live %d outside 0..C", K_live);
    COSA_REQUIRE(((size_t)record & 15) == 0, "cosa_export_maps: the record must be 16-byte aligned");
    size_t off[COSA_EXPORT_SLOTS];
    const size_t need = cosa_export_record_layout(C, H, W, K_live, what, off);
    COSA_REQUIRE(need && record_bytes >= need, "cosa_export_maps: record of %zu bytes, %zu needed", record_bytes, need);
    uint8_t *r = (uint8_t *)record;
    auto at = [&](int i) -> uint8_t * { return off[i] == (size_t)-1 ? nullptr : r + off[i]; };
    ExportArgs a;
    a.cam = cam; a.cam_aux = cam_aux; a.seg = seg; a.cls = cls_label;
    a.seg_out = at(0); a.pseudo[0] = at(1); a.pseudo[1] = at(2);
    a.raw[0] = K_live ? (float *)at(3) : nullptr; a.raw[1] = K_live ? (float *)at(4) : nullptr;
    a.raw_idx[0] = (int32_t *)at(5); a.raw_idx[1] = (int32_t *)at(6);
    a.C = C; a.S = S; a.H = H; a.W = W; a.K_live = K_live;
    a.sy = (float)S / (float)H; a.sx = (float)S / (float)W; a.hi = high_thre; a.lo = low_thre; a.ignore = ignore_index;
    const int threads = H * ((W + 3) / 4);
    hipLaunchKernelGGL(export_maps_kernel, dim3((threads + 255) / 256), dim3(256), 0, as_stream(stream), a);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

// ---- PAR-refined pseudo labels ------------------------------------------------------------------------------------------------------
namespace {
inline int refine_sets(unsigned what) { return ((what & COSA_EXPORT_PSEUDO_PAR) ? 1 : 0) + ((what & COSA_EXPORT_PSEUDO_AUX_PAR) ? 1 : 0); }
}

// workspace of cosa_export_refine: P | P2 ([2 * sets][K_live + 1][h * w] each) | image on the PAR grid [3][h * w] | aff [8 n_dil][h * w];
// 0 on bad arguments
extern "C" size_t cosa_export_refine_workspace_bytes(int H, int W, int K_live, unsigned what, int downscale, int n_dil)
{
    const int sets = refine_sets(what);
    if (H < 1 || W < 1 || K_live < 0 || K_live >= 255 || !sets || (downscale != 0 && downscale != 2) || n_dil < 1 || n_dil > kMaxDil) {
        set_error("cosa_export_refine_workspace_bytes: bad arguments (H %d, W %d, K_live %d, what 0x%x, downscale %d, n_dil %d)", H, W, K_live,
                  what, downscale, n_dil);
        return 0;
    }
    const size_t hw = (size_t)(downscale ? H / 2 : H) * (size_t)(downscale ? W / 2 : W);
    const size_t stack = align_up((size_t)2 * sets * (K_live + 1) * hw * sizeof(float), 256);
    return 2 * stack + align_up(3 * hw * sizeof(float), 256) + align_up((size_t)n_dil * 8 * hw * sizeof(float), 256);
}

// image [3,H,W] in [0,1] (cosa_denormalize_img), cam / cam_aux [C,S,S], cls_label [C] with exactly K_live non-zero entries.  `what` is
// the mask the record was laid out with; only the slots of COSA_EXPORT_PSEUDO_PAR / _AUX_PAR are written.
extern "C" int cosa_export_refine(const float *image, const float *cam, const float *cam_aux, const float *cls_label, int C, int S, int H,
                                  int W, int K_live, unsigned what, float high_thre, float low_thre, int ignore_index, int downscale,
                                  const int *dilations, int n_dil, int par_iters, void *record, size_t record_bytes, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    const int sets = refine_sets(what);
    COSA_REQUIRE(record && what && !(what & ~(unsigned)COSA_EXPORT_EVERY) && sets, "cosa_export_refine: bad arguments (what 0x%x names no PAR product)", what);
    COSA_REQUIRE(image && cls_label && workspace, "cosa_export_refine: the image, the image-level label row and a workspace are needed");
    COSA_REQUIRE(C > 0 && C < 255 && S > 0, "cosa_export_refine: C must be in 1..254 and S >= 1 (got C %d, S %d)", C, S);
    COSA_REQUIRE(H >= COSA_EXPORT_REFINE_MIN_SIDE && W >= COSA_EXPORT_REFINE_MIN_SIDE && (size_t)H * W < 0x7fffffffull,
                 "cosa_export_refine: size %d x %d outside the envelope (each side >= %d)", H, W, COSA_EXPORT_REFINE_MIN_SIDE);
    COSA_REQUIRE(ignore_index >= 0 && ignore_index <= 255, "cosa_export_refine: ignore_index %d does not fit a byte", ignore_index);
    COSA_REQUIRE(downscale == 0 || downscale == 2, "cosa_export_refine: downscale must be 0 or 2 (got %d)", downscale);
    COSA_REQUIRE(dilations && n_dil >= 1 && n_dil <= kMaxDil, "cosa_export_refine: PAR takes 1..%d dilations (got %d)", kMaxDil, n_dil);
    COSA_REQUIRE(par_iters >= 0, "cosa_export_refine: par_iters < 0");
    COSA_REQUIRE(!(what & COSA_EXPORT_PSEUDO_PAR) || cam, "cosa_export_refine: main-CAM product without the main CAM");
    COSA_REQUIRE(!(what & COSA_EXPORT_PSEUDO_AUX_PAR) || cam_aux, "cosa_export_refine: auxiliary-CAM product without the auxiliary CAM");
    COSA_REQUIRE(K_live >= 0 && K_live <= C, "cosa_export_refine: K_live %d outside 0..C", K_live);
    COSA_REQUIRE(((size_t)record & 15) == 0, "cosa_export_refine: the record must be 16-byte aligned");
    size_t off[COSA_EXPORT_SLOTS];
    const size_t need = cosa_export_record_layout(C, H, W, K_live, what, off);
    COSA_REQUIRE(need && record_bytes >= need, "cosa_export_refine: record of %zu bytes, %zu needed", record_bytes, need);
    const size_t ws_need = cosa_export_refine_workspace_bytes(H, W, K_live, what, downscale, n_dil);
    if (!ws_need || workspace_bytes < ws_need) {
        set_error("cosa_export_refine: workspace of %zu bytes, %zu needed", workspace_bytes, ws_need);
        return COSA_ENOMEM;
    }
    ParPlan plan;
    int rc = par_make_plan(dilations, n_dil, &plan);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    RefineArgs a;
    a.sets = 0;
    a.cams[1] = nullptr; a.out[1] = nullptr;
    if (what & COSA_EXPORT_PSEUDO_PAR) { a.cams[a.sets] = cam; a.out[a.sets] = (uint8_t *)record + off[7]; a.sets++; }
    if (what & COSA_EXPORT_PSEUDO_AUX_PAR) { a.cams[a.sets] = cam_aux; a.out[a.sets] = (uint8_t *)record + off[8]; a.sets++; }
    a.cls = cls_label;
    a.C = C; a.S = S; a.H = H; a.W = W; a.K1 = K_live + 1;
    a.h = downscale ? H / 2 : H; a.w = downscale ? W / 2 : W;
    a.cy = (float)S / (float)H; a.cx = (float)S / (float)W;
    a.dy = (float)H / (float)a.h; a.dx = (float)W / (float)a.w;
    a.uy = (float)a.h / (float)H; a.ux = (float)a.w / (float)W;
    a.hi = high_thre; a.lo = low_thre; a.ignore = ignore_index;
    const size_t hw = (size_t)a.h * a.w;
    const int planes = 2 * a.sets * a.K1;
    const dim3 gm((unsigned)((H * ((W + 3) / 4) + 255) / 256));
    if (K_live == 0) {                       // no present class: cam2mask's softmax over the threshold plane alone names key 0 everywhere
        a.P = nullptr;
        hipLaunchKernelGGL(refine_merge_kernel, gm, dim3(256), 0, st, a, static_cast<const float *>(nullptr));
        COSA_LAUNCH_CHECK();
        return COSA_OK;
    }
    Carver cv(workspace);
    float *P = cv.take<float>((size_t)planes * hw);
    float *P2 = cv.take<float>((size_t)planes * hw);
    float *img_lo = cv.take<float>(3 * hw);
    float *aff = cv.take<float>((size_t)n_dil * 8 * hw);
    a.P = P;
    const dim3 gl((unsigned)((hw + 255) / 256), a.sets);
    if (downscale)
        hipLaunchKernelGGL(refine_softmax_kernel<2>, gl, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(refine_softmax_kernel<0>, gl, dim3(256), 0, st, a);
    COSA_LAUNCH_CHECK();
    const float *Pfinal = P;
    if (par_iters > 0) {
        const float *im = image;
        if (downscale) {
            hipLaunchKernelGGL(resize_planes_r_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, st, image, img_lo, 3, H, W, a.h, a.w,
                               a.dy, a.dx);
            COSA_LAUNCH_CHECK();
            im = img_lo;
        }
        rc = par_launch_affinity(im, aff, 1, a.h, a.w, plan, st);          // once for the hi and lo stacks of every set
        if (rc) return rc;
        float *src = P, *dst = P2;
        for (int it = 0; it < par_iters; it++) {
            rc = par_launch_step(aff, src, dst, 1, planes, nullptr, 1, (size_t)planes * hw, a.h, a.w, plan, st);      // every plane is live
            if (rc) return rc;
            float *t = src; src = dst; dst = t;
        }
        Pfinal = src;
    }
    hipLaunchKernelGGL(refine_merge_kernel, gm, dim3(256), 0, st, a, Pfinal);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

// ---- per-step pseudo-label statistics ----------------------------------------------------------------------------
extern "C" size_t cosa_label_stats_layout(int K, size_t *offsets)
{
    if (!offsets || K < 2 || K > kStatsMaxK) {
        set_error("cosa_label_stats_layout: K must be in 2..%d (got %d) and offsets non-null", kStatsMaxK, K);
        return 0;
    }
    int off[COSA_LABEL_STATS_SLOTS];
    const int n = label_stats_offsets(K, off);
    for (int i = 0; i < COSA_LABEL_STATS_SLOTS; i++) offsets[i] = (size_t)off[i];
    return (size_t)n;
}

extern "C" int cosa_label_stats(const float *mask_main, const float *mask_aux, const float *seg_logits, const float *cls_label,
                                const int32_t *boxes, const float *cam, const float *cam_aux, int B, int K, int S, int h, int w,
                                int ignore_index, unsigned long long *counters, float *step_scale, void *workspace, void *stream)
{
    COSA_REQUIRE(mask_main && seg_logits && cls_label && boxes && counters && step_scale && workspace,
                 "cosa_label_stats: null argument (only mask_aux, cam and cam_aux may be NULL)");
    COSA_REQUIRE(K >= 2 && K <= kStatsMaxK, "cosa_label_stats: K must be in 2..%d (got %d)", kStatsMaxK, K);
    COSA_REQUIRE(B > 0 && S > 0 && h > 0 && w > 0 && h <= S && w <= S,
                 "cosa_label_stats: sizes outside the envelope (B %d, S %d, h %d, w %d: all > 0, h and w <= S)", B, S, h, w);
    COSA_REQUIRE(ignore_index < 0 || ignore_index >= K, "cosa_label_stats: ignore_index %d is a class index (K %d)", ignore_index, K);
    COSA_REQUIRE((size_t)B * S * ((S + 3) / 4) < 0x7fffffffull, "cosa_label_stats: maps too large (B %d, S %d)", B, S);
    COSA_REQUIRE((((size_t)counters | (size_t)workspace) & 7) == 0, "cosa_label_stats: counters and workspace must be 8-byte aligned");
    LabelStatsArgs a;
    a.mask_main = mask_main; a.mask_aux = mask_aux; a.seg = seg_logits; a.cls = cls_label; a.cam = cam; a.cam_aux = cam_aux;
    a.boxes = boxes; a.counters = counters; a.flag = (unsigned int *)workspace;
    a.B = B; a.K = K; a.S = S; a.h = h; a.w = w;
    a.sy = (float)h / (float)S; a.sx = (float)w / (float)S; a.ignore = (float)ignore_index;
    a.vec = (S & 3) == 0 && ((((size_t)mask_main | (size_t)mask_aux | (size_t)cam | (size_t)cam_aux) & 15) == 0);
    hipStream_t st = as_stream(stream);
    COSA_HIP_CHECK(hipMemsetAsync(workspace, 0, COSA_LABEL_STATS_WORKSPACE_BYTES, st));
    // at most kStatsMaxGroups workgroups (four per CU: one resident round, and few workgroups meeting at the global counters), the rest
    // by grid stride with every workgroup making the same number of rounds
    const unsigned groups = ((unsigned)B * S * ((S + 3) / 4) + 255u) / 256u;
    const unsigned rounds = (groups + kStatsMaxGroups - 1) / kStatsMaxGroups;
    const unsigned grid = (groups + rounds - 1) / rounds;
    hipLaunchKernelGGL(label_stats_kernel, dim3(grid), dim3(256), 0, st, a);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(label_stats_finish_kernel, dim3(1), dim3(64), 0, st, counters, (const unsigned int *)workspace, step_scale);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

// spec E as this translation unit computes it (test hook: y[i] = expf(x[i]))
extern "C" int cosa_spec_expf(const float *x, float *y, long long n, void *stream)
{
    COSA_REQUIRE(x && y && n > 0 && n < (1ll << 31), "cosa_spec_expf: bad arguments");
    hipLaunchKernelGGL(spec_expf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, y, n);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
