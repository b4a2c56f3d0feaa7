// loss_kernels.hip -- the student's dense losses without full-resolution intermediates (gfx950).
//
// Reference chain (main.py:167-212, utils/seg_helper.py:800-813, 210-230, 199-208):
//   seg_pred [b,K,h,w] --bilinear--> [b,K,S,S] --+-- seg_loss(mask_main), seg_loss(mask_aux)   (class-balanced CE, ignore 255)
//                                               +-- softmax -> DenseEnergyLoss: x0.5 (2x2 mean), ROI, nearest image/label
// The reference materialises the [b,K,S,S] logits, their log-softmax, softmax and all the gradients of those (>= 10 passes
// over 270 MB at b=16, K=21, S=448).  Here one forward kernel reads the low-res logits (LDS tile), the two label maps and
// the image, and emits only the 8 CE sums/counts and the S/2 energy inputs; one backward kernel recomputes the per-pixel
// softmax and scatters d loss / d logits straight into the [b,K,h,w] gradient (LDS-privatised float atomics).
//
// Thread = one 2x2 full-res quad (= one pixel of the energy grid); block = 16x16 quads = 32x32 pixels.
// (At the end: the weight gradient of the student's patch projection at K % 64, for the 8-pixel-patch encoder.)
#include "kernels.hpp"

namespace cosa {
namespace {

constexpr int TC = 6;     // low-res cells per block edge held in LDS (32 px / (S/h >= 8) + 2)

__device__ __forceinline__ void src_index(int dst, int in, float scale, int &i0, int &i1, float &l0, float &l1)
{
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.0f) src = 0.0f;
    int i = (int)src;
    if (i > in - 1) i = in - 1;
    i0 = i;
    i1 = i < in - 1 ? i + 1 : i;
    l1 = src - (float)i;
    l0 = 1.0f - l1;
}

struct Tap { int o00, o01, o10, o11; float w00, w01, w10, w11; };   // offsets inside the LDS tile plane + bilinear weights

__device__ __forceinline__ float tap(const float *pl, const Tap &t)
{
    return (pl[t.o00] * t.w00 + pl[t.o01] * t.w01) + (pl[t.o10] * t.w10 + pl[t.o11] * t.w11);
}

// common prologue: stage the low-res logits of this block into LDS, build the 4 pixel taps of this thread's quad
struct QuadCtx {
    Tap t[4];
    int Y, X;          // top-left full-res pixel
    bool valid;
    int cy0, cx0;      // first low-res cell row/col of the tile
};

__device__ __forceinline__ QuadCtx setup(const float *__restrict__ seg_lr, float *tile, int K, int hs, int ws, int S, float sy, float sx,
                                         int b)
{
    QuadCtx c;
    const int by = blockIdx.y * 32, bx = blockIdx.x * 32;
    int a0, a1, d0, d1;
    float u0, u1;
    src_index(by, hs, sy, a0, a1, u0, u1);
    c.cy0 = a0;
    src_index(bx, ws, sx, d0, d1, u0, u1);
    c.cx0 = d0;
    const int tid = threadIdx.y * 16 + threadIdx.x;
    for (int e = tid; e < K * TC * TC; e += 256) {
        const int k = e / (TC * TC), r = e - k * TC * TC;
        const int cy = min(c.cy0 + r / TC, hs - 1), cx = min(c.cx0 + r % TC, ws - 1);
        tile[e] = seg_lr[(((size_t)b * K + k) * hs + cy) * ws + cx];
    }
    __syncthreads();
    c.Y = by + 2 * threadIdx.y;
    c.X = bx + 2 * threadIdx.x;
    c.valid = c.Y < S && c.X < S;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        src_index(min(c.Y + (p >> 1), S - 1), hs, sy, y0, y1, ly0, ly1);
        src_index(min(c.X + (p & 1), S - 1), ws, sx, x0, x1, lx0, lx1);
        y0 -= c.cy0; y1 -= c.cy0; x0 -= c.cx0; x1 -= c.cx0;
        c.t[p].o00 = y0 * TC + x0; c.t[p].o01 = y0 * TC + x1; c.t[p].o10 = y1 * TC + x0; c.t[p].o11 = y1 * TC + x1;
        c.t[p].w00 = ly0 * lx0; c.t[p].w01 = ly0 * lx1; c.t[p].w10 = ly1 * lx0; c.t[p].w11 = ly1 * lx1;
    }
    return c;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sums that meet from many threads / workgroups are kept in 64-bit FIXED POINT and added with integer atomics: integer addition is
// associative, so the result does not depend on the order in which the adds land -- the loss and its gradient are the same bits every
// run (round 2 used float atomics in LDS and in global memory here: the last source of run-to-run differences in the student's
// gradients, together with the weight-gradient GEMM's).  Forward sums (up to ~1e7): 32 fractional bits; gradient cells: 48 fractional bits,
// i.e. finer than fp32's own resolution for every value above 2^-24 (a cell of the benchmark's step is 1e-6 ... 1e-2).
// A value the fixed-point form cannot carry -- NaN, an infinity (a diverged loss), or a magnitude beyond the range that keeps the 64-bit sum from
// wrapping -- contributes nothing and sets a sticky flag word instead; the kernels that convert the sums back to fp32 then write NaN, as the
// float atomics of round 2 would have.  Ranges: forward sums |v| < 2^31.  Gradient cells: a cell of the low-resolution logits receives at most
// (2 S / h)^2 = 1024 adds at the configured 16x up-sampling (one per full-resolution pixel whose bilinear taps touch it; fewer when a wave or a
// quad pre-sums its pixels).  One add: a pixel of label map M in class group c (background / foreground) carries w_Mc g / count_Mc on
// |p_k - [k == label]| <= 1 and bilinear weights <= 1; an add pre-sums any subset of the pixels, at most count_Mc of each group, so it is at most
// W g with W = wA_bg + wA_fg + wB_bg + wB_fg (the sum, not the larger of each pair: for a class k that is nobody's label every term is +p_k; the
// regulariser's share, weight 1e-7, is out of sight).  The trainer's table has W = (1-b)(1-a) + (1-b)a + b(1-a) + ba = 1 for every fg_alpha a and
// aux blend b -- the defaults' 4 x 0.25 included --, so |v| < 16 carries every add for every loss weight g < 16; the entry point admits
// weights in [0, 1] each, W <= 4, so g < 4 there.  The cell total is bounded by the same W g (all pixels once), far inside the 15 integer bits that
// 1024 adds below 16 could fill (48 + 15 bits + sign).  A larger g may trip the check: the sticky flag then gives NaN, never a wrapped sum.
// (Round 4 bounded |v| < 1 at 52 fractional bits, which a weight g >= 2 with few foreground pixels could trip: ADVICE r4.  This comment used
// to give 0.5 g per add and g < 32 for the defaults; summed over all four groups it is g, hence g < 16.)
__device__ __forceinline__ unsigned long long fix32(float v, unsigned long long *flag)
{
    if (!(__builtin_fabsf(v) < 2147483648.0f)) { atomicOr(flag, 1ull); return 0ull; }
    return (unsigned long long)(long long)__builtin_rint((double)v * 4294967296.0);
}
constexpr double kFixGrad = 281474976710656.0;          // 2^48
__device__ __forceinline__ unsigned long long fix52(float v, unsigned long long *flag)      // (the name is round 3's: 48 fractional bits since round 5)
{
    if (!(__builtin_fabsf(v) < 16.0f)) { atomicOr(flag, 1ull); return 0ull; }
    return (unsigned long long)(long long)__builtin_rint((double)v * kFixGrad);
}

// ---- forward ---------------------------------------------------------------------------------------------------
// sums[8] = {bgA_sum, bgA_cnt, fgA_sum, fgA_cnt, bgB_sum, bgB_cnt, fgB_sum, fgB_cnt}
// HAS_B = false: no second label map -- nothing of it is loaded and sums[4..7] stay zero (--aux_cam2seg false)
template <bool HAS_B>
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const float *__restrict__ seg_lr, const float *__restrict__ maskA,
                                                          const float *__restrict__ maskB, const float *__restrict__ simg,
                                                          const int32_t *__restrict__ boxes, unsigned long long *__restrict__ sums,
                                                          unsigned long long *__restrict__ flag, float *__restrict__ s_seg, float *__restrict__ s_img,
                                                          float *__restrict__ roi, unsigned char *__restrict__ unlabel,
                                                          int K, int hs, int ws, int S, float sy, float sx)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];
    __shared__ float red[4][8];
    const int b = blockIdx.z;
    const QuadCtx c = setup(seg_lr, tile, K, hs, ws, S, sy, sx, b);
    const int Sq = S >> 1;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float m[4], inv[4];
    if (c.valid) {
        const size_t SS = (size_t)S * S;
        // pass 1+2: per-pixel max and sum-exp; CE terms
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float mx = -INFINITY;
            for (int k = 0; k < K; k++) mx = fmaxf(mx, tap(tile + k * TC * TC, c.t[p]));
            float se = 0.f;
            for (int k = 0; k < K; k++) se += __expf(tap(tile + k * TC * TC, c.t[p]) - mx);
            m[p] = mx;
            inv[p] = 1.0f / se;
            const float lse = mx + __logf(se);
            const size_t pix = (size_t)(c.Y + (p >> 1)) * S + c.X + (p & 1);
            const int la = (int)maskA[(size_t)b * SS + pix], lb = HAS_B ? (int)maskB[(size_t)b * SS + pix] : 255;
            if (la == 0) { acc[0] += lse - tap(tile, c.t[p]); acc[1] += 1.f; }
            else if (la != 255) { acc[2] += lse - tap(tile + la * TC * TC, c.t[p]); acc[3] += 1.f; }
            if (HAS_B) {
                if (lb == 0) { acc[4] += lse - tap(tile, c.t[p]); acc[5] += 1.f; }
                else if (lb != 255) { acc[6] += lse - tap(tile + lb * TC * TC, c.t[p]); acc[7] += 1.f; }
            }
        }
        // pass 3: probabilities, 2x2 mean (the exact x0.5 bilinear), energy-grid outputs
        const int qy = c.Y >> 1, qx = c.X >> 1;
        const size_t q = (size_t)qy * Sq + qx, QQ = (size_t)Sq * Sq;
        for (int k = 0; k < K; k++) {
            const float *pl = tile + k * TC * TC;
            const float p0 = __expf(tap(pl, c.t[0]) - m[0]) * inv[0], p1 = __expf(tap(pl, c.t[1]) - m[1]) * inv[1];
            const float p2 = __expf(tap(pl, c.t[2]) - m[2]) * inv[2], p3 = __expf(tap(pl, c.t[3]) - m[3]) * inv[3];
            s_seg[((size_t)b * K + k) * QQ + q] = (p0 * 0.5f + p1 * 0.5f) * 0.5f + (p2 * 0.5f + p3 * 0.5f) * 0.5f;
        }
        const size_t pix0 = (size_t)c.Y * S + c.X;
        const float mean[3] = {123.675f, 116.28f, 103.53f}, sd[3] = {58.395f, 57.12f, 57.375f};
#pragma unroll
        for (int ch = 0; ch < 3; ch++) s_img[((size_t)b * 3 + ch) * QQ + q] = simg[((size_t)b * 3 + ch) * SS + pix0] * sd[ch] + mean[ch];
        const int32_t *bx = boxes + b * 4;
        roi[(size_t)b * QQ + q] = (c.Y >= bx[0] && c.Y < bx[1] && c.X >= bx[2] && c.X < bx[3]) ? 1.0f : 0.0f;
        unlabel[(size_t)b * QQ + q] = ((int)maskA[(size_t)b * SS + pix0] == 255) ? 1 : 0;
    }
    const int tid = threadIdx.y * 16 + threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float v = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    // 64 shards of the 8 sums (workgroup number & 63): thousands of workgroups adding to the same 8 addresses serialise at ~20 ns per add;
    // integer addition is associative, so the total does not depend on the sharding either
    const unsigned wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (tid < 8) atomicAdd(&sums[(wg & 63u) * 8 + tid], fix32(red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid], flag));
}

__global__ void seg_loss_sums_kernel(const unsigned long long *__restrict__ fix, const unsigned long long *__restrict__ flag, float *__restrict__ sums)
{
    if (threadIdx.x < 8) {
        unsigned long long t = 0;
        for (int sh = 0; sh < 64; sh++) t += fix[sh * 8 + threadIdx.x];
        sums[threadIdx.x] = *flag ? __builtin_nanf("") : (float)((double)(long long)t * (1.0 / 4294967296.0));
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------
// d/dz_k(pixel) = g_seg * [cA(pix) (p_k - [k==lA]) + cB(pix) (p_k - [k==lB])] + p_k (dP_k - sum_j p_j dP_j),
//   dP_k = 0.25 * G_k(quad),  G = -2 * g_regw * AS / N * roi   (utils/seg_helper.py:899-902 + the x0.5 mean's adjoint)
//   cM(pix) = w_M,bg / (count_M,bg + 1e-6) on a background pixel of map M, w_M,fg / (count_M,fg + 1e-6) on a foreground one, 0 on ignore
// SegWeights: the four blend weights of main.py:200-203 x seg_helper.py:813 (fg_alpha a, aux blend b): A = ((1-b)(1-a), (1-b)a), B = (b(1-a), ba)
struct SegWeights { float a_bg, a_fg, b_bg, b_fg; };

template <bool HAS_B>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float *__restrict__ seg_lr, const float *__restrict__ maskA,
                                                          const float *__restrict__ maskB, const float *__restrict__ sums,
                                                          const float *__restrict__ AS, const float *__restrict__ roi,
                                                          const float *__restrict__ g_seg, const float *__restrict__ g_regw,
                                                          unsigned long long *__restrict__ grad, unsigned long long *__restrict__ flag,
                                                          SegWeights wt, int B, int K, int hs, int ws, int S, float sy, float sx)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];       // [K][TC][TC] logits, then [K][TC][TC] gradient cells (64-bit fixed point)
    const int b = blockIdx.z;
    const QuadCtx c = setup(seg_lr, tile, K, hs, ws, S, sy, sx, b);
    unsigned long long *gt = reinterpret_cast<unsigned long long *>(tile + ((K * TC * TC + 1) & ~1));
    const int tid = threadIdx.y * 16 + threadIdx.x;
    for (int e = tid; e < K * TC * TC; e += 256) gt[e] = 0ull;
    __syncthreads();
    // The gradient of a low-res cell collects 16 x 16 pixels: per-thread LDS atomics on the same four addresses serialise.  In a wave, the
    // 4 x 4 quads whose lane numbers differ in bits 0, 1 (x) and 4, 5 (y) read the same four cells whenever the up-sampling factor is 16
    // and the tile origin a multiple of 32 (checked, not assumed); then they are summed with four butterfly steps and one lane adds.
    bool grp_ok = c.valid && c.t[0].o00 == c.t[3].o00 && c.t[0].o11 == c.t[3].o11 && c.t[0].o01 == c.t[3].o01 && c.t[0].o10 == c.t[3].o10;
#pragma unroll
    for (int sft = 0; sft < 4; sft++) {
        const int x = sft == 0 ? 1 : (sft == 1 ? 2 : (sft == 2 ? 16 : 32));
        grp_ok = grp_ok && __shfl_xor(c.t[0].o00, x, 64) == c.t[0].o00 && __shfl_xor(c.t[0].o11, x, 64) == c.t[0].o11;
    }
    const bool grouped = __all(grp_ok) != 0;
    if (c.valid) {
        const size_t SS = (size_t)S * S;
        const int Sq = S >> 1;
        const size_t QQ = (size_t)Sq * Sq, q = (size_t)(c.Y >> 1) * Sq + (c.X >> 1);
        const float gs = g_seg[0];
        // main.py:200-203, seg_helper.py:813: with fg_alpha = 0.5 and aux blend 0.5 each of the four terms carries 0.25 (w * gs / count, in this order)
        const float cbgA = wt.a_bg * gs / (sums[1] + 1e-6f), cfgA = wt.a_fg * gs / (sums[3] + 1e-6f);
        const float cbgB = HAS_B ? wt.b_bg * gs / (sums[5] + 1e-6f) : 0.f, cfgB = HAS_B ? wt.b_fg * gs / (sums[7] + 1e-6f) : 0.f;
        const float ge = -2.0f * g_regw[0] / (float)B * roi[(size_t)b * QQ + q] * 0.25f;
        float m[4], inv[4], dot[4], ca[4], cb[4];
        int la[4], lb[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float mx = -INFINITY;
            for (int k = 0; k < K; k++) mx = fmaxf(mx, tap(tile + k * TC * TC, c.t[p]));
            float se = 0.f;
            for (int k = 0; k < K; k++) se += __expf(tap(tile + k * TC * TC, c.t[p]) - mx);
            m[p] = mx;
            inv[p] = 1.0f / se;
            const size_t pix = (size_t)(c.Y + (p >> 1)) * S + c.X + (p & 1);
            la[p] = (int)maskA[(size_t)b * SS + pix];
            lb[p] = HAS_B ? (int)maskB[(size_t)b * SS + pix] : 255;
            ca[p] = la[p] == 0 ? cbgA : (la[p] != 255 ? cfgA : 0.f);
            cb[p] = lb[p] == 0 ? cbgB : (lb[p] != 255 ? cfgB : 0.f);
            dot[p] = 0.f;
        }
        if (ge != 0.f) {
            for (int k = 0; k < K; k++) {
                const float dP = ge * AS[((size_t)b * K + k) * QQ + q];
                const float *pl = tile + k * TC * TC;
#pragma unroll
                for (int p = 0; p < 4; p++) dot[p] += __expf(tap(pl, c.t[p]) - m[p]) * inv[p] * dP;
            }
        }
        const bool same = c.t[0].o00 == c.t[3].o00 && c.t[0].o11 == c.t[3].o11 && c.t[0].o01 == c.t[3].o01 && c.t[0].o10 == c.t[3].o10;
        for (int k = 0; k < K; k++) {
            const float *pl = tile + k * TC * TC;
            const float dP = ge != 0.f ? ge * AS[((size_t)b * K + k) * QQ + q] : 0.f;
            float dz[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const float pk = __expf(tap(pl, c.t[p]) - m[p]) * inv[p];
                if (HAS_B) dz[p] = ca[p] * (pk - (la[p] == k ? 1.f : 0.f)) + cb[p] * (pk - (lb[p] == k ? 1.f : 0.f)) + pk * (dP - dot[p]);
                else dz[p] = ca[p] * (pk - (la[p] == k ? 1.f : 0.f)) + pk * (dP - dot[p]);
            }
            unsigned long long *gp = gt + k * TC * TC;
            if (grouped) {    // 4 x 4 quads (lanes differing in bits 0, 1, 4, 5) share their four cells: one lane adds the sum of all sixteen
                float v00 = dz[0] * c.t[0].w00 + dz[1] * c.t[1].w00 + dz[2] * c.t[2].w00 + dz[3] * c.t[3].w00;
                float v01 = dz[0] * c.t[0].w01 + dz[1] * c.t[1].w01 + dz[2] * c.t[2].w01 + dz[3] * c.t[3].w01;
                float v10 = dz[0] * c.t[0].w10 + dz[1] * c.t[1].w10 + dz[2] * c.t[2].w10 + dz[3] * c.t[3].w10;
                float v11 = dz[0] * c.t[0].w11 + dz[1] * c.t[1].w11 + dz[2] * c.t[2].w11 + dz[3] * c.t[3].w11;
#pragma unroll
                for (int sft = 0; sft < 4; sft++) {
                    const int x = sft == 0 ? 1 : (sft == 1 ? 2 : (sft == 2 ? 16 : 32));
                    v00 += __shfl_xor(v00, x, 64);
                    v01 += __shfl_xor(v01, x, 64);
                    v10 += __shfl_xor(v10, x, 64);
                    v11 += __shfl_xor(v11, x, 64);
                }
                if (((threadIdx.y * 16 + threadIdx.x) & 0x33) == 0) {
                    atomicAdd(gp + c.t[0].o00, fix52(v00, flag));
                    atomicAdd(gp + c.t[0].o01, fix52(v01, flag));
                    atomicAdd(gp + c.t[0].o10, fix52(v10, flag));
                    atomicAdd(gp + c.t[0].o11, fix52(v11, flag));
                }
            } else if (same) {       // the quad's four pixels share their four low-res cells (always true for S = 16 h)
                atomicAdd(gp + c.t[0].o00, fix52(dz[0] * c.t[0].w00 + dz[1] * c.t[1].w00 + dz[2] * c.t[2].w00 + dz[3] * c.t[3].w00, flag));
                atomicAdd(gp + c.t[0].o01, fix52(dz[0] * c.t[0].w01 + dz[1] * c.t[1].w01 + dz[2] * c.t[2].w01 + dz[3] * c.t[3].w01, flag));
                atomicAdd(gp + c.t[0].o10, fix52(dz[0] * c.t[0].w10 + dz[1] * c.t[1].w10 + dz[2] * c.t[2].w10 + dz[3] * c.t[3].w10, flag));
                atomicAdd(gp + c.t[0].o11, fix52(dz[0] * c.t[0].w11 + dz[1] * c.t[1].w11 + dz[2] * c.t[2].w11 + dz[3] * c.t[3].w11, flag));
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    atomicAdd(gp + c.t[p].o00, fix52(dz[p] * c.t[p].w00, flag));
                    atomicAdd(gp + c.t[p].o01, fix52(dz[p] * c.t[p].w01, flag));
                    atomicAdd(gp + c.t[p].o10, fix52(dz[p] * c.t[p].w10, flag));
                    atomicAdd(gp + c.t[p].o11, fix52(dz[p] * c.t[p].w11, flag));
                }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < K * TC * TC; e += 256) {
        const unsigned long long v = gt[e];
        if (v != 0ull) {
            const int k = e / (TC * TC), r = e - k * TC * TC;
            const int cy = c.cy0 + r / TC, cx = c.cx0 + r % TC;
            if (cy < hs && cx < ws) atomicAdd(&grad[(((size_t)b * K + k) * hs + cy) * ws + cx], v);
        }
    }
}

__global__ __launch_bounds__(256) void seg_loss_grad_kernel(const unsigned long long *__restrict__ fix, const unsigned long long *__restrict__ flag,
                                                           float *__restrict__ grad, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) grad[i] = *flag ? __builtin_nanf("") : (float)((double)(long long)fix[i] * (1.0 / kFixGrad));
}


// ---- multilabel soft-margin loss (the two classification losses main.py:127-128 and cam_loss seg_helper.py:593-602), forward and gradient
// in one pass: loss = mean_r mean_c -( y log s(v) + (1 - y) log s(-v) ),  v = x or relu(x);  d loss / d x = (s(v) - y) / (R C) [x > 0].
// x, y, grad: element (r, c) at (r / HW) * C * HW + c * HW + r % HW  (HW = 1: row-major [R, C]; HW = h w: NCHW planes, r = (b, pixel)).
// torch evaluates this as ~10 element-wise kernels forward and as many backward, four times per step.
__global__ __launch_bounds__(256) void msm_loss_kernel(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ grad,
                                                      double *__restrict__ part, int R, int C, int HW, int relu, float inv_rc)
{
    __shared__ double red[4];
    const int r = blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    if (r < R) {
        const size_t base = (size_t)(r / HW) * C * HW + (size_t)(r % HW);
        float s = 0.f;
        for (int c = 0; c < C; c++) {
            const size_t o = base + (size_t)c * HW;
            const float xv = x[o], yv = y[o];
            const float v = relu ? fmaxf(xv, 0.f) : xv;
            const float e = __expf(-fabsf(v));
            const float ls = fminf(v, 0.f) - log1pf(e);                 // log sigmoid(v)
            s += (1.f - yv) * v - ls;
            const float sg = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);   // sigmoid(v)
            grad[o] = (relu && !(xv > 0.f)) ? 0.f : (sg - yv) * inv_rc;
        }
        acc = (double)s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void msm_loss_finalize_kernel(const double *__restrict__ part, int nparts, float *__restrict__ loss, float inv_rc)
{
    __shared__ double red[256];
    double t = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) t += part[i];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] * (double)inv_rc);
}

// ---- cam_loss targets without the full-resolution teacher seg ----------------------------------------------------
// main.py:227-228 + seg_helper.py:553-568,593-597: seg_ps (sum over scales of up(seg)+unflip(up(seg_flip)), [b,K,S,S]) ->
// mask absent classes with -1e5 -> softmax(x / T) -> foreground channels -> bilinear down to the CAM grid.  The
// down-sampling reads only 4 pixels of every (S/h)^2 block, so only those pixels are ever evaluated: each thread owns one
// (image, cell), evaluates the <=4 source pixels straight from the per-scale LOW-RES teacher outputs and blends them.
struct SegScales {
    const float *p[4];      // [2B, K, h_i, w_i] per scale (original batch then flipped batch)
    int h[4], w[4];
    int n;
};

__device__ __forceinline__ float bilerp_fma(const float *pl, int w, int y0, int y1, int x0, int x1, float ly0, float ly1, float lx0, float lx1)
{
    const float r0 = __builtin_fmaf(pl[y0 * w + x0], lx0, pl[y0 * w + x1] * lx1);
    const float r1 = __builtin_fmaf(pl[y1 * w + x0], lx0, pl[y1 * w + x1] * lx1);
    return __builtin_fmaf(r0, ly0, r1 * ly1);
}

// One WAVE per output cell, the class index on the lane (k = lane, lane + 64): every summed logit is evaluated once (the serial version
// recomputed it in three passes and ran 12 544 threads in total), max / sum are wave reductions.
// AFTER = true is the reference's other branch (seg_helper.py:558-561, --after_softmax true): the softmax runs over all K channels of
// sum_scales / T, then the channels of absent classes are set to zero.  The {0,1} label factor commutes exactly with the bilinear blend
// (0 * x = 0 and 1 * x = x in every term), so it is applied once, to the blended cell.
template <bool AFTER>
__global__ __launch_bounds__(256) void cam_target_kernel(SegScales sc, const float *__restrict__ labels, float *__restrict__ out,
                                                        int B, int K, int S, int oh, int ow, float inv_temp)
{
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= B * oh * ow) return;
    const int lane = threadIdx.x & 63;
    const int b = idx / (oh * ow), cell = idx - b * oh * ow;
    const int oy = cell / ow, ox = cell - oy * ow;
    int Y[2], X[2];
    float wy[2], wx[2];
    src_index(oy, S, (float)S / (float)oh, Y[0], Y[1], wy[0], wy[1]);
    src_index(ox, S, (float)S / (float)ow, X[0], X[1], wx[0], wx[1]);
    const int C = K - 1;
    constexpr int KR = 2;                           // classes per lane: K <= 128
    float z[KR][4];
    bool pres[KR];
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int kr = 0; kr < KR; kr++) {
        const int k = lane + 64 * kr;
        const bool live = k < K;
        const bool present = live && (k == 0 || labels[(size_t)b * C + k - 1] != 0.0f);
        pres[kr] = present;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float zz = -INFINITY;
            if (live) {
                const int py = Y[p >> 1], px = X[p & 1];
                float acc = 0.f;
                for (int s2 = 0; s2 < sc.n; s2++) {
                    const int h = sc.h[s2], w = sc.w[s2];
                    int y0, y1, x0, x1, f0, f1;
                    float ly0, ly1, lx0, lx1, fl0, fl1;
                    src_index(py, h, (float)h / (float)S, y0, y1, ly0, ly1);
                    src_index(px, w, (float)w / (float)S, x0, x1, lx0, lx1);
                    src_index(S - 1 - px, w, (float)w / (float)S, f0, f1, fl0, fl1);
                    const float *a = sc.p[s2] + ((size_t)b * K + k) * h * w;
                    const float *f = sc.p[s2] + ((size_t)(b + B) * K + k) * h * w;
                    const float v = bilerp_fma(a, w, y0, y1, x0, x1, ly0, ly1, lx0, lx1) + bilerp_fma(f, w, y0, y1, f0, f1, ly0, ly1, fl0, fl1);
                    acc = s2 == 0 ? v : acc + v;
                }
                zz = ((AFTER || present) ? acc : -1e5f) * inv_temp;
            }
            z[kr][p] = zz;
            m[p] = fmaxf(m[p], zz);
        }
    }
    float se[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m[p] = fmaxf(m[p], __shfl_xor(m[p], o, 64));
        float e = 0.f;
#pragma unroll
        for (int kr = 0; kr < KR; kr++) {
            z[kr][p] = __expf(z[kr][p] - m[p]);       // exp(-inf) = 0 for the lanes beyond K
            e += z[kr][p];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
        se[p] = e;
    }
#pragma unroll
    for (int kr = 0; kr < KR; kr++) {
        const int k = lane + 64 * kr;
        if (k > 0 && k < K) {
            float acc_out = 0.f;
#pragma unroll
            for (int p = 0; p < 4; p++) acc_out += wy[p >> 1] * wx[p & 1] * (z[kr][p] / se[p]);
            out[(((size_t)b * C + k - 1) * oh + oy) * ow + ox] = (AFTER && !pres[kr]) ? 0.f : acc_out;
        }
    }
}


// ---- softmax over the classes + the regulariser's half-resolution resize, fused (the drop-in get_energy_loss path) -------------------
// utils/seg_helper.py:210-230 hands the full-resolution logits to F.softmax and DenseEnergyLoss.forward resizes the probabilities by 0.5
// (bilinear, align_corners=False: at exactly 0.5 that is the mean of each 2x2 quad, written as torch's kernel writes it).  Through torch that
// is four passes over [b,K,S,S] forward and four backward (1.2 of the 3.2 ms of a b=16, K=21, S=448 forward + backward); here a thread owns
// one half-resolution pixel: per class-loop it reads its quad as two 8-byte loads, nothing of size [b,K,S,S] is written forward, and the
// backward writes d logits once.  Channel loops run in class order (as torch's SpatialSoftMax kernels do).
__global__ __launch_bounds__(256) void softmax_half_fwd_kernel(const float *__restrict__ logit, float *__restrict__ out, int K, int H, int W)
{
    const int Wq = W >> 1, Hq = H >> 1;
    const int xq = blockIdx.x * 64 + (threadIdx.x & 63), yq = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (xq >= Wq || yq >= Hq) return;
    const size_t plane = (size_t)H * W;
    const float *base = logit + (size_t)b * K * plane + (size_t)(2 * yq) * W + 2 * xq;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < K; k++) {
        const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
        m[0] = fmaxf(m[0], r0.x); m[1] = fmaxf(m[1], r0.y); m[2] = fmaxf(m[2], r1.x); m[3] = fmaxf(m[3], r1.y);
    }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k++) {
        const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
        sum[0] += expf(r0.x - m[0]); sum[1] += expf(r0.y - m[1]); sum[2] += expf(r1.x - m[2]); sum[3] += expf(r1.y - m[3]);
    }
    float *o = out + ((size_t)b * K * Hq + yq) * Wq + xq;
    for (int k = 0; k < K; k++) {
        const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
        const float p00 = expf(r0.x - m[0]) / sum[0], p01 = expf(r0.y - m[1]) / sum[1], p10 = expf(r1.x - m[2]) / sum[2], p11 = expf(r1.y - m[3]) / sum[3];
        o[(size_t)k * Hq * Wq] = 0.5f * (0.5f * p00 + 0.5f * p01) + 0.5f * (0.5f * p10 + 0.5f * p11);
    }
}

// d logits [b,K,H,W] from g = d loss / d (half-resolution probabilities): every pixel of a quad receives 0.25 g (the resize's transpose),
// then the softmax backward p (dp - sum_k dp p) with p recomputed from the logits
__global__ __launch_bounds__(256) void softmax_half_bwd_kernel(const float *__restrict__ logit, const float *__restrict__ g, float *__restrict__ dlogit,
                                                             int K, int H, int W)
{
    const int Wq = W >> 1, Hq = H >> 1;
    const int xq = blockIdx.x * 64 + (threadIdx.x & 63), yq = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (xq >= Wq || yq >= Hq) return;
    const size_t plane = (size_t)H * W, qplane = (size_t)Hq * Wq;
    const size_t off = (size_t)b * K * plane + (size_t)(2 * yq) * W + 2 * xq;
    const float *base = logit + off;
    const float *gq = g + ((size_t)b * K * Hq + yq) * Wq + xq;
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < K; k++) {
        const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
        m[0] = fmaxf(m[0], r0.x); m[1] = fmaxf(m[1], r0.y); m[2] = fmaxf(m[2], r1.x); m[3] = fmaxf(m[3], r1.y);
    }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k++) {
        const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
        sum[0] += expf(r0.x - m[0]); sum[1] += expf(r0.y - m[1]); sum[2] += expf(r1.x - m[2]); sum[3] += expf(r1.y - m[3]);
    }
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k++) {
        const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
        const float dp = 0.25f * gq[k * qplane];
        dot[0] += dp * (expf(r0.x - m[0]) / sum[0]); dot[1] += dp * (expf(r0.y - m[1]) / sum[1]);
        dot[2] += dp * (expf(r1.x - m[2]) / sum[2]); dot[3] += dp * (expf(r1.y - m[3]) / sum[3]);
    }
    float *d = dlogit + off;
    for (int k = 0; k < K; k++) {
        const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
        const float dp = 0.25f * gq[k * qplane];
        float2 o0, o1;
        o0.x = (dp - dot[0]) * (expf(r0.x - m[0]) / sum[0]); o0.y = (dp - dot[1]) * (expf(r0.y - m[1]) / sum[1]);
        o1.x = (dp - dot[2]) * (expf(r1.x - m[2]) / sum[2]); o1.y = (dp - dot[3]) * (expf(r1.y - m[3]) / sum[3]);
        *reinterpret_cast<float2 *>(d + k * plane) = o0;
        *reinterpret_cast<float2 *>(d + k * plane + W) = o1;
    }
}

// K <= KMAX (VOC: 21): the quad's K x 4 logits stay in registers -- ONE pass over the logits, where the loops above read them three (forward) and
// four times (backward); at b = 16, K = 21, 448^2 the logits are 270 MB, more than the Infinity Cache holds, so every further pass was an HBM
// pass (round 5).  The same operations on the same values in the same class order: the results are bit-identical to the kernels above.
template <int KMAX>
__global__ __launch_bounds__(256) void softmax_half_fwd_reg_kernel(const float *__restrict__ logit, float *__restrict__ out, int K, int H, int W)
{
    const int Wq = W >> 1, Hq = H >> 1;
    const int xq = blockIdx.x * 64 + (threadIdx.x & 63), yq = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (xq >= Wq || yq >= Hq) return;
    const size_t plane = (size_t)H * W;
    const float *base = logit + (size_t)b * K * plane + (size_t)(2 * yq) * W + 2 * xq;
    float z[KMAX][4];
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) {
            const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
            z[k][0] = r0.x; z[k][1] = r0.y; z[k][2] = r1.x; z[k][3] = r1.y;
        }
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) { m[0] = fmaxf(m[0], z[k][0]); m[1] = fmaxf(m[1], z[k][1]); m[2] = fmaxf(m[2], z[k][2]); m[3] = fmaxf(m[3], z[k][3]); }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) {
#pragma unroll
            for (int j = 0; j < 4; j++) { z[k][j] = expf(z[k][j] - m[j]); sum[j] += z[k][j]; }
        }
    float *o = out + ((size_t)b * K * Hq + yq) * Wq + xq;
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) {
            const float p00 = z[k][0] / sum[0], p01 = z[k][1] / sum[1], p10 = z[k][2] / sum[2], p11 = z[k][3] / sum[3];
            o[(size_t)k * Hq * Wq] = 0.5f * (0.5f * p00 + 0.5f * p01) + 0.5f * (0.5f * p10 + 0.5f * p11);
        }
}

template <int KMAX>
__global__ __launch_bounds__(256) void softmax_half_bwd_reg_kernel(const float *__restrict__ logit, const float *__restrict__ g, float *__restrict__ dlogit,
                                                                 int K, int H, int W)
{
    const int Wq = W >> 1, Hq = H >> 1;
    const int xq = blockIdx.x * 64 + (threadIdx.x & 63), yq = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (xq >= Wq || yq >= Hq) return;
    const size_t plane = (size_t)H * W, qplane = (size_t)Hq * Wq;
    const size_t off = (size_t)b * K * plane + (size_t)(2 * yq) * W + 2 * xq;
    const float *base = logit + off;
    const float *gq = g + ((size_t)b * K * Hq + yq) * Wq + xq;
    float z[KMAX][4], dp[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) {
            const float2 r0 = *reinterpret_cast<const float2 *>(base + k * plane), r1 = *reinterpret_cast<const float2 *>(base + k * plane + W);
            z[k][0] = r0.x; z[k][1] = r0.y; z[k][2] = r1.x; z[k][3] = r1.y;
            dp[k] = 0.25f * gq[k * qplane];
        }
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) { m[0] = fmaxf(m[0], z[k][0]); m[1] = fmaxf(m[1], z[k][1]); m[2] = fmaxf(m[2], z[k][2]); m[3] = fmaxf(m[3], z[k][3]); }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) {
#pragma unroll
            for (int j = 0; j < 4; j++) { z[k][j] = expf(z[k][j] - m[j]); sum[j] += z[k][j]; }
        }
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) {
#pragma unroll
            for (int j = 0; j < 4; j++) dot[j] += dp[k] * (z[k][j] / sum[j]);
        }
    float *d = dlogit + off;
#pragma unroll
    for (int k = 0; k < KMAX; k++)
        if (k < K) {
            float2 o0, o1;
            o0.x = (dp[k] - dot[0]) * (z[k][0] / sum[0]); o0.y = (dp[k] - dot[1]) * (z[k][1] / sum[1]);
            o1.x = (dp[k] - dot[2]) * (z[k][2] / sum[2]); o1.y = (dp[k] - dot[3]) * (z[k][3] / sum[3]);
            *reinterpret_cast<float2 *>(d + k * plane) = o0;
            *reinterpret_cast<float2 *>(d + k * plane + W) = o1;
        }
}

}  // namespace
}  // namespace cosa

using namespace cosa;

static int check_shapes(int B, int K, int hs, int ws, int S)
{
    COSA_REQUIRE(B > 0 && K > 0 && hs > 0 && ws > 0 && S > 0 && (S & 1) == 0 && B <= 65535, "seg_loss: bad shape");
    COSA_REQUIRE(S >= 8 * hs && S >= 8 * ws, "seg_loss: needs an up-sampling factor >= 8 (got %d -> %d)", hs, S);
    COSA_REQUIRE(K <= 255, "seg_loss: at most 255 classes (labels are stored with 255 = ignore)");
    return COSA_OK;
}

/* scratch of the two entry points below: the 64-bit fixed-point sums (8 of the forward, B*K*hs*ws gradient cells of the backward) */
extern "C" size_t cosa_seg_loss_workspace_bytes(int B, int K, int hs, int ws)
{
    if (B <= 0 || K <= 0 || hs <= 0 || ws <= 0) return 0;
    // 64 shards of the 8 forward sums + gradient cells + the sticky "not representable" flag word
    return align_up((size_t)B * K * hs * ws * sizeof(unsigned long long) + (64 * 8 + 1) * sizeof(unsigned long long), 256);
}

/* the general forms: maskB may be NULL (no second label map), four blend weights; the entry points without a suffix are these with both maps and 0.25 x 4 */
extern "C" int cosa_seg_loss_forward_w(const float *seg_lr, const float *maskA, const float *maskB, const float *simg,
                                       const int32_t *boxes, float *sums, float *s_seg, float *s_img, float *roi, uint8_t *unlabel,
                                       int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(seg_lr && maskA && simg && boxes && sums && s_seg && s_img && roi && unlabel && workspace, "cosa_seg_loss_forward: null pointer");
    int rc = check_shapes(B, K, hs, ws, S);
    if (rc) return rc;
    if (workspace_bytes < cosa_seg_loss_workspace_bytes(B, K, hs, ws)) {
        set_error("cosa_seg_loss_forward: workspace too small (size it with cosa_seg_loss_workspace_bytes)");
        return COSA_ENOMEM;
    }
    hipStream_t st = as_stream(stream);
    unsigned long long *fix = static_cast<unsigned long long *>(workspace);
    unsigned long long *flag = fix + 64 * 8 + (size_t)B * K * hs * ws;            // reset here, read by both conversions (a forward always precedes its backward)
    COSA_HIP_CHECK(hipMemsetAsync(fix, 0, 64 * 8 * sizeof(unsigned long long), st));
    COSA_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(unsigned long long), st));
    const dim3 grid((S + 31) / 32, (S + 31) / 32, B), blk(16, 16);
    const size_t lds = (size_t)K * TC * TC * sizeof(float);
    if (maskB)
        hipLaunchKernelGGL(seg_loss_fwd_kernel<true>, grid, blk, lds, st, seg_lr, maskA, maskB, simg, boxes, fix, flag, s_seg, s_img, roi, unlabel, K,
                           hs, ws, S, (float)hs / (float)S, (float)ws / (float)S);
    else
        hipLaunchKernelGGL(seg_loss_fwd_kernel<false>, grid, blk, lds, st, seg_lr, maskA, maskB, simg, boxes, fix, flag, s_seg, s_img, roi, unlabel, K,
                           hs, ws, S, (float)hs / (float)S, (float)ws / (float)S);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_loss_sums_kernel, dim3(1), dim3(64), 0, st, fix, flag, sums);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_seg_loss_forward(const float *seg_lr, const float *maskA, const float *maskB, const float *simg,
                                     const int32_t *boxes, float *sums, float *s_seg, float *s_img, float *roi, uint8_t *unlabel,
                                     int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(maskB, "cosa_seg_loss_forward: null pointer");
    return cosa_seg_loss_forward_w(seg_lr, maskA, maskB, simg, boxes, sums, s_seg, s_img, roi, unlabel, B, K, hs, ws, S, workspace, workspace_bytes,
                                   stream);
}

extern "C" int cosa_seg_loss_backward_w(const float *seg_lr, const float *maskA, const float *maskB, const float *sums, const float *AS,
                                        const float *roi, const float *g_seg, const float *g_regw, float *grad_seg_lr,
                                        float wA_bg, float wA_fg, float wB_bg, float wB_fg,
                                        int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(seg_lr && maskA && sums && AS && roi && g_seg && g_regw && grad_seg_lr && workspace, "cosa_seg_loss_backward: null pointer");
    // (a NaN fails every comparison: refused here as well)
    COSA_REQUIRE(wA_bg >= 0.f && wA_bg <= 1.f && wA_fg >= 0.f && wA_fg <= 1.f && wB_bg >= 0.f && wB_bg <= 1.f && wB_fg >= 0.f && wB_fg <= 1.f,
                 "cosa_seg_loss_backward: blend weights must lie in [0, 1] (got %g %g %g %g)", (double)wA_bg, (double)wA_fg, (double)wB_bg,
                 (double)wB_fg);
    int rc = check_shapes(B, K, hs, ws, S);
    if (rc) return rc;
    const size_t n = (size_t)B * K * hs * ws;
    if (workspace_bytes < cosa_seg_loss_workspace_bytes(B, K, hs, ws)) {
        set_error("cosa_seg_loss_backward: workspace too small (size it with cosa_seg_loss_workspace_bytes)");
        return COSA_ENOMEM;
    }
    hipStream_t st = as_stream(stream);
    unsigned long long *fix = static_cast<unsigned long long *>(workspace) + 64 * 8;
    unsigned long long *flag = fix + n;
    COSA_HIP_CHECK(hipMemsetAsync(fix, 0, n * sizeof(unsigned long long), st));
    const dim3 grid((S + 31) / 32, (S + 31) / 32, B), blk(16, 16);
    const size_t lds = (size_t)((K * TC * TC + 1) & ~1) * sizeof(float) + (size_t)K * TC * TC * sizeof(unsigned long long);
    static size_t lds_set[2] = {0, 0};
    const int hb = maskB ? 1 : 0;
    if (lds > 65536 && lds > lds_set[hb]) {
        const void *fn = hb ? (const void *)seg_loss_bwd_kernel<true> : (const void *)seg_loss_bwd_kernel<false>;
        COSA_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set[hb] = lds;
    }
    const SegWeights wt = {wA_bg, wA_fg, wB_bg, wB_fg};
    if (hb)
        hipLaunchKernelGGL(seg_loss_bwd_kernel<true>, grid, blk, lds, st, seg_lr, maskA, maskB, sums, AS, roi, g_seg, g_regw, fix, flag, wt, B, K,
                           hs, ws, S, (float)hs / (float)S, (float)ws / (float)S);
    else
        hipLaunchKernelGGL(seg_loss_bwd_kernel<false>, grid, blk, lds, st, seg_lr, maskA, maskB, sums, AS, roi, g_seg, g_regw, fix, flag, wt, B, K,
                           hs, ws, S, (float)hs / (float)S, (float)ws / (float)S);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_loss_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fix, flag, grad_seg_lr, n);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_seg_loss_backward(const float *seg_lr, const float *maskA, const float *maskB, const float *sums, const float *AS,
                                      const float *roi, const float *g_seg, const float *g_regw, float *grad_seg_lr,
                                      int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(maskB, "cosa_seg_loss_backward: null pointer");
    return cosa_seg_loss_backward_w(seg_lr, maskA, maskB, sums, AS, roi, g_seg, g_regw, grad_seg_lr, 0.25f, 0.25f, 0.25f, 0.25f, B, K, hs, ws, S,
                                    workspace, workspace_bytes, stream);
}

// multilabel_soft_margin_loss(v, y) with v = x or relu(x), and its gradient w.r.t. x for a unit upstream gradient (F.multilabel_soft_margin_loss,
// main.py:127-128, seg_helper.py:593-602).  x / y / grad fp32 with the element layout above; workspace: ceil(R / 256) doubles.
extern "C" int cosa_msm_loss(const float *x, const float *y, float *grad, float *loss, void *workspace, int R, int C, int HW, int relu, void *stream)
{
    COSA_REQUIRE(x && y && grad && loss && workspace && R > 0 && C > 0 && HW > 0 && R % HW == 0, "cosa_msm_loss: bad arguments");
    const int nblk = (R + 255) / 256;
    const float inv_rc = (float)(1.0 / ((double)R * (double)C));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(msm_loss_kernel, dim3(nblk), dim3(256), 0, st, x, y, grad, static_cast<double *>(workspace), R, C, HW, relu, inv_rc);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(msm_loss_finalize_kernel, dim3(1), dim3(256), 0, st, static_cast<const double *>(workspace), nblk, loss, inv_rc);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

/* after_softmax: 0 -- absent classes masked with -1e5 before the softmax (the reference's default); 1 -- softmax over all K channels, absent
 * classes zeroed afterwards (seg_helper.py:558-561) */
extern "C" int cosa_cam_loss_targets_m(const float *const *seg_scales, const int *hs, const int *ws, int n_scales, const float *labels,
                                       float *out, int B, int K, int S, int oh, int ow, float temperature, int after_softmax, void *stream)
{
    COSA_REQUIRE(seg_scales && hs && ws && labels && out && n_scales >= 1 && n_scales <= 4, "cosa_cam_loss_targets: bad arguments");
    COSA_REQUIRE(B > 0 && K > 1 && S > 0 && oh > 0 && ow > 0 && temperature > 0.f, "cosa_cam_loss_targets: bad shape");
    COSA_REQUIRE(after_softmax == 0 || after_softmax == 1, "cosa_cam_loss_targets: after_softmax must be 0 or 1 (got %d)", after_softmax);
    SegScales sc;
    sc.n = n_scales;
    for (int i = 0; i < 4; i++) {
        sc.p[i] = i < n_scales ? seg_scales[i] : nullptr;
        sc.h[i] = i < n_scales ? hs[i] : 1;
        sc.w[i] = i < n_scales ? ws[i] : 1;
    }
    COSA_REQUIRE(K <= 128, "cosa_cam_loss_targets: at most 128 classes (got %d)", K);
    const int total = B * oh * ow;
    if (after_softmax)
        hipLaunchKernelGGL(cam_target_kernel<true>, dim3((total + 3) / 4), dim3(256), 0, as_stream(stream), sc, labels, out, B, K, S, oh, ow,
                           1.0f / temperature);
    else
        hipLaunchKernelGGL(cam_target_kernel<false>, dim3((total + 3) / 4), dim3(256), 0, as_stream(stream), sc, labels, out, B, K, S, oh, ow,
                           1.0f / temperature);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_cam_loss_targets(const float *const *seg_scales, const int *hs, const int *ws, int n_scales, const float *labels,
                                     float *out, int B, int K, int S, int oh, int ow, float temperature, void *stream)
{
    return cosa_cam_loss_targets_m(seg_scales, hs, ws, n_scales, labels, out, B, K, S, oh, ow, temperature, 0, stream);
}

/* softmax over the classes of full-resolution logits [B,K,H,W] followed by DenseEnergyLoss's resize by 0.5 (H, W even), and its backward */
extern "C" int cosa_softmax_halfres_forward(const float *logit, float *out, int B, int K, int H, int W, void *stream)
{
    COSA_REQUIRE(logit && out && B > 0 && K > 0 && H > 0 && W > 0 && B <= 65535, "cosa_softmax_halfres_forward: bad arguments");
    COSA_REQUIRE(H % 2 == 0 && W % 2 == 0, "cosa_softmax_halfres_forward: H and W must be even");
    const dim3 grid((W / 2 + 63) / 64, (H / 2 + 3) / 4, B);
    if (K <= 24) hipLaunchKernelGGL(softmax_half_fwd_reg_kernel<24>, grid, dim3(256), 0, as_stream(stream), logit, out, K, H, W);
    else hipLaunchKernelGGL(softmax_half_fwd_kernel, grid, dim3(256), 0, as_stream(stream), logit, out, K, H, W);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_softmax_halfres_backward(const float *logit, const float *grad_out, float *grad_logit, int B, int K, int H, int W, void *stream)
{
    COSA_REQUIRE(logit && grad_out && grad_logit && B > 0 && K > 0 && H > 0 && W > 0 && B <= 65535, "cosa_softmax_halfres_backward: bad arguments");
    COSA_REQUIRE(H % 2 == 0 && W % 2 == 0, "cosa_softmax_halfres_backward: H and W must be even");
    const dim3 grid((W / 2 + 63) / 64, (H / 2 + 3) / 4, B);
    if (K <= 24) hipLaunchKernelGGL(softmax_half_bwd_reg_kernel<24>, grid, dim3(256), 0, as_stream(stream), logit, grad_out, grad_logit, K, H, W);
    else hipLaunchKernelGGL(softmax_half_bwd_kernel, grid, dim3(256), 0, as_stream(stream), logit, grad_out, grad_logit, K, H, W);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

// ---- the student's patch-projection weight gradient at K % 64 (an 8-pixel-patch ViT: K = 3 * 8 * 8 = 192) ----------------------------
// dW[N,K] (fp32) = dY[M,N]^T X[M,K],  db[N] = column sums of dY  (bf16 operands).  The 256 x 128-tile weight-gradient kernel of
// gemm_kernels.hip takes K % 128 only; this is ~15 GFLOP per step at 448^2 x 16 (against ~43 TFLOP for the student), so a plain VALU kernel:
// pass 1, grid (N/64, K/64, S): a 256-thread workgroup sums its slice of rows into a 64 x 64 partial tile (4 x 4 per thread, rows staged
// through LDS 32 at a time) and writes slab s of the workspace; pass 2 adds the S slabs in slab order.  No atomics: the same bits every run.
namespace cosa {
namespace {

constexpr int PW_T = 64, PW_R = 32;

__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

__global__ __launch_bounds__(256) void patch_wgrad_partial_kernel(const unsigned short *__restrict__ dY, const unsigned short *__restrict__ X,
                                                                  float *__restrict__ part, float *__restrict__ dbpart, int M, int N, int K,
                                                                  int rows_per)
{
    __shared__ float sY[PW_R][PW_T + 1], sX[PW_R][PW_T + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * PW_T, k0 = blockIdx.y * PW_T, s = blockIdx.z;
    const int m0 = s * rows_per, m1 = min(M, m0 + rows_per);
    const int lr = tid >> 3, lc = (tid & 7) * 8;                 // staging: one 16-byte piece (8 columns) of one row per thread
    float acc[4][4], dbacc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        dbacc[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.f;
    }
    for (int r0 = m0; r0 < m1; r0 += PW_R) {
        const int r = r0 + lr;
        uint4 qy = make_uint4(0, 0, 0, 0), qx = make_uint4(0, 0, 0, 0);
        if (r < m1) {
            qy = *reinterpret_cast<const uint4 *>(dY + (size_t)r * N + n0 + lc);
            qx = *reinterpret_cast<const uint4 *>(X + (size_t)r * K + k0 + lc);
        }
        __syncthreads();                                         // the previous stage's reads are done
        const unsigned wy[4] = {qy.x, qy.y, qy.z, qy.w}, wx[4] = {qx.x, qx.y, qx.z, qx.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            sY[lr][lc + 2 * q] = bf16_lo(wy[q]);
            sY[lr][lc + 2 * q + 1] = bf16_hi(wy[q]);
            sX[lr][lc + 2 * q] = bf16_lo(wx[q]);
            sX[lr][lc + 2 * q + 1] = bf16_hi(wx[q]);
        }
        __syncthreads();
#pragma unroll 4
        for (int rr = 0; rr < PW_R; rr++) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = sY[rr][ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; j++) b[j] = sX[rr][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                dbacc[i] += a[i];
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
            }
        }
    }
    float *slab = part + (size_t)s * N * K;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) slab[(size_t)(n0 + ty + 16 * i) * K + k0 + tx + 16 * j] = acc[i][j];
    if (dbpart && blockIdx.y == 0 && tx == 0)
#pragma unroll
        for (int i = 0; i < 4; i++) dbpart[(size_t)s * N + n0 + ty + 16 * i] = dbacc[i];
}

__global__ void patch_wgrad_reduce_kernel(const float *__restrict__ part, const float *__restrict__ dbpart, float *__restrict__ dW,
                                          float *__restrict__ db, int S, int N, int K)
{
    const long long NK = (long long)N * K, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < NK) {
        float v = 0.f;
        for (int s = 0; s < S; s++) v += part[(size_t)s * NK + i];
        dW[i] = v;
    } else if (db && i < NK + N) {
        const int n = (int)(i - NK);
        float v = 0.f;
        for (int s = 0; s < S; s++) v += dbpart[(size_t)s * N + n];
        db[n] = v;
    }
}

int patch_wgrad_splits(int M, int N, int K, int *rows_per)
{
    const int tiles = (N / PW_T) * (K / PW_T);
    int S = (2048 + tiles - 1) / tiles;                          // ~2048 workgroups (8 per CU)
    S = max(1, min(S, (M + 255) / 256));                         // at least 256 rows per slab
    int per = (M + S - 1) / S;
    per = (per + PW_R - 1) / PW_R * PW_R;
    if (rows_per) *rows_per = per;
    return (M + per - 1) / per;
}

}  // namespace
}  // namespace cosa

extern "C" size_t cosa_patch_wgrad_workspace_bytes(int M, int N, int K)
{
    if (M <= 0 || N <= 0 || K <= 0 || N % cosa::PW_T || K % cosa::PW_T) return 0;
    const int S = cosa::patch_wgrad_splits(M, N, K, nullptr);
    return cosa::align_up((size_t)S * ((size_t)N * K + N) * sizeof(float), 256);
}

extern "C" int cosa_patch_wgrad_bf16(const void *dY, const void *X, float *dW, float *db, int M, int N, int K, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    using namespace cosa;
    COSA_REQUIRE(dY && X && dW && workspace && M > 0 && N > 0 && K > 0, "cosa_patch_wgrad_bf16: bad arguments");
    COSA_REQUIRE(N % PW_T == 0 && K % PW_T == 0, "cosa_patch_wgrad_bf16: N and K must be multiples of 64 (got %d, %d)", N, K);
    COSA_REQUIRE(((uintptr_t)dY & 15) == 0 && ((uintptr_t)X & 15) == 0, "cosa_patch_wgrad_bf16: dY and X must be 16-byte aligned");
    int per = 0;
    const int S = patch_wgrad_splits(M, N, K, &per);
    const size_t need = (size_t)S * ((size_t)N * K + N) * sizeof(float);
    COSA_REQUIRE(workspace_bytes >= need, "cosa_patch_wgrad_bf16: workspace too small (%zu < %zu)", workspace_bytes, need);
    float *part = static_cast<float *>(workspace), *dbpart = db ? part + (size_t)S * N * K : nullptr;
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(patch_wgrad_partial_kernel, dim3(N / PW_T, K / PW_T, S), dim3(256), 0, st, static_cast<const unsigned short *>(dY),
                       static_cast<const unsigned short *>(X), part, dbpart, M, N, K, per);
    COSA_LAUNCH_CHECK();
    const long long nv = (long long)N * K + (db ? N : 0);
    hipLaunchKernelGGL(patch_wgrad_reduce_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, part, dbpart, dW, db, S, N, K);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
