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
// Both backward kernels add into the cells of scatter_begin / scatter_flush below under this one argument: it asks W g < 16, which
// seg_loss_bwd_kernel meets as above and cam_ce_bwd_kernel with W = g = 1 (two groups of weight 0.5, a unit upstream gradient).
__device__ __forceinline__ unsigned long long fix32(float v, unsigned long long *flag)
{
    if (!(__builtin_fabsf(v) < 2147483648.0f)) { atomicOr(flag, 1ull); return 0ull; }
    return (unsigned long long)(long long)__builtin_rint((double)v * 4294967296.0);
}
constexpr double kFixGrad = 281474976710656.0;          // 2^48
__device__ __forceinline__ unsigned long long fix48(float v, unsigned long long *flag)      // a gradient cell's add: 48 fractional bits, |v| < 16
{
    if (!(__builtin_fabsf(v) < 16.0f)) { atomicOr(flag, 1ull); return 0ull; }
    return (unsigned long long)(long long)__builtin_rint((double)v * kFixGrad);
}

// ---- the up-sampled cross-entropy's shared pieces: seg_loss_* and cam_ce_* (cam_loss v3, at the end of the file) both run on these ----------
// softmax of one quad pixel over the tile's K planes, in class order: its max and 1 / sum-exp; returns the log-sum-exp
__device__ __forceinline__ float pixel_softmax(const float *tile, const Tap &t, int K, float &m, float &inv)
{
    float mx = -INFINITY;
    for (int k = 0; k < K; k++) mx = fmaxf(mx, tap(tile + k * TC * TC, t));
    float se = 0.f;
    for (int k = 0; k < K; k++) se += __expf(tap(tile + k * TC * TC, t) - mx);
    m = mx;
    inv = 1.0f / se;
    return mx + __logf(se);
}

// the class-balanced CE's label rule: 0 is background, 0 < la < K foreground, anything else (255, a label outside the classes) is ignored
__device__ __forceinline__ bool ce_is_bg(int la) { return la == 0; }
__device__ __forceinline__ bool ce_is_fg(int la, int K) { return la > 0 && la < K; }

// backward: the pixel's coefficient on (p_k - [k == la])
__device__ __forceinline__ float ce_coef(int la, int K, float cbg, float cfg) { return ce_is_bg(la) ? cbg : (ce_is_fg(la, K) ? cfg : 0.f); }

// a pixel's weight from a weight map (the _rw entry points): in [0, 1]; anything else -- a NaN too -- counts 0 and sets the sticky flag: NaN out
__device__ __forceinline__ float pixel_weight(const float *__restrict__ rel, size_t at, unsigned long long *flag)
{
    const float w = rel[at];
    if (!(w >= 0.f && w <= 1.f)) { atomicOr(flag, 1ull); return 0.f; }
    return w;
}

// forward: the block's N sums -> shard (workgroup number & 63) of sums[64][N].  64 shards: thousands of workgroups adding to the same N addresses
// serialise at ~20 ns per add; integer addition is associative, so the total does not depend on the sharding either
template <int N>
__device__ __forceinline__ void block_sums_to_shard(const float (&acc)[N], unsigned long long *sums, unsigned long long *flag)
{
    __shared__ float red[4][N];
    const int tid = threadIdx.y * 16 + threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const float v = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    const unsigned wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (tid < N) atomicAdd(&sums[(wg & 63u) * N + tid], fix32(red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid], flag));
}

// sum i of sums[64][N] back in fp32; NaN if any add was not representable (the sticky flag)
__device__ __forceinline__ float shard_total(const unsigned long long *fix, const unsigned long long *flag, int N, int i)
{
    unsigned long long t = 0;
    for (int sh = 0; sh < 64; sh++) t += fix[sh * N + i];
    return *flag ? __builtin_nanf("") : (float)((double)(long long)t * (1.0 / 4294967296.0));
}

// backward: the gradient cells of the block's tile live in LDS behind the logits, in 64-bit fixed point.  A cell collects 16 x 16 pixels, and
// per-thread LDS atomics on the same four addresses serialise.  In a wave, the 4 x 4 quads whose lane numbers differ in bits 0, 1 (x) and 4, 5 (y)
// read the same four cells whenever the up-sampling factor is 16 and the tile origin a multiple of 32 (checked, not assumed): `grouped`, the
// kernels sum them with four butterfly steps and one lane adds.  `same`: the quad's four pixels share their four cells (always at S = 16 h).
// The sums of dz x weight themselves stay in each kernel: under -ffp-contract=fast their rounding follows the code around them, and each
// kernel keeps the form -- and so the bits -- it has always had.
struct Scatter { unsigned long long *cells; bool grouped, same; };

__device__ __forceinline__ Scatter scatter_begin(float *tile, const QuadCtx &c, int K)
{
    Scatter s;
    s.cells = reinterpret_cast<unsigned long long *>(tile + ((K * TC * TC + 1) & ~1));
    for (int e = threadIdx.y * 16 + threadIdx.x; e < K * TC * TC; e += 256) s.cells[e] = 0ull;
    __syncthreads();
    s.same = c.t[0].o00 == c.t[3].o00 && c.t[0].o11 == c.t[3].o11 && c.t[0].o01 == c.t[3].o01 && c.t[0].o10 == c.t[3].o10;
    bool grp_ok = c.valid && s.same;
#pragma unroll
    for (int sft = 0; sft < 4; sft++) {
        const int x = sft == 0 ? 1 : (sft == 1 ? 2 : (sft == 2 ? 16 : 32));
        grp_ok = grp_ok && __shfl_xor(c.t[0].o00, x, 64) == c.t[0].o00 && __shfl_xor(c.t[0].o11, x, 64) == c.t[0].o11;
    }
    s.grouped = __all(grp_ok) != 0;
    return s;
}

// the tile's cells -> the global cells grad[B][K][hs][ws] (every thread of the block)
__device__ __forceinline__ void scatter_flush(const Scatter &s, const QuadCtx &c, unsigned long long *grad, int b, int K, int hs, int ws)
{
    __syncthreads();
    for (int e = threadIdx.y * 16 + threadIdx.x; e < K * TC * TC; e += 256) {
        const unsigned long long v = s.cells[e];
        if (v != 0ull) {
            const int k = e / (TC * TC), r = e - k * TC * TC;
            const int cy = c.cy0 + r / TC, cx = c.cx0 + r % TC;
            if (cy < hs && cx < ws) atomicAdd(&grad[(((size_t)b * K + k) * hs + cy) * ws + cx], v);
        }
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------
// sums[8] = {bgA_sum, bgA_cnt, fgA_sum, fgA_cnt, bgB_sum, bgB_cnt, fgB_sum, fgB_cnt}
// HAS_B = false: no second label map -- nothing of it is loaded and sums[4..7] stay zero (--aux_cam2seg false)
// HAS_W = true (cosa_seg_loss_forward_rw): a per-pixel weight map beside each label map multiplies the pixel's cross-entropy term
// (utils/seg_helper.py:823-835, seg_weightloss); the counts stay the plain counts.  The term is formed as ever and multiplied afterwards: the
// HAS_W = false instantiations are the code they have always been, and a weight of 1.0f changes no bit (x * 1 and fma(x, 1, acc) are exact).
template <bool HAS_B, bool HAS_W>
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const float *__restrict__ seg_lr, const float *__restrict__ maskA,
                                                          const float *__restrict__ maskB, const float *__restrict__ relA,
                                                          const float *__restrict__ relB, const float *__restrict__ simg,
                                                          const int32_t *__restrict__ boxes, unsigned long long *__restrict__ sums,
                                                          unsigned long long *__restrict__ flag, float *__restrict__ s_seg, float *__restrict__ s_img,
                                                          float *__restrict__ roi, unsigned char *__restrict__ unlabel,
                                                          int K, int hs, int ws, int S, float sy, float sx)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];
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
            const float lse = pixel_softmax(tile, c.t[p], K, m[p], inv[p]);
            const size_t pix = (size_t)(c.Y + (p >> 1)) * S + c.X + (p & 1);
            const int la = (int)maskA[(size_t)b * SS + pix], lb = HAS_B ? (int)maskB[(size_t)b * SS + pix] : 255;
            if (!HAS_W) {
                if (ce_is_bg(la)) { acc[0] += lse - tap(tile, c.t[p]); acc[1] += 1.f; }
                else if (ce_is_fg(la, K)) { acc[2] += lse - tap(tile + la * TC * TC, c.t[p]); acc[3] += 1.f; }
                if (HAS_B) {
                    if (ce_is_bg(lb)) { acc[4] += lse - tap(tile, c.t[p]); acc[5] += 1.f; }
                    else if (ce_is_fg(lb, K)) { acc[6] += lse - tap(tile + lb * TC * TC, c.t[p]); acc[7] += 1.f; }
                }
            } else {
                const float wa = pixel_weight(relA, (size_t)b * SS + pix, flag);
                if (ce_is_bg(la)) { const float ce = lse - tap(tile, c.t[p]); acc[0] += ce * wa; acc[1] += 1.f; }
                else if (ce_is_fg(la, K)) { const float ce = lse - tap(tile + la * TC * TC, c.t[p]); acc[2] += ce * wa; acc[3] += 1.f; }
                if (HAS_B) {
                    const float wb = pixel_weight(relB, (size_t)b * SS + pix, flag);
                    if (ce_is_bg(lb)) { const float ce = lse - tap(tile, c.t[p]); acc[4] += ce * wb; acc[5] += 1.f; }
                    else if (ce_is_fg(lb, K)) { const float ce = lse - tap(tile + lb * TC * TC, c.t[p]); acc[6] += ce * wb; acc[7] += 1.f; }
                }
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
        const int la0 = (int)maskA[(size_t)b * SS + pix0];
        unlabel[(size_t)b * QQ + q] = (ce_is_bg(la0) || ce_is_fg(la0, K)) ? 0 : 1;
    }
    block_sums_to_shard<8>(acc, sums, flag);
}

__global__ void seg_loss_sums_kernel(const unsigned long long *__restrict__ fix, const unsigned long long *__restrict__ flag, float *__restrict__ sums)
{
    if (threadIdx.x < 8) sums[threadIdx.x] = shard_total(fix, flag, 8, threadIdx.x);
}

// ---- backward ---------------------------------------------------------------------------------------------------
// d/dz_k(pixel) = g_seg * [cA(pix) (p_k - [k==lA]) + cB(pix) (p_k - [k==lB])] + p_k (dP_k - sum_j p_j dP_j),
//   dP_k = 0.25 * G_k(quad),  G = -2 * g_regw * AS / N * roi   (utils/seg_helper.py:899-902 + the x0.5 mean's adjoint)
//   cM(pix) = w_M,bg / (count_M,bg + 1e-6) on a background pixel of map M, w_M,fg / (count_M,fg + 1e-6) on a foreground one, 0 on ignore
// SegWeights: the four blend weights of main.py:200-203 x seg_helper.py:813 (fg_alpha a, aux blend b): A = ((1-b)(1-a), (1-b)a), B = (b(1-a), ba)
struct SegWeights { float a_bg, a_fg, b_bg, b_fg; };

// HAS_W = true (cosa_seg_loss_backward_rw): the pixel's coefficient, formed as ever, times its weight
template <bool HAS_B, bool HAS_W>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float *__restrict__ seg_lr, const float *__restrict__ maskA,
                                                          const float *__restrict__ maskB, const float *__restrict__ relA,
                                                          const float *__restrict__ relB, const float *__restrict__ sums,
                                                          const float *__restrict__ AS, const float *__restrict__ roi,
                                                          const float *__restrict__ g_seg, const float *__restrict__ g_regw,
                                                          unsigned long long *__restrict__ grad, unsigned long long *__restrict__ flag,
                                                          SegWeights wt, int B, int K, int hs, int ws, int S, float sy, float sx)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];       // [K][TC][TC] logits, then [K][TC][TC] gradient cells (64-bit fixed point)
    const int b = blockIdx.z;
    const QuadCtx c = setup(seg_lr, tile, K, hs, ws, S, sy, sx, b);
    const Scatter sc = scatter_begin(tile, c, K);
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
            pixel_softmax(tile, c.t[p], K, m[p], inv[p]);
            const size_t pix = (size_t)(c.Y + (p >> 1)) * S + c.X + (p & 1);
            la[p] = (int)maskA[(size_t)b * SS + pix];
            lb[p] = HAS_B ? (int)maskB[(size_t)b * SS + pix] : 255;
            ca[p] = ce_coef(la[p], K, cbgA, cfgA);
            cb[p] = ce_coef(lb[p], K, cbgB, cfgB);
            if (HAS_W) {
                ca[p] *= pixel_weight(relA, (size_t)b * SS + pix, flag);
                if (HAS_B) cb[p] *= pixel_weight(relB, (size_t)b * SS + pix, flag);
            }
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
            unsigned long long *gp = sc.cells + k * TC * TC;
            if (sc.grouped) {    // 4 x 4 quads (lanes differing in bits 0, 1, 4, 5) share their four cells: one lane adds the sum of all sixteen
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
                    atomicAdd(gp + c.t[0].o00, fix48(v00, flag));
                    atomicAdd(gp + c.t[0].o01, fix48(v01, flag));
                    atomicAdd(gp + c.t[0].o10, fix48(v10, flag));
                    atomicAdd(gp + c.t[0].o11, fix48(v11, flag));
                }
            } else if (sc.same) {       // the quad's four pixels share their four low-res cells (always true for S = 16 h)
                atomicAdd(gp + c.t[0].o00, fix48(dz[0] * c.t[0].w00 + dz[1] * c.t[1].w00 + dz[2] * c.t[2].w00 + dz[3] * c.t[3].w00, flag));
                atomicAdd(gp + c.t[0].o01, fix48(dz[0] * c.t[0].w01 + dz[1] * c.t[1].w01 + dz[2] * c.t[2].w01 + dz[3] * c.t[3].w01, flag));
                atomicAdd(gp + c.t[0].o10, fix48(dz[0] * c.t[0].w10 + dz[1] * c.t[1].w10 + dz[2] * c.t[2].w10 + dz[3] * c.t[3].w10, flag));
                atomicAdd(gp + c.t[0].o11, fix48(dz[0] * c.t[0].w11 + dz[1] * c.t[1].w11 + dz[2] * c.t[2].w11 + dz[3] * c.t[3].w11, flag));
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    atomicAdd(gp + c.t[p].o00, fix48(dz[p] * c.t[p].w00, flag));
                    atomicAdd(gp + c.t[p].o01, fix48(dz[p] * c.t[p].w01, flag));
                    atomicAdd(gp + c.t[p].o10, fix48(dz[p] * c.t[p].w10, flag));
                    atomicAdd(gp + c.t[p].o11, fix48(dz[p] * c.t[p].w11, flag));
                }
            }
        }
    }
    scatter_flush(sc, c, grad, b, K, hs, ws);
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

// the bilinear taps of full-resolution pixel (py, px) in one h x w scale: rows, columns, and the columns of the mirrored pixel (the flipped half)
struct ScaleTaps { int h, w, y0, y1, x0, x1, f0, f1; float ly0, ly1, lx0, lx1, fl0, fl1; };

__device__ __forceinline__ ScaleTaps scale_taps(int py, int px, int h, int w, int S)
{
    ScaleTaps t;
    t.h = h; t.w = w;
    src_index(py, h, (float)h / (float)S, t.y0, t.y1, t.ly0, t.ly1);
    src_index(px, w, (float)w / (float)S, t.x0, t.x1, t.lx0, t.lx1);
    src_index(S - 1 - px, w, (float)w / (float)S, t.f0, t.f1, t.fl0, t.fl1);
    return t;
}

// class k of image b at that pixel in scale `p` [2B,K,h,w]: the original half plus the un-flipped flipped half
__device__ __forceinline__ float scale_value(const float *p, const ScaleTaps &t, int b, int B, int K, int k)
{
    const float *a = p + ((size_t)b * K + k) * t.h * t.w;
    const float *f = p + ((size_t)(b + B) * K + k) * t.h * t.w;
    return bilerp_fma(a, t.w, t.y0, t.y1, t.x0, t.x1, t.ly0, t.ly1, t.lx0, t.lx1) + bilerp_fma(f, t.w, t.y0, t.y1, t.f0, t.f1, t.ly0, t.ly1, t.fl0, t.fl1);
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
                    const float v = scale_value(sc.p[s2], scale_taps(py, px, sc.h[s2], sc.w[s2], S), b, B, K, k);
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

// the launch geometry of the four tile kernels (seg_loss_fwd / _bwd, cam_ce_fwd / _bwd): a block of 16 x 16 quads per 32 x 32 pixels, the
// forward's LDS (the logits tile) and the backward's (the tile, then its 64-bit gradient cells)
struct TileLaunch { dim3 grid, blk; float sy, sx; size_t lds_fwd, lds_bwd; };

static TileLaunch tile_launch(int B, int K, int hs, int ws, int S)
{
    // lds_bwd is 432 bytes per class: above 64 KB from K = 152, where seg_loss_bwd_kernel's entry point raises the kernel's limit;
    // cam_ce_bwd_kernel has K <= 128 (54 KB) and needs no such step
    return {dim3((S + 31) / 32, (S + 31) / 32, B), dim3(16, 16), (float)hs / (float)S, (float)ws / (float)S, (size_t)K * TC * TC * sizeof(float),
            (size_t)((K * TC * TC + 1) & ~1) * sizeof(float) + (size_t)K * TC * TC * sizeof(unsigned long long)};
}

// the per-scale teacher segs of cosa_cam_loss_targets_m / cosa_cam_label as the kernels take them: 1 to 4 scales, none null or empty
static int pack_scales(const char *who, const float *const *seg_scales, const int *hs, const int *ws, int n_scales, SegScales *sc)
{
    COSA_REQUIRE(seg_scales && hs && ws, "%s: null pointer", who);
    COSA_REQUIRE(n_scales >= 1 && n_scales <= 4, "%s: 1 to 4 scales (got %d)", who, n_scales);
    sc->n = n_scales;
    for (int i = 0; i < 4; i++) {
        COSA_REQUIRE(i >= n_scales || (seg_scales[i] && hs[i] > 0 && ws[i] > 0), "%s: scale %d is null or empty", who, i);
        sc->p[i] = i < n_scales ? seg_scales[i] : nullptr;
        sc->h[i] = i < n_scales ? hs[i] : 1;
        sc->w[i] = i < n_scales ? ws[i] : 1;
    }
    return COSA_OK;
}

/* scratch of the two entry points below: the 64-bit fixed-point sums (8 of the forward, B*K*hs*ws gradient cells of the backward) */
extern "C" size_t cosa_seg_loss_workspace_bytes(int B, int K, int hs, int ws)
{
    if (B <= 0 || K <= 0 || hs <= 0 || ws <= 0) return 0;
    // 64 shards of the 8 forward sums + gradient cells + the sticky "not representable" flag word
    return align_up((size_t)B * K * hs * ws * sizeof(unsigned long long) + (64 * 8 + 1) * sizeof(unsigned long long), 256);
}

/* the weight maps of the _rw entry points: relA beside maskA always, relB exactly when there is a maskB */
static int check_weight_maps(const char *who, const float *maskB, const float *relA, const float *relB)
{
    COSA_REQUIRE(relA, "%s: null weight map", who);
    COSA_REQUIRE((relB != nullptr) == (maskB != nullptr), "%s: a second weight map goes with a second label map, and only with one", who);
    return COSA_OK;
}

/* the general forms: maskB may be NULL (no second label map), four blend weights; the entry points without a suffix are these with both maps and 0.25 x 4.
 * relA / relB: the _rw entry points' weight maps, NULL for every other one */
static int seg_loss_forward_any(const float *seg_lr, const float *maskA, const float *maskB, const float *relA, const float *relB, const float *simg,
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
    const TileLaunch t = tile_launch(B, K, hs, ws, S);
    const auto kern = relA ? (maskB ? seg_loss_fwd_kernel<true, true> : seg_loss_fwd_kernel<false, true>)
                           : (maskB ? seg_loss_fwd_kernel<true, false> : seg_loss_fwd_kernel<false, false>);
    hipLaunchKernelGGL(kern, t.grid, t.blk, t.lds_fwd, st, seg_lr, maskA, maskB, relA, relB, simg, boxes, fix, flag, s_seg, s_img, roi, unlabel, K,
                       hs, ws, S, t.sy, t.sx);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_loss_sums_kernel, dim3(1), dim3(64), 0, st, fix, flag, sums);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_seg_loss_forward_w(const float *seg_lr, const float *maskA, const float *maskB, const float *simg,
                                       const int32_t *boxes, float *sums, float *s_seg, float *s_img, float *roi, uint8_t *unlabel,
                                       int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream)
{
    return seg_loss_forward_any(seg_lr, maskA, maskB, nullptr, nullptr, simg, boxes, sums, s_seg, s_img, roi, unlabel, B, K, hs, ws, S, workspace,
                                workspace_bytes, stream);
}

/* cosa_seg_loss_forward_w with a weight in [0, 1] per pixel of each label map (seg_weightloss, utils/seg_helper.py:823-835) */
extern "C" int cosa_seg_loss_forward_rw(const float *seg_lr, const float *maskA, const float *maskB, const float *simg,
                                        const int32_t *boxes, float *sums, float *s_seg, float *s_img, float *roi, uint8_t *unlabel,
                                        int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream,
                                        const float *relA, const float *relB)
{
    if (int rc = check_weight_maps("cosa_seg_loss_forward_rw", maskB, relA, relB)) return rc;
    return seg_loss_forward_any(seg_lr, maskA, maskB, relA, relB, simg, boxes, sums, s_seg, s_img, roi, unlabel, B, K, hs, ws, S, workspace,
                                workspace_bytes, stream);
}

extern "C" int cosa_seg_loss_forward(const float *seg_lr, const float *maskA, const float *maskB, const float *simg,
                                     const int32_t *boxes, float *sums, float *s_seg, float *s_img, float *roi, uint8_t *unlabel,
                                     int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(maskB, "cosa_seg_loss_forward: null pointer");
    return cosa_seg_loss_forward_w(seg_lr, maskA, maskB, simg, boxes, sums, s_seg, s_img, roi, unlabel, B, K, hs, ws, S, workspace, workspace_bytes,
                                   stream);
}

static int seg_loss_backward_any(const float *seg_lr, const float *maskA, const float *maskB, const float *relA, const float *relB,
                                 const float *sums, const float *AS, const float *roi, const float *g_seg, const float *g_regw,
                                 float *grad_seg_lr, float wA_bg, float wA_fg, float wB_bg, float wB_fg,
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
    const TileLaunch t = tile_launch(B, K, hs, ws, S);
    static size_t lds_set[4] = {0, 0, 0, 0};
    const int hb = maskB ? 1 : 0, inst = hb + (relA ? 2 : 0);
    const auto kern = relA ? (hb ? seg_loss_bwd_kernel<true, true> : seg_loss_bwd_kernel<false, true>)
                           : (hb ? seg_loss_bwd_kernel<true, false> : seg_loss_bwd_kernel<false, false>);
    if (t.lds_bwd > 65536 && t.lds_bwd > lds_set[inst]) {
        COSA_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds_bwd));
        lds_set[inst] = t.lds_bwd;
    }
    const SegWeights wt = {wA_bg, wA_fg, wB_bg, wB_fg};
    hipLaunchKernelGGL(kern, t.grid, t.blk, t.lds_bwd, st, seg_lr, maskA, maskB, relA, relB, sums, AS, roi, g_seg, g_regw, fix, flag, wt, B, K, hs,
                       ws, S, t.sy, t.sx);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_loss_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fix, flag, grad_seg_lr, n);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_seg_loss_backward_w(const float *seg_lr, const float *maskA, const float *maskB, const float *sums, const float *AS,
                                        const float *roi, const float *g_seg, const float *g_regw, float *grad_seg_lr,
                                        float wA_bg, float wA_fg, float wB_bg, float wB_fg,
                                        int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream)
{
    return seg_loss_backward_any(seg_lr, maskA, maskB, nullptr, nullptr, sums, AS, roi, g_seg, g_regw, grad_seg_lr, wA_bg, wA_fg, wB_bg, wB_fg, B, K,
                                 hs, ws, S, workspace, workspace_bytes, stream);
}

/* cosa_seg_loss_backward_w with the forward's weight maps: the pixel's coefficient times its weight (the counts in `sums` are the plain ones) */
extern "C" int cosa_seg_loss_backward_rw(const float *seg_lr, const float *maskA, const float *maskB, const float *sums, const float *AS,
                                         const float *roi, const float *g_seg, const float *g_regw, float *grad_seg_lr,
                                         float wA_bg, float wA_fg, float wB_bg, float wB_fg,
                                         int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream,
                                         const float *relA, const float *relB)
{
    if (int rc = check_weight_maps("cosa_seg_loss_backward_rw", maskB, relA, relB)) return rc;
    return seg_loss_backward_any(seg_lr, maskA, maskB, relA, relB, sums, AS, roi, g_seg, g_regw, grad_seg_lr, wA_bg, wA_fg, wB_bg, wB_fg, B, K, hs,
                                 ws, S, workspace, workspace_bytes, stream);
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
    COSA_REQUIRE(labels && out, "cosa_cam_loss_targets: null pointer");
    COSA_REQUIRE(B > 0 && K > 1 && S > 0 && oh > 0 && ow > 0 && temperature > 0.f, "cosa_cam_loss_targets: bad shape");
    COSA_REQUIRE(after_softmax == 0 || after_softmax == 1, "cosa_cam_loss_targets: after_softmax must be 0 or 1 (got %d)", after_softmax);
    COSA_REQUIRE(K <= 128, "cosa_cam_loss_targets: at most 128 classes (got %d)", K);
    SegScales sc;
    int rc = pack_scales("cosa_cam_loss_targets", seg_scales, hs, ws, n_scales, &sc);
    if (rc) return rc;
    const int total = B * oh * ow;
    const auto kern = after_softmax ? cam_target_kernel<true> : cam_target_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((total + 3) / 4), dim3(256), 0, as_stream(stream), sc, labels, out, B, K, S, oh, ow, 1.0f / temperature);
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

// ---- cam_loss v2 / v3 (the reference's --camloss_version v2 | v3, utils/seg_helper.py:604-653) ----------------------------------------
// Both normalise every CAM plane first: r = relu(x), mn = min r, mx = max r, d2 = mx + 1e-4, n = (r - mn) / d2, with the gradient flowing
// through mn and mx (adaptive_max_pool2d routes it to the FIRST position of the extremum in row-major order).  With g = dL/dn,
// G = sum_plane g and Gn = sum_plane g (r - mn):   dL/dr_i = g_i / d2 - [i == argmin] G / d2 - [i == argmax] Gn / d2^2,   dL/dx = dL/dr [x > 0].
//   v2: L = multilabel_soft_margin(n, y): element-wise, g = (sigmoid(n) - y) / (B h w C): value and gradient from one launch per plane.
//   v3: cam_mix = cat(1 - max_c n, n) [B,K,h,w], L = class-balanced CE (weights 0.5 / 0.5, ignore 255) of its bilinear up-sampling against one
//       label map [B,S,S]: the CE runs on the seg-loss scheme above (LDS tile of the low-resolution planes, taps, 64-bit fixed-point cells),
//       so nothing of size [B,K,S,S] exists; g_n[c] = g_mix[c + 1] - [c == first argmax_c n] g_mix[0].
// One workgroup owns one (b, c) plane, held in LDS.  Every reduction has a fixed order (strided per-thread sums, xor butterflies, the four
// waves in wave order) or is an integer sum: the same bytes every run.  No float atomics.
namespace cosa {
namespace {

constexpr int kCamPlaneMax = 6400;       // h w of one CAM plane: 80 x 80 (a 1280-pixel crop of the 16-pixel-patch encoder)

// (value, index) extrema, ties to the lower index: a total order, so the merge order does not matter
__device__ __forceinline__ void mm_merge(float &mn, int &imn, float &mx, int &imx, float omn, int oimn, float omx, int oimx)
{
    if (omn < mn || (omn == mn && oimn < imn)) { mn = omn; imn = oimn; }
    if (omx > mx || (omx == mx && oimx < imx)) { mx = omx; imx = oimx; }
}

// r[i] = relu(x[i]) into LDS (a NaN stays one); min / max of the plane with their first positions, in every thread
__device__ __forceinline__ void plane_minmax(const float *__restrict__ x, float *r, int HW, float (*redf)[2], int (*redi)[2], float &mn, int &imn,
                                             float &mx, int &imx)
{
    const int tid = threadIdx.x;
    mn = INFINITY; mx = -INFINITY; imn = imx = 0x7fffffff;
    for (int i = tid; i < HW; i += 256) {
        const float xv = x[i];
        const float v = xv > 0.f ? xv : (xv != xv ? xv : 0.f);
        r[i] = v;
        if (v < mn) { mn = v; imn = i; }
        if (v > mx) { mx = v; imx = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float omn = __shfl_xor(mn, o, 64), omx = __shfl_xor(mx, o, 64);
        const int oimn = __shfl_xor(imn, o, 64), oimx = __shfl_xor(imx, o, 64);
        mm_merge(mn, imn, mx, imx, omn, oimn, omx, oimx);
    }
    if ((tid & 63) == 0) { redf[tid >> 6][0] = mn; redf[tid >> 6][1] = mx; redi[tid >> 6][0] = imn; redi[tid >> 6][1] = imx; }
    __syncthreads();
    mn = redf[0][0]; mx = redf[0][1]; imn = redi[0][0]; imx = redi[0][1];
#pragma unroll
    for (int wv = 1; wv < 4; wv++) mm_merge(mn, imn, mx, imx, redf[wv][0], redi[wv][0], redf[wv][1], redi[wv][1]);
}

// NV per-thread doubles -> their plane sums in every thread: butterfly inside the wave, then the four waves in wave order
template <int NV>
__device__ __forceinline__ void plane_sums(double *v, double (*red)[NV])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < NV; j++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
        if ((tid & 63) == 0) red[tid >> 6][j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; j++) v[j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
}

// the normalisation's adjoint for element i of a plane (see the head of this section)
__device__ __forceinline__ float norm_adjoint(float g, float xv, int i, int imn, int imx, double d2, double G, double Gn)
{
    if (!(xv > 0.f)) return 0.f;
    double d = (double)g / d2;
    if (i == imn) d -= G / d2;
    if (i == imx) d -= Gn / (d2 * d2);
    return (float)d;
}

// v2: one plane per workgroup -- grad[plane] complete, part[plane] = the plane's sum of loss terms
__global__ __launch_bounds__(256) void cam_v2_plane_kernel(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ grad,
                                                          double *__restrict__ part, int HW, float inv_n)
{
    __shared__ float r[kCamPlaneMax], gl[kCamPlaneMax];
    __shared__ float redf[4][2];
    __shared__ int redi[4][2];
    __shared__ double redd[4][3];
    const size_t base = (size_t)blockIdx.x * HW;
    const int tid = threadIdx.x;
    float mn, mx;
    int imn, imx;
    plane_minmax(x + base, r, HW, redf, redi, mn, imn, mx, imx);
    const float d2 = mx + 1e-4f;
    double s[3] = {0.0, 0.0, 0.0};       // loss terms, G, Gn
    for (int i = tid; i < HW; i += 256) {
        const float rm = r[i] - mn, v = rm / d2, yv = y[base + i];
        const float e = __expf(-fabsf(v));
        const float ls = fminf(v, 0.f) - log1pf(e);                    // log sigmoid(v)
        const float sg = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);   // sigmoid(v)
        const float g = (sg - yv) * inv_n;
        gl[i] = g;
        s[0] += (double)((1.f - yv) * v - ls);
        s[1] += (double)g;
        s[2] += (double)g * (double)rm;
    }
    plane_sums<3>(s, redd);
    for (int i = tid; i < HW; i += 256) grad[base + i] = norm_adjoint(gl[i], x[base + i], i, imn, imx, (double)d2, s[1], s[2]);
    if (tid == 0) part[blockIdx.x] = s[0];
}

// v3 (a): n of plane (b, c) into channel c + 1 of cam_mix [B,C+1,h,w]; stats[plane] = {mn, d2}, idx[plane] = {argmin, argmax}
__global__ __launch_bounds__(256) void cam_v3_plane_kernel(const float *__restrict__ x, float *__restrict__ mix, float *__restrict__ stats,
                                                          int *__restrict__ idx, int C, int HW)
{
    __shared__ float r[kCamPlaneMax];
    __shared__ float redf[4][2];
    __shared__ int redi[4][2];
    const int plane = blockIdx.x, b = plane / C, c = plane - b * C;
    float mn, mx;
    int imn, imx;
    plane_minmax(x + (size_t)plane * HW, r, HW, redf, redi, mn, imn, mx, imx);
    const float d2 = mx + 1e-4f;
    float *o = mix + ((size_t)b * (C + 1) + c + 1) * HW;
    for (int i = threadIdx.x; i < HW; i += 256) o[i] = (r[i] - mn) / d2;
    if (threadIdx.x == 0) { stats[2 * plane] = mn; stats[2 * plane + 1] = d2; idx[2 * plane] = imn; idx[2 * plane + 1] = imx; }
}

// v3 (a), the cells: channel 0 of cam_mix = 1 - max_c n, arg = the first channel of that maximum
__global__ __launch_bounds__(256) void cam_v3_bg_kernel(float *__restrict__ mix, int *__restrict__ arg, int B, int C, int HW)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * HW) return;
    const int b = t / HW, i = t - b * HW;
    float *p = mix + (size_t)b * (C + 1) * HW + i;
    float m = p[HW];
    int a = 0;
    for (int c = 1; c < C; c++) {
        const float v = p[(size_t)(c + 1) * HW];
        if (v > m) { m = v; a = c; }
    }
    p[0] = 1.f - m;
    arg[t] = a;
}

// v3 (b), forward: class-balanced CE sums of the up-sampled planes against one label map (bytes; 255 and anything >= K: ignored).
// sums: 64 shards of {bg_sum, bg_cnt, fg_sum, fg_cnt} in fix32.
__global__ __launch_bounds__(256) void cam_ce_fwd_kernel(const float *__restrict__ lr, const unsigned char *__restrict__ label,
                                                        unsigned long long *__restrict__ sums, unsigned long long *__restrict__ flag,
                                                        int K, int hs, int ws, int S, float sy, float sx)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int b = blockIdx.z;
    const QuadCtx c = setup(lr, tile, K, hs, ws, S, sy, sx, b);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (c.valid) {
        const size_t SS = (size_t)S * S;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            float m, inv;
            const float lse = pixel_softmax(tile, c.t[p], K, m, inv);
            const int la = (int)label[(size_t)b * SS + (size_t)(c.Y + (p >> 1)) * S + c.X + (p & 1)];
            if (ce_is_bg(la)) { acc[0] += lse - tap(tile, c.t[p]); acc[1] += 1.f; }
            else if (ce_is_fg(la, K)) { acc[2] += lse - tap(tile + la * TC * TC, c.t[p]); acc[3] += 1.f; }
        }
    }
    block_sums_to_shard<4>(acc, sums, flag);
}

// sums[4] in fp32 and the loss 0.5 bg_sum / (bg_cnt + 1e-6) + 0.5 fg_sum / (fg_cnt + 1e-6)
__global__ void cam_ce_sums_kernel(const unsigned long long *__restrict__ fix, const unsigned long long *__restrict__ flag, float *__restrict__ sums,
                                   float *__restrict__ loss)
{
    __shared__ float s[4];
    if (threadIdx.x < 4) s[threadIdx.x] = sums[threadIdx.x] = shard_total(fix, flag, 4, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = 0.5f * (s[0] / (s[1] + 1e-6f)) + 0.5f * (s[2] / (s[3] + 1e-6f));
}

// v3 (b), backward for a unit upstream gradient: d/dz_k(pixel) = c(pix) (p_k - [k == label]), c = 0.5 / (count + 1e-6) of the pixel's group;
// scattered into the low-resolution cells as seg_loss_bwd_kernel does (a cell pre-sums at most all pixels once: |v| <= W g with W = 1, g = 1)
__global__ __launch_bounds__(256) void cam_ce_bwd_kernel(const float *__restrict__ lr, const unsigned char *__restrict__ label,
                                                        const float *__restrict__ sums, unsigned long long *__restrict__ grad,
                                                        unsigned long long *__restrict__ flag, int K, int hs, int ws, int S, float sy, float sx)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];       // [K][TC][TC] planes, then [K][TC][TC] gradient cells (64-bit fixed point)
    const int b = blockIdx.z;
    const QuadCtx c = setup(lr, tile, K, hs, ws, S, sy, sx, b);
    const Scatter sc = scatter_begin(tile, c, K);
    if (c.valid) {
        const size_t SS = (size_t)S * S;
        const float cbg = 0.5f / (sums[1] + 1e-6f), cfg = 0.5f / (sums[3] + 1e-6f);
        float m[4], inv[4], ca[4];
        int la[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            pixel_softmax(tile, c.t[p], K, m[p], inv[p]);
            la[p] = (int)label[(size_t)b * SS + (size_t)(c.Y + (p >> 1)) * S + c.X + (p & 1)];
            ca[p] = ce_coef(la[p], K, cbg, cfg);
        }
        for (int k = 0; k < K; k++) {
            const float *pl = tile + k * TC * TC;
            float dz[4];
#pragma unroll
            for (int p = 0; p < 4; p++) dz[p] = ca[p] * (__expf(tap(pl, c.t[p]) - m[p]) * inv[p] - (la[p] == k ? 1.f : 0.f));
            unsigned long long *gp = sc.cells + k * TC * TC;
            if (sc.grouped || sc.same) {
                float v00 = dz[0] * c.t[0].w00 + dz[1] * c.t[1].w00 + dz[2] * c.t[2].w00 + dz[3] * c.t[3].w00;
                float v01 = dz[0] * c.t[0].w01 + dz[1] * c.t[1].w01 + dz[2] * c.t[2].w01 + dz[3] * c.t[3].w01;
                float v10 = dz[0] * c.t[0].w10 + dz[1] * c.t[1].w10 + dz[2] * c.t[2].w10 + dz[3] * c.t[3].w10;
                float v11 = dz[0] * c.t[0].w11 + dz[1] * c.t[1].w11 + dz[2] * c.t[2].w11 + dz[3] * c.t[3].w11;
                if (sc.grouped) {
#pragma unroll
                    for (int sft = 0; sft < 4; sft++) {
                        const int x = sft == 0 ? 1 : (sft == 1 ? 2 : (sft == 2 ? 16 : 32));
                        v00 += __shfl_xor(v00, x, 64);
                        v01 += __shfl_xor(v01, x, 64);
                        v10 += __shfl_xor(v10, x, 64);
                        v11 += __shfl_xor(v11, x, 64);
                    }
                }
                if (!sc.grouped || ((threadIdx.y * 16 + threadIdx.x) & 0x33) == 0) {
                    atomicAdd(gp + c.t[0].o00, fix48(v00, flag));
                    atomicAdd(gp + c.t[0].o01, fix48(v01, flag));
                    atomicAdd(gp + c.t[0].o10, fix48(v10, flag));
                    atomicAdd(gp + c.t[0].o11, fix48(v11, flag));
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    atomicAdd(gp + c.t[p].o00, fix48(dz[p] * c.t[p].w00, flag));
                    atomicAdd(gp + c.t[p].o01, fix48(dz[p] * c.t[p].w01, flag));
                    atomicAdd(gp + c.t[p].o10, fix48(dz[p] * c.t[p].w10, flag));
                    atomicAdd(gp + c.t[p].o11, fix48(dz[p] * c.t[p].w11, flag));
                }
            }
        }
    }
    scatter_flush(sc, c, grad, b, K, hs, ws);
}

// v3 (c): the fixed-point cells of d L / d cam_mix -> d L / d x of plane (b, c)
__global__ __launch_bounds__(256) void cam_v3_adjoint_kernel(const float *__restrict__ x, const unsigned long long *__restrict__ gfix,
                                                            const unsigned long long *__restrict__ flag, const int *__restrict__ arg,
                                                            const float *__restrict__ stats, const int *__restrict__ idx, float *__restrict__ grad,
                                                            int C, int HW)
{
    __shared__ float gl[kCamPlaneMax];
    __shared__ double redd[4][2];
    const int plane = blockIdx.x, b = plane / C, c = plane - b * C, tid = threadIdx.x;
    const float mn = stats[2 * plane], d2 = stats[2 * plane + 1];
    const int imn = idx[2 * plane], imx = idx[2 * plane + 1];
    const unsigned long long *g0 = gfix + (size_t)b * (C + 1) * HW, *g1 = g0 + (size_t)(c + 1) * HW;
    const int *ar = arg + (size_t)b * HW;
    const float *xp = x + (size_t)plane * HW;
    const bool bad = *flag != 0ull;
    double s[2] = {0.0, 0.0};            // G, Gn
    for (int i = tid; i < HW; i += 256) {
        float g = (float)((double)(long long)g1[i] * (1.0 / kFixGrad));
        if (ar[i] == c) g -= (float)((double)(long long)g0[i] * (1.0 / kFixGrad));
        const float xv = xp[i];
        const float rm = (xv > 0.f ? xv : (xv != xv ? xv : 0.f)) - mn;
        gl[i] = g;
        s[0] += (double)g;
        s[1] += (double)g * (double)rm;
    }
    plane_sums<2>(s, redd);
    float *o = grad + (size_t)plane * HW;
    for (int i = tid; i < HW; i += 256) o[i] = bad ? __builtin_nanf("") : norm_adjoint(gl[i], xp[i], i, imn, imx, (double)d2, s[0], s[1]);
}

// v3 (d): the label map of cam_lossv3_wrap straight from the per-scale low-resolution teacher segs, one thread per pixel of [B,S,S]:
// z_k = sum over scales of scale_value (original half + un-flipped flipped half), what cam_target_kernel sums; an online max / sum-exp over k.
//   AFTER = false: label = first argmax of the masked z (absent classes at -1e5), maximum probability 1 / sum_k exp((z_k - z_max) / T)
//   AFTER = true:  softmax over all K; argmax and maximum over the present classes (background included)
// label = 255 where the maximum probability is not above `thre`.
template <bool AFTER>
__global__ __launch_bounds__(256) void cam_label_kernel(SegScales sc, const float *__restrict__ labels, unsigned char *__restrict__ out,
                                                       int B, int K, int S, float inv_temp, float thre)
{
    const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (px >= S || py >= S) return;
    ScaleTaps t[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++)
        if (s2 < sc.n) t[s2] = scale_taps(py, px, sc.h[s2], sc.w[s2], S);
    const int C = K - 1;
    float m = -INFINITY, se = 0.f, best = -INFINITY;
    int bk = 0;
    for (int k = 0; k < K; k++) {
        const bool present = k == 0 || labels[(size_t)b * C + k - 1] != 0.0f;
        float acc = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 4; s2++)
            if (s2 < sc.n) {
                const float v = scale_value(sc.p[s2], t[s2], b, B, K, k);
                acc = s2 == 0 ? v : acc + v;
            }
        const float z = (AFTER || present) ? acc : -1e5f;
        // (the max is kept on the summed logits and the DIFFERENCE is divided by T: no rounding of z / T itself)
        if (z > m) { se = se * expf((m - z) * inv_temp) + 1.f; m = z; }
        else se += expf((z - m) * inv_temp);
        if ((!AFTER || present) && z > best) { best = z; bk = k; }
    }
    const float maxp = expf((best - m) * inv_temp) / se;
    out[((size_t)b * S + py) * S + px] = maxp > thre ? (unsigned char)bk : (unsigned char)255;
}

size_t cam_v3_ws_layout(int B, int C, int HW, size_t *o_mix, size_t *o_arg, size_t *o_stats, size_t *o_idx, size_t *o_sums)
{
    const size_t cells = (size_t)B * (C + 1) * HW, planes = (size_t)B * C;
    size_t off = (64 * 4 + cells + 1) * sizeof(unsigned long long);      // CE sums (64 shards), gradient cells, the sticky flag
    *o_mix = off;   off += cells * sizeof(float);
    *o_arg = off;   off += (size_t)B * HW * sizeof(int);
    *o_stats = off; off += 2 * planes * sizeof(float);
    *o_idx = off;   off += 2 * planes * sizeof(int);
    *o_sums = off;  off += 4 * sizeof(float);
    return align_up(off, 256);
}

int cam_plane_shapes(const char *who, int B, int C, int h, int w)
{
    COSA_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && B <= 65535, "%s: bad shape", who);
    COSA_REQUIRE(C + 1 <= 128, "%s: at most 128 classes, background included (got %d)", who, C + 1);
    COSA_REQUIRE((long long)h * w <= kCamPlaneMax, "%s: a %d x %d plane is outside the envelope (h w <= %d)", who, h, w, kCamPlaneMax);
    return COSA_OK;
}

}  // namespace
}  // namespace cosa

/* cam_lossv2 on targets already at the CAM's size: cam / targets / grad fp32 [B,C,h,w], loss one float; grad is d loss / d cam for a unit
 * upstream gradient.  workspace: cosa_cam_lossv2_workspace_bytes(B, C) bytes (one double per plane). */
extern "C" size_t cosa_cam_lossv2_workspace_bytes(int B, int C)
{
    if (B <= 0 || C <= 0) return 0;
    return cosa::align_up((size_t)B * C * sizeof(double), 256);
}

extern "C" int cosa_cam_lossv2(const float *cam, const float *targets, float *grad, float *loss, int B, int C, int h, int w, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(cam && targets && grad && loss && workspace, "cosa_cam_lossv2: null pointer");
    int rc = cam_plane_shapes("cosa_cam_lossv2", B, C, h, w);
    if (rc) return rc;
    COSA_REQUIRE(workspace_bytes >= cosa_cam_lossv2_workspace_bytes(B, C), "cosa_cam_lossv2: workspace too small (size it with cosa_cam_lossv2_workspace_bytes)");
    const int HW = h * w, planes = B * C;
    const float inv_n = (float)(1.0 / ((double)planes * (double)HW));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(cam_v2_plane_kernel, dim3(planes), dim3(256), 0, st, cam, targets, grad, static_cast<double *>(workspace), HW, inv_n);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(msm_loss_finalize_kernel, dim3(1), dim3(256), 0, st, static_cast<const double *>(workspace), planes, loss, inv_n);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

/* cam_lossv3 (cambgmax): cam / grad fp32 [B,C,h,w], label bytes [B,S,S] (0 background, 1..C, 255 -- and anything above C -- ignored), loss one
 * float; grad is d loss / d cam for a unit upstream gradient.  S even, S >= 8 h, S >= 8 w. */
extern "C" size_t cosa_cam_lossv3_workspace_bytes(int B, int C, int h, int w)
{
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return 0;
    size_t o[5];
    return cosa::cam_v3_ws_layout(B, C, h * w, o, o + 1, o + 2, o + 3, o + 4);
}

extern "C" int cosa_cam_lossv3(const float *cam, const uint8_t *label, float *grad, float *loss, int B, int C, int h, int w, int S, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(cam && label && grad && loss && workspace, "cosa_cam_lossv3: null pointer");
    int rc = cam_plane_shapes("cosa_cam_lossv3", B, C, h, w);
    if (rc) return rc;
    COSA_REQUIRE(S > 0 && (S & 1) == 0, "cosa_cam_lossv3: the label map's size must be even (got %d)", S);
    COSA_REQUIRE(S >= 8 * h && S >= 8 * w, "cosa_cam_lossv3: needs an up-sampling factor >= 8 (got %d x %d -> %d)", h, w, S);
    COSA_REQUIRE(workspace_bytes >= cosa_cam_lossv3_workspace_bytes(B, C, h, w), "cosa_cam_lossv3: workspace too small (size it with cosa_cam_lossv3_workspace_bytes)");
    const int HW = h * w, K = C + 1, planes = B * C;
    size_t o_mix, o_arg, o_stats, o_idx, o_sums;
    cam_v3_ws_layout(B, C, HW, &o_mix, &o_arg, &o_stats, &o_idx, &o_sums);
    char *base = static_cast<char *>(workspace);
    const size_t cells = (size_t)B * K * HW;
    unsigned long long *fsum = reinterpret_cast<unsigned long long *>(base), *gfix = fsum + 64 * 4, *flag = gfix + cells;
    float *mix = reinterpret_cast<float *>(base + o_mix), *stats = reinterpret_cast<float *>(base + o_stats), *sums = reinterpret_cast<float *>(base + o_sums);
    int *arg = reinterpret_cast<int *>(base + o_arg), *idx = reinterpret_cast<int *>(base + o_idx);
    hipStream_t st = as_stream(stream);
    COSA_HIP_CHECK(hipMemsetAsync(fsum, 0, (64 * 4 + cells + 1) * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(cam_v3_plane_kernel, dim3(planes), dim3(256), 0, st, cam, mix, stats, idx, C, HW);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(cam_v3_bg_kernel, dim3((B * HW + 255) / 256), dim3(256), 0, st, mix, arg, B, C, HW);
    COSA_LAUNCH_CHECK();
    const TileLaunch t = tile_launch(B, K, h, w, S);
    hipLaunchKernelGGL(cam_ce_fwd_kernel, t.grid, t.blk, t.lds_fwd, st, mix, label, fsum, flag, K, h, w, S, t.sy, t.sx);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(cam_ce_sums_kernel, dim3(1), dim3(64), 0, st, fsum, flag, sums, loss);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(cam_ce_bwd_kernel, t.grid, t.blk, t.lds_bwd, st, mix, label, sums, gfix, flag, K, h, w, S, t.sy, t.sx);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(cam_v3_adjoint_kernel, dim3(planes), dim3(256), 0, st, cam, gfix, flag, arg, stats, idx, grad, C, HW);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

/* the label map of cam_lossv3_wrap from the per-scale low-resolution teacher segs (cosa_cam_loss_targets_m's inputs): out bytes [B,S,S] */
extern "C" int cosa_cam_label(const float *const *seg_scales, const int *hs, const int *ws, int n_scales, const float *labels, uint8_t *out,
                              int B, int K, int S, float temperature, float segconf_thre, int after_softmax, void *stream)
{
    COSA_REQUIRE(labels && out, "cosa_cam_label: null pointer");
    COSA_REQUIRE(B > 0 && B <= 65535 && K > 1 && S > 0, "cosa_cam_label: bad shape");
    COSA_REQUIRE(K <= 128, "cosa_cam_label: at most 128 classes (got %d)", K);
    COSA_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "cosa_cam_label: the temperature must be finite and positive (got %g)", (double)temperature);
    COSA_REQUIRE(std::isfinite(segconf_thre), "cosa_cam_label: segconf_thre must be finite (got %g)", (double)segconf_thre);
    COSA_REQUIRE(after_softmax == 0 || after_softmax == 1, "cosa_cam_label: after_softmax must be 0 or 1 (got %d)", after_softmax);
    SegScales sc;
    int rc = pack_scales("cosa_cam_label", seg_scales, hs, ws, n_scales, &sc);
    if (rc) return rc;
    const dim3 grid((S + 63) / 64, (S + 3) / 4, B);
    const auto kern = after_softmax ? cam_label_kernel<true> : cam_label_kernel<false>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, as_stream(stream), sc, labels, out, B, K, S, 1.0f / temperature, segconf_thre);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

// ---- the soft-label seg loss distilled from the teacher's segmentation (utils/seg_helper.py:837-861, seg_softloss) ---------
// Per full-resolution pixel inside the image's crop box: z_k = the sum over scales and flips of the up-sampled teacher segs (what cam_target_kernel and
// cam_label_kernel sum, by the same src_index / bilerp_fma calls), q = softmax(z / (2 n T)) over the background and the present classes,
// l = - sum_k q_k log p_k = lse(s) - sum_k q_k s_k on the student's up-sampled logits s (the seg-loss tile, setup() and pixel_softmax).  The first
// argmax of q puts the pixel into the background (0) or the foreground set; max q <= conf takes it out of both.
//   forward:  {sum_bg l, n_bg, sum_fg l, n_fg} through block_sums_to_shard; one pass over the classes per pixel (an online max / sum-exp that carries
//             sum_k e_k s_k along).
//   backward: d/ds_k(pixel) = c_set (p_k - q_k), c_bg = (1 - a) g / (n_bg + 1e-6), c_fg = a g / (n_fg + 1e-6), into the cells of scatter_begin /
//             scatter_flush (at most all pixels once per add: |v| <= g, the W g < 16 of the argument at fix48 with W = 1).
// The teacher's taps are read from global memory, as the two kernels above read them: per scale and half a 32 x 32 block touches at most
// (32 h_i / S + 2)^2 cells per class -- 8 x 8 at the 5.33x of an 8-pixel-patch encoder's 1.5 scale --, and LDS tiles of them for four scales, two
// halves and 81 classes (166 KB) do not fit beside the backward's cells (35 KB there); the low-resolution planes of a block stay in L1 / L2.
// A block that has no pixel inside the box returns before it reads anything; a pixel outside the box is never evaluated.
namespace cosa {
namespace {

// one axis of a bilinear tap, kept as src_index's first index and second weight: i1 = min(i0 + 1, in - 1) and l0 = 1 - l1 are what src_index
// itself forms from them, so they are formed again at each use -- half the registers of the four scales' taps
struct AxisTap { int i0; float l1; };
struct QuadTaps { AxisTap y[2], x[2], f[2]; };     // of one scale: the quad's two rows, two columns and the two mirrored columns (the flipped half)

__device__ __forceinline__ AxisTap axis_tap(int dst, int in, int S)
{
    AxisTap a;
    int i1;
    float l0;
    src_index(dst, in, (float)in / (float)S, a.i0, i1, l0, a.l1);
    return a;
}

__device__ __forceinline__ int axis_i1(const AxisTap &a, int in) { return a.i0 < in - 1 ? a.i0 + 1 : a.i0; }

__device__ __forceinline__ QuadTaps quad_taps(int Y, int X, int h, int w, int S)
{
    QuadTaps t;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int py = min(Y + j, S - 1), px = min(X + j, S - 1);
        t.y[j] = axis_tap(py, h, S);
        t.x[j] = axis_tap(px, w, S);
        t.f[j] = axis_tap(S - 1 - px, w, S);
    }
    return t;
}

// z_k of quad pixel `pix` (0..3): scale_value's sum, scale by scale in scale order
__device__ __forceinline__ float teacher_z(const SegScales &sc, const QuadTaps (&t)[4], int pix, int b, int B, int K, int k)
{
    float acc = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++)
        if (s2 < sc.n) {
            const int h = sc.h[s2], w = sc.w[s2];
            const AxisTap &y = t[s2].y[pix >> 1], &x = t[s2].x[pix & 1], &f = t[s2].f[pix & 1];
            const float *a = sc.p[s2] + ((size_t)b * K + k) * h * w;
            const float *fl = sc.p[s2] + ((size_t)(b + B) * K + k) * h * w;
            const int y1 = axis_i1(y, h);
            const float yl0 = 1.0f - y.l1;
            const float v = bilerp_fma(a, w, y.i0, y1, x.i0, axis_i1(x, w), yl0, y.l1, 1.0f - x.l1, x.l1) +
                            bilerp_fma(fl, w, y.i0, y1, f.i0, axis_i1(f, w), yl0, y.l1, 1.0f - f.l1, f.l1);
            acc = s2 == 0 ? v : acc + v;
        }
    return acc;
}

__device__ __forceinline__ bool soft_present(const float *__restrict__ labels, int b, int K, int k)
{
    return k == 0 || labels[(size_t)b * (K - 1) + k - 1] != 0.0f;
}

// the target's statistics at one pixel over the present classes, in class order: m = max z (bk its first position), se = sum exp((z - m) inv_t), so
// q_k = exp((z_k - m) inv_t) / se and max q = 1 / se; DOT: dot = sum exp((z_k - m) inv_t) s_k on the student's logit s_k of the same pixel.
// The forward and the backward run this one function: the same m, se and bk, so the same set and gate.
struct SoftStat { float m, se, dot; int bk; };

template <bool DOT>
__device__ __forceinline__ SoftStat soft_stat(const SegScales &sc, const QuadTaps (&t)[4], int pix, const float *__restrict__ labels, int b, int B, int K,
                                              float inv_t, const float *tile, const Tap &st)
{
    SoftStat s = {-INFINITY, 0.f, 0.f, 0};
    for (int k = 0; k < K; k++) {
        if (!soft_present(labels, b, K, k)) continue;
        const float z = teacher_z(sc, t, pix, b, B, K, k);
        const float sk = DOT ? tap(tile + k * TC * TC, st) : 0.f;
        if (z > s.m) {
            const float r = expf((s.m - z) * inv_t);
            s.se = s.se * r + 1.f;
            if (DOT) s.dot = s.dot * r + sk;
            s.m = z;
            s.bk = k;
        } else {
            const float e = expf((z - s.m) * inv_t);
            s.se += e;
            if (DOT) s.dot += e * sk;
        }
    }
    return s;
}

// does the block's 32 x 32 pixels meet the box (y0, y1, x0, x1)?  The same answer in every thread of the block.
__device__ __forceinline__ bool block_meets_box(const int32_t *bx)
{
    const int by = blockIdx.y * 32, bxx = blockIdx.x * 32;
    return by < bx[1] && by + 32 > bx[0] && bxx < bx[3] && bxx + 32 > bx[2];
}

__device__ __forceinline__ bool in_box(const int32_t *bx, int py, int px) { return py >= bx[0] && py < bx[1] && px >= bx[2] && px < bx[3]; }

// sums: 64 shards of {bg_sum, bg_cnt, fg_sum, fg_cnt} in fix32
__global__ __launch_bounds__(256) void seg_soft_fwd_kernel(const float *__restrict__ seg_lr, SegScales sc, const float *__restrict__ labels,
                                                          const int32_t *__restrict__ boxes, unsigned long long *__restrict__ sums,
                                                          unsigned long long *__restrict__ flag, int B, int K, int hs, int ws, int S, float sy, float sx,
                                                          float inv_t, float conf)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int b = blockIdx.z;
    const int32_t *bx = boxes + b * 4;
    if (!block_meets_box(bx)) return;
    const QuadCtx c = setup(seg_lr, tile, K, hs, ws, S, sy, sx, b);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (c.valid) {
        QuadTaps t[4];
#pragma unroll
        for (int s2 = 0; s2 < 4; s2++)
            if (s2 < sc.n) t[s2] = quad_taps(c.Y, c.X, sc.h[s2], sc.w[s2], S);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            if (!in_box(bx, c.Y + (p >> 1), c.X + (p & 1))) continue;
            float m, inv;
            const float lse = pixel_softmax(tile, c.t[p], K, m, inv);
            const SoftStat s = soft_stat<true>(sc, t, p, labels, b, B, K, inv_t, tile, c.t[p]);
            if (!(1.0f / s.se <= conf)) {       // (a NaN target passes the gate and reaches the sticky flag: NaN out, not a pixel dropped in silence)
                const float l = lse - s.dot / s.se;
                if (s.bk == 0) { acc[0] += l; acc[1] += 1.f; }
                else { acc[2] += l; acc[3] += 1.f; }
            }
        }
    }
    block_sums_to_shard<4>(acc, sums, flag);
}

// sums[4] in fp32 and the loss (1 - a) bg_sum / (bg_cnt + 1e-6) + a fg_sum / (fg_cnt + 1e-6): an empty set contributes 0
__global__ void seg_soft_sums_kernel(const unsigned long long *__restrict__ fix, const unsigned long long *__restrict__ flag, float *__restrict__ sums,
                                     float *__restrict__ loss, float fg_alpha)
{
    __shared__ float s[4];
    if (threadIdx.x < 4) s[threadIdx.x] = sums[threadIdx.x] = shard_total(fix, flag, 4, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (1.0f - fg_alpha) * (s[0] / (s[1] + 1e-6f)) + fg_alpha * (s[2] / (s[3] + 1e-6f));
}

__global__ __launch_bounds__(256) void seg_soft_bwd_kernel(const float *__restrict__ seg_lr, SegScales sc, const float *__restrict__ labels,
                                                          const int32_t *__restrict__ boxes, const float *__restrict__ sums,
                                                          const float *__restrict__ upstream, unsigned long long *__restrict__ grad,
                                                          unsigned long long *__restrict__ flag, int B, int K, int hs, int ws, int S, float sy, float sx,
                                                          float inv_t, float conf, float fg_alpha)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];       // [K][TC][TC] logits, then [K][TC][TC] gradient cells (64-bit fixed point)
    const int b = blockIdx.z;
    const int32_t *bx = boxes + b * 4;
    if (!block_meets_box(bx)) return;
    const QuadCtx c = setup(seg_lr, tile, K, hs, ws, S, sy, sx, b);
    const Scatter scat = scatter_begin(tile, c, K);
    if (c.valid) {
        const float g = upstream[0];
        const float cbg = (1.0f - fg_alpha) * g / (sums[1] + 1e-6f), cfg = fg_alpha * g / (sums[3] + 1e-6f);
        QuadTaps t[4];
#pragma unroll
        for (int s2 = 0; s2 < 4; s2++)
            if (s2 < sc.n) t[s2] = quad_taps(c.Y, c.X, sc.h[s2], sc.w[s2], S);
        float m[4], inv[4], tm[4], tinv[4], co[4];
        bool live[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            m[p] = inv[p] = tm[p] = tinv[p] = co[p] = 0.f;
            live[p] = false;
            if (!in_box(bx, c.Y + (p >> 1), c.X + (p & 1))) continue;
            const SoftStat s = soft_stat<false>(sc, t, p, labels, b, B, K, inv_t, tile, c.t[p]);
            if (!(1.0f / s.se <= conf)) {
                pixel_softmax(tile, c.t[p], K, m[p], inv[p]);
                tm[p] = s.m;
                tinv[p] = 1.0f / s.se;
                co[p] = s.bk == 0 ? cbg : cfg;
                live[p] = true;
            }
        }
        for (int k = 0; k < K; k++) {
            const float *pl = tile + k * TC * TC;
            const bool present = soft_present(labels, b, K, k);
            float dz[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                dz[p] = 0.f;
                if (live[p]) {
                    const float pk = __expf(tap(pl, c.t[p]) - m[p]) * inv[p];
                    const float qk = present ? expf((teacher_z(sc, t, p, b, B, K, k) - tm[p]) * inv_t) * tinv[p] : 0.f;
                    dz[p] = co[p] * (pk - qk);
                }
            }
            unsigned long long *gp = scat.cells + k * TC * TC;
            if (scat.grouped || scat.same) {
                float v00 = dz[0] * c.t[0].w00 + dz[1] * c.t[1].w00 + dz[2] * c.t[2].w00 + dz[3] * c.t[3].w00;
                float v01 = dz[0] * c.t[0].w01 + dz[1] * c.t[1].w01 + dz[2] * c.t[2].w01 + dz[3] * c.t[3].w01;
                float v10 = dz[0] * c.t[0].w10 + dz[1] * c.t[1].w10 + dz[2] * c.t[2].w10 + dz[3] * c.t[3].w10;
                float v11 = dz[0] * c.t[0].w11 + dz[1] * c.t[1].w11 + dz[2] * c.t[2].w11 + dz[3] * c.t[3].w11;
                if (scat.grouped) {
#pragma unroll
                    for (int sft = 0; sft < 4; sft++) {
                        const int x = sft == 0 ? 1 : (sft == 1 ? 2 : (sft == 2 ? 16 : 32));
                        v00 += __shfl_xor(v00, x, 64);
                        v01 += __shfl_xor(v01, x, 64);
                        v10 += __shfl_xor(v10, x, 64);
                        v11 += __shfl_xor(v11, x, 64);
                    }
                }
                if (!scat.grouped || ((threadIdx.y * 16 + threadIdx.x) & 0x33) == 0) {
                    atomicAdd(gp + c.t[0].o00, fix48(v00, flag));
                    atomicAdd(gp + c.t[0].o01, fix48(v01, flag));
                    atomicAdd(gp + c.t[0].o10, fix48(v10, flag));
                    atomicAdd(gp + c.t[0].o11, fix48(v11, flag));
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    if (!live[p]) continue;
                    atomicAdd(gp + c.t[p].o00, fix48(dz[p] * c.t[p].w00, flag));
                    atomicAdd(gp + c.t[p].o01, fix48(dz[p] * c.t[p].w01, flag));
                    atomicAdd(gp + c.t[p].o10, fix48(dz[p] * c.t[p].w10, flag));
                    atomicAdd(gp + c.t[p].o11, fix48(dz[p] * c.t[p].w11, flag));
                }
            }
        }
    }
    scatter_flush(scat, c, grad, b, K, hs, ws);
}

// the shared envelope of the two entry points below (include/cosa_hip.h)
int seg_soft_check(const char *who, const float *const *seg_scales, const int *hs_t, const int *ws_t, int n_scales, int B, int K, int hs, int ws, int S,
                   float temp, float conf, float fg_alpha, size_t workspace_bytes, SegScales *sc)
{
    COSA_REQUIRE(B > 0 && B <= 65535 && hs > 0 && ws > 0 && S > 0 && (S & 1) == 0, "%s: bad shape", who);
    COSA_REQUIRE(K >= 2 && K <= 128, "%s: 2 to 128 classes, background included (got %d)", who, K);
    COSA_REQUIRE(S >= 8 * hs && S >= 8 * ws, "%s: needs an up-sampling factor >= 8 for the student's logits (got %d x %d -> %d)", who, hs, ws, S);
    COSA_REQUIRE(std::isfinite(temp) && temp > 0.f, "%s: the temperature must be finite and positive (got %g)", who, (double)temp);
    COSA_REQUIRE(conf >= 0.f && conf < 1.f, "%s: conf must lie in [0, 1) (got %g)", who, (double)conf);
    COSA_REQUIRE(fg_alpha >= 0.f && fg_alpha <= 1.f, "%s: fg_alpha must lie in [0, 1] (got %g)", who, (double)fg_alpha);
    if (int rc = pack_scales(who, seg_scales, hs_t, ws_t, n_scales, sc)) return rc;
    for (int i = 0; i < n_scales; i++)
        COSA_REQUIRE(hs_t[i] <= S && ws_t[i] <= S, "%s: scale %d (%d x %d) is larger than the full resolution %d", who, i, hs_t[i], ws_t[i], S);
    COSA_REQUIRE(workspace_bytes >= cosa_seg_soft_workspace_bytes(B, K, hs, ws), "%s: workspace too small (size it with cosa_seg_soft_workspace_bytes)", who);
    return COSA_OK;
}

}  // namespace
}  // namespace cosa

/* 64 shards of the 4 forward sums, the B*K*hs*ws gradient cells of the backward, the sticky flag word */
extern "C" size_t cosa_seg_soft_workspace_bytes(int B, int K, int hs, int ws)
{
    if (B <= 0 || K <= 0 || hs <= 0 || ws <= 0) return 0;
    return cosa::align_up((size_t)B * K * hs * ws * sizeof(unsigned long long) + (64 * 4 + 1) * sizeof(unsigned long long), 256);
}

extern "C" int cosa_seg_soft_forward(const float *seg_lr, const float *const *seg_scales, const int *hs_t, const int *ws_t, int n_scales,
                                     const float *labels, const int32_t *boxes, float *sums, float *loss, int B, int K, int hs, int ws, int S,
                                     float temp, float conf, float fg_alpha, void *workspace, size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(seg_lr && labels && boxes && sums && loss && workspace, "cosa_seg_soft_forward: null pointer");
    SegScales sc;
    if (int rc = seg_soft_check("cosa_seg_soft_forward", seg_scales, hs_t, ws_t, n_scales, B, K, hs, ws, S, temp, conf, fg_alpha, workspace_bytes, &sc))
        return rc;
    hipStream_t st = as_stream(stream);
    unsigned long long *fix = static_cast<unsigned long long *>(workspace);
    unsigned long long *flag = fix + 64 * 4 + (size_t)B * K * hs * ws;             // reset here, read by both conversions (a forward precedes its backward)
    COSA_HIP_CHECK(hipMemsetAsync(fix, 0, 64 * 4 * sizeof(unsigned long long), st));
    COSA_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(unsigned long long), st));
    const TileLaunch t = tile_launch(B, K, hs, ws, S);
    hipLaunchKernelGGL(seg_soft_fwd_kernel, t.grid, t.blk, t.lds_fwd, st, seg_lr, sc, labels, boxes, fix, flag, B, K, hs, ws, S, t.sy, t.sx,
                       1.0f / (2.0f * (float)n_scales * temp), conf);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_soft_sums_kernel, dim3(1), dim3(64), 0, st, fix, flag, sums, loss, fg_alpha);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_seg_soft_backward(const float *seg_lr, const float *const *seg_scales, const int *hs_t, const int *ws_t, int n_scales,
                                      const float *labels, const int32_t *boxes, const float *sums, const float *upstream, float *grad_seg_lr,
                                      int B, int K, int hs, int ws, int S, float temp, float conf, float fg_alpha, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(seg_lr && labels && boxes && sums && upstream && grad_seg_lr && workspace, "cosa_seg_soft_backward: null pointer");
    SegScales sc;
    if (int rc = seg_soft_check("cosa_seg_soft_backward", seg_scales, hs_t, ws_t, n_scales, B, K, hs, ws, S, temp, conf, fg_alpha, workspace_bytes, &sc))
        return rc;
    hipStream_t st = as_stream(stream);
    const size_t n = (size_t)B * K * hs * ws;
    unsigned long long *fix = static_cast<unsigned long long *>(workspace) + 64 * 4;
    unsigned long long *flag = fix + n;
    COSA_HIP_CHECK(hipMemsetAsync(fix, 0, n * sizeof(unsigned long long), st));
    const TileLaunch t = tile_launch(B, K, hs, ws, S);                              // (K <= 128: lds_bwd is 54 KB at the most)
    hipLaunchKernelGGL(seg_soft_bwd_kernel, t.grid, t.blk, t.lds_bwd, st, seg_lr, sc, labels, boxes, sums, upstream, fix, flag, B, K, hs, ws, S, t.sy,
                       t.sx, 1.0f / (2.0f * (float)n_scales * temp), conf, fg_alpha);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_loss_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fix, flag, grad_seg_lr, n);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
