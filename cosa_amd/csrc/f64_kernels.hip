// f64_kernels.hip -- the "f64" operand family of the no-grad passes: every operand float64, every product on the f64 MFMA
// (v_mfma_f64_16x16x4_f64).  Mode string "fp64" (DESIGN.md section 20): the float64 side of the conformance criterion's exemption leg on the
// device, for a run's own weights and images.  A check mode only -- never a training teacher.
//
//   cosa_gemm_f64                    Y[M,N] = X[M,K] W[N,K]^T, epilogues +bias | +bias, erf-GELU | +bias +residual (float64, in place allowed);
//                                    X float64, W / bias fp32 (the masters, widened as they are read) or float64
//   cosa_conv3x3_dilated_f64         LargeFOV conv6 / conv7 as an implicit GEMM over the NHWC tokens: the same kernel, its A rows gathered per tap
//   cosa_attn_fwd_f64                softmax(q k^T * scale) v on the packed float64 qkv rows, flash style, nothing of size N^2 leaves the CU
//   cosa_layernorm_f64               nn.LayerNorm over float64 rows with the fp32 gamma / beta
//   cosa_im2col_flip_f64_tokens      the token-shaped float64 operand of the patch projection (images and their mirror images)
//   cosa_resize_bilinear_f64         fp32 images -> float64 planes (the teacher's input rescale)
//   cosa_cam_flip_merge_upsample_f64 the multi-scale tail's up-sampling / un-flip / merge, and per plane the raw logit magnitude
//   cosa_cam_minmax_norm_f64         min-max normalisation in place, and per plane what it divided by
//
// Numerics contract of the GEMM (and of the conv): every output element is ONE accumulator of the MFMA, fed the products of ascending k in
// steps of 4 starting from zero: no split-K, no atomics, the same sequence whatever M is, wherever the row sits and whatever the other rows
// hold (a lane's accumulator registers belong to one column and four rows; the MFMA forms each element from its own row of A and column of
// B alone).  The epilogue follows in float64.  Built with -ffp-contract=off -fno-fast-math: erf and exp are the double routines.
#include "wave_reduce.hpp"      // wave_max
#include <algorithm>
#include <cmath>

namespace cosa {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 64, BN = 64;   // block tile: 2 x 2 waves of 32 x 32, each 2 x 2 MFMA tiles of 16 x 16
constexpr int BK = 16;            // k per LDS stage (K % 16 == 0; a conv tap's Cin is a multiple, so a stage never straddles taps)
constexpr int LDS_LD = BM + 2;    // row stride of a k-major stage in doubles

enum { F64_EPI_BIAS = 0, F64_EPI_GELU = 1, F64_EPI_RESIDUAL = 2, F64_EPI_RELU = 3 };

struct GemmArgs {
    const double *X;
    const void *W, *bias;
    const double *res;
    double *Y;
    int M, N, K, ldx, ldw, ldr, ldy, epi;
    // implicit-GEMM conv (CONV): X is the token matrix, image b at X + b * img_stride, pixel rows of stride ldx; K = 9 * Cin
    int h, w, Cin, dil;
    long long img_stride;
};

__device__ __forceinline__ void load4(const double *p, double (&v)[4])
{
    const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
__device__ __forceinline__ void load4(const float *p, double (&v)[4])
{
    const float4 a = *reinterpret_cast<const float4 *>(p);
    v[0] = (double)a.x; v[1] = (double)a.y; v[2] = (double)a.z; v[3] = (double)a.w;
}

// C/D of the f64 MFMA: column lane & 15, row (lane >> 4) + 4 * register -- NOT the f32 16x16 map
template <typename WT, bool CONV>
__global__ __launch_bounds__(256) void gemm_f64_kernel(const GemmArgs a)
{
    __shared__ double As[2][BK][LDS_LD];
    __shared__ double Bs[2][BK][LDS_LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

    // what this thread stages: A row tid >> 2, B row likewise, k quarter tid & 3
    const int kq = tid & 3, srow = tid >> 2;
    const int row = m0 + srow;
    const bool aok = row < a.M;
    int ay = 0, ax = 0;
    const double *arow;
    if (CONV) {
        const int hw = a.h * a.w, b = aok ? row / hw : 0, p = aok ? row - b * hw : 0;
        ay = p / a.w;
        ax = p - ay * a.w;
        arow = a.X + (size_t)b * a.img_stride;
    } else {
        arow = a.X + (size_t)(aok ? row : 0) * a.ldx;
    }
    const bool bok = n0 + srow < a.N;
    const WT *brow = static_cast<const WT *>(a.W) + (size_t)(bok ? n0 + srow : 0) * a.ldw;

    double ra[4], rb[4];
    auto load_stage = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; j++) ra[j] = rb[j] = 0.0;
        if (CONV) {
            const int tap = k0 / a.Cin, c0 = k0 - tap * a.Cin;
            const int ys = ay + (tap / 3 - 1) * a.dil, xs = ax + (tap % 3 - 1) * a.dil;
            if (aok && ys >= 0 && ys < a.h && xs >= 0 && xs < a.w) load4(arow + (size_t)(ys * a.w + xs) * a.ldx + c0 + kq * 4, ra);
        } else if (aok) {
            load4(arow + k0 + kq * 4, ra);
        }
        if (bok) load4(brow + k0 + kq * 4, rb);
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            As[buf][kq * 4 + j][srow] = ra[j];
            Bs[buf][kq * 4 + j][srow] = rb[j];
        }
    };

    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[i][j][r] = 0.0;

    const int KT = a.K / BK;
    load_stage(0);
    store_stage(0);
    __syncthreads();
    const int am = wm * 32 + (lane & 15), bn = wn * 32 + (lane & 15), kh = lane >> 4;
    for (int kt = 0; kt < KT; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load_stage((kt + 1) * BK);
        // lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]: one step is k .. k + 3
#pragma unroll
        for (int kk = 0; kk < BK / 4; kk++) {
            double fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; i++) fa[i] = As[buf][4 * kk + kh][am + 16 * i];
#pragma unroll
            for (int j = 0; j < 2; j++) fb[j] = Bs[buf][4 * kk + kh][bn + 16 * j];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < KT) store_stage(buf ^ 1);       // (its last readers passed the barrier that closed stage kt - 1)
        __syncthreads();
    }

    const WT *bias = static_cast<const WT *>(a.bias);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int col = n0 + wn * 32 + 16 * j + (lane & 15);
            if (col >= a.N) continue;
            const double bv = (a.epi != F64_EPI_RELU && bias) ? (double)bias[col] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int orow = m0 + wm * 32 + 16 * i + (lane >> 4) + 4 * r;
                if (orow >= a.M) continue;
                double v = acc[i][j][r];
                if (a.epi == F64_EPI_RELU) {
                    v = fmax(v, 0.0);
                } else {
                    v = v + bv;
                    if (a.epi == F64_EPI_GELU) v = 0.5 * v * (1.0 + erf(v * 0.70710678118654752440));
                    else if (a.epi == F64_EPI_RESIDUAL) v = v + a.res[(size_t)orow * a.ldr + col];
                }
                a.Y[(size_t)orow * a.ldy + col] = v;
            }
        }
}

template <bool CONV>
int launch_gemm(const GemmArgs &a, bool w_f32, void *stream)
{
    const dim3 grid((a.M + BM - 1) / BM, (a.N + BN - 1) / BN);
    if (w_f32)
        hipLaunchKernelGGL((gemm_f64_kernel<float, CONV>), grid, dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL((gemm_f64_kernel<double, CONV>), grid, dim3(256), 0, as_stream(stream), a);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- attention --------------------------------------------------------------------------------------------------------------------------
// One block = 64 queries of one (batch, head) slice, 4 waves of 16 queries; key tiles of 16 through LDS.  On the MFMA, in the orientation that
// needs no lane movement between the two products (csrc/f32_kernels.hip, with the f64 MFMA's own C/D map):
//     S^T[key][query]  = K[key][d] Q^T[d][query]         A = K tile from LDS, B = Q held in 16 doubles;  steps of 4 over d
//     O^T[d][query]   += V^T[d][key] P^T[key][query]     B = the probabilities as the score accumulator holds them (register r of lane group
//                                                        g is key 4 r + g: step r of the second product), A = V tile from LDS
// A lane's column is its query in both results; the four lane groups hold different keys of the same query and meet in two exchanges.
constexpr int AQ = 64, AK = 16, HD = 64, K_LD = HD + 1, V_LD = HD + 2;

__global__ __launch_bounds__(256) void attn_fwd_f64_kernel(const double *__restrict__ qkv, double *__restrict__ out, int N, int H, double scale,
                                                           long long ldq, long long ldo)
{
    __shared__ double Ks[AK][K_LD];
    __shared__ double Vs[AK][V_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4;
    const int head = blockIdx.y, b = blockIdx.z;
    const double *base = qkv + (size_t)b * N * ldq;
    const double *qp = base + (size_t)head * HD, *kp = base + (size_t)(H + head) * HD, *vp = base + (size_t)(2 * H + head) * HD;
    const int query = blockIdx.x * AQ + wave * 16 + (lane & 15);

    double qreg[HD / 4];          // Q^T as the B operand: step s is d = 4 s + group
#pragma unroll
    for (int s = 0; s < HD / 4; s++) qreg[s] = query < N ? qp[(size_t)query * ldq + 4 * s + grp] : 0.0;

    f64x4 o[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[t][r] = 0.0;
    double m = -INFINITY, l = 0.0;

    // staging: thread -> key tid >> 4, d quarter-row (tid & 15) * 4; keys past N are zeros (their probability is an exact 0)
    double rk[4], rv[4];
    const int skey = tid >> 4, sd = (tid & 15) * 4;
    auto load_tile = [&](int key0) {
#pragma unroll
        for (int j = 0; j < 4; j++) rk[j] = rv[j] = 0.0;
        if (key0 + skey < N) {
            load4(kp + (size_t)(key0 + skey) * ldq + sd, rk);
            load4(vp + (size_t)(key0 + skey) * ldq + sd, rv);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            Ks[skey][sd + j] = rk[j];
            Vs[skey][sd + j] = rv[j];
        }
    };

    const int tiles = (N + AK - 1) / AK;
    load_tile(0);
    store_tile();
    __syncthreads();
    for (int kt = 0; kt < tiles; kt++) {
        if (kt + 1 < tiles) load_tile((kt + 1) * AK);
        f64x4 s;
#pragma unroll
        for (int r = 0; r < 4; r++) s[r] = 0.0;
#pragma unroll
        for (int st = 0; st < HD / 4; st++) s = __builtin_amdgcn_mfma_f64_16x16x4f64(Ks[lane & 15][4 * st + grp], qreg[st], s, 0, 0, 0);
        double mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int key = kt * AK + grp + 4 * r;
            s[r] = key < N ? s[r] * scale : -INFINITY;
            mx = fmax(mx, s[r]);
        }
        mx = fmax(mx, __shfl_xor(mx, 16, 64));
        mx = fmax(mx, __shfl_xor(mx, 32, 64));
        const double m_new = fmax(m, mx);           // finite from the first tile on: key 0 exists
        const double alpha = exp(m - m_new);        // (first tile: exp(-inf) = 0 on l = 0, o = 0)
        double psum = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            s[r] = exp(s[r] - m_new);
            psum += s[r];
        }
        l = l * alpha + psum;
        m = m_new;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) o[t][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int t = 0; t < 4; t++) o[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Vs[4 * r + grp][16 * t + (lane & 15)], s[r], o[t], 0, 0, 0);
        __syncthreads();
        if (kt + 1 < tiles) {
            store_tile();
            __syncthreads();
        }
    }
    l = l + __shfl_xor(l, 16, 64);
    l = l + __shfl_xor(l, 32, 64);
    const double inv = 1.0 / l;
    if (query < N) {
        double *op = out + ((size_t)b * N + query) * ldo + (size_t)head * HD;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) op[16 * t + grp + 4 * r] = o[t][r] * inv;          // register r of group g is d = 16 t + g + 4 r
    }
}

// ---- LayerNorm: one wavefront per row, sums by a fixed butterfly (the same value in every lane) ---------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void layernorm_f64_kernel(const double *__restrict__ x, const float *__restrict__ g, const float *__restrict__ bt,
                                                            double *__restrict__ y, int rows, int D, double eps)
{
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)rows) return;
    const double *xr = x + row * D;
    double s = 0.0;
    for (int i = lane; i < D; i += 64) s += xr[i];
    const double mean = wave_sum(s) / (double)D;
    double q = 0.0;
    for (int i = lane; i < D; i += 64) {
        const double d = xr[i] - mean;
        q += d * d;
    }
    const double rstd = 1.0 / sqrt(wave_sum(q) / (double)D + eps);
    double *yr = y + row * D;
    for (int i = lane; i < D; i += 64) yr[i] = (xr[i] - mean) * rstd * (double)g[i] + (double)bt[i];
}

// ---- token-shaped float64 im2col (csrc/f32_kernels.hip: im2col_flip_f32_kernel on float64 images): a selection, exact ---------------------
__global__ __launch_bounds__(256) void im2col_flip_f64_kernel(const double *__restrict__ x, double *__restrict__ rows, int B, int C, int H, int W, int P,
                                                              int flips, int cls_rows)
{
    const int h = H / P, w = W / P, KC = C * P * P, K4 = KC / 4;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)flips * B * h * w * K4;
    if (e >= total) return;
    const int k = (int)(e % K4) * 4;
    const size_t row_id = e / K4;
    size_t row = row_id;
    const int px = (int)(row % w);
    row /= w;
    const int py = (int)(row % h);
    row /= h;
    const int b = (int)(row % B), f = (int)(row / B);
    const int c = k / (P * P), dy = (k - c * P * P) / P, dx = k % P;          // P % 4 == 0: the 4 elements share (c, dy)
    const double *src = x + (((size_t)b * C + c) * H + (size_t)P * py + dy) * W;
    const int x0 = P * px + dx;
    const size_t out_row = row_id + (size_t)cls_rows * ((size_t)(f * B + b) + 1);
    double *dst = rows + out_row * (size_t)KC + k;
#pragma unroll
    for (int j = 0; j < 4; j++) dst[j] = f ? src[W - 1 - (x0 + j)] : src[x0 + j];
}

// ---- the float64 tail of multi_scale_camseg -----------------------------------------------------------------------------------------------
// F.interpolate(x.double(), size=(OH, OW), mode="bilinear", align_corners=False): ATen's formula as csrc/label_kernels.hip states it, in double
__global__ __launch_bounds__(256) void resize_bilinear_f64_kernel(const float *__restrict__ src, double *__restrict__ dst, int planes, int H, int W,
                                                                  int OH, int OW, double rh, double rw)
{
    const size_t n = (size_t)planes * OH * OW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
        const size_t pl = i / ((size_t)OW * OH);
        double h1r = __builtin_fma(rh, (double)oy + 0.5, -0.5);
        h1r = h1r < 0.0 ? 0.0 : h1r;
        double w1r = __builtin_fma(rw, (double)ox + 0.5, -0.5);
        w1r = w1r < 0.0 ? 0.0 : w1r;
        int h1 = (int)h1r, w1 = (int)w1r;
        h1 = h1 > H - 1 ? H - 1 : h1;
        w1 = w1 > W - 1 ? W - 1 : w1;
        const int h1p = h1 < H - 1 ? 1 : 0, w1p = w1 < W - 1 ? 1 : 0;
        const double h1l = h1r - (double)h1, h0l = 1.0 - h1l, w1l = w1r - (double)w1, w0l = 1.0 - w1l;
        const float *p = src + pl * (size_t)H * W + (size_t)h1 * W + w1;
        const double top = __builtin_fma(w0l, (double)p[0], w1l * (double)p[w1p]);
        const double bot = __builtin_fma(w0l, (double)p[(size_t)h1p * W], w1l * (double)p[(size_t)h1p * W + w1p]);
        dst[i] = __builtin_fma(h0l, top, h1l * bot);
    }
}

__device__ __forceinline__ void src_index64(int dst, int in, int out, double scale, int &i0, int &i1, double &l0, double &l1)
{
    if (in == out) { i0 = dst; i1 = dst < in - 1 ? dst + 1 : dst; l0 = 1.0; l1 = 0.0; return; }
    double src = scale * ((double)dst + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    int i = (int)src;
    if (i > in - 1) i = in - 1;
    i0 = i;
    i1 = i < in - 1 ? i + 1 : i;
    l1 = src - (double)i;
    l0 = 1.0 - l1;
}

__device__ __forceinline__ double bilerp64(double p00, double p01, double p10, double p11, double lx0, double lx1, double ly0, double ly1)
{
    const double r0 = __builtin_fma(p00, lx0, p01 * lx1);
    const double r1 = __builtin_fma(p10, lx0, p11 * lx1);
    return __builtin_fma(r0, ly0, r1 * ly1);
}

// thread per output pixel, grid (pixel blocks, images), the class planes a loop inside (csrc/label_kernels.hip: flip_merge_upsample_kernel)
__global__ __launch_bounds__(256) void flip_merge_upsample_f64_kernel(const double *__restrict__ src, double *__restrict__ dst, int B, int C, int h,
                                                                      int w, int S, double sy, double sx, int mode, int accumulate,
                                                                      const float *__restrict__ active)
{
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (pix >= S * S) return;
    const int Y = pix / S, X = pix - Y * S;
    int y0, y1, x0, x1, fx0, fx1;
    double ly0, ly1, lx0, lx1, flx0, flx1;
    src_index64(Y, h, S, sy, y0, y1, ly0, ly1);
    src_index64(X, w, S, sx, x0, x1, lx0, lx1);
    src_index64(S - 1 - X, w, S, sx, fx0, fx1, flx0, flx1);
    for (int c = 0; c < C; c++) {
        const size_t o = ((size_t)b * C + c) * S * S + pix;
        if (active && active[b * C + c] == 0.0f) {
            if (!accumulate) dst[o] = 0.0;
            continue;
        }
        const double *p = src + ((size_t)b * C + c) * h * w;
        const double *q = src + ((size_t)(b + B) * C + c) * h * w;
        const double u1 = bilerp64(p[y0 * w + x0], p[y0 * w + x1], p[y1 * w + x0], p[y1 * w + x1], lx0, lx1, ly0, ly1);
        const double u2 = bilerp64(q[y0 * w + fx0], q[y0 * w + fx1], q[y1 * w + fx0], q[y1 * w + fx1], flx0, flx1, ly0, ly1);
        double v;
        if (mode == 0) { v = fmax(u1, u2); v = v > 0.0 ? v : 0.0; }
        else v = u1 + u2;
        dst[o] = accumulate ? dst[o] + v : v;
    }
}

template <int NT>
__device__ __forceinline__ double block_max(double v, double *sh)
{
    v = wave_max(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wid] = v;
    __syncthreads();
    double r = sh[0];
#pragma unroll
    for (int i = 1; i < NT / 64; i++) r = fmax(r, sh[i]);
    return r;
}

// rawmax[b, c] (+)= max |logit| over the plane and its mirror image's plane: one workgroup per (b, c), inactive planes included (no flag read:
// the figure is defined for every plane)
__global__ __launch_bounds__(256) void rawmax_f64_kernel(const double *__restrict__ src, double *__restrict__ rawmax, int B, int C, int hw, int accumulate)
{
    __shared__ double sh[4];
    const int c = blockIdx.x, b = blockIdx.y;
    const double *p = src + ((size_t)b * C + c) * hw, *q = src + ((size_t)(b + B) * C + c) * hw;
    double mx = 0.0;
    for (int i = threadIdx.x; i < hw; i += 256) mx = fmax(mx, fmax(fabs(p[i]), fabs(q[i])));
    mx = block_max<256>(mx, sh);
    if (threadIdx.x == 0) rawmax[b * C + c] = accumulate ? rawmax[b * C + c] + mx : mx;
}

// one workgroup per (b, c) plane: x = (x - min) / (max(x - min) + 1e-5) in place; peak[plane] = that divisor
__global__ __launch_bounds__(256) void minmax_norm_f64_kernel(double *__restrict__ cam, int HW, const float *__restrict__ active, double *__restrict__ peak)
{
    __shared__ double sh[4];
    if (active && active[blockIdx.x] == 0.0f) return;   // all-zero plane stays all-zero
    double *x = cam + (size_t)blockIdx.x * HW;
    double mneg = -INFINITY;
    for (int i = threadIdx.x; i < HW; i += 256) mneg = fmax(mneg, -x[i]);
    mneg = block_max<256>(mneg, sh);
    double mx = -INFINITY;
    for (int i = threadIdx.x; i < HW; i += 256) mx = fmax(mx, x[i] + mneg);
    mx = block_max<256>(mx, sh);
    const double den = mx + 1e-5;
    for (int i = threadIdx.x; i < HW; i += 256) x[i] = (x[i] + mneg) / den;
    if (peak && threadIdx.x == 0) peak[blockIdx.x] = den;
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_gemm_f64(const double *X, const void *W, const void *bias, const double *residual, double *Y, int M, int N, int K, int ldx,
                             int ldw, int ldr, int ldy, int epilogue, int w_is_f32, void *stream)
{
    COSA_REQUIRE(X && W && Y, "cosa_gemm_f64: null operand");
    COSA_REQUIRE(M >= 1 && N >= 1 && K >= 16 && K % 16 == 0, "cosa_gemm_f64: M >= 1, N >= 1, K %% 16 == 0 (got M=%d N=%d K=%d)", M, N, K);
    COSA_REQUIRE(ldx >= K && ldx % 2 == 0 && ldw >= K && ldw % (w_is_f32 ? 4 : 2) == 0 && ldy >= N && aligned16(X) && aligned16(W),
                 "cosa_gemm_f64: row strides must cover the rows, those of X and W in multiples of 16 bytes on 16-byte aligned bases");
    COSA_REQUIRE(epilogue == F64_EPI_BIAS || epilogue == F64_EPI_GELU || epilogue == F64_EPI_RESIDUAL, "cosa_gemm_f64: epilogue 0 | 1 | 2");
    COSA_REQUIRE(epilogue != F64_EPI_RESIDUAL || (residual && ldr >= N), "cosa_gemm_f64: the residual epilogue needs a residual of row stride >= N");
    COSA_REQUIRE((N + BN - 1) / BN <= 65535, "cosa_gemm_f64: too many columns for one launch");
    GemmArgs a{X, W, bias, residual, Y, M, N, K, ldx, ldw, ldr, ldy, epilogue, 0, 0, 0, 0, 0};
    return launch_gemm<false>(a, w_is_f32 != 0, stream);
}

extern "C" int cosa_conv3x3_dilated_f64(const double *tok, const void *Wt, double *Y, int B, int h, int w, int Cin, int Cout, int dilation,
                                        int img_rows, int ldx, int relu, int w_is_f32, void *stream)
{
    COSA_REQUIRE(tok && Wt && Y, "cosa_conv3x3_dilated_f64: null operand");
    COSA_REQUIRE(B >= 1 && h >= 1 && w >= 1 && dilation >= 1 && Cin >= 16 && Cin % 16 == 0 && Cout >= 1,
                 "cosa_conv3x3_dilated_f64: Cin %% 16 == 0 (got B=%d h=%d w=%d Cin=%d Cout=%d d=%d)", B, h, w, Cin, Cout, dilation);
    COSA_REQUIRE(ldx >= Cin && ldx % 2 == 0 && img_rows >= h * w && aligned16(tok) && aligned16(Wt),
                 "cosa_conv3x3_dilated_f64: pixel rows of stride ldx >= Cin in multiples of 2, images of >= h*w rows, 16-byte aligned bases");
    COSA_REQUIRE((long long)B * h * w <= 0x7fffffffll / 2 && (Cout + BN - 1) / BN <= 65535 && Cin <= 0x7fffffff / 9,
                 "cosa_conv3x3_dilated_f64: too many pixels / channels for one launch");
    GemmArgs a{tok, Wt, nullptr, nullptr, Y, B * h * w, Cout, 9 * Cin, ldx, 9 * Cin, 0, Cout, relu ? F64_EPI_RELU : F64_EPI_BIAS,
               h, w, Cin, dilation, (long long)img_rows * ldx};
    return launch_gemm<true>(a, w_is_f32 != 0, stream);
}

extern "C" int cosa_attn_fwd_f64(const double *qkv, double *out, int B, int N, int H, int head_dim, double scale, int ldq, int ldo, void *stream)
{
    COSA_REQUIRE(qkv && out, "cosa_attn_fwd_f64: null operand");
    COSA_REQUIRE(B >= 1 && N >= 1 && H >= 1 && head_dim == HD, "cosa_attn_fwd_f64: head_dim must be 64 (got B=%d N=%d H=%d d=%d)", B, N, H, head_dim);
    COSA_REQUIRE(ldq >= 3 * H * HD && ldq % 2 == 0 && ldo >= H * HD && aligned16(qkv),
                 "cosa_attn_fwd_f64: token rows of stride ldq >= 3*H*64 (even) / ldo >= H*64, 16-byte aligned qkv");
    COSA_REQUIRE(H <= 65535 && B <= 65535, "cosa_attn_fwd_f64: too many heads / images for one launch");
    hipLaunchKernelGGL(attn_fwd_f64_kernel, dim3((N + AQ - 1) / AQ, H, B), dim3(256), 0, as_stream(stream), qkv, out, N, H, scale, (long long)ldq,
                       (long long)ldo);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_layernorm_f64(const double *x, const float *gamma, const float *beta, double *y, int rows, int dim, double eps, void *stream)
{
    COSA_REQUIRE(x && gamma && beta && y && rows >= 1 && dim >= 1, "cosa_layernorm_f64: bad arguments");
    hipLaunchKernelGGL(layernorm_f64_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, as_stream(stream), x, gamma, beta, y, rows, dim, eps);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_im2col_flip_f64_tokens(const double *x, double *rows, int B, int C, int H, int W, int P, int flips, int cls_rows, void *stream)
{
    COSA_REQUIRE(x && rows && B > 0 && C > 0 && H > 0 && W > 0 && P > 0 && cls_rows >= 0, "cosa_im2col_flip_f64_tokens: bad arguments");
    COSA_REQUIRE(P % 4 == 0 && H % P == 0 && W % P == 0,
                 "cosa_im2col_flip_f64_tokens: patch size must be a multiple of 4 and divide H and W (got P=%d H=%d W=%d)", P, H, W);
    COSA_REQUIRE(flips == 1 || flips == 2, "cosa_im2col_flip_f64_tokens: flips 1 | 2");
    const size_t total = (size_t)flips * B * (H / P) * (W / P) * (C * P * P / 4);
    COSA_REQUIRE(total / 256 < 0x7fffffffull, "cosa_im2col_flip_f64_tokens: too many elements for one launch");
    hipLaunchKernelGGL(im2col_flip_f64_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x, rows, B, C, H, W, P, flips,
                       cls_rows);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_resize_bilinear_f64(const float *src, double *dst, int planes, int H, int W, int OH, int OW, void *stream)
{
    COSA_REQUIRE(src && dst && planes > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "cosa_resize_bilinear_f64: bad arguments");
    const size_t n = (size_t)planes * OH * OW;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(resize_bilinear_f64_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), src, dst, planes, H, W, OH, OW,
                       (double)H / (double)OH, (double)W / (double)OW);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

// rawmax ([B*C] or NULL): (+)= per plane max over the plane and its mirror image of |src|, accumulated like dst
extern "C" int cosa_cam_flip_merge_upsample_f64(const double *src, double *dst, int B, int C, int h, int w, int S, int mode, int accumulate,
                                                const float *active, double *rawmax, void *stream)
{
    COSA_REQUIRE(src && dst && B > 0 && C > 0 && h > 0 && w > 0 && S > 0, "cosa_cam_flip_merge_upsample_f64: bad arguments");
    COSA_REQUIRE(mode == 0 || mode == 1, "cosa_cam_flip_merge_upsample_f64: mode must be 0 or 1");
    COSA_REQUIRE(C <= 65535 && B <= 65535 && S <= 46340, "cosa_cam_flip_merge_upsample_f64: grid too large");
    hipLaunchKernelGGL(flip_merge_upsample_f64_kernel, dim3((S * S + 255) / 256, B), dim3(256), 0, as_stream(stream), src, dst, B, C, h, w, S,
                       (double)h / (double)S, (double)w / (double)S, mode, accumulate, active);
    COSA_LAUNCH_CHECK();
    if (rawmax) {
        hipLaunchKernelGGL(rawmax_f64_kernel, dim3(C, B), dim3(256), 0, as_stream(stream), src, rawmax, B, C, h * w, accumulate);
        COSA_LAUNCH_CHECK();
    }
    return COSA_OK;
}

extern "C" int cosa_cam_minmax_norm_f64(double *cam, int BC, int HW, const float *active, double *peak, void *stream)
{
    COSA_REQUIRE(cam && BC > 0 && HW > 0, "cosa_cam_minmax_norm_f64: bad arguments");
    hipLaunchKernelGGL(minmax_norm_f64_kernel, dim3(BC), dim3(256), 0, as_stream(stream), cam, HW, active, peak);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
