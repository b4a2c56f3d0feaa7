// f32_kernels.hip -- the "f32" operand family of the no-grad passes: every operand fp32, every product on the exact f32-input MFMA
// (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, one rounding per product, no wider internal accumulation).  Teacher mode
// string "fp32" (DESIGN.md section 16): the reference's arithmetic on the device, for checks and for users who ask for it -- 1/16 of the
// 16-bit MFMA rate, so not the headline path.
//
//   cosa_gemm_f32              Y[M,N] = X[M,K] W[N,K]^T, epilogues +bias | +bias, erf-GELU | +bias +residual (fp32, in place allowed)
//   cosa_conv3x3_dilated_f32   LargeFOV conv6 / conv7 (3x3, dilation d, zero padding d, no bias, ReLU) as an implicit GEMM over the NHWC tokens:
//                              the same kernel, its A rows gathered per tap
//   cosa_attn_fwd_f32          softmax(q k^T * scale) v on the packed fp32 qkv rows, flash style, nothing of size N^2 leaves the CU
//   cosa_im2col_flip_f32_tokens  the token-shaped fp32 operand of the patch projection (images and their mirror images)
//
// Numerics contract of the GEMM (and of the conv): every output element is ONE fma chain over ascending k starting from zero -- the MFMA's
// accumulator is the only sum there is: no split-K, no atomics, the same chain whatever M is, wherever the row sits and whatever the other
// rows hold.  The epilogue follows in fp32.  This translation unit is built with -ffp-contract=off: what is an fma here is written fmaf.
#include "kernels.hpp"
#include "f32_attn_tile.hpp"      // f32x16, cd_row; the QK^T half of the attention kernel

namespace cosa {
namespace {

constexpr int BM = 128;        // block tile rows
constexpr int BK = 16;         // k per LDS stage (K % 16 == 0: 192 = 12 stages; a conv tap's Cin is a multiple, so a stage never straddles taps)
constexpr int LDS_PAD = 4;     // row stride BM + 4 words: the transposing stores of a wave hit 64 different banks

enum { F32_EPI_BIAS = 0, F32_EPI_GELU = 1, F32_EPI_RESIDUAL = 2, F32_EPI_RELU = 3 };

struct GemmArgs {
    const float *X, *W, *bias, *res;
    float *Y;
    int M, N, K, ldx, ldw, ldr, ldy, epi;
    // implicit-GEMM conv (CONV): X is the token matrix, image b at X + b * img_stride, pixel rows of stride ldx; K = 9 * Cin
    int h, w, Cin, dil;
    long long img_stride;
};

// BN: 128 (2 x 2 waves, 2 x 2 tiles of 32 x 32 each) when N % 128 == 0, else 64 (4 x 1 waves, 1 x 2 tiles).  The tile shape moves no bit:
// an element's chain is over k alone.
template <int BN, bool CONV>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const GemmArgs a)
{
    constexpr int WAVES_N = BN / 64, WAVES_M = 4 / WAVES_N, TM = BM / (WAVES_M * 32), TN = 2;
    constexpr int A_LD = BM + LDS_PAD, B_LD = BN + LDS_PAD;
    constexpr int A_PER = BM * BK / 4 / 256, B_PER = BN * BK / 4 / 256;          // float4 loads per thread and stage
    __shared__ float As[2][BK][A_LD];
    __shared__ float Bs[2][BK][B_LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;

    // what this thread stages: A rows (tid + 256 i) >> 2, B rows likewise, k quarter tid & 3
    const int kq = tid & 3;
    const float *arow[A_PER];
    int ay[A_PER], ax[A_PER];
    bool aok[A_PER];
#pragma unroll
    for (int i = 0; i < A_PER; i++) {
        const int row = m0 + ((tid + 256 * i) >> 2);
        aok[i] = row < a.M;
        ay[i] = ax[i] = 0;
        if (CONV) {
            const int hw = a.h * a.w, b = row / hw, p = row - b * hw;
            ay[i] = p / a.w;
            ax[i] = p - ay[i] * a.w;
            arow[i] = a.X + (size_t)b * a.img_stride;
        } else {
            arow[i] = a.X + (size_t)row * a.ldx;
        }
    }
    const float *brow[B_PER];
#pragma unroll
    for (int i = 0; i < B_PER; i++) brow[i] = a.W + (size_t)(n0 + ((tid + 256 * i) >> 2)) * a.ldw;

    float4 ra[A_PER], rb[B_PER];
    auto load_stage = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_PER; i++) {
            ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (CONV) {
                const int tap = k0 / a.Cin, c0 = k0 - tap * a.Cin;
                const int ys = ay[i] + (tap / 3 - 1) * a.dil, xs = ax[i] + (tap % 3 - 1) * a.dil;
                if (aok[i] && ys >= 0 && ys < a.h && xs >= 0 && xs < a.w)
                    ra[i] = *reinterpret_cast<const float4 *>(arow[i] + (size_t)(ys * a.w + xs) * a.ldx + c0 + kq * 4);
            } else if (aok[i]) {
                ra[i] = *reinterpret_cast<const float4 *>(arow[i] + k0 + kq * 4);
            }
        }
#pragma unroll
        for (int i = 0; i < B_PER; i++) rb[i] = *reinterpret_cast<const float4 *>(brow[i] + k0 + kq * 4);
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_PER; i++) {
            const int r = (tid + 256 * i) >> 2;
            As[buf][kq * 4 + 0][r] = ra[i].x; As[buf][kq * 4 + 1][r] = ra[i].y; As[buf][kq * 4 + 2][r] = ra[i].z; As[buf][kq * 4 + 3][r] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < B_PER; i++) {
            const int r = (tid + 256 * i) >> 2;
            Bs[buf][kq * 4 + 0][r] = rb[i].x; Bs[buf][kq * 4 + 1][r] = rb[i].y; Bs[buf][kq * 4 + 2][r] = rb[i].z; Bs[buf][kq * 4 + 3][r] = rb[i].w;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int KT = a.K / BK;
    load_stage(0);
    store_stage(0);
    __syncthreads();
    const int am = wm * (TM * 32) + (lane & 31), bn = wn * (TN * 32) + (lane & 31), kh = lane >> 5;
    for (int kt = 0; kt < KT; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load_stage((kt + 1) * BK);
        // lane l feeds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]: one step is k, k + 1 in that order
#pragma unroll
        for (int kk = 0; kk < BK / 2; kk++) {
            float fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; i++) fa[i] = As[buf][2 * kk + kh][am + 32 * i];
#pragma unroll
            for (int j = 0; j < TN; j++) fb[j] = Bs[buf][2 * kk + kh][bn + 32 * j];
#pragma unroll
            for (int i = 0; i < TM; i++)
#pragma unroll
                for (int j = 0; j < TN; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < KT) store_stage(buf ^ 1);       // (its last readers passed the barrier that closed stage kt - 1)
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const int col = n0 + wn * (TN * 32) + 32 * j + (lane & 31);
            const float bv = (a.epi != F32_EPI_RELU && a.bias) ? a.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = m0 + wm * (TM * 32) + 32 * i + cd_row(r, lane);
                if (row >= a.M) continue;
                float v = acc[i][j][r];
                if (a.epi == F32_EPI_RELU) {
                    v = fmaxf(v, 0.f);
                } else {
                    v = v + bv;
                    if (a.epi == F32_EPI_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
                    else if (a.epi == F32_EPI_RESIDUAL) v = v + a.res[(size_t)row * a.ldr + col];
                }
                a.Y[(size_t)row * a.ldy + col] = v;
            }
        }
}

template <bool CONV>
int launch_gemm(const GemmArgs &a, void *stream)
{
    const dim3 grid128(a.N / 128, (a.M + BM - 1) / BM), grid64(a.N / 64, (a.M + BM - 1) / BM);
    if (a.N % 128 == 0)
        hipLaunchKernelGGL((gemm_f32_kernel<128, CONV>), grid128, dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL((gemm_f32_kernel<64, CONV>), grid64, dim3(256), 0, as_stream(stream), a);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- attention --------------------------------------------------------------------------------------------------------------------------
// One block = 128 queries of one (batch, head) slice, 4 waves of 32 queries; key tiles of 32 through LDS.  On the MFMA, in the orientation
// that needs no lane movement between the two products:
//     S^T[key][query]  = K[key][d] Q^T[d][query]         A = K tile from LDS, B = Q held in 32 VGPRs;  the chain over d ascends
//     O^T[d][query]   += V^T[d][key] P^T[key][query]     B = the probabilities as the score accumulators hold them, A = V tile from LDS
// A lane's column is its query in both results, so the running maximum, the rescale and the row sum are per lane; the two lane halves hold
// different keys of the same query and meet in one exchange per tile.  exp is expf (no exp2 folding, no fast variant).
constexpr int V_LD = HD + 4;          // (AQ, AK, HD, K_LD: f32_attn_tile.hpp)

__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(const float *__restrict__ qkv, float *__restrict__ out, int N, int H, float scale,
                                                           long long ldq, long long ldo)
{
    __shared__ float Ks[AK][K_LD];
    __shared__ float Vs[AK][V_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const float *base = qkv + (size_t)b * N * ldq;
    const float *qp = base + (size_t)head * HD, *kp = base + (size_t)(H + head) * HD, *vp = base + (size_t)(2 * H + head) * HD;
    const int query = blockIdx.x * AQ + wave * 32 + (lane & 31);

    float qreg[HD / 2];
    attn_load_q(qp, query, N, ldq, half, qreg);

    f32x16 o[2];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[t][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    // staging: keys past N are zeros (their probability is an exact 0)
    float4 rk[2], rv[2];
    auto load_tile = [&](int key0) {
        attn_load_rows(kp, key0, N, ldq, tid, rk);
        attn_load_rows(vp, key0, N, ldq, tid, rv);
    };
    auto store_tile = [&]() {
        attn_store_k(Ks, tid, rk);
#pragma unroll
        for (int i = 0; i < 2; i++) *reinterpret_cast<float4 *>(&Vs[(tid + 256 * i) >> 4][(tid & 15) * 4]) = rv[i];
    };

    const int tiles = (N + AK - 1) / AK;
    load_tile(0);
    store_tile();
    __syncthreads();
    for (int kt = 0; kt < tiles; kt++) {
        if (kt + 1 < tiles) load_tile((kt + 1) * AK);
        f32x16 s = attn_scores(Ks, qreg, lane);
        const float mx = attn_mask_max(s, kt * AK, N, scale, lane);
        const float m_new = fmaxf(m, mx);            // finite from the first tile on: key 0 exists
        const float alpha = expf(m - m_new);         // (first tile: expf(-inf) = 0 on l = 0, o = 0)
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            s[r] = expf(s[r] - m_new);
            psum += s[r];
        }
        l = fmaf(l, alpha, psum);
        m = m_new;
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[t][r] *= alpha;
        // step r sums the two keys the lane halves hold in register r: (r & 3) + 8 (r >> 2) and that + 4
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int key = cd_row(r, lane);
#pragma unroll
            for (int t = 0; t < 2; t++) o[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key][32 * t + (lane & 31)], s[r], o[t], 0, 0, 0);
        }
        __syncthreads();
        if (kt + 1 < tiles) {
            store_tile();
            __syncthreads();
        }
    }
    const float inv = 1.0f / (l + __shfl_xor(l, 32, 64));
    if (query < N) {
        float *op = out + ((size_t)b * N + query) * ldo + (size_t)head * HD;
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int g = 0; g < 4; g++)          // registers 4g .. 4g + 3 are d = 32 t + 8 g + 4 half + (0 .. 3)
                *reinterpret_cast<float4 *>(op + 32 * t + 8 * g + 4 * half) =
                    make_float4(o[t][4 * g] * inv, o[t][4 * g + 1] * inv, o[t][4 * g + 2] * inv, o[t][4 * g + 3] * inv);
    }
}

// ---- token-shaped fp32 im2col (the f32 analogue of split_kernels.hip: im2col_flip_split_kernel): the row of patch (f, b, py, px) is
//     cols[c*P*P + dy*P + dx] = x[b][c][P*py + dy][f ? W-1-(P*px+dx) : P*px+dx]
// at token row (f*B + b) * (h*w + cls_rows) + cls_rows + py*w + px; the class-token rows in between are not touched (zero for good)
__global__ __launch_bounds__(256) void im2col_flip_f32_kernel(const float *__restrict__ x, float *__restrict__ rows, int B, int C, int H, int W, int P,
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
    const float *src = x + (((size_t)b * C + c) * H + (size_t)P * py + dy) * W;
    const int x0 = P * px + dx;
    float4 v;
    if (!f) {
        v = *reinterpret_cast<const float4 *>(src + x0);
    } else {
        const float4 t = *reinterpret_cast<const float4 *>(src + (W - 4 - x0));          // source columns W-4-x0 .. W-1-x0, reversed
        v = make_float4(t.w, t.z, t.y, t.x);
    }
    const size_t out_row = row_id + (size_t)cls_rows * ((size_t)(f * B + b) + 1);
    *reinterpret_cast<float4 *>(rows + out_row * (size_t)KC + k) = v;
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_gemm_f32(const float *X, const float *W, const float *bias, const float *residual, float *Y, int M, int N, int K, int ldx,
                             int ldw, int ldr, int ldy, int epilogue, void *stream)
{
    COSA_REQUIRE(X && W && Y, "cosa_gemm_f32: null operand");
    COSA_REQUIRE(M >= 1 && N >= 64 && N % 64 == 0 && K >= 16 && K % 16 == 0, "cosa_gemm_f32: M >= 1, N %% 64 == 0, K %% 16 == 0 (got M=%d N=%d K=%d)", M,
                 N, K);
    COSA_REQUIRE(ldx >= K && ldx % 4 == 0 && ldw >= K && ldw % 4 == 0 && ldy >= N && aligned16(X) && aligned16(W),
                 "cosa_gemm_f32: row strides must cover the rows, those of X and W in multiples of 4 on 16-byte aligned bases");
    COSA_REQUIRE(epilogue == F32_EPI_BIAS || epilogue == F32_EPI_GELU || epilogue == F32_EPI_RESIDUAL, "cosa_gemm_f32: epilogue 0 | 1 | 2");
    COSA_REQUIRE(epilogue != F32_EPI_RESIDUAL || (residual && ldr >= N), "cosa_gemm_f32: the residual epilogue needs a residual of row stride >= N");
    COSA_REQUIRE((M + BM - 1) / BM <= 65535, "cosa_gemm_f32: too many rows for one launch");
    GemmArgs a{X, W, bias, residual, Y, M, N, K, ldx, ldw, ldr, ldy, epilogue, 0, 0, 0, 0, 0};
    return launch_gemm<false>(a, stream);
}

extern "C" int cosa_conv3x3_dilated_f32(const float *tok, const float *Wt, float *Y, int B, int h, int w, int Cin, int Cout, int dilation,
                                        int img_rows, int ldx, int relu, void *stream)
{
    COSA_REQUIRE(tok && Wt && Y, "cosa_conv3x3_dilated_f32: null operand");
    COSA_REQUIRE(B >= 1 && h >= 1 && w >= 1 && dilation >= 1 && Cin >= 16 && Cin % 16 == 0 && Cout >= 64 && Cout % 64 == 0,
                 "cosa_conv3x3_dilated_f32: Cin %% 16 == 0, Cout %% 64 == 0 (got B=%d h=%d w=%d Cin=%d Cout=%d d=%d)", B, h, w, Cin, Cout, dilation);
    COSA_REQUIRE(ldx >= Cin && ldx % 4 == 0 && img_rows >= h * w && aligned16(tok) && aligned16(Wt),
                 "cosa_conv3x3_dilated_f32: pixel rows of stride ldx >= Cin in multiples of 4, images of >= h*w rows, 16-byte aligned bases");
    COSA_REQUIRE((long long)B * h * w <= 65535ll * BM, "cosa_conv3x3_dilated_f32: too many pixels for one launch");
    GemmArgs a{tok, Wt, nullptr, nullptr, Y, B * h * w, Cout, 9 * Cin, ldx, 9 * Cin, 0, Cout, relu ? F32_EPI_RELU : F32_EPI_BIAS,
               h, w, Cin, dilation, (long long)img_rows * ldx};
    return launch_gemm<true>(a, stream);
}

extern "C" int cosa_attn_fwd_f32(const float *qkv, float *out, int B, int N, int H, int head_dim, float scale, int ldq, int ldo, void *stream)
{
    COSA_REQUIRE(qkv && out, "cosa_attn_fwd_f32: null operand");
    COSA_REQUIRE(B >= 1 && N >= 1 && H >= 1 && head_dim == HD, "cosa_attn_fwd_f32: head_dim must be 64 (got B=%d N=%d H=%d d=%d)", B, N, H, head_dim);
    COSA_REQUIRE(ldq >= 3 * H * HD && ldq % 4 == 0 && ldo >= H * HD && ldo % 4 == 0 && aligned16(qkv) && aligned16(out),
                 "cosa_attn_fwd_f32: token rows of stride ldq >= 3*H*64 / ldo >= H*64 in multiples of 4, 16-byte aligned bases");
    COSA_REQUIRE(H <= 65535 && B <= 65535, "cosa_attn_fwd_f32: too many heads / images for one launch");
    hipLaunchKernelGGL(attn_fwd_f32_kernel, dim3((N + AQ - 1) / AQ, H, B), dim3(256), 0, as_stream(stream), qkv, out, N, H, scale, (long long)ldq,
                       (long long)ldo);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_im2col_flip_f32_tokens(const float *x, float *rows, int B, int C, int H, int W, int P, int flips, int cls_rows, void *stream)
{
    COSA_REQUIRE(x && rows && B > 0 && C > 0 && H > 0 && W > 0 && P > 0 && cls_rows >= 0, "cosa_im2col_flip_f32_tokens: bad arguments");
    COSA_REQUIRE(P % 4 == 0 && H % P == 0 && W % P == 0 && aligned16(x) && aligned16(rows),
                 "cosa_im2col_flip_f32_tokens: patch size must be a multiple of 4 and divide H and W (got P=%d H=%d W=%d)", P, H, W);
    COSA_REQUIRE(flips == 1 || flips == 2, "cosa_im2col_flip_f32_tokens: flips 1 | 2");
    const size_t total = (size_t)flips * B * (H / P) * (W / P) * (C * P * P / 4);
    COSA_REQUIRE(total / 256 < 0x7fffffffull, "cosa_im2col_flip_f32_tokens: too many elements for one launch");
    hipLaunchKernelGGL(im2col_flip_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x, rows, B, C, H, W, P, flips,
                       cls_rows);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
