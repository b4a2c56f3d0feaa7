// tokcon_kernels.hip -- the supervised-contrastive token loss on the student's final patch tokens: this project's own
// objective, the form of Khosla et al. 2020 over the step's pseudo labels; the reference has no code for it.
//
//   cosa_token_labels          label map [B,S,S] -> one byte per token: the class that holds >= need of the cell's p x p pixels, else 255
//   cosa_token_contrast_fwd    L = (1/M) sum_anchors (lse_i - possum_i / |P(i)|), per image, with lse / possum / counts / M kept for the backward
//   cosa_token_contrast_bwd    dL/dx (bf16) from them: W = G + G^T per image into scratch, dZ = W Z, the normalisation's backward per row
//   cosa_token_junction_bwd4   the heads' junction for four live bf16 gradients (decoder, CAM head, classification head, feature map)
//
// Arithmetic: tokens widened to fp32 and normalised once (z = x / max(|x|, 1e-12)); every product on the exact f32-input MFMA
// (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, as csrc/f32_kernels.hip); s = chain / tau; the log-sum-exp over the keys is online, tile by
// tile in ascending key order; the batch sum is one workgroup's strided double sums met in a fixed tree.  No float atomics anywhere: the same
// input gives the same bytes on every run.  Built with -ffp-contract=off.
#include "kernels.hpp"
#include "f32_attn_tile.hpp"      // f32x16, cd_row

namespace cosa {
namespace {

constexpr int TD = 768;            // token width (ViT-B)
constexpr int TB = 128;            // tile edge: 128 A rows x 128 B columns per workgroup, 4 waves of 128 x 32
constexpr int TK = 16;             // k per LDS stage
constexpr int T_LD = TB + 4;       // row stride of a stage (f32_kernels.hip: LDS_PAD)
constexpr int TIGN = 255;
constexpr int TMAXN = 4096;
constexpr size_t kScratchCap = 256ull << 20;

struct __attribute__((aligned(16))) TileLds {
    float A[2][TK][T_LD];
    float B[2][TK][T_LD];
};

// acc[t][r] = sum_k A[32 t + cd_row(r, lane)][k] * Bm[wave * 32 + (lane & 31)][k], k ascending from 0 (acc zeroed here).
//   A: rows of stride lda, k contiguous; rows >= a_rows are zeros.
//   B_KROWS false: B like A (b_rows valid rows).  true: B[k][column], columns contiguous, 128 of them from B, K rows of stride ldb.
// K % 16 == 0; every row 16-byte aligned.  All 256 threads call; ends behind a barrier (the stages may be overwritten at once).
template <bool B_KROWS>
__device__ __forceinline__ void tile_product(TileLds &s, const float *__restrict__ A, int lda, int a_rows, const float *__restrict__ B, int ldb,
                                             int b_rows, int K, f32x16 (&acc)[4])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = tid & 3, kh = lane >> 5;
    float4 ra[2], rb[2];
    auto load_stage = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int e = tid + 256 * i, r = e >> 2;
            ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < a_rows) ra[i] = *reinterpret_cast<const float4 *>(A + (size_t)r * lda + k0 + kq * 4);
            if (B_KROWS) {
                rb[i] = *reinterpret_cast<const float4 *>(B + (size_t)(k0 + (e >> 5)) * ldb + (e & 31) * 4);
            } else {
                rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < b_rows) rb[i] = *reinterpret_cast<const float4 *>(B + (size_t)r * ldb + k0 + kq * 4);
            }
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int e = tid + 256 * i, r = e >> 2;
            s.A[buf][kq * 4 + 0][r] = ra[i].x; s.A[buf][kq * 4 + 1][r] = ra[i].y; s.A[buf][kq * 4 + 2][r] = ra[i].z; s.A[buf][kq * 4 + 3][r] = ra[i].w;
            if (B_KROWS) {
                *reinterpret_cast<float4 *>(&s.B[buf][e >> 5][(e & 31) * 4]) = rb[i];
            } else {
                s.B[buf][kq * 4 + 0][r] = rb[i].x; s.B[buf][kq * 4 + 1][r] = rb[i].y; s.B[buf][kq * 4 + 2][r] = rb[i].z; s.B[buf][kq * 4 + 3][r] = rb[i].w;
            }
        }
    };
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
    const int KT = K / TK;
    load_stage(0);
    store_stage(0);
    __syncthreads();
    const int am = lane & 31, bn = wave * 32 + (lane & 31);
    for (int kt = 0; kt < KT; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load_stage((kt + 1) * TK);
#pragma unroll
        for (int kk = 0; kk < TK / 2; kk++) {
            float fa[4];
#pragma unroll
            for (int t = 0; t < 4; t++) fa[t] = s.A[buf][2 * kk + kh][am + 32 * t];
            const float fb = s.B[buf][2 * kk + kh][bn];
#pragma unroll
            for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[t], fb, acc[t], 0, 0, 0);
        }
        if (kt + 1 < KT) store_stage(buf ^ 1);
        __syncthreads();
    }
}

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __builtin_bit_cast(float, (unsigned)h << 16); }

__device__ __forceinline__ unsigned short f32_to_bf16(float v)          // round to nearest even; a NaN stays one
{
    const unsigned u = __builtin_bit_cast(unsigned, v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x0040u);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float wave_sum_f32(float v)                  // xor butterfly: every lane ends with the same bits
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- token labels: one wavefront per token, bytes and integers only.  need > p^2 / 2, so a class that qualifies is the strict majority of
// the cell and each of its bits is the majority of that bit: the candidate is read off eight bit counts, then counted.
__global__ __launch_bounds__(256) void tokcon_labels_kernel(const unsigned char *__restrict__ mask, int esize, unsigned char *__restrict__ labels,
                                                           long long tokens, int S, int p, int need)
{
    const int lane = threadIdx.x & 63;
    const long long tok = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= tokens) return;                                          // (wave-uniform)
    const int g = S / p, n = g * g, pp = p * p;
    const long long b = tok / n;
    const int t = (int)(tok - b * n), r0 = (t / g) * p, c0 = (t % g) * p;
    const unsigned char *base = mask + ((size_t)b * S * S) * esize;
    auto pixel = [&](int idx) -> int { return base[((size_t)(r0 + idx / p) * S + c0 + idx % p) * esize]; };
    int ones[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k0 = 0; k0 < pp; k0 += 64) {
        const bool ok = k0 + lane < pp;
        const int v = ok ? pixel(k0 + lane) : 0;
#pragma unroll
        for (int bit = 0; bit < 8; bit++) ones[bit] += __popcll(__ballot(ok && ((v >> bit) & 1)));
    }
    int cand = 0;
#pragma unroll
    for (int bit = 0; bit < 8; bit++) cand |= (2 * ones[bit] > pp) << bit;
    int cnt = 0;
    for (int k0 = 0; k0 < pp; k0 += 64) {
        const bool ok = k0 + lane < pp;
        const int v = ok ? pixel(k0 + lane) : -1;
        cnt += __popcll(__ballot(ok && v == cand));
    }
    if (lane == 0) labels[tok] = (unsigned char)((cnt >= need && cand != TIGN) ? cand : TIGN);
}

// ---- per-image class counts of the token labels: counts[b][c], c < 256 (integer LDS atomics: exact in any order)
__global__ __launch_bounds__(256) void tokcon_count_kernel(const unsigned char *__restrict__ labels, int *__restrict__ counts, int n)
{
    __shared__ int hist[256];
    const int b = blockIdx.x;
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) atomicAdd(&hist[labels[(size_t)b * n + i]], 1);
    __syncthreads();
    counts[b * 256 + threadIdx.x] = hist[threadIdx.x];
}

// ---- z = x / max(|x|, 1e-12) in fp32, one wavefront per row; rows n .. np - 1 of an image are zeros (the k padding of W Z)
__global__ __launch_bounds__(256) void tokcon_prep_kernel(const unsigned short *__restrict__ x, float *__restrict__ Z, float *__restrict__ den, int n,
                                                         int np)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), img = blockIdx.y;
    if (row >= np) return;
    float *zr = Z + ((size_t)img * np + row) * TD;
    if (row >= n) {
#pragma unroll
        for (int k = 0; k < 3; k++) *reinterpret_cast<float4 *>(zr + (k * 64 + lane) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane == 0) den[(size_t)img * np + row] = 1.f;
        return;
    }
    const unsigned short *xr = x + ((size_t)img * n + row) * TD;
    float v[12], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint2 u = *reinterpret_cast<const uint2 *>(xr + (k * 64 + lane) * 4);
        v[4 * k + 0] = bf16_to_f32((unsigned short)(u.x & 0xffffu)); v[4 * k + 1] = bf16_to_f32((unsigned short)(u.x >> 16));
        v[4 * k + 2] = bf16_to_f32((unsigned short)(u.y & 0xffffu)); v[4 * k + 3] = bf16_to_f32((unsigned short)(u.y >> 16));
    }
#pragma unroll
    for (int e = 0; e < 12; e++) ss = fmaf(v[e], v[e], ss);
    ss = wave_sum_f32(ss);
    const float d = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int k = 0; k < 3; k++)
        *reinterpret_cast<float4 *>(zr + (k * 64 + lane) * 4) = make_float4(v[4 * k] / d, v[4 * k + 1] / d, v[4 * k + 2] / d, v[4 * k + 3] / d);
    if (lane == 0) den[(size_t)img * np + row] = d;
}

// ---- the score tiles.  A = keys j (tile rows), B = anchors i (a lane's column): S^T[j][i] = z_j . z_i, the chain over d ascending, so s_ij
// and s_ji are the same bits.  MODE 0 (forward): the workgroup owns 128 anchors and walks every key tile; per anchor the running maximum,
// sum and positive sum, the two lane halves (different keys of the same anchor) met once at the end.  MODE 1 (backward): one key tile per
// workgroup, W[j][i] = G_ij + G_ji, zeros on the diagonal and in the padding.
template <int MODE>
__global__ __launch_bounds__(256) void tokcon_scores_kernel(const float *__restrict__ Z, const unsigned char *__restrict__ labels, float *__restrict__ lse,
                                                           float *__restrict__ pos, const int *__restrict__ counts, const int *__restrict__ Mp,
                                                           float *__restrict__ W, int n, int np, float tau)
{
    __shared__ TileLds tl;
    __shared__ int ykey[TB];
    __shared__ float lkey[TB], pkey[TB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, img = blockIdx.z;
    Z += (size_t)img * np * TD;
    labels += (size_t)img * n;
    lse += (size_t)img * n;
    pos += (size_t)img * n;
    const int i0 = blockIdx.x * TB, i = i0 + wave * 32 + (lane & 31);
    const int yi = i < n ? labels[i] : TIGN;
    float lse_i = 0.f, invp_i = 0.f, invM = 0.f;
    bool anc_i = false;
    if (MODE == 1) {
        counts += (size_t)img * 256;
        W += (size_t)img * np * np;
        const int ci = yi != TIGN ? counts[yi] : 0, M = *Mp;
        anc_i = ci >= 2;
        invp_i = anc_i ? 1.0f / (float)(ci - 1) : 0.f;
        lse_i = i < n ? lse[i] : 0.f;
        invM = M > 0 ? 1.0f / (float)M : 0.f;
    }
    float m = -INFINITY, l = 0.f, ps = 0.f;
    const int tiles = (n + TB - 1) / TB;
    const int kt0 = MODE == 1 ? blockIdx.y : 0, kt1 = MODE == 1 ? blockIdx.y + 1 : tiles;
    for (int kt = kt0; kt < kt1; kt++) {
        const int j0 = kt * TB;
        if (tid < TB) {
            const int j = j0 + tid, yj = j < n ? labels[j] : TIGN;
            ykey[tid] = yj;
            if (MODE == 1) {
                const int cj = yj != TIGN ? counts[yj] : 0;
                pkey[tid] = cj >= 2 ? 1.0f / (float)(cj - 1) : -1.f;          // -1: not an anchor
                lkey[tid] = j < n ? lse[j] : 0.f;
            }
        }
        f32x16 acc[4];
        tile_product<false>(tl, Z + (size_t)j0 * TD, TD, n - j0, Z + (size_t)i0 * TD, TD, n - i0, TD, acc);      // (its barriers publish ykey)
        if (MODE == 0) {
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int jl = 32 * t + cd_row(r, lane), yj = ykey[jl];
                    const bool ok = yj != TIGN && j0 + jl != i;          // (a key past n carries 255)
                    const float sv = acc[t][r] / tau;
                    if (ok && yj == yi) ps += sv;
                    acc[t][r] = ok ? sv : -INFINITY;
                    mx = fmaxf(mx, acc[t][r]);
                }
            if (mx > -INFINITY) {
                const float m_new = fmaxf(m, mx);
                float sum = 0.f;
#pragma unroll
                for (int t = 0; t < 4; t++)
#pragma unroll
                    for (int r = 0; r < 16; r++) sum += expf(acc[t][r] - m_new);          // (expf(-inf) = 0)
                l = l * expf(m - m_new) + sum;
                m = m_new;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int jl = 32 * t + cd_row(r, lane), j = j0 + jl;
                    float w = 0.f;
                    if (i < n && j < n && i != j) {
                        const int yj = ykey[jl];
                        const float sv = acc[t][r] / tau, pj = pkey[jl];
                        if (anc_i) w += invM * ((yj != TIGN ? expf(sv - lse_i) : 0.f) - (yj == yi ? invp_i : 0.f));
                        if (pj >= 0.f) w += invM * ((yi != TIGN ? expf(sv - lkey[jl]) : 0.f) - (yi == yj ? pj : 0.f));
                    }
                    if (i < np && j < np) W[(size_t)j * np + i] = w;
                }
        }
        __syncthreads();          // the key labels are rewritten by the next tile
    }
    if (MODE == 0) {
        const float m2 = __shfl_xor(m, 32, 64), l2 = __shfl_xor(l, 32, 64), ps2 = __shfl_xor(ps, 32, 64);
        if (lane < 32 && i < n) {
            const float mm = fmaxf(m, m2);
            float lt = 0.f;
            if (m > -INFINITY) lt += l * expf(m - mm);
            if (m2 > -INFINITY) lt += l2 * expf(m2 - mm);
            lse[i] = lt > 0.f ? mm + logf(lt) : 0.f;          // (no key in A(i): not an anchor, never read)
            pos[i] = ps + ps2;
        }
    }
}

// ---- dZ[i][d] = sum_j W[i][j] Z[j][d] (W symmetric, stored with its padding zeroed): A = W rows, B = Z read as [k = j][d]
__global__ __launch_bounds__(256) void tokcon_wz_kernel(const float *__restrict__ W, const float *__restrict__ Z, float *__restrict__ dZ, int n, int np)
{
    __shared__ TileLds tl;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, img = blockIdx.z;
    const int d0 = blockIdx.x * TB, i0 = blockIdx.y * TB;
    W += (size_t)img * np * np;
    Z += (size_t)img * np * TD;
    dZ += (size_t)img * np * TD;
    f32x16 acc[4];
    tile_product<true>(tl, W + (size_t)i0 * np, np, np - i0, Z + d0, TD, 0, np, acc);
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = i0 + 32 * t + cd_row(r, lane);
            if (row < n) dZ[(size_t)row * TD + d0 + wave * 32 + (lane & 31)] = acc[t][r];
        }
}

// ---- dx_i = (g_i - (g_i . z_i) z_i) * up / (tau max(|x_i|, 1e-12)), g_i the row of W Z; one wavefront per row, rounded once to bf16
__global__ __launch_bounds__(256) void tokcon_rows_kernel(const float *__restrict__ dZ, const float *__restrict__ Z, const float *__restrict__ den,
                                                         const float *__restrict__ upstream, unsigned short *__restrict__ dx, int n, int np, float tau)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), img = blockIdx.y;
    if (row >= n) return;
    const float *g = dZ + ((size_t)img * np + row) * TD, *z = Z + ((size_t)img * np + row) * TD;
    float4 gv[3], zv[3];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        gv[k] = *reinterpret_cast<const float4 *>(g + (k * 64 + lane) * 4);
        zv[k] = *reinterpret_cast<const float4 *>(z + (k * 64 + lane) * 4);
        dot = fmaf(gv[k].x, zv[k].x, dot); dot = fmaf(gv[k].y, zv[k].y, dot); dot = fmaf(gv[k].z, zv[k].z, dot); dot = fmaf(gv[k].w, zv[k].w, dot);
    }
    dot = wave_sum_f32(dot);
    const float scale = *upstream / (tau * den[(size_t)img * np + row]);
    unsigned short *o = dx + ((size_t)img * n + row) * TD;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const unsigned a = f32_to_bf16((gv[k].x - dot * zv[k].x) * scale), b = f32_to_bf16((gv[k].y - dot * zv[k].y) * scale);
        const unsigned c = f32_to_bf16((gv[k].z - dot * zv[k].z) * scale), d = f32_to_bf16((gv[k].w - dot * zv[k].w) * scale);
        *reinterpret_cast<uint2 *>(o + (k * 64 + lane) * 4) = make_uint2(a | (b << 16), c | (d << 16));
    }
}

// ---- M and the loss: one workgroup.  M = the anchors of the batch (integers); the sum of l_i over thread-strided tokens in double, the
// wavefronts' butterflies, the four wave sums in wave order.  M = 0: the loss is an exact 0.
__global__ __launch_bounds__(256) void tokcon_finalize_kernel(const unsigned char *__restrict__ labels, const float *__restrict__ lse,
                                                             const float *__restrict__ pos, int *__restrict__ counts, float *__restrict__ loss, int B,
                                                             int n)
{
    __shared__ int Ms;
    __shared__ double part[4];
    const int tid = threadIdx.x;
    if (tid == 0) Ms = 0;
    __syncthreads();
    int mine = 0;
    for (long long e = tid; e < (long long)B * 256; e += 256) {
        const int c = counts[e];
        if ((e & 255) != TIGN && c >= 2) mine += c;
    }
    atomicAdd(&Ms, mine);
    double sum = 0.0;
    for (long long e = tid; e < (long long)B * n; e += 256) {
        const int y = labels[e];
        if (y == TIGN) continue;
        const int c = counts[(e / n) * 256 + y];
        if (c >= 2) sum += (double)lse[e] - (double)pos[e] / (double)(c - 1);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        const int M = Ms;
        counts[(size_t)B * 256] = M;
        *loss = M > 0 ? (float)((((part[0] + part[1]) + part[2]) + part[3]) / (double)M) : 0.f;
    }
}

// ---- the junction for four consumers (vit_kernels.hip: token_junction_bwd_kernel is the three-pointer one and stays as it is)
__global__ __launch_bounds__(256) void token_junction_bwd4_kernel(const unsigned short *__restrict__ g0, const unsigned short *__restrict__ g1,
                                                                 const unsigned short *__restrict__ g2, const unsigned short *__restrict__ g3,
                                                                 float *__restrict__ dx, int N, long long total4)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;            // one float4 of dx
    if (i >= total4) return;
    constexpr int D4 = TD / 4;
    const long long row = i / D4;
    const int c4 = (int)(i - row * D4), t = (int)(row % N);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t != 0) {
        const size_t src = ((size_t)((row / N) * (N - 1) + t - 1) * D4 + c4) * 4;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        bool first = true;
        for (const unsigned short *g : {g0, g1, g2, g3}) {
            if (!g) continue;
            const uint2 u = *reinterpret_cast<const uint2 *>(g + src);
            const float v[4] = {__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                                __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u)};
            if (first) { a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3]; first = false; }
            else { a[0] += v[0]; a[1] += v[1]; a[2] += v[2]; a[3] += v[3]; }
        }
        o = make_float4(a[0], a[1], a[2], a[3]);
    }
    *reinterpret_cast<float4 *>(dx + i * 4) = o;
}

inline int padded(int n) { return (n + 15) / 16 * 16; }
inline size_t image_bytes(int n)          // Z, dZ, W and the row norms of one image
{
    const size_t np = padded(n);
    return align_up(np * TD * sizeof(float), 256) * 2 + align_up(np * np * sizeof(float), 256) + align_up(np * sizeof(float), 256);
}
inline int chunk_images(int B, int n)
{
    const size_t fit = kScratchCap / image_bytes(n);
    return (int)(fit < 1 ? 1 : (fit > (size_t)B ? (size_t)B : fit));
}

struct Scratch { float *Z, *dZ, *W, *den; };
inline Scratch carve(void *ws, int n, int c)
{
    const size_t np = padded(n);
    Carver cv(ws);
    Scratch s;
    s.Z = cv.take<float>((size_t)c * np * TD);
    s.dZ = cv.take<float>((size_t)c * np * TD);
    s.W = cv.take<float>((size_t)c * np * np);
    s.den = cv.take<float>((size_t)c * np);
    return s;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_envelope(const char *who, const void *tokens, const void *labels, int B, int n, int dim, float tau, const void *ws, size_t ws_bytes)
{
    COSA_REQUIRE(tokens && labels && ws, "%s: null operand", who);
    COSA_REQUIRE(dim == TD, "%s: token width must be 768 (got %d)", who, dim);
    COSA_REQUIRE(B >= 1 && B <= 65535 && n >= 2 && n <= TMAXN, "%s: 1 <= B <= 65535, 2 <= n <= %d (got B=%d n=%d)", who, TMAXN, B, n);
    COSA_REQUIRE(tau >= 0.01f && tau <= 10.0f, "%s: the temperature must lie in [0.01, 10] (got %g)", who, (double)tau);
    COSA_REQUIRE(aligned16(tokens) && aligned16(ws), "%s: tokens and workspace must be 16-byte aligned", who);
    COSA_REQUIRE(ws_bytes >= cosa_token_contrast_workspace_bytes(B, n), "%s: workspace too small", who);
    return COSA_OK;
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_token_labels(const void *mask, int elem_bytes, uint8_t *labels, int B, int S, int p, int need, void *stream)
{
    COSA_REQUIRE(mask && labels, "cosa_token_labels: null operand");
    COSA_REQUIRE(elem_bytes == 1 || elem_bytes == 8, "cosa_token_labels: a uint8 or int64 label map (element size %d)", elem_bytes);
    COSA_REQUIRE(B >= 1 && p >= 1 && S >= p && S % p == 0 && S <= 32768, "cosa_token_labels: the patch size must divide the map (got B=%d S=%d p=%d)", B, S, p);
    COSA_REQUIRE(need <= p * p && 2 * need > p * p, "cosa_token_labels: need must lie in (p^2 / 2, p^2] (got %d for p=%d)", need, p);
    const long long tokens = (long long)B * (S / p) * (S / p);
    COSA_REQUIRE((tokens + 3) / 4 < 0x7fffffffll, "cosa_token_labels: too many tokens for one launch");
    hipLaunchKernelGGL(tokcon_labels_kernel, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, as_stream(stream), static_cast<const unsigned char *>(mask),
                       elem_bytes, labels, tokens, S, p, need);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" size_t cosa_token_contrast_workspace_bytes(int B, int n)
{
    if (B < 1 || n < 2 || n > TMAXN) return 0;
    return image_bytes(n) * (size_t)chunk_images(B, n);
}

extern "C" int cosa_token_contrast_fwd(const void *tokens, const uint8_t *labels, float *rows, int32_t *counts, float *loss, int B, int n, int dim,
                                       float tau, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_envelope("cosa_token_contrast_fwd", tokens, labels, B, n, dim, tau, workspace, workspace_bytes)) return rc;
    COSA_REQUIRE(rows && counts && loss, "cosa_token_contrast_fwd: null output");
    hipStream_t st = as_stream(stream);
    const int np = padded(n), cb = chunk_images(B, n), tiles = (n + TB - 1) / TB;
    float *lse = rows, *pos = rows + (size_t)B * n;
    hipLaunchKernelGGL(tokcon_count_kernel, dim3(B), dim3(256), 0, st, labels, counts, n);
    COSA_LAUNCH_CHECK();
    for (int b0 = 0; b0 < B; b0 += cb) {
        const int c = B - b0 < cb ? B - b0 : cb;
        const Scratch s = carve(workspace, n, c);
        hipLaunchKernelGGL(tokcon_prep_kernel, dim3((np + 3) / 4, c), dim3(256), 0, st, static_cast<const unsigned short *>(tokens) + (size_t)b0 * n * TD,
                           s.Z, s.den, n, np);
        COSA_LAUNCH_CHECK();
        hipLaunchKernelGGL(tokcon_scores_kernel<0>, dim3(tiles, 1, c), dim3(256), 0, st, s.Z, labels + (size_t)b0 * n, lse + (size_t)b0 * n,
                           pos + (size_t)b0 * n, nullptr, nullptr, nullptr, n, np, tau);
        COSA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tokcon_finalize_kernel, dim3(1), dim3(256), 0, st, labels, lse, pos, counts, loss, B, n);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_token_contrast_bwd(const void *tokens, const uint8_t *labels, const float *rows, const int32_t *counts, const float *upstream,
                                       void *dx, int B, int n, int dim, float tau, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_envelope("cosa_token_contrast_bwd", tokens, labels, B, n, dim, tau, workspace, workspace_bytes)) return rc;
    COSA_REQUIRE(rows && counts && upstream && dx && aligned16(dx), "cosa_token_contrast_bwd: null or misaligned operand");
    hipStream_t st = as_stream(stream);
    const int np = padded(n), cb = chunk_images(B, n), tiles = (n + TB - 1) / TB;
    float *lse = const_cast<float *>(rows), *pos = lse + (size_t)B * n;
    for (int b0 = 0; b0 < B; b0 += cb) {
        const int c = B - b0 < cb ? B - b0 : cb;
        const Scratch s = carve(workspace, n, c);
        hipLaunchKernelGGL(tokcon_prep_kernel, dim3((np + 3) / 4, c), dim3(256), 0, st, static_cast<const unsigned short *>(tokens) + (size_t)b0 * n * TD,
                           s.Z, s.den, n, np);
        COSA_LAUNCH_CHECK();
        hipLaunchKernelGGL(tokcon_scores_kernel<1>, dim3(tiles, tiles, c), dim3(256), 0, st, s.Z, labels + (size_t)b0 * n, lse + (size_t)b0 * n,
                           pos + (size_t)b0 * n, counts + (size_t)b0 * 256, counts + (size_t)B * 256, s.W, n, np, tau);
        COSA_LAUNCH_CHECK();
        hipLaunchKernelGGL(tokcon_wz_kernel, dim3(TD / TB, tiles, c), dim3(256), 0, st, s.W, s.Z, s.dZ, n, np);
        COSA_LAUNCH_CHECK();
        hipLaunchKernelGGL(tokcon_rows_kernel, dim3((n + 3) / 4, c), dim3(256), 0, st, s.dZ, s.Z, s.den, upstream,
                           static_cast<unsigned short *>(dx) + (size_t)b0 * n * TD, n, np, tau);
        COSA_LAUNCH_CHECK();
    }
    return COSA_OK;
}

extern "C" int cosa_token_junction_bwd4(const void *g0, const void *g1, const void *g2, const void *g3, float *dx, int B, int N, int dim, void *stream)
{
    COSA_REQUIRE((g0 || g1 || g2 || g3) && dx && B > 0 && N > 1, "cosa_token_junction_bwd4: bad arguments");
    COSA_REQUIRE(dim == TD, "cosa_token_junction_bwd4: dim must be 768 (ViT-B)");
    const long long total4 = (long long)B * N * (TD / 4);
    COSA_REQUIRE((total4 + 255) / 256 < 0x7fffffffll, "cosa_token_junction_bwd4: too many elements for one launch");
    hipLaunchKernelGGL(token_junction_bwd4_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       static_cast<const unsigned short *>(g0), static_cast<const unsigned short *>(g1), static_cast<const unsigned short *>(g2),
                       static_cast<const unsigned short *>(g3), dx, N, total4);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
