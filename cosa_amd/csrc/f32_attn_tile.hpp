// f32_attn_tile.hpp -- the QK^T half that attn_fwd_f32_kernel (f32_kernels.hip) and attn_stats_f32_kernel (act_stats_kernels.hip) share, so
// that the monitor sees the logits the forward kernel's softmax sees: the same blocks, tiles, MFMA orientation and chain over d.
//
// One block = 128 queries of one (batch, head) slice, 4 waves of 32 queries; key tiles of 32 through LDS;
//     S^T[key][query] = K[key][d] Q^T[d][query]         A = K tile from LDS, B = Q held in 32 VGPRs;  the chain over d ascends
// A lane's column is its query; the two lane halves hold different keys of the same query and share one maximum per tile.
// Include from a translation unit compiled with -ffp-contract=off (build.py: EXACT).
#pragma once
#include "common.hpp"

namespace cosa {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int AQ = 128, AK = 32, HD = 64, K_LD = HD + 1;

// row of the C/D tile a lane holds in accumulator register r (32x32 MFMA; the column is lane & 31)
__device__ __forceinline__ int cd_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Q^T as the B operand: step s is d = 2s, 2s + 1; a query past N is zeros
__device__ __forceinline__ void attn_load_q(const float *__restrict__ qp, int query, int N, long long ldq, int half, float (&qreg)[HD / 2])
{
    const float *q = qp + (size_t)query * ldq + half;
#pragma unroll
    for (int s = 0; s < HD / 2; s++) qreg[s] = 0.f;
    if (query < N) {
#pragma unroll
        for (int s = 0; s < HD / 2; s++) qreg[s] = q[2 * s];
    }
}

// staging of a 32-row tile by 256 threads: thread -> row (tid + 256 i) >> 4, d quarter-row (tid & 15) * 4; rows past N are zeros
__device__ __forceinline__ void attn_load_rows(const float *__restrict__ p, int key0, int N, long long ldq, int tid, float4 (&reg)[2])
{
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int key = key0 + ((tid + 256 * i) >> 4), d = (tid & 15) * 4;
        reg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (key < N) reg[i] = *reinterpret_cast<const float4 *>(p + (size_t)key * ldq + d);
    }
}

__device__ __forceinline__ void attn_store_k(float (&Ks)[AK][K_LD], int tid, const float4 (&rk)[2])
{
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int key = (tid + 256 * i) >> 4, d = (tid & 15) * 4;
        Ks[key][d] = rk[i].x; Ks[key][d + 1] = rk[i].y; Ks[key][d + 2] = rk[i].z; Ks[key][d + 3] = rk[i].w;
    }
}

// the scores of one key tile: 32 MFMA steps from a zero accumulator
__device__ __forceinline__ f32x16 attn_scores(const float (&Ks)[AK][K_LD], const float (&qreg)[HD / 2], int lane)
{
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; r++) s[r] = 0.f;
#pragma unroll
    for (int st = 0; st < HD / 2; st++) s = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[lane & 31][2 * st + (lane >> 5)], qreg[st], s, 0, 0, 0);
    return s;
}

struct NoLook {
    __device__ __forceinline__ void operator()(float, bool) const {}
};

// s <- s * scale, -inf for a key past N; -> the query's maximum over the tile (both lane halves).  look(s[r], live) sees every logit once
template <typename Look = NoLook>
__device__ __forceinline__ float attn_mask_max(f32x16 &s, int key0, int N, float scale, int lane, Look look = Look())
{
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const bool live = key0 + cd_row(r, lane) < N;
        s[r] = live ? s[r] * scale : -INFINITY;
        look(s[r], live);
        mx = fmaxf(mx, s[r]);
    }
    return fmaxf(mx, __shfl_xor(mx, 32, 64));
}

}  // namespace
}  // namespace cosa
