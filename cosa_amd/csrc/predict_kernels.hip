// predict_kernels.hip -- the two kernels of label-free prediction export.
//
// cosa_predict_classes: the image-level class row from the network's own classification logits.  One wavefront per image, classes on the
//   lanes (class c on lane c % 64, register c / 64: at most four per lane at C <= 256).  Class c is present iff logit_c >= L (a NaN never
//   is); the count is a ballot / popcount per register.  If fewer than cls_min are present, the largest remaining logit is added per
//   round -- wave_max of wave_reduce.hpp, then the first lane of the first register that holds it, i.e. the lowest class index among equal
//   logits -- until cls_min are present or nothing addable is left (a NaN and -inf are never added).  nonfinite counts the image's NaN
//   and +-inf logits.  Every output word is written by a plain vector store; no atomics, no workspace.
//
// cosa_export_overlay: the written `seg` map painted over the image, as interleaved RGB bytes, into the image's export record.  Integer
//   blending: the same bytes on every run.  A thread owns four consecutive pixels: one dwordx4 per colour plane (the planes of an image
//   whose H W is no multiple of four start off a 16-byte boundary: those loads are made as unaligned ones), one dword of labels, three
//   dwords out; the H W % 4 pixels behind the last group go one per thread.
#include "common.hpp"
#include "wave_reduce.hpp"

namespace cosa {
namespace {

constexpr int kPredictRegs = COSA_PREDICT_MAX_CLASSES / 64;

__global__ __launch_bounds__(64) void predict_classes_kernel(const float *__restrict__ logits, int C, float L, int cls_min,
                                                             float *__restrict__ rows, int *__restrict__ k_live, int *__restrict__ nonfinite)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    const float *x = logits + (size_t)g * C;
    float v[kPredictRegs];
    bool present[kPredictRegs], addable[kPredictRegs];
    int count = 0, bad = 0;
#pragma unroll
    for (int j = 0; j < kPredictRegs; j++) {
        const int c = lane + 64 * j;
        const bool live = c < C;
        v[j] = live ? x[c] : 0.0f;
        present[j] = live && v[j] >= L;                                  // false for a NaN
        addable[j] = live && !present[j] && v[j] == v[j] && v[j] != -INFINITY;
        count += __popcll(__ballot(present[j]));
        bad += __popcll(__ballot(live && nonfinite_bits(v[j])));
    }
    // the fill: `count` and `m` are wave-uniform, so every lane leaves the loop in the same round
    while (count < cls_min) {
        float m = -INFINITY;                                             // no addable logit is -inf: -inf left over means none is left
#pragma unroll
        for (int j = 0; j < kPredictRegs; j++) m = fmaxf(m, addable[j] ? v[j] : -INFINITY);
        m = wave_max(m);
        if (m == -INFINITY) break;
        bool taken = false;
#pragma unroll
        for (int j = 0; j < kPredictRegs; j++) {                         // register j holds classes 64 j .. 64 j + 63: the first hit is the lowest index
            const unsigned long long hit = __ballot(!taken && addable[j] && v[j] == m);
            if (hit && !taken) {
                if (lane == __ffsll(hit) - 1) {
                    present[j] = true;
                    addable[j] = false;
                }
                taken = true;
            }
        }
        count++;
    }
#pragma unroll
    for (int j = 0; j < kPredictRegs; j++) {
        const int c = lane + 64 * j;
        if (c < C) rows[(size_t)g * C + c] = present[j] ? 1.0f : 0.0f;
    }
    if (lane == 0) {
        k_live[g] = count;
        nonfinite[g] = bad;
    }
}

struct OverlayArgs {
    const float *image;                     // [3, H W] normalised
    const uint8_t *seg;                     // [H W]
    const uint8_t *palette;                 // [256, 3]
    uint8_t *out;                           // [H W, 3]
    size_t hw, groups;                      // groups: the four-pixel items of the body [0, 4 groups)
    int a;                                  // round(alpha * 256), 0..256
    unsigned aligned;                       // bit c: colour plane c starts on a 16-byte boundary
};

// (uint8 - mean) / std back to the byte it came from: the product and the sum each round once (no contraction in this file), together far
// below the half unit that rint needs
__device__ __forceinline__ int overlay_byte(float x, int c)
{
    const float mean = c == 0 ? 123.675f : c == 1 ? 116.28f : 103.53f;
    const float sd = c == 0 ? 58.395f : c == 1 ? 57.12f : 57.375f;
    const float u = rintf(x * sd + mean);
    return (int)fminf(fmaxf(u, 0.0f), 255.0f);                           // (a NaN leaves fmaxf as 0)
}

__device__ __forceinline__ unsigned overlay_blend(const uint8_t *pal, int label, int c, int img, int a)
{
    return label ? (unsigned)((a * (int)pal[3 * label + c] + (256 - a) * img + 128) >> 8) : (unsigned)img;
}

__global__ __launch_bounds__(256) void export_overlay_kernel(const OverlayArgs p)
{
    __shared__ uint8_t pal[768];
    for (int i = threadIdx.x; i < 768; i += 256) pal[i] = p.palette[i];
    __syncthreads();
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < p.groups; q += (size_t)gridDim.x * 256) {
        const unsigned lab4 = *reinterpret_cast<const unsigned *>(p.seg + 4 * q);
        float px[3][4];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float *src = p.image + (size_t)c * p.hw + 4 * q;
            float4 f;
            if ((p.aligned >> c) & 1)
                f = *reinterpret_cast<const float4 *>(src);
            else
                __builtin_memcpy(&f, src, 16);                           // a plane off the 16-byte grid: a load the target takes unaligned
            px[c][0] = f.x; px[c][1] = f.y; px[c][2] = f.z; px[c][3] = f.w;
        }
        unsigned w[3] = {0, 0, 0};                                       // twelve bytes R G B R G B ..., little-endian into three dwords
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int label = (lab4 >> (8 * k)) & 255;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int b = 3 * k + c;
                w[b >> 2] |= overlay_blend(pal, label, c, overlay_byte(px[c][k], c), p.a) << (8 * (b & 3));
            }
        }
        unsigned *dst = reinterpret_cast<unsigned *>(p.out + 12 * q);
        dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
    }
    const size_t body = 4 * p.groups;
    // fewer than four pixels -- or every pixel, when the caller's buffers keep the body from being formed (see the host)
    for (size_t i = body + (size_t)blockIdx.x * 256 + threadIdx.x; i < p.hw; i += (size_t)gridDim.x * 256) {
        const int label = p.seg[i];
#pragma unroll
        for (int c = 0; c < 3; c++)
            p.out[3 * i + c] = (uint8_t)overlay_blend(pal, label, c, overlay_byte(p.image[(size_t)c * p.hw + i], c), p.a);
    }
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_predict_classes(const float *logits, int G, int C, float L, int cls_min, float *rows, int *k_live, int *nonfinite,
                                    void *stream)
{
    COSA_REQUIRE(logits && rows && k_live && nonfinite, "cosa_predict_classes: null argument");
    COSA_REQUIRE(C >= 1 && C <= COSA_PREDICT_MAX_CLASSES, "cosa_predict_classes: C must be in 1..%d (got %d)", COSA_PREDICT_MAX_CLASSES, C);
    COSA_REQUIRE(G >= 1 && G <= 65535, "cosa_predict_classes: G must be in 1..65535 (got %d)", G);
    COSA_REQUIRE(cls_min >= 0 && cls_min <= C, "cosa_predict_classes: cls_min must be in 0..C (got %d, C = %d)", cls_min, C);
    COSA_REQUIRE(L == L, "cosa_predict_classes: the threshold logit is NaN");
    hipLaunchKernelGGL(predict_classes_kernel, dim3((unsigned)G), dim3(64), 0, as_stream(stream), logits, C, L, cls_min, rows, k_live,
                       nonfinite);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_export_overlay(const float *image, const uint8_t *seg, const uint8_t *palette, int H, int W, int alpha256, uint8_t *out,
                                   void *stream)
{
    COSA_REQUIRE(image && seg && palette && out, "cosa_export_overlay: null argument");
    COSA_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1ll << 29), "cosa_export_overlay: H, W must be > 0 and H W < 2^29 (got %d x %d)", H, W);
    COSA_REQUIRE(alpha256 >= 0 && alpha256 <= 256, "cosa_export_overlay: alpha256 must be in 0..256 (got %d)", alpha256);
    OverlayArgs p;
    p.image = image; p.seg = seg; p.palette = palette; p.out = out; p.a = alpha256;
    p.hw = (size_t)H * W;
    // the four-pixel body needs the label dword, the output dwords and the first colour plane on their natural boundaries; a caller whose
    // buffers are not gets the one-pixel path for the whole image
    const bool vec = ((size_t)image & 15) == 0 && ((size_t)seg & 3) == 0 && ((size_t)out & 3) == 0;
    p.groups = vec ? p.hw / 4 : 0;
    p.aligned = 0;
    for (int c = 0; c < 3; c++)
        if ((((size_t)image + (size_t)c * p.hw * 4) & 15) == 0) p.aligned |= 1u << c;
    const size_t loose = p.hw - 4 * p.groups, items = p.groups > loose ? p.groups : loose;
    size_t blocks = (items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(export_overlay_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), p);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
