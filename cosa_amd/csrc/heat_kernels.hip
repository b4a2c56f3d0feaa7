// heat_kernels.hip -- the CAM pictures of prediction export: per-class heat maps over the image, and the
// comparison panel.
//
// cosa_export_camheat: k class planes [k, H W] fp32 (a record's rawcam slot) over one normalised image, as k interleaved RGB pictures.
//   Integers throughout: idx = trunc(255 m) clamped to 0..255 (a NaN gives 0); the ramp jet[idx][c] = (clamp(765 - |8 idx - k_c|, 0, 510)
//   + 1) >> 1 with k = 1530, 1020, 510; s = jet + the image's byte (overlay_byte's rule); M = the picture's maximum of s; the byte is
//   255 s / M in integer division.  Two launches whatever k is (grid.y = the picture): the maxima -- a wave butterfly, one LDS atomicMax
//   per wave, one global atomicMax per workgroup, on k words the entry zeroes on the stream -- then the bytes.  The access pattern is
//   export_overlay_kernel's: a thread owns four consecutive pixels, one dwordx4 per colour plane and one of the class plane (a plane that
//   H W % 4 != 0 moves off the 16-byte grid is loaded unaligned), three dwords out (picture j starts 3 H W j bytes in: off the dword grid
//   for odd H W, a store the target takes unaligned); the H W % 4 pixels behind go one per thread.
//   The division: n = 255 s <= 130050, M <= 510; with r = floor((2^32 - 1) / M) + 1 the error e = r M - 2^32 lies in 0..M, so
//   n e <= 130050 * 510 < 2^32 and mulhi(n, r) = floor(n / M) exactly (Granlund & Montgomery 1994, Theorem 4.2).
//
// cosa_export_panel: per class j one picture [H, cols W, 3]: the heat picture | seg == class | gt == class (when gt is given) | the image.
//   One launch, a thread per output pixel, grid.y = the picture.
#include "common.hpp"
#include "wave_reduce.hpp"

namespace cosa {
namespace {

constexpr int kHeatThreads = 256;
constexpr int kPanelR = 10, kPanelG = 186, kPanelB = 181;

// (uint8 - mean) / std back to the byte it came from: export_overlay's rule (product and sum each rounded once: no contraction in this file)
__device__ __forceinline__ int heat_image_byte(float x, int c)
{
    const float mean = c == 0 ? 123.675f : c == 1 ? 116.28f : 103.53f;
    const float sd = c == 0 ? 58.395f : c == 1 ? 57.12f : 57.375f;
    const float u = rintf(x * sd + mean);
    return (int)fminf(fmaxf(u, 0.0f), 255.0f);                           // (a NaN leaves fmaxf as 0)
}

__device__ __forceinline__ int heat_index(float m)
{
    return (int)fminf(fmaxf(255.0f * m, 0.0f), 255.0f);                  // the conversion truncates; a NaN leaves fmaxf as 0
}

__device__ __forceinline__ int heat_jet(int idx, int c)
{
    const int d = 8 * idx - (c == 0 ? 1530 : c == 1 ? 1020 : 510);
    const int v = 765 - (d < 0 ? -d : d);
    return ((v < 0 ? 0 : v > 510 ? 510 : v) + 1) >> 1;
}

__device__ __forceinline__ int heat_sum(float m, float x, int c) { return heat_jet(heat_index(m), c) + heat_image_byte(x, c); }

__device__ __forceinline__ float4 load4(const float *src)
{
    float4 f;
    if (((size_t)src & 15) == 0)
        f = *reinterpret_cast<const float4 *>(src);
    else
        __builtin_memcpy(&f, src, 16);                                   // a plane off the 16-byte grid: a load the target takes unaligned
    return f;
}

struct HeatArgs {
    const float *planes;                    // [k, H W]
    const float *image;                     // [3, H W] normalised
    uint8_t *out;                           // [k, H W, 3]
    unsigned *maxima;                       // [k]
    size_t hw, groups;                      // groups: the four-pixel items of the body [0, 4 groups)
};

// the twelve sums of one four-pixel group, s[c][i]
__device__ __forceinline__ void heat_group(const HeatArgs &p, const float *plane, size_t q, int s[3][4])
{
    const float4 m = load4(plane + 4 * q);
    const float mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float4 f = load4(p.image + (size_t)c * p.hw + 4 * q);
        const float fv[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int i = 0; i < 4; i++) s[c][i] = heat_sum(mv[i], fv[i], c);
    }
}

__global__ __launch_bounds__(kHeatThreads) void camheat_max_kernel(const HeatArgs p)
{
    __shared__ unsigned lds_max;
    if (threadIdx.x == 0) lds_max = 0;
    __syncthreads();
    const float *plane = p.planes + (size_t)blockIdx.y * p.hw;
    int best = 0;
    for (size_t q = (size_t)blockIdx.x * kHeatThreads + threadIdx.x; q < p.groups; q += (size_t)gridDim.x * kHeatThreads) {
        int s[3][4];
        heat_group(p, plane, q, s);
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) best = s[c][i] > best ? s[c][i] : best;
    }
    for (size_t i = 4 * p.groups + (size_t)blockIdx.x * kHeatThreads + threadIdx.x; i < p.hw; i += (size_t)gridDim.x * kHeatThreads) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int s = heat_sum(plane[i], p.image[(size_t)c * p.hw + i], c);
            best = s > best ? s : best;
        }
    }
    const unsigned w = wave_max32((unsigned)best);                       // every lane is here: the loops above hold no barrier
    if ((threadIdx.x & 63) == 0) atomicMax(&lds_max, w);
    __syncthreads();
    if (threadIdx.x == 0 && lds_max) atomicMax(&p.maxima[blockIdx.y], lds_max);
}

__global__ __launch_bounds__(kHeatThreads) void camheat_bytes_kernel(const HeatArgs p)
{
    const float *plane = p.planes + (size_t)blockIdx.y * p.hw;
    uint8_t *out = p.out + (size_t)blockIdx.y * 3 * p.hw;
    const unsigned M = p.maxima[blockIdx.y];                             // >= 128: every pixel's blue sum holds jet's 128 or more ...
    const unsigned r = 0xffffffffu / (M ? M : 1u) + 1u;                  // ... (the guard only keeps a foreign workspace from a division by zero)
    for (size_t q = (size_t)blockIdx.x * kHeatThreads + threadIdx.x; q < p.groups; q += (size_t)gridDim.x * kHeatThreads) {
        int s[3][4];
        heat_group(p, plane, q, s);
        unsigned w[3] = {0, 0, 0};                                       // twelve bytes R G B R G B ..., little-endian into three dwords
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int b = 3 * i + c;
                w[b >> 2] |= __umulhi(255u * (unsigned)s[c][i], r) << (8 * (b & 3));
            }
        __builtin_memcpy(out + 12 * q, w, 12);                           // one dwordx3, on the dword grid or off it (odd H W, j > 0)
    }
    for (size_t i = 4 * p.groups + (size_t)blockIdx.x * kHeatThreads + threadIdx.x; i < p.hw; i += (size_t)gridDim.x * kHeatThreads) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            out[3 * i + c] = (uint8_t)__umulhi(255u * (unsigned)heat_sum(plane[i], p.image[(size_t)c * p.hw + i], c), r);
    }
}

struct PanelArgs {
    const uint8_t *heat;                    // [k, H W, 3]
    const uint8_t *seg;                     // [H W]
    const uint8_t *gt;                      // [H W] or null
    const int *class_idx;                   // [k] 0-based
    const float *image;                     // [3, H W] normalised
    uint8_t *out;                           // [k, H, cols W, 3]
    unsigned hw, W, cols;
};

__global__ __launch_bounds__(kHeatThreads) void panel_kernel(const PanelArgs p)
{
    const unsigned j = blockIdx.y, row = p.cols * p.W, n = p.cols * p.hw;          // n < 2^31: H W < 2^29, cols <= 4
    const int cls = p.class_idx[j] + 1;
    const uint8_t *heat = p.heat + (size_t)j * 3 * p.hw;
    uint8_t *out = p.out + (size_t)j * 3 * n;
    for (unsigned o = blockIdx.x * kHeatThreads + threadIdx.x; o < n; o += gridDim.x * kHeatThreads) {
        const unsigned y = o / row, xo = o - y * row, col = xo / p.W, i = y * p.W + (xo - col * p.W);
        int v[3];
        if (col == 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = heat[3 * (size_t)i + c];
        } else if (col == p.cols - 1) {
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = heat_image_byte(p.image[(size_t)c * p.hw + i], c);
        } else {
            const bool on = col == 1 ? p.seg[i] == cls : (p.gt[i] == cls && cls != 255);         // a gt of 255 is `ignore`, never a class
            v[0] = on ? kPanelR : 0; v[1] = on ? kPanelG : 0; v[2] = on ? kPanelB : 0;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) out[3 * (size_t)o + c] = (uint8_t)v[c];
    }
}

unsigned heat_blocks(size_t items)
{
    size_t blocks = (items + kHeatThreads - 1) / kHeatThreads;
    return (unsigned)(blocks > 2048 ? 2048 : blocks < 1 ? 1 : blocks);
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" int cosa_export_camheat(const float *planes, const float *image, int k, int H, int W, uint8_t *out, size_t out_bytes,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    COSA_REQUIRE(planes && image && out && workspace, "cosa_export_camheat: null argument");
    COSA_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1ll << 29), "cosa_export_camheat: H, W must be > 0 and H W < 2^29 (got %d x %d)", H, W);
    COSA_REQUIRE(k >= 1 && k <= COSA_CAMHEAT_MAX_CLASSES, "cosa_export_camheat: k_live must be in 1..%d (got %d)", COSA_CAMHEAT_MAX_CLASSES, k);
    HeatArgs p;
    p.hw = (size_t)H * W;
    COSA_REQUIRE(out_bytes >= (size_t)k * 3 * p.hw, "cosa_export_camheat: out holds %zu bytes, %zu are needed", out_bytes, (size_t)k * 3 * p.hw);
    COSA_REQUIRE(workspace_bytes >= (size_t)k * sizeof(unsigned) && ((size_t)workspace & 3) == 0,
                 "cosa_export_camheat: the workspace must be 4-byte aligned and hold %zu bytes (got %zu)", (size_t)k * sizeof(unsigned),
                 workspace_bytes);
    COSA_REQUIRE((((size_t)planes | (size_t)image) & 3) == 0, "cosa_export_camheat: planes and image must be 4-byte aligned");
    p.planes = planes; p.image = image; p.out = out; p.maxima = static_cast<unsigned *>(workspace);
    p.groups = p.hw / 4;
    const size_t loose = p.hw - 4 * p.groups;
    const dim3 grid(heat_blocks(p.groups > loose ? p.groups : loose), (unsigned)k);
    COSA_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)k * sizeof(unsigned), as_stream(stream)));
    hipLaunchKernelGGL(camheat_max_kernel, grid, dim3(kHeatThreads), 0, as_stream(stream), p);
    COSA_LAUNCH_CHECK();
    hipLaunchKernelGGL(camheat_bytes_kernel, grid, dim3(kHeatThreads), 0, as_stream(stream), p);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}

extern "C" int cosa_export_panel(const uint8_t *heat, const uint8_t *seg, const uint8_t *gt, const int *class_idx, const float *image, int k,
                                 int H, int W, uint8_t *out, size_t out_bytes, void *stream)
{
    COSA_REQUIRE(heat && seg && class_idx && image && out, "cosa_export_panel: null argument");
    COSA_REQUIRE(H > 0 && W > 0 && (long long)H * W < (1ll << 29), "cosa_export_panel: H, W must be > 0 and H W < 2^29 (got %d x %d)", H, W);
    COSA_REQUIRE(k >= 1 && k <= COSA_CAMHEAT_MAX_CLASSES, "cosa_export_panel: k_live must be in 1..%d (got %d)", COSA_CAMHEAT_MAX_CLASSES, k);
    PanelArgs p;
    p.hw = (unsigned)((size_t)H * W); p.W = (unsigned)W; p.cols = gt ? 4u : 3u;
    const size_t need = (size_t)k * 3 * p.cols * p.hw;
    COSA_REQUIRE(out_bytes >= need, "cosa_export_panel: out holds %zu bytes, %zu are needed", out_bytes, need);
    COSA_REQUIRE((((size_t)class_idx | (size_t)image) & 3) == 0, "cosa_export_panel: class_idx and image must be 4-byte aligned");
    p.heat = heat; p.seg = seg; p.gt = gt; p.class_idx = class_idx; p.image = image; p.out = out;
    hipLaunchKernelGGL(panel_kernel, dim3(heat_blocks((size_t)p.cols * p.hw), (unsigned)k), dim3(kHeatThreads), 0, as_stream(stream), p);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
