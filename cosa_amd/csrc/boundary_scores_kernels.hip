// boundary_scores_kernels.hip -- per-image Boundary IoU counters: cosa_image_scores' row
//   row = [ n, n_valid, then for map m, class c: I, P, G, A ]
// counted over BAND pixels.  A class pixel is interior iff its whole (2d+1) x (2d+1) window lies in the image and holds its own label;
// a class pixel that is not interior is a band pixel of its class, a pixel that is no class is in no band.  Separable:
//   h(y, x) = the 2d+1 pixels of the row window are in the image and equal L(y, x)
//   interior(y, x) = for every row y' of the column window: inside the image, h(y', x) and L(y', x) == L(y, x)
// and each half is a run length: walking a row left to right with the length `run` of the run of equal labels that ends at x',
// h(y, x' - d) = run >= 2d+1; walking a column down with the length `up` of the run of rows with h set and one label that ends at y',
// interior(y' - d, x) = up >= 2d+1.  Positions outside the image are staged as 255, which is no class at any num_classes and so
// breaks every class run.
// A workgroup of 256 threads owns 64 x 64 output tiles (grid stride): it stages the tile and a halo of d of ONE map at a time in LDS
// (16-byte loads where the 16 columns lie inside the row, bytes at the image's edges), runs the row pass over every staged row
// (items = rows x 4 column segments, each with its own warm-up of 2d columns) and the column pass with 64 columns x 4 row segments.
// The ground truth goes first and leaves its label and band flag per tile pixel; each map's column pass then counts the pixel it
// finishes straight into cosa_image_scores' LDS counters: four DISJOINT counts per map and class (I, Px, Gx, X), one LDS atomic per
// run of equal slots, P = I + Px, G = I + Gx, A = I + Px + X at the flush, non-zero words out with 64-bit integer atomics.  No float,
// no workspace, no host sync; the same bytes on every run and for every grid.
#include "common.hpp"
#include "wave_reduce.hpp"

namespace cosa {
namespace {

constexpr int kTile = 64;                  // output tile side
constexpr int kSeg = 16;                   // columns (rows) of a tile that one item of the row (column) pass finishes
constexpr int kMaxD = 64;

struct BoundaryArgs {
    const uint8_t *gt;
    const uint8_t *pred[COSA_IMAGE_SCORES_MAX_MAPS];
    unsigned long long *row;
    int H, W, d, n_maps, nc;
    int tiles_x;
    unsigned long long tiles;
    int R, stride;                          // staged rows (= columns) 64 + 2d; bytes from one staged row to the next
};

inline int staged_stride(int d)             // a multiple of 16 plus one word: full 16-byte items per row, an odd number of banks per row
{
    return (kTile + 2 * d + 15) / 16 * 16 + 4;
}

inline size_t boundary_lds_bytes(int d, int cells)
{
    const int R = kTile + 2 * d;
    return (size_t)4 * cells * 4 + (size_t)R * staged_stride(d) + (size_t)R * kTile + 2 * kTile * kTile;
}

struct Run {                                // a run of equal LDS slots, added with one atomic when it ends; slot < 0: nothing to count
    int slot = -1;
    unsigned cnt = 0;
    __device__ __forceinline__ void push(unsigned *ctr, int s)
    {
        if (s == slot) { cnt++; return; }
        if (slot >= 0) atomicAdd(&ctr[slot], cnt);
        slot = s;
        cnt = 1;
    }
    __device__ __forceinline__ void end(unsigned *ctr)
    {
        if (slot >= 0) atomicAdd(&ctr[slot], cnt);
    }
};

// cosa_image_scores' rule on band membership: t, p the labels, tb, pb "is a band pixel of its class" (false where the label is no
// class).  Counted iff t < nc and p < nc.  base = 4 nc m.
__device__ __forceinline__ void score_band_pixel(unsigned *ctr, int base, int nc, int t, bool tb, int p, bool pb, Run &a, Run &b)
{
    int s1 = -1, s2 = -1;
    if (p < nc) {
        if (pb) {
            if (t >= nc) {
                s1 = base + 4 * p + 3;                      // X
            } else if (tb && t == p) {
                s1 = base + 4 * t;                          // I
            } else {
                s1 = base + 4 * p + 1;                      // Px
                if (tb) s2 = base + 4 * t + 2;              // Gx
            }
        } else if (tb) {
            s2 = base + 4 * t + 2;                          // Gx
        }
    }
    a.push(ctr, s1);
    b.push(ctr, s2);
}

// four pixels of a line from column x on, byte by byte: 255 where the column is outside the image
__device__ __forceinline__ unsigned edge_word(const uint8_t *line, long long x, int W)
{
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) w |= (x + j >= 0 && x + j < W ? (unsigned)line[x + j] : 255u) << (8 * j);
    return w;
}

// the staged region of one map: rows y0 - d .. y0 + 64 + d, columns x0 - d .. , 255 outside the image
__device__ __forceinline__ void stage(const BoundaryArgs &a, const uint8_t *src, uint8_t *lab, long long y0, long long x0)
{
    const int per_row = (a.stride - 4) / 16;
    for (int it = threadIdx.x; it < a.R * per_row; it += 256) {
        const int r = it / per_row, k = it - r * per_row;
        const long long gy = y0 - a.d + r, gx = x0 - a.d + 16 * k;
        uint4 w = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        if (gy >= 0 && gy < a.H) {
            const uint8_t *line = src + (size_t)gy * a.W;
            if (gx >= 0 && gx + 16 <= a.W) {
                __builtin_memcpy(&w, line + gx, 16);            // any byte offset: a load the target takes unaligned
            } else {
                w.x = edge_word(line, gx, a.W);
                w.y = edge_word(line, gx + 4, a.W);
                w.z = edge_word(line, gx + 8, a.W);
                w.w = edge_word(line, gx + 12, a.W);
            }
        }
        unsigned *dst = reinterpret_cast<unsigned *>(lab + (size_t)r * a.stride + 16 * k);
        dst[0] = w.x; dst[1] = w.y; dst[2] = w.z; dst[3] = w.w;
    }
}

// hfl[r][x] for every staged row r and tile column x: item (segment s, row r) walks the staged columns 16 s .. 16 s + 16 + 2d
__device__ __forceinline__ void row_pass(const BoundaryArgs &a, const uint8_t *lab, uint8_t *hfl)
{
    const int need = 2 * a.d + 1;
    for (int it = threadIdx.x; it < 4 * a.R; it += 256) {
        const int s = it / a.R, r = it - s * a.R;                // a wavefront's lanes: consecutive rows, stride an odd number of banks
        const uint8_t *line = lab + (size_t)r * a.stride;
        int prev = 256, run = 0;
        for (int cc = kSeg * s; cc < kSeg * s + kSeg + 2 * a.d; cc++) {
            const int l = line[cc];
            run = l == prev ? run + 1 : 1;
            prev = l;
            if (cc - 2 * a.d >= kSeg * s) hfl[r * kTile + cc - 2 * a.d] = run >= need ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(256) void boundary_scores_kernel(const BoundaryArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned int valid_lds;
    const int nc = a.nc, cells = a.n_maps * nc, d = a.d, need = 2 * d + 1;
    unsigned *ctr = reinterpret_cast<unsigned *>(smem);
    uint8_t *lab = smem + (size_t)16 * cells;
    uint8_t *hfl = lab + (size_t)a.R * a.stride;
    uint8_t *gtl = hfl + (size_t)a.R * kTile;                    // the tile's ground truth: label ...
    uint8_t *gtb = gtl + kTile * kTile;                          // ... and band flag
    for (int i = threadIdx.x; i < 4 * cells; i += 256) ctr[i] = 0;
    if (threadIdx.x == 0) valid_lds = 0;
    const int x = threadIdx.x & 63, seg = threadIdx.x >> 6;      // the column pass: tile column x, tile rows 16 seg .. 16 seg + 16
    unsigned n_valid = 0;
    for (unsigned long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long y0 = (long long)(tile / a.tiles_x) * kTile, x0 = (long long)(tile % a.tiles_x) * kTile;
        const bool col_in = x0 + x < a.W;
        for (int m = -1; m < a.n_maps; m++) {
            __syncthreads();                                      // the zeroing; the passes of the map before
            const uint8_t *src = a.gt;
#pragma unroll
            for (int q = 0; q < COSA_IMAGE_SCORES_MAX_MAPS; q++) src = m == q ? a.pred[q] : src;       // (constant indices: the arguments stay in SGPRs)
            stage(a, src, lab, y0, x0);
            __syncthreads();
            row_pass(a, lab, hfl);
            __syncthreads();
            int prev = 256, up = 0;
            Run r1, r2;
            for (int rr = kSeg * seg; rr < kSeg * seg + kSeg + 2 * d; rr++) {
                const int l = lab[(size_t)rr * a.stride + x + d];
                up = hfl[rr * kTile + x] ? (l == prev ? up + 1 : 1) : 0;
                prev = l;
                const int ty = rr - 2 * d;                        // the tile row this step finishes
                if (ty < kSeg * seg || !col_in || y0 + ty >= a.H) continue;
                const int c = lab[(size_t)(ty + d) * a.stride + x + d];
                const bool band = c < nc && up < need;
                if (m < 0) {
                    gtl[ty * kTile + x] = (uint8_t)c;
                    gtb[ty * kTile + x] = band ? 1 : 0;
                    n_valid += c < nc ? 1u : 0u;
                } else {
                    score_band_pixel(ctr, 4 * nc * m, nc, gtl[ty * kTile + x], gtb[ty * kTile + x] != 0, c, band, r1, r2);
                }
            }
            r1.end(ctr);
            r2.end(ctr);
        }
    }
    n_valid = wave_sum32(n_valid);
    if (__lane_id() == 0 && n_valid) atomicAdd(&valid_lds, n_valid);
    __syncthreads();
    unsigned long long *out = a.row + 2;
    for (int i = threadIdx.x; i < cells; i += 256) {
        const unsigned long long I = ctr[4 * i], Px = ctr[4 * i + 1], Gx = ctr[4 * i + 2], X = ctr[4 * i + 3];
        if (I) atomicAdd(&out[4 * i], I);
        if (I + Px) atomicAdd(&out[4 * i + 1], I + Px);
        if (I + Gx) atomicAdd(&out[4 * i + 2], I + Gx);
        if (I + Px + X) atomicAdd(&out[4 * i + 3], I + Px + X);
    }
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) atomicAdd(&a.row[0], (unsigned long long)a.H * (unsigned long long)a.W);
        if (valid_lds) atomicAdd(&a.row[1], (unsigned long long)valid_lds);
    }
}

}  // namespace
}  // namespace cosa

using namespace cosa;

extern "C" size_t cosa_boundary_scores_words(int num_classes, int n_maps)
{
    if (num_classes < 1 || num_classes > 255 || n_maps < 1 || n_maps > COSA_IMAGE_SCORES_MAX_MAPS) {
        set_error("cosa_boundary_scores_words: num_classes must be in 1..255 and n_maps in 1..%d (got %d, %d)", COSA_IMAGE_SCORES_MAX_MAPS,
                  num_classes, n_maps);
        return 0;
    }
    return 2 + (size_t)n_maps * num_classes * 4;
}

extern "C" int cosa_boundary_scores(const uint8_t *gt, const uint8_t *const *preds, int n_maps, int H, int W, int d, int num_classes,
                                    unsigned long long *row, void *stream)
{
    COSA_REQUIRE(gt && preds && row, "cosa_boundary_scores: null argument");
    COSA_REQUIRE(num_classes >= 1 && num_classes <= 255, "cosa_boundary_scores: num_classes must be in 1..255 (got %d)", num_classes);
    COSA_REQUIRE(n_maps >= 1 && n_maps <= COSA_IMAGE_SCORES_MAX_MAPS, "cosa_boundary_scores: n_maps must be in 1..%d (got %d)",
                 COSA_IMAGE_SCORES_MAX_MAPS, n_maps);
    COSA_REQUIRE(H >= 1 && W >= 1 && (unsigned long long)H * (unsigned long long)W <= 0xffffffffull,
                 "cosa_boundary_scores: H, W must be >= 1 and H * W below 2^32 (got %d x %d)", H, W);
    COSA_REQUIRE(d >= 1 && d <= kMaxD, "cosa_boundary_scores: d must be in 1..%d (got %d)", kMaxD, d);
    COSA_REQUIRE(((size_t)row & 7) == 0, "cosa_boundary_scores: the row must be 8-byte aligned");
    BoundaryArgs a;
    a.gt = gt; a.row = row; a.H = H; a.W = W; a.n_maps = n_maps; a.nc = num_classes;
    for (int m = 0; m < COSA_IMAGE_SCORES_MAX_MAPS; m++) {
        a.pred[m] = m < n_maps ? preds[m] : nullptr;
        COSA_REQUIRE(m >= n_maps || preds[m], "cosa_boundary_scores: map %d is null", m);
    }
    const int side = H > W ? H : W;
    a.d = d < side ? d : side;                       // no pixel is interior from d = max(H, W) on: the same row, a smaller halo
    a.R = kTile + 2 * a.d;
    a.stride = staged_stride(a.d);
    a.tiles_x = (W - 1) / kTile + 1;
    a.tiles = (unsigned long long)a.tiles_x * (unsigned long long)((H - 1) / kTile + 1);
    const size_t lds = boundary_lds_bytes(a.d, n_maps * num_classes);
    static size_t lds_allowed = 0;
    if (lds > 65536 && lds > lds_allowed) {
        COSA_HIP_CHECK(hipFuncSetAttribute((const void *)boundary_scores_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_allowed = lds;
    }
    const unsigned blocks = (unsigned)(a.tiles < 1024 ? a.tiles : 1024);
    hipLaunchKernelGGL(boundary_scores_kernel, dim3(blocks), dim3(256), lds, as_stream(stream), a);
    COSA_LAUNCH_CHECK();
    return COSA_OK;
}
