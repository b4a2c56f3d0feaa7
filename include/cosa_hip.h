/*
 * cosa_hip.h -- C ABI of libcosa_hip.so: the MI355X (gfx950) implementation of CoSA's
 * per-iteration training hot path.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every *_dev / device entry point takes DEVICE pointers and a `void *stream`
 *     (a hipStream_t; NULL = the null stream), enqueues work and returns without
 *     synchronising.  Return value: COSA_OK or a COSA_E* code; cosa_last_error()
 *     gives the message for the calling thread.
 *   - tensors are dense row-major ("NCHW") float32 unless a parameter says otherwise.
 *   - workspaces are caller-allocated; *_workspace_bytes() tells the size.  Nothing in the
 *     launch path calls hipMalloc/hipFree/hipDeviceSynchronize (graph-capturable).
 *   - reference file:line citations are relative to the CoSA repository root.
 */
#ifndef COSA_HIP_H
#define COSA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COSA_OK 0
#define COSA_EINVAL 1   /* bad argument / unsupported shape            */
#define COSA_EHIP 2     /* a HIP runtime call failed                    */
#define COSA_ERANGE 3   /* lattice key left the packable range          */
#define COSA_ENOMEM 4   /* workspace too small                          */

int cosa_abi_version(void);
const char *cosa_last_error(void);

/* ---------------------------------------------------------------------------------------
 * utils/torch_helper.py:354-367  denormalize_img
 *   out = float(uint8(img*std+mean)) / 255      img,out [B,3,H,W]
 * ------------------------------------------------------------------------------------- */
int cosa_denormalize_img(const float *img, float *out, int B, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * utils/seg_helper.py:264-270  per-(b,c) plane  x -= min(x); x /= max(x) + 1e-5  (in place)
 *   cam [BC, HW]; `active` (optional, [BC]): planes whose entry is 0 are known all-zero and skipped
 * ------------------------------------------------------------------------------------- */
int cosa_cam_minmax_norm(float *cam, int BC, int HW, const float *active /* [BC] or NULL */, void *stream);
/* the same result bit for bit with a plane spread over several workgroups; workspace: 2 * BC unsigned ints of device memory */
int cosa_cam_minmax_norm_ws(float *cam, int BC, int HW, const float *active /* [BC] or NULL */, void *workspace, void *stream);

/* utils/seg_helper.py:247-250: F.interpolate(imgs, size, mode="bilinear", align_corners=False) of the teacher's input batch to the 0.5x / 1.5x
 * scales; src [planes, H, W] fp32 -> dst [planes, OH, OW] (ATen's formula incl. its fused source-index multiply-add: within 1 ulp of the image range of the CPU operator) */
int cosa_resize_bilinear(const float *src, float *dst, int planes, int H, int W, int OH, int OW, void *stream);
/* ---------------------------------------------------------------------------------------
 * utils/seg_helper.py:252-270  fused tail of multi_scale_camseg for ONE scale:
 *   up   = bilinear(src[2b,C,h,w] -> (S,S), align_corners=False)
 *   v    = mode 0: relu(max(up[:b], flip_w(up[b:])))          (cam / cam_aux, :253-258)
 *          mode 1: up[:b] + flip_w(up[b:])                    (seg,           :260-262)
 *   dst  = accumulate ? dst + v : v                           (sum over scales, :264,273)
 *   src [2*B, C, h, w]   dst [B, C, S, S]
 *   active (optional, the image-level labels): channels with active[b,c]==0 are written as 0 --
 *   what cam_validation (:547-551) makes of them one call later -- and cost nothing.
 * ------------------------------------------------------------------------------------- */
int cosa_cam_flip_merge_upsample(const float *src, float *dst, int B, int C, int h, int w, int S,
                                 int mode, int accumulate, const float *active /* [B,C] or NULL */, void *stream);
/* the same for a destination buffer that the previous call filled under the activity map prev_active [B*C]: planes absent then and now are
 * not touched (they are still zero) -- the training loop keeps its CAM buffers from step to step                                        */
int cosa_cam_flip_merge_upsample_reuse(const float *src, float *dst, int B, int C, int h, int w, int S, int mode, int accumulate,
                                       const float *active, const float *prev_active, void *stream);

/* ---------------------------------------------------------------------------------------
 * utils/seg_helper.py:721-797  cam2mask (+ _refine_cams), with cam_validation (:547-551)
 * folded in and, optionally, models/PAR.py:64-91 as the refine_model.
 *
 *   images  [B,3,S,S]  de-normalised image in [0,1] (read only when par_iters > 0)
 *   boxes   [B,4] int32 device (h0,h1,w0,w1)
 *   cams    [B,C,S,S]  cams; fold_validation=1: raw cams, multiplied by labels here
 *                      (cam_validation); 0: the caller already did (reference call order)
 *   labels  [B,C]      {0,1}
 *   mask    [B,S,S]    float32 out: {0..C, ignore_index}
 *   downscale 2 or 0;  par_iters 0 => refine_model=None;  dilations host int[n_dil]
 * ------------------------------------------------------------------------------------- */
size_t cosa_cam2mask_workspace_bytes(int B, int C, int S, int downscale, int n_dil);
int cosa_cam2mask(const float *images, const int32_t *boxes, const float *cams, const float *labels,
                  float *mask, int B, int C, int S, float thr_hi, float thr_lo, int downscale,
                  int fold_validation, const int *dilations, int n_dil, int par_iters, float ignore_index,
                  void *workspace, size_t workspace_bytes, void *stream);

/* The same for G CAM sets of the SAME images in one pass (the training step's two calls, main.py:137-166: main CAMs
 * and auxiliary CAMs with their own thresholds).  cams / masks: host arrays of G device pointers ([B,C,S,S] / [B,S,S]),
 * thr_hi / thr_lo: host float[G].  Bit-identical to G cosa_cam2mask calls; the affinities of the refine model are built
 * once and streamed once per propagation step for all sets.  thr_dev (optional): device float[G][2] = (hi, lo) per set,
 * read by the kernels instead of the host values -- the adaptive thresholds of main.py:138-151 without a host sync. */
size_t cosa_cam2mask_multi_workspace_bytes(int G, int B, int C, int S, int downscale, int n_dil);
int cosa_cam2mask_multi(const float *images, const int32_t *boxes, const float *const *cams, const float *labels,
                        float *const *masks, const float *thr_hi, const float *thr_lo, const float *thr_dev, int G, int B, int C,
                        int S,
                        int downscale, int fold_validation, const int *dilations, int n_dil, int par_iters,
                        float ignore_index, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * dataloaders/voc.py:262-275 `__transforms` (transforms.py:10-28,52-77,104-120,150-202; randaug.py:58-130) for a batch:
 * random_scaling -> random_fliplr -> random_crop -> GaussianBlur -> weak / OneOf(9 ops) strong -> ToTensor + Normalize,
 * with the random draws made by the caller (cosa_amd/dataloaders/augment.py: draw_params) and shipped as records.
 *   raw      device uint8: the decoded images, HWC, packed (record.raw_off = byte offset)
 *   records  device, B records of cosa_augment_record_bytes() bytes (26 int32, layout in csrc/aug_kernels.hip: AugImage)
 *   wimg, simg   device float32 [B,3,S,S] out;   crop_u8 / weak_u8 / strong_u8: optional device uint8 [B,S,S,3] stages
 * Bit-exact with Pillow's integer / fixed-point arithmetic (resize BILINEAR, GaussianBlur, ImageOps, ImageEnhance).
 * ------------------------------------------------------------------------------------- */
int cosa_augment_record_bytes(void);
size_t cosa_augment_workspace_bytes(int B, int S, int max_rows);
int cosa_augment_batch(const uint8_t *raw, const void *records, int B, int S, int max_rows, float *wimg, float *simg,
                       uint8_t *crop_u8, uint8_t *weak_u8, uint8_t *strong_u8, void *workspace, size_t workspace_bytes,
                       void *stream);
/* Ground-truth maps through the same geometry (--gt_stats): out[b][y][x] = map_b[src_y[y]][src_x[x]], or 255
 * where either table entry is -1 (or lies outside its map, or the map outside raw: nothing is read there).  raw: device uint8
 * [raw_bytes], the buffer the maps ride in;
 * maps: device int64 [B][3] = (byte offset of image b's [rows][pitch] uint8 map in raw, pitch, rows), 8-byte aligned; tables: device
 * int32 [B][2][S] = src_y | src_x (cosa_amd/dataloaders/augment.py: label_tables: Pillow's NEAREST resize, the flip, the padding and
 * the crop as one source row per output row and one source column per output column); out: device uint8 [B,S,S].  One launch.
 * Anything outside the envelope is COSA_EINVAL with nothing launched. */
int cosa_augment_labels(const uint8_t *raw, size_t raw_bytes, const long long *maps, const int32_t *tables, int B, int S, uint8_t *out,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * utils/seg_helper.py:924-943  rungmm -- the adaptive-threshold fit of main.py:138-151,174-184:
 * scikit-learn GaussianMixture(modal, weights 1/modal, means (min, median, max) | (min, max), precisions 1,
 * tol, reg_covar, max_iter).fit_predict on the queue samples above the filter threshold, then
 * max(samples of component 0) [and min(samples of component 2) for modal = 3].  One launch, float64, no host sync.
 *   sorted  device float64: the samples above the filter threshold in ascending order (positive)
 *   n_dev   device int64: how many of them (<= capacity)
 *   out     device float64[13]: [0] low threshold, [1] high threshold (NaN for modal 2), [2] EM iterations,
 *           [3] status bits (1: component 0 empty, 2: component 2 empty, 4: fewer samples than components,
 *           8: grid barrier expired), [4..] means, [7..] weights, [10..] 1/sigma
 * ------------------------------------------------------------------------------------- */
size_t cosa_gmm_workspace_bytes(void);
int cosa_gmm_fit_thresholds(const double *sorted, const long long *n_dev, long long capacity, int modal, double tol,
                            double reg_covar, int max_iter, double *out, void *workspace, size_t workspace_bytes,
                            void *stream);

/* ---------------------------------------------------------------------------------------
 * models/PAR.py:64-91  PAR.forward for a batch of same-sized images / mask stacks.
 *   imgs [B,3,h,w]   masks [B,K,h,w] (in)   out [B,K,h,w]
 * ------------------------------------------------------------------------------------- */
size_t cosa_par_workspace_bytes(int B, int K, int h, int w, int n_dil);
int cosa_par_forward(const float *imgs, const float *masks, float *out, int B, int K, int h, int w,
                     const int *dilations, int n_dil, int num_iter,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * utils/bilateralfilter/bilateralfilter.hpp:10-12 (SWIG module `bilateralfilter`,
 * bilateralfilter.i:21-25).  HOST-pointer drop-ins with the reference's exact argument list
 * (the SWIG typemaps turn each (ptr,len) pair into one NumPy array); they stage through the
 * GPU and synchronise.  `out(s)` is written in place.
 * ------------------------------------------------------------------------------------- */
void bilateralfilter(float *image, int len_image, float *in, int len_in, float *out, int len_out,
                     int H, int W, float sigmargb, float sigmaxy);
void bilateralfilter_batch(float *images, int len_images, float *ins, int len_ins, float *outs, int len_outs,
                           int N, int K, int H, int W, float sigmargb, float sigmaxy);

/* Device-resident form of the same filter (utils/bilateralfilter/permutohedral.cpp:115-297
 * init, :507-571 compute): images [N,3,H,W] (0..255), in/out [N,K,H,W].                     */
size_t cosa_bilateral_workspace_bytes(int N, int K, int H, int W);
int cosa_bilateralfilter_batch_dev(const float *images, const float *ins, float *outs,
                                   int N, int K, int H, int W, float sigmargb, float sigmaxy,
                                   int32_t *lattice_sizes /* [N] device, may be NULL */,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * utils/seg_helper.py:864-903  DenseEnergyLossFunction, device resident.
 *   forward:  Gate = clamp(ROI - max_k seg, 0); Gate[unlabel] = 1; segm = seg*ROI;
 *             AS = BF(images, segm) * Gate;  loss = -<segm, AS> / N
 *   backward: grad_seg = -2 * grad_out * AS / N * ROI
 *   images [N,3,H,W] 0..255, seg [N,K,H,W], roi [N,H,W], unlabel [N,H,W] uint8
 *   AS [N,K,H,W] out (kept for backward), loss: 1 float (device)
 * ------------------------------------------------------------------------------------- */
int cosa_dense_energy_forward(const float *images, const float *seg, const float *roi, const uint8_t *unlabel,
                              float *AS, float *loss, int N, int K, int H, int W,
                              float sigmargb, float sigmaxy,
                              void *workspace, size_t workspace_bytes, void *stream);
/* the forward in two halves, so that the image-only half overlaps the networks: `prepare` takes the NORMALISED strong image
 * [N,3,S,S], writes F.interpolate(denormalize_img(.), scale_factor=0.5) to s_img [N,3,S/2,S/2] and builds the lattice in
 * `workspace`; `forward_prepared` (H = W = S/2) runs the filter through it.  Same K and workspace for both calls.          */
int cosa_dense_energy_prepare(const float *simg, float *s_img, int N, int K, int S, float sigmargb, float sigmaxy,
                              void *workspace, size_t workspace_bytes, void *stream);
int cosa_dense_energy_forward_prepared(const float *seg, const float *roi, const uint8_t *unlabel, float *AS, float *loss,
                                       int N, int K, int H, int W, float sigmargb, float sigmaxy,
                                       void *workspace, size_t workspace_bytes, void *stream);
int cosa_dense_energy_backward(const float *AS, const float *roi, const float *grad_out /* 1 float, device */,
                               float *grad_seg, int N, int K, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * models/vit/vit.py:119-137  Attention core: softmax(q k^T * scale) v per head, fused (the
 * [B,H,N,N] score tensor is never materialised).  bf16 in/out, fp32 softmax and accumulation.
 *   qkv [B,N,3,H,64] bf16 (output of the qkv projection)   out [B,N,H*64] bf16
 *   lse [B,H,N] f32 (log-sum-exp of the scaled scores, kept for the backward pass)
 *   V is read in place (its V^T fragments come from the transposing LDS read): the workspace is a token 256 bytes and
 *   cosa_attn_prepare_vt a no-op, both kept for callers written against the earlier V^T-copy version; `flags` bits 8 / 9
 *   force 4 / 2 waves per workgroup (default: by the number of rounds, attn_kernels.hip); bit 10 marks a pass WITHOUT backward (the
 *   teacher's / evaluation's torch.no_grad() calls of the same module): the kernel may then hold q pre-multiplied by scale * log2(e) in
 *   the operand type and feed the softmax's running maximum through the score MFMAs (one more rounding of q; lse is the log of the sum of
 *   the ROUNDED probabilities); the other bits are ignored.
 * ------------------------------------------------------------------------------------- */
size_t cosa_attn_workspace_bytes(int B, int N, int H);
int cosa_attn_prepare_vt(const void *qkv, int B, int N, int H, void *workspace, size_t workspace_bytes, void *stream);
int cosa_attn_fwd(const void *qkv, void *out, float *lse, int B, int N, int H, int head_dim, float scale,
                  int flags, uint64_t *stamps /* NULL, or 64 x {min start, max end} 100 MHz device ticks of this launch (workgroup id & 63 picks the pair) */,
                  void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the same attention (autograd of vit.py:128-134): dqkv [B,N,3,H,64] bf16 from
 * dout [B,N,H*64]; P is recomputed from lse, nothing of size N^2 touches HBM; no atomics
 * (one kernel owns query blocks for dQ, one owns key blocks for dK/dV); K^T / Q^T / dO^T operands come
 * from transposing LDS reads of the row-major tiles (no transposed copies): the workspace only holds
 * delta = rowsum(dO * O), [B,H,N] fp32.                                                        */
size_t cosa_attn_bwd_workspace_bytes(int B, int N, int H);
int cosa_attn_bwd(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv,
                  int B, int N, int H, int head_dim, float scale, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * models/vit/vit.py:96-102,119-137,154-158  the nn.Linear projections of a ViT block with their
 * element-wise tails fused:   Y = X[M,K] * W[N,K]^T + bias[N]   (bf16 operands, fp32 accumulate)
 *   epilogue 0: Y bf16                      (attn.qkv)
 *   epilogue 1: Y bf16 = gelu_erf(.)        (mlp.fc1 + nn.GELU)
 *   epilogue 2: Y fp32 = residual fp32 + .  (attn.proj / mlp.fc2 + the block's residual add;
 *                                            Y may alias residual)
 *   N % 128 == 0, K % 64 == 0.
 * cosa_layernorm: nn.LayerNorm(768, eps) over the fp32 residual stream -> bf16 (and/or fp32).
 * ------------------------------------------------------------------------------------- */
int cosa_gemm_bf16(const void *X, const void *W, const void *bias, const float *residual, void *Y,
                   int M, int N, int K, int epilogue, void *stream);
/* weight (and bias) gradient of the same Linear: dW[N,K] (fp32) = (zero_first ? 0 : dW) + dY[M,N]^T X[M,K]  (bf16 operands);
 * db[N] (fp32, optional) = (zero_first ? 0 : db) + column sums of dY.  N % 128 == 0, K % 128 == 0.  Deterministic: the token range is
 * split over workgroups, every split writes an fp32 partial slab into `workspace` (cosa_gemm_wgrad_workspace_bytes) and a second
 * kernel adds the slabs in split order -- no float atomics, the same bits every run.                                           */
size_t cosa_gemm_wgrad_workspace_bytes(int M, int N, int K);
int cosa_gemm_wgrad_bf16(const void *dY, const void *X, float *dW, float *db, int M, int N, int K, int zero_first,
                         void *workspace, size_t workspace_bytes, void *stream);
/* The same weight / bias gradients for MANY linears that share M, in one persistent launch (the student's encoder: autograd of
 * models/vit/vit.py:96-137 for all twelve blocks, launched when the backward pass has produced every dY).  With hundreds of 256 x 128 tiles
 * no item needs split-K: every tile runs the whole token loop and writes dW (and db) once -- overwritten, never accumulated; no workspace,
 * no atomics, the same bits every run.  `items`: host array, read during the call.                                                        */
typedef struct CosaWgradItem { const void *dY, *X; float *dW, *db; int N, K; } CosaWgradItem;
int cosa_gemm_wgrad_batched(const CosaWgradItem *items, int n_items, int M, void *stream);
/* The weight / bias gradient of the patch projection when K % 128 != 0 (an 8-pixel-patch ViT: [768, 3*8*8]): dW[N,K] and db[N] (optional)
 * OVERWRITTEN with dY[M,N]^T X[M,K] and the column sums of dY (bf16 operands, 16-byte aligned).  N % 64 == 0, K % 64 == 0.  Rows split over
 * workgroups, fp32 partial slabs in `workspace` (cosa_patch_wgrad_workspace_bytes) added in slab order: deterministic (loss_kernels.hip). */
size_t cosa_patch_wgrad_workspace_bytes(int M, int N, int K);
int cosa_patch_wgrad_bf16(const void *dY, const void *X, float *dW, float *db, int M, int N, int K, void *workspace, size_t workspace_bytes,
                          void *stream);
/* models/decoder/conv_head.py:11-41  LargeFOV's 3x3 dilated, bias-free convolution on NHWC tokens (implicit GEMM, optional ReLU):
 *   X: image b = rows [b*img_rows + row_off, +h*w) of a [*, ldx] bf16 matrix (so the token tensor minus its cls row needs no copy)
 *   Wt [9][Cout][Cin] bf16 (tap-major: t = ky*3 + kx);  Y [B*h*w, Cout] bf16;  padding = dilation                               */
int cosa_conv3x3_dilated_nhwc(const void *X, const void *Wt, void *Y, int B, int h, int w, int Cin, int Cout, int dilation,
                              int img_rows, int row_off, int ldx, int relu, void *stream);
/* its weight gradient (autograd of the same conv): dW9 [Cout][9*Cin] fp32, tap-major columns (t*Cin + c), = (zero_first ? 0 : dW9) +
 * dY[B*h*w, Cout]^T im2col(X), the im2col implicit in the operand addressing; X is addressed as in the forward call.
 * (The input gradient is the forward entry point itself on dY with Wt'[t][c][o] = Wt[8-t][o][c].)                              */
int cosa_conv3x3_dilated_wgrad(const void *dY, const void *X, float *dW9, int B, int h, int w, int Cin, int Cout, int dilation,
                               int img_rows, int row_off, int ldx, int zero_first, void *workspace, size_t workspace_bytes,
                               void *stream);      /* workspace: cosa_gemm_wgrad_workspace_bytes(B*h*w, Cout, 9*Cin) */
void cosa_gemm_set_variant(int v);   /* 0 (default): per-shape choice; 1: the 128x128 two-stage kernel; 6: the persistent 256x256 kernel;
                                      * 9: the same on 256x192 jobs; 7 / 8 / 61-65: store-policy and timing variants of it (tools/) */
/* persistent-grid policy of cosa_gemm_bf16: 0 (default) one workgroup per CU; 1 the workgroups balanced over the rounds the launch needs
 * anyway (600 jobs: 200 workgroups x 3 instead of 256 x 2.3; launches of fewer than 40 000 rows, i.e. the student's), which leaves CUs to
 * concurrently running kernels -- RCCL's channels when the
 * process is one rank of a data-parallel job (utils/misc.py:439 init_distributed_mode + main.py:49-50 DDP)                              */
void cosa_gemm_set_grid_policy(int balanced);
void cosa_gemm_set_grid_policy_f16(int balanced);
/* measurement hook: the NEXT cosa_gemm_bf16 launch (persistent 256x256 kernel only) writes its device-clock span
 * (100 MHz s_memrealtime: min start / max end over workgroups) to 64 pairs slot[2s], slot[2s + 1] (uint64, s = workgroup id & 63,
 * caller-initialised to max / 0: the span is the min over the starts and the max over the ends).
 * One-shot; used by bench.py because HIP events cannot be recorded inside a captured hipGraph.                       */
void cosa_gemm_set_stamp_slot(void *slot);
/* vit.py:254-262 (PatchEmbed: stride-16 conv) as a GEMM needs the image as im2col rows; the teacher's passes run every scale as
 * cat(x, x.flip(-1)) (seg_helper.py:241-246).  cols [flips*B*(H/P)*(W/P), C*P*P] in a 16-bit type (dtype 1 = bf16, 2 = fp16) from
 * x [B,C,H,W] fp32: rows of the images first, then (flips = 2) of their horizontal mirror images.  P % 8 == 0, P | H, P | W.
 * dtype 3: the rows as fp16c8 operand rows (hi fp16 | lo8 | hi8 | aug = (1, 1, 0, ...), 4*C*P*P + 128 bytes each; see cosa_c8_rows).    */
int cosa_im2col_flip(const float *x, void *cols, int B, int C, int H, int W, int P, int flips, int dtype, void *stream);
/* the dtype-3 form writing into a token matrix with cls_rows free rows in front of every image's patch rows (kept zero by the caller): the
 * patch projection's fp32 residual epilogue then produces the residual stream [images, 1 + n, D] in place, without concatenations */
int cosa_im2col_flip_c8_tokens(const float *x, void *rows, int B, int C, int H, int W, int P, int flips, int cls_rows, void *stream);
/* the same token-shaped operand as split rows (hi | lo | aug = (1, 1, 0, ...); bf16 halves, `_f16`: fp16 halves) for the three-term (bf16x3 /
 * fp16x3) patch projection: rows [flips * B * (h*w + cls_rows), 2 C P P + 64], class-token rows untouched (vit.py:254-262, seg_helper.py:241-246) */
int cosa_im2col_flip_split_tokens(const float *x, void *rows, int B, int C, int H, int W, int P, int flips, int cls_rows, void *stream);
int cosa_im2col_flip_split_tokens_f16(const float *x, void *rows, int B, int C, int H, int W, int P, int flips, int cls_rows, void *stream);
/* vit.py:303-313 (prepare_tokens: cat(cls_token, patch tokens) + interpolated pos_embed) for the no-grad passes, written straight into
 * the fp32 residual stream: out [B, n+1, D] = (cls [D] | tok [B, n, D]) + pos [n+1, D]; tok / cls / pos share one 16-bit type
 * (dtype 1 = bf16, 2 = fp16), each sum is rounded to that type before it is widened (the 16-bit torch expression's value); D % 8 == 0. */
int cosa_embed_finish(const void *tok, const void *cls, const void *pos, float *out, int B, int n, int D, int dtype, void *stream);
/* models/__init__.py:190-192 (classifier / aux_classifier as 1x1 convs over the tokens) and conv_head.py:38 (conv8): the narrow heads
 * Y[M, N] (fp32, columns [col0, col0+N) of rows with stride ldy; N of a few dozen rows, slices of 32 inside the kernel) = X W^T, fp32
 * accumulation, fixed reduction order per row
 * (results do not depend on what else is in the batch).  X: image b = rows_per_img rows at X + b*img_stride (elements), row stride
 * ldx; dtype 0: fp32 X and W, 1: bf16, 2: fp16 X and W (round_bf16 = 1 rounds the result to the operand precision).                               */
int cosa_head_gemm(const void *X, const void *W, float *Y, int M, int N, int K, int rows_per_img, long long img_stride,
                   int ldx, int dtype, int round_bf16, int ldy, int col0, void *stream);
/* autograd of the same heads (the reference trains them through torch autograd: models/__init__.py:190-204, conv_head.py:38).
 * dX [M,K] bf16 = dY [M,N] (fp32, contiguous) W [N,K] (bf16);  dW [N,K] fp32 = dY^T X (X [M,K] bf16, contiguous), summed in a fixed
 * order (workspace: cosa_head_gemm_wgrad_workspace(M, K) bytes of device memory).  K % 128 == 0; the weight gradient takes N <= 32
 * rows per call (wider heads in slices).                                                                                          */
int cosa_head_gemm_dgrad(const float *dY, const void *W, void *dX, int M, int N, int K, void *stream);
size_t cosa_head_gemm_wgrad_workspace(int M, int K);
int cosa_head_gemm_wgrad(const float *dY, const void *X, float *dW, void *workspace, int M, int N, int K, void *stream);
int cosa_layernorm(const float *x, const void *gamma, const void *beta, void *y_bf16, float *y_f32,
                   int rows, int dim, float eps, void *stream);
/* the student's training path (autograd of models/vit/vit.py:96-102,119-137) on the same GEMM kernels:
 *   cosa_gemm_bf16_dual_gelu    mlp.fc1 forward: H = X W^T + b (bf16, kept for GELU') and A = gelu_erf(H) (bf16) from one pass
 *   cosa_gelu_backward          dH = dA * gelu_erf'(H) (bf16, n % 8 == 0)
 *   cosa_transpose_cast_batched bf16 W^T shadows of the fp32 master weights (one launch for all tensors): the input gradient
 *                               dX = dY W is then cosa_gemm_bf16(dY, W^T, zeros) -- the forward kernel, no second GEMM family   */
/* dst [B][n] fp32 = src [n] for every b (n % 4 == 0): the fp32 token stream of a no-grad pass starts as (cls + pos_0 | pos rows) per image,
 * models/vit/vit.py:283-300; the patch projection then adds into it in place */
int cosa_broadcast_rows(const float *src, float *dst, int B, long long n, void *stream);
/* vit.py:288-291: bicubic resize of the frozen 14 x 14 position grid to the token grid as a 16-tap gather (idx / wgt [P,16]: the non-zero
 * entries of the interpolation matrix's rows): out[P, D] fp32 = sum_t wgt[p][t] * pe[idx[p][t]][:]                                 */
int cosa_pos_resize(const float *pe, const int *idx, const float *wgt, float *out, int P, int D, void *stream);
int cosa_gemm_bf16_dual_gelu(const void *X, const void *W, const void *bias, void *H, void *A, int M, int N, int K, void *stream);
int cosa_gelu_backward(const void *dA, const void *H, void *dH, long long n, void *stream);
size_t cosa_transpose_record_bytes(void);
int cosa_transpose_cast_batched(const void *records, int n, int total_tiles, void *stream);

/* The same kernels with IEEE fp16 operands (fp32 accumulation, same MFMA rate; gemm_kernels.hip / attn_kernels.hip built a second
 * time with -DCOSA_OP_F16=1): the no-grad passes -- the teacher's six multi-scale forwards per step (utils/seg_helper.py:232-275) and
 * evaluation -- may run on fp16 operands, which keeps the pseudo-label maps within the stated tolerance of the fp32 reference where
 * bf16's 8 significant bits do not.  Argument lists are those of the bf16 entry points, every "bf16" buffer
 * being fp16 instead.                                                                                                            */
int cosa_gemm_f16(const void *X, const void *W, const void *bias, const float *residual, void *Y,
                  int M, int N, int K, int epilogue, void *stream);
int cosa_gemm_wgrad_f16(const void *dY, const void *X, float *dW, float *db, int M, int N, int K, int zero_first,
                        void *workspace, size_t workspace_bytes, void *stream);
int cosa_layernorm_f16(const float *x, const void *gamma, const void *beta, void *y_f16, float *y_f32,
                       int rows, int dim, float eps, void *stream);
int cosa_conv3x3_dilated_nhwc_f16(const void *X, const void *Wt, void *Y, int B, int h, int w, int Cin, int Cout, int dilation,
                                  int img_rows, int row_off, int ldx, int relu, void *stream);
int cosa_conv3x3_dilated_wgrad_f16(const void *dY, const void *X, float *dW9, int B, int h, int w, int Cin, int Cout, int dilation,
                                   int img_rows, int row_off, int ldx, int zero_first, void *workspace, size_t workspace_bytes,
                                   void *stream);
void cosa_gemm_set_variant_f16(int v);
void cosa_gemm_set_stamp_slot_f16(void *slot);
size_t cosa_attn_workspace_bytes_f16(int B, int N, int H);
int cosa_attn_prepare_vt_f16(const void *qkv, int B, int N, int H, void *workspace, size_t workspace_bytes, void *stream);
int cosa_attn_fwd_f16(const void *qkv, void *out, float *lse, int B, int N, int H, int head_dim, float scale,
                      int flags, uint64_t *stamps, void *workspace, size_t workspace_bytes, void *stream);
size_t cosa_attn_bwd_workspace_bytes_f16(int B, int N, int H);
int cosa_attn_bwd_f16(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv,
                      int B, int N, int H, int head_dim, float scale, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * bf16x3 ("split") operands: the parity-grade precision of the no-grad passes (teacher pseudo-labels, utils/seg_helper.py:232-275;
 * evaluation).  The reference runs fp32; bf16's 8 significant bits put the normalised CAMs ~1e-2 and the label maps
 * ~0.2 % away from it at 448^2, so every MFMA operand of these passes can instead be carried as hi = bf16(v), lo = bf16(v - hi)
 * (16 significant bits) with three MFMA terms per product (hi*hi + lo*hi + hi*lo) and fp32 accumulation -- still bf16 MFMA, 3x the
 * work.  A split row of logical width K is [hi (K) | lo (K) | aug (64)], row stride 2K + 64; aug = (1, 1, 0, ...) for activations and
 * (bias_hi, bias_lo, 0, ...) for weight row n, so nn.Linear's bias rides in the GEMM as one more K tile.
 *   cosa_split_rows       src fp32 [R, K] (row stride src_ld) (+ bias fp32 [R] | ones) -> dst split rows [R, 2K + 64]
 *   cosa_layernorm_split  nn.LayerNorm(768, eps), fp32 gamma / beta, over the fp32 residual stream -> split rows and/or fp32
 *   cosa_gemm_bf16x3      Y = Xs Ws^T (bias inside Ws): epilogue 0 / 1 (GELU): Y bf16 [M, ldy >= 2N] = [hi | lo]; epilogue 2: Y fp32
 *                         [M, N] = residual + . (may alias);  zeros: N bf16 zeros (the kernels' bias operand)
 *   cosa_attn_fwd_bf16x3  attention on the split qkv rows [B*N, ldq] = [hi (3*H*64) | lo ...] -> split rows [B*N, ldo >= 2*H*64 + 64]
 *                         for the output projection; lse optional
 * ------------------------------------------------------------------------------------- */
int cosa_split_rows(const float *src, const float *bias, void *dst, int R, int K, long long src_ld, int ones, void *stream);
int cosa_layernorm_split(const float *x, const float *gamma, const float *beta, void *y_split, float *y_f32, int rows, int dim,
                         float eps, void *stream);
int cosa_gemm_bf16x3(const void *Xs, const void *Ws, const void *zeros, const float *residual, void *Y,
                     int M, int N, int K, int epilogue, int ldy, void *stream);
int cosa_attn_fwd_bf16x3(const void *qkv_split, void *out_split, float *lse, int B, int N, int H, int head_dim, float scale,
                         int ldq, int ldo, uint64_t *stamps /* optional device-clock span of the launch, as cosa_attn_fwd */, void *stream);
/* fp16x3 (round 6): the same four entry points with hi = fp16(v), lo = fp16(v - hi) halves -- 11 + 11 significant bits (a lo half below 2^-14
 * is an fp16 subnormal: an absolute 2^-24), three fp16 MFMA terms, same cost as bf16x3 and ~10x closer to the fp32 reference
 * (tools/sim_precision_map.py scheme `hh`).  Same layouts with fp16 halves; the attention carries its probabilities scaled by 2^10 so that
 * their lo halves stay normal numbers (the factor cancels in O / l).  Teacher mode string: "fp16x3". */
int cosa_split_rows_f16(const float *src, const float *bias, void *dst, int R, int K, long long src_ld, int ones, void *stream);
int cosa_layernorm_split_f16(const float *x, const float *gamma, const float *beta, void *y_split, float *y_f32, int rows, int dim,
                             float eps, void *stream);
int cosa_gemm_f16x3(const void *Xs, const void *Ws, const void *zeros, const float *residual, void *Y,
                    int M, int N, int K, int epilogue, int ldy, void *stream);
int cosa_attn_fwd_f16x3(const void *qkv_split, void *out_split, float *lse, int B, int N, int H, int head_dim, float scale,
                        int ldq, int ldo, uint64_t *stamps, void *stream);

/* ---------------------------------------------------------------------------------------
 * "f32" operands (csrc/f32_kernels.hip; teacher mode string "fp32"): the no-grad passes in the reference's own
 * arithmetic (models/vit/vit.py:96-137, models/decoder/conv_head.py:32-41 run fp32) -- every operand fp32, read from the fp32 masters, every
 * product on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain).  1/16 of the 16-bit MFMA rate.
 *   cosa_gemm_f32             Y[M, N] (row stride ldy) = X[M, K] (ldx) W[N, K]^T (ldw); epilogue 0: + bias, 1: + bias then erf-form GELU
 *                             (erff), 2: + bias + residual (fp32, row stride ldr; may alias Y).  bias may be null (none).  Every output
 *                             element is ONE fma chain over ascending k starting from zero, the epilogue applied afterwards in fp32: no
 *                             split-K, no atomics, no dependence on M, on the row's position or on the other rows.  Envelope: M >= 1 (tail
 *                             rows guarded), N % 64 == 0, K % 16 == 0, ldx / ldw % 4 == 0 on 16-byte aligned bases; anything else is
 *                             COSA_EINVAL and nothing is launched.
 *   cosa_conv3x3_dilated_f32  Y[B*h*w, Cout] = relu?(conv3x3(tokens, dilation d, zero padding d, no bias)) as an implicit GEMM on the same
 *                             kernel: tokens NHWC, image b at tok + b * img_rows * ldx, pixel rows of stride ldx; Wt [Cout, 9 * Cin] tap-major
 *                             (ky, kx, cin).  Per output element one chain over (tap, cin) ascending, a padded tap contributing exact zeros:
 *                             independent of the batch.  Cin % 16 == 0, Cout % 64 == 0.
 *   cosa_attn_fwd_f32         out [B, N, H*64] (token stride ldo) = softmax(q k^T * scale) v on fp32 qkv [B, N, 3, H, 64] (token stride ldq: a
 *                             row slice of the packed buffer); scores, max-subtracted expf, row sums and P V in fp32 on the f32 MFMA, key
 *                             tiles of 32 through LDS, tail keys masked; a (batch, head) slice's result depends on that slice alone.  N >= 1.
 *   cosa_layernorm_f32out     nn.LayerNorm(768, eps), fp32 in / gamma / beta / out: cosa_layernorm_split's y_f32 by-product alone, same bits
 *   cosa_im2col_flip_f32_tokens  cosa_im2col_flip_split_tokens with plain fp32 rows [flips * B * (h*w + cls_rows), C P P]; P % 4 == 0
 * ------------------------------------------------------------------------------------- */
int cosa_gemm_f32(const float *X, const float *W, const float *bias, const float *residual, float *Y, int M, int N, int K, int ldx, int ldw,
                  int ldr, int ldy, int epilogue, void *stream);
int cosa_conv3x3_dilated_f32(const float *tok, const float *Wt, float *Y, int B, int h, int w, int Cin, int Cout, int dilation, int img_rows,
                             int ldx, int relu, void *stream);
int cosa_attn_fwd_f32(const float *qkv, float *out, int B, int N, int H, int head_dim, float scale, int ldq, int ldo, void *stream);
int cosa_layernorm_f32out(const float *x, const float *gamma, const float *beta, float *y_f32, int rows, int dim, float eps, void *stream);
int cosa_im2col_flip_f32_tokens(const float *x, float *rows, int B, int C, int H, int W, int P, int flips, int cls_rows, void *stream);

/* ---------------------------------------------------------------------------------------
 * "f64" operands (csrc/f64_kernels.hip; mode string "fp64"): the no-grad passes in float64 on the f64 MFMA
 * (v_mfma_f64_16x16x4_f64), from the input rescale to the normalised CAM -- the float64 side of the criterion's exemption leg on the device.
 * A check mode, never a training teacher.  Weights are the fp32 masters, widened as the kernels read them (w_is_f32) or float64 rows.
 *   cosa_gemm_f64             Y[M, N] (ldy) = X[M, K] (ldx, float64) W[N, K]^T (ldw; W and bias fp32 with w_is_f32, else float64); epilogue 0:
 *                             + bias, 1: + bias then erf-form GELU (double erf), 2: + bias + residual (float64, ldr; may alias Y).  bias may
 *                             be null.  Every output element is ONE accumulator of the MFMA, fed the products of ascending k in steps of 4
 *                             from zero, the epilogue applied afterwards in float64: no split-K, no atomics, no dependence on M, on the row's
 *                             position or on the other rows (NaN and 1e300 rows included).  |err| <= gamma_{K+2} (sum |x||w| + |bias| + |res|)
 *                             with u = 2^-53.  Envelope: M >= 1, N >= 1 (tail rows and columns guarded: the head widths 20, 21, 80, 81
 *                             directly), K % 16 == 0, ldx % 2 == 0, ldw % 4 (fp32) or % 2 (float64) == 0 on 16-byte aligned bases; anything
 *                             else is COSA_EINVAL and nothing is launched.
 *   cosa_conv3x3_dilated_f64  cosa_conv3x3_dilated_f32's implicit GEMM on that kernel: K = 9 * Cin, a stage never straddles a tap (Cin % 16
 *                             == 0), padded taps contribute exact zeros, ReLU fused; Wt [Cout, 9 * Cin] tap-major
 *   cosa_attn_fwd_f64         cosa_attn_fwd_f32 in float64: queries in blocks of 64, key tiles of 16 through LDS, exp in double, tail keys
 *                             masked; a (batch, head) slice's result depends on that slice alone.  head_dim 64, N >= 1.
 *   cosa_layernorm_f64        nn.LayerNorm(dim, eps) over contiguous float64 rows with the fp32 gamma / beta: two-pass mean and variance
 *   cosa_im2col_flip_f64_tokens  cosa_im2col_flip_f32_tokens on float64 images: a selection, exact
 *   cosa_resize_bilinear_f64  F.interpolate(x.double(), (OH, OW), "bilinear", align_corners=False): fp32 planes in, float64 planes out
 *   cosa_cam_flip_merge_upsample_f64  cosa_cam_flip_merge_upsample on float64 maps (modes 0 / 1, accumulate, active [B*C] fp32 or null);
 *                             rawmax [B*C] or null: (+)= max |src| over a plane and its mirror image's plane, accumulated like dst
 *   cosa_cam_minmax_norm_f64  x = (x - min) / (max(x - min) + 1e-5) per plane in place; peak [BC] or null: that divisor
 * ------------------------------------------------------------------------------------- */
int cosa_gemm_f64(const double *X, const void *W, const void *bias, const double *residual, double *Y, int M, int N, int K, int ldx, int ldw,
                  int ldr, int ldy, int epilogue, int w_is_f32, void *stream);
int cosa_conv3x3_dilated_f64(const double *tok, const void *Wt, double *Y, int B, int h, int w, int Cin, int Cout, int dilation, int img_rows,
                             int ldx, int relu, int w_is_f32, void *stream);
int cosa_attn_fwd_f64(const double *qkv, double *out, int B, int N, int H, int head_dim, double scale, int ldq, int ldo, void *stream);
int cosa_layernorm_f64(const double *x, const float *gamma, const float *beta, double *y, int rows, int dim, double eps, void *stream);
int cosa_im2col_flip_f64_tokens(const double *x, double *rows, int B, int C, int H, int W, int P, int flips, int cls_rows, void *stream);
int cosa_resize_bilinear_f64(const float *src, double *dst, int planes, int H, int W, int OH, int OW, void *stream);
int cosa_cam_flip_merge_upsample_f64(const double *src, double *dst, int B, int C, int h, int w, int S, int mode, int accumulate,
                                     const float *active, double *rawmax, void *stream);
int cosa_cam_minmax_norm_f64(double *cam, int BC, int HW, const float *active, double *peak, void *stream);

/* ---------------------------------------------------------------------------------------
 * The CAM criterion per plane (csrc/conformance_kernels.hip; DESIGN.md sections 3 and 20).  camA (the mode under test) and cam32 (the "fp32"
 * pass) fp32 [planes, HW], cam64 float64, active [planes] fp32 or null, peak64 / rawmax64 [planes] float64 from the float64 pass.  One
 * workgroup per plane, fixed reduction tree.  fig [planes, COSA_CONFORMANCE_FIGS] float64 = d = max |A - c32|, lit = d / max(max |c32|, 1e-6),
 * cond = rawmax / peak, own = d peak / max(rawmax, 1e-30), e_ref = max |c32 - c64|, e_hip = max |A - c64|, bound = cam_bar + fp64_factor
 * e_ref, max |c32|; verdict [planes, 2] int32 = (-1 inactive | 0 ok: lit <= cam_bar | 1 exempt: cond > cond_max and own <= cam_bar and
 * e_hip <= bound | 2 fail, also any plane of A with a non-finite element), count of non-finite elements of A.
 * ------------------------------------------------------------------------------------- */
#define COSA_CONFORMANCE_FIGS 8
int cosa_conformance_planes(const float *camA, const float *cam32, const double *cam64, const float *active, const double *peak64,
                            const double *rawmax64, int planes, int HW, double cam_bar, double cond_max, double fp64_factor, double *fig,
                            int *verdict, void *stream);

/* ---------------------------------------------------------------------------------------
 * utils/seg_helper.py:961-996 (DenseCRF / crf_inference_infv2, final evaluation only): the position-only Gaussian kernel of the dense
 * CRF -- pydensecrf's addPairwiseGaussian: features (x / sxy, y / sxy) -- as a permutohedral-lattice filter on a 2-D lattice (the lattice
 * kernels of the bilateral filter, csrc/permuto_kernels.hip, compiled a second time with -DCOSA_PD=2).  ins / outs [N, K, H, W] fp32.
 * The bilateral kernel of the CRF is cosa_bilateralfilter_batch_dev itself; the mean-field update around the two filters is host code
 * (cosa_amd/utils/seg_helper.py: DenseCRF).  pydensecrf is not under the reference tree: parity of this row is unpinned (oracle/crf_oracle.py).
 * ------------------------------------------------------------------------------------- */
/* the lattice's own stable LSD radix sort of (key, value) pairs by the low `bits` bits of the key (csrc/radix_sort.hpp; exported for the tests) */
size_t cosa_radix_sort_workspace_bytes(long long n);
int cosa_radix_sort_pairs(uint32_t *keys_in, uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out, long long n, int bits,
                          void *workspace, size_t workspace_bytes, void *stream);
size_t cosa_lattice_filter_d2_workspace_bytes(int N, int K, int H, int W);
int cosa_lattice_filter_d2(const float *ins, float *outs, int N, int K, int H, int W, float sigmaxy, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * fp16c8 operands: the parity-grade precision of the no-grad passes at 2x (not 3x) the MFMA work of the 16-bit path
 * (teacher pseudo-labels, utils/seg_helper.py:232-275; replaces the fp32 arithmetic of models/vit/vit.py:96-137 on the no-grad path).
 * A value v is carried as hi = fp16(v) plus two e5m2 bytes: hi8 = e5m2(hi) and lo8 = e5m2((v - hi) * 2^11); a product is
 * x_hi w_hi (fp16 MFMA) + 2^-11 (x_lo8 w_hi8 + x_hi8 w_lo8) (block-scaled 8-bit MFMA, K = 128 per instruction, twice the fp16 rate; the
 * 2^-11 is the instruction's E8M0 scale).  e5m2 has fp16's exponent range: no per-tensor statistics or scales exist.  A c8 row of logical
 * width K is, in bytes, [hi fp16 (2K) | lo8 (K) | hi8 (K) | aug fp16 (128)], row stride 4K + 128 (= the bf16x3 stride); aug = (1, 1, 0, ...)
 * for activations and (bias_hi, bias_lo, 0, ...) for weight row n (the bias rides in the GEMM as one more fp16 K tile).
 *   cosa_c8_rows          src fp32 [R, K] (row stride src_ld) (+ bias fp32 [R] | ones) -> dst c8 rows; K % 128 == 0
 *   cosa_layernorm_c8     nn.LayerNorm(768, eps), fp32 gamma / beta, over the fp32 residual stream -> c8 rows and/or fp32
 *   cosa_gemm_f16c8       Y = Xs Ws^T (bias inside Ws); N % 256 == 0, K % 128 == 0.  epilogue 0: Y fp16 [M, ldy >= N] (plain: the
 *                         qkv projection feeds the fp16 attention kernel); 1 (GELU): Y = c8 rows [M, ldy = 2N + 64 fp16 units], hi | lo8 |
 *                         hi8 written, the augmentation block left to the caller; 2: Y fp32 [M, N] = residual + . (may alias);
 *                         zeros: N fp16 zeros (the kernel's unused bias operand)
 *   cosa_attn_fwd_f16c8   attention on plain fp16 qkv rows [B, N, 3, H, 64] -> c8 rows [B*N, 4*H*64 + 128 bytes] (incl. the augmentation
 *                         block) for the c8 output projection; lse optional
 * ------------------------------------------------------------------------------------- */
int cosa_c8_rows(const float *src, const float *bias, void *dst, int R, int K, long long src_ld, int ones, void *stream);
size_t cosa_c8_record_bytes(void);       /* { const float *src; const float *bias; void *dst; int rows, K, row0, qrows; }: the first qrows rows and bias
                                          * entries are multiplied by 64^-0.5 log2(e) first (the q third of a qkv projection, for cosa_attn_fwd_f16c8
                                          * called with scale = ln 2: the attention scale folded into the weights, no extra rounding of q) */
int cosa_c8_rows_batched(const void *records /* device */, int n_records, int total_rows, void *stream);   /* all weight matrices, one launch */
int cosa_layernorm_c8(const float *x, const float *gamma, const float *beta, void *y_c8, float *y_f32, int rows, int dim,
                      float eps, void *stream);
int cosa_gemm_f16c8(const void *Xs, const void *Ws, const void *zeros, const float *residual, void *Y,
                    int M, int N, int K, int epilogue, int ldy, void *stream);
int cosa_attn_fwd_f16c8(const void *qkv, void *out_c8, float *lse, int B, int N, int H, int head_dim, float scale,
                        uint64_t *stamps, void *stream);

/* ---------------------------------------------------------------------------------------
 * fp16c4 operands (round 4; csrc/c4.hpp): the fp16c8 scheme with FP4 (e2m1) correction terms in MX blocks -- both terms
 * 2^-11 (x_lo' w_hi + x_hi w_lo') in ONE stream of block-scaled MFMAs at 4x the fp16 rate (e5m2: 2x): ~1.58x instead of ~2.08x the MFMA work
 * of the plain 16-bit path at K = 768.  Same purpose and call sites as fp16c8 (the teacher's no-grad projections, models/vit/vit.py:96-137).
 * A c4 operand is a PAIR: rows [R][4K + 128 bytes] = [hi fp16 (2K) | 16-byte blocks (K) | unused (K) | aug fp16 (128)] -- the c8 stride; a
 * block holds the 16 lo' = (v - hi) 2^11 and the 16 hi copies of 16 consecutive features as e2m1 nibbles ([lo' | hi] for activations,
 * [hi | lo'] for weights) -- and a scale tensor of cosa_c4_scale_bytes(R, K) bytes with one E8M0 byte per block (smallest 2^e with
 * amax / 2^e <= 6; weights carry the 2^-11), laid out per 256-row panel and 128-feature tile as the GEMM's lanes read it (c4.hpp).  K % 256 == 0.
 *   cosa_c4_rows          src fp32 [R, K] (+ bias fp32 [R] | ones) -> rows + scales; weight != 0: weight block order / scale bias
 *   cosa_c4_rows_batched  the weight matrices of a network in one launch ({src, bias, dst, scales, rows, K, row0, qrows} records; qrows as for cosa_c8_rows_batched)
 *   cosa_layernorm_c4     nn.LayerNorm(768, eps), fp32 gamma / beta, over the fp32 residual stream -> c4 rows + scales and/or fp32
 *   cosa_gemm_f16c4       Y = Xs Ws^T (bias inside Ws); N % 256 == 0.  epilogue 0: Y fp16 [M, ldy >= N]; 1 (GELU): Y = c4 rows [M, ldy = 2N + 64
 *                         fp16 units] + Yscales (activation layout; the augmentation block left to the caller); 2: Y fp32 [M, N] = residual + .
 * ------------------------------------------------------------------------------------- */
size_t cosa_c4_scale_bytes(int rows, int K);
int cosa_c4_rows(const float *src, const float *bias, void *dst, void *scales, int R, int K, long long src_ld, int ones, int weight, void *stream);
size_t cosa_c4_record_bytes(void);       /* { const float *src; const float *bias; void *dst; void *scales; int rows, K, row0, qrows; } */
int cosa_c4_rows_batched(const void *records /* device */, int n_records, int total_rows, void *stream);
int cosa_layernorm_c4(const float *x, const float *gamma, const float *beta, void *y_c4, void *y_scales, float *y_f32, int rows, int dim,
                      float eps, void *stream);
int cosa_gemm_f16c4(const void *Xs, const void *Xscales, const void *Ws, const void *Wscales, const void *zeros, const float *residual,
                    void *Y, void *Yscales, int M, int N, int K, int epilogue, int ldy, void *stream);
/* attention on plain fp16 qkv rows [B, N, 3, H, 64] -> fp16c4 rows [B*N, 4*H*64 + 128 bytes] (incl. the augmentation block) for the c4 output
 * projection; out_scales = the scale tensor of the WHOLE operand these rows belong to, row0 = the index of out_c4's first row in it */
int cosa_attn_fwd_f16c4(const void *qkv, void *out_c4, void *out_scales, int row0, float *lse, int B, int N, int H, int head_dim, float scale,
                        uint64_t *stamps, void *stream);

/* ---------------------------------------------------------------------------------------
 * main.py:167-212 + utils/seg_helper.py:800-813,199-230  the student's dense losses, fused:
 *   seg_loss(main) and seg_loss(aux) of the bilinearly up-sampled logits, and the inputs of the
 *   dense-energy regulariser (softmax -> x0.5, ROI from boxes, nearest image / label), without
 *   materialising anything at [B,K,S,S].
 *   seg_lr [B,K,hs,ws] logits; maskA/maskB [B,S,S] labels {0..K-1,255}; simg [B,3,S,S] normalised image
 *   forward  -> sums[8] = {bgA_sum,bgA_cnt,fgA_sum,fgA_cnt,bgB_...}; s_seg [B,K,S/2,S/2]; s_img [B,3,S/2,S/2] (0..255);
 *               roi [B,S/2,S/2]; unlabel [B,S/2,S/2] u8   (then cosa_dense_energy_forward on these)
 *   backward -> grad_seg_lr [B,K,hs,ws] for  g_seg * (0.5*seg_loss_A + 0.5*seg_loss_B)  +  g_regw * energy
 *               (AS = the gated filter output kept by cosa_dense_energy_forward)
 *   Sums that meet from many threads (the eight loss sums, the gradient cells) are accumulated in 64-bit fixed point with INTEGER atomics
 *   in `workspace` (cosa_seg_loss_workspace_bytes) and converted at the end: order-independent, the same bits every run.
 * ------------------------------------------------------------------------------------- */
size_t cosa_seg_loss_workspace_bytes(int B, int K, int hs, int ws);
int cosa_seg_loss_forward(const float *seg_lr, const float *maskA, const float *maskB, const float *simg,
                          const int32_t *boxes, float *sums, float *s_seg, float *s_img, float *roi, uint8_t *unlabel,
                          int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream);
int cosa_seg_loss_backward(const float *seg_lr, const float *maskA, const float *maskB, const float *sums, const float *AS,
                           const float *roi, const float *g_seg, const float *g_regw, float *grad_seg_lr,
                           int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream);
/* The same two for every setting of --segfg_alpha a, --aux_cam2seg_alpha b, --aux_cam2seg (main.py:200-203, seg_helper.py:813):
 *   loss = wA_bg bgA + wA_fg fgA + wB_bg bgB + wB_fg fgB, each term sum / (count + 1e-6), with
 *   wA_bg = (1-b)(1-a), wA_fg = (1-b) a, wB_bg = b (1-a), wB_fg = b a;  --aux_cam2seg false: b = 0 and maskB = NULL.
 *   maskB == NULL: nothing of a second label map is read, sums[4..7] come back 0 and the B terms add nothing to the gradient.
 *   The forward emits the sums (the weights enter on the host: sum_i w_i sums_i / (cnt_i + 1e-6)); the backward takes the weights.  Each
 *   weight must lie in [0, 1] (non-finite ones are refused too): COSA_EINVAL, nothing is launched.  The entry points above are these with
 *   both maps and 0.25 x 4 -- same kernels, same bits.  Fixed-point range of the gradient cells: every value is carried while
 *   g_seg (wA_bg + wA_fg + wB_bg + wB_fg) < 16, i.e. g_seg < 16 for the table above; beyond it the result may be NaN (sticky flag), never a
 *   wrapped sum.
 *   Labels: 0 is background, 0 < label < K foreground, every other value is ignored -- 255 (K <= 255 keeps it free) and, exactly as 255 is,
 *   a label in [K, 255): it enters no sum, no count and no gradient, and its quad counts as unlabelled in `unlabel`. */
int cosa_seg_loss_forward_w(const float *seg_lr, const float *maskA, const float *maskB, const float *simg,
                            const int32_t *boxes, float *sums, float *s_seg, float *s_img, float *roi, uint8_t *unlabel,
                            int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream);
int cosa_seg_loss_backward_w(const float *seg_lr, const float *maskA, const float *maskB, const float *sums, const float *AS,
                             const float *roi, const float *g_seg, const float *g_regw, float *grad_seg_lr,
                             float wA_bg, float wA_fg, float wB_bg, float wB_fg,
                             int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream);
/* The same two with a weight per pixel of each label map (utils/seg_helper.py:823-835, seg_weightloss):
 *   relA [B,S,S] beside maskA (required), relB [B,S,S] beside maskB (NULL exactly when maskB is NULL), each weight in [0, 1].
 *   The weight multiplies the pixel's cross-entropy term; the denominators stay the plain counts of labelled pixels, so `sums` keeps its
 *   layout {bgA_wsum, bgA_cnt, fgA_wsum, fgA_cnt, bgB_...} and the host forms the loss from it as above.  In the backward the pixel's
 *   coefficient is multiplied by its weight.  Energy-grid outputs, the regulariser's share, the scatter and the fixed-point cells are those of
 *   the _w entry points, and with every weight 1.0f so is every output bit.  Weights in [0, 1] keep the fixed-point range argument as it
 *   is; a weight outside [0, 1] or a NaN contributes nothing and sets the sticky flag: NaN out, never a wrapped sum.
 *   relA == NULL, or relB given without maskB (or maskB without relB): COSA_EINVAL, nothing is launched. */
int cosa_seg_loss_forward_rw(const float *seg_lr, const float *maskA, const float *maskB, const float *simg,
                             const int32_t *boxes, float *sums, float *s_seg, float *s_img, float *roi, uint8_t *unlabel,
                             int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream,
                             const float *relA, const float *relB);
int cosa_seg_loss_backward_rw(const float *seg_lr, const float *maskA, const float *maskB, const float *sums, const float *AS,
                              const float *roi, const float *g_seg, const float *g_regw, float *grad_seg_lr,
                              float wA_bg, float wA_fg, float wB_bg, float wB_fg,
                              int B, int K, int hs, int ws, int S, void *workspace, size_t workspace_bytes, void *stream,
                              const float *relA, const float *relB);

/* F.multilabel_soft_margin_loss (main.py:127-128 on the classification logits; seg_helper.py:593-602 on relu(cam) against the resized teacher
 * probabilities) and its gradient in one pass: loss[0] = mean_r mean_c -(y log s(v) + (1-y) log s(-v)), v = relu ? max(x,0) : x;
 * grad = d loss / d x.  Element (r, c) of x / y / grad lies at (r / HW) * C * HW + c * HW + r % HW (HW = 1: row-major [R,C]; HW = h*w: NCHW).
 * workspace: ceil(R / 256) doubles.                                                                                                   */
int cosa_msm_loss(const float *x, const float *y, float *grad, float *loss, void *workspace, int R, int C, int HW, int relu, void *stream);
/* main.py:227-228 + utils/seg_helper.py:553-568,593-597: targets of cam_loss -- seg_refine_by_label(teacher seg, T) foreground
 * channels, bilinearly down-sampled to the CAM grid -- evaluated only at the pixels the down-sampling reads, straight from the
 * per-scale low-res teacher seg outputs seg_scales[i] [2B,K,hs[i],ws[i]] (original batch, then the flipped batch).
 *   out [B, K-1, oh, ow]                                                                                                      */
int cosa_cam_loss_targets(const float *const *seg_scales, const int *hs, const int *ws, int n_scales, const float *labels,
                          float *out, int B, int K, int S, int oh, int ow, float temperature, void *stream);
/* ... with the reference's other branch (seg_helper.py:558-561, --after_softmax true) selectable: after_softmax = 1 takes the softmax of
 * sum_scales / T over all K channels and sets the channels of absent classes to zero afterwards; 0 is the call above, bit for bit.
 * 1 to 4 scales; a null or empty scale (seg_scales[i] NULL, hs[i] or ws[i] <= 0) is refused as cosa_cam_label refuses it: COSA_EINVAL,
 * nothing is launched.                                                                                                              */
int cosa_cam_loss_targets_m(const float *const *seg_scales, const int *hs, const int *ws, int n_scales, const float *labels,
                            float *out, int B, int K, int S, int oh, int ow, float temperature, int after_softmax, void *stream);
/* --camloss_version v2 | v3 (utils/seg_helper.py:604-653).  Both normalise every plane of relu(cam) to n = (r - min r) / (max r + 1e-4) with
 * the gradient flowing through the minimum and the maximum (to the FIRST position of each, as adaptive_max_pool2d routes it).
 *   cam / grad fp32 [B,C,h,w], loss one float, grad = d loss / d cam for a unit upstream gradient (value and gradient from one call).
 *   One workgroup per plane: h w <= 6400 (80 x 80), C + 1 <= 128; fixed-order reductions and integer sums -- the same bytes every run.
 * cosa_cam_lossv2: multilabel_soft_margin(n, targets), targets fp32 [B,C,h,w] already at the CAM's size (cosa_cam_loss_targets_m's output).
 * cosa_cam_lossv3: cam_mix = cat(1 - max_c n, n); class-balanced cross-entropy (0.5 background + 0.5 foreground, each a mean over its pixels)
 *   of bilinear_up(cam_mix, S) against label bytes [B,S,S]: 0 background, 1..C, 255 (and anything above C) ignored.  S even, S >= 8 h and
 *   S >= 8 w.  The up-sampled tensor is never written: the cross-entropy runs on the cosa_seg_loss_* scheme.  At equal n the lowest channel
 *   takes the background's gradient.
 * cosa_cam_label: the label map of cam_lossv3_wrap from cosa_cam_loss_targets_m's inputs at every pixel: the argmax (lowest index at a tie)
 *   of seg_refine_by_label(sum of scales, T, after_softmax), 255 where its maximum probability is not above segconf_thre.  out bytes [B,S,S].
 * A refused call (COSA_EINVAL: null pointer, more than 128 classes, a plane outside the envelope, an up-sampling factor below 8, a
 * non-finite temperature or threshold, a short workspace) launches nothing.                                                              */
size_t cosa_cam_lossv2_workspace_bytes(int B, int C);
int cosa_cam_lossv2(const float *cam, const float *targets, float *grad, float *loss, int B, int C, int h, int w, void *workspace,
                    size_t workspace_bytes, void *stream);
size_t cosa_cam_lossv3_workspace_bytes(int B, int C, int h, int w);
int cosa_cam_lossv3(const float *cam, const uint8_t *label, float *grad, float *loss, int B, int C, int h, int w, int S, void *workspace,
                    size_t workspace_bytes, void *stream);
int cosa_cam_label(const float *const *seg_scales, const int *hs, const int *ws, int n_scales, const float *labels, uint8_t *out,
                   int B, int K, int S, float temperature, float segconf_thre, int after_softmax, void *stream);
/* The soft-label seg loss distilled from the teacher's segmentation (utils/seg_helper.py:837-861, seg_softloss).  Per pixel
 * (y, x) of image b inside boxes[b] = (y0, y1, x0, x1): z_k = the sum over scales and both flips of the bilinearly up-sampled teacher segs
 * (cosa_cam_loss_targets_m's inputs and sum), q = softmax(z / (2 n_scales temp)) over the background and the classes of labels[b] (q_k = 0
 * exactly for an absent class), l = - sum_k q_k log p_k with p the softmax of bilinear_up(seg_lr).  The pixel is background when the first
 * argmax of q is 0 and foreground otherwise, and in neither set when max q <= conf or outside the box.
 *   sums[4] = {sum_bg l, n_bg, sum_fg l, n_fg}     loss[0] = (1 - fg_alpha) sums[0] / (sums[1] + 1e-6) + fg_alpha sums[2] / (sums[3] + 1e-6)
 *   grad_seg_lr [B,K,hs,ws] = upstream[0] * d loss / d seg_lr (the target is a constant), from the forward's `sums` on the device.
 * 64-bit fixed-point sums and gradient cells, integer atomics only: the same bytes every run; a sum the fixed point cannot carry gives NaN.
 * Nothing of size [B,K,S,S] is written, and no pixel outside its box is evaluated.  Envelope: 2 <= K <= 128, 1 to 4 scales of at most S x S,
 * S even, S >= 8 hs and S >= 8 ws, temp finite and positive, conf in [0, 1), fg_alpha in [0, 1]; anything else is COSA_EINVAL and launches
 * nothing.  workspace: cosa_seg_soft_workspace_bytes(B, K, hs, ws) bytes, the same buffer for a forward and its backward.                  */
size_t cosa_seg_soft_workspace_bytes(int B, int K, int hs, int ws);
int cosa_seg_soft_forward(const float *seg_lr, const float *const *seg_scales, const int *hs_t, const int *ws_t, int n_scales,
                          const float *labels, const int32_t *boxes, float *sums, float *loss, int B, int K, int hs, int ws, int S,
                          float temp, float conf, float fg_alpha, void *workspace, size_t workspace_bytes, void *stream);
int cosa_seg_soft_backward(const float *seg_lr, const float *const *seg_scales, const int *hs_t, const int *ws_t, int n_scales,
                           const float *labels, const int32_t *boxes, const float *sums, const float *upstream, float *grad_seg_lr,
                           int B, int K, int hs, int ws, int S, float temp, float conf, float fg_alpha, void *workspace,
                           size_t workspace_bytes, void *stream);
/* utils/seg_helper.py:210-230 (get_energy_loss: F.softmax over the classes of the full-resolution logits) + :199-203 (DenseEnergyLoss.forward:
 * bilinear resize of the probabilities by 0.5 = the mean of each 2x2 quad) in one pass, and the backward of the pair:
 *   logit [B,K,H,W] (H, W even)   out / grad_out [B,K,H/2,W/2]   grad_logit [B,K,H,W]                                                     */
int cosa_softmax_halfres_forward(const float *logit, float *out, int B, int K, int H, int W, void *stream);
int cosa_softmax_halfres_backward(const float *logit, const float *grad_out, float *grad_logit, int B, int K, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * utils/torch_helper.py:261-293 (AdamW with the scheduled LR) + main.py:250-252 (teacher EMA) + the bf16 shadow
 * refresh, one multi-tensor pass.  `records`: device array, one per parameter tensor:
 *   { float *p; const float *g (NULL = frozen: EMA only); float *m, *v; float *teacher; bf16 *p16, *t16 (or NULL);
 *     float lr, wd; int64 n }   (cosa_optim_record_bytes() bytes each)
 * `chunks`: device array of {int tensor, int chunk} covering every tensor in pieces of cosa_optim_chunk_elems().
 * ------------------------------------------------------------------------------------- */
size_t cosa_optim_record_bytes(void);
int cosa_optim_chunk_elems(void);
int cosa_fused_adamw_ema(const void *records, const void *chunks, int n_chunks, float beta1, float beta2, float eps,
                         int step, float ema_momentum, void *stream);

/* ---------------------------------------------------------------------------------------
 * The gradient guard: clip by the global norm and refuse a step with a non-finite gradient, decided
 * on the device.  Both calls take the record table and chunk list of cosa_fused_adamw_ema and go on the same stream.
 * `guard`: one device record of cosa_grad_guard_bytes() = 40 bytes, 8-byte aligned, zeroed once by the caller:
 *   { float norm;  float coef;  int32 skip;  int32 pad;  int64 applied, skipped, clipped }
 * cosa_grad_norm: norm = sqrt(sum g^2) over every record with g != NULL, summed in double in a fixed order (the same bits
 *   from run to run; non-finite exactly when some gradient element is); coef = min(1, max_norm / (norm + 1e-6)), or 1 when
 *   max_norm == 0 (no clipping); skip = skip_nonfinite && the double sum is not finite.  The counters advance by one call:
 *   skipped on skip, else applied (and clipped when coef < 1).  `workspace`: cosa_grad_norm_workspace_bytes(n_chunks) bytes,
 *   8-byte aligned.
 * cosa_fused_adamw_ema_guarded: cosa_fused_adamw_ema on g * coef (the gradients are only read; with coef == 1 the bits of the
 *   unguarded call), or, on skip, nothing at all: masters, moments, teacher and every 16-bit shadow keep their bytes.
 *   `step` is the host's count and advances over a refused step too (nothing of the decision ever reaches the host).
 * ------------------------------------------------------------------------------------- */
size_t cosa_grad_guard_bytes(void);
size_t cosa_grad_norm_workspace_bytes(int n_chunks);
int cosa_grad_norm(const void *records, const void *chunks, int n_chunks, float max_norm, int skip_nonfinite, void *workspace,
                   size_t workspace_bytes, void *guard, void *stream);
int cosa_fused_adamw_ema_guarded(const void *records, const void *chunks, int n_chunks, float beta1, float beta2, float eps,
                                 int step, float ema_momentum, const void *guard, void *stream);

/* ---------------------------------------------------------------------------------------
 * Gradient accumulation over micro-batches, over the record table and chunk list of
 * cosa_fused_adamw_ema: one block per chunk, one launch.  `acc_ptrs`: device array of one float* per record (NULL: no
 * accumulator, the tensor is skipped; so is a record with g == NULL, whose accumulator keeps its bytes).  An accumulator
 * holds the record's n floats and, when n % 4 == 0, is 16-byte aligned (as g is).
 *   mode 0: acc = g                    (first micro-step: acc is not read, it needs no clear)
 *   mode 1: acc = acc + g
 *   mode 2: acc = (acc + g) * scale    (closing micro-step, scale = fl(1/N))
 * fp32, one rounding per operation, so N micro-steps leave fl(fl(...fl(g1 + g2)... + gN) * scale) -- what the same torch
 * expression gives bit for bit.  Non-finite values propagate.  The gradient buffers are only read.
 * Refused with COSA_EINVAL, nothing launched: a NULL table, chunk list or pointer array, n_chunks <= 0, a mode outside
 * 0..2, a non-finite scale (whatever the mode).
 * ------------------------------------------------------------------------------------- */
int cosa_grad_accumulate(const void *records, const void *chunks, int n_chunks, const void *acc_ptrs, int mode, float scale,
                         void *stream);

/* ---------------------------------------------------------------------------------------
 * Training-state arena: every tensor that defines the future of a run, gathered into ONE contiguous
 * device arena by one launch (and scattered back by one), with two 64-bit checksums per tensor.
 * cosa_state_layout: THE definition of the arena for host and device: tensor i (nbytes[i] bytes, any dtype, contiguous)
 *   occupies [offsets_out[i], offsets_out[i] + nbytes[i]) of a slot rounded up to 16 bytes whose tail is zero; slots follow
 *   each other in table order.  Returns the arena's size; (size_t)-1 (message in cosa_last_error()) for n outside 0..4096 or a
 *   tensor above 2^40 bytes.  Zero-length tensors are accepted (empty slot, checksums 0).
 * `records`: device array of n_tensors { void *ptr; uint64 nbytes; uint64 off } (cosa_state_record_bytes() each); `chunks`:
 *   device array of n_chunks {int tensor, int chunk} covering every SLOT in pieces of cosa_state_chunk_bytes().
 * `sums`: device uint64 [n_tensors][2], zeroed by the call itself on `stream`: over the little-endian 32-bit words w_i of the
 *   zero-padded slot, s0 = sum w_i and s1 = sum (i+1) w_i, both mod 2^64 (order-independent: bit-identical from run to run).
 * cosa_state_snapshot: tensors -> arena (+ checksums of what was written).  The arena must be 16-byte aligned; sources of any
 *   alignment and odd byte counts are taken (16-byte accesses where the pointer allows).
 * cosa_state_restore: scatter == 0 only recomputes the checksums of the arena's slots (nothing is written but `sums`): the host
 *   compares them with the recorded ones BEFORE it calls again with scatter == 1, which copies the slots back into the tensors.
 * ------------------------------------------------------------------------------------- */
size_t cosa_state_record_bytes(void);
size_t cosa_state_chunk_bytes(void);
size_t cosa_state_layout(int n, const unsigned long long *nbytes, unsigned long long *offsets_out);
int cosa_state_snapshot(const void *records, const void *chunks, int n_tensors, int n_chunks, void *arena, void *sums, void *stream);
int cosa_state_restore(const void *records, const void *chunks, int n_tensors, int n_chunks, const void *arena, void *sums, int scatter,
                       void *stream);

/* ---------------------------------------------------------------------------------------
 * models/vit/vit.py:154-158  the student's pre-LN residual blocks (training, bf16 stream), element-wise side:
 *   cosa_add_layernorm_fwd: x_out = bf16(x + delta) (delta may be NULL: x_out optional), y = LayerNorm(x_out; gamma, beta, eps),
 *     mean / rstd [rows] kept for the backward.  All tensors bf16 [rows, 768] except mean / rstd (fp32).
 *   cosa_layernorm_bwd: dx = dLayerNorm(dy) + dskip (dskip optional: the gradient arriving at x_out through the skip path),
 *     dgamma / dbeta [768] fp32 (= or += with accumulate != 0), summed deterministically through `workspace`.
 * ------------------------------------------------------------------------------------- */
int cosa_add_layernorm_fwd(const void *x, const void *delta, const void *gamma, const void *beta, void *x_out, void *y,
                           float *mean, float *rstd, int rows, int dim, float eps, void *stream);
size_t cosa_layernorm_bwd_workspace_bytes(int rows, int dim);
int cosa_layernorm_bwd(const void *dy, const void *x_new, const float *mean, const float *rstd, const void *gamma,
                       const void *dskip, void *dx, float *dgamma, float *dbeta, int accumulate, int rows, int dim,
                       void *workspace, size_t workspace_bytes, void *stream);
/* fp32 residual stream (the student's default since round 4; the reference trains in fp32, main.py:124-246): the forward of a block's
 * LayerNorm is cosa_layernorm on the fp32 stream, the residual add is cosa_gemm_bf16's fp32 residual epilogue, and the backward is
 *   cosa_layernorm_bwd_f32: dx (fp32) = dLayerNorm(dy: bf16, or fp32 with dy_is_f32; x fp32, gamma bf16, eps) + dskip (fp32, optional), dx16 (optional) = bf16(dx)
 *     -- the dY operand of the preceding projection's gradient GEMMs; mean / rstd are recomputed from x; dgamma / dbeta as above. */
int cosa_layernorm_bwd_f32(const void *dy, int dy_is_f32, const float *x, const void *gamma, const float *dskip, float *dx, void *dx16,
                           float *dgamma, float *dbeta, int accumulate, int rows, int dim, float eps, void *workspace,
                           size_t workspace_bytes, void *stream);
/* models/__init__.py:163-206 + autograd: the gradient junction of the training path's heads.  g0, g1, g2: bf16 gradients [B, N - 1, dim] of the
 * consumers of the patch tokens (decoder, CAM head, pooled classification head; NULL = consumer absent); dx [B, N, dim] fp32 = their sum in
 * fp32 (order g0, g1, g2), zero in the class-token row.                                                                                   */
int cosa_token_junction_bwd(const void *g0, const void *g1, const void *g2, float *dx, int B, int N, int dim, void *stream);

/* ---------------------------------------------------------------------------------------
 * Evaluation path (SURVEY f-1; evaluation_engine.py:96-126,198-200, utils/seg_helper.py:515-546,581-591,
 * utils/evaluation.py:10-70).
 *   cosa_eval_labels: one launch replaces F.interpolate(cam), cam_to_label, F.interpolate(seg), seg_validation and the
 *     three argmaxes.  cam [B,C,S,S], seg [B,C+1,S,S] (either may be NULL), cls_label [B,C] -> uint8 maps [B,H,W]:
 *     lab_cam = argmax_c(cls*cam)+1 or 0 where the max <= bkg_thre; lab_ps = argmax(seg); lab_vd = argmax with the
 *     classes absent from cls_label masked to -1e5 (background always present).
 *   cosa_cam_to_label: cam_to_label on an already sized CAM [B,C,H,W] -> int64 label [B,H,W]; cls_label, boxes
 *     ([B,4] h0,h1,w0,w1; NULL = the reference's `img_box is None` return) and valid_cam (= cls*cam) optional.
 *   cosa_confusion_hist: hist[nc*t + p] += 1 over n pixels with truth t < nc (uint8 maps, 255 = ignore);
 *     pseudo != 0 drops the pixels whose prediction is 255 (pseudo_scores).  hist: nc*nc uint64, caller-zeroed, accumulates.
 * ------------------------------------------------------------------------------------- */
int cosa_eval_labels(const float *cam, const float *seg, const float *cls_label, int B, int C, int S, int H, int W,
                     float bkg_thre, uint8_t *lab_cam, uint8_t *lab_ps, uint8_t *lab_vd, void *stream);
int cosa_cam_to_label(const float *cam, const float *cls_label, int B, int C, int H, int W, float bkg_thre,
                      const int32_t *boxes, int ignore_mid, float high_thre, float low_thre, long long ignore_index,
                      long long *label, float *valid_cam, void *stream);
int cosa_confusion_hist(const uint8_t *gt, const uint8_t *pred, size_t n, int num_classes, int pseudo,
                        unsigned long long *hist, void *stream);

/* ---------------------------------------------------------------------------------------
 * Per-image evaluation counters (what the reference's assist_seg, evaluation_engine.py:311-329, takes
 * from a prediction).  One launch scores ONE image: gt and n_maps label maps of it (uint8, n pixels each, 255 = ignore) ADD
 * into a caller-zeroed row of cosa_image_scores_words(num_classes, n_maps) uint64 words
 *   row = [ n, n_valid, then for map m, class c: I, P, G, A ]            (2 + n_maps * num_classes * 4 words)
 * n_valid = #{gt < num_classes}.  A pixel is counted for map m under the rule of cosa_confusion_hist: gt < num_classes and
 * pred < num_classes -- a prediction that is no class drops the pixel, 255 included, so pseudo[m] (pseudo_scores' "a
 * prediction of 255 drops the pixel") changes no count at num_classes <= 255; it is taken for symmetry with that entry and
 * recorded by the host.  Over counted pixels I = #{gt == c and pred == c}, P = #{pred == c}, G = #{gt == c}; A = #{pred == c}
 * over all n pixels, ignored truth included (assist_seg's seg_area).  Rows summed over a dataset give the diagonal (I), the
 * column sums (P) and the row sums (G) of cosa_confusion_hist's matrix for the same maps, exactly.  Integer atomics only: the
 * row holds the same bytes on every run.  preds and pseudo are HOST arrays of n_maps entries; the maps are device pointers of
 * any byte alignment.  Envelope: gt, preds, every preds[m], pseudo and row non-NULL, row 8-byte aligned,
 * 1 <= num_classes <= 255, 1 <= n_maps <= COSA_IMAGE_SCORES_MAX_MAPS, 1 <= n < 2^32; anything else is COSA_EINVAL, nothing is
 * launched and the row is untouched.  One launch, no workspace, no host sync.
 * ------------------------------------------------------------------------------------- */
#define COSA_IMAGE_SCORES_MAX_MAPS 8
size_t cosa_image_scores_words(int num_classes, int n_maps);   /* uint64 words of one row; 0 on bad arguments */
int cosa_image_scores(const uint8_t *gt, const uint8_t *const *preds, const int *pseudo, int n_maps, size_t n,
                      int num_classes, unsigned long long *row, void *stream);

/* ---------------------------------------------------------------------------------------
 * Per-image Boundary IoU counters (Cheng et al., CVPR 2021): cosa_image_scores' row over BAND pixels.
 * A label map is uint8 [H, W]; a value < num_classes is a class, any other value (255 included) is no class.  For d >= 1 a
 * class pixel is INTERIOR iff its whole (2d+1) x (2d+1) window lies inside the image and every pixel of it holds the pixel's
 * own label; a class pixel that is not interior is a BAND pixel of its class; a pixel that is no class is in no band (d
 * erosions of the class's mask on a zero border, mask minus eroded, for every class at once).  One call scores ONE image: gt
 * and n_maps maps of it ADD into a caller-zeroed row of cosa_boundary_scores_words(num_classes, n_maps) uint64 words
 *   row = [ n, n_valid, then for map m, class c: I, P, G, A ]            (= cosa_image_scores_words)
 * n = H * W, n_valid = #{gt < num_classes}.  A pixel is counted for map m under cosa_image_scores' rule on the maps
 * themselves: gt < num_classes and pred_m < num_classes.  Over counted pixels I = #{gt band c and pred band c},
 * P = #{pred band c}, G = #{gt band c}; A = #{pred band c} over all n pixels.  Boundary IoU of class c is I / (P + G - I).
 * Any d >= max(H, W) leaves no pixel interior: the row is then cosa_image_scores' row word for word.  Integer atomics only:
 * the row holds the same bytes on every run and for any grid.  preds is a HOST array of n_maps device pointers of any byte
 * alignment; the maps are dense H x W.  Envelope: gt, preds, every preds[m] and row non-NULL, row 8-byte aligned,
 * 1 <= num_classes <= 255, 1 <= n_maps <= COSA_IMAGE_SCORES_MAX_MAPS, H, W >= 1, H * W < 2^32, 1 <= d <= 64; anything else is
 * COSA_EINVAL, nothing is launched and the row is untouched.  One launch, no workspace, no host sync.
 * ------------------------------------------------------------------------------------- */
size_t cosa_boundary_scores_words(int num_classes, int n_maps);   /* uint64 words of one row; 0 on bad arguments */
int cosa_boundary_scores(const uint8_t *gt, const uint8_t *const *preds, int n_maps, int H, int W, int d,
                         int num_classes, unsigned long long *row, void *stream);

/* ---------------------------------------------------------------------------------------
 * Export: every file product of ONE image, at the image's own (generally non-square) H x W, in one
 * packed record, from what multi_scale_camsegv3 returns for it: cam / cam_aux [C,S,S], seg [C+1,S,S], cls_label [C] or
 * NULL (no image-level labels: seg only, plain argmax).  `what` is a mask of COSA_EXPORT_* bits:
 *   SEG         uint8 [H,W]   argmax of the logits resized to H x W, absent classes masked first (the bits of
 *                             cosa_eval_labels' lab_vd; lab_ps without a label row)
 *   PSEUDO(_AUX) uint8 [H,W]  v = cls * resized CAM; m = max over present classes: m > high_thre -> class + 1, else
 *                             m > low_thre -> ignore_index, else 0 (cam2mask without refine model, whole image box)
 *   RAWCAM(_AUX) fp32 [K_live,H,W] + int32 [K_live]: the planes v of the present classes in class order and their indices
 *   PSEUDO_PAR / PSEUDO_AUX_PAR uint8 [H,W]  the PAR-refined labels CoSA trains on, written by cosa_export_refine (below)
 * K_live = number of non-zero entries of cls_label (the host knows it: it sizes the record).
 * cosa_export_record_layout: offsets[COSA_EXPORT_SLOTS] (bytes from the record's start, each 16-byte aligned; (size_t)-1
 * when not asked for) in the order seg, pseudo, pseudo_aux, rawcam, rawcam_aux, rawcam indices, rawcam_aux indices,
 * pseudo_par, pseudo_aux_par (the PAR slots come last: a record without them is laid out as if they did not exist);
 * returns the record's size in bytes, 0 on bad arguments.  Host and device use this one definition.
 * ------------------------------------------------------------------------------------- */
#define COSA_EXPORT_SEG 1u
#define COSA_EXPORT_PSEUDO 2u
#define COSA_EXPORT_PSEUDO_AUX 4u
#define COSA_EXPORT_RAWCAM 8u
#define COSA_EXPORT_RAWCAM_AUX 16u
#define COSA_EXPORT_ALL 31u               /* what cosa_export_maps writes */
#define COSA_EXPORT_PSEUDO_PAR 32u
#define COSA_EXPORT_PSEUDO_AUX_PAR 64u
#define COSA_EXPORT_EVERY 127u
#define COSA_EXPORT_SLOTS 9
#define COSA_EXPORT_REFINE_MIN_SIDE 16    /* smallest H and W cosa_export_refine takes */
size_t cosa_export_record_layout(int C, int H, int W, int K_live, unsigned what, size_t *offsets);
int cosa_export_maps(const float *cam, const float *cam_aux, const float *seg, const float *cls_label, int C, int S, int H, int W,
                     int K_live, unsigned what, float high_thre, float low_thre, int ignore_index, void *record,
                     size_t record_bytes, void *stream);

/* PAR-refined pseudo labels of ONE image at its own H x W into the record's PSEUDO_PAR / PSEUDO_AUX_PAR slots (nothing else is
 * written; `what` is the mask the record was laid out with and must name at least one of the two).  The reference's
 *   cam2mask(images=image, img_boxes=[[0,H,0,W]], cams=cls * resize(cam, (H,W)), cls_labels, high, low,
 *            refine_model=PAR(par_iters, dilations), ignore_index, downscale)
 * (utils/seg_helper.py:721-797) read literally at H != W: PAR grid (H/2, W/2) (integer division; downscale 0: (H, W)), the
 * threshold plane is key 0, softmax over the present classes, every resize bilinear align_corners=False by spec R, exp by spec E,
 * first maximum wins, m = hi; m[hi == 0] = ignore; m[hi + lo == 0] = 0.  image: [3,H,W] in [0,1] (cosa_denormalize_img);
 * cls_label must hold exactly K_live non-zero entries; K_live == 0 gives all-zero maps.  downscale: 0 or 2; 1..8 dilations;
 * H, W >= COSA_EXPORT_REFINE_MIN_SIDE (smaller sizes are refused, nothing is clamped).  The affinity tensor is built once and
 * streamed once per step for the hi and lo stacks of both CAM sets.  Workspace: cosa_export_refine_workspace_bytes (0 on bad
 * arguments); too small a workspace is COSA_ENOMEM. */
size_t cosa_export_refine_workspace_bytes(int H, int W, int K_live, unsigned what, int downscale, int n_dil);
int cosa_export_refine(const float *image, const float *cam, const float *cam_aux, const float *cls_label, int C, int S, int H, int W,
                       int K_live, unsigned what, float high_thre, float low_thre, int ignore_index, int downscale,
                       const int *dilations, int n_dil, int par_iters, void *record, size_t record_bytes, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Label-free export (csrc/predict_kernels.hip).
 * cosa_predict_classes: the image-level class rows of G images from their classification logits [G, C] (fp32; the summed
 *   `cls_final` of the multi-scale pass).  Class c is present iff logit_c >= L (the host passes L = float32(log(t / (1 - t)))
 *   for a probability threshold t); a NaN is never present.  If fewer than cls_min classes are present, the classes with the
 *   largest remaining logits are added, one per round, equal logits in index order, until cls_min are present or nothing is
 *   left to add: a NaN and -inf are never added (+inf is >= L, so present).  rows [G, C] fp32 in {0, 1}; k_live [G] int32
 *   = the row's sum; nonfinite [G] int32 = the image's NaN and +-inf logits.  One wavefront per image, classes on the lanes;
 *   plain stores, no atomics, no workspace, one launch.  Envelope: non-NULL pointers, 1 <= C <= COSA_PREDICT_MAX_CLASSES,
 *   1 <= G <= 65535, 0 <= cls_min <= C, L not NaN; anything else is COSA_EINVAL, nothing is launched, the outputs are untouched.
 * cosa_export_overlay: the label map `seg` [H, W] (uint8, e.g. the SEG slot of an export record) painted over the image it
 *   belongs to.  image: [3, H, W] fp32, normalised as the loaders give it ((byte - mean_c) / std_c, mean 123.675, 116.28,
 *   103.53, std 58.395, 57.12, 57.375); per pixel and channel img = clamp(rint(x * std_c + mean_c), 0, 255) (product and sum
 *   rounded separately); label 0 keeps img, label l > 0 gives (alpha256 * palette[l][c] + (256 - alpha256) * img + 128) >> 8.
 *   palette: 256 x 3 bytes on the device.  out: 3 H W bytes, interleaved R G B per pixel (the engine appends them to the
 *   image's record behind every slot of cosa_export_record_layout, which does not know them).  Integer blending: the same
 *   bytes on every run.  Four pixels per thread by one dwordx4 per colour plane where image is 16-byte and seg / out are
 *   4-byte aligned, the H W % 4 last pixels (else all) one per thread.  Envelope: non-NULL pointers, H, W > 0, H W < 2^29,
 *   0 <= alpha256 <= 256; anything else is COSA_EINVAL, nothing is launched.  One launch, no workspace.
 * ------------------------------------------------------------------------------------- */
#define COSA_PREDICT_MAX_CLASSES 256
int cosa_predict_classes(const float *logits, int G, int C, float L, int cls_min, float *rows, int *k_live, int *nonfinite,
                         void *stream);
int cosa_export_overlay(const float *image, const uint8_t *seg, const uint8_t *palette, int H, int W, int alpha256, uint8_t *out,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * The CAM pictures of prediction export (csrc/heat_kernels.hip).
 * cosa_export_camheat: k class planes [k, H, W] fp32 (the RAWCAM or RAWCAM_AUX slot of an export record) as k heat maps over
 *   the image [3, H, W] (fp32, normalised as for cosa_export_overlay).  Per picture, pixel and colour c, in integers:
 *     idx = trunc(255 m) clamped to 0..255 (a NaN gives 0);
 *     jet[idx][c] = (clamp(765 - |8 idx - k_c|, 0, 510) + 1) >> 1, k = 1530, 1020, 510 for R, G, B;
 *     s = jet[idx][c] + img (img as in cosa_export_overlay); M = max of s over the picture's 3 H W values (>= 128);
 *     byte = 255 s / M (integer division).
 *   out: [k, H, W, 3] uint8, dense.  Two launches whatever k is: the k maxima by 32-bit integer atomics into `workspace`
 *   (4 k bytes, 4-byte aligned; zeroed here, on the stream), then the bytes.  No float
 *   atomics, no host sync: the same bytes on every run.  Four pixels per thread by one dwordx4 per plane (unaligned where
 *   H W % 4 != 0 moves a plane off the 16-byte grid), the H W % 4 last pixels one per thread.
 * cosa_export_panel: per class j one picture [H, cols W, 3] of column blocks, left to right: heat[j] ([k, H, W, 3], what
 *   cosa_export_camheat wrote); (10,186,181) where seg == class_idx[j] + 1, else black; the same for gt (a gt of 255 never
 *   matches); the image's bytes.  gt may be NULL: the block is then left out, cols = 3, else 4.  seg, gt: uint8 [H, W];
 *   class_idx: int32 [k] on the device, 0-based (a record's RAWCAM index slot).  One launch.
 * Envelope of both: non-NULL pointers (gt excepted), H, W > 0, H W < 2^29, 1 <= k <= COSA_CAMHEAT_MAX_CLASSES, out_bytes
 *   (workspace_bytes) at least what is written, float / int32 arrays 4-byte aligned; anything else is COSA_EINVAL and nothing
 *   is launched.
 * ------------------------------------------------------------------------------------- */
#define COSA_CAMHEAT_MAX_CLASSES 256
int cosa_export_camheat(const float *planes, const float *image, int k, int H, int W, uint8_t *out, size_t out_bytes,
                        void *workspace, size_t workspace_bytes, void *stream);
int cosa_export_panel(const uint8_t *heat, const uint8_t *seg, const uint8_t *gt, const int *class_idx, const float *image, int k,
                      int H, int W, uint8_t *out, size_t out_bytes, void *stream);
/* ---------------------------------------------------------------------------------------
 * Per-step pseudo-label statistics and the teacher finite check: one reduction over tensors the
 * training step already holds, accumulated on the device in a vector of uint64 counters.
 * cosa_label_stats_layout: THE definition of that vector for host and device.  K = num_classes (background included,
 *   2..128).  offsets[COSA_LABEL_STATS_SLOTS] (in elements) of, in order: steps; pix (pixels inside the crop boxes);
 *   main[K+1] (pixels of the main label map per value 0..K-1, slot K = ignore); aux[K+1]; agree (pixels where main and
 *   auxiliary label are equal, ignore counted as a value); inter[K] and pred[K] (per class: student label == main label,
 *   and student label, over the pixels whose main label is not ignore); bad_cam; bad_cam_aux (non-finite CAM elements).
 *   Returns the number of elements (4K + 7), 0 on bad arguments.
 * cosa_label_stats: mask_main / mask_aux fp32 [B,S,S] in {0..K-1, ignore_index} (cosa_cam2mask_multi's output);
 *   seg_logits fp32 [B,K,h,w], the student's low-resolution logits; cls_label fp32 [B,K-1]; boxes int32 [B,4]
 *   (y0,y1,x0,x1); cam / cam_aux fp32 [B,K-1,S,S].  mask_aux, cam and cam_aux may be NULL: their slots stay untouched and
 *   agree is not advanced.  A mask value that is neither an integer in 0..K-1 nor ignore_index is counted in pix only.
 *   Only pixels inside an image's box count, for every slot; an empty box contributes nothing.
 *   Student label: the K planes resized to (S,S) by spec R (scale = (float)h / (float)S), classes absent from cls_label
 *   replaced by -1e5 (background always live), first maximum in class order: the lab_vd rule of cosa_eval_labels.
 *   bad_*: elements that are not finite, over the planes of PRESENT classes only (an absent class's plane is never read).
 *   step_scale: one device fp32, written by every call: 1.0f when this call met no non-finite element, a quiet NaN
 *   otherwise.  The counters accumulate from call to call (integer atomics: the same bits in any order) and steps
 *   advances by one.  workspace: COSA_LABEL_STATS_WORKSPACE_BYTES of device memory, 8-byte aligned: the step-local flag
 *   behind step_scale, cleared by the call itself on `stream`.  Envelope: K <= 128, S, h, w > 0, h and w <= S; anything
 *   else is COSA_EINVAL, nothing is launched or clamped.  One memset node and two launches.
 * ------------------------------------------------------------------------------------- */
#define COSA_LABEL_STATS_SLOTS 9
#define COSA_LABEL_STATS_WORKSPACE_BYTES 8
size_t cosa_label_stats_layout(int K, size_t *offsets);
int cosa_label_stats(const float *mask_main, const float *mask_aux, const float *seg_logits, const float *cls_label,
                     const int32_t *boxes, const float *cam, const float *cam_aux, int B, int K, int S, int h, int w,
                     int ignore_index, unsigned long long *counters, float *step_scale, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * --gt_stats: pseudo labels and the student's prediction scored against the ground truth of the
 * training crops, one reduction per step accumulated on the device in a vector of uint64 counters.
 * cosa_gt_stats_layout: THE definition of that vector for host and device.  K = num_classes (background included, 2..128).
 *   offsets[COSA_GT_STATS_SLOTS] (in elements) of, in order: steps; pix (pixels inside the crop boxes); valid (of those, the
 *   ones whose ground truth is a class 0..K-1); gt_other (in-box pixels whose ground truth is neither a class nor 255: treated
 *   as ignore); main[K][K+1] (row: ground-truth class, column: the main label map's value, column K = its ignore);
 *   aux[K][K+1]; student[K][K] (column: the student's label).  Returns the number of elements, 4 + 2K(K+1) + K^2; 0 on bad
 *   arguments.
 * cosa_gt_stats: gt uint8 [B,S,S] (cosa_augment_labels' output); mask_main / mask_aux fp32 [B,S,S] in {0..K-1, ignore_index}
 *   (cosa_cam2mask_multi's output), mask_aux may be NULL: the aux block's bytes stay as they are; seg_logits fp32 [B,K,h,w];
 *   cls_label fp32 [B,K-1]; boxes int32 [B,4] (y0,y1,x0,x1).  Only pixels inside an image's box with a class as ground truth
 *   reach the matrices: pixels outside a box, an empty box and gt = 255 contribute nothing.  A mask value that is neither an
 *   integer in 0..K-1 nor ignore_index is counted in pix and valid only.  Student label: cosa_label_stats' (the same device
 *   function): planes resized by spec R, absent classes at -1e5, first maximum in class order.  The counters accumulate from
 *   call to call with 64-bit integer atomics (the same bytes in any order and on every run) and steps advances by one.  Where
 *   the three matrices fit 40 KiB of LDS as u32 (K <= 58) a workgroup counts there and flushes its non-zero entries; above
 *   that the counts go to global memory directly.  Envelope as cosa_label_stats: K <= 128, S, h, w > 0, h and w <= S,
 *   ignore_index no class; anything else is COSA_EINVAL, nothing is launched or clamped.  One launch, no workspace.
 * cosa_gt_stats_uses_lds: 1 when K takes the LDS path, 0 for global atomics, -1 on bad K.
 * ------------------------------------------------------------------------------------- */
#define COSA_GT_STATS_SLOTS 7
size_t cosa_gt_stats_layout(int K, size_t *offsets);
int cosa_gt_stats(const uint8_t *gt, const float *mask_main, const float *mask_aux, const float *seg_logits, const float *cls_label,
                  const int32_t *boxes, int B, int K, int S, int h, int w, int ignore_index, unsigned long long *counters,
                  void *stream);
int cosa_gt_stats_uses_lds(int K);

/* ---------------------------------------------------------------------------------------
 * Per-tensor training diagnostics: norms, the EMA gap and the blame counters, over the record table
 * and chunk list of cosa_fused_adamw_ema.  Every buffer of the table (p, g, m, v, tp, the shadows) is only ever read.
 * `first_chunk`: device int32 [n_tensors + 1]: tensor t owns the chunks first_chunk[t] .. first_chunk[t+1] - 1 of the chunk
 *   list (contiguous and ascending; a tensor without elements owns none); first_chunk[0] == 0, first_chunk[n_tensors] ==
 *   n_chunks.
 * cosa_tensor_stats_layout: THE definition of a tensor's row for host and device: COSA_TENSOR_STATS_SLOTS 8-byte slots,
 *   offsets[] in bytes from the row's start, in the order
 *     g_sq        f64  sum of g^2 over the finite elements of the gradient; 0 for a frozen tensor (g == NULL)
 *     w_sq        f64  sum of p^2 over the finite elements of the student master
 *     gap_sq      f64  sum of (tp - p)^2 over the elements where both are finite
 *     g_absmax    f64  max of finite |g| (an fp32 value held in an f64 slot); 0 for a frozen or empty tensor
 *     g_nonfinite u64  elements of g with an all-ones exponent
 *     w_nonfinite u64  elements where p or tp has an all-ones exponent
 *   Returns the row's size in bytes (48), 0 when offsets is NULL.
 * cosa_tensor_stats: out [n_tensors][6] (8-byte aligned) = the rows, written whole by the call (a tensor without chunks gets a
 *   zero row).  One block per chunk leaves one partial row per chunk in `workspace` (cosa_tensor_stats_workspace_bytes,
 *   8-byte aligned); one thread per tensor then adds its chunks in index order, counts as integers, maxima as maxima: no
 *   float atomics, the same bits from run to run.  Sums are formed in double; the g_sq partial of a chunk is formed exactly
 *   as cosa_grad_norm forms its partial, a non-finite element contributing 0: on an all-finite chunk the two have the same bits.
 *   Refused with COSA_EINVAL, nothing launched and `out` untouched: a NULL pointer, n_tensors <= 0, n_chunks <= 0, a
 *   workspace that is too small or misaligned, a first_chunk that does not start at 0, is not monotone or does not end at
 *   n_chunks.  For that check the n_tensors + 1 ints are read back on a stream of the library's own (one per device, created
 *   on first use, thread-safe): the host waits for that copy and for nothing else -- the caller's stream is not waited for --
 *   and first_chunk must not be pending on another stream.  Two launches.
 * cosa_grad_blame: one launch, one thread per tensor, over the per-chunk partials cosa_grad_norm has just left in ITS
 *   workspace (`partials`: n_chunks doubles): blame[t] (uint64, caller-zeroed once, 8-byte aligned) advances by one when any
 *   of tensor t's partials is non-finite -- which is exactly when some element of its gradient is.  Ordinary loads and stores.
 *   first_chunk is not read back here (the call is made every step): the kernel clamps every range to 0 .. n_chunks.
 * ------------------------------------------------------------------------------------- */
#define COSA_TENSOR_STATS_SLOTS 6
size_t cosa_tensor_stats_layout(size_t *offsets);
size_t cosa_tensor_stats_workspace_bytes(int n_chunks);
int cosa_tensor_stats(const void *records, const void *chunks, const int *first_chunk, int n_tensors, int n_chunks, void *workspace,
                      size_t workspace_bytes, void *out, void *stream);
int cosa_grad_blame(const void *partials, const int *first_chunk, int n_tensors, int n_chunks, unsigned long long *blame, void *stream);

/* ---------------------------------------------------------------------------------------
 * The --teacher_check monitor: two teacher passes over the same weights and images, on two operand
 * modes (A, B), scored against each other by one reduction, accumulated on the device in a vector of uint64 counters.
 * cosa_teacher_check_layout: THE definition of that vector for host and device.  K = num_classes (background included,
 *   2..256).  offsets[COSA_TEACHER_CHECK_SLOTS] (in elements) of, in order: checks (calls accumulated); then for each map
 *   set (cam, aux, tgt): planes, over, worst, hist[COSA_TEACHER_CHECK_BINS], nonfinite_a, nonfinite_b; then for each label
 *   pair (main, aux): pix, agree, ign_a, ign_b, cnt_a[K], cnt_b[K], inter[K].  Returns the number of elements (48 + 6K), 0 on
 *   bad arguments.
 * cosa_teacher_check: camA/camB and auxA/auxB fp32 [B,C,S,S] (the min-max normalised CAMs of the two passes); tgtA/tgtB fp32
 *   [B,C,h,w] (the cam-loss targets; the pair may be NULL); mainA/mainB and lauxA/lauxB fp32 [B,S,S] label maps in {0..K-1,
 *   ignore_index} (the auxiliary pair may be NULL); cls_label fp32 [B,C] or NULL (every plane active); boxes int32 [B,4]
 *   (y0,y1,x0,x1).  An absent pair leaves its slots untouched.
 *   Per map set, over the ACTIVE planes (cls_label != 0; a plane of an absent class is never read): a plane's figure is the
 *   maximum of |a - b| over its elements, +inf (bits 0x7f800000) when either pass holds a non-finite element in it.  planes
 *   counts the active planes; over those with figure > bar (a figure equal to the bar is not over); worst is the largest
 *   figure met so far as its fp32 bit pattern (non-negative floats order as unsigned integers); hist[i] counts the planes in
 *   the first bin with figure <= edge, edges 1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, +inf as fp32; nonfinite_a /
 *   nonfinite_b count the non-finite elements of the active planes of each pass.
 *   Per label pair, over the pixels inside an image's box only: pix; agree (a == b, ignore counted as a value); ign_a,
 *   ign_b; per class k < K cnt_a[k], cnt_b[k] and inter[k] (a == b == k).  A value that is neither an integer in 0..K-1
 *   nor ignore_index is counted in pix (and, where the two maps hold the same value, in agree) only.
 *   Every sum is an integer atomic, every maximum an integer maximum of bit patterns of exactly computed fp32 values: the
 *   same bits in any order.  workspace: cosa_teacher_check_workspace_bytes(B, C) of device memory (0 on bad arguments),
 *   8-byte aligned, cleared by the call itself on `stream`.  Envelope: C <= 255, K == C + 1, B, S > 0, with a tgt pair h, w
 *   > 0 and <= S, ignore_index no class, bar >= 0; anything else is COSA_EINVAL, nothing is launched or clamped.  One
 *   memset node and two launches.
 * ------------------------------------------------------------------------------------- */
#define COSA_TEACHER_CHECK_SLOTS 33
#define COSA_TEACHER_CHECK_BINS 8
size_t cosa_teacher_check_layout(int K, size_t *offsets);
size_t cosa_teacher_check_workspace_bytes(int B, int C);
int cosa_teacher_check(const float *camA, const float *camB, const float *auxA, const float *auxB, const float *tgtA,
                       const float *tgtB, const float *mainA, const float *mainB, const float *lauxA, const float *lauxB,
                       const float *cls_label, const int32_t *boxes, int B, int C, int K, int S, int h, int w, int ignore_index,
                       float bar, unsigned long long *counters, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * The --student_check monitor: the student's training forward (a) against a second forward of the
 * same weights on the same images (b, the fp32 family by default), scored by one reduction, accumulated on the device in a
 * vector of uint64 counters (passed as long long: the values stay below 2^63).
 * cosa_student_check_counters(K): the number of elements, COSA_STUDENT_CHECK_HEAD + 2K; 0 for K outside 2..256.
 * The vector, in elements:
 *   0 checks (calls accumulated);  1 flags (sticky OR: bit t -- tensor t held a non-finite element or a term outside its
 *   fixed-point range, which then contributed to no sum; bit 8 + j -- the same for loss term j);
 *   2 + 7 t + f, tensors t = seg, cam, cam_aux, cls, cls_aux, fields f = elements compared, non-finite elements of a, of
 *   b, the largest finite |a - b| and the largest finite |b| as fp32 bit patterns (non-negative floats order as unsigned
 *   integers), sum (a - b)^2 with COSA_STUDENT_CHECK_D2_FRAC fractional bits, sum b^2 with COSA_STUDENT_CHECK_B2_FRAC;
 *   37 cells compared;  38 cells whose seg argmax differs;  39..42 those cells binned by the b pass's top-1 minus top-2
 *   margin: < 1e-3, < 1e-2, < 1e-1, the rest (the edges as fp32; a NaN margin, inf - inf, falls in the last bin);
 *   43, 44 columns of cls / cls_aux with sign(a) != sign(b) over all K-1 columns (the sign of NaN is 0);  45 columns seen
 *   per matrix (B (K-1) a call);
 *   46 + 4 j + f, loss terms j = cls, cls_aux, seg, cam, fields f = sum |a - b| and sum |b| with
 *   COSA_STUDENT_CHECK_LOSS_FRAC fractional bits, the largest |a - b| as bits, checks counted for the term;
 *   62 .. 62 + K: cells the b pass labels class k;  62 + K .. 62 + 2K: those among them where the a pass agrees.
 * Which elements: seg channels 0 (background) and 1 + c for every class c with cls_label[b][c] != 0; the CAM planes and the
 *   cls columns of those classes.  The argmax of a cell runs over the same seg channels (seg_validation's rule), NaN read as
 *   -inf, the lowest channel index among equals.
 * Fixed point: a term is computed in fp32 with round-to-nearest operations (d = a - b, d * d, b * b, |d|), multiplied by
 *   2^FRAC in double (exact) and rounded to an integer half-to-even.  It is added only when both elements are finite and the
 *   term is below 2^INT; FRAC + INT = 42, so 2^22 terms fit whatever their values.  (a - b)^2: 2^-32 resolves |a - b| down
 *   to 2e-5, the range reaches |a - b| < 32; b^2: logits and CAM scores of |b| < 2048 at a resolution of 1e-6; the losses:
 *   below 1024 at 2e-10.
 * Every figure is an integer sum, maximum or OR: the same counters in any order of arrival, on every run.  One launch, no
 *   workspace.  Envelope: every pointer non-NULL, counters 8-byte aligned, B, h, w > 0, 2 <= K <= 256, B K h w < 2^31;
 *   anything else is COSA_EINVAL and nothing is launched.
 * ------------------------------------------------------------------------------------- */
#define COSA_STUDENT_CHECK_MAX_K 256
#define COSA_STUDENT_CHECK_HEAD 62
#define COSA_STUDENT_CHECK_D2_FRAC 32
#define COSA_STUDENT_CHECK_D2_INT 10
#define COSA_STUDENT_CHECK_B2_FRAC 20
#define COSA_STUDENT_CHECK_B2_INT 22
#define COSA_STUDENT_CHECK_LOSS_FRAC 32
#define COSA_STUDENT_CHECK_LOSS_INT 10
size_t cosa_student_check_counters(int K);
int cosa_student_check(const float *seg_a, const float *seg_b, const float *cam_a, const float *cam_b, const float *aux_a,
                       const float *aux_b, const float *cls_a, const float *cls_b, const float *clsaux_a, const float *clsaux_b,
                       const float *loss_a, const float *loss_b, const float *cls_label, long long *counters, int B, int K, int h,
                       int w, void *stream);

/* ---------------------------------------------------------------------------------------
 * The --act_stats_iters monitor: activation range and attention sharpness of an fp32 no-grad pass
 * (csrc/act_stats_kernels.hip).  Both reductions ADD into int64 words that the caller zeroes: counts, per-row terms in fixed
 * point with COSA_ACT_STATS_FRAC fractional bits (rint of term * 2^32 in double), and maxima as the bit pattern of a finite
 * non-negative fp32 value under an integer max.  The same input gives the same bytes in any order of arrival; a second call
 * on the same words doubles counts and sums and keeps maxima.  One launch each, no workspace, no host sync.
 *   cosa_range_stats_f32   a column window of an fp32 matrix: `cols` columns from x, `rows` rows of stride ld (elements).
 *                          out6: 0 finite elements;  1 bits of the largest finite |x|;  2 finite |x| > 65504 (an fp16 hi
 *                          half would be inf);  3 finite |x| > 32768 (less than one bit of headroom);  4 elements with
 *                          0 < |x| < 2^-14 (the hi half goes subnormal);  5 non-finite elements.  Each byte of the window
 *                          is read once and nothing outside it; float4 loads where x is 16-byte aligned and ld % 4 == 0, a
 *                          scalar path otherwise.  Refused: a NULL pointer, rows < 1, cols < 1, ld < cols.
 *   cosa_attn_stats_f32    the logits of cosa_attn_fwd_f32 (same blocks, key tiles and MFMA orientation, scale applied to the
 *                          fp32 chain) without the PV product; nothing of size N^2 or N d is written.  Per query row, online:
 *                          the maximum m, l = sum e^(s-m), t = sum e^(s-m)(s-m) (expf in fp32, the sums carried in double);
 *                          H = log l - t / l, Hn = H / log N clamped to [0, 1] (0 for N = 1), top1 = 1 / l.
 *                          out [H][COSA_ACT_STATS_HEAD_WORDS]: 0 rows;  1 sum rint(Hn 2^32);  2 sum rint(top1 2^32);
 *                          3 rows with top1 > 0.5;  4 bits of the largest finite |s|;  5 bits of max (1 - Hn) as fp32 (0:
 *                          nothing seen);  6 rows with a non-finite logit, which are left out of words 0..5.
 *                          Envelope as cosa_attn_fwd_f32: head_dim == 64, ldq >= 3 H 64, ldq % 4 == 0, 16-byte aligned qkv.
 * Anything else is COSA_EINVAL, nothing is launched and the words are untouched.
 * ------------------------------------------------------------------------------------- */
#define COSA_ACT_STATS_RANGE_WORDS 6
#define COSA_ACT_STATS_HEAD_WORDS 7
#define COSA_ACT_STATS_FRAC 32
int cosa_range_stats_f32(const float *x, long long rows, int cols, long long ld, int64_t *out6, void *stream);
int cosa_attn_stats_f32(const float *qkv, int B, int N, int H, int head_dim, float scale, long long ldq, int64_t *out /* [H][7] */,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * The --grad_check_iters check (csrc/grad_check_kernels.hip): the step's raw fp32 gradient g against
 * central differences of the loss along g itself.  These two entry points are the streams over the parameters; the losses
 * are evaluated by the caller between them.
 * The table: n_tensors records {const float *w; const float *g; float *dst; int64 n; int32 dir; int32 pad}
 *   (COSA_GRAD_CHECK_RECORD_BYTES each) followed at once by n_chunks {int32 tensor; int32 chunk}: every chunk of
 *   COSA_GRAD_CHECK_CHUNK elements of every tensor once, tensors ascending, a tensor's chunks from 0.  dir: the direction the
 *   tensor belongs to, -1 for none (g may then be NULL).  The table is passed twice: `table_host`, on which the envelope is
 *   checked, and `table_dev`, the device copy of the same bytes the kernels read.
 * The record: n_dirs rows of COSA_GRAD_CHECK_RECORD doubles --
 *   COSA_GRAD_CHECK_G2 sum g^2;  _W2 sum w^2 (both in double over the direction's tensors);  _S the step length
 *   float(rho sqrt(W2 / G2)) as a double;  _FLAGS the OR of COSA_GRAD_CHECK_FLAG_* (s is 0 whenever one is set);
 *   _T + k, k < COSA_GRAD_CHECK_STEPS, the realised step sum (dst - w) g of perturb's slot k;  _LOSS + 5 j + i the caller's:
 *   loss term i at evaluation j (0: at w, 1 + k: at slot k's weights);  _BAD_G, _BAD_W the non-finite elements counted.
 * cosa_grad_check_norms    writes G2, W2, S, FLAGS, BAD_G, BAD_W of every row.  rho finite and > 0.
 * cosa_grad_check_perturb  reads row `dir`'s S on the device (no host sync) and writes, for EVERY tensor of the table,
 *                          dst = w + fl32(fl32(c S) g) inside direction `dir` -- the product and the sum rounded separately
 *                          -- and dst = w outside it or with S = 0; then row `dir`'s T + slot.  c finite.
 * Sums: each thread adds its strided elements in double, a wavefront's sums meet in an xor butterfly, the wavefronts in wave
 *   order, one partial per chunk, the partials lane-strided in chunk order: no atomics, the same bytes on every run.  dwordx4
 *   accesses where w, g and dst are 16-byte aligned, single elements otherwise.  Two launches each, no host sync.
 * Workspace: cosa_grad_check_workspace_bytes(n_chunks) serves both.
 * Refused with COSA_EINVAL, nothing launched and nothing written: a NULL table, record or workspace, counts < 1, a record
 *   with n < 0, dir outside [-1, n_dirs), a NULL or misaligned w / dst, a direction's tensor without g, a chunk list that is
 *   not exactly the tensors' chunks in order, a short workspace, a non-finite or non-positive rho, a non-finite c, `dir`
 *   outside [0, n_dirs), `slot` outside [0, COSA_GRAD_CHECK_STEPS).
 * ------------------------------------------------------------------------------------- */
#define COSA_GRAD_CHECK_CHUNK 16384
#define COSA_GRAD_CHECK_RECORD_BYTES 40
#define COSA_GRAD_CHECK_RECORD 36
#define COSA_GRAD_CHECK_STEPS 4
#define COSA_GRAD_CHECK_G2 0
#define COSA_GRAD_CHECK_W2 1
#define COSA_GRAD_CHECK_S 2
#define COSA_GRAD_CHECK_FLAGS 3
#define COSA_GRAD_CHECK_T 4
#define COSA_GRAD_CHECK_LOSS 8
#define COSA_GRAD_CHECK_BAD_G 33
#define COSA_GRAD_CHECK_BAD_W 34
#define COSA_GRAD_CHECK_FLAG_ZERO_GRAD 1   /* G2 == 0 (or the direction is empty)                     */
#define COSA_GRAD_CHECK_FLAG_BAD_GRAD 2    /* a non-finite gradient element or a non-finite G2        */
#define COSA_GRAD_CHECK_FLAG_BAD_WEIGHT 4  /* a non-finite weight or a non-finite W2                  */
#define COSA_GRAD_CHECK_FLAG_NO_STEP 8     /* rho sqrt(W2 / G2) is 0 or outside fp32                  */
size_t cosa_grad_check_workspace_bytes(int n_chunks);
int cosa_grad_check_norms(const void *table_host, const void *table_dev, int n_tensors, int n_chunks, int n_dirs, double rho,
                          double *record, void *workspace, size_t workspace_bytes, void *stream);
int cosa_grad_check_perturb(const void *table_host, const void *table_dev, int n_tensors, int n_chunks, int n_dirs, int dir,
                            float c, int slot, double *record, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * The supervised-contrastive token loss (csrc/tokcon_kernels.hip): this project's own objective on the
 * student's final patch tokens, off by default.
 * cosa_token_labels   label map [B,S,S] (uint8 or int64 elements of value 0..255, elem_bytes 1 | 8; the low byte is read) ->
 *                     labels uint8 [B,(S/p)^2]: the class holding >= need of the token's p x p pixels, else 255.  need in
 *                     (p^2 / 2, p^2], so at most one class qualifies.  Byte loads and integer counts; one launch.
 * cosa_token_contrast_fwd   tokens bf16 [B,n,768] contiguous, labels uint8 [B,n], tau.  Per image z = x / max(|x|, 1e-12) in
 *                     fp32, s_ij = z_i . z_j / tau on the f32-input MFMA, A(i) = labelled j != i, P(i) = those with y_i's
 *                     label, anchors = labelled i with |P(i)| >= 1, M their number over the batch;
 *                     loss = (1/M) sum_anchors (log sum_A exp s_ia - (1/|P(i)|) sum_P s_ij), an exact 0 with M = 0.
 *                     Writes rows float [2][B][n] (lse_i, sum_P s_ij), counts int32 [B*256 + 1] (per-image class counts,
 *                     then M) and loss float [1].  Nothing of size n^2 is written; no float atomics, no host sync.
 * cosa_token_contrast_bwd   dx bf16 [B,n,768] = upstream[0] * dL/dx from the same tokens / labels and the forward's rows and
 *                     counts: per image W = G + G^T into scratch (G_ij = (1/M)(exp(s_ij - lse_i)[j in A(i)] - [j in
 *                     P(i)]/|P(i)|) on anchor rows), dZ = W Z on the f32-input MFMA, then per row
 *                     (dZ_i - (dZ_i . z_i) z_i) upstream / (tau max(|x_i|, 1e-12)) rounded once.  upstream: a device float.
 * Envelope of both: dim == 768, 1 <= B <= 65535, 2 <= n <= 4096, 0.01 <= tau <= 10, 16-byte aligned tokens / dx /
 * workspace of cosa_token_contrast_workspace_bytes(B, n) bytes (at most 256 MiB unless one image needs more: the batch is
 * walked in image chunks, which moves no bit).  Anything else is COSA_EINVAL and nothing is launched.
 * cosa_token_junction_bwd4  cosa_token_junction_bwd for four consumers: dx fp32 [B,N,768] = 0 in the class-token row,
 *                     g0 + g1 + g2 + g3 elsewhere (fp32 adds in that order, absent ones null); g bf16 [B,N-1,768].
 * ------------------------------------------------------------------------------------- */
int cosa_token_labels(const void *mask, int elem_bytes, uint8_t *labels, int B, int S, int p, int need, void *stream);
size_t cosa_token_contrast_workspace_bytes(int B, int n);
int cosa_token_contrast_fwd(const void *tokens, const uint8_t *labels, float *rows, int32_t *counts, float *loss, int B, int n, int dim,
                            float tau, void *workspace, size_t workspace_bytes, void *stream);
int cosa_token_contrast_bwd(const void *tokens, const uint8_t *labels, const float *rows, const int32_t *counts, const float *upstream,
                            void *dx, int B, int n, int dim, float tau, void *workspace, size_t workspace_bytes, void *stream);
int cosa_token_junction_bwd4(const void *g0, const void *g1, const void *g2, const void *g3, float *dx, int B, int N, int dim, void *stream);

/* ---------------------------------------------------------------------------------------
 * The per-pixel weight of the reliability-weighted seg loss (csrc/reliability_kernels.hip): this project's own
 * weighting, off by default.  For CAM set g with thresholds (hi, lo), image b, pixel p, l = (int)masks[g][b,p], y = labels[b]:
 *   l == 0        m = max_c (y[c] cams[g][b,c,p]),  r = (lo - m) / lo
 *   1 <= l <= C   v = y[l-1] cams[g][b,l-1,p],      r = (v - hi) / (1 - hi)
 *   otherwise     rel = 0, and the pixel enters no statistic
 *   r = (r != r) ? 0 : min(max(r, 0), 1);  u = 1 (beta == 0) | r (beta == 1) | (r == 0 ? 0 : exp2f(beta log2f(r)))
 *   rel[g][b,p] = floor + (1 - floor) u            (fp32 in this order, no contraction; floor == 0 gives u exactly)
 * cams / masks / rel: host arrays of G device pointers ([B,C,S,S] / [B,S,S] / [B,S,S] fp32), labels [B,C] in {0,1}: multiplying by y
 * folds cam_validation in, so raw and validated CAMs give the same map.  The plane of a class absent from y is never read.
 * thr_hi / thr_lo: host float[G]; thr_dev (optional): device float[G][2] = (hi, lo) per set, read by the kernel instead -- no host
 * sync under adaptive thresholds, as cosa_cam2mask_multi.  stats (optional): device int64 [G][4] = {Sum_bg rint(rel 2^32), n_bg,
 * Sum_fg rint(rel 2^32), n_fg}, ADDED to with integer atomics (no float atomics: the same bytes every run).  One launch for all sets.
 * Envelope: 1 <= G <= 4, 1 <= C <= 255, 1 <= B <= 65535, 1 <= S <= 32768 (no alignment demand: float4 accesses where S*S % 4 == 0
 * and the pointers allow, scalar ones elsewhere), 0 <= beta <= 8, 0 <= floor < 1.  Anything else is COSA_EINVAL and nothing is launched.
 * ------------------------------------------------------------------------------------- */
int cosa_label_reliability(const float *const *cams, const float *labels, const float *const *masks, float *const *rel,
                           const float *thr_hi, const float *thr_lo, const float *thr_dev, int G, int B, int C, int S, float beta, float floor,
                           long long *stats, void *stream);

/* y[i] = the deterministic expf (spec E) as the export translation unit computes it: a test hook */
int cosa_spec_expf(const float *x, float *y, long long n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* COSA_HIP_H */
