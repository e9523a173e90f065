/*
 * umamd -- MI355X (gfx950) kernels for the self-supervised depth+uncertainty
 * training step of Probabilistic-Surgical-Vision/uncertainty-model.
 *
 * C ABI (drop-in boundary under the Python host layer in
 * uncertainty-model_amd/umamd/).  Rules:
 *   - plain pointers, sizes and enums only; no torch types;
 *   - device pointers are caller-owned (PyTorch caching allocator); the
 *     library never allocates or frees and never synchronises the host;
 *   - every entry takes the HIP stream to launch on (torch's current stream);
 *   - returns UM_OK (0) or an error code; um_last_error() gives a
 *     thread-local message (entries are called from PyTorch's autograd thread).
 *
 * Tensor conventions: activations are NHWC with a pixel stride `ld`
 * (elements between consecutive pixels; >= channels), element type UM_F32 or
 * UM_BF16 as given by `dtype`; arithmetic is always f32.  Conv weights are
 * repacked per step from the reference's NCHW f32 parameters
 * ([K][C][R][R], reference nn.Conv2d) into [K][R][R][Cp] ("forward") and
 * [Cp][R][R][K] ("transposed", for the data gradient), Cp = C rounded up to 8.
 *
 * Each entry cites the reference operation it replaces (file:line in the
 * reference repository).
 */
#ifndef UMAMD_H
#define UMAMD_H

#include <hip/hip_runtime.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UM_OK = 0, UM_ERR_ARG = 1, UM_ERR_HIP = 2 };
enum { UM_F32 = 0, UM_BF16 = 1 };
/* OR'ed into the dtype of the um_bn_elu_* entries (and um_conv2d_fwd_up2's): the pre-BN conv output y is stored in the activation
 * dtype instead of f32 (the bf16 build's default, as a bf16 autocast conv
 * feeding BatchNorm2d; statistics are still taken in f32 in the conv
 * epilogue).  um_conv2d_fwd_up2: y and the low-resolution map up2. */
enum { UM_Y_ACT = 0x100 };
enum { UM_PAD_ZERO = 0, UM_PAD_REFLECT = 1 };
enum {
  UM_EPI_NONE = 0,           /* y = acc (+ bias)                               */
  UM_EPI_STATS = 1,          /* y = acc + bias, per-block BN partial sums      */
  UM_EPI_SIGMOID_SCALE = 2,  /* y(f32) = scale * sigmoid(acc + bias)           */
  UM_EPI_RESIDUAL = 3,       /* y = acc + bias + residual                      */
  UM_EPI_STAT_SLOTS = 4,     /* y = acc + bias, BN sums f64-atomically added into
                                stats_partials viewed as double[UM_STAT_SLOTS][K][2]
                                (zeroed by the caller; see um_bn_elu_fwd_slots)  */
  UM_EPI_ELU = 5             /* y = elu(acc + bias), stored in ydtype (the
                                activation dtype or f32): the inference form of
                                Conv2d -> BatchNorm2d(eval) -> ELU with the BN
                                folded into wf / bias (um_bn_fold).  um_conv2d_fwd
                                only (not um_conv2d_fwd_up2); takes no statistics
                                and never accumulates                            */
};
/* f64 slots of the atomic BN statistics (UM_EPI_STAT_SLOTS, *_slots entries) */
#define UM_STAT_SLOTS 16

const char* um_last_error(void);
int um_version(void);
/* kernel-selection values ("tuning keys"; tests force code paths, tuning
 * sweeps): every key of the table in uncertainty-model_amd/csrc/knobs.h, the
 * same keys UMAMD_TUNING="key=value,..." presets at load.  Returns the
 * previous value, -1 for an unknown key. */
int um_set_tuning(const char* key, int value);

/* ---------------------------------------------------------------- conv ---
 * Replaces nn.Conv2d forward/backward with its padding:
 *   encoder ConvELUBlock: F.pad zero + Conv2d(k, stride)
 *       reference model/layers/encoder.py:42-52
 *   decoder ConvLayer: ReflectionPad2d(1) + Conv2d(3) / 1x1 without padding
 *       reference model/layers/decoder.py:30-52
 *   attention 1x1 K/Q/V/reprojection: reference model/layers/attention.py:37-40,66-76
 * Implicit GEMM on MFMA (bf16: v_mfma_f32_16x16x32_bf16, f32: v_mfma_f32_16x16x4_f32).
 */
/* number of BN partial rows written by um_conv2d_fwd with UM_EPI_STATS for M
 * output pixels and K channels (UM_EPI_STAT_SLOTS writes UM_STAT_SLOTS f64 rows
 * instead, through the same stats_partials pointer) */
int um_conv_stats_parts(int M, int K);

/* split-K workspace (bytes) the kernels want for a shape; 0 = no split.
 * Passing a smaller (or null) workspace is allowed: the split shrinks. */
long um_conv_fwd_ws(int dtype, int N, int P, int Q, int K, int R, int C);
/* the data gradient's, plus the padded-input buffer of the reflect data
 * gradient's padded form (knob "pad_dgrad"): a zero-pad transposed conv onto
 * the (H+2p) x (W+2p) reflect-padded input, folded back onto dx */
long um_conv_dgrad_ws_pad(int dtype, int N, int H, int W, int C, int R, int K, int stride,
                          int pad, int pad_mode);

int um_conv2d_fwd(int dtype, int N, int H, int W, int C, int ldx, const void* x,
                  const void* wf, const float* bias, int K, int R, int stride,
                  int pad, int pad_mode, int P, int Q, int ydtype, void* y,
                  int ldy, int epilogue, float epi_scale, const void* residual,
                  int ldr, float* stats_partials, void* ws, long ws_bytes,
                  hipStream_t stream);

/* 1x1 conv forward (f32 output, zero pad, stride 1) plus the bilinear x2
 * (align_corners=True) upsample of a low-resolution f32 map added before the
 * epilogue's BN statistics: y = W x + bias + up2(z), z = [N][up2_h][up2_w]
 * [up2_ld] (channels [0, K) used).  The decoder's cat(feature_map,
 * interpolate(skip)) -> 1x1 conv (reference model/layers/decoder.py:230-238)
 * with the skip half convolved at the skip's resolution (the 1x1 conv and
 * the upsample commute): the full-resolution concat is never built. */
int um_conv2d_fwd_up2(int dtype, int N, int H, int W, int C, int ldx, const void* x,
                      const void* wf, const float* bias, int K, int P, int Q, void* y, int ldy,
                      int epilogue, float* stats, const void* up2, int up2_h, int up2_w,
                      int up2_ld, hipStream_t stream);
/* data gradient: dx[N,H,W,C] (= or +=) conv^T(dy[N,P,Q,K], wT) incl. the
 * reflect-pad fold and the stride-2 scatter */
int um_conv2d_dgrad(int dtype, int N, int H, int W, int C, int ldx, void* dx,
                    int accumulate, const void* wT, int K, int R, int stride,
                    int pad, int pad_mode, int P, int Q, const void* dy, int ldy,
                    void* ws, long ws_bytes, hipStream_t stream);
/* 1 when um_conv2d_fwd (dgrad 0) or the main pass of um_conv2d_dgrad (dgrad 1:
 * x is [N][H][W][C], dy [N][P][Q][K], with the workspace of
 * um_conv_dgrad_ws_pad) would run on the halo-tiled kernel (csrc/halo_conv.hip)
 * under the current tuning keys, else 0.  Dense operands (ldx = C, ldy = K);
 * the dispatch itself decides, so this cannot drift from it.  Host only: needs
 * no device.  The halo kernel does not take partial-row statistics
 * (UM_EPI_STATS) unless P % 8 == 0 and Q % 32 == 0, nor reflect padding where
 * a tile's halo would need a second reflection. */
int um_conv_halo_ok(int dtype, int N, int H, int W, int C, int K, int R, int stride, int pad,
                    int pad_mode, int P, int Q, int epilogue, int dgrad);

/* weight gradient partial slabs [splits][K][R*R*C] (f32); splits from
 * um_conv_wgrad_splits (which also picks the kernel: the halo-tiled one for
 * bf16 small-channel spatial convs, the implicit-GEMM one otherwise) */
int um_conv_wgrad_splits(int dtype, int N, int H, int W, int C, int ldx, int K, int R,
                         int stride, int pad, int pad_mode, int P, int Q, int ldy);
int um_conv2d_wgrad(int dtype, int N, int H, int W, int C, int ldx, const void* x,
                    int K, int R, int stride, int pad, int pad_mode, int P, int Q,
                    const void* dy, int ldy, float* slabs, int splits,
                    hipStream_t stream);

/* um_conv_wgrad_reduce_seg: sum slabs -> reference NCHW weight grad
 * [Kreal][Creal][R][R] (f32), (+)=.  Segments (both entries): reference input
 * channels [src0[i], src0[i]+len[i]) are placed at packed channels
 * [dst0[i], ...) (host arrays, nseg <= 4; nseg = 0: channel c at c); the rest
 * of the packed channels are zero.  Keeps concat sources 8-channel aligned. */
int um_conv_wgrad_reduce_seg(const float* slabs, int splits, int K, int Kreal, int R, int C,
                             int Creal, float* dw, int accumulate, int nseg, const int* src0,
                             const int* dst0, const int* len, hipStream_t stream);
int um_pack_weight_seg(int dtype, const float* w, int K, int Creal, int R, int C, void* wf,
                       void* wT, int ldT, int nseg, const int* src0, const int* dst0,
                       const int* len, hipStream_t stream);

/* Batched repack of many conv weights in ONE launch (the per-step weight
 * refresh of every conv in the model).  Each descriptor is one
 * um_pack_weight_seg call; a descriptor covers um_pack_tiles(K, C, R)
 * workgroups, numbered from `block0`;
 * blk2desc[b] (device int array, nblocks entries) names the descriptor of
 * workgroup b.  `table` and `blk2desc` are device memory (caller-owned). */
#define UM_PACK_MAXSEG 4
typedef struct {
  const float* w;   /* [K][Creal][R][R] f32 */
  void* wf;         /* [K][R][R][C] (nullable) */
  void* wT;         /* [C][R][R][ldT] (nullable; column offset applied) */
  int K, Creal, R, C, ldT, block0;
  int nseg, src0[UM_PACK_MAXSEG], dst0[UM_PACK_MAXSEG], len[UM_PACK_MAXSEG];
  int split;        /* bf16 only: pack 2K rows, see um_pack_weight_split (tiles: 2K) */
} um_pack_desc;
int um_pack_batch(int dtype, const um_pack_desc* table, int ndesc, const int* blk2desc,
                  int nblocks, hipStream_t stream);
int um_pack_tiles(int K, int C, int R);
/* sizeof(um_pack_desc), for bindings that build the table */
int um_pack_desc_size(void);

/* repack f32 NCHW weight [K][Creal][R][R] -> wf [K][R][R][C] (row stride ldf
 * elements) and wT [C][R][R][ldT] (column offset applied by the caller); C >= Creal, zero fill */
int um_pack_weight(int dtype, const float* w, int K, int Creal, int R, int C,
                   void* wf, void* wT, int ldT, hipStream_t stream);

/* split-bf16 pack (bf16 only): wf [2K][R][R][C] and wT [C][R][R][ldT >= 2K]
 * hold rows k < K = bf16(w[k]) and rows K + k = bf16(w[k] - bf16(w[k])), so a
 * GEMM over the 2K rows whose output pairs (k, K + k) are summed in f32 sees
 * the f32 weight to ~2^-17 relative at bf16 MFMA rates.  Used by the
 * disparity/uncertainty heads (reference model/layers/decoder.py:244-247),
 * whose 4 outputs pad to 8 GEMM columns anyway. */
int um_pack_weight_split(const float* w, int K, int Creal, int R, int C, void* wf, void* wT,
                         int ldT, hipStream_t stream);

/* per-channel column sums of y[M][C] (pixel stride ld) -> partial rows [parts][C] */
/* Several bias gradients (um_colsum + um_reduce_rows each) in two launches:
 * the weight-gradient side stream batches the bias reductions of a flush
 * (the attention's K/Q/V/reprojection and the disparity heads' conv biases,
 * reference model/layers/attention.py:24-33, decoder.py:244-247).  descs:
 * HOST array of n <= UM_CSUM_MAX entries (passed by value); out[c] =
 * sum_m y[m][c] for c < creal, parts = a [nparts][C] f32 workspace with
 * nparts = um_colsum_parts(M); one dtype for all entries. */
#define UM_CSUM_MAX 24
typedef struct {
  const void* y;
  float* parts;
  float* out;
  int M, C, ld, nparts, creal;
} um_csum_desc;
int um_colsum_batch(int dtype, const um_csum_desc* descs, int n, hipStream_t stream);
int um_colsum_parts(int M);
int um_colsum(int dtype, int M, int C, int ld, const void* y, float* partials,
              hipStream_t stream);
/* out[c] (+)= sum_p partials[p][c*1] (row stride `stride`), one launch;
 * ws: um_colred_ws(parts, C, 1) bytes (f64 slab rows of the per-workgroup sums) */
int um_reduce_rows(const float* partials, int parts, int C, int stride, float* out,
                   int accumulate, double* ws, hipStream_t stream);
/* workspace bytes of the one-launch column reductions (nv values per channel) */
long um_colred_ws(int nparts, int C, int nv);

/* ------------------------------------------------------------------ BN ---
 * Training-mode nn.BatchNorm2d + nn.ELU, reference model/layers/encoder.py:43-44,
 * model/layers/decoder.py:82-84; SyncBatchNorm semantics when the host
 * all-reduces the f64 per-channel sums between the phases
 * (reference parallel_main.py:157).
 */
/* f64 per-channel sums of [nparts][C][2] partials (the SyncBN path all-reduces them
 * before um_bn_coeffs / um_bn_bwd_coeffs); ws: um_colred_ws(nparts, C, 2) bytes */
int um_bn_stats_reduce(const float* parts, int nparts, int C, double* out, double* ws,
                       hipStream_t stream);
/* single-process BN: reduce the forward partials AND compute the coefficients
 * (+ running statistics) in one launch (um_bn_stats_reduce + um_bn_coeffs) */
int um_bn_stats_coeffs(const float* parts, int nparts, int C, double* ws, double count,
                       const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, long long* num_batches_tracked,
                       float* mean, float* invstd, float* scale, float* shift,
                       hipStream_t stream);
/* single-process BN backward: reduce the bwd partials and compute k1..k3,
 * dgamma, dbeta in one launch (um_bn_stats_reduce + um_bn_bwd_coeffs).
 * dbias (optional): the gradient of the bias of the conv feeding this BN,
 * sum_m dy = k1 (sum dz - n k2 - k3 sum xhat) with sum xhat = 0 by
 * construction of the batch mean -- evaluated in closed form from the
 * reduced sums instead of a reduction of dy over the pixels */
int um_bn_bwd_stats_coeffs(const float* parts, int nparts, int C, double* ws, double count,
                           const float* gamma, const float* invstd, float* dgamma,
                           float* dbeta, float* dbias, float* k1, float* k2, float* k3,
                           hipStream_t stream);
/* count <= 0: read the element count from stats[2C] (SyncBN: the per-rank
 * counts are all-reduced with the statistics) -- also for um_bn_bwd_coeffs */
int um_bn_coeffs(const double* stats, double count, int C, const float* gamma,
                 const float* beta, float eps, float momentum, float* running_mean,
                 float* running_var, long long* num_batches_tracked, float* mean,
                 float* invstd, float* scale, float* shift, hipStream_t stream);
/* Inference: fold an eval-mode nn.BatchNorm2d (running statistics) into the
 * nn.Conv2d in front of it, so that Conv2d -> BatchNorm2d.eval() -> ELU
 * (reference model/layers/encoder.py:41-44, model/layers/decoder.py:80-84)
 * becomes one um_conv2d_fwd(UM_EPI_ELU).  Per output channel k, in f64:
 *   s[k]         = gamma[k] / sqrt(running_var[k] + eps)
 *   w_out[k,...] = w[k,...] * s[k]                      ([K][Creal][R][R], f32)
 *   b_out[k]     = (bias[k] - running_mean[k]) * s[k] + beta[k]
 * gamma / beta null: 1 / 0 (affine=False); bias null: 0; running_mean and
 * running_var null: no BN (w_out = w, b_out = bias).  All buffers f32,
 * caller-owned; w_out then goes through um_pack_weight_seg.  Build / refresh
 * time only (one small launch per layer). */
int um_bn_fold(const float* w, const float* bias, int K, int Creal, int R, const float* gamma,
               const float* beta, const float* running_mean, const float* running_var,
               float eps, float* w_out, float* b_out, hipStream_t stream);
/* pool_parts (optional, SE squeeze of decoder.py:124-136 fused in): per-block
 * channel sums of a, [um_bn_fwd_pool_parts_c(M, HW, C)][C], HW = pixels per
 * image (the forward pass may split small layers into 64-channel slices with
 * their own row blocking): the pool row count um_bn_elu_fwd /
 * um_bn_elu_fwd_slots write */
int um_bn_fwd_pool_parts_c(long M, long HW, int C);
int um_bn_elu_fwd(int dtype, long M, int C, const void* y, int ldy, const float* scale,
                  const float* shift, void* a, int lda, int apply_elu, long HW, float* pool_parts,
                  hipStream_t stream);
/* BN with the statistics in f64 slots (no reduction launch): the conv ran
 * with UM_EPI_STAT_SLOTS into `slots` ([UM_STAT_SLOTS][C][2], count = M
 * elements per channel); every workgroup sums the slots and derives
 * scale/shift itself, workgroup 0 also writes mean/invstd/scale/shift (kept
 * for the backward) and updates the running statistics -- the semantics of
 * um_bn_stats_coeffs + um_bn_elu_fwd in one launch.  The conv (and
 * um_bn_elu_bwd_reduce_slots) also store the element count after the slots
 * (slots[UM_STAT_SLOTS*C*2], so a slot buffer holds UM_STAT_SLOTS*C*2 + 1
 * doubles); SyncBN all-reduces slots + count and passes count <= 0 to read
 * the global count there. */
int um_bn_elu_fwd_slots(int dtype, long M, int C, const void* y, int ldy, const double* slots,
                        double count, const float* gamma, const float* beta, float eps,
                        float momentum, float* running_mean, float* running_var,
                        long long* num_batches_tracked, float* mean, float* invstd, float* scale,
                        float* shift, void* a, int lda, int apply_elu, long HW, float* pool_parts,
                        hipStream_t stream);
/* um_bn_elu_fwd_slots plus the NodeBlock merge of the next graph node
 * (reference model/layers/encoder.py:115-124): merged = sum_i
 * sigmoid(w[widx[i]]) * src_i over nsrc (2..8) sources [M][lda] of the
 * activation dtype, where source `self` is the a this call writes (srcs[self]
 * is ignored).  Replaces um_bn_elu_fwd_slots + um_merge_fwd when this layer
 * is the last predecessor computed before that node. */
int um_bn_elu_fwd_slots_merge(int dtype, long M, int C, const void* y, int ldy,
                              const double* slots, double count, const float* gamma,
                              const float* beta, float eps, float momentum, float* running_mean,
                              float* running_var, long long* num_batches_tracked, float* mean,
                              float* invstd, float* scale, float* shift, void* a, int lda,
                              int apply_elu, int nsrc, const void* const* srcs, const int* widx,
                              const float* w, int self, void* merged, hipStream_t stream);
/* backward sums (sum dz, sum dz*xhat) added into zeroed f64 slots
 * [UM_STAT_SLOTS][C][2] instead of partial rows */
int um_bn_elu_bwd_reduce_slots(int dtype, long M, int C, long HW, const void* da, int ldda,
                               const void* y, int ldy, const float* mean, const float* invstd,
                               const float* scale, const float* shift, const float* add_nc,
                               int apply_elu, double* slots, hipStream_t stream);
/* dy from the slot sums: every workgroup derives k1..k3 (as
 * um_bn_bwd_stats_coeffs), workgroup 0 writes dgamma, dbeta and the
 * closed-form conv-bias gradient dbias times dbias_scale (each optional).
 * SyncBN: slots are all-reduced (count <= 0 reads the count after them, as
 * um_bn_elu_fwd_slots), local_slots are this rank's slots before the
 * all-reduce (dgamma/dbeta from local sums, as torch SyncBatchNorm) and
 * dbias_scale = 1/world; single process: local_slots null, dbias_scale 1 */
int um_bn_elu_bwd_apply_slots(int dtype, long M, int C, long HW, const void* da, int ldda,
                              const void* y, int ldy, const float* mean, const float* invstd,
                              const float* scale, const float* shift, const float* add_nc,
                              int apply_elu, const double* slots, double count,
                              const double* local_slots, const float* gamma, float* dgamma,
                              float* dbeta, float* dbias, float dbias_scale, void* dy, int lddy,
                              hipStream_t stream);
int um_bn_bwd_parts(long M);
int um_bn_elu_bwd_reduce(int dtype, long M, int C, long HW, const void* da, int ldda,
                         const void* y, int ldy, const float* mean, const float* invstd,
                         const float* scale, const float* shift, const float* add_nc,
                         int apply_elu, float* parts, hipStream_t stream);
/* dbias as in um_bn_bwd_stats_coeffs from the all-reduced sums, times
 * dbias_scale (SyncBN: 1/world, so that the data-parallel gradient average
 * over ranks gives the global sum's average, as the reference's DDP does) */
int um_bn_bwd_coeffs(const double* stats, double count, int C, const float* gamma,
                     const float* invstd, const double* stats_local, float* dgamma,
                     float* dbeta, float* dbias, float dbias_scale, int accumulate, float* k1,
                     float* k2, float* k3, hipStream_t stream);
/* sum_parts (optional): per-block partial sums of dy, [um_bn_bwd_parts(M)][C]
 * (the conv-bias gradient, reduced by um_reduce_rows; only needed when no
 * coefficient kernel supplies it) */
int um_bn_elu_bwd_apply(int dtype, long M, int C, long HW, const void* da, int ldda,
                        const void* y, int ldy, const float* mean, const float* invstd,
                        const float* scale, const float* shift, const float* add_nc,
                        int apply_elu, const float* k1, const float* k2, const float* k3,
                        void* dy, int lddy, float* sum_parts, hipStream_t stream);

/* ------------------------------------------------------- encoder misc ---
 * NodeBlock merge, reference model/layers/encoder.py:115-124 (F3 index map
 * passed in widx: input i weighted by sigmoid(w[widx[i]])).
 */
/* Several um_merge_wgrad calls in ONE launch (one workgroup each): the
 * weight-gradient side stream batches the merge-weight gradients of a flush.
 * descs: HOST array of n <= UM_MWG_MAX entries, passed by value. */
#define UM_MWG_MAX 24
#define UM_MWG_SRC 8
typedef struct {
  const float* parts;  /* [nparts][nsrc] (um_merge_bwd) */
  const float* w;
  float* dw;
  int nparts, nsrc, nw, accumulate;
  int widx[UM_MWG_SRC];
} um_mwg_desc;
int um_merge_wgrad_batch(const um_mwg_desc* descs, int n, hipStream_t stream);
/* coefficient of input i: sigmoid(w[widx[i]]) if w, else coefs[i] (host array), else 1 */
int um_merge_fwd(int dtype, int nsrc, const void* const* srcs, const int* widx,
                 const float* w, const float* coefs, long count, void* dst, hipStream_t stream);
int um_merge_parts(long count);
int um_merge_bwd(int dtype, int nsrc, const void* const* srcs, void* const* dsrcs,
                 const int* accumulate, const int* widx, const float* w, const float* coefs,
                 long count, const void* dm, float* parts, hipStream_t stream);
/* um_merge_bwd that also takes the BN-ELU backward statistics of source fsrc,
 * whose gradient dsrcs[fsrc] it completes (the same sums as
 * um_bn_elu_bwd_reduce_slots over that gradient as stored, into `slots`):
 * reference model/layers/encoder.py:115-124 (merge) + 42-44 (BN+ELU).
 * dtype: activation dtype | UM_Y_ACT (the pre-BN y's type);
 * C / 8 must divide 256 */
/* partial rows of um_merge_bwd_bn's merge-weight dot products (its grid) */
int um_merge_bn_parts(long count);
int um_merge_bwd_bn(int dtype, int nsrc, const void* const* srcs, void* const* dsrcs,
                    const int* accumulate, const int* widx, const float* w, const float* coefs,
                    long count, const void* dm, float* parts, int fsrc, const void* y, int C,
                    const float* mean, const float* invstd, const float* scale,
                    const float* shift, int apply_elu, double* slots, hipStream_t stream);
int um_merge_wgrad(const float* parts, int nparts, int nsrc, const int* widx,
                   const float* w, float* dw, int nw, int accumulate, hipStream_t stream);
int um_image_to_nhwc(int dtype, const float* x, int N, int C, int H, int W, int Cp,
                     void* out, hipStream_t stream);
/* d/dlogit of scale*sigmoid(logit): disp head, reference model/layers/decoder.py:246 */
int um_sigmoid_scale_bwd(int dtype, long M, int C, const float* d, int ldd, const float* dd,
                         int lddd, float scale, void* dlogit, int ldo, hipStream_t stream);
/* split-bf16 head (um_pack_weight_split): forward finish d[m][k] = scale *
 * sigmoid(z[m][k] + z[m][K + k] + bias[k]) over the 2K-column f32 GEMM
 * output z, and the backward's dlogit written to channels k AND K + k (so the
 * data-gradient GEMM over the 2K split rows sums both halves of the weight);
 * channels [2K, ldo) zeroed. */
int um_head_split_fin(long M, int K, const float* z, int ldz, const float* bias, float scale,
                      float* d, int ldd, hipStream_t stream);
int um_sigmoid_scale_bwd_split(int dtype, long M, int C, const float* d, int ldd, const float* dd,
                               int lddd, float scale, void* dlogit, int ldo, hipStream_t stream);
/* One-pass bf16 disparity heads (csrc/disphead.hip), reference
 * model/layers/decoder.py:244-247 (ConvLayer: ReflectionPad2d(1) + Conv2d 3x3,
 * 4 outputs) + :246 (scale * sigmoid).  x NHWC bf16 [N][H][W][ldx] with C in
 * {32, 64, 128, 256} channels, W % 16 == 0 (um_disp_head_ok); wf / wT the
 * split-bf16 weights of um_pack_weight_split with K = 4 ([8][3][3][C] and
 * [C][3][3][8]).
 * fwd  : d[m][k] = scale * sigmoid(sum (w_hi + w_lo) x + bias[k]), d f32 [M][ldd]
 * dgrad: dx (+)= the reflect-pad conv adjoint of dlogit [M][ldl] bf16 (the 8
 *        channels of um_sigmoid_scale_bwd_split), dx bf16 [M][ldx] */
int um_disp_head_ok(int N, int H, int W, int C, int ldx);
int um_disp_head_fwd(int N, int H, int W, int C, const void* x, int ldx, const void* wf,
                     const float* bias, float scale, float* d, int ldd, hipStream_t stream);
int um_disp_head_dgrad(int N, int H, int W, int C, const void* dl, int ldl, const void* wT,
                       void* dx, int ldx, int accumulate, hipStream_t stream);

/* ----------------------------------------------------------- attention ---
 * EfficientAttention core, reference model/layers/attention.py:42-76.
 * qkv [N*S][ld]: K cols [0,C), Q [C,2C), V [2C,3C).
 */
long um_attn_ws_kstats(int N, int S, int C);
long um_attn_ws_ctx(int N, int S, int C, int heads);
long um_attn_ws_tiles(int N, int S, int C, int heads);
int um_attn_fwd(int dtype, int N, int S, int C, int heads, const void* qkv, int ld,
                float* kmax, float* ksum, float* ctx, float* ws, void* att, int ldo,
                hipStream_t stream);
int um_attn_bwd(int dtype, int N, int S, int C, int heads, const void* qkv, int ld,
                const float* kmax, const float* ksum, const float* ctx, const void* datt,
                int ldd, void* dqkv, int ldq, float* dks_ws, float* ws, float* dctx,
                float* r, hipStream_t stream);

/* ------------------------------------------------------------- decoder ---
 * Decoder-stage concat/upsample/pixel-shuffle/SE, reference
 * model/layers/decoder.py:90-136,210-249.
 */
enum { UM_CAT_COPY = 0, UM_CAT_UP2 = 1, UM_CAT_PSHUF = 2 };
typedef struct {
  const void* ptr;     /* source (NHWC, pixel stride ld) */
  const float* scale;  /* optional per-(n,c) gate [N][C] */
  int C, ld, op, coff, dtype, h, w; /* channels, stride, op, dst channel offset, dtype, src size */
} um_cat_src;
int um_concat_build(int dtype, int N, int H, int W, void* dst, int ld, int Ctot, int nsrc,
                    const um_cat_src* srcs, hipStream_t stream);
/* dscale (+=) needs ws: um_concat_bwd_ws(N, src.h, src.w, src.C) floats.
 * accumulate: bit 0 = dsrc (+=), bit 1 = dscale written (=) instead of (+=) */
long um_concat_bwd_ws(int N, int h, int w, int C);
int um_concat_bwd_src(int dtype, int N, int H, int W, const void* g, int ldg,
                      const um_cat_src* src, void* dsrc, int ldd, int dsrc_dtype,
                      int accumulate, float* dscale, float* ws, hipStream_t stream);
int um_channel_mean(int dtype, int N, long S, int C, const void* x, int ld, float* out,
                    hipStream_t stream);
/* pooled[n][c] = inv_hw * sum of the image's parts_per_image pool rows (written
 * for the backward), then z1 = relu(W1 pooled), s = sigmoid(W2 z1) */
int um_se_mlp_fwd(int N, int C, int R, const float* pool_parts, int parts_per_image,
                  float inv_hw, float* pooled, const float* w1, const float* w2, float* z1,
                  float* s, hipStream_t stream);
/* dw1/dw2 written (=); dz: f32 [N][R] scratch */
int um_se_mlp_bwd(int N, int C, int R, const float* ds, const float* s, const float* z1,
                  const float* pooled, const float* w1, const float* w2, float* dw1,
                  float* dw2, float* dpool_scaled, float* dz, float inv_S, hipStream_t stream);

/* ---------------------------------------------------------------- loss ---
 * Loss stack: scale_pyramid (reference train/utils.py:27-50), reconstruct
 * (train/utils.py:65-109), TukraUncertaintyLoss forward/backward
 * (train/loss.py:15-264,340-434,512-568).  Images NCHW f32 [N][6][H][W];
 * predictions NHWC f32 [N][H][W][pld] (d_L, d_R, sigma_L, sigma_R).
 * loss_type: 0 l1, 1 bayesian, 2 log_bayesian (train/loss.py:364-375).
 */
/* image pyramid, every level in ONE launch: out[l] = [NC][H>>l][W>>l], level 0
 * an exact copy (F.interpolate(bilinear, align_corners=True), utils.py:27-50) */
int um_pyramid(const float* x, int NC, int H, int W, int nlevels, float* const* out,
               hipStream_t stream);
/* reconstruct (utils.py:65-97): out = grid_sample(img, linspace grid + sign*disp) */
int um_warp(const float* img, int N, int C, int H, int W, const float* disp, long disp_sn,
            long disp_sp, float sign, float* out, hipStream_t stream);
/* its adjoint w.r.t. the disparity (the image is data): gdisp = sum_c gout_c d(warp_c)/d(disp) */
int um_warp_bwd(const float* img, int N, int C, int H, int W, const float* disp, long disp_sn,
                long disp_sp, float sign, const float* gout, float* gdisp, long g_sn, long g_sp,
                hipStream_t stream);
/* reconstruct_pyramid (utils.py:112-135), every level and both views in ONE
 * launch: out[l] = [N][6][H>>l][W>>l]; pred[l] strided [N][4][h][w] with
 * pred_strides[3l..3l+2] = (image, channel, pixel) strides in elements */
int um_recon_pyramid(int nlevels, int N, int H, int W, const float* const* img,
                     const float* const* pred, const long* pred_strides, float* const* out,
                     hipStream_t stream);
/* TukraUncertaintyLoss.forward (loss.py:512-568) over every scale in ONE launch:
 * img[s] = pyramid level s [N][6][H>>s][W>>s], pred[s] NHWC [N][H>>s][W>>s][4].
 * The recon is re-derived in the kernel (warp of the opposite view).
 * ws: um_loss_ws() bytes of f64 scratch; out[6] = disp_loss, error_loss,
 * wssim, consistency, smoothness, error term (disp_loss / error_loss,
 * optional: out[0] / out[1] again, as the two 0-d loss tensors the reference
 * returns); emap_last (optional) = the last
 * scale's error map [N][2][h][w] (WeightedSSIMLoss.previous_image_error);
 * recon_out (optional, per scale) receives the reconstruction [N][6][h][w]
 * the kernel derives (reconstruct_pyramid's result, as a side output).
 * gpart (optional, per scale NHWC [N][h][w][4] f32): the forward of a step
 * that will differentiate the loss.  The launch then also computes the
 * gradient per unit gout (channels 0/1: d disp_loss / d d_v without the
 * consistency scatter, 2/3: d error_loss / d sigma_v), one tile pass for
 * both, and um_loss_bwd completes it from gpart. */
long um_loss_ws(int nscales, int N, int H, int W);
int um_loss_fwd(int nscales, int N, int H, int W, const float* const* img,
                const float* const* pred, float alpha, int loss_type, float esw, float ecw,
                float w_wssim, float w_cons, float w_smooth, float w_err, double* ws,
                float* emap_last, float* const* recon_out, float* out, float* disp_loss,
                float* error_loss, float* const* gpart, hipStream_t stream);
/* its backward (the reference's autograd through loss.py:512-568):
 * dpred[s] NHWC [N][h][w][4] = d(gout_disp*disp_loss + gout_err*error_loss)/d pred[s]
 * (gout_disp / gout_err: device scalars, NULL = 0).  gpart NULL: two launches (the consistency scatter,
 * then every other term); gpart = um_loss_fwd's partials of the same inputs:
 * ONE launch (the scatter, which scales and completes them). */
int um_loss_bwd(int nscales, int N, int H, int W, const float* const* img,
                const float* const* pred, float alpha, int loss_type, float esw, float ecw,
                float w_wssim, float w_cons, float w_smooth, float w_err,
                const float* gout_disp, const float* gout_err, const float* const* gpart,
                float* const* dpred, hipStream_t stream);
/* The same loss with ReprojectionErrorLoss(pooling=True) (loss.py:405-434): at
 * every scale the prediction, the image and the detached error map go through
 * AvgPool2d(3, stride 1) ([h,w] -> [h-2,w-2]) before the error term (NLL,
 * esw * smoothness, ecw * consistency) is evaluated; the last scale must be
 * at least 4x4.  Arguments as um_loss_fwd / um_loss_bwd, except:
 * emaps[s] [N][2][H>>s][W>>s] receives the unpooled error map of EVERY scale
 * (emaps[nscales-1] is previous_image_error); pool_ws: um_loss_pool_ws() bytes,
 * 16-byte aligned, caller-owned (no allocation, no host synchronisation).
 * out[1] / out[5] / error_loss hold the pooled term; out[0], out[2..4] and
 * disp_loss are what um_loss_fwd gives.  With gpart the forward also leaves
 * the gradient w.r.t. the pooled maps in pool_ws: um_loss_pool_bwd with the
 * same gpart and pool_ws is then two launches (the consistency scatter and
 * the pool adjoint).  Without gpart the backward needs the forward's emaps
 * and runs every stage itself; pool_ws is scratch.  The scatter into the
 * sampled pooled disparity uses fixed-point integer atomics: the gradient
 * does not depend on their order. */
long um_loss_pool_ws(int nscales, int N, int H, int W);
int um_loss_pool_fwd(int nscales, int N, int H, int W, const float* const* img,
                     const float* const* pred, float alpha, int loss_type, float esw, float ecw,
                     float w_wssim, float w_cons, float w_smooth, float w_err, double* ws,
                     float* const* emaps, float* const* recon_out, float* out, float* disp_loss,
                     float* error_loss, float* const* gpart, void* pool_ws, hipStream_t stream);
int um_loss_pool_bwd(int nscales, int N, int H, int W, const float* const* img,
                     const float* const* pred, float alpha, int loss_type, float esw, float ecw,
                     float w_wssim, float w_cons, float w_smooth, float w_err,
                     const float* gout_disp, const float* gout_err, const float* const* gpart,
                     const float* const* emaps, void* pool_ws, float* const* dpred,
                     hipStream_t stream);
/* WeightedSSIMLoss.image_error (loss.py:96-131) of an explicit recon: out [N][2][H][W] */
int um_image_error(const float* img, const float* rec, int N, int H, int W, float alpha,
                   float* out, hipStream_t stream);

/* -------------------------------------------------------- loss terms ---
 * The sub-losses of train/loss.py as standalone, differentiable entries
 * (csrc/lossterms.hip): what a composition other than the fused
 * TukraUncertaintyLoss above is built from.  Strided [N][C][h][w] operands
 * are given as pointer + image stride (sn) + channel stride (sc) + pixel
 * stride (sp): element (n, c, y, x) at p[n*sn + c*sc + (y*w + x)*sp], so
 * channel slices of an NHWC prediction are passed without a copy.  A scalar
 * is accumulated as one f64 partial per workgroup in ws (um_lossterm_ws(N, H,
 * W) bytes, any term of that geometry) and finished on the device into a f32
 * device scalar; an upstream scalar gradient g is a device pointer.  No entry
 * allocates or synchronises.  Launches: forward = term + finish, backward =
 * one adjoint launch (+ the scatter where an image is sampled).
 */
long um_lossterm_ws(int N, int H, int W);
/* WeightedSSIMLoss.image_error (loss.py:96-131, ssim/dssim :43-90) with
 * c1 = k1^2, c2 = k2^2 at run time: out [N][2][H][W], one launch; with ws and
 * mean_out (both or neither) the same launch leaves the block partials of
 * mean(e_L + e_R) (WeightedSSIMLoss.forward, loss.py:133-151) and a finish
 * launch writes mean_out.  H, W >= 3 */
int um_image_error_k(const float* img, const float* rec, int N, int H, int W, float alpha,
                     float c1, float c2, float* out, double* ws, float* mean_out,
                     hipStream_t stream);
/* its adjoint w.r.t. rec (wrt 0) or img (wrt 1), grad [N][6][H][W], one launch.
 * Upstream gradient of the map: g [N][2][H][W] (or NULL) plus g_mean[0] / (N*H*W)
 * (or NULL: the mean's path).  L1 part: (1-alpha)/3 sign(X-Y) g, sign(0) = 0;
 * SSIM part: alpha/3 times the sum over the <= 9 SSIM-grid cells whose window
 * covers the pixel of G(cell) d(dssim_c(cell))/dX(pixel), G the adjoint of the
 * align_corners resize (H-2)x(W-2) -> HxW applied to the upstream gradient;
 * the clamp passes gradient where 0 <= (1-ssim)/2 <= 1 */
int um_image_error_bwd(const float* img, const float* rec, int N, int H, int W, float alpha,
                       float c1, float c2, int wrt, const float* g, const float* g_mean,
                       float* grad, hipStream_t stream);
/* adjoint of um_warp w.r.t. the sampled image (F.grid_sample's image gradient,
 * utils.py:65-97): gimg[n][c] = sum over source pixels of gout[n][c][y][x] *
 * w_tap at the four bilinear taps; taps outside the image receive nothing.
 * One workgroup owns one target row of one image: the source rows t-1, t, t+1
 * (the only ones whose row taps reach t; the row taps do not depend on the
 * shift) scatter along x into f32 row accumulators in LDS, in that order, and
 * every output element is stored exactly once: nothing is pre-zeroed and no
 * global atomic is used.  The last bits depend on the arrival order of the LDS
 * adds within a row (as grid_sample's own backward).  The C*W accumulators
 * must fit 64 KiB of LDS: C*W <= um_warp_bwd_img_max_cw() = 16384 (W <= 5461
 * at C = 3); a larger C*W is UM_ERR_ARG naming the limit, and nothing is
 * launched */
int um_warp_bwd_img_max_cw(void);
int um_warp_bwd_img(const float* gout, int N, int C, int H, int W, const float* disp,
                    long disp_sn, long disp_sp, float sign, float* gimg, hipStream_t stream);
/* ConsistencyLoss.forward(disp, images) (loss.py:167-188): out[0] =
 * mean|d_L - warp(i_R, -d_L)| + mean|d_R - warp(i_L, +d_R)|; disp and images
 * strided [N][2][H][W] and may alias (images=None: the F5 quirk, disp is both
 * the compared map and the sampled one).  H, W >= 2 */
int um_consistency_fwd(const float* disp, long d_sn, long d_sc, long d_sp, const float* images,
                       long i_sn, long i_sc, long i_sp, int N, int H, int W, double* ws,
                       float* out, hipStream_t stream);
/* gdisp [N][2][H][W] (or NULL) = the direct sign term + the shift term
 * (d(warp)/d(shift) * sign * W); gimages [N][2][H][W] (or NULL) = the scatter
 * of -sign(r) g/(NHW) through the taps (the um_warp_bwd_img rows, W <= 16384),
 * staged in scratch [N][2][H][W].  alias != 0 (images is disp): gimages
 * receives the sum of both, gdisp the direct part only */
int um_consistency_bwd(const float* disp, long d_sn, long d_sc, long d_sp, const float* images,
                       long i_sn, long i_sc, long i_sp, int N, int H, int W, const float* g,
                       float* gdisp, float* gimages, float* scratch, int alias,
                       hipStream_t stream);
/* SmoothnessLoss.forward(disp, images) (loss.py:208-264): replicate-padded
 * forward differences of disp (strided [N][2][H][W]) weighted by
 * exp(-mean_c |grad I|), images [N][6][H][W]; out[0] = mean(e_L + e_R).  The
 * gradient is w.r.t. disp only ([N][2][H][W]).  H, W >= 2 */
int um_smoothness_fwd(const float* disp, long d_sn, long d_sc, long d_sp, const float* images,
                      int N, int H, int W, double* ws, float* out, hipStream_t stream);
int um_smoothness_bwd(const float* disp, long d_sn, long d_sc, long d_sp, const float* images,
                      int N, int H, int W, const float* g, float* gdisp, hipStream_t stream);
/* ReprojectionErrorLoss.l1 / .bayesian / .log_bayesian (loss.py:389-403) of
 * (uncertainty, error), both strided [N][2][H][W]; loss_type as above.  The
 * gradient is w.r.t. the uncertainty ([N][2][H][W]); the error is detached by
 * definition (loss.py:418) */
int um_nll_fwd(const float* unc, long u_sn, long u_sc, long u_sp, const float* err, long e_sn,
               long e_sc, long e_sp, int N, int H, int W, int loss_type, double* ws, float* out,
               hipStream_t stream);
int um_nll_bwd(const float* unc, long u_sn, long u_sc, long u_sp, const float* err, long e_sn,
               long e_sc, long e_sp, int N, int H, int W, int loss_type, const float* g,
               float* gunc, hipStream_t stream);

/* ------------------------------------------------------- adversarial ---
 * RandomDiscriminator pieces around its EncoderStages (reference
 * model/discriminator.py:53-86, train/loss.py:267-337).
 */
/* adjoint of um_image_to_nhwc: NHWC [N][H][W][ld] (dtype) -> NCHW f32 [N][C][H][W] */
int um_nhwc_to_image(int dtype, const void* x, int N, int C, int H, int W, int ld, float* out,
                     hipStream_t stream);
/* prob[n] = sigmoid(b + sum w[c*HW + p] x[n][p][c]): Linear over the NCHW flatten + sigmoid */
int um_disc_head_fwd(int dtype, const void* x, int N, int HW, int C, const float* w,
                     const float* bias, float* prob, hipStream_t stream);
int um_disc_head_bwd(int dtype, const void* x, int N, int HW, int C, const float* w,
                     const float* prob, const float* dprob, void* dx, float* dw, float* db,
                     hipStream_t stream);
/* out[0] = mean |a - b| over n elements (ws: um_l1_mean_ws() bytes) and its backward */
long um_l1_mean_ws(void);
int um_l1_mean(int dtype, const void* a, const void* b, long n, double* ws, float* out,
               hipStream_t stream);
int um_l1_mean_bwd(int dtype, const void* a, const void* b, long n, const float* g, void* da,
                   void* db, hipStream_t stream);
/* nn.MSELoss / nn.BCELoss (reduction 'mean') of N probabilities p against
 * step labels y[n] = 1 for n < n_real, else 0, which are never materialised:
 * replaces ones_like + the ATen loss in GeneratorLoss (reference
 * train/loss.py:331-337, n_real = N) and zeros_like + the slice fill + the
 * ATen loss in run_discriminator (train/utils.py:266-273, n_real =
 * batch_size).  MSE: mean (p-y)^2; BCE: -mean(y max(log p, -100) + (1-y)
 * max(log1p(-p), -100)), finite at a saturated p of exactly 0 or 1.  One
 * workgroup, f64 accumulation.  bwd: dp = g 2(p-y)/N resp.
 * g (p-y) / max(p(1-p), 1e-12) / N with g a device scalar (capturable). */
#define UM_LABEL_MSE 0
#define UM_LABEL_BCE 1
int um_label_loss_fwd(int kind, const float* p, int N, int n_real, float* out,
                      hipStream_t stream);
int um_label_loss_bwd(int kind, const float* p, int N, int n_real, const float* g, float* dp,
                      hipStream_t stream);
/* two NCHW f32 images [N][C][H][W] -> one NHWC batch [2N][H][W][Cp] (dtype):
 * rows 0..N-1 from a, N..2N-1 from b; padding and rounding of
 * um_image_to_nhwc.  Replaces detach().clone() + torch.cat + the layout
 * conversion per pyramid level in run_discriminator (reference
 * train/utils.py:262-264).  No gradient. */
int um_image_pair_to_nhwc(int dtype, const float* a, const float* b, int N, int C, int H, int W,
                          int Cp, void* out, hipStream_t stream);

/* ---------------------------------------------------------- evaluation ---
 * evaluate_model / sparsification (reference train/evaluate.py:66-196,
 * train/sparsification.py:8-61).  Off the training hot path.
 */
/* torchmetrics structural_similarity_index_measure (gaussian window, sigma ->
 * 11 taps, k1 0.01, k2 0.03) per image: out[n] = mean SSIM over the C x
 * (H-10) x (W-10) full windows; ws: um_ssim_ws() bytes */
long um_ssim_ws(int N, int H, int W);
int um_ssim_gauss(const float* x, const float* y, int N, int C, int H, int W, float data_range,
                  float sigma, double* ws, float* out, hipStream_t stream);
/* nn.AvgPool2d(k, stride=1): out [NC][H-k+1][W-k+1] */
int um_avgpool_valid(const float* x, int NC, int H, int W, int k, float* out, hipStream_t stream);
/* argsort(keys, descending) + gather(vals) per segment of L (nseg segments) */
long um_spars_sort_ws(int nseg, int L);
int um_spars_sort(const float* keys, const float* vals, int nseg, int L, float* keys_out,
                  float* vals_out, void* ws, long ws_bytes, hipStream_t stream);
/* curve[k] = mean_seg( mean(sorted[int(k/steps*L):]) / mean(sorted) ); ws: nseg*steps f64 */
int um_spars_curve(const float* sorted_vals, int nseg, int L, int steps, double* ws,
                   float* curve, hipStream_t stream);

/* The fused per-batch form of the above for the captured evaluation engine
 * (umamd/evalengine.py).  acc is the engine's f64 accumulator block
 * {left SSIM sum, right SSIM sum, AUSE sum, AURG sum, batch count}
 * (the running_* sums of reference train/evaluate.py:160-176). */
/* Both views of one batch in one launch + a finish launch, replacing
 * reconstruct_left/right_image, the two SSIM calls and image_error of
 * evaluate.py:137-151.  left/right [N][3][H][W]; pred NHWC f32, element
 * (n, y, x, ch) at pred[n*pred_sn + (y*W + x)*pred_sp + ch], channels 0/1 the
 * disparities (the strides of um_warp).  recon [N][6][H][W] or NULL (not
 * written); err [N][2][H][W] = WeightedSSIMLoss(alpha=1).image_error;
 * acc[0] / acc[1] += the view's gaussian SSIM (11 taps, sigma 1.5, data range
 * 1) summed over the batch (reduction='sum').  H, W >= 12; ws: um_eval_ws()
 * bytes */
long um_eval_ws(int N, int H, int W);
int um_eval_maps(const float* left, const float* right, const float* pred, long pred_sn,
                 long pred_sp, int N, int H, int W, float* recon, float* err, double* ws,
                 double* acc, hipStream_t stream);
/* nn.AvgPool2d(11, stride=1) (sparsification.py:14-16) of err [N][2][H][W],
 * of channels 2/3 of pred (strides as above) and of rnd [N][2][H][W], each
 * written as sort-ready segments [2N][(H-10)*(W-10)].  Only k = 11. */
int um_eval_pool(const float* err, const float* pred, long pred_sn, long pred_sp,
                 const float* rnd, int N, int H, int W, int k, float* err_out, float* unc_out,
                 float* rnd_out, hipStream_t stream);
/* acc[2] += ause = sum(pred - oracle)/steps, acc[3] += aurg = sum(random -
 * pred)/steps (sparsification.py:43-61), acc[4] += 1 */
int um_eval_accum(const float* oracle_curve, const float* pred_curve, const float* random_curve,
                  int steps, double* acc, hipStream_t stream);

/* ---------------------------------------------------------------- adam ---
 * torch.optim.Adam step, reference train/train.py:228-229.
 */
int um_adam_chunk(void);
/* graph-replayable: *dstep += 1 on the device, bias corrections from it; lr from *dlr if non-null */
int um_adam_step_dev(const void* table, const void* chunks, int nchunks, float lr,
                     const float* dlr, float beta1, float beta2, float eps, float weight_decay,
                     int* dstep, hipStream_t stream);

/* --------------------------------------------------- input pipeline ---
 * The reference's training transforms (train/transforms.py:15-129 composed
 * in main.py:78-89 / parallel_main.py:111-124: ResizeImage((256, 512)) ->
 * RandomFlip(0.5) -> ToTensor() -> RandomAugment(0.5, ...)) for a batch of
 * both views.  left/right: uint8 [N][Hs][Ws][3] (decoded RGB); the resize is
 * Pillow's 8-bit bilinear resampler (host-made coefficient tables:
 * bounds [out][2] = (first tap, taps), kk [out][ks] 22-bit fixed point),
 * horizontal pass into `tmp` (um_stereo_prep_ws bytes), then the vertical
 * pass, /255, the flip and the augment with per-sample params [N][8] =
 * (flip, augment, gamma, brightness, colour[3], 0) drawn on the host in the
 * reference's order.  out_left/out_right: f32 [N][3][Hd][Wd].
 */
long um_stereo_prep_ws(int N, int Hs, int Wd);
int um_stereo_prep(int N, int Hs, int Ws, const unsigned char* left,
                   const unsigned char* right, int Hd, int Wd, const int* bounds_h,
                   const int* kk_h, int ks_h, const int* bounds_v, const int* kk_v, int ks_v,
                   const float* params, unsigned char* tmp, float* out_left, float* out_right,
                   hipStream_t stream);

/* ---------------------------------------------------------- deployment ---
 * A camera frame to metric depth around the inference engine
 * (umamd/deploy.py DepthPipeline: um_frame_prep -> forward -> um_depth_post
 * as one captured graph).
 */
/* ResizeImage -> ToTensor (reference train/transforms.py:15-41) of one view
 * in ONE launch: src uint8 [N][Hs][Ws][3] -> out f32 [N][3][Hd][Wd], written
 * into the caller's buffer.  Tables and integer arithmetic of um_stereo_prep
 * (22-bit fixed point, round half up, clip to [0, 255] after each pass, then
 * / 255.0f): bit-identical to PIL and to um_stereo_prep without flip or
 * augment.  A workgroup owns 8 output rows x 32 output columns, runs the
 * horizontal pass for the source rows its vertical taps need into LDS (u8)
 * and the vertical pass out of LDS: no workspace, no 8-bit intermediate in
 * memory.
 * The limit (um_frame_prep_ok answers 0, um_frame_prep returns UM_ERR_ARG):
 * ceil(7 * Hs / Hd) + 1 + ks_v source rows of a tile must fit 64 KiB of LDS
 * at 128 bytes per row, i.e. be <= 512 (every upscale; a vertical downscale
 * up to 56x), and ks_h <= 257 (a horizontal downscale up to 128x).  N <= 65535. */
int um_frame_prep_ok(int Hs, int Ws, int Hd, int Wd, int ks_h, int ks_v);
int um_frame_prep(int N, int Hs, int Ws, const unsigned char* src, int Hd, int Wd,
                  const int* bounds_h, const int* kk_h, int ks_h, const int* bounds_v,
                  const int* kk_v, int ks_v, float* out, hipStream_t stream);
/* Everything after the forward, for the LEFT view at the frame's size
 * (Hs, Ws), in one launch.  pred NHWC f32 with the strides of um_eval_maps
 * (pred_sp >= 4), channels d_L, d_R, sigma_L, sigma_R at model size (H, W).
 *   e           = |d_L - reconstruct_left_image(d_L, d_R)|: the left half of
 *                 ConsistencyLoss (reference train/loss.py:179-185) with the
 *                 warp of train/utils.py:65-103 (linspace(0, 1) grid,
 *                 grid_sample bilinear / zeros / align_corners=False)
 *   up(t)       = bilinear, align_corners=True, to (Hs, Ws) (the reference's
 *                 map resize, loss.py:120-121, evaluate.py:152-153)
 *   disparity   = up(d_L) * Ws      [source pixels]
 *   lr_error    = up(e) * Ws        [source pixels]
 *   uncertainty = up(sigma_L)
 *   depth       = fb / disparity where disparity > min_disp_px, else 0
 *   valid       = disparity > min_disp_px && uncertainty <= max_unc &&
 *                 lr_error <= max_lr_px   (u8 0 / 1)
 * The reference's only post-processing helper, train.utils.combine_disparity
 * (utils.py:202-245), goes through numpy on the host and is not called; this
 * is the device form of what follows its forward.  params: DEVICE f32[4] = (fb,
 * min_disp_px, max_unc, max_lr_px), read by the kernel, so a captured graph
 * sees new values at its next replay.  Outputs [N][Hs][Ws]; any of them may
 * be NULL (skipped).  H, W, Hs, Ws >= 2; H, W <= 32768. */
int um_depth_post(const float* pred, long pred_sn, long pred_sp, int N, int H, int W, int Hs,
                  int Ws, const float* params, float* disparity, float* depth,
                  float* uncertainty, float* lr_error, unsigned char* valid,
                  hipStream_t stream);
/* The display image (umamd/render.py, DepthPipeline(render=...)): a float map
 * coloured through a 256-entry table and blended over the camera frame.
 * Everything is per pixel over flat maps, count = N * Hs * Ws.
 *
 * um_depth_render: value f32 [count]; valid u8 [count] or NULL (all valid);
 * frame u8 [count][3] RGB or NULL (black); lut u8 [256][3]; rparams DEVICE
 * f32[4] = (lo, hi, opacity, invalid_opacity), read by the kernel, so a
 * captured graph sees new values at its next replay; range DEVICE f32[2] or
 * NULL, if given it replaces (lo, hi) (the output of um_value_range); rgb u8
 * [count][3].  Every float step a separate f32 operation, IEEE division:
 *   t   = (v - lo) / (hi - lo);  if inverse: t = 1 - t
 *   s   = t * 256
 *   c   = isnan(s) ? (0,0,0) : lut[s < 0 ? 0 : (int)min(s, 255)]   (truncates)
 *   a   = q(valid[i] != 0 ? opacity : invalid_opacity),
 *         q(x) = (int)(clamp(x, 0, 1) * 256 + 0.5), q(NaN) = 0
 *   rgb = (c * a + frame[i] * (256 - a) + 128) >> 8       per channel, integer
 * With lut = floor(cmap(arange(256))[:, :3] * 255 + 0.5) this is matplotlib's
 * Colormap.__call__ on an f32 array (reference train/utils.py:177-199
 * to_heatmap: below the range entry 0, s >= 256 entry 255, NaN black) followed
 * by the x * 255 + 0.5 rounding of save_image; a = 256 returns c, a = 0 the
 * frame.  One thread per 4 pixels (16-byte value load, dword mask, three
 * dwords of frame and rgb; a scalar form for the tail and for bases that are
 * not aligned: value 16, valid / frame / rgb 4), the table in LDS.
 *
 * um_value_range: range[0] = min, range[1] = max of value[i] over the pixels
 * with valid[i] != 0 (NULL: every pixel) that are not NaN; +-inf take part;
 * no such pixel: (+inf, -inf), which renders black.  Two launches (at most 256
 * workgroup partials in ws, then one workgroup), no atomics and no state
 * between calls: deterministic, safe to replay.  ws: um_value_range_ws(count)
 * bytes (host query), 4-byte aligned.
 * Measured inside DepthPipeline's graph (tools/bench_depth_render.py, MI355X,
 * 1024x1280, B=1, medians of 3 alternated repeats): um_depth_render adds
 * 0.0024 ms to the 1.1906 ms frame, um_value_range + um_depth_render 0.0172 ms;
 * the same picture from torch device ops adds 0.247 ms, the host path
 * (copy back, matplotlib, numpy) 27.6 ms.
 * count <= 0 or a null value / lut / rparams / rgb / range / ws: UM_ERR_ARG. */
long um_value_range_ws(long count);
int um_value_range(const float* value, const unsigned char* valid, long count, float* range,
                   void* ws, hipStream_t stream);
int um_depth_render(const float* value, const unsigned char* valid, const unsigned char* frame,
                    long count, const unsigned char* lut, const float* rparams,
                    const float* range, int inverse, unsigned char* rgb, hipStream_t stream);
/* 3-D points (umamd/points.py, DepthPipeline(points=...)): the depth map
 * back-projected through pinhole intrinsics.  intr: DEVICE f32[4] = (fx, fy,
 * cx, cy) in source pixels, read by the kernels, so a captured graph sees new
 * values at its next replay.  For pixel (image n, row v, column u), every step
 * a separate f32 operation, IEEE division:
 *   Z = depth[n][v][u]
 *   X = (((float)u - cx) * Z) / fx
 *   Y = (((float)v - cy) * Z) / fy
 * u and v are the integer indices: the pixel centre sits AT the integer
 * coordinate, no half-pixel shift (a caller whose calibration puts the centre
 * of pixel 0 at 0.5 passes cx - 0.5 and cy - 0.5).  A pixel is kept when
 * valid[n][v][u] != 0 (any non-zero byte); valid NULL: every pixel is kept.
 *
 * um_depth_backproject: depth f32 [N][Hs][Ws], valid u8 [N][Hs][Ws] or NULL
 * -> the organised map xyz f32 [N][Hs][Ws][3]: (X, Y, Z) at a kept pixel,
 * (0, 0, 0) elsewhere whatever depth holds there (NaN, inf).  One launch, one
 * thread per 4 pixels (a 16-byte depth load, a dword of valid, three 16-byte
 * stores; a scalar form for the tail and for bases that are not aligned:
 * depth / xyz 16, valid 4).
 *
 * um_depth_cloud: the packed cloud over the lattice v % stride == 0 &&
 * u % stride == 0, Hl = ceil(Hs / stride) x Wl = ceil(Ws / stride) sites per
 * image.  The kept sites in order, image-major then row-major, are the rows of
 *   xyzu   f32 [N * Hl * Wl][4]: (X, Y, Z, uncertainty at the site; 0 with
 *          uncertainty NULL), one 16-byte store per row (16-byte aligned)
 *   rgba   u8 [N * Hl * Wl][4]: the frame's (r, g, b) at the site and 255, one
 *          4-byte store per row (4-byte aligned); skipped if frame (u8
 *          [N][Hs][Ws][3]) or rgba is NULL
 *   offsets  int [N + 1]: image n owns rows offsets[n] .. offsets[n + 1];
 *          offsets[0] = 0, offsets[N] the number of points
 * Rows at and past offsets[N] are not written: their content is unspecified
 * for the caller (whatever the buffer held).  uncertainty f32 [N][Hs][Ws] or
 * NULL.  Three launches, no atomics and no state between calls, so the order
 * is fixed, the result deterministic and the call safe to capture and replay:
 * (1) the kept sites of every tile -- 1024 consecutive lattice sites of one
 * image; a tile never spans two images -- into ws; (2) one workgroup of 256
 * threads turns the counts into their exclusive prefix sums, 256 tiles per
 * turn of a loop, and writes offsets; (3) every workgroup packs its tile from
 * that base: 4 sites per thread, thread counts scanned over the 64 lanes
 * (__shfl_up), wave totals through LDS, so a tile's rows are one contiguous
 * run.  stride 1 reads 4 consecutive pixels per thread with vector loads where
 * the addresses allow, stride > 1 gathers.  ws: um_depth_cloud_ws(N, Hs, Ws,
 * stride) bytes (host query: 4 per tile, N * ceil(Hl * Wl / 1024) tiles; 0 for
 * sizes the call refuses), 4-byte aligned.
 * Measured inside DepthPipeline's graph (tools/bench_depth_points.py, MI355X,
 * 1024x1280, B=1, 39 % of the pixels kept, medians of 3 alternated repeats):
 * um_depth_backproject adds 0.0143 ms to the 1.1858 ms frame, um_depth_cloud
 * 0.0186 ms (0.0165 ms at stride 2), both 0.0261 ms; the same cloud from torch
 * device ops (nonzero, gathers) adds 0.2049 ms and synchronises with the host.
 * UM_ERR_ARG before any launch: a size or stride < 1; N * Hl * Wl or N * Hs
 * above INT_MAX; a null depth / intr / xyz, or ws / xyzu / offsets; a float
 * pointer that is not 4-byte aligned. */
int um_depth_backproject(const float* depth, const unsigned char* valid, int N, int Hs, int Ws,
                         const float* intr, float* xyz, hipStream_t stream);
long um_depth_cloud_ws(int N, int Hs, int Ws, int stride);
int um_depth_cloud(const float* depth, const unsigned char* valid, const float* uncertainty,
                   const unsigned char* frame, int N, int Hs, int Ws, int stride,
                   const float* intr, void* ws, float* xyzu, unsigned char* rgba, int* offsets,
                   hipStream_t stream);
/* Rectification (umamd/rectify.py, DepthPipeline(rectify=...)): stage 0 of the
 * deployment path.  The raw camera frame src u8 [N][Hs][Ws][3] is undistorted
 * and stereo-rectified into dst u8 [N][Hr][Wr][3], the pinhole image every
 * later stage assumes.  Same model as OpenCV's initUndistortRectifyMap + remap
 * (pinhole + Brown-Conrady, bilinear), own rounding: the result is defined to
 * the bit below, it is not bit-equal to cv2.remap.
 *
 * Map.  For output pixel (row v, column u) -- integer indices, the pixel
 * centre AT the integer coordinate as in the point stage -- the source
 * coordinate (mx, my) comes from cal, DEVICE f32[24] =
 *   (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, m0..m8, 0, 0, 0)
 * with (fx, fy, cx, cy) the raw camera's matrix, k* / p* its distortion
 * coefficients and m = inv(K_new * R), row-major, made on the host in f64 and
 * rounded to f32.  Every step one exactly rounded f32 operation, IEEE
 * division, no contraction, in exactly this order:
 *   X = (m0*u + m1*v) + m2;  Y = (m3*u + m4*v) + m5;  W = (m6*u + m7*v) + m8
 *   x = X / W;  y = Y / W;  x2 = x*x;  y2 = y*y;  xy = x*y;  r2 = x2 + y2
 *   num = 1 + r2*(k1 + r2*(k2 + r2*k3));  den = 1 + r2*(k4 + r2*(k5 + r2*k6))
 *   kr = num / den
 *   xd = (x*kr + (2*p1)*xy) + p2*(r2 + 2*x2)
 *   yd = (y*kr + p1*(r2 + 2*y2)) + (2*p2)*xy
 *   mx = fx*xd + cx;   my = fy*yd + cy
 * Fixed point: q(c) = (int)rintf(c * 32) if c is finite and |c| < 2^20, else
 * q(c) = OUT = INT32_MIN.  (qx, qy) = (q(mx), q(my)).
 * Table mode skips the formulas: (qx, qy) is read from map, DEVICE int32
 * [Hr][Wr][2] (other lens models, maps a user already has).  Exactly one of
 * cal and map is non-NULL; both are read by the kernel, so a captured graph
 * sees new values at its next replay.
 *
 * Sample.  Integer arithmetic, border value 0:
 *   ix = qx >> 5 (arithmetic shift), ax = qx & 31; iy, ay the same from qy
 *   p00 = src[iy][ix], p01 = src[iy][ix+1], p10 = src[iy+1][ix],
 *   p11 = src[iy+1][ix+1]; a tap outside [0,Hs) x [0,Ws) counts as 0 and is
 *   not read
 *   out = ((32-ax)*(32-ay)*p00 + ax*(32-ay)*p01 + (32-ax)*ay*p10 + ax*ay*p11
 *          + 512) >> 10                                        per channel
 *   a pixel with qx == OUT or qy == OUT is 0
 * Inside mask: inside[v][u] = 1 when neither coordinate is OUT and
 * 0 <= qx <= (Ws-1)*32 and 0 <= qy <= (Hs-1)*32, else 0; u8 [Hr][Wr], the same
 * for every image of the batch, written once per call; NULL: skipped.
 *
 * um_frame_rectify: one launch, one thread per 4 consecutive output pixels of
 * the flat [N*Hr*Wr] index (a group may straddle a row or an image, (v, u) is
 * found per pixel): three dword stores of dst and one of inside, a scalar form
 * for the tail and for bases that are not 4-byte aligned.  The 6 bytes of a
 * tap row are read as a dword and a half-word where all four taps are inside,
 * as bytes at the border; exactly the taps are read and src needs no
 * alignment.  No LDS, no atomics, no state between calls: safe to capture and
 * replay.
 * Limits: N >= 1; Hs, Ws, Hr, Wr >= 2; Hs, Ws <= 32767; N*Hr*Wr <= INT_MAX.
 * UM_ERR_ARG before any launch: a size outside the limits; both or neither of
 * cal / map; a null src / dst; a cal or map that is not 4-byte aligned.
 *
 * um_valid_and: valid[n][i] = valid[n][i] && inside[i], written as 0 / 1, for
 * valid u8 [N][HW] (any non-zero byte counts as set) and inside u8 [HW]: the
 * pipeline's mask restricted to the pixels whose source lies in the raw
 * frame.  One launch after um_depth_post, a dword form (four masks per
 * thread) and a scalar form.  N < 1, HW < 1 or a null pointer: UM_ERR_ARG.
 *
 * Measured inside DepthPipeline's graph (tools/bench_depth_rectify.py, MI355X,
 * 1024x1280 raw -> 1024x1280 rectified -> 256x512 bf16, B=1, medians of 3
 * alternated repeats): the stage (um_frame_rectify + um_valid_and) adds
 * 0.0129 ms to the 1.1898 ms frame in analytic mode and 0.0118 ms in table
 * mode; the same frame from torch device ops (grid_sample on the f32 map,
 * round) ahead of the plain pipeline adds 0.0666 ms (5.2x the stage), on the
 * host (scipy.ndimage.map_coordinates per channel) 60.3 ms (4700x).  Both
 * modes beat the torch composition in each of the 3 repeats.  The torch frame
 * differs from the stage's in 2 350 118 of 3 932 160 bytes of a uniform-noise
 * frame, by at most 7: its coordinates are not rounded to 1/32 pixel. */
int um_frame_rectify(const unsigned char* src, int N, int Hs, int Ws, int Hr, int Wr,
                     const float* cal, const int* map, unsigned char* dst,
                     unsigned char* inside, hipStream_t stream);
int um_valid_and(unsigned char* valid, const unsigned char* inside, int N, long HW,
                 hipStream_t stream);
/* Refinement (umamd/refine.py, DepthPipeline(refine=...)): a stage of our own
 * between um_depth_post and um_valid_and; the reference has none.  In both
 * kernels every float step below is one exactly rounded f32 operation, in the
 * order written, IEEE division, no contraction.  fp: DEVICE f32[8] = (eps, a,
 * floor, q, g2, 0, 0, 0); the kernels read it and the tables, so a captured
 * graph sees new values at its next replay.  "finite": neither NaN nor +-inf.
 *
 * um_disp_smooth: a dilated joint-bilateral filter weighted by confidence.
 * disp, unc f32 [N][Hs][Ws]; frame u8 [N][Hs][Ws][3], the guide; radius R and
 * dilation step: the taps sit at offsets (j*step, i*step) (rows, columns), j
 * and i in [-R, R]; S f32 [(R+1)*(R+1)] indexed [|j|][|i|], the spatial table;
 * G f32 [768], the colour table.  -> disp_out, unc_out f32 [N][Hs][Ws],
 * distinct from the inputs.  For output pixel p the taps t are visited in
 * row-major order (j outer, i inner, both ascending).  A tap takes part only
 * if it lies inside the image and disp[t] and unc[t] are both finite; every
 * other tap is skipped (no border is replicated, a skipped tap is not read):
 *   c_t = 1 / (unc[t]*unc[t] + eps)
 *   k   = |r_p - r_t| + |g_p - g_t| + |b_p - b_t|        (integer, 0..765)
 *   w   = (S[|j|][|i|] * G[k]) * c_t
 *   num = num + w*disp[t];   nus = nus + w*unc[t];   den = den + w
 * (num, nus, den start at 0).  If den > 0 and den is finite, disp_out[p] =
 * num/den and unc_out[p] = nus/den; otherwise disp[p] and unc[p] pass through
 * bit for bit.  The host makes S = exp(-(i*i + j*j) / (2 sigma_s^2)) (sigma_s
 * in taps) and G = exp(-k*k / (2 sigma_c^2)) (sigma_c in summed 8-bit levels)
 * in f64 and rounds them to f32; any other table is as valid.
 * One launch.  A workgroup of 256 threads owns a tile of 64 columns x 16 rows
 * (8 rows where R*step > 13) and stages the tile and its halo of R*step
 * pixels in LDS once, as four planes: disp, unc, c (computed once per staged
 * pixel) and the packed colour with the takes-part flag in byte 3; G lives in
 * LDS too.  A wave owns one tile row at a time, so its 64 lanes read 64
 * consecutive dwords of a plane for every tap, whatever the step: no bank
 * conflict but in the G lookup, whose index is data.  k is one v_sad_u8.  No
 * atomics, no state between calls.
 * Limits: 1 <= R <= 3, step >= 1, R*step <= 16, N, Hs, Ws >= 1, N*Hs*Ws <=
 * INT_MAX.  UM_ERR_ARG before any launch: a value outside them, a null
 * pointer, a float pointer that is not 4-byte aligned.
 *
 * um_disp_fuse: a per-pixel recursive filter over the frames of a stream plus
 * finalise.  disp_in, unc_in, lr_error f32 [count]; params: the DEVICE f32[4]
 * block of um_depth_post (fb, min_disp, max_unc, max_lr); state mean, var f32
 * [count], both given or both NULL, var < 0 marking an empty state (reset: a
 * fill of var with -1).  With state, for pixel i, d = disp_in[i], s =
 * unc_in[i]:
 *   t = a*s;  m = t*t + floor;  fresh = finite(d) && finite(m)
 *   p = var[i] + q;  e = d - mean[i];  pm = p + m
 *   keep = fresh && var[i] >= 0 && e*e <= g2*pm
 *   keep:          K = p/pm;  mean' = mean[i] + K*e;  var' = p - K*p
 *   !keep, fresh:  mean' = d;  var' = m                      (reset)
 *   !fresh:        mean' = mean[i];  var' = var[i]           (state untouched)
 *   D = var' >= 0 ? mean' : d;   U = s;   disp_var[i] = var'
 * and mean', var' are stored.  Without state D = d, U = s and disp_var is not
 * written.  Then, as um_depth_post: depth = D > min_disp ? fb / D : 0; valid =
 * D > min_disp && U <= max_unc && lr_error[i] <= max_lr (0 / 1).  Outputs
 * disparity (D), uncertainty (U), depth, valid (u8), disp_var: any may be
 * NULL.  The model's sigma is a photometric quantity: a (noise_scale) turns it
 * into a disparity noise and floor keeps the gain below 1.
 * One launch, one thread per 4 pixels with 16-byte accesses, a scalar form
 * for the tail and for bases that are not aligned (floats 16, valid 4).
 * Elementwise: an output may be its own input (disp_in == disparity).
 * UM_ERR_ARG before any launch: count < 1; a null disp_in / unc_in / params /
 * fp; valid without lr_error; one of mean and var alone; a float pointer that
 * is not 4-byte aligned.
 *
 * Measured inside DepthPipeline's graph (tools/bench_depth_refine.py, MI355X,
 * 1024x1280 -> 256x512 bf16, B=1, R=2, step=2, medians of 3 alternated
 * repeats, uniform-noise frames): 'spatial' (um_disp_smooth + um_disp_fuse
 * without state) adds 0.0392 ms to the 1.1909 ms frame, 'temporal' (um_disp_fuse)
 * 0.0099 ms, 'both' 0.0435 ms; the maps of 'both' composed from torch device
 * ops (25 shifted-slice taps, elementwise filter) after the plain pipeline add
 * 2.5978 ms (59.7x).  'both' beat the composition in each of the 3 repeats; the
 * composition's five maps differ from the stage's in 0 of 1 310 720 elements
 * each. */
int um_disp_smooth(const float* disp, const float* unc, const unsigned char* frame, int N, int Hs,
                   int Ws, int R, int step, const float* S, const float* G, const float* fp,
                   float* disp_out, float* unc_out, hipStream_t stream);
int um_disp_fuse(const float* disp_in, const float* unc_in, const float* lr_error, long count,
                 const float* params, const float* fp, float* mean, float* var, float* disparity,
                 float* uncertainty, float* depth, unsigned char* valid, float* disp_var,
                 hipStream_t stream);

/* ------------------------------------------------ SyncBN exchange (IPC) ---
 * SyncBatchNorm statistics exchanged device-side over IPC-mapped per-rank
 * arenas instead of one RCCL all-reduce per layer and direction (reference
 * parallel_main.py:156-158: torch SyncBatchNorm's all-reduce).  Host-only:
 * um_bnx_bytes (arena size for nslots exchanges of <= max_c channels),
 * um_bnx_alloc (uncached arena, zeroed, + its 64-byte hipIpcMemHandle_t),
 * um_bnx_open / um_bnx_close (a peer's arena), um_bnx_free, um_bnx_status
 * (1 if an exchange timed out waiting for a peer).  um_bnx_allreduce: the
 * statistics slots `stats` ([UM_STAT_SLOTS][C][2] f64 + count) of this rank
 * become the rank-ordered sum over all ranks (slot 0; slots 1.. zero; the
 * global count after them) -- the in-place all-reduce of the slots.
 * table: device array of the world arena base addresses (own at [rank]). */
long um_bnx_bytes(int nslots, int max_c);
int um_bnx_alloc(long bytes, void** base, void* handle64);
int um_bnx_open(const void* handle64, void** ptr);
int um_bnx_close(void* ptr);
int um_bnx_free(void* base);
int um_bnx_status(const void* base);
int um_bnx_allreduce(double* stats, int C, const unsigned long long* table, int world, int rank,
                     int slot, int nslots, int max_c, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UMAMD_H */
