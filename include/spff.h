/* spff.h -- C ABI of the MI355X-native SPFF-UNet engine (libspff_hip.so).
 *
 * This is the drop-in boundary for the reference's hot path: the SPFF-UNet
 * forward (innovative3D/models.py:693-701 UNet3D_SpectralCore.forward with the
 * _DoubleConvSpectral_Novel blocks of models.py:1448-1544, built by
 * build_spct_energyfilm_fourier models.py:1547-1555 behind
 * LitSPCT_EFiLM_FourierGate models.py:1558-1564), the loss
 * ce_plus_macro_dice_loss (helpers.py:797-803) and autograd's backward of both.
 * The reference binds these through PyTorch; the Python mirror in
 * spff-unet-spcct_amd/innovative3D binds them with ctypes.
 *
 * Conventions: plain device pointers + sizes, no torch types.  All calls are
 * stream-ordered and asynchronous (hipStream_t passed as void*; NULL = default
 * stream).  Activations are fp32; the network input is the reference layout
 * [B][Cin][D][H][W]; logits/dlogits are channel-last [B][D][H][W][K] (a
 * torch.channels_last_3d view of the reference's [B][K][D][H][W]).  Params /
 * dparams are ONE flat fp32 buffer in reference state-dict order (see
 * spff_param_info; the lazily created FourierGate mask appears once, under
 * "...fgate.freq_mask", and stands for the aliased "...fgate._mask" key).
 * Functions return 0 on success, a negative SPFF_E* code otherwise (never
 * throw); spff_last_error() describes the last failure of the calling thread.
 * A plan is not thread-safe and holds one forward's saved activations inside
 * the caller's workspace until the matching backward.
 */
#ifndef SPFF_H_
#define SPFF_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPFF_OK 0
#define SPFF_EINVAL (-1)
#define SPFF_EHIP (-2)
#define SPFF_ESHAPE (-3)
#define SPFF_ECOLL (-4) /* a shard-group collective callback (spff_coll) returned non-zero */

/* arithmetic of the 3x3x3 conv contractions (spff_cfg.math):
 *   SPFF_MATH_F32     fp32 MFMA (v_mfma_f32_32x32x2_f32, an exact fp32 fma chain)
 *   SPFF_MATH_BF16X6  fp32 operands split exactly into 3 bf16 planes, 6 cross
 *                     products on the bf16 MFMA, fp32 accumulate: dropped terms
 *                     < 2^-24 |xy| per product (fp32 accuracy class), ~2.7x the rate
 *   SPFF_MATH_BF16X3  2 planes, 3 products: ~2^-17 relative per product (opt-in)
 *   SPFF_MATH_F16X3   each operand scaled by a power of two (max |x| 2^e < 2^14, from an
 *                     on-device absmax) and split into 2 fp16 planes, 3 products on the
 *                     fp16 MFMA: <= 2^-22 |x| per operand, dropped l*l <= 2^-22 |xy|,
 *                     at the bf16x3 rate (the ConvTranspose and head GEMMs follow the conv
 *                     arithmetic: scaled fp16 planes too; the bias-free 1x1x1 convs and
 *                     nn.Linear layers of the SwinUNETR / R2UNet3D plans run the fp32 MFMA) */
/* largest num_classes of the SPFF / 3DUNet plans and of spff_loss / spff_confusion
 * (the SwinUNETR plan's soft-Dice loss: 32) */
#define SPFF_MAX_CLASSES 128

#define SPFF_MATH_F32 0
#define SPFF_MATH_BF16X6 1
#define SPFF_MATH_BF16X3 2
#define SPFF_MATH_F16X3 3

typedef struct spff_cfg {
  int batch, in_ch, depth, height, width;  /* input [B][Cin][D][H][W] */
  int num_classes;                          /* K, 1 .. SPFF_MAX_CLASSES */
  int base;                                 /* f: a multiple of 8 (>= 8) */
  int ksd;                                  /* spectral kernel depth: 1 or 3 */
  int use_efilm, use_fgate;                 /* novel block (models.py:1448) */
  int use_se, use_specse;                   /* encoder post (models.py:684) */
  int math;                                 /* SPFF_MATH_* (0 = fp32 MFMA) */
  /* depth sharding (BASELINE config 4): this plan holds global depths
   * [shard_rank * depth, (shard_rank + 1) * depth) of a volume of depth
   * shard_world * depth; requires batch == 1 and a collectives table, see spff_coll below.
   * shard_world <= 1: unsharded. */
  int shard_world, shard_rank;
  /* saved-activation layout: SPFF_MEM_FULL keeps every block's conv outputs, IN /
   * gate outputs and up-conv outputs (~2.8 KB per input voxel); SPFF_MEM_LEAN keeps
   * only the conv outputs y1, y2 and per-(b,c[,d]) coefficients and recomputes the
   * rest in the backward (~1.7 KB per voxel: one 5 x 512^3 volume fits one MI355X;
   * +~3 % step time); SPFF_MEM_AUTO (0) = lean from 2^26 voxels per plan, never the
   * forward-only layout; SPFF_MEM_INFER: see below. */
  int memory_mode;
  /* the axis a sharded plan (shard_world > 1) splits: SPFF_SHARD_DEPTH (0) -- above;
   * SPFF_SHARD_HEIGHT (1) -- the registry layout [B, 1, 5, H, W]: this
   * plan holds global rows [shard_rank * height, (shard_rank + 1) * height) of a volume
   * of height shard_world * height; height and width multiples of 8 (the three (1,2,2)
   * pools stay rank-local), any batch.  Same collectives table. */
  int shard_axis;
  /* the novel block's EnergyFiLM3D(hidden, pe_dims) and FourierGate3D(learn_phase)
   * (models.py:1484-1489, 1521-1541), the same in every block; 0 = the reference's
   * defaults (32, 16, off: what _DoubleConvSpectral_Novel builds).  hidden 1..64,
   * pe_dims 2..32 ((hidden + pe_dims) * depth * 4 B of LDS <= 160 KiB) */
  int efilm_hidden, efilm_pe_dims, fgate_learn_phase;
  /* UNet3D_SpectralCore(use_spatial, use_skip_gate) (models.py:654-682): CBAM spatial
   * attention after each encoder stage's Spectral-SE / Channel-SE (parameters
   * sa.{0..3}.conv.weight [1][2][3][7][7]) and attention gates g3, g2, g1 on the skips (the
   * gate multiplies the up-conv output; the decoder reads [up | gated up]).  0, 0: the plans
   * as before.  Either flag: unsharded plans only (SPFF_EINVAL otherwise), never the lean
   * layout (SPFF_MEM_LEAN: SPFF_EINVAL; SPFF_MEM_AUTO resolves to the full one);
   * use_skip_gate needs H and W multiples of 8 (SPFF_ESHAPE: where the reference's _cat
   * would resize, its gate fails on the mismatched shapes). */
  int use_spatial, use_skip_gate;
} spff_cfg;

#define SPFF_SHARD_DEPTH 0
#define SPFF_SHARD_HEIGHT 1

#define SPFF_MEM_AUTO 0
#define SPFF_MEM_FULL 1
#define SPFF_MEM_LEAN 2
/* forward-only layout (inference): nothing is kept for a backward; the activations are
 * placed by liveness in three level-0 buffers (~0.6 KB per input voxel at base 32: one
 * 5 x 512^3 volume in ~73 GiB).  spff_forward returns the full layout's logits bit for bit;
 * spff_backward returns SPFF_EINVAL; spff_saved_tensor knows only "x_cl", the pools, the
 * per-(b,c) coefficients and "dec1.y2".  Unsharded plans without use_spatial /
 * use_skip_gate only (SPFF_EINVAL otherwise). */
#define SPFF_MEM_INFER 3

/* The shard group's collectives, implemented by the caller (e.g. RCCL through
 * torch.distributed) and called by the engine in stream order on the stream
 * argument: the stream of the current spff_forward / spff_backward, or -- for a
 * halo that overlaps a convolution's interior depth tiles -- the plan's side
 * stream, which the engine has made wait for the data and whose completion the
 * main stream waits for.  Issue the work on the stream given.  Return 0 on success.
 *   allreduce: in-place sum over the group of n elements at device pointer buf
 *              (dtype 0 = fp32, 1 = fp64).
 *   halo:      interior points at slice 0 of a [d_local][slice_floats] slab
 *              that has one writable slice before it and one after it: send
 *              slice 0 to rank - 1 and slice d_local - 1 to rank + 1, and receive
 *              rank - 1's last slice into interior[-slice_floats ..) and
 *              rank + 1's first slice into interior[d_local * slice_floats ..).
 *              Slices beyond the global ends are zeroed by the engine. */
typedef struct spff_coll {
  void* ctx;
  int (*allreduce)(void* ctx, void* buf, int64_t n, int dtype, void* stream);
  int (*halo)(void* ctx, float* interior, int64_t slice_floats, int d_local, void* stream);
} spff_coll;

typedef struct spff_plan spff_plan;

/* plan lifetime (replaces build_class(...)() -> module construction, config.py:159-182) */
int spff_plan_create(const spff_cfg* cfg, spff_plan** out);
void spff_plan_destroy(spff_plan* plan);
/* attach the shard group's collectives (required before the first forward of a
 * plan with shard_world > 1; the table is copied) */
int spff_plan_set_coll(spff_plan* plan, const spff_coll* coll);
/* gradient-ready hook (data parallelism; replaces the bucketed gradient
 * all-reduce torch DDP hangs on autograd for the reference's module, SURVEY
 * §8(e) DP row): during spff_backward the engine calls fn(ctx, off, n, stream)
 * in stream order as soon as dparams[off, off + n) is final (one call per
 * block's parameters, per SE / up-conv / head group; together they cover every
 * float once), so the caller can issue that range's all-reduce on a
 * collective stream that waits on `stream` while the backward continues.
 * fn == NULL removes the hook.  Return 0 from fn, else the backward fails. */
typedef int (*spff_grad_ready_fn)(void* ctx, int64_t off, int64_t n, void* stream);
int spff_plan_set_grad_hook(spff_plan* plan, spff_grad_ready_fn fn, void* ctx);
const char* spff_last_error(void);

/* flat parameter layout (reference state-dict order, models.py:655-681) */
int spff_num_params(const spff_plan* plan);
int spff_param_info(const spff_plan* plan, int i, const char** name, int* ndim,
                    int64_t shape[5], int64_t* offset, int64_t* numel);
int64_t spff_param_floats(const spff_plan* plan);
size_t spff_workspace_bytes(const spff_plan* plan);

/* forward: x [B][Cin][D][H][W] -> logits [B][D][H][W][K]  (models.py:693-701) */
int spff_forward(spff_plan* plan, const float* x, const float* params, float* logits,
                 void* workspace, void* stream);
/* forward + class mask (test.py evaluate, per_class_metrics_3d helpers.py:668-725), on a
 * plan of any memory mode with K <= 255: mask [V] (V = B D H W, rows in logits order) = the
 * argmax of each voxel's logits, first maximum wins (spff_confusion's rule); with labels
 * [V], conf = K*(K+1) int64 as spff_confusion gives for the same logits (use_ignore = 0: no
 * voxel is masked), zeroed on the stream by a kernel (a captured graph replays it); conf is
 * NULL exactly when labels is.  logits [V][K] channel-last as spff_forward's, or NULL: where
 * the streaming head covers the plan (base 32 or 64, K <= 32) the head forms the class and
 * the counts from the logits it holds in registers and NULL means they are never written;
 * elsewhere logits must be given (SPFF_EINVAL otherwise) and a row-argmax pass reads them.
 * No host synchronisation. */
int spff_predict(spff_plan* plan, const float* x, const float* params,
                 uint8_t* mask,            /* [V] class index */
                 float* logits,            /* [V][K] channel-last, or NULL */
                 const int64_t* labels,    /* [V] or NULL */
                 int use_ignore, int ignore_index,
                 int64_t* conf,            /* K*(K+1), as spff_confusion; NULL iff labels NULL */
                 void* workspace, void* stream);
/* backward of the last forward: dlogits [B][D][H][W][K] -> dparams (flat, every
 * entry written).  Input gradient is not produced (the hot path never needs it). */
int spff_backward(spff_plan* plan, const float* dlogits, const float* params, float* dparams,
                  void* workspace, void* stream);
/* device pointer + shape of a saved intermediate (debug / tests), e.g. "enc1.out"
 * (fp32 [nvox][channels]); "pool1.idx" .. "pool3.idx" are the max-pools' argmax BYTES
 * [nvox][channels] (k = 2 dh + dw of each 2 x 2 window, first max in scan order) */
int spff_saved_tensor(const spff_plan* plan, void* workspace, const char* name,
                      const float** ptr, int64_t* nvox, int* channels);
/* The backward's scratch, "grad.out", "grad.dy2", "grad.da1", "grad.dx" and
 * "grad.dskip0" .. "grad.dskip2", holds the last block that ran (debug key 0 stops after a
 * chosen one).  The four views are reported as level-0 [V0][base]; a level-l tensor is the
 * flat prefix [V_l][C_l] of that.  After a block:
 *   grad.dy2  the gradient at its conv2 output y2 (after the gate backward, the LeakyReLU
 *             and the InstanceNorm backward);
 *   grad.da1  the gradient at its conv1 output y1 (at a1 before the in-place IN backward);
 *   grad.dx   its input gradient: for dec1..3 the up-conv half only, [V_l][C_l] (the skip
 *             half goes to grad.dskip<l>, or to grad.dy2 when skips are gated); for bott,
 *             enc3 and enc2 the gradient at the pool output; enc1 writes none;
 *   grad.out  the gradient at the output of dec3, dec2 or bott, as the up-conv's input
 *             gradient left it; at dec1's only with key 4 = 0 (the folded head never
 *             stores it).  Lean plans reuse it and grad.dy2 within a decoder block;
 *   grad.dskip<l>  [V_l][C_l]: after decoder block l the skip's share of the gradient at
 *             encoder output l; after the whole backward with key 2 = 0 the total (skip +
 *             MaxPool backward); with key 2 = 1 the readers form the total and it stays
 *             the skip's share. */

/* debug knobs (tests):
 * key 0 = stop the backward after N blocks: 1, 2, 3 = after dec1, dec2, dec3 (before that
 * block's up-conv gradients), 4 = after bott, 5 = after enc3, 6 = after enc2; -1 (the
 * default), 0 or 7 = the whole backward.  Parameter gradients of the blocks not run are
 * left unwritten;
 * key 1 = also store the block outputs the up-conv / head GEMMs apply on the fly
 * (bott/dec*.out; otherwise spff_saved_tensor reports them as not stored);
 * key 2 = 0: the encoder blocks' output gradient (skip + MaxPool backward) materialised by a
 * pass of its own into grad.dskip<l>, instead of formed by its two readers (the default, 1);
 * key 3 = 0: conv1's InstanceNorm-backward sums by a slab reduction over (da1, y1) instead
 * of in the epilogue of the input-gradient conv that writes da1 (the default, 1);
 * key 4 = 0: the head's backward as passes of its own (weight gradient, input gradient)
 * before the last block's tail reduction, instead of folded into that block's passes;
 * key 5 = 1: spff_forward / spff_predict run the head alone, on the last block's conv output
 * and coefficients that the previous call left in the workspace (timing the head by itself) */
int spff_debug_set(spff_plan* plan, int key, int value);

/* optional HIP-event timing of the engine's kernels on the plan's stream (bench.py):
 * classes 0 = conv3d fwd, 1 = conv3d dgrad (same kernel), 2 = conv3d wgrad,
 * 3 = ConvTranspose / 1x1 head GEMMs, and the HBM-bound passes 4 = per-(b,c,d)
 * slab reductions (IN statistics, gate sums; incl. the split combine),
 * 5 = IN/gate apply (act_apply), 6 = IN backward apply (in_bwd_apply), 7 = the
 * SPFF_MATH_F16X3 operand-max passes of the weight gradients' scales (the weights, the
 * block inputs, the a1 bound; per launch in sharded plans).
 * collect() syncs on the recorded events and writes out[4*c + {0,1,2,3}] =
 * {total ms, algorithmic FLOPs, launches, algorithmic HBM bytes (operands read
 * once, result written once)}. */
int spff_prof_enable(spff_plan* plan, int on);
int spff_prof_collect(spff_plan* plan, double* out, int nclass);
/* Library-wide conv timing: HIP events around every 3x3x3 conv launch (forward, input
 * gradient, weight gradient) on the stream it runs on, whichever plan or op entry point
 * issues it (the 3DUNet / SwinUNETR plans included).  collect: out[4 c + {0,1,2,3}] =
 * (ms, algorithmic fp32 flops 2 V Cin Cout T, launches, 0) for class c = 0 fwd, 1 dgrad,
 * 2 wgrad; synchronises on the recorded events and resets the record.  The UNETR plan also
 * brackets its token path (class 5: patch embedding, ViT blocks, final norm, forward and
 * backward) and its resampling passes (class 6), without flops. */
int spff_conv_prof_enable(int on);
int spff_conv_prof_collect(double* out, int nclass);

/* ce_plus_macro_dice_loss (helpers.py:797-803) on channel-last logits [V][K].
 * out4 (device) = [ce, ce + 0.5*hard_dice_loss, hard_dice_loss, n_valid];
 * dlogits = d(ce)/dlogits (softmax - onehot)/N_valid (0 for ignored voxels);
 * conf (device) = K*(K+1) int64: conf[pred*(K+1) + label] over non-ignored
 * voxels (argmax, first max wins), column K = labels outside [0,K) (the
 * reference raises on those in the loss; they are excluded from CE here).
 * count_override (device int64*, may be NULL): global N_valid for data-parallel
 * runs (all-reduced by the caller); NULL -> counted locally. */
size_t spff_loss_ws_bytes(int64_t nvox, int num_classes);
int spff_loss(const float* logits, const int64_t* labels, int64_t nvox, int num_classes,
              int ignore_index, double smooth, const int64_t* count_override, float* out4,
              float* dlogits, int64_t* conf, void* ws, void* stream);
/* argmax confusion only (per_class_metrics_3d, helpers.py:668-725) */
int spff_confusion(const float* logits, const int64_t* labels, int64_t nvox, int num_classes,
                   int ignore_index, int64_t* conf, void* stream);
int spff_count_valid(const int64_t* labels, int64_t nvox, int ignore_index, int64_t* count,
                     void* stream);
/* The ranking metrics of the test-only block of BaseLitModel._shared_step
 * (models.py:510-584: precision_recall_curve + auc and roc_auc_score per class,
 * models.py:521-535, and over the concatenated classes 1..K-1, models.py:552-565) and of
 * the per-volume rows of train.py:773-798, exact and tie-aware (rank.hip: a segmented
 * radix sort of (score, is_positive) keys and a scan over the groups of equal scores).
 * scores: channel-last rows [batch][vox_per_sample][K]; from_logits = 1: logits, ranked by
 * their fp32 softmax; 0: the scores themselves, finite and >= 0 (-0.0 ranks as +0.0).
 * A voxel is positive for class c iff label == c; every other label value, 255 included,
 * is a negative (models.py:522: there is no ignore mask).
 * per_sample = 0: one segment per class over the whole batch and the micro segment;
 * out = K + 1 rows, the micro row last (NaN when K < 2).  per_sample = 1: batch * K
 * segments of vox_per_sample voxels, out = batch * K rows in (b, c) order.
 * A row is 4 device doubles [pr_auc, roc_auc, n_pos, n_neg]; both areas are NaN when
 * n_pos == 0 or n_neg == 0 (models.py:530).  Two calls on the same input give the same
 * bits.  ws >= spff_rank_auc_ws_bytes device bytes (at most 16 K batch vox_per_sample +
 * 1 MiB; 0 for arguments that spff_rank_auc rejects). */
size_t spff_rank_auc_ws_bytes(int batch, int64_t vox_per_sample, int num_classes, int per_sample);
int spff_rank_auc(const float* scores, const int64_t* labels, int batch, int64_t vox_per_sample,
                  int num_classes, int from_logits, int per_sample, double* out, void* ws,
                  void* stream);
/* The qualitative views of the reference's figures (views.hip), formed where the logits
 * lie instead of on the host after a copy.
 * spff_pred_views: _prediction_views_and_mip (train.py:649-671, 933-951) for every sample
 * of logits [B][D][H][W][K] channel-last fp32, K in 1..32.  Per voxel the reference's
 * fp32 softmax (max-subtracted expf summed in class order, divided by sum + 1e-8f);
 *   center_pred  uint8 [B][H][W]     argmax over the classes at depth D / 2, first maximum
 *   alpha_center float [B][H][W]     that row's largest probability
 *   mip_prob     float [B][H][W][K]  the maximum over depth of every class's probability
 *   mip_pred     uint8 [B][H][W]     argmax over the classes of mip_prob, first maximum
 *                                    (the reference's summary_pred and mip_pred)
 * depth_split = 0: the depth is split over workgroups as the kernel sees fit; n in 1..D:
 * over n ranges.  A maximum does not depend on grouping or order: every split, and every
 * call, gives the same bits.  ws >= spff_pred_views_ws_bytes device bytes (0 for arguments
 * that spff_pred_views rejects); it needs no clearing.  No allocation, no host
 * synchronisation.  SPFF_EINVAL before any device call: a null pointer, K outside 1..32,
 * an extent below 1, depth_split < 0 or > D. */
size_t spff_pred_views_ws_bytes(int B, int D, int H, int W, int num_classes);
int spff_pred_views(const float* logits, int B, int D, int H, int W, int num_classes,
                    int depth_split, uint8_t* center_pred, float* alpha_center, float* mip_prob,
                    uint8_t* mip_pred, void* ws, void* stream);
/* The input's two grey images (_center_frame_from_input and _mip_from_input_tensor,
 * train.py:616-634): x [B][C][D][H][W] fp32; center [B][H][W] = x[b][0][D / 2],
 * mip [B][H][W] = the maximum over depth of x[b][0]; range [B][4] = (min, max) of center
 * and (min, max) of mip, which imshow's grey scale needs. */
int spff_input_views(const float* x, int B, int C, int D, int H, int W, float* center, float* mip,
                     float* range, void* stream);
/* The five panels of _render_buffer (train.py:1096-1111; test.py:581-744 draws the same)
 * as one strip rgb uint8 [B][H][5 W][3], without titles and legend.  Grey value of an image:
 * g = rint(255 (v - min) / (max - min)), 0 where max == min.  Panels: 0 the centre frame;
 * 1 it under the ground-truth centre slice; 2 it under center_pred; 3 the MIP under
 * mip_pred; 4 the centre frame under center_pred with confidence-weighted alpha.  A blended
 * pixel is rint((1 - a) g + a colour[class]): a = 0.85 in panels 1..3 and
 * 0.8 clamp(alpha_center, 0.35, 1) in panel 4.  colors: uint8 [256][3] on the device (a class
 * without an entry is black: _color_mask, train.py:636-641).  labels_center: int64 [B][H][W],
 * may be NULL (panel 1 is then the grey frame); a label of 255 or >= num_classes leaves the
 * grey pixel.  center, mip, range: as spff_input_views writes them. */
int spff_overlay_rgb(const float* center, const float* mip, const float* range,
                     const int64_t* labels_center, const uint8_t* center_pred,
                     const uint8_t* mip_pred, const float* alpha_center, const uint8_t* colors,
                     int B, int H, int W, int num_classes, uint8_t* rgb, void* stream);
/* Sliding-window inference (tile.hip): the network runs on overlapping windows
 * [rd][rh][rw] of one volume and the window outputs are blended with a separable
 * window-centred weight.  windows: a HOST array [n][4] = z0, y0, x0, flip bits (1 = D,
 * 2 = H, 4 = W), n in 1..SPFF_TILE_MAX_WINDOWS; it travels to the kernels by value and is
 * validated first.  A flipped window is gathered mirrored along its axes and accumulated
 * mirrored back.
 *   gather      out [n][C][rd][rh][rw] = the windows of x [C][D][H][W].
 *   accumulate  acc[v][k] += (wz wy wx)(v) s[v][k] over the n windows in table order, fp32
 *               fmaf; s is the tile value or (softmax = 1) the fp32 softmax of the tile's row
 *               (max-subtracted expf summed in class order, a true division).  Windows of
 *               one call may overlap; a voxel's sum does not depend on how the table is
 *               split into calls.  tiles may hold more than n windows: the rest is not read.
 *   finalize    mask = the first maximum of each acc row (the rule of the confusion counts: a
 *               NaN counts as the largest); with labels, conf = K (K + 1) int64 counts as the
 *               confusion entry gives for the same rows, zeroed on the stream by a kernel;
 *               scores (may be NULL, may be acc itself) = acc / (flips nz[z] ny[y] nx[x]).
 * Stream-ordered, no allocation, no host synchronisation; a captured graph replays them.
 * Before any device call: SPFF_EINVAL for K outside 2..32, n outside 1..64, a null required
 * pointer, an extent below 1, flip bits outside 0..7, conf NULL without labels NULL or the
 * reverse; SPFF_ESHAPE for a window extent above the volume's or a window not wholly inside
 * the volume. */
#define SPFF_TILE_MAX_WINDOWS 64
int spff_tile_gather(const float* x, int C, int D, int H, int W, /* one volume [C][D][H][W] */
                     const int32_t* windows, int n, int rd, int rh, int rw,
                     float* out, /* [n][C][rd][rh][rw] */
                     void* stream);
int spff_tile_accumulate(const float* tiles, /* [n][rd][rh][rw][K] channel-last */
                         const int32_t* windows, int n, int rd, int rh, int rw, int K,
                         int D, int H, int W,
                         const float* wz, const float* wy, const float* wx, /* device [rd], [rh], [rw] */
                         int softmax,
                         float* acc, /* [D][H][W][K], zeroed by the caller */
                         void* stream);
int spff_tile_finalize(const float* acc, int D, int H, int W, int K,
                       const float* nz, const float* ny, const float* nx, float flips, /* scores only */
                       uint8_t* mask,  /* [D][H][W] */
                       float* scores,  /* [D][H][W][K] or NULL */
                       const int64_t* labels, int use_ignore, int ignore_index,
                       int64_t* conf,  /* K*(K+1); NULL iff labels NULL */
                       void* stream);
/* x[i] *= *scale (scale is a device scalar) */
int spff_scale(float* x, int64_t n, const float* scale, void* stream);

/* fused Adam / AdamW step over n contiguous fp32 elements (replaces the
 * torch.optim.Adam of BaseLitModel.configure_optimizers, models.py:591-594, and
 * unified_optimizer.py:5-60): decoupled = 1 is AdamW; step = the 1-based step
 * count after this update; arithmetic in torch's fp32 operation order. */
int spff_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   int64_t n, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int decoupled, int64_t step, void* stream);

/* op-level entry points (parity tests): channel-last activations, reference
 * weight layout W[Cout][Cin][ksd][3][3].  ws >= spff_conv3d_ws_bytes(...). */
size_t spff_conv3d_ws_bytes(int B, int D, int H, int W, int cin, int cout, int ksd);
int spff_conv3d_fwd(const float* x, int ldx, const float* w, float* y, int B, int D, int H, int W,
                    int cin, int cout, int ksd, void* ws, void* stream);
int spff_conv3d_dgrad(const float* dy, const float* w, float* dx, int B, int D, int H, int W,
                      int cin, int cout, int ksd, void* ws, void* stream);
/* the same with an explicit SPFF_MATH_* arithmetic (the two above use SPFF_MATH_F32) */
int spff_conv3d_fwd_ex(const float* x, int ldx, const float* w, float* y, int B, int D, int H,
                       int W, int cin, int cout, int ksd, int math, void* ws, void* stream);
int spff_conv3d_dgrad_ex(const float* dy, const float* w, float* dx, int B, int D, int H, int W,
                         int cin, int cout, int ksd, int math, void* ws, void* stream);
int spff_conv3d_wgrad(const float* x, int ldx, const float* dy, float* dw, int B, int D, int H,
                      int W, int cin, int cout, int ksd, void* ws, void* stream);
int spff_conv3d_wgrad_ex(const float* x, int ldx, const float* dy, float* dw, int B, int D,
                         int H, int W, int cin, int cout, int ksd, int math, void* ws,
                         void* stream);
/* the same with dy's channel stride lddy >= cout (a multiple of 4), so cout need not be one */
int spff_conv3d_wgrad_ld(const float* x, int ldx, const float* dy, int lddy, float* dw, int B,
                         int D, int H, int W, int cin, int cout, int ksd, int math, void* ws,
                         void* stream);
/* Op-level ConvTranspose3d(cin -> cout, kernel = stride = (1,2,2)) + bias (reference
 * models.py:668-672, the decoder up-convolutions) on channel-last tensors: x [B][D][H][W][cin]
 * low resolution, y [B][D][2H][2W][cout]; weight W[cin][cout][1][2][2], bias [cout].
 * math = SPFF_MATH_*: the GEMM arithmetic (f32 MFMA, the exact bf16x6 split, or f16x3 with
 * per-chunk power-of-two scales).  dgrad: dx = the input gradient of dy; wgrad: dw, db
 * (overwritten).  ws >= spff_upconv_ws_bytes(...). */
size_t spff_upconv_ws_bytes(int B, int D, int H, int W, int cin, int cout);
int spff_upconv_fwd(const float* x, const float* w, const float* b, float* y, int B, int D, int H,
                    int W, int cin, int cout, int math, void* ws, void* stream);
int spff_upconv_dgrad(const float* dy, const float* w, float* dx, int B, int D, int H, int W,
                      int cin, int cout, int math, void* ws, void* stream);
int spff_upconv_wgrad(const float* x, const float* dy, float* dw, float* db, int B, int D, int H,
                      int W, int cin, int cout, int math, void* ws, void* stream);
/* Op-level CBAM spatial attention (reference SpatialAttention3D, models.py:434-446) on
 * channel-last fp32 x, y, dy, dx [B][D][H][W][C], C a multiple of 8; w is conv.weight
 * [1][2][3][7][7] (no bias).  fwd: map [V][2] = (mean_c x, max_c x), idx [V] = the lowest
 * channel that holds the max, attn [V] = sigmoid(conv3d(map, w, zero padding (1,3,3))),
 * y = x * attn (V = B D H W).  bwd takes what fwd wrote and gives dx and dw [294]
 * (overwritten; dx may be dy, y may be x).  Every sum has a fixed order: two calls give the same bits.
 * x, y, dy, dx, map and ws are 16-byte aligned; ws >= spff_spatial_attn_ws_bytes(...) for
 * bwd (fwd does not touch it and takes NULL). */
size_t spff_spatial_attn_ws_bytes(int B, int D, int H, int W, int C);
int spff_spatial_attn_fwd(const float* x, const float* w, int B, int D, int H, int W, int C,
                          float* y, float* attn, float* map, int32_t* idx, void* ws,
                          void* stream);
int spff_spatial_attn_bwd(const float* dy, const float* x, const float* w, const float* attn,
                          const float* map, const int32_t* idx, int B, int D, int H, int W, int C,
                          float* dx, float* dw, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * 3D U-Net baseline variant (BASELINE config 3; registry entry "3DUNet",
 * config.py:283-311): LitCicek3DUNet_DepthAdapter_Published (models.py:756-853)
 * = _resize_depth_like (models.py:153-157) -> Cicek3DUNet (models.py:718-753:
 * 4 x [Conv3d(3, bias=False) -> BatchNorm3d -> ReLU] x 2 + MaxPool3d(2) down,
 * ConvTranspose3d(2, stride 2) + concat [up, skip] up, 1x1x1 head) ->
 * _resize_logits_depth_like (models.py:159-163).  Same conventions as above:
 * params flat in reference state-dict order (names without the "backbone."
 * prefix), BatchNorm running_mean / running_var in a second flat fp32 buffer
 * (spff_unet3d_buffer_info; num_batches_tracked stays with the caller).
 * -------------------------------------------------------------------------- */
typedef struct spff_unet3d_cfg {
  int batch, in_ch, depth, height, width;  /* input [B][Cin][D][H][W] */
  int target_depth;  /* depth adapter: D is resampled to this before the backbone and the
                        logits back to D (trilinear, align_corners=False); 0 = none.  The
                        backbone depth, H and W must be multiples of 16 (4 poolings). */
  int num_classes;   /* K (<= 32) */
  int base;          /* f (power of two, >= 8); the reference wrapper uses 32 */
  int math;          /* SPFF_MATH_* for the 3x3x3 convolutions */
  int reserved[7];   /* zero */
} spff_unet3d_cfg;

typedef struct spff_unet3d spff_unet3d;

int spff_unet3d_create(const spff_unet3d_cfg* cfg, spff_unet3d** out);
void spff_unet3d_destroy(spff_unet3d* net);
int spff_unet3d_num_params(const spff_unet3d* net);
int spff_unet3d_param_info(const spff_unet3d* net, int i, const char** name, int* ndim,
                           int64_t shape[5], int64_t* offset, int64_t* numel);
int64_t spff_unet3d_param_floats(const spff_unet3d* net);
int spff_unet3d_num_buffers(const spff_unet3d* net);
int spff_unet3d_buffer_info(const spff_unet3d* net, int i, const char** name, int64_t* offset,
                            int64_t* numel);
int64_t spff_unet3d_buffer_floats(const spff_unet3d* net);
size_t spff_unet3d_workspace_bytes(const spff_unet3d* net);
/* forward: x [B][Cin][D][H][W] -> logits [B][D][H][W][K].  training = 1:
 * BatchNorm normalises with batch statistics and updates running_mean /
 * running_var in `buffers` (momentum 0.1, unbiased variance); 0: normalises
 * with the running statistics (buffers read only). */
int spff_unet3d_forward(spff_unet3d* net, const float* x, const float* params, float* buffers,
                        int training, float* logits, void* workspace, void* stream);
/* backward of the last forward: dlogits [B][D][H][W][K] -> dparams (every entry written) */
int spff_unet3d_backward(spff_unet3d* net, const float* dlogits, const float* params,
                         float* dparams, void* workspace, void* stream);
/* Synchronised BatchNorm for data parallelism (torch.nn.SyncBatchNorm semantics): with a
 * table (only its allreduce is used; in-place fp64 sum over the group, in stream order) and
 * world > 1, every train-mode BatchNorm3d all-reduces its per-channel batch moments and its
 * backward's two per-channel sums, so each rank normalises with the global batch statistics
 * and updates identical running statistics; the BN weight / bias gradients stay this
 * rank's partial sums (the caller SUM-all-reduces the flat gradient).  Every rank must run
 * the plan's shape.  NULL or world <= 1: per-replica statistics (the default). */
int spff_unet3d_set_sync_bn(spff_unet3d* net, const spff_coll* coll, int world);
int spff_unet3d_saved_tensor(const spff_unet3d* net, void* workspace, const char* name,
                             const float** ptr, int64_t* nvox, int* channels);

/* the weighted softmax CE of the 3DUNet wrapper (_weighted_softmax_ce,
 * models.py:779-799): as spff_loss, plus optional per-class weights
 * (class_weights: K device floats or NULL) and clamp_denominator = 1 for the
 * wrapper's sum / max(N_valid, 1). */
int spff_loss_ex(const float* logits, const int64_t* labels, int64_t nvox, int num_classes,
                 int ignore_index, double smooth, const int64_t* count_override,
                 const float* class_weights, int clamp_denominator, float* out4,
                 float* dlogits, int64_t* conf, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * R2UNet3D variant (registry entry "R2UNet3D"): LitR2UNet3D_Published around
 * R2UNet3D_backbone, the recurrent residual 3D U-Net.  Block(cin -> C, t):
 *   x1 = inp(x) (1x1x1, no bias);
 *   r_k = relu(IN(conv3x3x3(r_{k-1} + h_{k-1}))), r_0 = x1, h_0 = 0, h_k = r_k, k = 1..t,
 *         one conv and one affine InstanceNorm3d shared by the t steps;
 *   o = relu(IN(x1 + out(r_t))) (out: 1x1x1, no bias).
 * Five levels (channels base << l) with MaxPool3d(2) down, ConvTranspose3d(2, stride 2)
 * + concat [up, skip] up, and the wrapper's 1x1x1 head with bias.  InstanceNorm uses the
 * instance statistics in training and evaluation alike, so forward has no mode.
 * Parameters: one flat fp32 buffer in the Lit module's state-dict order and names
 * ("backbone.e1.inp.weight", "backbone.e1.ru.conv.weight", "backbone.e1.ru.inn.weight",
 * ... "backbone.d1.bn.bias", "head.weight", "head.bias": 73 entries).  D, H and W must be
 * multiples of 16 (the wrapper's replicate padding and centre crop stay with the caller).
 * Saved tensors (spff_r2u_saved_tensor), for <blk> in e1..e4, b, d4..d1: "<blk>.x1",
 * "<blk>.ru<k>" (k = 1..t: step k's activation as stored, i.e. the ReLU output for k = t
 * and twice it -- the next step's conv input r + h -- for k < t) and "<blk>.out".
 * -------------------------------------------------------------------------- */
typedef struct spff_r2u_cfg {
  int batch, in_ch, depth, height, width;  /* input [B][Cin][D][H][W], Cin 1..8 */
  int num_classes;   /* K, 2..32 (K = 1, the sigmoid branch, is not built) */
  int base;          /* a multiple of 8; the registry uses 16 */
  int t;             /* recurrence steps, 1..8; the registry uses 2 */
  int math;          /* SPFF_MATH_* for the 3x3x3 convolutions */
  int reserved[7];   /* zero */
} spff_r2u_cfg;

typedef struct spff_r2u spff_r2u;

int spff_r2u_create(const spff_r2u_cfg* cfg, spff_r2u** out);
void spff_r2u_destroy(spff_r2u* net);
int spff_r2u_num_params(const spff_r2u* net);
int spff_r2u_param_info(const spff_r2u* net, int i, const char** name, int* ndim,
                        int64_t shape[5], int64_t* offset, int64_t* numel);
int64_t spff_r2u_param_floats(const spff_r2u* net);
size_t spff_r2u_workspace_bytes(const spff_r2u* net);
/* forward: x [B][Cin][D][H][W] -> logits [B][D][H][W][K] (channel-last) */
int spff_r2u_forward(spff_r2u* net, const float* x, const float* params, float* logits,
                     void* workspace, void* stream);
/* backward of the last forward: dlogits [B][D][H][W][K] -> dparams (every entry written;
 * the shared conv / InstanceNorm gradients are summed over the steps t .. 1 in that order) */
int spff_r2u_backward(spff_r2u* net, const float* dlogits, const float* params, float* dparams,
                      void* workspace, void* stream);
int spff_r2u_saved_tensor(const spff_r2u* net, void* workspace, const char* name,
                          const float** ptr, int64_t* nvox, int* channels);
/* LitR2UNet3D_Published._dice_only_loss_with_logits, multi-class branch: p = softmax(logits)
 * and the one-hot labels, both masked by [y != ignore_index] (use_ignore = 0: no mask);
 * classes k >= 1 only; a sample counts iff it has a valid voxel with label >= 1; per kept
 * sample and class dice = (2 sum p g + 1e-6) / (sum p + sum g + 1e-6); loss = 1 - mean.
 * out4 = [dice_mean, loss, kept_samples, N_valid]; no sample kept: loss = dice = 0 and
 * dlogits = 0.  logits / dlogits [B][vox_per_sample][K] channel-last rows.
 * ws >= spff_r2u_dice_loss_ws_bytes device bytes. */
size_t spff_r2u_dice_loss_ws_bytes(int batch, int num_classes);
int spff_r2u_dice_loss(const float* logits, const int64_t* labels, int batch,
                       int64_t vox_per_sample, int num_classes, int use_ignore, int ignore_index,
                       float* out4, float* dlogits, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * ResUNet++ variant (registry entry "ResUNet++"): LitResUNetPP3D_Published around
 * ResUNetPP3D_backbone.  Channels c = base * (1, 2, 4, 8, 16), five levels, MaxPool3d(2).
 *   ResidualUnit(cin -> C): s = skip(x) (1x1x1 without bias; the identity when cin == C),
 *     a1 = relu(IN1(c1(x))), out = relu(IN2(c2(a1)) + s); c1, c2 3x3x3 without bias.
 *   e1..e4 with pools between; b = b_aspp_out(ASPP(b_aspp_in(pool(e4)))).
 *   ASPP(C): four 3x3x3 convs of one input with dilation = padding = 1, 2, 4, 8, concatenated
 *     in branch order, then a 1x1x1 conv without bias and a ReLU.
 *   SE(C): x * sigmoid(W2 relu(W1 mean(x) + b1) + b2), hidden max(1, C / 16).
 *   Decoder level l = 4..2: u = up_l(below); s = u * sigmoid(psi(relu(W_x u + W_g se_l(e_l))))
 *     (the gate multiplies the up-sampled tensor: the reference's argument order);
 *     d_l = ResidualUnit([u | s]).  Level 1 has no gate: d1 = ResidualUnit([u1 | se1(e1)]).
 *   logits = head(d1), a 1x1x1 conv with bias.
 * Parameters: one flat fp32 buffer in the Lit module's named_parameters() order and names
 * ("backbone.e1.c1.weight" ... "backbone.d1.skip.weight", "head.weight", "head.bias": 118
 * entries; b_aspp_out has no skip.weight).  D, H and W must be multiples of 16 and the
 * bottleneck must keep more than one voxel per sample (InstanceNorm).
 * Saved tensors (spff_rupp_saved_tensor): for <blk> in e1..e4, b_aspp_in, b_aspp_out,
 * d4..d1: "<blk>.a1" and "<blk>.out"; "b_aspp.out"; "ag<l>.att" (the gate's hidden row
 * after its ReLU, l = 4..2).
 * -------------------------------------------------------------------------- */
typedef struct spff_rupp_cfg {
  int batch, in_ch, depth, height, width;  /* input [B][Cin][D][H][W], Cin 1..8 */
  int num_classes;   /* K, 2..32 */
  int base;          /* a multiple of 8; the registry uses 16 */
  int math;          /* SPFF_MATH_* for the undilated 3x3x3 convolutions (the ASPP's dilated
                        convolutions always run fp32 MFMA arithmetic) */
  int reserved[8];   /* zero */
} spff_rupp_cfg;

typedef struct spff_rupp spff_rupp;

int spff_rupp_create(const spff_rupp_cfg* cfg, spff_rupp** out);
void spff_rupp_destroy(spff_rupp* net);
int spff_rupp_num_params(const spff_rupp* net);
int spff_rupp_param_info(const spff_rupp* net, int i, const char** name, int* ndim,
                         int64_t shape[5], int64_t* offset, int64_t* numel);
int64_t spff_rupp_param_floats(const spff_rupp* net);
size_t spff_rupp_workspace_bytes(const spff_rupp* net);
/* forward: x [B][Cin][D][H][W] -> logits [B][D][H][W][K] (channel-last) */
int spff_rupp_forward(spff_rupp* net, const float* x, const float* params, float* logits,
                      void* workspace, void* stream);
/* backward of the last forward: dlogits [B][D][H][W][K] -> dparams (every entry written) */
int spff_rupp_backward(spff_rupp* net, const float* dlogits, const float* params,
                       float* dparams, void* workspace, void* stream);
int spff_rupp_saved_tensor(const spff_rupp* net, void* workspace, const char* name,
                           const float** ptr, int64_t* nvox, int* channels);
/* dice_ce_loss_with_metrics: p = softmax(logits) and the one-hot labels, both masked by
 * [y != ignore_index] (use_ignore = 0: no mask); I, P, G summed over the whole batch;
 * dice_k = (2 I_k + 1e-6) / (P_k + G_k + 1e-6) over the classes 1..K-1 (include_bg: 0..K-1);
 * loss = dice_weight (1 - mean_k dice_k) + ce_weight CE, CE the mean over valid voxels.
 * out4 = [ce, loss, dice_mean, N_valid]; logits / dlogits [B][vox_per_sample][K]
 * channel-last rows.  ws >= spff_rupp_loss_ws_bytes device bytes. */
size_t spff_rupp_loss_ws_bytes(int batch, int num_classes);
int spff_rupp_loss(const float* logits, const int64_t* labels, int batch, int64_t vox_per_sample,
                   int num_classes, int use_ignore, int ignore_index, int include_bg,
                   double ce_weight, double dice_weight, float* out4, float* dlogits, void* ws,
                   void* stream);
/* The two losses below run on the same two passes.  m_v = [y_v != ignore_index] (use_ignore
 * = 0: no such mask), and m_v = 0 too for a label outside [0, K): such a voxel enters no sum
 * and its dlogits row is zero.  p = softmax(logits) in fp32, g = one-hot(y).  logits /
 * dlogits [B][vox_per_sample][K] channel-last rows; K in 2..32; SPFF_EINVAL (before any
 * device call) for K outside that range, batch < 1, vox_per_sample < 1 or a null out4,
 * dlogits or ws.
 *
 * spff_unet3d_loss: LitCicek3DUNet_DepthAdapter_Published._weighted_softmax_ce + ._dice_loss.
 *   ce = sum_v m u w[y] nll / max(sum_v m u, 1), u = voxel_weights [B vox_per_sample] (NULL:
 *   1), w = class_weights [K] (NULL: 1; class weights never enter the denominator);
 *   per sample b and class k = 1..K-1 (include_bg: 0..K-1) dice = 2 I / (P + G + 1e-6),
 *   I = sum m p g, P = sum m p, G = sum m g;  dice_loss = 1 - mean_{b,k} dice;
 *   loss = ce_weight ce + dice_weight dice_loss.
 *   out4 = [ce, loss, dice_loss, sum_v m u (before the clamp)].
 *   ws >= spff_unet3d_loss_ws_bytes device bytes. */
size_t spff_unet3d_loss_ws_bytes(int batch, int num_classes);
int spff_unet3d_loss(const float* logits, const int64_t* labels, int batch, int64_t vox_per_sample,
                     int num_classes, int use_ignore, int ignore_index,
                     const float* class_weights, const float* voxel_weights, int include_bg,
                     double ce_weight, double dice_weight, float* out4, float* dlogits, void* ws,
                     void* stream);
/* spff_nnunet_loss: models.dice_ce_loss (soft_dice_loss_from_logits + cross_entropy).
 *   I = sum m p g, Q = sum m p^2, G = sum m g over the whole batch;
 *   dice_k = (2 I_k + 1e-5) / (Q_k + G_k + 1e-5) over the classes 1..K-1 (include_bg: 0..K-1);
 *   loss = ce_weight CE + dice_weight (1 - mean_k dice_k), CE the mean over the voxels with
 *   m = 1 (NaN when there is none).
 *   out4 = [ce, loss, dice_mean, N_valid].  ws >= spff_nnunet_loss_ws_bytes device bytes. */
size_t spff_nnunet_loss_ws_bytes(int batch, int num_classes);
int spff_nnunet_loss(const float* logits, const int64_t* labels, int batch, int64_t vox_per_sample,
                     int num_classes, int use_ignore, int ignore_index, int include_bg,
                     double ce_weight, double dice_weight, float* out4, float* dlogits, void* ws,
                     void* stream);
/* Op-level dilated 3x3x3 convolution (the ASPP branches): dilation = padding = `dilation`
 * in all three axes, channel-last rows with pitches ldx / ldy (multiples of 4 floats, so a
 * branch can write its channel range of a wider row), weight W[cout][cin][3][3][3]; cin and
 * cout multiples of 4.  fp32 MFMA arithmetic.  Taps that lie outside the volume for every
 * output voxel are skipped (their weight gradient is zero).  dgrad: dx [.][ldx] = the input
 * gradient of dy [.][ldy], added to dx when accumulate != 0.  ws >=
 * spff_conv3d_dil_ws_bytes(cin, cout). */
size_t spff_conv3d_dil_ws_bytes(int cin, int cout);
int spff_conv3d_dil_fwd(const float* x, int ldx, const float* w, float* y, int ldy, int B, int D,
                        int H, int W, int cin, int cout, int dilation, void* ws, void* stream);
int spff_conv3d_dil_dgrad(const float* dy, int ldy, const float* w, float* dx, int ldx, int B,
                          int D, int H, int W, int cin, int cout, int dilation, int accumulate,
                          void* ws, void* stream);
int spff_conv3d_dil_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, int B,
                          int D, int H, int W, int cin, int cout, int dilation, void* ws,
                          void* stream);

/* ------------------------------------------------------------------------
 * SwinUNETR variant (BASELINE config 5; registry "SwinUNETR", config.py:366-386
 * -> LitSwinUNETR_Published / SwinUNETR_Published, models.py:858-982, i.e.
 * MONAI 1.5.2 SwinUNETR).  Replaces SwinUNETR_Published.forward
 * (models.py:877) and its autograd backward, and LitSwinUNETR_Published._loss
 * (models.py:910-928).  Parameters: a flat fp32 buffer in MONAI's state-dict
 * order / names without the "model.model." prefix (spff_swin_param_info);
 * the relative_position_index buffers are not needed.  D, H, W must be
 * multiples of 32.  Parity is unpinned (MONAI is not available offline);
 * semantics in oracle/swin_oracle.py.
 * ------------------------------------------------------------------------ */
typedef struct spff_swin_cfg {
  int batch, in_ch, depth, height, width;  /* input [B][Cin][D][H][W], Cin <= 8 */
  int num_classes;   /* K (<= 32) */
  int feature_size;  /* 12 on the registry path */
  int window;        /* MONAI window_size (7: the registry's (2,2,2) never reaches MONAI) */
  int heads[4];      /* (1, 2, 4, 8) */
  float mlp_ratio;   /* 2.0 */
  int math;          /* SPFF_MATH_* for the 3x3x3 convolutions */
  int reserved[6];   /* zero */
} spff_swin_cfg;

typedef struct spff_swin spff_swin;

int spff_swin_create(const spff_swin_cfg* cfg, spff_swin** out);
void spff_swin_destroy(spff_swin* net);
int spff_swin_num_params(const spff_swin* net);
int spff_swin_param_info(const spff_swin* net, int i, const char** name, int* ndim,
                         int64_t shape[5], int64_t* offset, int64_t* numel);
int64_t spff_swin_param_floats(const spff_swin* net);
size_t spff_swin_workspace_bytes(const spff_swin* net);
/* forward: x [B][Cin][D][H][W] -> logits [B][D][H][W][K] (channel-last) */
int spff_swin_forward(spff_swin* net, const float* x, const float* params, float* logits,
                      void* workspace, void* stream);
/* backward of the last forward: dlogits [B][D][H][W][K] -> dparams (every entry written) */
int spff_swin_backward(spff_swin* net, const float* dlogits, const float* params,
                       float* dparams, void* workspace, void* stream);
int spff_swin_saved_tensor(const spff_swin* net, void* workspace, const char* name,
                           const float** ptr, int64_t* rows, int* channels);
/* (1 - ce_weight) * soft-Dice loss (classes >= 1 unless include_bg) + ce_weight * CE
 * (ignore_index), LitSwinUNETR_Published._loss: out4 = [ce, loss, dice_loss, N_valid],
 * dlogits [V][K] = dloss/dlogits.  ws >= spff_swin_loss_ws_bytes device bytes. */
size_t spff_swin_loss_ws_bytes(int batch, int num_classes);
int spff_swin_loss(const float* logits, const int64_t* labels, int batch, int64_t vox_per_sample,
                   int num_classes, int ignore_index, int include_bg, double ce_weight,
                   float* out4, float* dlogits, void* ws, void* stream);

/* ------------------------------------------------------------------------
 * UNETR variant (registry "UNETR", config.py:316-339 -> LitUNETR_Published /
 * UNETR_Published, models.py:984-1115, i.e. MONAI 1.5.2 UNETR: 16^3 conv patch
 * embedding, learnable position embedding, twelve ViT blocks, InstanceNorm,
 * res_block).  Replaces the wrapper's resample -> UNETR -> resample (forward steps
 * 3-5) and its autograd backward; the loss is spff_swin_loss (the reference's
 * _loss is the Swin one line for line).  Parameters: a flat fp32 buffer in
 * MONAI's state-dict order / names without the "net.net." prefix
 * (spff_unetr_param_info); the cross-attention parameters that MONAI >= 1.4
 * registers in every block and never uses on this path are not part of it.
 * Parity is unpinned (MONAI is not available offline): every statement about
 * MONAI's UNETR here is an assumption restated in tests/_unetr_oracle.py.
 * ------------------------------------------------------------------------ */
typedef struct spff_unetr_cfg {
  int batch, in_ch, depth, height, width; /* the padded input [B][Cin][D][H][W], multiples of 16;
                        Cin = 1, the registry's: no other patch-embedding width is tested */
  int img[3];        /* the network grid (96, 96, 96), multiples of the 16^3 patch; at most 512
                        tokens, the attention kernels' two 256-row LDS chunks */
  int num_classes;   /* K (<= 32: spff_swin_loss) */
  int feature_size;  /* 16; a multiple of 8 (the conv kernels' channel tiles) */
  int hidden;        /* 768; <= 768 because the LayerNorm kernels hold a row as 12 channels
                        in each of a wave's 64 lanes */
  int mlp_dim;       /* 3072; a multiple of 4 (16-byte row loads of the Linear GEMMs) */
  int heads;         /* 12; hidden / heads in {16, 32, 64}, the attention kernels' instances */
  int math;          /* SPFF_MATH_* for the 3x3x3 convolutions */
  int reserved[6];   /* zero */
} spff_unetr_cfg;

typedef struct spff_unetr spff_unetr;

int spff_unetr_create(const spff_unetr_cfg* cfg, spff_unetr** out);
void spff_unetr_destroy(spff_unetr* net);
int spff_unetr_num_params(const spff_unetr* net);
int spff_unetr_param_info(const spff_unetr* net, int i, const char** name, int* ndim,
                          int64_t shape[5], int64_t* offset, int64_t* numel);
int64_t spff_unetr_param_floats(const spff_unetr* net);
size_t spff_unetr_workspace_bytes(const spff_unetr* net);
/* forward: x [B][Cin][D][H][W] -> logits [B][D][H][W][K] (channel-last); when (D, H, W)
 * differs from img the input is resampled to img and the logits back (trilinear,
 * align_corners=False) inside */
int spff_unetr_forward(spff_unetr* net, const float* x, const float* params, float* logits,
                       void* workspace, void* stream);
/* backward of the last forward: dlogits [B][D][H][W][K] -> dparams (every entry written) */
int spff_unetr_backward(spff_unetr* net, const float* dlogits, const float* params,
                        float* dparams, void* workspace, void* stream);
/* "tok", "h3", "h6", "h9", "hN", "enc1" .. "enc4", "dec5" .. "dec2", "block<i>.qkv|O|x1|out",
 * "<residual block>.y1|a1|y2|y3|out" */
int spff_unetr_saved_tensor(const spff_unetr* net, void* workspace, const char* name,
                            const float** ptr, int64_t* rows, int* channels);

/* Global multi-head self-attention (vit_attn.hip): qkv [batch tokens][3 hidden] split as
 * (qkv, head, d), scale d^-0.5, softmax over all tokens of the sample; out [batch tokens]
 * [hidden], lse [batch][heads][tokens].  hidden / heads in {16, 32, 64}, tokens <= 512,
 * else SPFF_EINVAL.  The backward writes all of dqkv; ws >= spff_vit_attn_ws_bytes. */
size_t spff_vit_attn_ws_bytes(int batch, int tokens, int heads);
int spff_vit_attn_fwd(const float* qkv, int batch, int tokens, int hidden, int heads, float* out,
                      float* lse, void* stream);
int spff_vit_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                      int batch, int tokens, int hidden, int heads, float* dqkv, void* ws,
                      void* stream);
/* ATen upsample_trilinear3d (align_corners=False, output size given) on channel-last rows
 * x [B][din][hin][win][C] -> y [B][dout][hout][wout][C], and its adjoint dy -> dx (gather
 * form, fixed order) */
int spff_resize3d_fwd(const float* x, float* y, int batch, int channels, int din, int hin,
                      int win, int dout, int hout, int wout, void* stream);
int spff_resize3d_bwd(const float* dy, float* dx, int batch, int channels, int din, int hin,
                      int win, int dout, int hout, int wout, void* stream);

/* ------------------------------------------------------------------------
 * Training data path on the device (oracle/data_oracle.py).
 * ------------------------------------------------------------------------ */
/* label map of the ellipse ROIs (x0, y0, w0, h0, label) [nroi][5] (device int32), later
 * ROIs overwriting earlier ones, replicated over `frames`: labels [frames][H][W] int64.
 * Replaces the ROI loop of create_image_and_labels_for_dataset (helpers.py:125-129, 199-204). */
int spff_rasterize_ellipses(const int* rois, int nroi, int frames, int height, int width,
                            int64_t* labels, void* stream);
/* [n][hin][win] -> [n][hout][wout] antialiased bilinear (align_corners=False), PyTorch's
 * weights: TF.resize(t, (H, W)) of helpers.py:196.  tmp >= n*hin*wout floats. */
int spff_resize_bilinear_aa(const float* in, int n, int hin, int win, float* out, int hout,
                            int wout, float* tmp, void* stream);
/* TrainGridAug.__call__ (datasets.py:158-209) on a batch x [B][F][H][W] (+ labels y, may be
 * NULL): per sample, prm[8] = {flip_w, flip_h, rot_k, jitter_on, scale, shift, noise_cap
 * (0: no noise), stamp} and maps[H + W] = source row / column of the stripe shuffle in the
 * rotated frame (device arrays; the random draws are the caller's).  xo / yo [B][F][Ho][Wo].
 * ws >= spff_grid_aug_ws_bytes(B). */
size_t spff_grid_aug_ws_bytes(int batch);
int spff_grid_aug(const float* x, const int64_t* y, int batch, int frames, int height, int width,
                  const int* maps, const float* prm, uint64_t seed, float* xo, int64_t* yo,
                  void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPFF_H_ */
