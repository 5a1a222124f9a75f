/*
 * kd6d.h -- C ABI of libkd6d.so, the MI355X (gfx950) implementation of the
 * teacher->student KD training step of GUOShuxuan/kd-6d-pose-adlp.
 *
 * The reference has no FFI layer (it is 100 % Python/PyTorch); its boundary is
 * the Python call surface of train_kd.py:94-140 -> models/model_kd.py:55-95 ->
 * losses/kd_loss.py:111-160.  Each entry point below names the reference
 * op group (file:line) whose arithmetic it replaces.  The Python host
 * (kd-6d-pose-adlp_amd/kd6d) binds these with ctypes; INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (kd6d_last_error());
 *   - all pointers are DEVICE pointers owned by the caller (PyTorch
 *     allocations) unless the name ends in _host; nothing is allocated or
 *     freed here and no call synchronises the device;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - activations are NHWC ("rows" = pixels, channels contiguous); a tensor
 *     may hold several pyramid levels back to back ("segments");
 *   - dtype: KD6D_BF16 (bf16 storage, fp32 accumulate on MFMA 16x16x32) or
 *     KD6D_F32 (fp32 storage, exact-fp32 MFMA 16x16x4).
 */
#ifndef KD6D_H
#define KD6D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KD6D_ABI_VERSION 11

enum { KD6D_BF16 = 0, KD6D_F32 = 1 };
enum { KD6D_ACT_NONE = 0, KD6D_ACT_LEAKY = 1, KD6D_ACT_RELU = 2 };
enum {
  KD6D_OK = 0,
  KD6D_ERR_ARG = -1,
  KD6D_ERR_LAUNCH = -2,
  KD6D_ERR_UNSUPPORTED = -3
};

#define KD6D_MAX_SEG 5

/* One pyramid level of a (possibly multi-level) convolution.
 * in_*  : input feature map grid,  out_* : output grid (forward sense).
 * row0  : index of the level's first pixel row inside the packed tensor. */
typedef struct kd6d_seg {
  int32_t in_h, in_w;
  int32_t out_h, out_w;
  int32_t in_row0;
  int32_t out_row0;
} kd6d_seg;

/* Forward-sense geometry of a conv layer; the same struct drives fwd, dgrad
 * and wgrad.  cin/cout are the STORED channel counts (multiples of 8). */
typedef struct kd6d_conv_geom {
  int32_t nseg;
  int32_t batch;
  int32_t cin, cout;
  int32_t ksize, stride, pad;
  int32_t reserved;
  kd6d_seg seg[KD6D_MAX_SEG];
} kd6d_conv_geom;

const char* kd6d_last_error(void);
int kd6d_abi_version(void);

/* ---- reproducible reductions (ABI v8) -------------------------------------------------------------------------
 * Every sum this library forms ACROSS workgroups -- normalisation statistics, the sums of the normalisation
 * backwards, weight / bias / scale gradients, loss values, the gradient norm -- is accumulated with 64-bit INTEGER
 * atomics on a fixed-point image of the fp32 addends (csrc/kd6d_det.h), never with floating-point atomics: integer
 * addition is associative, so two executions of the same launch sequence on the same inputs give BITWISE identical
 * results whatever order the hardware retires the atomics in (the reference's CPU step is deterministic too:
 * train_kd.py:137-140 is one single-threaded backward).
 *   kd6d_acc: one accumulator, two words; value = hi * 2^(47-E) + lo * 2^-E with E = KD6D_ACC_ACT for statistics of
 *   activations and loss values, KD6D_ACC_GRAD for everything summed in the reverse sweep.  Zero-initialised by the
 *   caller (the engine zeroes its whole statistics arena once per step), only ever added to; a non-finite addend
 *   poisons it (the value reads as NaN).  Arrays of kd6d_acc are INTERLEAVED {lo, hi} per element.
 *   Small gradient outputs (dbias of kd6d_conv2d_wgrad, dgamma / dbeta of kd6d_gn_relu_bwd, dseg_scale of
 *   kd6d_loss_backward) use the PLANAR layout instead: `int64_t* acc` + `acc_hi_stride`, word lo of element i at
 *   acc[i], word hi at acc[i + acc_hi_stride].  The engine keeps ONE such accumulator image of its flat gradient bucket
 *   (lo plane then hi plane).  Per-layer WEIGHT gradients use no atomics at all: every pixel split of the launch
 *   stores its partial dW image into a caller-owned slab (plain stores, 4-5x the byte rate of atomic adds) and the
 *   splits are added in a fixed order.  kd6d_grad_acc_resolve turns both kinds into fp32 gradients, one launch at the
 *   end of the reverse sweep.
 * kd6d_acc_read: out[i] (=, or += when accumulate != 0) value(acc[i]) for n interleaved accumulators of class
 * `kind`; clear != 0 zeroes them afterwards.  kd6d_grad_acc_resolve: desc_dev holds n_regions int64 quintuples
 * {first element, element count, first workgroup, parts, slab address}, regions in ascending workgroup order,
 * total_blocks workgroups of 1024 elements each.  parts == 0: grads[e] += value(planar accumulator of element e, class
 * KD6D_ACC_GRAD), accumulator cleared.  parts >= 1: grads[first + i] += the sum over the `parts` partial images
 * slab[part][i] of `count` floats each (what kd6d_conv2d_wgrad wrote), in a fixed association (fp32 throughout): PG =
 * kd6d_grad_acc_resolve_part_groups(parts) groups; group g owns parts g, g + PG, g + 2 PG, ... and keeps FOUR running
 * sums t_0 .. t_3 that start at 0, t_k adding parts g + k PG, g + (k + 4) PG, g + (k + 8) PG, ... in that order; the
 * group's sum is (t_0 + t_1) + (t_2 + t_3); the PG group sums are added in g order and that total is added to grads.
 * (Up to three parts per group this equals adding them one after the other; beyond, it does not.)  PG is 1 for parts
 * <= 16 and doubles at 32, 64, 128 and 256 parts, 32 at most.  tests/optim_ref.py: slab_sum is this sentence in numpy.
 * Workgroups per region: ceil(count / 1024) for parts == 0, ceil(count / (1024 / PG)) otherwise. */
typedef struct kd6d_acc { int64_t lo, hi; } kd6d_acc;
/* Workspace of a launch that reduces to ONE fp32 scalar (kd6d_focal_fwd, kd6d_student_points' loss_reg):
 * 32 bytes, pre-zeroed; the launch's LAST workgroup converts the fixed-point total and WRITES the scalar (the running
 * total if the workspace is reused without zeroing -- the "+=" of earlier ABI versions); arrivals is left at 0. */
typedef struct kd6d_scalar_ws { int64_t lo, hi; uint32_t arrivals; uint32_t reserved[3]; } kd6d_scalar_ws;
#define KD6D_ACC_ACT 32
#define KD6D_ACC_GRAD 52
int kd6d_acc_read(kd6d_acc* acc, int64_t n, int kind, float* out, int accumulate, int clear, void* stream);
int kd6d_grad_acc_resolve_part_groups(int parts);
int kd6d_grad_acc_resolve(const int64_t* desc_dev, int n_regions, int total_blocks, int64_t* acc,
                          int64_t acc_hi_stride, float* grads, void* stream);

/* Pair bracket: between _begin and _end, convolutions that resolve to the 3x3 "halo patch" kernel (forward or
 * data gradient) are recorded instead of launched; _end issues two recorded launches of the same kernel variant,
 * geometry and stream as ONE launch (workgroups of both convolutions in one grid), anything else one by one, in
 * call order.  For two independent convolutions of identical shape that each fill only part of the device -- the
 * cls and the pose tower layer of the head (models/model.py:438-451).  Everything else called inside the bracket
 * launches immediately; the recorded convolutions run at _end, so nothing inside the bracket may depend on them.
 * Thread-local; not nestable. */
int kd6d_conv2d_pair_begin(void);
int kd6d_conv2d_pair_end(void);
int kd6d_conv2d_pair_pending(void);   /* launches recorded so far in the open bracket (0 outside one) */

/* ---- convolution: replaces torch conv2d inside backbone/common.py:316-324
 * (ConvBlock), models/model.py:64-83,97-103 (FPN) and :438-451 (PoseHead).
 * Implicit GEMM on MFMA, weights KRSC: w[cout][ky][kx][cin].
 *   y = act((conv(x) * ch_scale[c] + ch_shift[c]) * seg_scale[level]) + residual
 * ch_scale/ch_shift/seg_scale/residual may be NULL.  out_f32 != 0 writes fp32
 * regardless of dtype.
 * stats (optional, caller-zeroed accumulators, class KD6D_ACC_ACT): statistics of the stored y accumulated by the
 * epilogue, so that the normalisation that follows needs no separate reduction pass:
 *   stats_groups == 0: {sum[cout], sumsq[cout]}           (BatchNorm batch statistics, = kd6d_colstats)
 *   stats_groups  > 0: {sum, sumsq} per (level, image, group), the layout kd6d_gn_relu_fwd consumes.
 *     Refused (KD6D_ERR_UNSUPPORTED / invalid argument, nothing launched): a pixel tile that spans more (level, image)
 *     keys than the kernel's LDS table holds (1 x 1 levels at a batch above ~60), and a level of H * W % 16 != 0 unless
 *     cout / 4 (cout / 8 for a bf16 y) divides 256 (conv_plan.h: stats_table_fits, stats_followup_ok).
 * workspace (optional device scratch, any contents): lets layers with few output tiles and a long K run
 * split-K (fp32 partial slabs + a finalize launch); without it they run as one pass. */
int kd6d_conv2d_fwd(const kd6d_conv_geom* g, int dtype, const void* x,
                    const void* w, void* y, const float* ch_scale,
                    const float* ch_shift, int act, const void* residual,
                    const float* seg_scale, int out_f32, kd6d_acc* stats, int stats_groups,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* Convolution (+ bias) with the normalisation and activation that follow it fused into its epilogue: one launch
 * instead of conv -> statistics -> normalise, and the fp32 pre-normalisation tensor is not re-read (eval-mode callers
 * do not even store it).  Replaces, of the reference: models/model.py:395-417,438-451 (tower Conv2d -> GroupNorm(32) ->
 * ReLU) and backbone/common.py:316-324 in train mode (Conv2d -> BatchNorm2d(batch statistics) -> LeakyReLU(0.1)).
 * The workgroups of the launch exchange their partial statistics through device-scope atomics and wait for the ones
 * they need at an in-kernel barrier (GroupNorm: the tiles of the same (level, image); BatchNorm: the whole launch);
 * every wait is bounded and counted by kd6d_barrier_timeouts().
 *   kind      KD6D_NORM_GROUP | KD6D_NORM_BATCH;  groups: GroupNorm groups (4 or 8 channels per group)
 *   y         (rows_out, cout) in `dtype`: act(norm(conv(x) + bias))
 *   raw_out   optional (rows_out, cout) fp32: conv(x) + bias, what the backward pass of the normalisation reads
 *   stats     pre-zeroed accumulators: GROUP nseg*batch*groups*2 (the layout kd6d_gn_relu_bwd consumes);
 *             BATCH KD6D_BN_FUSED_REPLICAS*2*cout (private layout)
 *   counters  pre-zeroed 32-bit words: GROUP nseg*batch*KD6D_NORM_MAX_CTILES; BATCH KD6D_BARRIER_WORDS
 *   BATCH only: momentum, running_mean / running_var (updated in place), save_mean / save_invstd (outputs for
 *   kd6d_bn_train_bwd); all optional except the save pair.
 * kd6d_conv2d_fwd_norm_fusable() tells whether this geometry takes the fused path (1) or not (0: the kernel the layer
 * would run on has no fused epilogue, or -- BatchNorm -- its workgroups cannot all be resident at once on half of the
 * device; call kd6d_conv2d_fwd + kd6d_bn_train_fwd / kd6d_gn_relu_fwd instead).  kd6d_conv2d_fwd_norm returns
 * KD6D_ERR_UNSUPPORTED in that case.  Option "conv.fuse_norm" = 0 makes every geometry report 0. */
#define KD6D_NORM_GROUP 1
#define KD6D_NORM_BATCH 2
#define KD6D_BN_FUSED_REPLICAS 8
#define KD6D_NORM_MAX_CTILES 8
typedef struct kd6d_conv_norm {
  int32_t kind;
  int32_t groups;
  int32_t act;
  float eps;
  float momentum;
  const float* gamma;
  const float* beta;
  void* y;
  kd6d_acc* stats;
  unsigned int* counters;
  float* running_mean;
  float* running_var;
  float* save_mean;
  float* save_invstd;
} kd6d_conv_norm;
int kd6d_conv2d_fwd_norm_fusable(const kd6d_conv_geom* g, int dtype, int kind, int groups);
int kd6d_conv2d_fwd_norm(const kd6d_conv_geom* g, int dtype, const void* x, const void* w, void* raw_out,
                         const float* bias, const kd6d_conv_norm* norm, void* stream);

/* The convolution of a train-mode ConvBlock (backbone/common.py:316-324: Conv2d(no bias) -> BatchNorm2d -> LeakyReLU):
 * y_raw (rows_out, cout) fp32 = conv(input, w), with the batch sums of y_raw accumulated into `stats` (pre-zeroed,
 * stats_replicas rows of {sum[cout], sumsq[cout]}; workgroup b adds to row b % stats_replicas, consumers add the rows).
 * The input is either x (rows_in, cin) in `dtype` (bn == NULL), or -- bn != NULL -- the PREVIOUS block's fp32 conv
 * output, whose BatchNorm + activation is applied while it is loaded (no separate normalise launch, no wait inside the
 * kernel): bn->sums are that block's `stats` rows, save_mean / save_invstd (for kd6d_bn_train_bwd of that block) and the
 * running statistics are written by this launch, and z_out (optional, (rows_in, cin) in `dtype`) receives the
 * activation the weight gradient of THIS convolution reads.  bn != NULL needs a 1x1 or 3x3 stride-1 'same' convolution. */
typedef struct kd6d_bn_in {
  const kd6d_acc* sums;
  int32_t replicas;
  int32_t act;
  float eps;
  float momentum;
  const float* gamma;
  const float* beta;
  float* running_mean;
  float* running_var;
  float* save_mean;
  float* save_invstd;
} kd6d_bn_in;
int kd6d_conv2d_fwd_block(const kd6d_conv_geom* g, int dtype, const void* x, const kd6d_bn_in* bn, void* z_out,
                          const void* w, float* y_raw, kd6d_acc* stats, int stats_replicas, void* stream);

/* dx (+)= conv_transpose(dy, w).  wt is the dgrad packing wt[cin][ky][kx][cout]
 * produced by kd6d_pack_dgrad_weights.  accumulate != 0 adds into dx. */
int kd6d_conv2d_dgrad(const kd6d_conv_geom* g, int dtype, const void* dy,
                      const void* wt, void* dx, int accumulate, void* stream);

/* Weight gradient dw[cout][ky][kx][cin] = sum_pixels dy (x) x as PARTIAL IMAGES: the pixel axis is split over
 * workgroups and split s stores its partial dW, all cout*k*k*cin floats, at dw_slab + s * cout*k*k*cin (plain stores;
 * every element of every part is written).  kd6d_conv2d_wgrad_parts() tells how many parts the launch writes for a
 * geometry, dtype, bias flag and cu_budget (>= 1; a deterministic function of its arguments and the device);
 * slab_floats is checked against it.  The caller adds the parts in a fixed association (kd6d_grad_acc_resolve;
 * "reproducible reductions").  dbias_acc (optional): += sum_pixels dy, the bias gradient of the same layer, taken from the dY tiles the
 * kernel stages anyway, into PLANAR accumulators (class KD6D_ACC_GRAD, stride acc_hi_stride).
 * cu_budget: how many compute units this launch should aim to fill (0 = the whole device): a caller that keeps k
 * weight gradients in flight on k streams passes CUs/k -- same k-loop work, 1/k of the partial images. */
int kd6d_conv2d_wgrad_parts(const kd6d_conv_geom* g, int dtype, int with_bias, int cu_budget);
int kd6d_conv2d_wgrad(const kd6d_conv_geom* g, int dtype, const void* x, const void* dy, float* dw_slab,
                      int64_t slab_floats, int64_t* dbias_acc, int64_t acc_hi_stride, int cu_budget, void* stream);

/* Several weight gradients behind ONE point of the caller's stream: every call is exactly a kd6d_conv2d_wgrad call (same
 * arguments, same checks, same plan for its cu_budget, same parts, same bits in its slab and bias accumulators).  The
 * bf16 calls of the transposing kernel family go out as list launches of up to KD6D_WGRAD_LIST_MAX calls each -- one
 * kernel whose workgroups are the calls' own grids back to back, so the calls run side by side without a stream each;
 * n may exceed KD6D_WGRAD_LIST_MAX: consecutive lists, call order kept.  A call the list kernel does not take (the
 * narrow-layer family, fp32) is launched on its own directly behind the list that reached it. */
#define KD6D_WGRAD_LIST_MAX 4
typedef struct kd6d_wgrad_call {
  const kd6d_conv_geom* g;
  int dtype;
  const void* x;
  const void* dy;
  float* dw_slab;
  int64_t slab_floats;
  int64_t* dbias_acc;
  int64_t acc_hi_stride;
  int cu_budget;
} kd6d_wgrad_call;
int kd6d_conv2d_wgrad_list(const kd6d_wgrad_call* calls, int n, void* stream);

/* wt[cin][ky][kx][cout] <- w[cout][ky][kx][cin] for n_layers layers in one
 * launch.  desc_dev: int32[n_layers*6] = {w_off, wt_off, cout, cin, ksize,
 * first_block}; offsets in elements of the w / wt base arrays. */
/* Grouped weight gradient (bf16): the dW (+ bias gradients) of several layers as ONE launch pair -- a work list of
 * (layer, 128- or 16-channel row block of dW, kernel row ky, 128 input channels, pixel range) items sized so that
 * `n_workgroups` workgroups run equally long, each leaving an fp32 partial tile in `slab`, and a reduction launch
 * that adds the partial tiles into dw / dbias (+=, plain stores: bitwise reproducible).  Takes layers with
 * stride 1, 1x1 or 3x3 "same" padding, cin %% 128 == 0 (kd6d_wgrad_group_supported); anything else stays on
 * kd6d_conv2d_wgrad.  kd6d_wgrad_group_plan builds the work list in HOST memory (plan_host = NULL: size query);
 * the caller copies it to the device once and replays kd6d_wgrad_group_launch with it (the plan holds the items'
 * device pointers).  info[0] = workgroups, info[1] = reduction blocks, info[2] + (info[3] << 31) = slab floats. */
typedef struct kd6d_wgrad_item {
  kd6d_conv_geom geom;
  const void* x;      /* input activations (rows_in, cin), bf16 */
  const void* dy;     /* output gradient (rows_out, cout), bf16 */
  float* dw;          /* (cout, k, k, cin) fp32, accumulated into */
  float* dbias;       /* (cout) fp32 or NULL */
} kd6d_wgrad_item;
int kd6d_wgrad_group_supported(const kd6d_conv_geom* g, int dtype);
int64_t kd6d_wgrad_group_plan(const kd6d_wgrad_item* items, int n_items, int dtype, int n_workgroups, void* plan_host,
                              int64_t plan_capacity, int32_t* info);
int kd6d_wgrad_group_launch(const void* plan_dev, int n_workgroups, int n_reduce_blocks, float* slab_dev, void* stream);

int kd6d_pack_dgrad_weights(int dtype, const void* w_base, void* wt_base,
                            const int32_t* desc_dev, int n_layers,
                            int total_blocks, void* stream);


/* Pyramid description for the loss-side kernels: level l has an h[l] x w[l] grid of cells,
 * anchor stride / size as in configs/ape.yaml:3-4; rows are packed level-major, then image. */
typedef struct kd6d_levels {
  int32_t n;
  int32_t batch;
  int32_t h[KD6D_MAX_SEG];
  int32_t w[KD6D_MAX_SEG];
  float anchor_stride[KD6D_MAX_SEG];
  float anchor_size[KD6D_MAX_SEG];   /* all 5 entries are read by teacher_select (postprocess_kd.py:143) */
} kd6d_levels;

#define KD6D_MAX_GT 4   /* instances per image handled by the assignment kernel */

int kd6d_device_cu_count(void);

/* Kernel-selection options.  The dispatch rules inside the library are measured defaults; the parity tests and the
 * per-layer benches pin one kernel family for a call through this table (per context, see kd6d_ctx below; set between
 * launches by the launching thread).  The product path sets none of them.  Names and values:
 *   conv.halo      -1 auto | 0 off | 1 256x128, 2 128x128 (4 waves), 3 128x128, 4 128x64, 5 128x32, 6 192x128, 9 64x64,
 *                  11-15 the two-workgroups-per-CU twins (maps <= 32 wide): 128x128 on 4 / 8 waves, 128x64, 64x64, 128x32
 *   conv.halo_pairing  1 | 0 keep the one-workgroup-per-CU halo tiles on maps <= 32 wide
 *   conv.halo_wide     1 | 0 maps 65 ... 80 wide (the 60 x 80 level of 480 x 640 full frames) stay off the halo-patch kernel
 *   conv.smallc    -1 auto | 0 off | 1 the resident-patch kernel also below 2^17 pixels
 *   conv.splitk    -1 auto | 0 off | tile*100 + splits (tile 1 = 128x64, 2 = 64x64)
 *   conv.tile      -1 auto | 0 register-staged kernel | 1 128x128, 2 128x64, 3 64x64 (LDS-DMA kernel)
 *   wgrad.small    -1 auto | 0 off | 1 the narrow-layer weight-gradient kernel at any size
 *   bn.onepass      1 | 0 two-launch BatchNorm backward     bn.onepass_max  largest x in 16-B granules (65536)
 *   gn.onepass      1 | 0 two-launch GroupNorm backward     sinkhorn.lanes  1 | 0 general path for every point set
 *   conv.fuse_norm  bit 0: GroupNorm, bit 1: BatchNorm geometries may take kd6d_conv2d_fwd_norm (3 | 0: fusable() = 0)
 *   sinkhorn.dense_mfma  dense OT, D = 16: 1 softmin passes on the matrix pipe (inner products at fp32 accuracy from
 *                  bf16 pieces; the gradient-carrying pass's weighted sums as a second product) while
 *                  eps >= 1.5e-4 diameter^2 | 0 never | 2 every pass (error studies) | 3 as 1, the gradient-carrying
 *                  softmins in the difference form
 *   conv.smallc_wmax  widest map the resident-patch kernel (3x3, 8-32 input channels) takes: 640 | 256 (rounds 1-2)
 *   sinkhorn.dense_screen  dense OT, D = 16, passes with eps below the matrix-pipe rule: 1 approximate exponents on the
 *                  matrix pipe screen the pairs, those within 40 (+ the error bound) of a row's running maximum are
 *                  evaluated exactly in the difference form | 0 every pair in the difference form
 *   sinkhorn.dense_rows  rows per workgroup of the dense matrix-pipe softmins (each workgroup streams all columns through
 *                  LDS): -1 = 128 from 8192 rows up, 64 below | 64 | 128
 *   stem.fused      1 | 0 kd6d_bn_pool_bwd_wgrad_parts reports 0: the apply pass and the weight gradient stay two launches
 *   wgrad.list      the largest number of per-layer weight gradients a reverse sweep collects before it forks them onto a
 *                  side stream as one kd6d_conv2d_wgrad_list call; 0 or 1: a fork per layer (read by the caller's sweep,
 *                  kd6d/engine.py; the library's launches do not depend on it)
 * Unknown names return KD6D_ERR_ARG. */
/* Context: the library's mutable state -- the option table, the pair bracket of kd6d_conv2d_pair_begin/_end and the
 * counter of in-kernel barrier waits that gave up -- lives in a kd6d_ctx.  Every entry point of this header acts on the
 * CALLING THREAD'S CURRENT context: the one set with kd6d_ctx_make_current(), else the process-wide default context
 * (what a host that never creates one gets; it cannot be destroyed).  Two models in one process that must not share
 * kernel-selection state each create a context and make it current around their calls (or use the kd6d_ctx_* forms,
 * which take the context explicitly; ctx == NULL means "the current one").  Contexts are not thread-safe: one thread
 * at a time per context.  The RCCL communicator (kd6d_comm) is its own handle and is passed explicitly already. */
typedef struct kd6d_ctx kd6d_ctx;
int kd6d_ctx_create(kd6d_ctx** out);               /* options at their defaults, no bracket open, counter 0; needs a device */
int kd6d_ctx_destroy(kd6d_ctx* ctx);
int kd6d_ctx_make_current(kd6d_ctx* ctx);          /* NULL: back to the default context */
kd6d_ctx* kd6d_ctx_current(void);
int kd6d_ctx_set_option(kd6d_ctx* ctx, const char* name, long long value);
int kd6d_ctx_get_option(kd6d_ctx* ctx, const char* name, long long* value);
int kd6d_ctx_reset_options(kd6d_ctx* ctx);
int kd6d_ctx_barrier_timeouts(kd6d_ctx* ctx);      /* of launches issued under that context */
int kd6d_ctx_conv2d_pair_begin(kd6d_ctx* ctx);
int kd6d_ctx_conv2d_pair_end(kd6d_ctx* ctx);
int kd6d_ctx_conv2d_pair_pending(kd6d_ctx* ctx);

int kd6d_set_option(const char* name, long long value);
int kd6d_get_option(const char* name, long long* value);
int kd6d_reset_options(void);

/* Step prologue: zero up to KD6D_MAX_ZERO device regions (16-B aligned, sizes multiples of 4 bytes; a size of 0
 * skips the entry) and add 1 to each of n_counter (<= 256) int64 counters, in ONE launch.  Stands where the
 * reference's step has optimizer.zero_grad() (train_kd.py:104) and BatchNorm's num_batches_tracked += 1; here the
 * same launch also clears the statistics arena, the dense head gradient and the loss-side slot arrays. */
#define KD6D_MAX_ZERO 8
typedef struct kd6d_zero_list {
  int32_t n;
  int32_t pad_;
  void* ptr[KD6D_MAX_ZERO];
  int64_t bytes[KD6D_MAX_ZERO];
} kd6d_zero_list;
int kd6d_zero_regions(const kd6d_zero_list* list, long long* counter, int n_counter, void* stream);

/* n uniform [0, 1) fp32 keys for kd6d_ssc_assign (the random in-mask cells of losses/loss.py:224-228), generated on
 * the device from (seed, *counter, index): *counter is a device int64 the caller advances every step (the step
 * prologue's counters), so a captured launch draws new keys at every replay.  Not torch's generator: the sequence is
 * reproducible from the seed and the step count alone. */
int kd6d_uniform_keys(float* out, int64_t n, const long long* counter, unsigned long long seed, void* stream);

/* Timing aid: stores the device's 100-MHz wall clock into *slot when the launch executes on `stream`
 * (phase boundaries inside a replayed hipGraph; tools/step_timeline.py). */
int kd6d_mark(unsigned long long* slot, void* stream);

/* ---- normalisation / pooling (HBM-bound, 16-B granules) ------------------------------------
 * BatchNorm2d(train)+LeakyReLU of ConvBlock (backbone/common.py:316-324): batch statistics by
 * kd6d_colstats (per-channel sum / sum of squares into pre-zeroed accumulators, class KD6D_ACC_ACT), then
 * kd6d_bn_train_fwd normalises, updates running stats (momentum 0.1, unbiased var) and saves
 * mean / invstd for the backward pair.  x_f32 != 0: the pre-normalisation tensor x is fp32 while
 * activations/gradients are `dtype` (keeps (x - mean) free of bf16 cancellation error).
 * Backward pair: sum_dy / sum_dy_xhat are `replicas` (1..64) rows of C accumulators (KD6D_ACC_GRAD) each, pre-zeroed; the
 * reduction's workgroups spread their per-channel atomics over the rows (same-address atomics retire
 * serially, ~27 ns each, and this kernel needs hundreds of workgroups), the apply kernel sums the rows. */
int kd6d_colstats(int dtype, const void* x, int64_t rows, int C, kd6d_acc* sum, kd6d_acc* sumsq, void* stream);
int kd6d_bn_train_fwd(int dtype, int x_f32, const void* x, void* y, int64_t rows, int C, const kd6d_acc* sum,
                      const kd6d_acc* sumsq, const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                      int act, void* stream);
/* kd6d_bn_train_fwd plus a residual added after the activation: y = act(bn(x)) + residual, summed in fp32 and rounded
 * once to `dtype` (the DarkUnit of backbone/darknet53.py:54-58 in training mode).  residual has y's dtype and layout
 * (rows, C); statistics, running buffers and save_mean / save_invstd as in kd6d_bn_train_fwd. */
int kd6d_bn_train_fwd_res(int dtype, int x_f32, const void* x, const void* residual, void* y, int64_t rows, int C,
                          const kd6d_acc* sum, const kd6d_acc* sumsq, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean, float* running_var, float* save_mean,
                          float* save_invstd, int act, void* stream);
int kd6d_bn_train_bwd_reduce(int dtype, int x_f32, const void* x, const void* dz, int64_t rows, int C,
                             const float* mean, const float* invstd, const float* gamma, const float* beta,
                             int act, kd6d_acc* sum_dy, kd6d_acc* sum_dy_xhat, int replicas, void* stream);
int kd6d_bn_train_bwd_apply(int dtype, int x_f32, const void* x, const void* dz, void* dx, int64_t rows, int C,
                            const float* mean, const float* invstd, const float* gamma, const float* beta,
                            int act, const kd6d_acc* sum_dy, const kd6d_acc* sum_dy_xhat, float* dgamma,
                            float* dbeta, int replicas, void* stream);

/* BN(train) + activation + MaxPool2d(2,2) in one pass: the last ConvBlock of a darknet-tiny stage and the pool
 * behind it (backbone/darknet.py:94-97).  x: (B,H,W,C) conv output; y / dy: the POOLED tensors (B,H/2,W/2,C);
 * dx: gradient of x.  The un-pooled activation and its gradient are never stored: the backward re-derives each
 * 2x2 window from x with the forward's arithmetic and rounding and sends dy to the first maximum in row-major
 * window order (MaxPool2d's rule).  Statistics, saved mean / invstd, replicas and workspaces as in the unpooled
 * entry points above; kd6d_bn_pool_train_bwd runs the reduction and the apply pass. */
int kd6d_bn_pool_train_fwd(int dtype, int x_f32, const void* x, void* y, int B, int H, int W, int C,
                           const kd6d_acc* sum, const kd6d_acc* sumsq, const float* gamma, const float* beta, float eps,
                           float momentum, float* running_mean, float* running_var, float* save_mean,
                           float* save_invstd, int act, void* stream);
int kd6d_bn_pool_train_bwd(int dtype, int x_f32, const void* x, const void* dy, void* dx, int B, int H, int W,
                           int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           int act, kd6d_acc* sum_dy, kd6d_acc* sum_dy_xhat, unsigned int* counter, float* dgamma,
                           float* dbeta, int replicas, void* stream);

/* A pooled block whose INPUT needs no gradient (the first block of a network: its input is the image): the gradient
 * of the convolution output is read by the weight gradient alone, so it is never stored.
 * kd6d_bn_pool_train_bwd_reduce: the reduction pass of kd6d_bn_pool_train_bwd alone -- the two sums, into `replicas`
 * rows.  kd6d_bn_pool_bwd_wgrad: the apply pass and the weight gradient of the convolution in front as ONE launch.  It
 * re-derives the windows from raw (fp32 convolution output, (B,H,W,cout)) exactly as kd6d_bn_pool_train_bwd does, forms
 * the gradient of raw in registers, rounds it to bf16 as the stored tensor was, and contracts it with x (the block's
 * input, (B,H,W,cin) bf16) in fp32: the products of the separate path, another association of their sum.  dgamma /
 * dbeta (optional): += the totals, one writer per channel.  The weight gradient arrives as partial images in dw_slab,
 * laid out as kd6d_conv2d_wgrad's (dw_slab + s * cout*9*cin, every element of every part written, no atomics: two
 * executions give the same bits); kd6d_bn_pool_bwd_wgrad_parts() tells how many for a geometry, dtype and cu_budget
 * -- or 0 when the geometry is not taken: 3x3 / stride 1 / pad 1, cin = 8, cout = 8 or 16, one level packed from row
 * 0 with even H and W <= 256, bf16 (csrc/conv_plan.h, stem_bwd_rule); option stem.fused = 0 makes it report 0 for
 * every geometry.  cu_budget as in kd6d_conv2d_wgrad. */
int kd6d_bn_pool_train_bwd_reduce(int dtype, int x_f32, const void* x, const void* dy, int B, int H, int W, int C,
                                  const float* mean, const float* invstd, const float* gamma, const float* beta,
                                  int act, kd6d_acc* sum_dy, kd6d_acc* sum_dy_xhat, int replicas, void* stream);
int kd6d_bn_pool_bwd_wgrad_parts(const kd6d_conv_geom* g, int dtype, int cu_budget);
int kd6d_bn_pool_bwd_wgrad(const kd6d_conv_geom* g, int dtype, const void* x, const float* raw, const void* dz,
                           const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                           const kd6d_acc* sum_dy, const kd6d_acc* sum_dy_xhat, int replicas, float* dgamma,
                           float* dbeta, float* dw_slab, int64_t slab_floats, int cu_budget, void* stream);

#define KD6D_BARRIER_WORDS 32
/* BN backward as ONE launch (also kd6d_bn_pool_train_bwd, and kd6d_gn_relu_bwd below): when `counter`
 * (KD6D_BARRIER_WORDS pre-zeroed 32-bit words per call, e.g. in the per-step zeroed arena beside sum_dy) is given and the tensor fits
 * the registers of one resident grid (512 workgroups x 4 granules per thread), every workgroup keeps its slice of x / dz in registers,
 * adds its partial sums, meets the others at an in-kernel barrier on `counter` and finishes dx -- one read of x
 * and dz instead of two, one launch instead of two.  By default only tensors of up to 65536 granules take it
 * (<= 128 workgroups: there the barrier is cheaper than a launch; beyond, exchanging the sums costs more than the
 * second read -- option bn.onepass_max = <granules> moves the limit).  counter == NULL, a larger tensor or
 * option bn.onepass = 0: the reduce + apply pair above.  kd6d_barrier_timeouts(): number of barrier waits that gave up (must stay 0). */
int kd6d_bn_train_bwd(int dtype, int x_f32, const void* x, const void* dz, void* dx, int64_t rows, int C,
                      const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                      kd6d_acc* sum_dy, kd6d_acc* sum_dy_xhat, unsigned int* counter, float* dgamma, float* dbeta,
                      int replicas, void* stream);
int kd6d_barrier_timeouts(void);

/* GroupNorm(groups)+ReLU of the PoseHead towers (models/model.py:395-417) over a multi-level
 * tensor; level_hw_host[l] = H*W of level l (HOST array).  stats: 2 accumulators (KD6D_ACC_ACT) per
 * (level, image, group) = RAW sums {sum x, sum x^2} (mean/rstd are derived by the consumers, which is
 * why the backward takes eps too); gsum_ws (backward): 2*nseg*batch*groups accumulators (KD6D_ACC_GRAD) followed by
 * nseg*batch 32-bit barrier counters -- the backward is ONE launch whose workgroups of a (level, image) meet at
 * an in-kernel barrier (see kd6d_bn_train_bwd; option gn.onepass = 0: the reduce + apply pair).
 * flags: bit 0 (KD6D_GN_STATS_READY) -- stats were already accumulated by kd6d_conv2d_fwd(..., stats,
 * groups): skip the reduction pass; bit 1 (KD6D_GN_WS_ZEROED) -- the caller zeroed stats (fwd, when not
 * ready) / gsum_ws (bwd) itself (e.g. one memset of a whole scratch arena per step): skip the memset node.
 * dgamma / dbeta (backward, optional): PLANAR gradient accumulators with stride acc_hi_stride (see "reproducible
 * reductions").  Requires C/groups >= granule/2 (a 16-B granule spans <= 2 groups).
 * kd6d_gn_relu_bwd (and _pair) accept C <= 512 only -- the kernels keep 32*C bytes of per-channel accumulators in
 * the 16 KB of LDS they are launched with; a wider tensor is refused with KD6D_ERR_ARG. */
#define KD6D_GN_STATS_READY 1
#define KD6D_GN_WS_ZEROED 2
int kd6d_gn_relu_fwd(int dtype, int x_f32, const void* x, void* y, const int32_t* level_hw_host, int nseg, int batch,
                     int C, int groups, const float* gamma, const float* beta, float eps, kd6d_acc* stats,
                     int flags, void* stream);
int kd6d_gn_relu_bwd(int dtype, int x_f32, const void* x, const void* dz, void* dx, const int32_t* level_hw_host,
                     int nseg, int batch, int C, int groups, const float* gamma, const float* beta, float eps,
                     const kd6d_acc* stats, kd6d_acc* gsum_ws, int64_t* dgamma_acc, int64_t* dbeta_acc,
                     int64_t acc_hi_stride, int flags, void* stream);
/* Two GroupNorm+ReLU backwards of identical geometry (the cls and the pose tower layer of PoseHead,
 * models/model.py:438-451) as ONE launch of the in-kernel-barrier form: alone each is 170 four-wave workgroups on
 * 256 CUs.  Same arguments as kd6d_gn_relu_bwd, the per-tensor ones in an item each; falls back to two launches
 * where the one-launch form does not apply (gn.onepass = 0, too few resident workgroups). */
typedef struct kd6d_gn_item {
  const void* x;
  const void* dz;
  void* dx;
  const float* gamma;
  const float* beta;
  const kd6d_acc* stats;
  kd6d_acc* gsum_ws;
  int64_t* dgamma;      /* planar gradient accumulators (acc_hi_stride of the call) */
  int64_t* dbeta;
} kd6d_gn_item;
int kd6d_gn_relu_bwd_pair(int dtype, int x_f32, const kd6d_gn_item* a, const kd6d_gn_item* b,
                          const int32_t* level_hw_host, int nseg, int batch, int C, int groups, float eps,
                          int64_t acc_hi_stride, int flags, void* stream);

/* MaxPool2d(2,2) (backbone/darknet.py:94-97), nearest-x2 upsample + add (models/model.py:75-78)
 * and its adjoint, ReLU / ReLU-backward / add (mode 0/1/2), NCHW fp32 image -> padded NHWC. */
int kd6d_maxpool2_fwd(int dtype, const void* x, void* y, int B, int H, int W, int C, void* stream);
int kd6d_maxpool2_bwd(int dtype, const void* x, const void* dy, void* dx, int B, int H, int W, int C,
                      int accumulate, void* stream);
int kd6d_upsample2_add(int dtype, const void* fine, const void* coarse, void* out, int B, int H, int W,
                       int C, void* stream);
int kd6d_sumpool2(int dtype, const void* dfine, void* dcoarse, int B, int H, int W, int C, int accumulate,
                  void* stream);
int kd6d_eltwise(int dtype, int mode, const void* x, const void* dy, void* y, int64_t n_elems, void* stream);
int kd6d_image_to_nhwc(int dtype, const float* img_nchw, void* out, int B, int Cimg, int H, int W, int Cpad,
                       void* stream);

/* ---- optimal-transport KD loss: replaces geomloss.SamplesLoss("sinkhorn", p=2, blur, scaling,
 * reach) as called from losses/loss_libs.py:22-51 (one call per image, batch dim = 8 keypoints)
 * and its autograd.  Image b uses student points xs[(s_start[b]+i)*8+k][2] (i < s_cnt[b]) with
 * weights alpha[(..)*8+k] and teacher points/weights likewise; reach <= 0 means balanced.
 * The small-set launch contract (csrc/pointset_small.h; kd6d_kernel_div_fwd_bwd below keeps the same one): one workgroup
 *   per problem, one wave per keypoint.
 * Outputs: loss_img[b] = sum_k S_k, valid_img[b] = 1 (0 when a set is empty; -1 = set larger than
 * kd6d_sinkhorn_max_points() = 128), loss_kp (optional, n_images*8) = the eight S_k themselves (what SamplesLoss returns
 * for a batch of 8 problems), grad_xs / grad_alpha = d loss_img / d xs, alpha.
 * What is written: grad_xs / grad_alpha rows of problems with valid_img[b] <= 0, and rows that lie in no segment,
 *   are NOT written (callers that scatter or sum whole arrays zero them first, as ops.sinkhorn_div does unless it is
 *   handed out= buffers); loss_img[b] and the eight loss_kp of such problems are 0.  loss_img[b] is the fp32 sum of the
 *   eight loss_kp in keypoint order.
 *   Segments may lie in any order, with gaps; a problem's results depend on its own rows only (two launches, or
 *   the problem launched alone, agree bitwise), and permuting the keypoint axis of all inputs permutes the results.
 * Small sets: when both sets hold <= 16 points the four softmins of an update run side by side on the four 16-lane
 *   rows of a wave (option sinkhorn.lanes = 0: the general path for every size).  Both paths give bitwise the same
 *   grad_xs / grad_alpha; loss_img / loss_kp differ in the last bits (another summation order).
 * Schedule: geomloss' epsilon_schedule evaluated in double from the fp32 box diagonal of the problem's 8*(N+M)
 *   points (clamped to 1e-12); the geometric part is capped at 4096 steps, which differs from geomloss when scaling
 *   is so close to 1 that ln(diameter/blur)/ln(1/scaling) exceeds that. */
int kd6d_sinkhorn_div_fwd_bwd(const float* xs, const float* alpha, const int32_t* s_start,
                              const int32_t* s_cnt, const float* yt, const float* beta,
                              const int32_t* t_start, const int32_t* t_cnt, int n_images, float p, float blur,
                              float scaling, float reach, float* loss_img, int32_t* valid_img, float* loss_kp,
                              float* grad_xs, float* grad_alpha, void* stream);
int kd6d_sinkhorn_max_points(void);

/* ---- kernel distances (csrc/kernel_loss.hip; added under ABI 11, new symbols only): geomloss.SamplesLoss("gaussian" |
 * "laplacian" | "energy", blur) -- the kernel (MMD) losses of the reference's --gtype -- and their autograd, restated
 * from geomloss 0.2.4 kernel_samples.py (tensorized path; geomloss is absent from the reference tree: parity unpinned
 * at that boundary).  For x (N,D) with weights a and y (M,D) with weights b, the weights used as given (not
 * normalised):
 *   L = 1/2 sum_ij a_i a_j k(x_i,x_j) + 1/2 sum_ij b_i b_j k(y_i,y_j) - sum_ij a_i b_j k(x_i,y_j),
 *   r2(u,v) = sum_d (u_d - v_d)^2 from direct differences,
 *   gaussian k = exp(-r2 / (2 blur^2)); laplacian k = exp(-sqrt(max(r2 / blur^2, 1e-8))); energy k = -sqrt(max(r2, 1e-8)),
 *   dL/da_i = sum_j a_j k(x_i,x_j) - sum_j b_j k(x_i,y_j),
 *   dL/dx_i = a_i [ sum_j a_j grad1 k(x_i,x_j) - sum_j b_j grad1 k(x_i,y_j) ],
 * with grad1 k = 0 where the clamp is active (torch's clamp_min rule: the gradient passes at equality, is zero below):
 * coincident points, the diagonal included, contribute k = -1e-4 (energy) or exp(-1e-4) (laplacian) and no gradient.
 * Weights enter as values, never as logarithms: a weight of 0 is an ordinary value.  blur is ignored by the energy
 * distance and must be > 0 for the other two.
 * kd6d_kernel_div_fwd_bwd: the KD step's launch (D = 2, eight keypoint problems per segment pair), under the small-set
 *   launch contract stated at kd6d_sinkhorn_div_fwd_bwd above -- layouts, valid_img = 1 / 0 / -1 with
 *   kd6d_kernel_div_max_points() = kd6d_sinkhorn_max_points() = 128, what is and is not written, loss_img as the ordered
 *   fp32 sum of loss_kp, independence of the problems -- with L_k in the place of S_k.  n_images = 0 launches nothing.
 *   One pass over the pairs; every sum in a fixed order.
 * kd6d_kernel_dense_fwd_bwd: ONE problem, D in {2,4,8,16}, N, M >= 1 of any size (the counterpart of
 *   kd6d_sinkhorn_dense_fwd_bwd); the pair matrices are never materialised (one row per thread, column tiles staged in
 *   LDS, columns in ascending order).  workspace: kd6d_kernel_dense_workspace_floats(N, M, D) floats, any contents
 *   (one partial of L per workgroup, added in index order by a last pass).  Outputs: loss (1), grad_x (N,D),
 *   grad_alpha (N).  Two launches agree bitwise.  fp32 vector arithmetic only. */
#define KD6D_KERNEL_GAUSSIAN 0
#define KD6D_KERNEL_LAPLACIAN 1
#define KD6D_KERNEL_ENERGY 2
int kd6d_kernel_div_fwd_bwd(int kind, const float* xs, const float* alpha, const int32_t* s_start,
                            const int32_t* s_cnt, const float* yt, const float* beta, const int32_t* t_start,
                            const int32_t* t_cnt, int n_images, float blur, float* loss_img, int32_t* valid_img,
                            float* loss_kp, float* grad_xs, float* grad_alpha, void* stream);
int kd6d_kernel_div_max_points(void);
int64_t kd6d_kernel_dense_workspace_floats(int N, int M, int D);
int kd6d_kernel_dense_fwd_bwd(int kind, const float* x, const float* alpha, const float* y, const float* beta, int N,
                              int M, int D, float blur, float* workspace, int64_t workspace_floats, float* loss,
                              float* grad_x, float* grad_alpha, void* stream);

/* ---- loss-side kernels (cls logits (rows,16) fp32 [15 classes + pad], reg logits (rows,240)) --
 * kd6d_teacher_select  <- postprocess/postprocess_kd.py:22-203 (PnP gate treated as true):
 *   slot layout: image b owns slots [b*cap, b*cap + t_cnt[b]); t_kp (slots,8,2) full-frame px,
 *   t_score (slots,8) = sqrt(sigmoid), t_row = packed row of the chosen cell; t_kp_norm =
 *   t_kp / (frame_w, frame_h) and t_beta = t_score^2 are the OT inputs (loss_libs.py:8-12,
 *   kd_loss.py:82).
 * kd6d_ssc_assign      <- losses/loss.py:164-268; per-image inputs are padded to KD6D_MAX_GT
 *   instances; keys (rows) are caller-supplied uniform randoms (the n smallest in-mask keys per
 *   level are the reference's randperm(...)[:n]).  labels (rows): -1 ignore, 0 bg, c+1.
 *   Capacity: image b's positives are pos_row / pos_gt [b*cap, b*cap + pos_cnt[b]), ascending packed row, cap <= 64.
 *   An instance draws at most floor(positive_num + 0.5 * levels) cells (the per-level counts are rounded half up), so
 *   cap >= KD6D_MAX_GT * floor(positive_num + 0.5 * levels) -- 48 at the reference's positive_num = 10 -- holds every
 *   pick and the labels are the reference's.  Beyond it the result is TRUNCATED, not an error: the cap picks with the
 *   smallest packed rows are kept, pos_cnt[b] = cap, and every other pick keeps the in-mask label -1 (ignore)
 *   instead of c+1.  The Python host (kd6d.kd_losses.KDLoss) refuses configurations that could get there.
 * kd6d_focal_fwd/bwd   <- losses/loss.py:20-40 (sum reduction into *loss through loss_ws, see kd6d_scalar_ws; bwd
 *   writes ALL of dcls).
 * kd6d_student_points  <- losses/kd_loss.py:40-71,152: decoded full-frame keypoints of the
 *   positive cells (normalised by frame_w/h into xs), OT weights alpha, loss_reg (through loss_reg_ws) and its
 *   gradient w.r.t. the full-frame points.
 * kd6d_kd_mean         <- kd_loss.py:99-103.
 * kd6d_loss_backward   <- autograd of the above into dcls (+=) / dreg (positive rows only); dseg_scale_acc (optional):
 *   the gradient of PoseHead.scales, PLANAR gradient accumulators (one per level) with stride acc_hi_stride. */
int kd6d_teacher_select(const kd6d_levels* levels, const float* cls, const float* reg,
                        const float* bbox_trans, float threshold, float positive_num, float positive_lambda,
                        int cap, float frame_w, float frame_h, int32_t* t_cnt, float* t_kp, float* t_score,
                        int32_t* t_row, float* t_kp_norm, float* t_beta, void* stream);

/* Pose candidates of the evaluation path (postprocess/postprocess.py:22-121, up to the PnP solver): the
 * same per-level top-n rule as kd6d_teacher_select, run for EVERY ground-truth slot g < n_gt[b] of image b on
 * the class class_ids[b*KD6D_MAX_GT + g] (the reference keeps only labels present in target.class_ids).
 * Output block o = b*KD6D_MAX_GT + g: cnt[o] cells, kp[(o*cap + i)*16 + k*2 + {0,1}] full-frame pixels of
 * keypoint k, score[(o*cap + i)*8 + k] = sqrt(sigmoid).  The solver (EPnP-RANSAC) runs on the host. */
int kd6d_pose_candidates(const kd6d_levels* levels, const float* cls, const float* reg,
                         const float* bbox_trans, const int32_t* class_ids, const int32_t* n_gt,
                         float threshold, float positive_num, float positive_lambda, int cap,
                         int32_t* cnt, float* kp, float* score, void* stream);
/* ---- PnP-RANSAC on the device (csrc/pnp.hip): kd6d/libs/pnp.py's solve_pnp_ransac for a batch of problems.
 * Problem p: cnt[p] <= cap cells (cap <= KD6D_PNP_MAX_CAP), kp (P*cap, 8, 2) full-frame px with problem p's cells at
 * p*cap (the layout of t_kp and of kd6d_pose_candidates' kp), box (P, 8, 3) object-space corners, K (P, 3, 3);
 * correspondence (cell i, keypoint k) belongs to corner k.  `iters` hypotheses, each one cell per corner drawn by a
 * counter-based hash of (seed, h, k): DLT, loose consensus (3 x reproj_err, z > 0), DLT re-fit on it, 4 Gauss-Newton
 * steps, tight consensus (reproj_err), 6 more steps when that set holds >= 6 points on >= 6 corners.  The winner has
 * the most tight inliers (ties: the smallest h).  Outputs: ok[p] = (winner's count >= 6, R and T finite), R (P,3,3),
 * T (P,3), n_inliers[p]; all zero when !ok (cnt[p] == 0, a box with < 6 distinct corners, a non-finite input).  A pure
 * function of the problem's own inputs and `seed`: bitwise reproducible, independent of the batch around it.
 * workspace: kd6d_pnp_workspace_floats(P, iters) floats, any contents.
 * kd6d_teacher_pnp_gate: the gate of postprocess_kd.py:187-202 on kd6d_teacher_select's slot arrays.  For every image
 * b with t_cnt[b] > 0 the class c is the first c < n_cls with sigmoid(cls[t_row[b*cap]*16 + c]) > threshold, else the
 * argmax; the problem is (image b's t_kp cells, kp3d[b, c] of kp3d (batch, n_class_rows, 8, 3), K[b]); t_cnt[b] = 0
 * when no pose is found (written by the launch's last kernel only). */
#define KD6D_PNP_MAX_CAP 32
int64_t kd6d_pnp_workspace_floats(int n_problems, int iters);
int kd6d_pnp_ransac(int n_problems, int cap, const int32_t* cnt, const float* kp, const float* box, const float* K,
                    float reproj_err, int iters, uint64_t seed, int32_t* ok, float* R, float* T, int32_t* n_inliers,
                    float* workspace, int64_t workspace_floats, void* stream);
int kd6d_teacher_pnp_gate(const float* cls, int n_cls, float threshold, const int32_t* t_row, int32_t* t_cnt,
                          const float* t_kp, int cap, int batch, const float* kp3d, int n_class_rows, const float* K,
                          float reproj_err, int iters, uint64_t seed, float* workspace, int64_t workspace_floats,
                          void* stream);
/* ---- pose remap of the augmentation chain on the device (csrc/pnp.hip; added under ABI 11, a new symbol only):
 * kd6d/libs/pnp.py's remap_pose for every instance of a batch, chained twice as kd6d/libs/augment.py::draw_params
 * chains it (Resize, then RandomShiftScaleRotate).  ONE LANE PER INSTANCE.  Instance i belongs to image inst_img[i]
 * (n_inst) and has class inst_cls[i] (n_inst); src_K (n_images, 9), src_R (n_inst, 9) and src_T (n_inst, 3) are DOUBLE
 * (the annotation files are read in double; rounding T ~ 1000 mm to fp32 first would by itself move a corner by about
 * 3e-5 px); box (n_class, 8, 3) fp32 object-space corners; dst_K_host (9) double, read before the call
 * returns; M_resize and M_ssr (n_images, 6) double: the first two rows of the homographies, the third is (0, 0, 1);
 * M_ssr may be NULL.
 * A stage (source K, M, source pose (R, T)): pts_k = M (K (R X_k + T)), xy_k = pts_k.xy / (pts_k.z + 1e-8) for the 8
 * corners X_k of the instance's class; DLT of the 8 correspondences on dst_K's normalised coordinates, then 20
 * Gauss-Newton steps on (rotation vector, t) (the solver of kd6d_pnp_ransac with one observation per corner; dst_K
 * enters it rounded to fp32 like every K of that solver).  Stage 1 = (src_K, M_resize, (src_R, src_T)); stage 2 =
 * (dst_K, M_ssr, stage 1's result rounded to fp32), or a copy of stage 1 when M_ssr is NULL.
 * pose_out (n_inst, 2, 12) fp32 = per stage {R (9), T (3)}, ok_out (n_inst, 2).  A stage that finds no pose (the DLT
 * fails, a non-finite value, a box with fewer than 6 distinct corners) has ok = 0 and returns its SOURCE pose rounded to
 * fp32 -- remap_pose's (srcR, srcT, -1) -- and the chain goes on from it.  An inst_img outside [0, n_images) or an
 * inst_cls outside [0, n_class) is never dereferenced: ok = 0 and a zero pose for both stages.  No LDS, no atomics, no
 * cross-lane arithmetic: a lane's result is a pure function of its own instance -- bitwise reproducible, independent
 * of the instance's position and of the batch around it.  Rows from n_inst on are not written. */
int kd6d_pose_remap(int n_inst, int n_images, int n_class, const int32_t* inst_img, const int32_t* inst_cls,
                    const double* src_K, const double* src_R, const double* src_T, const float* box,
                    const double* dst_K_host, const double* M_resize, const double* M_ssr, float* pose_out,
                    int32_t* ok_out, void* stream);
/* ---- pose errors of evaluation on the device (csrc/pose_err.hip; added under ABI 11, a new symbol only):
 * libs/utils.py::compute_pose_diff for n_problems (ground truth, prediction) pairs in ONE launch, one workgroup per
 * problem.  Problem p scores vcnt[p] (1 ... max_v, max_v <= KD6D_POSE_ERR_MAX_V = the reference's subsample size)
 * vertices of one mesh: verts[voff[p] + vidx[p*max_v + i]], or verts[voff[p] + i] when vidx == NULL.  Both sets are
 * moved into the camera frame ((Rg, Tg) and (Rp, Tp), K per problem); sym[p] != 0 matches every ground-truth vertex
 * with the predicted vertex at the smallest 3D distance (ties: the lowest index, as np.argmin), else vertex i with
 * vertex i.  err[p] = {mean 3D distance, mean distance of the pinhole projections p / (p_z + 1e-8) through K} of the
 * matched pairs; nn (optional, (P, max_v)) = position i' < vcnt[p] of the vertex matched to vertex i, -1 from
 * vcnt[p] on.  Differences are formed as Rg m_i - Rp m_j + (Tg - Tp), in fp32.  No atomics, sums in a fixed order: a
 * pure function of the problem's own inputs, bitwise reproducible.  The caller guarantees that every index lies
 * inside the pool (kd6d.ops.pose_errors checks it); a vcnt outside 0 ... max_v is clamped, 0 gives err = {0, 0}. */
#define KD6D_POSE_ERR_MAX_V 1000
int kd6d_pose_errors(int n_problems, int max_v, const float* verts, const int32_t* voff, const int32_t* vcnt,
                     const int32_t* vidx, const float* K, const float* Rg, const float* Tg, const float* Rp,
                     const float* Tp, const int32_t* sym, float* err, int32_t* nn, void* stream);
/* ---- BOP pose errors on the device (csrc/bop_err.hip; added under ABI 11, new symbols only): MSSD and MSPD of
 * n_problems (ground truth, prediction) pairs.  Problem p scores ALL vcnt[p] vertices v_i = verts[voff[p] + i] (no cap,
 * no index table) under the symmetry transforms S_s = syms[soff[p] + s], s < scnt[p] (12 floats each: R row-major, then
 * t; scnt[p] <= 0: the identity alone, syms is then not read for p):
 *   err[p][0] = min_s max_i |(Rp v_i + Tp) - (Rg (S_s v_i) + Tg)|                           (mssd, the vertices' unit)
 *   err[p][1] = the same min / max over the pinhole projections q.xy / (q.z + 1e-8), q = K x  (mspd, pixels)
 * K, Rg, Rp (P, 9), Tg, Tp (P, 3) per problem.  Rg S_R and Rg S_t are composed once per (problem, symmetry);
 * differences are formed as (Rg S_R) v + (Rg S_t + (Tg - Tp)) - Rp v, in fp32.  vcnt[p] <= 0 gives err = {0, 0}.
 * Two launches: the maximum of every (problem, symmetry) goes to `workspace`, row p holding
 * cap = workspace_floats / (2 n_problems) symmetries; the second launch takes the minima.  A scnt[p] above cap is
 * clamped to cap: size the workspace with kd6d_bop_errors_workspace_floats(n_problems, the largest scnt).
 * n_problems == 0 returns success without a launch and reads no pointer.  The caller guarantees that every vertex and
 * symmetry index lies inside its pool (kd6d.ops.bop_errors checks it).
 * Bitwise property: max and min of floats are exact in any order -- no atomics, no accumulators, no in-kernel
 * cross-workgroup barrier.  err[p] is a pure function of problem p's own inputs: two launches agree bit for bit, a
 * problem scores the same alone and inside any batch, under any order of its vertices and any order of its symmetries;
 * a duplicated symmetry changes nothing and an added one can only lower an error. */
int64_t kd6d_bop_errors_workspace_floats(int n_problems, int max_scnt);
int kd6d_bop_errors(int n_problems, const float* verts, const int32_t* voff, const int32_t* vcnt, const float* syms,
                    const int32_t* soff, const int32_t* scnt, const float* K, const float* Rg, const float* Tg,
                    const float* Rp, const float* Tp, float* workspace, int64_t workspace_floats, float* err,
                    void* stream);
/* ---- BOP's VSD on the device (csrc/bop_vsd.hip; added under ABI 11, new symbols only): a depth rasteriser and the
 * visible-surface-discrepancy counts of n (ground truth, estimate) pairs.  kd6d/libs/bop_metrics.py holds the float64
 * definitions (render_depth_host, vsd_errors_host) and the rasteriser contract: pixel centres at integer coordinates,
 * K = [fx s cx; 0 fy cy; 0 0 1], inclusive edges, both windings, a triangle with a vertex at z <= 0 dropped whole (no
 * near-plane clipping), depth = the triangle's plane along the pixel's ray clamped to its vertex z range, minimum over
 * the triangles, background 0.
 * Item i draws the fcnt[i] triangles faces[foff[i] + f] (int32 triples, indices RELATIVE to voff[i], each < vcnt[i]) of
 * the vertices verts[voff[i] ...]; n_verts / n_faces are the pools' sizes.  An item whose offsets or counts leave a
 * pool (or, for kd6d_bop_vsd, whose frame index is outside [0, n_img)) is never dereferenced: its map / counts stay 0;
 * a face with an index outside [0, vcnt[i]) is skipped (kd6d.ops checks all of this with validate=True).
 * kd6d_render_depth: depth_out (n, H, W) fp32, the z of the camera frame, under (R[i], T[i]), K[i].
 * kd6d_bop_vsd: depth (n_img, H, W) fp32 in the vertices' unit (0 = missing), frame[p] the image of problem p.  With
 * dist = depth * |K^-1 (x, y, 1)| per pixel, vis(t, m) = (t > 0 && m > 0 && m - t <= delta) || (t == 0 && m > 0):
 *   visib_gt = vis(dist_test, dist_gt),  visib_est = vis(dist_test, dist_est) || (visib_gt && dist_est > 0)
 *   counts[p] = { n_u = |gt or est|, n_inter = |gt and est|,
 *                 cost_k = #{inter: |dist_gt - dist_est| >= tau[k] * diameter[p]} + n_u - n_inter,  k < n_tau }
 *   err[p][k] = cost_k / n_u,  1 when n_u == 0                              (BOP19: visib_mode bop19, the step cost)
 * tau_host: n_tau <= 16 values read on the host at the call.  workspace: kd6d_bop_vsd_workspace_ints(n) int32 (the
 * regions of interest), for both entry points.  n == 0 returns success without a launch and reads no pointer.
 * Bitwise property: the z-test is an unsigned-integer minimum in LDS and the counts are integer sums -- no float
 * atomics, no accumulators.  A map and counts[p] are pure functions of the item's own inputs: two calls agree bit for
 * bit, an item scores the same alone and inside any batch, under any order of its faces and with a face repeated;
 * err is one division of two of those integers. */
int64_t kd6d_bop_vsd_workspace_ints(int n);
int kd6d_render_depth(int n, const float* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* voff,
                      const int32_t* vcnt, const int32_t* foff, const int32_t* fcnt, const float* K, const float* R,
                      const float* T, int H, int W, int32_t* workspace, int64_t workspace_ints, float* depth_out,
                      void* stream);
int kd6d_bop_vsd(int n, const float* verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* voff,
                 const int32_t* vcnt, const int32_t* foff, const int32_t* fcnt, const float* K, const float* Rg,
                 const float* Tg, const float* Rp, const float* Tp, const float* diameter, const int32_t* frame,
                 const float* depth, int n_img, int H, int W, float delta, const float* tau_host, int n_tau,
                 int32_t* workspace, int64_t workspace_ints, int32_t* counts, float* err, void* stream);
/* ---- training frames on the device (csrc/render_frames.hip; added under ABI 11, new symbols only): a colour rasteriser.
 * One call draws n_frames frames of H x W pixels; frame f shows the items with item_frame[i] == f, each in its own slot
 * g = item_slot[i] < KD6D_MAX_GT, over backgrounds[bg_index[f]].  kd6d/libs/render.py::render_frames_host is the float64
 * definition.  Mesh pools, offsets and counts as kd6d_render_depth (faces relative to voff[i]); vcol: uint8 RGB per vertex,
 * indexed as verts; R (n_items, 9), T (n_items, 3); per frame K (n_frames, 9), light (n_frames, 3: a unit vector of the
 * camera frame pointing FROM the surface TO the light), ambient (n_frames) in [0, 1], bg_index (n_frames);
 * backgrounds (n_bg, H, W, 3) uint8, copied as they are (BGR).
 * Coverage and depth: the rasteriser contract above, bit for bit (both units share csrc/kd6d_raster.h): the depth of a
 * frame with one item equals kd6d_render_depth's map of that item.
 * Owner: the triangle of the smallest depth at the pixel; among triangles of bit-equal depth the lowest (slot, face index).
 * Colour, from the owner (vertices v0 v1 v2 with colours c0 c1 c2 and camera z Z0 Z1 Z2; E01, E12, E20 the projected edge
 * functions of the pixel centre times the sign of the projected area, as in the coverage test):
 *   b0 = E12 / Z0, b1 = E20 / Z1, b2 = E01 / Z2          (perspective-correct barycentric weights, normalised below)
 *   albedo_c = (b0 c0_c + b1 c1_c + b2 c2_c) / (b0 + b1 + b2)
 *   n = R normalize((v1 - v0) x (v2 - v0)), negated when n . X0 > 0 so that it faces the camera
 *   shade = ambient + (1 - ambient) max(0, n . light)
 *   channel = clamp(floor(albedo_c * shade + 0.5), 0, 255)
 * Outputs: frames_out (n_frames, H, W, 3) uint8 BGR; masks_out (n_frames, H, W) uint8, 0 = background, g + 1 = the slot
 * that owns the pixel (the VISIBLE mask); depth_out (n_frames, H, W) fp32 or NULL.  A pixel without an owner takes the
 * background's pixel (zeros when bg_index[f] is outside [0, n_bg)), mask 0, depth 0.
 * An item whose offsets or counts leave a pool, whose fcnt >= 2^28, whose frame is outside [0, n_frames) or whose slot is
 * outside [0, KD6D_MAX_GT) is never dereferenced and draws nothing; of several items that claim one (frame, slot) the one
 * of the lowest index is drawn; a face with an index outside [0, vcnt[i]) is skipped (kd6d.ops checks all of this with
 * validate=True).  n_frames == 0 returns success without a launch; n_items == 0 gives the backgrounds.
 * workspace: kd6d_render_frames_workspace_ints(n_frames, n_items) int32.
 * Bitwise property: two unsigned-integer minima in LDS (depth bits, then the packed owner id) decide every pixel -- no
 * float atomics, no global z-buffer.  A frame is a pure function of its own inputs: two calls agree bit for bit, a frame
 * is the same alone and inside any batch, under any order of the items and with a face repeated. */
int64_t kd6d_render_frames_workspace_ints(int n_frames, int n_items);
int kd6d_render_frames(int n_frames, int n_items, const float* verts, int n_verts, const int32_t* faces, int n_faces,
                       const uint8_t* vcol, const int32_t* voff, const int32_t* vcnt, const int32_t* foff,
                       const int32_t* fcnt, const int32_t* item_frame, const int32_t* item_slot, const float* R,
                       const float* T, const float* K, const float* light, const float* ambient,
                       const int32_t* bg_index, const uint8_t* backgrounds, int n_bg, int H, int W, int32_t* workspace,
                       int64_t workspace_ints, uint8_t* frames_out, uint8_t* masks_out, float* depth_out, void* stream);
int kd6d_ssc_assign(const kd6d_levels* levels, const float* mask, int mask_h, int mask_w, const float* kp3d,
                    const float* K, const int32_t* class_ids, const int32_t* n_gt, const float* rot,
                    const float* trans, const float* bbox_trans, const float* keys, float positive_num,
                    float positive_lambda, int cap, int32_t* labels, int32_t* pos_cnt, int32_t* pos_row,
                    int32_t* pos_gt, void* stream);
int kd6d_focal_fwd(const float* cls, const int32_t* labels, int rows, float gamma, float alpha, float* loss,
                   kd6d_scalar_ws* loss_ws, void* stream);
int kd6d_focal_bwd(int dtype, const float* cls, const int32_t* labels, int rows, float gamma, float alpha,
                   const float* weight, void* dcls, void* stream);
int kd6d_student_points(const kd6d_levels* levels, const float* cls, const float* reg, const int32_t* pos_cnt,
                        const int32_t* pos_row, const int32_t* pos_gt, const int32_t* class_ids,
                        const float* kp3d, const float* rot, const float* trans, const float* bbox_trans,
                        const float* diameters, const float* kinv_host, float frame_w, float frame_h, int cap,
                        float* xs, float* alpha, float* g_reg_xy, float* loss_reg, kd6d_scalar_ws* loss_reg_ws,
                        int32_t* s_start, void* stream);
int kd6d_kd_mean(const float* loss_img, const int32_t* valid_img, int n_images, float* loss_kd,
                 int32_t* n_valid, void* stream);
int kd6d_loss_backward(const kd6d_levels* levels, int dtype, const float* cls, const float* reg,
                       const int32_t* pos_cnt, const int32_t* pos_row, const int32_t* pos_gt,
                       const int32_t* class_ids, const float* bbox_trans, const float* g_reg_xy,
                       const float* g_kd_xs, const float* g_kd_alpha, const int32_t* n_valid,
                       const int32_t* valid_img, const float* weights, const float* seg_scale,
                       int64_t* dseg_scale_acc, int64_t acc_hi_stride, float frame_w, float frame_h, int cap,
                       int detach_alpha, void* dcls, void* dreg, void* stream);

/* ---- per-object KD (added under ABI 11, new symbols only): one OT problem per (image, ground-truth slot) instead of
 * one per image.  Object o = b*KD6D_MAX_GT + g exists for g < n_gt[b].
 * kd6d_teacher_select_objects: kd6d_pose_candidates' selection (the kd6d_teacher_select rule restricted to class
 *   class_ids[b*KD6D_MAX_GT + g]) with kd6d_teacher_select's full outputs: object o owns slots
 *   [o*cap, o*cap + t_cnt[o]) of t_kp / t_score / t_row / t_kp_norm / t_beta; t_cnt[o] = 0 for g >= n_gt[b].  t_kp and
 *   t_score are bitwise kd6d_pose_candidates' kp and score.  Two slots of one image with the same class get the same
 *   cells (the teacher cannot tell instances of one class apart).
 * kd6d_kd_group_objects: stable partition of image b's positive slots [b*cap, b*cap + pos_cnt[b]) (cap <= 64) by
 *   pos_gt.  obj_start[o] / obj_cnt[o]: object o's segment of the object-major arrays, inside the image's own block
 *   and in ascending slot (= packed row) order; dest[b*cap + i] = where slot i went; xs_obj (slots,8,2) / alpha_obj
 *   (slots,8) = bit copies of xs / alpha in that order.  A slot whose pos_gt is outside 0..KD6D_MAX_GT-1 goes behind
 *   the last object and belongs to none.  Slots from pos_cnt[b] on are not written.
 * kd6d_kd_scatter_objects: grad_xs[slot] = grad_xs_obj[dest[slot]] (grad_alpha alike) for the cells of an object with
 *   valid_obj[o] > 0, zeros for every other positive slot; valid_img[b] = 1 when image b has a valid object, else 0.
 * The step: kd6d_student_points -> kd6d_kd_group_objects -> kd6d_sinkhorn_div_fwd_bwd over batch*KD6D_MAX_GT problems
 * (student segments obj_start / obj_cnt, teacher segments o*cap / t_cnt) -> kd6d_kd_mean over the same count ->
 * kd6d_kd_scatter_objects -> kd6d_loss_backward with valid_img and n_valid = the number of valid objects.
 * No atomics; every output is a function of the image's own rows: two launches agree bitwise. */
int kd6d_teacher_select_objects(const kd6d_levels* levels, const float* cls, const float* reg,
                                const float* bbox_trans, const int32_t* class_ids, const int32_t* n_gt,
                                float threshold, float positive_num, float positive_lambda, int cap, float frame_w,
                                float frame_h, int32_t* t_cnt, float* t_kp, float* t_score, int32_t* t_row,
                                float* t_kp_norm, float* t_beta, void* stream);
int kd6d_kd_group_objects(const int32_t* pos_cnt, const int32_t* pos_gt, const float* xs, const float* alpha,
                          int batch, int cap, int32_t* obj_start, int32_t* obj_cnt, int32_t* dest, float* xs_obj,
                          float* alpha_obj, void* stream);
int kd6d_kd_scatter_objects(const int32_t* pos_cnt, const int32_t* pos_gt, const int32_t* dest,
                            const int32_t* valid_obj, const float* grad_xs_obj, const float* grad_alpha_obj,
                            int batch, int cap, float* grad_xs, float* grad_alpha, int32_t* valid_img, void* stream);

/* ---- dense optimal transport (BASELINE config 5: D-dimensional local predictions over a whole cell grid,
 * thousands of points per set; the reference would need geomloss' KeOps backend above 5000^2 pairs).  Same
 * divergence and gradients as kd6d_sinkhorn_div_fwd_bwd for ONE problem: x (N,D) with weights alpha (N)
 * against y (M,D) with beta (M), D in {2,4,8,16}; cost matrices are never materialised (online logsumexp over
 * LDS-staged column tiles).  `diameter` > 0 is the box diagonal of all points (geomloss' diameter= argument);
 * kd6d_sinkhorn_dense_diameter computes it on the device (scratch64: 64 floats).  workspace:
 * kd6d_sinkhorn_dense_workspace_floats(N, M, D) floats, any contents (its regions and their sum are
 * csrc/sinkhorn_plan.h's DenseWorkspace, as are the epsilon schedule and the kernel, rows and grid of every softmin
 * launch).  Outputs: loss (1), grad_x (N,D), grad_alpha (N). */
int64_t kd6d_sinkhorn_dense_workspace_floats(int N, int M, int D);
int kd6d_sinkhorn_dense_diameter(const float* x, const float* y, int N, int M, int D, float* scratch64,
                                 float* diam_out, void* stream);
int kd6d_sinkhorn_dense_fwd_bwd(const float* x, const float* alpha, const float* y, const float* beta, int N, int M,
                                int D, float p, float blur, float scaling, float reach, double diameter,
                                float* workspace, int64_t workspace_floats, float* loss, float* grad_x,
                                float* grad_alpha, void* stream);

/* ---- Dynamic-Zoom-In front-end (the stage before the hot path): replaces
 * transform.py:299-308 (Normalize, ToTensor) + dzi_libs.py:55-95,142-210 (affine from the jittered box,
 * cv2.warpAffine bilinear on the image / nearest on the mask) for a whole batch.
 * frames_bgr (B,H,W,3) uint8 as decoded; masks (B,H,W) float or NULL; center_scale (B,3) = {cx, cy, box side}
 * (host: aug_bbox_DZI); lut_rgb (3,256) = float32((v/255 - mean_c)/std_c), RGB order.
 * Out: images_nchw (B,3,out,out) fp32, masks_out (B,out,out), bbox_trans (B,2,3), bbox_scale (B) = out/side. */
int kd6d_dzi_crop(const uint8_t* frames_bgr, const float* masks, int B, int H, int W, const float* center_scale,
                  const float* lut_rgb, int out_res, float* images_nchw, float* masks_out, float* bbox_trans,
                  float* bbox_scale, void* stream);

/* ---- device-resident frame cache (csrc/frame_cache.hip; added under ABI 11, new symbols only): the decoded frames of
 * a whole image list stay in device memory and a batch is assembled from sampler indices (kd6d/libs/frame_cache.py,
 * train_kd.py / test.py --frame_cache device).  Pure data movement: the outputs are byte for byte what the host loader
 * uploads, and kd6d_dzi_crop / the augmentation front-end consume them unchanged.
 * kd6d_cache_gather_frames: frames_u8 (n,H,W,3) BGR and masks_u8 (n,H,W) merged instance ids; index_dev (B) int32;
 *   frames_out_u8 (B,H,W,3) = frames_u8[index[b]], masks_out_f32 (B,H,W) = float(masks_u8[index[b]]).  No alignment is
 *   required of any pointer beyond masks_out_f32's own 4 bytes, nor of H*W*3: lanes move 16-byte granules where source
 *   and destination of a frame can both be aligned to them, 4-byte or single bytes otherwise, heads and tails bytewise.
 *   An index outside [0, n) is never dereferenced: that batch entry is zero-filled (the host validates before upload).
 * kd6d_cache_gather_targets: the small fields of a batch in the packed layout of kd6d.kd_losses.PackedTargets, one
 *   launch.  table_f (n, KD6D_CACHE_ROW_F) = per frame {K 9, rot KD6D_MAX_GT*9, trans KD6D_MAX_GT*3}, table_i
 *   (n, KD6D_CACHE_ROW_I) = {n_gt, class_ids KD6D_MAX_GT}, both zero-padded behind n_gt instances; kp3d (kp_elems =
 *   classes*24, a multiple of 4): the 3D box corners, the same for every frame; bbox_trans (B,2,3): the output of the
 *   kd6d_dzi_crop launch of this batch (copied, not recomputed: the packed block is the host path's bit for bit).
 *   flat_f_out = {kp3d B*kp_elems | K B*9 | bbox_trans B*6 | rot B*MAX_GT*9 | trans B*MAX_GT*3}, flat_i_out =
 *   {class_ids B*MAX_GT | n_gt B}, every field rounded up to 4 elements, the padding written as zero.  An index
 *   outside [0, n) yields an image without instances. */
#define KD6D_CACHE_ROW_F (9 + KD6D_MAX_GT * 12)
#define KD6D_CACHE_ROW_I (1 + KD6D_MAX_GT)
int kd6d_cache_gather_frames(const uint8_t* frames_u8, const uint8_t* masks_u8, int n, int H, int W,
                             const int32_t* index_dev, int B, uint8_t* frames_out_u8, float* masks_out_f32, void* stream);
int kd6d_cache_gather_targets(const float* table_f, const int32_t* table_i, const float* kp3d, int kp_elems, int n,
                              const int32_t* index_dev, int B, const float* bbox_trans, float* flat_f_out,
                              int32_t* flat_i_out, void* stream);

/* ---- train-time augmentation of full frames (csrc/augment.hip): the reference's train transform chain
 * (libs/train_libs.py:212-238: Resize, RandomOcclusion, RandomShiftScaleRotate, RandomHSV, RandomSmooth,
 * RandomNoise, Grayscalize) and remove_invalids (poses.py:172-200), on the uint8 BGR frames (B,H,W,3) and float
 * instance masks (B,H,W) the DZI crop consumes.  The host (kd6d/libs/augment.py) draws every scalar parameter;
 * per-pixel randomness is a counter-based hash of (key, image, pixel, channel).  The arithmetic restates cv2's
 * 8-bit fixed-point paths (parity unpinned at the cv2 boundary; tests/augment_ref.py).
 * kd6d_aug_warp_u8     fwd_mats (B,6) double: FORWARD 2x3 matrices (dst = M src), inverted in double like
 *                      cv2.warpAffine; frame bilinear with 15-bit tap weights and border 128, mask nearest with
 *                      border 0.  src_mask / dst_mask both or neither; src != dst.
 * kd6d_aug_mask_stats  stats (B,max_id,5) int32 = {area, xmin, ymin, xmax, ymax} of mask == id (id 1..max_id);
 *                      {0,0,0,0,0} when id is absent.  Integer atomics only (order-free).
 * kd6d_aug_occlude     in place; per image the first min(n_inst[b], KD6D_MAX_GT) instances: rectangle from
 *                      stats (stats_ids ids per image) and uniforms (B,KD6D_MAX_GT,5) double (RandomOcclusion's five
 *                      random.uniform draws, as u in [0,1)); random bytes into the frame, -1 into the mask.
 * kd6d_aug_hsv         in place; factors (B,3) float32 = the (h, s, v) multipliers of distort_hsv.
 * kd6d_aug_filter      src -> dst (distinct): box blur ksize (B) int32 (odd, NULL = 1, BORDER_REFLECT_101), then
 *                      Gaussian noise sigma (B) float32 (NULL or 0 = none), then BGR2GRAY into 3 channels if gray.
 * kd6d_aug_relabel     in place; mask id in 1..max_id -> lut[b*(max_id+1) + id], any other value -> 0. */
#define KD6D_AUG_MAX_ID 16
int kd6d_aug_warp_u8(const uint8_t* src, const float* src_mask, int B, int H, int W, const double* fwd_mats, int Ho,
                     int Wo, uint8_t* dst, float* dst_mask, void* stream);
int kd6d_aug_mask_stats(const float* masks, int B, int H, int W, int max_id, int32_t* stats, void* stream);
int kd6d_aug_occlude(uint8_t* frames, float* masks, int B, int H, int W, const int32_t* stats, int stats_ids,
                     const double* uniforms, const int32_t* n_inst, double prob, uint64_t key, void* stream);
int kd6d_aug_hsv(uint8_t* frames, int B, int H, int W, const float* factors, void* stream);
int kd6d_aug_filter(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* ksize, const float* sigma,
                    int gray, uint64_t key, void* stream);
int kd6d_aug_relabel(float* masks, int B, int H, int W, const float* lut, int max_id, void* stream);

/* ---- the two remaining stages of the train transform chain (csrc/augment.hip; added under ABI 11, new symbols
 * only; train_kd.py --aug_chain full).  Restatements like the stages above: parity unpinned at the cv2 boundary,
 * the same arithmetic in numpy in tests/augment_full_ref.py.
 * kd6d_aug_background  RandomBackground / merge_background_mask, in place on frames; masks are read only.  Image b with
 *                      bg_index[b] = i in [0, n_bg): every pixel whose mask value is exactly 0 takes the pixel of
 *                      cv2.resize(background i, (W, H)), 8-bit INTER_LINEAR with 11-bit coefficients (the integer recipe
 *                      stands at the kernel), gathered from `pool`: n_bg BGR uint8 images at their native sizes in one
 *                      buffer of pool_bytes, image i = bg_hw[2i] x bg_hw[2i+1] pixels at byte bg_off[i].  A background
 *                      of the frame's size is copied exactly.  bg_index[b] = -1: untouched.  Defined no-ops, nothing
 *                      dereferenced: an index outside [-1, n_bg), h or w < 1 (or > 32768), off < 0 or
 *                      off + h*w*3 > pool_bytes.  The reference's alpha-channel merge is not built (frames are 3-channel).
 * kd6d_aug_sharpen     RandomPencilSharpen, src -> dst (distinct).  Per image: ksize (B) int32 in {0, 5, 7, 9, 11}
 *                      (0, and any other value, copies the image), mode (B) int32 (non-zero: edge = img / (blur + 0.01),
 *                      zero: img - blur, float32), alpha (B) double.  edge -> uint8 by cv2.normalize(NORM_MINMAX, 0, 255)
 *                      over all pixels and channels, blended img * (1 - alpha) + e * alpha in double, normalised again.
 *                      The whole-image extrema are merged with integer atomic min / max on order-preserving encodings
 *                      (exact in any order: reproducible).  ws: kd6d_aug_sharpen_ws_bytes(B) bytes, 8-byte aligned,
 *                      initialised inside the call. */
int kd6d_aug_background(uint8_t* frames, const float* masks, int B, int H, int W, const uint8_t* pool, int64_t pool_bytes,
                        const int64_t* bg_off, const int32_t* bg_hw, int n_bg, const int32_t* bg_index, void* stream);
int64_t kd6d_aug_sharpen_ws_bytes(int B);
int kd6d_aug_sharpen(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* ksize, const int32_t* mode,
                     const double* alpha, void* ws, int64_t ws_bytes, void* stream);

/* ---- optimiser: replaces clip_grad_norm_ + AdamW.step of train_kd.py:138-139 on one flat buffer.
 * kd6d_sumsq writes KD6D_SUMSQ_PARTS partial sums of x^2 (one per workgroup, unused slots zeroed; no atomics);
 * kd6d_clip_adamw adds them in a fixed order (reproducible), writes the total to *gnorm_sq_out (optional) and applies
 * g *= min(1, max_norm/(sqrt(total)+1e-6)) (gnorm_partials == NULL: no clipping) then the decoupled-weight-decay Adam update
 * (torch.optim.AdamW semantics, step counted from 1) and refreshes the bf16 shadow if given.
 * hyper_dev (optional, 4 floats on the device: lr, 1-beta1^t, sqrt(1-beta2^t), and a fourth that kd6d_set_hyper
 * sets to 0 -- the host passes it as gnorm_sq_out) overrides lr/step:
 * it lets the launch sit inside a captured hipGraph while the OneCycle schedule of
 * libs/train_libs.py:120 keeps advancing on the host; kd6d_set_hyper writes it (values travel in
 * the kernel arguments, so the host may run ahead of the device). */
#define KD6D_SUMSQ_PARTS 128
int kd6d_sumsq(const float* x, int64_t n, float* partials, void* stream);
int kd6d_clip_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                    const float* gnorm_partials, float* gnorm_sq_out, double max_norm, double lr, double beta1,
                    double beta2, double eps, double weight_decay, int64_t step, const float* hyper_dev,
                    void* bf16_shadow, void* stream);
int kd6d_set_hyper(float* hyper_dev, double lr, double beta1, double beta2, int64_t step, void* stream);
int kd6d_cast_f32_to_bf16(const float* x, void* y, int64_t n, void* stream);

/* ---- data-parallel exchange over RCCL / xGMI: replaces the reference's process-group plumbing for the step --
 * libs/distributed.py:9-41 (gloo rank / world / barrier helpers), train_kd.py:48-51 (init_process_group + barrier),
 * the DDP constructor's one-time parameter broadcast (libs/train_libs.py:123-130) -- and adds the per-step gradient
 * all-reduce the reference lacks (its DDP wrapper is discarded, libs/train_libs.py:130).
 * One communicator per process (= per GPU, the current HIP device at kd6d_comm_init).  Rendezvous: rank 0 calls
 * kd6d_comm_unique_id (128 bytes, host memory) and hands the id to the other ranks by any out-of-band channel
 * (the Python host uses the torch.distributed store); every rank then calls kd6d_comm_init (collective).
 * kd6d_comm_allreduce: in place, fp32, sum or mean over ranks, asynchronous on `stream` (stream-ordered behind
 * the caller's last weight gradient: no host synchronisation).  kd6d_comm_broadcast: in place, raw bytes from
 * `root`.  librccl is resolved at run time (a copy already mapped into the process is shared); without it these
 * return KD6D_ERR_UNSUPPORTED and everything else in this header still works. */
typedef struct kd6d_comm kd6d_comm;
int kd6d_comm_unique_id(void* id_out_host /* 128 bytes */);
int kd6d_comm_init(kd6d_comm** comm, int rank, int world, const void* unique_id_host /* 128 bytes */);
int kd6d_comm_rank(const kd6d_comm* comm);
int kd6d_comm_world(const kd6d_comm* comm);
int kd6d_comm_version(void);      /* RCCL version code (e.g. 22703), -1 without librccl */
int kd6d_comm_allreduce(kd6d_comm* comm, float* buf, int64_t n, int mean, void* stream);
int kd6d_comm_broadcast(kd6d_comm* comm, void* buf, int64_t nbytes, int root, void* stream);
int kd6d_comm_destroy(kd6d_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* KD6D_H */
