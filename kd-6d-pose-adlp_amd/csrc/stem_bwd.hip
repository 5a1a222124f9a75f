// BatchNorm (train) + activation + MaxPool2d(2,2) backward fused into the weight gradient of the convolution in front of
// it, for a block whose input needs no gradient (the first block of the darknet-tiny students: the image has none).
//
// On the separate path bn_pool_bwd_apply_kernel (norm_ops.hip) writes the gradient of the convolution output, d_raw, as
// a bf16 tensor of the full resolution and conv_wgrad_tr_kernel reads it back -- its only reader.  Here a persistent
// workgroup walks tiles of R whole image rows (conv_plan.h, stem_bwd_rule) and per tile
//   * brings the source rows (+1 above and below) into LDS by LDS-DMA in the ZERO-PADDED 2-D layout of
//     conv_wgrad_small_kernel: one zero column left and right of every image row, so tap (ky,kx) of position q is
//     position q + ky*(W+2) + kx and no validity mask exists;
//   * re-derives the four activations of every 2x2 window from the fp32 convolution output, finds the first maximum,
//     routes the pooled gradient there and forms d_raw -- the arithmetic of bn_pool_bwd_apply_kernel, expression by
//     expression, and its rounding to bf16 -- into an LDS tile in plain pixel order (row * W + column, no pad columns;
//     only the patch is padded: pixel l of row r sits at patch position l + 2 r + 1);
//   * contracts d_raw^T x patch on the matrix pipe in steps of 32 consecutive PIXELS, in pixel order; both operands (8
//     consecutive pixels of one channel per lane) come out of the transposing LDS read.  The five 16 x 16 blocks of the
//     16 x 80 (Cout x 9 taps x 8 channels, padded) image are dealt to the four waves; a block lives in its wave's
//     registers across all tiles of the workgroup, which are CONSECUTIVE (tiles_per_wg of them): one partial image is the
//     sum over a contiguous pixel range in steps of 32, exactly how conv_wgrad_tr_kernel forms the partial image of a
//     pixel split -- and stem_bwd_rule takes the range from that kernel's split, so on the students' stems the slab
//     holds bit for bit what the separate path leaves there.
// The blocks go through LDS into the workgroup's partial image (slab[part][n][j], parts = grid): plain stores, no
// atomics, the same bits on every execution.
// The convolution output and the pooled gradient of the NEXT tile are fetched into registers before the matrix loop of
// the current one, so the long reads overlap it.
#include "conv_common.h"

namespace {

using namespace kd6d_detail;
typedef long long acc_t;
typedef short s16x4_t __attribute__((ext_vector_type(4)));

struct StemBwdParams {
  const float* raw;          // (B, H, W, NOUT) fp32 convolution output
  const bf16_t* dz;          // (B, H/2, W/2, NOUT) gradient of the pooled output
  const bf16_t* x;           // (B, H, W, 8) the block's input
  const float *mean, *invstd, *gamma, *beta;
  const acc_t *sum_dy, *sum_dy_xhat;      // `replicas` rows of NOUT accumulators each (bn_pool_bwd_reduce_kernel)
  float *dgamma, *dbeta, *dw;
  int replicas, B, H, W, act;
  float inv_rows;
  int R, tiles_per_img, ntiles, Qpad, prow, tiles_per_wg;
};

// 8 consecutive pixels of one 16-bit column per lane: this lane's 8-byte piece of pixels 0 .. 3 at `lo_piece`, of pixels
// 4 .. 7 at `hi_piece` (ds_read_b64_tr_b16: every lane of the wave takes part -- selects, never branches, around it)
__device__ __forceinline__ bf16x8_t tr_read8(const char* lo_piece, const char* hi_piece) {
  typedef s16x4_t __attribute__((address_space(3))) * lds_ptr_t;
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr_t)lo_piece);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr_t)hi_piece);
  typedef short s16x8_t __attribute__((ext_vector_type(8)));
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}

// as bn_act / bn_scale_shift of norm_ops.hip: the explicit fma keeps the argmax of a window what the forward saw
__device__ __forceinline__ float stem_act(float v, float sc, float sh, int act) {
  float t = __builtin_fmaf(v, sc, sh);
  if (act == KD6D_ACT_LEAKY) t = t > 0.f ? t : 0.1f * t;
  else if (act == KD6D_ACT_RELU) t = fmaxf(t, 0.f);
  return t;
}

template <int E>
__device__ __forceinline__ float replica_sum(const acc_t* __restrict__ rows, int C, int replicas, int c) {
  acc_t lo = 0, hi = 0;
  for (int r = 0; r < replicas; ++r) {
    lo += rows[((size_t)r * C + c) * 2];
    hi += rows[((size_t)r * C + c) * 2 + 1];
  }
  return det_value<E>(lo, hi);
}

// One work item = one 2x2 window x 4 channels: 4 x 16 B of the convolution output, 8 B of the pooled gradient.
struct StemItem {
  f32x4_t xv[4];
  u32x2_t dz;
};

template <int NOUT>
__global__ __launch_bounds__(256) void stem_bwd_wgrad_kernel(const StemBwdParams p) {
  constexpr int CQ = NOUT / 4;          // channel quads
  constexpr int IPT = NOUT / 8;         // work items per thread and tile: R * W <= 512 positions
  constexpr int DYB = 2 * NOUT;         // LDS bytes of one d_raw position
  constexpr int PXB = 16;               // LDS bytes of one source position
  constexpr int J = 72, JB = 5, JP = JB * 16, MAXB = 2;      // blocks wave, wave + 4 of the JB belong to a wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tot = reinterpret_cast<float*>(smem);      // 2 * NOUT totals
  char* dyp = smem + 128;
  char* pat = dyp + p.Qpad * DYB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = p.H, W = p.W, Wp = W + 2, Wh = W >> 1;
  const float inv_wp = 1.0f / (float)Wp, inv_w = 1.0f / (float)W;
  const int nitems = (p.R >> 1) * Wh * CQ;
  const char* zero = reinterpret_cast<const char*>(kd6d_zero_page);

  // ---- per-channel constants of this thread's quad; the totals once per workgroup ----
  const int cq = tid % CQ;
  float m[4], is[4], ga[4], be[4], sc[4], sh[4], k1[4], k2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = cq * 4 + e;
    m[e] = p.mean[c]; is[e] = p.invstd[c]; ga[e] = p.gamma[c]; be[e] = p.beta[c];
    sc[e] = ga[e] * is[e];
    sh[e] = __builtin_fmaf(-m[e], sc[e], be[e]);
  }
  for (int i = tid; i < 2 * NOUT; i += 256)
    tot[i] = i < NOUT ? replica_sum<KD6D_DET_GRAD>(p.sum_dy, NOUT, p.replicas, i)
                      : replica_sum<KD6D_DET_GRAD>(p.sum_dy_xhat, NOUT, p.replicas, i - NOUT);
  for (int i = tid; i < p.Qpad * DYB / 16; i += 256) reinterpret_cast<u32x4_t*>(dyp)[i] = u32x4_t{0u, 0u, 0u, 0u};
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    k1[e] = tot[cq * 4 + e] * p.inv_rows;
    k2[e] = tot[NOUT + cq * 4 + e] * p.inv_rows;
  }
  if (blockIdx.x == 0) {                     // one writer per channel: plain adds, reproducible
    for (int c = tid; c < NOUT; c += 256) {
      if (p.dgamma) p.dgamma[c] += tot[NOUT + c];
      if (p.dbeta) p.dbeta[c] += tot[c];
    }
  }

  // item i of a tile: window (wr, wx) of the tile's R/2 x W/2, channel quad cq (the same for every item of a thread)
  auto fetch = [&](int tile, StemItem (&it)[IPT]) {
    const int img = tile / p.tiles_per_img;
    const int y0 = (tile - img * p.tiles_per_img) * p.R;
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const int item = tid + 256 * i;
      const int win = item / CQ;
      const int wr = win / Wh, wx = win - wr * Wh;
      const int y = y0 + 2 * wr;
      const bool ok = item < nitems && y < H;
#pragma unroll
      for (int k = 0; k < 4; ++k) it[i].xv[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      it[i].dz = u32x2_t{0u, 0u};
      if (ok) {
        const size_t pix = ((size_t)img * H + y) * W + 2 * wx;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          it[i].xv[k] = *reinterpret_cast<const f32x4_t*>(p.raw + (pix + (size_t)(k >> 1) * W + (k & 1)) * NOUT + cq * 4);
        const size_t pw = ((size_t)img * (H >> 1) + (y >> 1)) * Wh + wx;
        it[i].dz = *reinterpret_cast<const u32x2_t*>(p.dz + pw * NOUT + cq * 4);
      }
    }
  };

  // d_raw of the items -> the gradient tile.  The expressions are those of pool_rederive / bn_pool_bwd_apply_kernel.
  auto form = [&](int tile, const StemItem (&it)[IPT]) {
    const int y0 = (tile % p.tiles_per_img) * p.R;
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const int item = tid + 256 * i;
      if (item >= nitems) continue;
      const int win = item / CQ;
      const int wr = win / Wh, wx = win - wr * Wh;
      const bool inside = y0 + 2 * wr < H;      // rows below the image (H % R != 0): zero positions
      float dv[4];
      dv[0] = __uint_as_float(it[i].dz.x << 16); dv[1] = __uint_as_float(it[i].dz.x & 0xffff0000u);
      dv[2] = __uint_as_float(it[i].dz.y << 16); dv[3] = __uint_as_float(it[i].dz.y & 0xffff0000u);
      float xh[4][4], best[4];
      int arg[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float a = stem_act(it[i].xv[k][e], sc[e], sh[e], p.act);
          a = to_f32<bf16_t>(from_f32<bf16_t>(a));              // through the storage format and back
          if (k == 0 || a > best[e]) { best[e] = a; arg[e] = k; }
          xh[k][e] = (it[i].xv[k][e] - m[e]) * is[e];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pre = xh[k][e] * ga[e] + be[e];
          float d = arg[e] == k ? dv[e] : 0.f;
          if (p.act == KD6D_ACT_LEAKY) d = pre > 0.f ? d : 0.1f * d;
          else if (p.act == KD6D_ACT_RELU) d = pre > 0.f ? d : 0.f;
          o[e] = ga[e] * is[e] * (d - k1[e] - xh[k][e] * k2[e]);
        }
        // pixel (2 wr + k/2, 2 wx + k%2) of the tile, in pixel order
        const int q = (2 * wr + (k >> 1)) * W + 2 * wx + (k & 1);
        const u32x2_t v = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
        *reinterpret_cast<u32x2_t*>(dyp + q * DYB + cq * 8) = inside ? v : u32x2_t{0u, 0u};
      }
    }
  };

  auto issue_patch = [&](int tile) {
    const int img = tile / p.tiles_per_img;
    const int y0 = (tile - img * p.tiles_per_img) * p.R;
    const size_t ibase = (size_t)img * H * W;
    for (int s0 = wave * 64; s0 < p.prow; s0 += 256) {
      const int pi = s0 + lane - 1;                                  // patch row 0 is a spare zero row (tap -W-3)
      const int rr = pi >= 0 ? fast_div(pi, Wp, inv_wp) : 0;
      const int xx = pi - rr * Wp - 1;
      const int y = y0 + rr - 1;
      const void* src = zero;
      if (pi >= 0 && rr < p.R + 2 && (unsigned)xx < (unsigned)W && (unsigned)y < (unsigned)H)
        src = p.x + (ibase + (size_t)y * W + xx) * 8;
      glds16(src, pat + s0 * 16);
    }
  };

  // ---- this lane's pieces of the operands ----
  const int fr = lane & 15, fq = lane >> 4, tq = fr >> 2, tp = fr & 3;
  const bool a_zero = tp * 4 >= NOUT;         // Cout = 8: rows 8 .. 15 of the image come from the zero rows of the patch
  const int a_col = tp * 8;
  const char* zrow = pat + (p.prow - 8 + tq) * PXB;      // the patch ends in 8 zero rows
  int b_add[MAXB];                            // bytes from a pixel's own patch position to this lane's piece of its tap
  bool b_zero[MAXB];
#pragma unroll
  for (int i = 0; i < MAXB; ++i) {
    const int j0 = (wave + 4 * i) * 16 + tp * 4;      // this lane's 4 columns j0 .. j0+3 share a tap
    const int tap = j0 / 8, c = j0 - tap * 8;
    b_zero[i] = j0 >= J;
    const int ky = tap / 3, kx = tap - ky * 3;
    b_add[i] = (ky * Wp + kx) * PXB + c * 2;  // patch row of padded position q under tap (ky,kx): (q + ky*Wp + kx - 1) + 1
  }
  f32x4_t acc[MAXB];
#pragma unroll
  for (int i = 0; i < MAXB; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  StemItem items[IPT];
  int tile = blockIdx.x * p.tiles_per_wg;
  int tile_end = tile + p.tiles_per_wg;
  if (tile_end > p.ntiles) tile_end = p.ntiles;
  if (tile < tile_end) fetch(tile, items);
  for (; tile < tile_end; ++tile) {
    __syncthreads();                       // the previous tile's fragment reads are done
    issue_patch(tile);
    form(tile, items);
    wait_vmcnt<0>();
    __syncthreads();
    if (tile + 1 < tile_end) fetch(tile + 1, items);      // in flight during the matrix loop
    for (int qc = 0; qc < p.Qpad; qc += 32) {
      // this lane's pixels qc + 8 fq + tq (+ 4) of the tile and their padded patch positions (row * (W+2) + column + 1)
      const int l0 = qc + 8 * fq + tq, l1 = l0 + 4;
      const int r0 = fast_div(l0, W, inv_w), r1 = fast_div(l1, W, inv_w);
      const char* x0 = pat + (l0 + 2 * r0 + 1) * PXB;
      const char* x1 = pat + (l1 + 2 * r1 + 1) * PXB;
      const bf16x8_t fa = tr_read8(a_zero ? zrow : dyp + l0 * DYB + a_col, a_zero ? zrow + 4 * PXB : dyp + l1 * DYB + a_col);
#pragma unroll
      for (int i = 0; i < MAXB; ++i) {
        if (wave + 4 * i < JB) {           // (the same for the whole wave)
          const bf16x8_t fb = tr_read8(b_zero[i] ? zrow : x0 + b_add[i], b_zero[i] ? zrow + 4 * PXB : x1 + b_add[i]);
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[i], 0, 0, 0);
        }
      }
    }
  }

  // ---- the blocks -> the [n][j] image in LDS; one partial image per workgroup ----
  __syncthreads();
  float* et = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < MAXB; ++i) {
    const int jb = wave + 4 * i;
    if (jb >= JB) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) et[(fq * 4 + r) * JP + jb * 16 + fr] = acc[i][r];
  }
  __syncthreads();
  float* part = p.dw + (size_t)blockIdx.x * (NOUT * J);
  for (int i = tid; i < NOUT * J; i += 256) {
    const int n = i / J, j = i - n * J;
    part[i] = et[n * JP + j];
  }
}

// the geometry of the call as the rule reads it
kd6d_conv::Shape stem_shape(const kd6d_conv_geom* g) {
  const int M = g->batch * g->seg[0].out_h * g->seg[0].out_w;
  return plan_shape(g, M, g->cout, g->cin, g->ksize * g->ksize * g->cin);
}

bool stem_plan(const kd6d_conv_geom* g, int dtype, int cu_budget, kd6d_conv::StemBwdPlan& pl) {
  kd6d_conv::Flags f;
  f.dtype = dtype;
  return kd6d_conv::stem_bwd_rule(stem_shape(g), f, false, plan_options(), cached_cu_count(),
                                  kd6d_conv::clamp_cu_budget(cu_budget, cached_cu_count()), pl);
}

}  // namespace

extern "C" int kd6d_bn_pool_bwd_wgrad_parts(const kd6d_conv_geom* g, int dtype, int cu_budget) {
  int rc = check_geom(g, dtype, "kd6d_bn_pool_bwd_wgrad_parts");
  if (rc) return rc;
  KD6D_CHECK_ARG(cu_budget >= 0, "kd6d_bn_pool_bwd_wgrad_parts: cu_budget=%d", cu_budget);
  kd6d_conv::StemBwdPlan pl;
  return stem_plan(g, dtype, cu_budget, pl) ? pl.parts : 0;
}

extern "C" int kd6d_bn_pool_bwd_wgrad(const kd6d_conv_geom* g, int dtype, const void* x, const float* raw, const void* dz,
                                      const float* mean, const float* invstd, const float* gamma, const float* beta,
                                      int act, const kd6d_acc* sum_dy, const kd6d_acc* sum_dy_xhat, int replicas,
                                      float* dgamma, float* dbeta, float* dw_slab, int64_t slab_floats, int cu_budget,
                                      void* stream) {
  int rc = check_geom(g, dtype, "kd6d_bn_pool_bwd_wgrad");
  if (rc) return rc;
  KD6D_CHECK_ARG(cu_budget >= 0, "kd6d_bn_pool_bwd_wgrad: cu_budget=%d", cu_budget);
  KD6D_CHECK_ARG(replicas >= 1 && replicas <= 64, "kd6d_bn_pool_bwd_wgrad: replicas=%d outside [1,64]", replicas);
  KD6D_CHECK_ARG(act == KD6D_ACT_NONE || act == KD6D_ACT_LEAKY || act == KD6D_ACT_RELU, "kd6d_bn_pool_bwd_wgrad: bad act %d", act);
  KD6D_CHECK_ARG(x && raw && dz && mean && invstd && gamma && beta && sum_dy && sum_dy_xhat && dw_slab,
                 "kd6d_bn_pool_bwd_wgrad: null pointer");
  kd6d_conv::StemBwdPlan pl;
  KD6D_CHECK_ARG(stem_plan(g, dtype, cu_budget, pl),
                 "kd6d_bn_pool_bwd_wgrad: not a stem geometry (3x3/s1/p1, cin 8, cout 8 or 16, one level of even size up to "
                 "256 wide, bf16; kd6d_bn_pool_bwd_wgrad_parts reports 0)");
  KD6D_CHECK_ARG(pl.slab_floats <= (long long)slab_floats,
                 "kd6d_bn_pool_bwd_wgrad: slab of %lld floats is too small, %lld needed (kd6d_bn_pool_bwd_wgrad_parts x cout*9*8)",
                 (long long)slab_floats, pl.slab_floats);
  StemBwdParams p;
  p.raw = raw; p.dz = reinterpret_cast<const bf16_t*>(dz); p.x = reinterpret_cast<const bf16_t*>(x);
  p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta;
  p.sum_dy = reinterpret_cast<const acc_t*>(sum_dy); p.sum_dy_xhat = reinterpret_cast<const acc_t*>(sum_dy_xhat);
  p.dgamma = dgamma; p.dbeta = dbeta; p.dw = dw_slab;
  p.replicas = replicas; p.B = g->batch; p.H = g->seg[0].in_h; p.W = g->seg[0].in_w; p.act = act;
  p.inv_rows = 1.f / (float)((long long)p.B * p.H * p.W);
  p.R = pl.R; p.tiles_per_img = pl.tiles_per_img; p.ntiles = pl.ntiles; p.Qpad = pl.Qpad; p.prow = pl.prow; p.tiles_per_wg = pl.tiles_per_wg;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (pl.NOUT == 8) launch_kernel<stem_bwd_wgrad_kernel<8>>(dim3(pl.grid), 256, pl.lds_bytes, st, p);
  else launch_kernel<stem_bwd_wgrad_kernel<16>>(dim3(pl.grid), 256, pl.lds_bytes, st, p);
  KD6D_CHECK_LAUNCH("kd6d_bn_pool_bwd_wgrad");
  return KD6D_OK;
}
