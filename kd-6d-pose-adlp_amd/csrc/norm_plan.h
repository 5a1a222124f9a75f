// The launch rules of norm_ops.hip as pure host functions: which channel counts an entry point accepts, the grid and
// the dynamic LDS bytes of every launch, which tensors take the one-launch (in-kernel barrier) backwards, and where
// the GroupNorm backward keeps its barrier counters.  No HIP include: norm_ops.hip uses these for its launches and
// tests/norm_plan_host.cpp builds the same header with g++, so every rule below is checked without a GPU.
#pragma once
#include <stdint.h>

namespace kd6d_norm {

// ---- constants the rules share with the kernels ----------------------------------------------------------------
constexpr int kThreads = 256;              // threads of every workgroup of norm_ops.hip
constexpr int kFlushLdsBytes = 16384;      // dynamic LDS of every kernel that ends in block_channel_flush or has a barrier
constexpr int kBnHold = 4;                 // granules a thread of bn_bwd_onepass_kernel keeps in registers
constexpr int kPoolHold = 2;               // 2x2 windows a thread of bn_pool_bwd_onepass_kernel keeps
constexpr int kGnHold = 8;                 // granules a thread of the GN one-pass backward keeps
constexpr int kBnOnepassBlocks = 512;      // largest grid of a BN one-launch backward
// Every workgroup of a per-channel reduction ends with one atomic per channel, and same-address atomics
// retire serially, ~27 ns each (measured: time grows linearly with the workgroup count, 512 -> 2048 = 18 -> 55 us
// on a 17-MB tensor).  colstats' plain load loop tolerates long per-thread walks, so it is capped at 128
// workgroups; the BatchNorm backward reduction is latency-bound per thread (8 granules at most) and keeps 512.
constexpr int kColstatsCap = 128;
constexpr int kBnBwdReduceCap = 512;
// rows of one (level, sample) handled by a GroupNorm reduction workgroup (GnGeom::chunk_rows)
inline int gn_chunk_rows() { return 128; }

// ---- granules and channels -------------------------------------------------------------------------------------
// elements of a 16-B granule
inline int granule_width(bool bf16) { return bf16 ? 8 : 4; }
// BatchNorm / GroupNorm / pooled entry points: thread t owns channel granule t % (C/eg) for the whole launch
inline bool channels_ok(int C, int eg) { return C > 0 && C % eg == 0 && C / eg <= kThreads && kThreads % (C / eg) == 0; }
// gn_stats_levels (the group statistics of the levels a convolution epilogue leaves out): whole granules inside a pair of groups
inline bool gn_stats_levels_ok(int C, int G, bool src_bf16) {
  const int eg = granule_width(src_bf16);
  return G >= 1 && G <= 64 && C % G == 0 && channels_ok(C, eg) && (C / G) * 2 >= eg;
}
// colstats (row-tiled ownership): any C of up to 256 granules
inline bool colstats_channels_ok(int C, int eg) { return C > 0 && C % eg == 0 && C / eg <= kThreads; }

// ---- grids -----------------------------------------------------------------------------------------------------
inline int capped_grid(long long items, long long per_workgroup, int cap) {
  long long b = (items + per_workgroup - 1) / per_workgroup;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}
// grid-stride kernels: one work item per thread, at most 2048 workgroups
inline int grid_for(long long work_items) { return capped_grid(work_items, kThreads, 2048); }
// colstats: 8 passes of 256 / (C/eg) rows per workgroup
inline int colstats_grid(long long rows, int cgs) { return capped_grid(rows, (long long)(kThreads / cgs) * 8, kColstatsCap); }
// BN backward reduction: 8 granules per thread; pooled: 2 windows (8 input granules) per thread
inline int bn_bwd_reduce_grid(long long ngran) { return capped_grid(ngran, kThreads * 8, kBnBwdReduceCap); }
inline int bn_pool_bwd_reduce_grid(long long items) { return capped_grid(items, kThreads * 2, kBnBwdReduceCap); }

// ---- dynamic LDS the kernels use, in bytes ---------------------------------------------------------------------
// block_channel_flush<NACC, EG>: `pre` and `nparts` as the kernel computes them; fp32 slots [nparts][NACC * C], or
// NACC * C two-word accumulators where a channel has more than 16 partials
inline long long flush_lds_bytes(int C, int eg, int nacc) {
  const int cgs = C / eg;
  const bool pre = cgs < 16 && (16 % cgs) == 0;
  const int nparts = pre ? kThreads / 16 : kThreads / cgs;
  return nparts > 16 ? (long long)nacc * C * 16 : (long long)nparts * nacc * C * 4;
}
// bn_bwd_apply_kernel, bn_pool_bwd_apply_kernel: the two totals per channel as floats
inline long long bn_apply_lds_bytes(int C) { return 2ll * C * 4; }
// the BN one-launch kernels: the flush (two sums), then the totals in the same space
inline long long bn_onepass_lds_bytes(int C, int eg) {
  return flush_lds_bytes(C, eg, 2) > bn_apply_lds_bytes(C) ? flush_lds_bytes(C, eg, 2) : bn_apply_lds_bytes(C);
}
// gn_relu_bwd_reduce_kernel, gn_relu_bwd_onepass_body: red[4 * C] 64-bit words in kFlushLdsBytes, so C <= kGnBwdMaxC
inline long long gn_bwd_lds_bytes(int C) { return 32ll * C; }
constexpr int kGnBwdMaxC = kFlushLdsBytes / 32;

// ---- BN backward in one launch ---------------------------------------------------------------------------------
// The two forms: what a thread holds at most, what it gets while the device has room, input granules per work item.
struct BnOnepassForm { int hold, first, granules_per_item; };
constexpr BnOnepassForm kBnPlain = {kBnHold, 2, 1};       // work item = granule
constexpr BnOnepassForm kBnPooled = {kPoolHold, 1, 4};    // work item = 2x2 window of granules
struct BnOnepassPlan { bool taken; int grid, per_thread; };
// resident: workgroups of the kernel the device keeps resident at once (0: the query failed).  The whole grid must be
// resident for the barrier, so a launch uses 3/4 of them at most, and never more than kBnOnepassBlocks.
// Largest tensor that takes it, max_granules = option bn.onepass_max.  Measured on an MI355X (tools/bench_norm.py): up
// to ~128 workgroups the barrier is cheaper than a second launch (11-13 us against 15 us per layer); at 256-512
// workgroups publishing and collecting the partial sums through device-scope returning atomics costs more than
// re-reading x and dz (27-29 us against 20 us), so those keep the pair.
inline BnOnepassPlan bn_onepass_plan(long long items, BnOnepassForm form, int resident, bool has_counter, bool enabled,
                                     long long max_granules) {
  long long cap = (long long)resident * 3 / 4;
  if (cap > kBnOnepassBlocks) cap = kBnOnepassBlocks;
  if (!(has_counter && enabled && items > 0 && cap > 0 && items <= cap * kThreads * form.hold &&
        items * form.granules_per_item <= max_granules))
    return BnOnepassPlan{false, 0, 0};
  const long long grid = capped_grid(items, (long long)kThreads * form.first, (int)cap);
  return BnOnepassPlan{true, (int)grid, (int)((items + grid * kThreads - 1) / (grid * kThreads))};
}

// ---- GN backward in one pass -----------------------------------------------------------------------------------
// Row chunks small enough for the registers of one workgroup; the workgroups of a (level, image) -- its `siblings`
// -- wait for each other, so `factor` launches' worth of the largest sibling group must be resident at once
// (2 for the single launch, 4 for the pair).
inline int gn_onepass_chunk_rows(int C, int eg) {
  const int cgs = C / eg, hold = kGnHold * kThreads / cgs;
  return gn_chunk_rows() < hold ? gn_chunk_rows() : hold;
}
struct GnOnepassPlan { int chunk_rows, siblings; bool fits; };
inline GnOnepassPlan gn_onepass_plan(int C, int eg, const int32_t* level_hw, int nseg, int resident, int factor) {
  GnOnepassPlan p = {gn_onepass_chunk_rows(C, eg), 1, false};      // >= kGnHold rows: C / eg <= kThreads
  for (int s = 0; s < nseg; ++s) {
    const int cps = (level_hw[s] + p.chunk_rows - 1) / p.chunk_rows;
    if (cps > p.siblings) p.siblings = cps;
  }
  p.fits = resident >= factor * p.siblings;
  return p;
}

// ---- GN backward workspace (gsum_ws of kd6d_gn_relu_bwd) -------------------------------------------------------
// 2 * nseg * batch * groups accumulators of 16 B, then one 32-bit barrier counter per (level, image)
struct GnBwdWorkspace { long long sums_bytes, counters_offset, total_bytes; };
inline GnBwdWorkspace gn_bwd_workspace(int nseg, int batch, int groups) {
  const long long sums = 16ll * 2 * nseg * batch * groups;
  return GnBwdWorkspace{sums, sums, sums + 4ll * nseg * batch};
}

}  // namespace kd6d_norm
