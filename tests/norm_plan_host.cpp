// Host build of csrc/norm_plan.h's launch rules for tests/test_norm_plan_host.py (g++, no GPU): the SAME header
// norm_ops.hip takes its grids, LDS sizes and one-launch decisions from.
#include "../kd-6d-pose-adlp_amd/csrc/norm_plan.h"

using namespace kd6d_norm;

extern "C" {
// kThreads, kFlushLdsBytes, kBnHold, kPoolHold, kGnHold, kBnOnepassBlocks, kColstatsCap, kBnBwdReduceCap, kGnBwdMaxC
void np_constants(int* out) {
  const int v[9] = {kThreads, kFlushLdsBytes, kBnHold, kPoolHold, kGnHold, kBnOnepassBlocks, kColstatsCap, kBnBwdReduceCap,
                    kGnBwdMaxC};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
}
int np_granule_width(int bf16) { return granule_width(bf16 != 0); }
int np_channels_ok(int C, int eg) { return channels_ok(C, eg); }
int np_colstats_channels_ok(int C, int eg) { return colstats_channels_ok(C, eg); }
int np_grid_for(long long items) { return grid_for(items); }
int np_colstats_grid(long long rows, int cgs) { return colstats_grid(rows, cgs); }
int np_bn_bwd_reduce_grid(long long ngran) { return bn_bwd_reduce_grid(ngran); }
int np_bn_pool_bwd_reduce_grid(long long items) { return bn_pool_bwd_reduce_grid(items); }
long long np_flush_lds_bytes(int C, int eg, int nacc) { return flush_lds_bytes(C, eg, nacc); }
long long np_bn_apply_lds_bytes(int C) { return bn_apply_lds_bytes(C); }
long long np_bn_onepass_lds_bytes(int C, int eg) { return bn_onepass_lds_bytes(C, eg); }
long long np_gn_bwd_lds_bytes(int C) { return gn_bwd_lds_bytes(C); }
// out = {taken, grid, per_thread}
void np_bn_onepass_plan(long long items, int pooled, int resident, int has_counter, int enabled, long long max_granules,
                        int* out) {
  const BnOnepassPlan p = bn_onepass_plan(items, pooled ? kBnPooled : kBnPlain, resident, has_counter != 0, enabled != 0,
                                          max_granules);
  out[0] = p.taken; out[1] = p.grid; out[2] = p.per_thread;
}
// out = {chunk_rows, siblings, fits}
void np_gn_onepass_plan(int C, int eg, const int32_t* level_hw, int nseg, int resident, int factor, int* out) {
  const GnOnepassPlan p = gn_onepass_plan(C, eg, level_hw, nseg, resident, factor);
  out[0] = p.chunk_rows; out[1] = p.siblings; out[2] = p.fits;
}
// out = {sums_bytes, counters_offset, total_bytes}
void np_gn_bwd_workspace(int nseg, int batch, int groups, long long* out) {
  const GnBwdWorkspace w = gn_bwd_workspace(nseg, batch, groups);
  out[0] = w.sums_bytes; out[1] = w.counters_offset; out[2] = w.total_bytes;
}
}
