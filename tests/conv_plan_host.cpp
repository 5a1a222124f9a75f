// Host build of csrc/conv_plan.h for tests/test_conv_plan_host.py (g++, no GPU): the SAME header conv_igemm.hip and
// conv_halo.hip take their kernel choice, grids, LDS sizes and launch arguments from.
#include "../kd-6d-pose-adlp_amd/csrc/conv_plan.h"

using namespace kd6d_conv;

namespace {
// shape = {M, N, C, K, ks, stride, pad, batch, nseg, then per level in_h, in_w, in_row0, out_row0}
Shape shape_of(const int* v) {
  Shape s = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], {}};
  for (int i = 0; i < s.nseg; ++i) s.seg[i] = {v[9 + 4 * i], v[10 + 4 * i], v[11 + 4 * i], v[12 + 4 * i]};
  return s;
}
// opts = {halo, halo_pairing, halo_wide, smallc, smallc_wmax, splitk, tile, wgrad_small}
Options options_of(const int* v) {
  Options o;
  o.halo = v[0]; o.halo_pairing = v[1]; o.halo_wide = v[2]; o.smallc = v[3]; o.smallc_wmax = v[4]; o.splitk = v[5];
  o.tile = v[6]; o.wgrad_small = v[7];
  return o;
}
Flags flags_of(const int* flags, long long ws_bytes) {
  Flags f;
  f.dtype = flags[0]; f.has_stats = flags[1] != 0; f.stats_groups = flags[2]; f.stats_replicas = flags[3];
  f.norm_fused = flags[4] != 0; f.xf = flags[5] != 0; f.has_workspace = flags[6] != 0; f.pair_active = flags[7] != 0;
  f.ws_bytes = ws_bytes;
  return f;
}
}  // namespace

extern "C" {
// flags = {dtype, has_stats, stats_groups, stats_replicas, norm_fused, xf, has_workspace, pair_active}
// out = {family, BP, BC, WP, WC, NSTAGE, HMAX, CG, NB, PDB, NORM, XF, grid_x, grid_y, threads, lds_bytes, n_ctiles, n_ptiles,
//        p_fastest, nk_split, nsplit, finalize_grid, halo, total_rows, patch_bytes, wbytes, fused_epilogue}
void cp_plan_conv(const int* shape, const int* flags, long long ws_bytes, const int* opts, int ncu, int dgrad, long long* out) {
  const Flags f = flags_of(flags, ws_bytes);
  const FwdPlan p = dgrad ? plan_dgrad(shape_of(shape), f, options_of(opts), ncu) : plan_fwd(shape_of(shape), f, options_of(opts), ncu);
  const long long v[27] = {p.family, p.BP, p.BC, p.WP, p.WC, p.NSTAGE, p.HMAX, p.CG, p.NB, p.PDB, p.NORM, p.XF, p.grid_x, p.grid_y,
                           p.threads, p.lds_bytes, p.n_ctiles, p.n_ptiles, p.p_fastest, p.nk_split, p.nsplit, p.finalize_grid,
                           p.halo, p.total_rows, p.patch_bytes, p.wbytes, p.fused_epilogue};
  for (int i = 0; i < 27; ++i) out[i] = v[i];
}
// cu_budget as the caller passes it (0 = the whole device)
// out = {family, BN, BJ, WN, WJ, CG, NB, KS, parts, m_chunk, n_jtiles, grid_x, grid_y, lds_bytes, R, tiles_per_img, ntiles,
//        buf_bytes, prow}
void cp_plan_wgrad(const int* shape, int dtype, int with_bias, const int* opts, int ncu, int cu_budget, long long* out) {
  Flags f;
  f.dtype = dtype; f.with_bias = with_bias != 0;
  const WgradPlan p = plan_wgrad(shape_of(shape), f, options_of(opts), ncu, clamp_cu_budget(cu_budget, ncu));
  const long long v[19] = {p.family, p.BN, p.BJ, p.WN, p.WJ, p.CG, p.NB, p.KS, p.parts, p.m_chunk, p.n_jtiles, p.grid_x, p.grid_y,
                           p.lds_bytes, p.R, p.tiles_per_img, p.ntiles, p.buf_bytes, p.prow};
  for (int i = 0; i < 19; ++i) out[i] = v[i];
}
// the group-statistics table of the forward launch planned for (shape, flags): flags[2] groups
// out = {keys per tile the planned kernel's LDS holds, most keys any tile touches (the walk), stats_table_fits,
//        bytes of the table at that many keys, the plan's lds_bytes}
void cp_stats_table(const int* shape, const int* flags, const int* opts, int ncu, long long* out) {
  const Shape s = shape_of(shape);
  const Flags f = flags_of(flags, 0);
  const FwdPlan p = plan_fwd(s, f, options_of(opts), ncu);
  const int cs = s.N / f.stats_groups == 8 ? 3 : 2;
  out[0] = stats_table_max_keys(p, s.N, f.stats_groups);
  out[1] = stats_tile_keys(s, p.BP, -1);
  out[2] = stats_table_fits(s, p, f.stats_groups);
  out[3] = stats_table_bytes(p.BP, p.BC, cs, (int)out[1]);
  out[4] = p.lds_bytes;
}
int cp_stats_row_key(const int* shape, int m) { return stats_row_key(shape_of(shape), m); }
int cp_stats_level_skipped(int dst_hw, int m_begin) { return stats_level_skipped(dst_hw, m_begin); }
int cp_stats_followup_ok(int cout, int groups, int dst_f32) { return stats_followup_ok(cout, groups, dst_f32 != 0); }
int cp_stats_groups_ok(int cout, int groups) { return stats_channels_ok(cout) && stats_groups_ok(cout, groups); }
int cp_norm_fusable(const int* shape, const int* out_hw, int dtype, int kind, int groups, int fuse_norm, int pair_active,
                    const int* opts, int ncu) {
  return norm_fusable(shape_of(shape), out_hw, dtype, kind, groups, fuse_norm, pair_active != 0, options_of(opts), ncu);
}
// the variant lists, as rows of 6 ints (unused columns 0); returns the number of rows
int cp_variants(int list, int* out) {
  int n = 0;
  auto row = [&](int a, int b, int c, int d, int e, int f) {
    const int v[6] = {a, b, c, d, e, f};
    for (int i = 0; i < 6; ++i) out[6 * n + i] = v[i];
    ++n;
  };
#define R4(a, b, c, d) row(a, b, c, d, 0, 0);
#define R5(a, b, c, d, e) row(a, b, c, d, e, 0);
#define R6(a, b, c, d, e, f) row(a, b, c, d, e, f);
#define R2(a, b) row(a, b, 0, 0, 0, 0);
#define R3(a, b, c) row(a, b, c, 0, 0, 0);
  switch (list) {
    case 0: KD6D_CONV_IGEMM_TILES(R4) break;
    case 1: KD6D_CONV_GLDS_TILES(R5) break;
    case 2: KD6D_CONV_SPLITK_TILES(R5) break;
    case 3: KD6D_CONV_SMALLC_TILES(R2) break;
    case 4: KD6D_CONV_HALO_TILES(R6) break;
    case 5: KD6D_CONV_HALO_NORM_TILES(R6) break;
    case 6: KD6D_CONV_WGRAD_TILES(R4) break;
    case 7: KD6D_CONV_WGRAD_TR_TILES(R3) break;
    case 8: KD6D_CONV_WGRAD_SMALL_TILES(R3) break;
    default: break;
  }
  return n;
}
}
