// The per-layer convolution kernel choice as pure host functions: which kernel family and tile a
// forward / data-gradient / weight-gradient call runs, with what grid, block and dynamic LDS, and every derived value
// the launch passes to the kernel.  No HIP include, no library state: conv_igemm.hip and conv_halo.hip plan with
// plan_fwd / plan_dgrad / plan_wgrad and only launch what the plan says; tests/conv_plan_host.cpp builds the same
// header with g++, so "what would this layer run" is answered -- and tested -- without a GPU.
#ifndef KD6D_CONV_PLAN_H_
#define KD6D_CONV_PLAN_H_
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "norm_plan.h"

namespace kd6d_conv {

// ---- constants the rules share with the kernels and entry points -----------------------------------------------
constexpr int kMaxSeg = 5;                 // KD6D_MAX_SEG
constexpr int kNormMaxCtiles = 8;          // KD6D_NORM_MAX_CTILES
constexpr int kLdsPerCu = 160 << 10;       // bytes of LDS of one CU
constexpr int kWaveSlotsPerCu = 32;
enum { kBf16 = 0, kF32 = 1 };              // KD6D_BF16, KD6D_F32
enum { kFwd = 0, kDgrad = 1 };             // MODE_FWD, MODE_DGRAD
enum { kNormGroup = 1, kNormBatch = 2 };   // KD6D_NORM_GROUP, KD6D_NORM_BATCH

// ---- inputs ----------------------------------------------------------------------------------------------------
struct Level { int in_h, in_w, in_row0, out_row0; };       // forward sense, as kd6d_seg
// The GEMM of the call.  fwd: C = cin, N = cout; dgrad: C = cout, N = cin; wgrad: C = cin, N = cout; K = ks * ks * C;
// M = destination pixels (fwd / wgrad: output grid, dgrad: input grid).
struct Shape {
  int M, N, C, K, ks, stride, pad, batch, nseg;
  Level seg[kMaxSeg];
};
struct Flags {
  int dtype = kBf16, mode = kFwd;
  bool has_stats = false;          // fused statistics of the stored values
  int stats_groups = 0, stats_replicas = 0;
  bool norm_fused = false;         // normalisation + activation behind the convolution (ConvParams::norm_dst)
  bool xf = false;                 // BatchNorm of the previous block applied on load
  bool has_workspace = false;      // split-K slabs
  long long ws_bytes = 0;
  bool with_bias = false;          // wgrad: a bias gradient is asked for
  bool pair_active = false;        // inside a kd6d_conv2d_pair_begin/_end bracket
};
struct Options {                   // kd6d_set_option values (kd6d_common.h)
  int halo = -1, halo_pairing = 1, halo_wide = 1, smallc = -1, smallc_wmax = 640, splitk = -1, tile = -1, wgrad_small = -1;
  int stem_fused = 1;
};

// ---- kernel variants: the one list of each family; the launchers expand their instantiations from these ----------
// register-staged kernel, X(BP, BC, WP, WC)
#define KD6D_CONV_IGEMM_TILES(X) \
  X(256, 16, 4, 1) X(64, 16, 4, 1) X(256, 32, 4, 1) X(64, 32, 4, 1) X(128, 64, 2, 2) X(64, 64, 2, 2) X(128, 128, 2, 2)
// LDS-DMA kernel, X(BP, BC, WP, WC, NSTAGE)
#define KD6D_CONV_GLDS_TILES(X) X(128, 128, 2, 2, 3) X(128, 64, 2, 2, 3) X(64, 64, 2, 2, 4) X(64, 64, 2, 2, 6)
// its split-K form (forward only), X(BP, BC, WP, WC, NSTAGE)
#define KD6D_CONV_SPLITK_TILES(X) X(128, 64, 2, 2, 3) X(64, 64, 2, 2, 3)
// resident-patch kernel, X(CG, NB): 8 * CG source channels, 16 * NB result channels per tile
#define KD6D_CONV_SMALLC_TILES(X) \
  X(1, 1) X(1, 2) X(1, 4) X(1, 8) X(2, 1) X(2, 2) X(2, 4) X(2, 8) X(4, 1) X(4, 2) X(4, 4) X(4, 8)
// halo-patch kernel, X(BP, BC, WP, WC, HMAX, PDB); forward and data gradient
#define KD6D_CONV_HALO_TILES(X) \
  X(128, 128, 2, 2, 33, false) X(128, 128, 4, 2, 33, false) X(128, 64, 4, 2, 33, false) X(64, 64, 4, 2, 33, false) \
  X(128, 32, 4, 1, 33, false) \
  X(256, 128, 4, 2, 81, true) X(128, 128, 4, 2, 81, true) X(128, 64, 4, 2, 81, true) X(128, 32, 4, 1, 81, true) \
  X(64, 64, 4, 2, 81, true) \
  X(256, 128, 4, 2, 65, true) X(128, 128, 4, 2, 65, true) X(128, 64, 4, 2, 65, true) X(128, 32, 4, 1, 65, true) \
  X(192, 128, 4, 2, 65, true) X(64, 64, 4, 2, 65, true) X(128, 128, 2, 2, 65, true)
// ... with the fused-normalisation epilogue: forward only
#define KD6D_CONV_HALO_NORM_TILES(X) X(128, 128, 4, 2, 81, true) X(128, 128, 4, 2, 65, true) X(128, 128, 4, 2, 33, false)
// weight gradient, fp32: X(BN, BJ, WN, WJ); bf16 (transposing loader, BJ = 128): X(BN, WN, WJ)
#define KD6D_CONV_WGRAD_TILES(X) X(16, 128, 1, 4) X(32, 128, 1, 4) X(64, 64, 2, 2) X(128, 128, 2, 2)
#define KD6D_CONV_WGRAD_TR_TILES(X) X(16, 1, 4) X(32, 1, 4) X(64, 1, 4) X(128, 2, 2)
// narrow weight gradient, X(CG, NB, KS)
#define KD6D_CONV_WGRAD_SMALL_TILES(X) \
  X(1, 1, 3) X(1, 2, 3) X(1, 4, 3) X(2, 1, 3) X(2, 2, 3) X(2, 4, 3) X(4, 1, 3) X(4, 2, 3) X(4, 4, 3) \
  X(1, 1, 1) X(2, 1, 1) X(4, 1, 1) X(1, 2, 1) X(2, 2, 1) X(4, 2, 1) X(1, 4, 1) X(2, 4, 1) X(4, 4, 1)

// ---- outputs ---------------------------------------------------------------------------------------------------
enum Family { kNone = -1, kSmallc = 0, kHalo, kSplitk, kGlds, kIgemm };
struct FwdPlan {
  int family = kNone, dtype = kBf16, mode = kFwd;
  // the variant: tile BP x BC of WP x WC waves (+ NSTAGE | HMAX, PDB), or CG / NB of the resident-patch kernel
  int BP = 0, BC = 0, WP = 0, WC = 0, NSTAGE = 0, HMAX = 0, CG = 0, NB = 0;
  bool PDB = false, NORM = false, XF = false;
  int grid_x = 0, grid_y = 1, threads = 0;
  long long lds_bytes = 0;
  // what the launch puts into ConvParams or passes as kernel arguments
  int n_ctiles = 0, n_ptiles = 0, p_fastest = 0;
  int nk_split = 0, nsplit = 0, finalize_grid = 0;                       // split-K
  int halo = 0, total_rows = 0, patch_bytes = 0, wbytes = 0;             // halo-patch / resident-patch
  bool fused_epilogue = false;     // the kernel ends in conv_epilogue_full (fused normalisation, replica rows)
};
enum WgradFamily { kWgNone = -1, kWgSmall = 0, kWgTr, kWgGeneric };
struct WgradPlan {
  int family = kWgNone;
  int BN = 0, BJ = 0, WN = 0, WJ = 0;      // tr / generic tile
  int CG = 0, NB = 0, KS = 0;              // small
  int parts = 0, m_chunk = 0, n_jtiles = 0, grid_x = 0, grid_y = 1;
  long long lds_bytes = 0;
  int R = 0, tiles_per_img = 0, ntiles = 0, buf_bytes = 0, prow = 0;      // small
};
// BatchNorm + max-pool backward fused into the weight gradient (stem_bwd.hip): a block whose input needs no gradient
struct StemBwdPlan {
  int NOUT = 0;                            // the variant: result channels, 8 or 16
  int R = 0, tiles_per_img = 0, ntiles = 0, Qpad = 0, prow = 0, tiles_per_wg = 0;
  int grid = 0, parts = 0;                 // workgroups = partial dW images
  long long lds_bytes = 0, slab_floats = 0;
};

// ---- shared arithmetic -----------------------------------------------------------------------------------------
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int nblocks(const Shape& s, int bp, int bc) { return ceil_div(s.M, bp) * ceil_div(s.N, bc); }

// Workgroup order.  After the XCD remap an XCD runs a CONTIGUOUS range of ~1/8 of the tile ids, so the
// fastest-varying tile index decides which operand that XCD's 4 MiB L2 can keep: channel tiles fastest
// -> the XCD touches few pixel tiles but ALL weights; pixel tiles fastest -> few weight tiles but many
// pixels.  Pick the order with the smaller per-XCD footprint (small-M / wide-N layers: weights).
inline int p_fastest(const Shape& s, int ptiles, int ctiles, int BP, int BC) {
  const double tiles = (double)ptiles * ctiles;
  const double per_xcd = tiles / 8.0;
  const double w_tile = (double)BC * s.K * 2.0, x_tile = (double)BP * s.C * 2.0 * (s.ks > 1 ? 1.5 : 1.0);
  // channel tiles fastest: an XCD spans per_xcd / n_ctiles pixel tiles (>= 1) and min(per_xcd, n_ctiles) weight tiles
  auto foot = [&](double n_fast, double t_fast, double t_slow) {
    const double fast = per_xcd < n_fast ? per_xcd : n_fast;
    const double slow = per_xcd / n_fast < 1.0 ? 1.0 : per_xcd / n_fast;
    return fast * t_fast + slow * t_slow;
  };
  const double c_fast = foot(ctiles, w_tile, x_tile);
  const double p_fast = foot(ptiles, x_tile, w_tile);
  return p_fast < c_fast ? 1 : 0;
}

// tile counts, order and the one-dimensional grid of a BP x BC tiling
inline void set_tiles(FwdPlan& pl, const Shape& s, int BP, int BC, int WP, int WC, bool ordered = true) {
  pl.BP = BP; pl.BC = BC; pl.WP = WP; pl.WC = WC;
  pl.n_ctiles = ceil_div(s.N, BC);
  pl.n_ptiles = ceil_div(s.M, BP);
  pl.p_fastest = ordered ? p_fastest(s, pl.n_ptiles, pl.n_ctiles, BP, BC) : 0;
  pl.grid_x = pl.n_ptiles * pl.n_ctiles;
  pl.threads = WP * WC * 64;
}

// both sides of every level packed identically and back to back (the patch kernels address source and destination
// rows alike); reports the widest level and the total rows
inline bool packed_alike(const Shape& s, int* wmax, int* rows) {
  *wmax = 0; *rows = 0;
  for (int i = 0; i < s.nseg; ++i) {
    const Level& q = s.seg[i];
    if (q.in_row0 != q.out_row0 || q.in_row0 != *rows) return false;
    if (q.in_w > *wmax) *wmax = q.in_w;
    *rows += s.batch * q.in_h * q.in_w;
  }
  return true;
}

// ---- dynamic LDS, in bytes: each formula once --------------------------------------------------------------------
// register-staged kernel: the two operand tiles, double-buffered (+ XF: scale and shift per source channel)
inline long long igemm_lds(int BP, int BC, bool XF, int C) { return (long long)(BP + BC) * 256 + (XF ? 8ll * C : 0); }
// LDS-DMA kernel and its split-K form: a ring of NSTAGE stages
inline long long glds_lds(int BP, int BC, int NSTAGE) { return (long long)(BP + BC) * 128 * NSTAGE; }
// halo-patch kernel: 3 weight stages + 2 patch buffers (PDB) or 1 (as halo_tile lays them out)
inline long long halo_lds(int BP, int BC, int WP, int WC, int HMAX, bool PDB) {
  const int NW = WP * WC;
  const int PSLOT = (BP + 2 * HMAX + 7) / 8 + 1;
  const int PL = (PSLOT + NW - 1) / NW;
  return (PDB ? 2ll * PL * NW : (long long)PSLOT) * 1024 + 3ll * BC * 128;
}
// resident-patch kernel: patch rows [m0 - halo, m0 + 256 + halo) + the zero row, padded to whole 1-KB LDS-DMA bursts,
// the weights, 256 row offsets; or the statistics scratch of the epilogue
inline void smallc_lds(FwdPlan& pl, int CG, int NB, int halo) {
  const int BP = 256, BC = 16 * NB;
  const int NKC = (9 * 8 * CG + 31) / 32, WG = NKC * 4 + 1;
  pl.patch_bytes = ((BP + 2 * halo + 1) * 16 * CG + 1023) / 1024 * 1024;
  pl.wbytes = (BC * WG + 63) / 64 * 1024;
  const long long lds = (long long)pl.patch_bytes + pl.wbytes + 256 * 4;
  const long long epi = 2ll * BC * 4 + 4096;
  pl.lds_bytes = lds < epi ? epi : lds;
}
// weight gradient: fp32 kernel: both operand tiles double-buffered; transposing bf16 kernel: stages or the epilogue image
inline long long wgrad_lds(int BN, int BJ) { return (long long)(BN + BJ) * 256; }
inline long long wgrad_tr_lds(int BN) {
  const long long stage = 2ll * 2 * 64 * 256, epi = (long long)BN * (128 + 4) * 4;
  return stage > epi ? stage : epi;
}
// narrow weight gradient: two buffers of R map rows (dY tile + source patch), or the flush's [n][j] image
inline void wgrad_small_lds(WgradPlan& pl, int W) {
  const int Wp = pl.KS == 3 ? W + 2 : W;
  const int Qpad = (pl.R * Wp + 31) & ~31;
  int prow = Qpad + (pl.KS == 3 ? 2 * Wp + 3 : 0) + 8;          // furthest tap of the last position + 8 zero rows
  const int unit = 64 / pl.CG;                                  // whole 1-KB LDS-DMA bursts
  pl.prow = (prow + unit - 1) / unit * unit;
  pl.buf_bytes = Qpad * 32 * pl.NB + pl.prow * 16 * pl.CG;
  const int JB = (pl.KS * pl.KS * 8 * pl.CG + 15) / 16;
  const long long image = (long long)pl.NB * 16 * JB * 16 * 4;
  pl.lds_bytes = 2ll * pl.buf_bytes > image ? 2ll * pl.buf_bytes : image;
}

// ---- forward / data-gradient family rules: false = "not mine" ---------------------------------------------------
// 3x3/s1/p1 layers with 8, 16 or 32 gather-source channels on maps up to 256 wide, both sides packed identically.
inline bool smallc_rule(const Shape& p, const Flags& f, const Options& o, FwdPlan& pl) {
  const int force = o.smallc;
  if (force == 0) return false;
  if (p.ks != 3 || p.stride != 1 || p.pad != 1 || (p.C != 8 && p.C != 16 && p.C != 32) || (p.N & 3)) return false;
  if (f.has_stats && f.stats_groups > 0) return false;      // the group-statistics table wants the big staging buffers
  if (f.norm_fused || f.stats_replicas > 1) return false;   // no fused-normalisation epilogue / replica rows in this kernel
  // one burst per workgroup, no pipeline: pays once >= 2 workgroups per CU overlap each other (measured: the
  // 64x64-pixel layers and below are faster on the pipelined kernels)
  if (force < 0 && p.M < (1 << 17)) return false;
  int wmax, rows;
  if (!packed_alike(p, &wmax, &rows)) return false;
  // the patch is 256 pixels + a halo of (width + 1) rows on either side: up to 256-wide maps always (the size the kernel
  // was tuned on), wider ones (the 640- and 320-wide levels of full frames) while it stays within 32 KB, i.e. 8 or 16
  // channels -- read amplification (256 + 2 halo) / 256 grows to 6x at 640, all of it L2 hits, against 9 taps on the
  // generic kernels: 480 x 640 x 8 -> 32 forward 298 -> 165 us, 8 -> 8 forward / dgrad 266 / 289 -> 78 / 79,
  // 240 x 320 x 8 -> 16 71 / 90 -> 24 / 33; with 32 channels (57 KB, one or two workgroups per CU) 129 -> 216, excluded
  if (wmax > 256 && (wmax > o.smallc_wmax || (256 + 2 * (wmax + 1) + 1) * 2 * p.C > 32768)) return false;
  pl.family = kSmallc;
  pl.CG = p.C / 8;
  pl.NB = p.N <= 16 ? 1 : (p.N <= 32 ? 2 : (p.N <= 64 ? 4 : 8));
  set_tiles(pl, p, 256, 16 * pl.NB, 4, 1, false);
  pl.halo = wmax + 1; pl.total_rows = rows;
  smallc_lds(pl, pl.CG, pl.NB, pl.halo);
  return true;
}

// 3x3/s1/p1 layers with C % 64 == 0 on maps at most 80 wide, both sides packed identically.
inline bool halo_rule(const Shape& p, const Flags& f, const Options& o, int ncu, FwdPlan& pl) {
  const int force = o.halo;
  if (force == 0) return false;
  if (p.ks != 3 || p.stride != 1 || p.pad != 1 || (p.C & 63) || (p.N & 3)) return false;
  if (p.N < 64 && p.N > 32) return false;
  if (!f.norm_fused && f.stats_replicas > 1) return false;      // replica rows of the batch statistics: register-staged kernel
  int wmax, rows;
  if (!packed_alike(p, &wmax, &rows)) return false;
  if (wmax > (o.halo_wide != 0 ? 80 : 64)) return false;      // (80: the 60 x 80 level of 480 x 640 full frames)
  const int halo = wmax + 1;
  // measured on the step's layers (tools/bench_conv.py), all variants with 8 waves (2 per SIMD: with 4 waves
  // the same 128x128 tile is 25-40 % slower, one wave per SIMD cannot hide the LDS-DMA / fragment latency):
  //   256x128 once it yields >= 150 workgroups (teacher head, stage 2);
  //   128x128 from >= 160 workgroups (teacher stage 3, FPN 32x32 level, student head towers fwd + dgrad);
  //   128x64  from >= 64 workgroups (teacher stage 4, student FPN 32x32 level) -- ahead of split-K;
  //   192x128 / 64x64 / 128x32: the tile-count corner cases below;
  // below that the layer goes to split-K / the generic kernels.
  // inside a kd6d_conv2d_pair_begin/_end bracket the launch shares the device with its twin: count tiles twice
  const int pf = f.pair_active ? 2 : 1;
  const int pt128 = pf * ceil_div(p.M, 128);
  int pick = 0;
  const int ct128 = ceil_div(p.N, 128);
  const int ct64 = ceil_div(p.N, 64);
  // few result channels (cls logits, dgrad into the narrow student stages): 128 x 32, or 64 x 64 on small maps
  if (p.N <= 32) pick = pt128 <= ncu / 2 ? 9 : 5;
  // 128 x 64 tiles would occupy at most half of the CUs: 64 x 64 (FPN 16x16 level, stage 5, student FPN)
  else if (pt128 * ct64 <= ncu / 2 && pf * ceil_div(p.M, 64) * ct64 >= 64) pick = 9;
  // 192 x 128 where it turns 256-pixel tiles that leave a third of the CUs idle into one full round (teacher head
  // towers: 172 tiles of 256 pixels on 256 CUs -> 228 tiles of 192)
  else if (pf * ceil_div(p.M, 256) * ct128 >= 150 && pf * ceil_div(p.M, 256) * ct128 <= (3 * ncu) / 4 &&
           pf * ceil_div(p.M, 192) * ct128 <= ncu) pick = 6;
  else if (pf * ceil_div(p.M, 256) * ct128 >= 150) pick = 1;
  else if (pt128 * ct128 >= 160) pick = 3;
  else if (pt128 * ct64 >= 64) pick = 4;
  // maps up to 32 wide (halo <= 33): the single-patch-buffer twin of the picked tile, 38-74 KB of LDS instead of
  // 104-144, so that two workgroups -- of this launch or of the other stream's -- share a CU.  Alone on the device a
  // twin is as fast as its original or up to 40 % slower (chunk-boundary stalls, no partner to cover them); inside
  // the step the pairs give +4 % (4889-4918 -> 5097 images/s, interleaved runs; profiles/r02_halo_pairing.md)
  if (o.halo_pairing != 0 && halo <= 33) {
    // (96 x 128 tiles for the 342-tile tower shape -- 456 tiles on 512 slots instead of 86 CUs carrying two tiles of 128 x
    //  128 and 170 one -- were built and measured in round 3: 5064-5099 against 5184-5192 images/s, interleaved; removed)
    // (256 x 128, one workgroup per CU, is what the counts above pick from ~40 000 rows on -- the teacher's towers over
    //  the 32 images of a grouped pass: 2.25 us per image against 1.75 for the twins, 1.91 for 192 x 128; tools/bench_conv.py
    //  --batch 32 --opt conv.halo=N)
    if (pick == 3 || pick == 6 || pick == 1) pick = 12;
    else if (pick == 4) pick = 13;
    else if (pick == 9) pick = 14;
    else if (pick == 5) pick = 15;
  }
  if (force > 0 && (force < 10 || halo <= 33)) pick = force;      // 11..15: the twins, maps <= 32 wide only
  if (pick == 0) return false;
  auto take = [&](int BP, int BC, int WP, int WC, int HMAX, bool PDB, bool NORM) {
    pl.family = kHalo;
    set_tiles(pl, p, BP, BC, WP, WC);
    pl.HMAX = HMAX; pl.PDB = PDB; pl.NORM = NORM; pl.fused_epilogue = NORM;
    pl.halo = halo; pl.total_rows = rows;
    pl.lds_bytes = halo_lds(BP, BC, WP, WC, HMAX, PDB);
    return true;
  };
  if (f.norm_fused) {
    // a fused normalisation behind the convolution (kd6d_conv2d_fwd_norm): compiled into the 128 x 128 forward tiles only
    if (f.mode != kFwd) return false;
    if (halo > 65) return take(128, 128, 4, 2, 81, true, true);
    if (halo > 33 || o.halo_pairing == 0) return take(128, 128, 4, 2, 65, true, true);
    return take(128, 128, 4, 2, 33, false, true);
  }
  if (pick == 11) return take(128, 128, 2, 2, 33, false, false);
  if (pick == 12) return take(128, 128, 4, 2, 33, false, false);
  if (pick == 13) return take(128, 64, 4, 2, 33, false, false);
  if (pick == 14) return take(64, 64, 4, 2, 33, false, false);
  if (pick == 15) return take(128, 32, 4, 1, 33, false, false);
  // maps 65 ... 80 wide: the same tiles with the patch sized for a halo of 81 rows (the 256 x 128 tile then takes
  // exactly the CU's 160 KB); 192 x 128 and the 4-wave tile have no such form: 128 x 128
  const int HMAX = halo > 65 ? 81 : 65;
  if (pick == 1) return take(256, 128, 4, 2, HMAX, true, false);
  if (pick == 3) return take(128, 128, 4, 2, HMAX, true, false);      // 8 waves on the 128x128 tile
  if (pick == 4) return take(128, 64, 4, 2, HMAX, true, false);
  if (pick == 5) return take(128, 32, 4, 1, HMAX, true, false);
  if (pick == 9) return take(64, 64, 4, 2, HMAX, true, false);
  if (HMAX == 81) return take(128, 128, 4, 2, 81, true, false);
  if (pick == 6) return take(192, 128, 4, 2, 65, true, false);
  return take(128, 128, 2, 2, 65, true, false);
}

// Split-K for the layers whose output yields too few tiles to fill 256 CUs while K is long (teacher
// stages 4/5, FPN top: M <= 4096, K = 2304..9216): partial tiles go to fp32 slabs in the caller's
// workspace (plain 16-B stores, no atomics), a small second launch sums them and applies the epilogue.
inline bool splitk_rule(const Shape& p, const Flags& f, const Options& o, FwdPlan& pl) {
  const int force = o.splitk;
  if (force == 0 || !f.has_workspace || f.has_stats || (p.N & 3) || p.N <= 32) return false;
  const int nk = ceil_div(p.K, 64);
  int tile = 0, ns = 0;
  if (force > 0) { tile = force / 100; ns = force % 100; }
  else if (nk >= 16 && nblocks(p, 64, 64) <= 320) {
    tile = 2;
    ns = 768 / nblocks(p, 64, 64);
    if (ns > nk / 6) ns = nk / 6;
    if (ns > 16) ns = 16;
  }
  if (tile == 0 || ns < 2) return false;
  // (the workspace is checked against the count asked for, before the count is recomputed from whole k-steps)
  if ((size_t)ns * p.M * p.N * sizeof(float) > (size_t)(f.ws_bytes > 0 ? f.ws_bytes : 0)) return false;
  pl.family = kSplitk;
  set_tiles(pl, p, tile == 1 ? 128 : 64, 64, 2, 2);
  pl.NSTAGE = 3;
  pl.nk_split = ceil_div(nk, ns);
  pl.nsplit = ceil_div(nk, pl.nk_split);
  pl.grid_y = pl.nsplit;
  pl.lds_bytes = glds_lds(pl.BP, pl.BC, pl.NSTAGE);
  const long long total = (long long)p.M * (p.N >> 2);
  pl.finalize_grid = (int)((total + 255) / 256);
  if (pl.finalize_grid > 2048) pl.finalize_grid = 2048;
  return true;
}

// bf16, N > 32: LDS-DMA kernel.  Tile by how many workgroups the layer yields (256 CUs).
inline bool glds_rule(const Shape& p, const Flags& f, const Options& o, FwdPlan& pl) {
  const int force = o.tile;
  if (force == 0 || p.N <= 32) return false;
  // launches with a fused normalisation (kd6d_conv2d_fwd_norm) or replica rows of the batch statistics take the
  // register-staged kernel: this one is not compiled with that epilogue (and its 64-KB rings would not leave a
  // grid-barrier launch room to be resident at once)
  if (f.norm_fused || f.stats_replicas > 1) return false;
  // measured (tools/bench_conv.py): with enough workgroups the register-staged kernel is as fast or faster
  // (several workgroups per CU hide the load round trip); the layers with <= ~1 workgroup per CU and a long
  // K (teacher stages 4/5, FPN top) are bound by that round trip and gain from a deep LDS-DMA ring
  int pick = 0;
  if (nblocks(p, 128, 64) < 384) pick = 3;
  else if (nblocks(p, 128, 64) <= 640 && p.K >= 1024) pick = 2;       // stride-2 stage-3 entry: 28 -> 25 us
  // k-steps that straddle taps (source channels not a multiple of 64) pay a tap decode per step here; on the
  // large maps (dgrad of the student's cls / pose heads) the register-staged kernel is 15-25 % faster
  if (pick == 3 && (p.C & 63) && p.M > 16384) pick = 0;
  if (force > 0) pick = force;
  if (pick == 0) return false;
  pl.family = kGlds;
  if (pick == 1) { set_tiles(pl, p, 128, 128, 2, 2); pl.NSTAGE = 3; }
  else if (pick == 2) { set_tiles(pl, p, 128, 64, 2, 2); pl.NSTAGE = 3; }
  else if (pick == 3) { set_tiles(pl, p, 64, 64, 2, 2); pl.NSTAGE = 4; }
  else { set_tiles(pl, p, 64, 64, 2, 2); pl.NSTAGE = 6; }
  pl.lds_bytes = glds_lds(pl.BP, pl.BC, pl.NSTAGE);
  return true;
}

// register-staged kernel: takes every layer
inline void igemm_rule(const Shape& p, const Flags& f, FwdPlan& pl) {
  pl.family = kIgemm;
  if (p.N <= 16) {
    if (nblocks(p, 256, 16) >= 512) set_tiles(pl, p, 256, 16, 4, 1);
    else set_tiles(pl, p, 64, 16, 4, 1);
  } else if (p.N <= 32) {
    if (nblocks(p, 256, 32) >= 512) set_tiles(pl, p, 256, 32, 4, 1);
    else set_tiles(pl, p, 64, 32, 4, 1);
  } else if (p.N <= 64) {
    if (nblocks(p, 128, 64) >= 384) set_tiles(pl, p, 128, 64, 2, 2);
    else set_tiles(pl, p, 64, 64, 2, 2);
  } else {
    if (nblocks(p, 128, 128) >= 384) set_tiles(pl, p, 128, 128, 2, 2);
    else if (nblocks(p, 128, 64) >= 384) set_tiles(pl, p, 128, 64, 2, 2);
    else set_tiles(pl, p, 64, 64, 2, 2);
  }
  pl.XF = f.xf;
  // the fused-normalisation epilogue exists in the forward, non-XF variants only (kd6d_conv2d_fwd_norm), and so do
  // the replica rows of the fused batch statistics (kd6d_conv2d_fwd_block)
  pl.NORM = f.mode == kFwd && !f.xf && (f.norm_fused || f.stats_replicas > 1);
  pl.fused_epilogue = pl.NORM;
  pl.lds_bytes = igemm_lds(pl.BP, pl.BC, pl.XF, p.C);
}

// the forward chain; bf16: smallc -> halo -> splitk -> glds -> igemm; fp32 and BatchNorm-on-load: igemm only
inline FwdPlan plan_fwd(const Shape& p, Flags f, const Options& o, int ncu) {
  f.mode = kFwd;
  FwdPlan pl;
  pl.dtype = f.dtype; pl.mode = kFwd;
  if (f.dtype == kBf16 && !f.xf &&
      (smallc_rule(p, f, o, pl) || halo_rule(p, f, o, ncu, pl) || splitk_rule(p, f, o, pl) || glds_rule(p, f, o, pl)))
    return pl;
  igemm_rule(p, f, pl);
  return pl;
}
// the data gradient: the same without split-K
inline FwdPlan plan_dgrad(const Shape& p, Flags f, const Options& o, int ncu) {
  f.mode = kDgrad;
  FwdPlan pl;
  pl.dtype = f.dtype; pl.mode = kDgrad;
  if (f.dtype == kBf16 && (smallc_rule(p, f, o, pl) || halo_rule(p, f, o, ncu, pl) || glds_rule(p, f, o, pl))) return pl;
  igemm_rule(p, f, pl);
  return pl;
}

// ---- fused statistics and the conv + normalisation launch ---------------------------------------------------------
// the channel counts the fused statistics take: cout % 4 == 0; groups of 4 or 8 channels
inline bool stats_channels_ok(int cout) { return cout % 4 == 0; }
inline bool stats_groups_ok(int cout, int groups) {
  return groups == 0 || (groups > 0 && cout % groups == 0 && (cout / groups) % 4 == 0 && cout / groups <= 8);
}
// group statistics: bit s set = level s is NOT summed by the epilogue, which sums whole 16-row fragments that lie inside
// one image (dst_hw, m_begin: pixels of the level's destination grid and its first GEMM row)
inline bool stats_level_skipped(int dst_hw, int m_begin) { return (dst_hw % 16) != 0 || (m_begin % 16) != 0; }
// ... such levels are summed from the stored tensor by a gn_stats launch behind the convolution (stats_followup), which has
// channel rules of its own (norm_plan.h: cout / 4 -- cout / 8 for a bf16 tensor -- divides 256): kd6d_conv2d_fwd refuses a
// call with a skipped level that the follow-up would not take, before it launches anything
inline bool stats_followup_ok(int cout, int groups, bool dst_f32) { return kd6d_norm::gn_stats_levels_ok(cout, groups, !dst_f32); }

// Group statistics, the LDS image of conv_epilogue_stats in the kernel's dead staging memory: the accumulator table
// [key of the tile][group of the channel tile] of {sum, sumsq}, 16 bytes each, the staged entries (one f32x2 per 4-channel
// slice of a 16-row fragment: BP * BC / 64 of them) and one key per fragment row.  `nkeys` counts EVERY (level, image) key
// between the tile's first and last row, the levels the epilogue skips included.
inline long long stats_table_bytes(int BP, int BC, int cpg_shift, int nkeys) {
  return (long long)nkeys * (BC >> cpg_shift) * 32 + (long long)BP * BC / 8 + BP / 4;
}
// pixels of level i's destination grid (forward sense)
inline int out_pixels(const Shape& s, int i) {
  return ((s.seg[i].in_h + 2 * s.pad - s.ks) / s.stride + 1) * ((s.seg[i].in_w + 2 * s.pad - s.ks) / s.stride + 1);
}
// (level, image) key of forward GEMM row m: the host form of the kernels' stats_key
inline int stats_row_key(const Shape& s, int m) {
  int key = 0;
  for (int i = 0, mb = 0; i < s.nseg; ++i) {
    const int hw = out_pixels(s, i);
    if (m >= mb) key = i * s.batch + (m - mb) / hw;
    mb += s.batch * hw;
  }
  return key;
}
// the most keys any tile of BP rows touches.  First the bound of a window of BP rows laid anywhere (at most
// ceil((BP - 1) / hw) + 1 images of a level, every level at once); the walk over the tiles only where that is not enough
inline int stats_tile_keys(const Shape& s, int BP, int enough) {
  int bound = 0;
  for (int i = 0; i < s.nseg; ++i) {
    const int hw = out_pixels(s, i), span = (BP + hw - 2) / hw + 1;
    bound += span < s.batch ? span : s.batch;
  }
  if (bound <= enough) return bound;
  int most = 0;
  for (int m0 = 0; m0 < s.M; m0 += BP) {
    const int m_last = (m0 + BP < s.M ? m0 + BP : s.M) - 1;
    const int n = stats_row_key(s, m_last) - stats_row_key(s, m0) + 1;
    if (n > most) most = n;
  }
  return most;
}
// keys per tile the planned kernel's LDS takes with `groups` groups over N channels
inline int stats_table_max_keys(const FwdPlan& pl, int N, int groups) {
  const int cs = N / groups == 8 ? 3 : 2;
  const long long room = pl.lds_bytes - stats_table_bytes(pl.BP, pl.BC, cs, 0);
  return room <= 0 ? 0 : (int)(room / ((pl.BC >> cs) * 32));
}
// Does the table of every tile of the planned launch fit?  The entry points refuse a launch where it does not (small
// levels at a large batch: a 128 x 128 tile over 1 x 1 levels of 62 or more images).  A fused GroupNorm launch
// (norm_fusable) has whole levels only, 16 pixels or more per key: at most BP / 16 + 1 keys, which fit every kernel.
inline bool stats_table_fits(const Shape& s, const FwdPlan& pl, int groups) {
  if (groups <= 0) return true;
  const int room = stats_table_max_keys(pl, s.N, groups);
  return stats_tile_keys(s, pl.BP, room) <= room;
}

// Would kd6d_conv2d_fwd_norm take the fused path?  `fuse_norm`: option conv.fuse_norm (bit 0 = GroupNorm launches,
// bit 1 = BatchNorm launches).  The plan of the call as kd6d_conv2d_fwd_norm makes it, then the residency rule of
// kd6d_barrier.h.  `out_hw`: pixels of each level's output grid.
inline bool norm_fusable(const Shape& p, const int* out_hw, int dtype, int kind, int groups, int fuse_norm, bool pair_active,
                         const Options& o, int ncu) {
  if ((fuse_norm & (kind == kNormGroup ? 1 : 2)) == 0) return false;
  const int stats_groups = kind == kNormGroup ? groups : 0;
  if (!stats_channels_ok(p.N) || stats_groups < 0 || !stats_groups_ok(p.N, stats_groups)) return false;
  if (kind == kNormGroup && groups <= 0) return false;
  // a level whose statistics need the separate pass: nothing to wait for in-kernel
  for (int s = 0, m = 0; s < p.nseg; m += p.batch * out_hw[s], ++s)
    if (stats_groups > 0 && stats_level_skipped(out_hw[s], m)) return false;
  Flags f;
  f.dtype = dtype; f.has_stats = true; f.stats_groups = stats_groups; f.norm_fused = true; f.pair_active = pair_active;
  const FwdPlan plan = plan_fwd(p, f, o, ncu);
  if (!plan.fused_epilogue || plan.grid_x <= 0) return false;
  const size_t lds = plan.lds_bytes > 0 ? (size_t)plan.lds_bytes : 1;
  const int waves = plan.threads / 64;
  if (kind == kNormBatch) {
    // grid barrier: every workgroup of the launch pinned until the last one has arrived.  Admit only launches that fit
    // in HALF of the device's LDS and wave slots (the other half is what window-barrier launches on other streams and
    // fragmentation may hold), at no more than two workgroups per CU
    if ((size_t)plan.grid_x * lds > (size_t)ncu * kLdsPerCu / 2) return false;
    if (plan.grid_x * waves > ncu * kWaveSlotsPerCu / 2) return false;
    if (plan.grid_x > 2 * ncu) return false;
  } else {
    // window barrier: with workgroup id == tile id a tile waits for the pixel tiles of its own (level, image) keys only
    const int n_ctiles = (p.N + 15) / 16;       // upper bound of the channel tiles
    if (n_ctiles > 16 * kNormMaxCtiles) return false;
  }
  return true;
}

// ---- weight gradient -------------------------------------------------------------------------------------------
// CUs a launch aims to fill: the caller's budget, 0 or more than the device = all of it
inline int clamp_cu_budget(int cu_budget, int ncu) { return (cu_budget == 0 || cu_budget > ncu) ? ncu : cu_budget; }

inline void wgrad_split(WgradPlan& pl, const Shape& p, int tiles, int splits, int steps_total, int BKM) {
  const int steps_per = ceil_div(steps_total, splits);
  pl.m_chunk = steps_per * BKM;
  pl.parts = ceil_div(p.M, pl.m_chunk);
  pl.grid_x = tiles; pl.grid_y = pl.parts;
}

inline bool wgrad_small_listed(int cg, int nb, int ks) {
#define KD6D_CONV_LISTED(a, b, c) if (cg == a && nb == b && ks == c) return true;
  KD6D_CONV_WGRAD_SMALL_TILES(KD6D_CONV_LISTED)
#undef KD6D_CONV_LISTED
  return false;
}

// wide, shallow layers: Cin in {8,16,32}, Cout <= 64, 3x3/s1/p1 or 1x1/s1, one level, >= 2^15 pixels, no bias gradient
inline bool wgrad_small_rule(const Shape& p, const Flags& f, const Options& o, int cu_budget, WgradPlan& pl) {
  const int force = o.wgrad_small;
  if (force == 0 || f.with_bias || p.nseg != 1 || p.stride != 1) return false;
  if (!((p.ks == 3 && p.pad == 1) || (p.ks == 1 && p.pad == 0))) return false;
  if ((p.C != 8 && p.C != 16 && p.C != 32) || p.N > 64 || (p.N & 7)) return false;
  const Level& q = p.seg[0];
  if (q.in_row0 != 0 || q.out_row0 != 0 || q.in_w > 256) return false;
  // measured (tools/bench_conv.py, B = 16): the 1x1 layers gain (64x64 map, 16 -> 8 channels: 16.2 -> 7.5 us); the
  // 3x3 layers do NOT -- a tile is one DMA round trip of ~3 us for ~0.3 us of MFMA work and the persistent grid
  // that keeps the atomic flush small also keeps too few round trips in flight (256x256x8->8: 46 -> 45 us,
  // 128x128x8->16: 26 -> 31, 64x64x8->64: 21 -> 20; more workgroups: slower, the flush serialises).  They stay
  // on the general kernel unless forced; a deeper DMA ring per workgroup is the open improvement.
  if (force < 0 && (p.M < (1 << 15) || p.ks != 1)) return false;
  const int W = q.in_w, H = q.in_h;      // (a "same" stride-1 layer: the output grid is the input grid)
  WgradPlan t;
  t.family = kWgSmall;
  t.NB = (p.N + 15) / 16; t.CG = p.C / 8; t.KS = p.ks;
  if (!wgrad_small_listed(t.CG, t.NB, t.KS)) return false;      // (33 ... 48 result channels: no 3-block variant)
  t.R = 512 / W;                         // ~512 positions per tile (256: 9.5 us on the 16 -> 8 layer, 512: 7.5)
  if (t.R < 1) t.R = 1;
  if (t.R > H) t.R = H;
  wgrad_small_lds(t, W);
  while (t.R > 1 && 2ll * t.buf_bytes > 72 * 1024) { t.R >>= 1; wgrad_small_lds(t, W); }      // two workgroups per CU
  if (2ll * t.buf_bytes > 144 * 1024) return false;
  t.tiles_per_img = ceil_div(H, t.R);
  t.ntiles = p.batch * t.tiles_per_img;
  t.grid_x = 2 * cu_budget;              // persistent: one flush per workgroup
  if (t.grid_x > t.ntiles) t.grid_x = t.ntiles;
  t.parts = t.grid_x;
  pl = t;
  return true;
}

// bf16: the transposing kernel, 128-wide j tiles
inline void wgrad_tr_rule(const Shape& p, int ncu, int cu_budget, WgradPlan& pl) {
  const int BJ = 128, BKM = 64;
  pl.family = kWgTr;
  pl.BJ = BJ;
  if (p.N <= 16) { pl.BN = 16; pl.WN = 1; pl.WJ = 4; }
  else if (p.N <= 32) { pl.BN = 32; pl.WN = 1; pl.WJ = 4; }
  else if (p.N <= 64) { pl.BN = 64; pl.WN = 1; pl.WJ = 4; }
  else { pl.BN = 128; pl.WN = 2; pl.WJ = 2; }
  pl.n_jtiles = ceil_div(p.K, BJ);
  const int tiles = pl.n_jtiles * ceil_div(p.N, pl.BN);
  const int steps_total = ceil_div(p.M, BKM);
  // time ~ (steps/S) * t_step + S * |dW| / (flush rate), t_step ~ 1.6 us measured.  A split's partial image costs a plain
  // store here (~6 TB/s) and a read by kd6d_grad_acc_resolve at the end of the sweep (~4 TB/s): 2.4 TB/s together (the fp32
  // atomic flush of rounds 1-3: 1.3 TB/s)
  //   => S* = sqrt(steps * t_step * rate / |dW|); at most 2 workgroups per CU, because many
  //   workgroups adding into one small dW are contention-bound (measured: 2048 -> 512 = -25 %)
  // a caller that keeps several weight gradients in flight asks each for a fraction of the device: fewer,
  // longer splits -> proportionally fewer atomic tile flushes for the same k-loop work
  const double frac = (double)cu_budget / (double)ncu;
  const double dw_bytes = (double)p.N * (double)p.K * 4.0;
  int splits = (int)(frac * sqrt((double)steps_total * 3.8e6 / dw_bytes) + 0.5);
  if (splits > 512 / tiles) splits = 512 / tiles;
  if (splits > steps_total / 2) splits = steps_total / 2;
  if (splits < 1) splits = 1;
  wgrad_split(pl, p, tiles, splits, steps_total, BKM);
  pl.lds_bytes = wgrad_tr_lds(pl.BN);
}

// The first block of the darknet-tiny students: 3x3/s1/p1, 8 stored source channels, 8 or 16 result channels, one level
// packed from row 0, train-mode BatchNorm + activation + 2x2 max-pool behind it and NO data gradient wanted.  There the
// gradient of the convolution output is read by the weight gradient alone, so one kernel forms it in LDS from the
// convolution output and the pooled gradient and contracts it with the source patch at once (kd6d_bn_pool_bwd_wgrad).
// A tile is R whole image rows (R even: whole pool windows) of at most 512 pixels; workgroup s walks the T consecutive
// tiles s*T ... and stores one partial image, every (channel, tap) block accumulated over 32-pixel steps in pixel order.
// T comes from the pixel split of the transposing kernel (wgrad_tr_rule) this launch stands in for: where that split is
// a whole number of tiles of whole 32-pixel steps (the students' stems: 2048 pixels = 4 tiles of 2 x 256, 512 parts) the
// partial images are the SAME sums in the SAME association as the separate path's, bit for bit; elsewhere another valid
// association of the same products.  cu_budget: clamp_cu_budget().  Option stem.fused = 0 turns the rule off.
inline bool stem_bwd_rule(const Shape& p, const Flags& f, bool need_dx, const Options& o, int ncu, int cu_budget,
                          StemBwdPlan& pl) {
  if (o.stem_fused == 0 || need_dx || f.dtype != kBf16 || f.with_bias || p.nseg != 1) return false;
  if (p.ks != 3 || p.stride != 1 || p.pad != 1 || p.C != 8 || (p.N != 8 && p.N != 16)) return false;
  const Level& q = p.seg[0];
  const int W = q.in_w, H = q.in_h;
  if (q.in_row0 != 0 || q.out_row0 != 0 || W < 2 || H < 2 || (W & 1) || (H & 1) || W > 256) return false;
  StemBwdPlan t;
  t.NOUT = p.N;
  t.R = (512 / W) & ~1;                   // (W <= 256: at least 2)
  if (t.R > H) t.R = H;
  const int Wp = W + 2;
  t.Qpad = (t.R * W + 31) & ~31;          // pixels of a tile, whole 32-pixel steps (the tail: zero gradient rows)
  // patch rows: the furthest tap of the last (tail) pixel + 8 zero rows, whole 1-KB LDS-DMA bursts
  t.prow = (((t.Qpad - 1) / W + 3) * Wp + 3 + 8 + 63) / 64 * 64;
  t.tiles_per_img = ceil_div(H, t.R);
  t.ntiles = p.batch * t.tiles_per_img;
  WgradPlan tr;
  wgrad_tr_rule(p, ncu, cu_budget, tr);
  t.tiles_per_wg = tr.m_chunk / (t.R * W);
  if (t.tiles_per_wg < 1) t.tiles_per_wg = 1;
  t.grid = ceil_div(t.ntiles, t.tiles_per_wg);
  t.parts = t.grid;
  // the two per-channel totals, the gradient tile (2 bytes x NOUT per pixel), the source patch; or the flush's image
  const long long tile = 128 + (long long)t.Qpad * 2 * t.NOUT + (long long)t.prow * 16;
  const long long image = 16ll * 80 * 4;
  t.lds_bytes = tile > image ? tile : image;
  t.slab_floats = (long long)t.parts * p.N * p.K;
  pl = t;
  return true;
}

// fp32 (exact-parity path): the generic kernel
inline void wgrad_generic_rule(const Shape& p, int dtype, WgradPlan& pl) {
  const int BKM = 8 * (dtype == kBf16 ? 8 : 4);
  pl.family = kWgGeneric;
  if (p.N <= 16) { pl.BN = 16; pl.BJ = 128; pl.WN = 1; pl.WJ = 4; }
  else if (p.N <= 32) { pl.BN = 32; pl.BJ = 128; pl.WN = 1; pl.WJ = 4; }
  else if (p.N <= 64 || p.K <= 64) { pl.BN = 64; pl.BJ = 64; pl.WN = 2; pl.WJ = 2; }
  else { pl.BN = 128; pl.BJ = 128; pl.WN = 2; pl.WJ = 2; }
  pl.n_jtiles = ceil_div(p.K, pl.BJ);
  const int tiles = pl.n_jtiles * ceil_div(p.N, pl.BN);
  const int steps_total = ceil_div(p.M, BKM);
  int splits = ceil_div(1024, tiles);               // aim for ~1024 workgroups
  int max_splits = (steps_total + 3) / 4;           // at least 4 k-steps per split
  if (max_splits < 1) max_splits = 1;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  wgrad_split(pl, p, tiles, splits, steps_total, BKM);
  pl.lds_bytes = wgrad_lds(pl.BN, pl.BJ);
}

// the weight gradient; bf16: small -> tr, fp32: generic.  cu_budget: clamp_cu_budget()
inline WgradPlan plan_wgrad(const Shape& p, const Flags& f, const Options& o, int ncu, int cu_budget) {
  WgradPlan pl;
  if (f.dtype != kBf16) wgrad_generic_rule(p, f.dtype, pl);
  else if (!wgrad_small_rule(p, f, o, cu_budget, pl)) wgrad_tr_rule(p, ncu, cu_budget, pl);
  return pl;
}

// ---- list launch of the transposing weight gradient (conv_wgrad_tr_list_kernel) ---------------------------------
// Up to kWgradListMax per-layer weight gradients as ONE launch: entry e keeps the grid plan_wgrad gave its call (same
// cu_budget, same tiles, same pixel splits) and owns the workgroups first_block[e] ... first_block[e + 1] - 1 of the list's
// one-dimensional grid, row-major over its own (grid_x, grid_y).  Listable: what plan_wgrad sends to the transposing
// family (bf16, not the narrow-layer kernel).  kWgradListBytes: sizeof of the kernel's by-value argument (conv_igemm.hip
// asserts it), under the 4-KB kernel-argument limit.
constexpr int kWgradListMax = 4;
constexpr int kWgradListBytes = 1288;
constexpr int kKernargLimit = 4096;
static_assert(kWgradListBytes < kKernargLimit, "the list is passed by value");

struct WgradListPlan {
  int n = 0;                               // entries of this list (0: no listable call in [begin, end))
  int end = 0;                             // the next list starts at this call
  int call[kWgradListMax] = {0, 0, 0, 0};  // which call an entry stands for, in call order
  int variant[kWgradListMax] = {0, 0, 0, 0};       // its tile of KD6D_CONV_WGRAD_TR_TILES, named by BN
  int grid_x[kWgradListMax] = {0, 0, 0, 0}, grid_y[kWgradListMax] = {0, 0, 0, 0};
  int first_block[kWgradListMax + 1] = {0, 0, 0, 0, 0};
  int grid = 0;                            // workgroups of the launch = first_block[n]
  long long lds_bytes = 0;                 // the largest entry's
};

inline bool wgrad_listable(const WgradPlan& pl) {
  if (pl.family != kWgTr) return false;
#define KD6D_CONV_LISTED(bn, wn, wj) if (pl.BN == bn && pl.WN == wn && pl.WJ == wj) return true;
  KD6D_CONV_WGRAD_TR_TILES(KD6D_CONV_LISTED)
#undef KD6D_CONV_LISTED
  return false;
}

// The list that starts at call `begin` of plans[0 .. n_calls): the next (at most kWgradListMax) listable calls in call
// order.  Calls of [begin, end) that are not listable get no slot: the caller launches each on its own behind the list.
inline WgradListPlan plan_wgrad_list(const WgradPlan* plans, int n_calls, int begin) {
  WgradListPlan L;
  int i = begin;
  for (; i < n_calls && L.n < kWgradListMax; ++i) {
    const WgradPlan& pl = plans[i];
    if (!wgrad_listable(pl)) continue;
    const int e = L.n++;
    L.call[e] = i; L.variant[e] = pl.BN;
    L.grid_x[e] = pl.grid_x; L.grid_y[e] = pl.grid_y;
    L.first_block[e + 1] = L.first_block[e] + pl.grid_x * pl.grid_y;
    if (pl.lds_bytes > L.lds_bytes) L.lds_bytes = pl.lds_bytes;
  }
  // (a list that filled up ends right behind its last entry: what follows belongs to the next list)
  L.end = i;
  L.grid = L.first_block[L.n];
  return L;
}

// which (entry, block_x, block_y) workgroup `block` of the list's grid is: the kernel's own decode
inline void wgrad_list_decode(const WgradListPlan& L, int block, int& entry, int& block_x, int& block_y) {
  entry = 0;
  for (int i = 1; i < L.n; ++i)
    if (block >= L.first_block[i]) entry = i;
  const int local = block - L.first_block[entry];
  block_y = local / L.grid_x[entry];
  block_x = local - block_y * L.grid_x[entry];
}

}  // namespace kd6d_conv
#endif  // KD6D_CONV_PLAN_H_
