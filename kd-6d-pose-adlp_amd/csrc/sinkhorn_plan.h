// The host decisions of the dense Sinkhorn launcher (sinkhorn_dense.hip), each stated once: the epsilon schedule, the
// workspace layout, which softmin kernel a pass takes, rows per workgroup and the grid of every softmin launch.  No HIP
// include: sinkhorn_dense.hip fills its launches from these and tests/sinkhorn_plan_host.cpp builds the header with g++,
// so every rule below is checked without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

namespace kd6d_sinkhorn {

// ---- constants the rules share with the kernels ----------------------------------------------------------------
constexpr int kThreadsD = 512;     // difference form: 2 waves per SIMD (a lone wave issues one VALU op per 4+ clk)
constexpr int kRows = 256;         // its rows per workgroup: 2 threads per row, each takes its share of every column tile
constexpr int kGradRows = 128;     // ... of its gradient form (SPLIT = 4): runs on two of the four softmins only and still
                                   // yields one workgroup per CU at N = 16384
constexpr int kMRows = 64;         // matrix pipe: 2 row groups of 32; the other two waves take the other column half
constexpr int kMRowsWide = 128;    // ... with 8 waves (sinkhorn.dense_rows)
constexpr int kWideFromRows = 8192;     // sinkhorn.dense_rows = -1: kMRowsWide from this many rows up
constexpr int kSplitBytes = 96;    // prepared point: 3 pieces x 2 k-halves x 8 bf16
constexpr int kYtBytes = 64;       // A operand of the gradient's second product, per point: 16 dimensions x (hi, lo) fp16
constexpr int kYtPadPoints = 128;  // ... sets padded to a multiple of this many points (zeros)
constexpr int kCenterWgs = 64;     // partial sums per set of dense_center_kernel, 16 floats each
constexpr double kMfmaEpsRel = 1.5e-4;  // eps / diameter^2 from which the matrix-pipe softmin is taken (measured: tests)
constexpr int kMaxScaledSteps = 4096;   // cap of the schedule's geometric part

// ---- epsilon schedule (geomloss epsilon_schedule, p = 2) -------------------------------------------------------
// [d^2] + exp(arange(2 ln d, 2 ln blur, 2 ln scaling)) + [blur^2], in double like the reference's python floats.
// blur, scaling and reach are the callers' fp32 arguments, widened.  (The small-set kernel of sinkhorn.hip evaluates the
// same expressions on the device, per workgroup, from the diameter it measures.)
struct EpsSchedule {
  double diameter, blur, e_start, e_step;
  double rho;                      // reach^2; -1 when balanced (reach <= 0)
  int n_ar;                        // steps of the geometric part
  EpsSchedule(double diameter_, double blur_, double scaling, double reach)
      : diameter(diameter_ < 1e-12 ? 1e-12 : diameter_), blur(blur_), rho(reach > 0.0 ? reach * reach : -1.0), n_ar(0) {
    e_start = 2.0 * log(diameter);
    e_step = 2.0 * log(scaling);
    const double e_stop = 2.0 * log(blur);
    if (e_step < 0.0 && e_start > e_stop) n_ar = (int)ceil((e_stop - e_start) / e_step);
    if (n_ar < 0) n_ar = 0;
    if (n_ar > kMaxScaledSteps) n_ar = kMaxScaledSteps;
  }
  int n_eps() const { return n_ar + 2; }
  double at(int i) const {
    if (i == 0) return diameter * diameter;
    if (i <= n_ar) return exp(e_start + (double)(i - 1) * e_step);
    return blur * blur;
  }
  // damping of the unbalanced updates, 1 / (1 + eps / rho)
  float lam(double eps) const { return rho > 0.0 ? (float)(1.0 / (1.0 + eps / rho)) : 1.f; }
};

// ---- workspace of kd6d_sinkhorn_dense_fwd_bwd ------------------------------------------------------------------
// Regions in bytes from the workspace pointer.  For D = 16 the matrix-pipe softmin's prepared points follow the
// centre: |p - centre|^2, kSplitBytes of bf16 pieces per point (16-byte aligned, hence `misalign`: the workspace
// pointer's address modulo 16 -- 0, 4, 8 or 12) and kYtBytes of fp16 pieces per point of the padded sets.
struct Region { int64_t off, bytes; };
constexpr int kCenterFloats = 64;       // 16 sums and padding
constexpr int kAlignSlackFloats = 16;   // counted in total_floats for the alignment of `xs`
struct DenseWorkspace {
  Region la, lb;                   // log weights (N), (M)
  Region pot[2];                   // the two potential sets, [a_x (N) | b_x (N) | b_y (M) | a_y (M)] each
  Region grad_xx, grad_xy;         // (N, D) each
  Region center;
  Region n2;                       // (N + M)
  Region xs, ys;                   // "splits"
  Region xt, yt;
  Region partials;                 // dense_center_kernel's partial sums borrow the head of xt: dense_split_kernel fills it afterwards
  int64_t total_floats;
};
constexpr int64_t kPartialsBytes = 2 * kCenterWgs * 16 * (int64_t)sizeof(float);
static_assert(kPartialsBytes <= (int64_t)kYtPadPoints * kYtBytes, "the centre's partial sums must fit xt of a one-point set");

inline DenseWorkspace dense_workspace(int N, int M, int D, int misalign) {
  DenseWorkspace w;
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const Region r = {at, bytes}; at += bytes; return r; };
  const int64_t f = sizeof(float), n = N, m = M, mfma = D == 16;
  const int64_t pad = kYtPadPoints - 1;
  w.la = take(n * f);
  w.lb = take(m * f);
  w.pot[0] = take(2 * (n + m) * f);
  w.pot[1] = take(2 * (n + m) * f);
  w.grad_xx = take(n * D * f);
  w.grad_xy = take(n * D * f);
  w.center = take(kCenterFloats * f);
  w.n2 = take(mfma * (n + m) * f);
  if (mfma) at = ((at + misalign + 15) & ~(int64_t)15) - misalign;
  w.xs = take(mfma * n * kSplitBytes);           // kSplitBytes and kYtBytes are multiples of 16: all four stay aligned
  w.ys = take(mfma * m * kSplitBytes);
  w.xt = take(mfma * ((n + pad) & ~pad) * kYtBytes);
  w.yt = take(mfma * ((m + pad) & ~pad) * kYtBytes);
  w.partials = Region{w.xt.off, mfma * kPartialsBytes};
  // the sum of the regions (what the Python callers allocate), not the end of yt: independent of the pointer
  w.total_floats = (w.center.off + w.center.bytes) / f +
                   mfma * ((w.n2.bytes + w.xs.bytes + w.ys.bytes + w.xt.bytes + w.yt.bytes) / f + kAlignSlackFloats);
  return w;
}

// ---- which softmin kernel a pass takes -------------------------------------------------------------------------
enum class Path { Difference, MatrixPipe, Screened };
// options sinkhorn.dense_mfma (0 = never the matrix pipe | 1 = while eps >= kMfmaEpsRel * diameter^2 | 2 = always
// (tests: how wrong it gets) | 3 = as 1, the gradient-carrying launch in the difference form), sinkhorn.dense_screen
// and sinkhorn.dense_rows
struct DenseOptions { long long mfma, screen, rows; };
// The matrix-pipe kernel while the cancellation of its |r|^2 + |c|^2 - 2 r.c form stays below ~1e-4 in the exponent
// (header of dense_softmin_mfma_kernel); below that rule the matrix pipe screens and the difference form evaluates
// what passes (dense_softmin_screen_kernel).  `grad`: the launch of the last extrapolation that carries the gradient
// (its companion, the other two softmins, is a gradient-free launch).  Under mode 3 that launch takes the difference
// form where the rule holds -- also with dense_screen set, which only acts below the rule.
inline Path softmin_path(int D, double eps, double diameter, const DenseOptions& o, bool grad) {
  if (D != 16 || o.mfma == 0) return Path::Difference;
  const bool mfma_ok = o.mfma == 2 || eps >= kMfmaEpsRel * diameter * diameter;
  if (mfma_ok) return grad && o.mfma == 3 ? Path::Difference : Path::MatrixPipe;
  return o.screen != 0 ? Path::Screened : Path::Difference;
}
// Exponent distance from the running maximum beyond which the screened form drops a pair: 40 + twice the bound of the
// approximate exponent's error, k2 2^-21 S with S <= diameter^2 (centred points)
inline float screen_threshold(double eps, double diameter) {
  return (float)(40.0 + (0.5 / eps) * 1.4426950408889634 * diameter * diameter * (1.0 / 1048576.0));
}

// ---- rows per workgroup and grids ------------------------------------------------------------------------------
// Matrix-pipe and screened softmins: every workgroup streams ALL columns (108-172 bytes each) through LDS, so the
// launch moves (rows / rows-per-workgroup) x columns x bytes from L2 -- 1.8-2.9 GB at N = M = 16384 with 64 rows, which
// is what bounds it (6-9 TB/s); 128 rows (8 waves) halve that.  rows_opt (sinkhorn.dense_rows): 64 | 128 | anything
// else = 128 from kWideFromRows rows up
inline int matrix_rows(int nmax, long long rows_opt) {
  return rows_opt == kMRowsWide || (rows_opt != kMRows && nmax >= kWideFromRows) ? kMRowsWide : kMRows;
}
struct SoftminLaunch { int rows; unsigned grid_x, grid_y, block; };
// One launch of `softmins` (4, or 2 in the last extrapolation) softmins, one per blockIdx.y.  grad: the two softmins over
// the rows of x with their gradient sums; the matrix-pipe and screened forms of it cover the N rows of x only, every
// other launch max(N, M) rows.  mrows = matrix_rows().
inline SoftminLaunch softmin_launch(Path path, bool grad, int softmins, int N, int M, int mrows) {
  int rows = grad ? kGradRows : kRows, extent = N > M ? N : M, block = kThreadsD;
  if (path != Path::Difference) {
    rows = path == Path::MatrixPipe && grad ? kMRows : mrows;      // dense_softmin_mfma_grad_kernel has the one form
    block = 4 * rows;                                              // a wave per 32 rows, times two column halves
    if (grad) extent = N;
  }
  return SoftminLaunch{rows, (unsigned)((extent + rows - 1) / rows), (unsigned)(grad ? 2 : softmins), (unsigned)block};
}

}  // namespace kd6d_sinkhorn
