// Host build of csrc/sinkhorn_plan.h for tests/test_sinkhorn_plan_host.py (g++, no GPU): the SAME header
// sinkhorn_dense.hip takes its schedule, workspace layout, kernel choice and grids from.
#include "../kd-6d-pose-adlp_amd/csrc/sinkhorn_plan.h"

using namespace kd6d_sinkhorn;

extern "C" {
// kThreadsD, kRows, kGradRows, kMRows, kMRowsWide, kWideFromRows, kSplitBytes, kYtBytes, kYtPadPoints, kCenterWgs,
// kMaxScaledSteps, kCenterFloats, kAlignSlackFloats
void sp_constants(int* out) {
  const int v[13] = {kThreadsD, kRows, kGradRows, kMRows, kMRowsWide, kWideFromRows, kSplitBytes, kYtBytes, kYtPadPoints,
                     kCenterWgs, kMaxScaledSteps, kCenterFloats, kAlignSlackFloats};
  for (int i = 0; i < 13; ++i) out[i] = v[i];
}
double sp_mfma_eps_rel() { return kMfmaEpsRel; }
// values[0 .. min(n_eps, cap)) = at(i); facts = {diameter, rho}; returns n_eps
int sp_schedule(double diameter, double blur, double scaling, double reach, double* values, int cap, double* facts) {
  const EpsSchedule s(diameter, blur, scaling, reach);
  for (int i = 0; i < s.n_eps() && i < cap; ++i) values[i] = s.at(i);
  facts[0] = s.diameter; facts[1] = s.rho;
  return s.n_eps();
}
float sp_lam(double diameter, double blur, double scaling, double reach, double eps) {
  return EpsSchedule(diameter, blur, scaling, reach).lam(eps);
}
// out = (off, bytes) of la, lb, pot[0], pot[1], grad_xx, grad_xy, center, n2, xs, ys, xt, yt, partials; returns total_floats
long long sp_workspace(int N, int M, int D, int misalign, long long* out) {
  const DenseWorkspace w = dense_workspace(N, M, D, misalign);
  const Region r[13] = {w.la, w.lb, w.pot[0], w.pot[1], w.grad_xx, w.grad_xy, w.center, w.n2, w.xs, w.ys, w.xt, w.yt,
                        w.partials};
  for (int i = 0; i < 13; ++i) { out[2 * i] = r[i].off; out[2 * i + 1] = r[i].bytes; }
  return w.total_floats;
}
// 0 Difference, 1 MatrixPipe, 2 Screened
int sp_path(int D, double eps, double diameter, long long mfma, long long screen, int grad) {
  return (int)softmin_path(D, eps, diameter, DenseOptions{mfma, screen, -1}, grad != 0);
}
float sp_screen_threshold(double eps, double diameter) { return screen_threshold(eps, diameter); }
int sp_matrix_rows(int nmax, long long rows_opt) { return matrix_rows(nmax, rows_opt); }
// out = {rows, grid_x, grid_y, block}
void sp_softmin_launch(int path, int grad, int softmins, int N, int M, int mrows, int* out) {
  const SoftminLaunch l = softmin_launch((Path)path, grad != 0, softmins, N, M, mrows);
  out[0] = l.rows; out[1] = (int)l.grid_x; out[2] = (int)l.grid_y; out[3] = (int)l.block;
}
}
