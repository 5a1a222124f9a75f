// Batched PnP-RANSAC on the GPU: the solver of kd6d/libs/pnp.py (solve_pnp_ransac) restated for a whole batch of
// problems, and the teacher PnP gate of postprocess_kd.py:187-202 fused behind kd6d_teacher_select.
//
// Problem p: cnt[p] <= cap cells of 8 keypoints (full-frame px, (P*cap, 8, 2) like t_kp), a box of 8 object-space
// corners and an intrinsic K.  Correspondence (cell i, keypoint k) belongs to corner k.
//
//   pnp_hyp_kernel   ONE LANE PER HYPOTHESIS: grid (ceil(iters / 64), P), 64 threads.  Hypothesis h takes one cell
//                    per corner (counter-based hash of (seed, h, k)), fits a DLT on normalised image coordinates
//                    (3D points centred and scaled to unit RMS; 12x12 smallest eigenvector by shifted inverse
//                    iteration in fp64), counts the loose consensus (3 x reproj_err, z > 0), re-fits the DLT on it
//                    (>= 6 corners), runs 4 Gauss-Newton steps on (rotation vector, t), counts the tight consensus
//                    and, with >= 6 points on >= 6 corners, runs 6 more steps and counts again.  It writes
//                    {count, R, T} to its own workspace slot.
//   pnp_pick_kernel  one wave per problem: the winner is (count desc, h asc); ok = count >= 6 and R, T finite.
//   pose_remap_kernel (kd6d_pose_remap, further down): ONE LANE PER INSTANCE, the same DLT and Gauss-Newton on one clean
//                    observation per corner -- the two pose remaps of the augmentation chain, kd6d/libs/pnp.py's remap_pose.
//
// Every correspondence of corner k is scored against the same projected corner, so a consensus set reduces to eight
// per-corner sums (count, sum of residuals, their second moments): the Gauss-Newton normal equations and the DLT's
// normal matrix are built from those, lane-locally, without cross-lane arithmetic.  The cells are read at
// wave-uniform addresses.  Each lane's result is a pure function of (problem, seed, h) and the pick is a fixed-order
// comparison: bitwise reproducible, independent of the problem's position and of the batch size.  No atomics.
#include <math.h>

#include "kd6d_common.h"

namespace {

constexpr int kSlot = 16;          // workspace floats per hypothesis: count (int bits), R (9), T (3), 3 unused
constexpr int kMaxIters = 1 << 20;
constexpr int kInvIters = 12;      // inverse-iteration steps of the DLT's smallest eigenvector

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// the cell through which hypothesis h observes corner k: counter-based, no hypothesis depends on another
__device__ __forceinline__ int sample_cell(unsigned long long seed, int h, int k, int n) {
  const unsigned long long z = splitmix64(seed ^ splitmix64(((unsigned long long)(unsigned)h << 3) | (unsigned)k));
  return (int)((z >> 32) % (unsigned long long)n);
}

struct Problem {
  const float* kp;       // (n, 8, 2) pixels of this problem's cells
  int n;
  float X[8][3];         // corners as given
  double c[3], inv_s;    // normalisation of the DLT: (X - c) * inv_s has unit RMS
  float K[9];
  double a[3], b[3];     // the first two rows of K^-1 (normalised image coordinates, as the host's `uv1 @ Kinv.T`)
};

struct Pose {
  double R[9], t[3];
};

// one consensus pass: per-corner sums of the inliers' residuals e = u - pu_k, f = v - pv_k
struct Pass {
  int count;
  unsigned cmask;        // corners with at least one inlier
  float nk[8], se[8], sf[8], see[8], sef[8], sff[8];
  float pu[8], pv[8];    // the projected corners
};

// ---- problem set-up (wave-uniform); false: the problem is degenerate or holds a non-finite value ---------------------
__device__ bool load_problem(Problem& P, const float* kp, int n, const float* box, const float* K) {
  P.kp = kp;
  P.n = n;
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      P.X[k][d] = box[k * 3 + d];
      fin = fin && isfinite(P.X[k][d]);
    }
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    P.K[i] = K[i];
    fin = fin && isfinite(P.K[i]);
  }
  for (int j = 0; j < n * 16; ++j) fin = fin && isfinite(kp[j]);
  if (!fin) return false;
  // distinct corners, compared exactly
  int distinct = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    bool first = true;
#pragma unroll
    for (int q = 0; q < k; ++q)
      first = first && !(P.X[q][0] == P.X[k][0] && P.X[q][1] == P.X[k][1] && P.X[q][2] == P.X[k][2]);
    distinct += first ? 1 : 0;
  }
  if (distinct < 6) return false;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) m += (double)P.X[k][d];
    P.c[d] = m * 0.125;
  }
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double v = (double)P.X[k][d] - P.c[d];
      ss += v * v;
    }
  const double rms = sqrt(ss * 0.125);
  if (!(rms > 0.0)) return false;
  P.inv_s = 1.0 / rms;
  // K^-1 by cofactors (fp64)
  const double k0 = P.K[0], k1 = P.K[1], k2 = P.K[2], k3 = P.K[3], k4 = P.K[4], k5 = P.K[5], k6 = P.K[6],
               k7 = P.K[7], k8 = P.K[8];
  const double c00 = k4 * k8 - k5 * k7, c01 = k5 * k6 - k3 * k8, c02 = k3 * k7 - k4 * k6;
  const double det = k0 * c00 + k1 * c01 + k2 * c02;
  if (!(fabs(det) > 0.0) || !isfinite(det)) return false;
  const double id = 1.0 / det;
  P.a[0] = c00 * id; P.a[1] = (k2 * k7 - k1 * k8) * id; P.a[2] = (k1 * k5 - k2 * k4) * id;
  P.b[0] = c01 * id; P.b[1] = (k0 * k8 - k2 * k6) * id; P.b[2] = (k2 * k3 - k0 * k5) * id;
  return true;
}

// ---- consensus (fp32) -----------------------------------------------------------------------------------------------
template <bool kMoments>
__device__ __forceinline__ void score(const Problem& P, const Pose& ps, float thr2, Pass& o) {
  float R[9], T[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (float)ps.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) T[i] = (float)ps.t[i];
  bool zpos[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float cx = R[0] * P.X[k][0] + R[1] * P.X[k][1] + R[2] * P.X[k][2] + T[0];
    const float cy = R[3] * P.X[k][0] + R[4] * P.X[k][1] + R[5] * P.X[k][2] + T[1];
    const float cz = R[6] * P.X[k][0] + R[7] * P.X[k][1] + R[8] * P.X[k][2] + T[2];
    const float w = P.K[6] * cx + P.K[7] * cy + P.K[8] * cz + 1e-12f;
    o.pu[k] = (P.K[0] * cx + P.K[1] * cy + P.K[2] * cz) / w;
    o.pv[k] = (P.K[3] * cx + P.K[4] * cy + P.K[5] * cz) / w;
    zpos[k] = cz > 0.f;
    o.nk[k] = o.se[k] = o.sf[k] = o.see[k] = o.sef[k] = o.sff[k] = 0.f;
  }
  for (int i = 0; i < P.n; ++i) {
    const float* q = P.kp + i * 16;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float e = q[2 * k] - o.pu[k], f = q[2 * k + 1] - o.pv[k];
      const float m = (zpos[k] && e * e + f * f < thr2) ? 1.f : 0.f;
      o.nk[k] += m;
      o.se[k] += m * e;
      o.sf[k] += m * f;
      if (kMoments) {
        o.see[k] += m * e * e;
        o.sef[k] += m * e * f;
        o.sff[k] += m * f * f;
      }
    }
  }
  int cnt = 0;
  unsigned cm = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    cnt += (int)o.nk[k];
    cm |= o.nk[k] > 0.f ? (1u << k) : 0u;
  }
  o.count = cnt;
  o.cmask = cm;
}

// ---- DLT ------------------------------------------------------------------------------------------------------------
// Normal matrix of the DLT rows [Xh, 0, -x Xh], [0, Xh, -y Xh] (Xh = (normalised corner, 1)) from the per-corner sums
// n_k, sum x, sum y, sum x^2 + y^2; its smallest eigenvector by inverse iteration on N + mu I (Cholesky, fp64).
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }

__device__ bool dlt(const Problem& P, const double n[8], const double sx[8], const double sy[8], const double sr[8],
                    Pose& out) {
  double Q0[10], Qx[10], Qy[10], Qr[10];      // packed lower 4x4 of sum_k w_k Xh_k Xh_k^T
#pragma unroll
  for (int e = 0; e < 10; ++e) Q0[e] = Qx[e] = Qy[e] = Qr[e] = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double xh[4];
#pragma unroll
    for (int d = 0; d < 3; ++d) xh[d] = ((double)P.X[k][d] - P.c[d]) * P.inv_s;
    xh[3] = 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const double q = xh[i] * xh[j];
        Q0[tri(i, j)] += n[k] * q;
        Qx[tri(i, j)] += sx[k] * q;
        Qy[tri(i, j)] += sy[k] * q;
        Qr[tri(i, j)] += sr[k] * q;
      }
  }
  double L[78];
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 12; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const int bi = i >> 2, bj = j >> 2, ii = i & 3, jj = j & 3;
      const int e = ii >= jj ? tri(ii, jj) : tri(jj, ii);
      double v = 0.0;
      if (bi == bj) v = bi == 2 ? Qr[e] : Q0[e];
      else if (bi == 2) v = bj == 0 ? -Qx[e] : -Qy[e];
      L[tri(i, j)] = v;
      if (i == j) tr += v;
    }
  if (!(tr > 0.0) || !isfinite(tr)) return false;
  const double mu = 1e-10 * tr;
  // Cholesky of N + mu I, in place
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    double d = L[tri(j, j)] + mu;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[tri(j, k)] * L[tri(j, k)];
    if (!(d > 0.0)) return false;
    const double r = sqrt(d);
    L[tri(j, j)] = r;
    const double ir = 1.0 / r;
#pragma unroll
    for (int i = j + 1; i < 12; ++i) {
      double s = L[tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[tri(i, k)] * L[tri(j, k)];
      L[tri(i, j)] = s * ir;
    }
  }
  double v[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) v[i] = i == 11 ? 1.0 : 0.1;     // the depth column carries most of the null vector
  for (int it = 0; it < kInvIters; ++it) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      double s = v[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[tri(i, k)] * v[k];
      v[i] = s / L[tri(i, i)];
    }
#pragma unroll
    for (int i = 11; i >= 0; --i) {
      double s = v[i];
#pragma unroll
      for (int k = i + 1; k < 12; ++k) s -= L[tri(k, i)] * v[k];
      v[i] = s / L[tri(i, i)];
    }
    double nn = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) nn += v[i] * v[i];
    const double inv = 1.0 / sqrt(nn);
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] *= inv;
  }
  // undo the normalisation: x ~ M' (X - c) / s + p4'  ->  M = M' / s, p4 = p4' - M c
  double M[9], p4[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int d = 0; d < 3; ++d) M[r * 3 + d] = v[r * 4 + d];
    p4[r] = v[r * 4 + 3];
  }
  const double detp = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) +
                      M[2] * (M[3] * M[7] - M[4] * M[6]);
  if (!isfinite(detp) || fabs(detp) < 1e-18) return false;
  const double sg = detp < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i] *= sg * P.inv_s;
#pragma unroll
  for (int r = 0; r < 3; ++r) p4[r] = sg * p4[r] - (M[r * 3] * P.c[0] + M[r * 3 + 1] * P.c[1] + M[r * 3 + 2] * P.c[2]);
  // rotation = orthogonal polar factor of M (scaled Newton iteration), scale = mean singular value = tr(R^T M) / 3
  double X[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) X[i] = M[i];
  for (int it = 0; it < 10; ++it) {
    const double c0 = X[4] * X[8] - X[5] * X[7], c1 = X[5] * X[6] - X[3] * X[8], c2 = X[3] * X[7] - X[4] * X[6];
    const double c3 = X[2] * X[7] - X[1] * X[8], c4 = X[0] * X[8] - X[2] * X[6], c5 = X[1] * X[6] - X[0] * X[7];
    const double c6 = X[1] * X[5] - X[2] * X[4], c7 = X[2] * X[3] - X[0] * X[5], c8 = X[0] * X[4] - X[1] * X[3];
    const double det = X[0] * c0 + X[1] * c1 + X[2] * c2;
    if (!(det > 0.0) || !isfinite(det)) return false;
    const double g = cbrt(1.0 / det);            // det(g X) = 1
    const double h = 0.5 * g, hi = 0.5 / (g * det);
    // X <- (g X + X^-T / g) / 2, X^-T = cofactors / det
    X[0] = h * X[0] + hi * c0; X[1] = h * X[1] + hi * c1; X[2] = h * X[2] + hi * c2;
    X[3] = h * X[3] + hi * c3; X[4] = h * X[4] + hi * c4; X[5] = h * X[5] + hi * c5;
    X[6] = h * X[6] + hi * c6; X[7] = h * X[7] + hi * c7; X[8] = h * X[8] + hi * c8;
  }
  double scale = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) scale += X[i] * M[i];
  scale *= (1.0 / 3.0);
  if (!(scale > 0.0) || !isfinite(scale)) return false;
#pragma unroll
  for (int i = 0; i < 9; ++i) out.R[i] = X[i];
#pragma unroll
  for (int r = 0; r < 3; ++r) out.t[r] = p4[r] / scale;
  return true;
}

// ---- Gauss-Newton on (rotation vector, t) (fp64) ---------------------------------------------------------------------
// Every point of corner k has corner k's Jacobian, so J^T J = sum_k n_k J_k^T J_k and J^T r = sum_k J_k^T (n_k pred_k -
// sum of the observed pixels): the per-corner counts and coordinate sums of the set are all it needs.
// d(cam)/d(r) = -[R X]_x (left perturbation), d(cam)/d(t) = I; R <- Rodrigues(step) R.
__device__ void gauss_newton(const Problem& P, const double n[8], const double su[8], const double sv[8], Pose& ps,
                             int iters) {
  const double fx = P.K[0], fy = P.K[4], ccx = P.K[2], ccy = P.K[5];
  for (int it = 0; it < iters; ++it) {
    double A[21], g[6];
#pragma unroll
    for (int i = 0; i < 21; ++i) A[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    bool flat = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double X0 = P.X[k][0], X1 = P.X[k][1], X2 = P.X[k][2];
      const double r0 = ps.R[0] * X0 + ps.R[1] * X1 + ps.R[2] * X2;
      const double r1 = ps.R[3] * X0 + ps.R[4] * X1 + ps.R[5] * X2;
      const double r2 = ps.R[6] * X0 + ps.R[7] * X1 + ps.R[8] * X2;
      const double c0 = r0 + ps.t[0], c1 = r1 + ps.t[1], z = r2 + ps.t[2];
      const bool used = n[k] > 0.0;
      flat = flat || (used && fabs(z) < 1e-9);
      const double iz = used && fabs(z) >= 1e-9 ? 1.0 / z : 0.0;
      const double du0 = fx * iz, du2 = -fx * c0 * iz * iz;
      const double dv1 = fy * iz, dv2 = -fy * c1 * iz * iz;
      // rotation columns: (R X) x d
      double ju[6], jv[6];
      ju[0] = r1 * du2;             ju[1] = r2 * du0 - r0 * du2;  ju[2] = -r1 * du0;
      jv[0] = r1 * dv2 - r2 * dv1;  jv[1] = -r0 * dv2;            jv[2] = r0 * dv1;
      ju[3] = du0; ju[4] = 0.0; ju[5] = du2;
      jv[3] = 0.0; jv[4] = dv1; jv[5] = dv2;
      const double ru = iz != 0.0 ? n[k] * (fx * c0 * iz + ccx) - su[k] : 0.0;
      const double rv = iz != 0.0 ? n[k] * (fy * c1 * iz + ccy) - sv[k] : 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) A[tri(i, j)] += n[k] * (ju[i] * ju[j] + jv[i] * jv[j]);
        g[i] += ju[i] * ru + jv[i] * rv;
      }
    }
    if (flat) break;
    // A step = -g by Cholesky
    bool okc = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double d = A[tri(j, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) d -= A[tri(j, k)] * A[tri(j, k)];
      okc = okc && d > 0.0;
      const double r = sqrt(d > 0.0 ? d : 1.0);
      A[tri(j, j)] = r;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double s = A[tri(i, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= A[tri(i, k)] * A[tri(j, k)];
        A[tri(i, j)] = s / r;
      }
    }
    if (!okc) break;
    double s[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double a = -g[i];
#pragma unroll
      for (int k = 0; k < i; ++k) a -= A[tri(i, k)] * s[k];
      s[i] = a / A[tri(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double a = s[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) a -= A[tri(k, i)] * s[k];
      s[i] = a / A[tri(i, i)];
    }
    // R <- Rodrigues(s[0:3]) R, t += s[3:6]
    const double th = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    if (th >= 1e-12) {
      const double kx = s[0] / th, ky = s[1] / th, kz = s[2] / th;
      const double sn = sin(th), cs1 = 1.0 - cos(th);
      // E = I + sin(th) [k]_x + (1 - cos(th)) [k]_x^2
      const double E[9] = {1.0 - cs1 * (ky * ky + kz * kz), -sn * kz + cs1 * kx * ky, sn * ky + cs1 * kx * kz,
                           sn * kz + cs1 * kx * ky, 1.0 - cs1 * (kx * kx + kz * kz), -sn * kx + cs1 * ky * kz,
                           -sn * ky + cs1 * kx * kz, sn * kx + cs1 * ky * kz, 1.0 - cs1 * (kx * kx + ky * ky)};
      double Rn[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          Rn[r * 3 + c] = E[r * 3] * ps.R[c] + E[r * 3 + 1] * ps.R[3 + c] + E[r * 3 + 2] * ps.R[6 + c];
#pragma unroll
      for (int i = 0; i < 9; ++i) ps.R[i] = Rn[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) ps.t[i] += s[3 + i];
  }
}

// absolute per-corner sums of a pass (fp64): n_k, sum u, sum v
__device__ __forceinline__ void gn_sums(const Pass& o, double n[8], double su[8], double sv[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    n[k] = o.nk[k];
    su[k] = n[k] * (double)o.pu[k] + (double)o.se[k];
    sv[k] = n[k] * (double)o.pv[k] + (double)o.sf[k];
  }
}

struct HypArgs {
  int cap, iters;
  const int32_t* cnt;
  const float* kp;
  const float* box;          // general: (P, 8, 3); gate: kp3d (P, n_class_rows, 8, 3)
  const float* K;            // (P, 3, 3)
  float reproj_err;
  unsigned long long seed;
  // gate only (cls != nullptr): the class of image p is read from its first teacher cell
  const float* cls;
  const int32_t* t_row;
  int n_cls, n_class_rows;
  float threshold;
  float* ws;                 // (P, iters, kSlot)
};

__global__ __launch_bounds__(64) void pnp_hyp_kernel(HypArgs a) {
  const int p = blockIdx.y;
  const int h = blockIdx.x * 64 + threadIdx.x;
  int n = a.cnt[p];
  if (n <= 0 || h >= a.iters) return;                   // cnt 0: the pick writes "no pose" without reading a slot
  n = n < a.cap ? n : a.cap;
  const float* box = a.box + (size_t)p * 24;
  if (a.cls) {
    // _apply_pnp_gate: sigmoid of the first cell's logits, the first class above the threshold, else the argmax
    const float* lg = a.cls + (size_t)a.t_row[(size_t)p * a.cap] * 16;
    int c = -1, am = 0;
    float best = -1.f;
    for (int j = 0; j < a.n_cls; ++j) {
      const float pr = 1.f / (1.f + expf(-lg[j]));
      if (c < 0 && pr > a.threshold) c = j;
      if (pr > best) { best = pr; am = j; }
    }
    c = c < 0 ? am : c;
    box = a.box + ((size_t)p * a.n_class_rows + c) * 24;
  }
  Problem P;
  const bool valid = load_problem(P, a.kp + (size_t)p * a.cap * 16, n, box, a.K + (size_t)p * 9);
  int count = -1;
  Pose ps;
#pragma unroll
  for (int i = 0; i < 9; ++i) ps.R[i] = 0.0;
  ps.t[0] = ps.t[1] = ps.t[2] = 0.0;
  if (valid) {
    const float thr2 = a.reproj_err * a.reproj_err;
    double n8[8], sx[8], sy[8], sr[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cell = sample_cell(a.seed, h, k, n);
      const double u = P.kp[cell * 16 + 2 * k], v = P.kp[cell * 16 + 2 * k + 1];
      const double x = P.a[0] * u + P.a[1] * v + P.a[2], y = P.b[0] * u + P.b[1] * v + P.b[2];
      n8[k] = 1.0; sx[k] = x; sy[k] = y; sr[k] = x * x + y * y;
    }
    Pose fit;
    if (dlt(P, n8, sx, sy, sr, fit)) {
      Pass o;
      score<true>(P, fit, 9.f * thr2, o);
      if (o.count >= 6 && __builtin_popcount(o.cmask) >= 6) {
        // loose set -> DLT sums around the projected corners: x = xp_k + (a0 e + a1 f), y likewise
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const double pu = o.pu[k], pv = o.pv[k], nk = o.nk[k];
          const double xp = P.a[0] * pu + P.a[1] * pv + P.a[2], yp = P.b[0] * pu + P.b[1] * pv + P.b[2];
          const double ex = P.a[0] * o.se[k] + P.a[1] * o.sf[k], ey = P.b[0] * o.se[k] + P.b[1] * o.sf[k];
          const double exx = P.a[0] * P.a[0] * o.see[k] + 2.0 * P.a[0] * P.a[1] * o.sef[k] + P.a[1] * P.a[1] * o.sff[k];
          const double eyy = P.b[0] * P.b[0] * o.see[k] + 2.0 * P.b[0] * P.b[1] * o.sef[k] + P.b[1] * P.b[1] * o.sff[k];
          n8[k] = nk;
          sx[k] = nk * xp + ex;
          sy[k] = nk * yp + ey;
          sr[k] = nk * (xp * xp + yp * yp) + 2.0 * (xp * ex + yp * ey) + exx + eyy;
        }
        double su[8], sv[8];
        gn_sums(o, n8, su, sv);
        if (dlt(P, n8, sx, sy, sr, ps)) {
          gauss_newton(P, n8, su, sv, ps, 4);
          score<false>(P, ps, thr2, o);
          if (o.count >= 6 && __builtin_popcount(o.cmask) >= 6) {
            gn_sums(o, n8, su, sv);
            gauss_newton(P, n8, su, sv, ps, 6);
            score<false>(P, ps, thr2, o);
          }
          count = o.count;
        }
      }
    }
  }
  float* slot = a.ws + ((size_t)p * a.iters + h) * kSlot;
  slot[0] = __int_as_float(count);
#pragma unroll
  for (int i = 0; i < 9; ++i) slot[1 + i] = (float)ps.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) slot[10 + i] = (float)ps.t[i];
}

// winner of problem p: (count desc, h asc).  Gate (t_cnt_out != nullptr): t_cnt[p] = 0 when no pose was found.
__global__ __launch_bounds__(64) void pnp_pick_kernel(const int32_t* cnt, int iters, const float* ws, int32_t* ok,
                                                      float* R, float* T, int32_t* n_inliers, int32_t* t_cnt_out) {
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = cnt[p];
  int bc = -1, bh = 0x7fffffff;
  if (n > 0) {
    for (int h = lane; h < iters; h += 64) {
      const int c = __float_as_int(ws[((size_t)p * iters + h) * kSlot]);
      if (c > bc) { bc = c; bh = h; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o, 64), oh = __shfl_xor(bh, o, 64);
    if (oc > bc || (oc == bc && oh < bh)) { bc = oc; bh = oh; }
  }
  if (lane != 0) return;
  float r[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) r[i] = 0.f;
  bool good = n > 0 && bc >= 6;
  if (good) {
    const float* s = ws + ((size_t)p * iters + bh) * kSlot;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      r[i] = s[1 + i];
      good = good && isfinite(r[i]);
    }
  }
  if (t_cnt_out) {
    if (n > 0 && !good) t_cnt_out[p] = 0;
    return;
  }
  ok[p] = good ? 1 : 0;
  n_inliers[p] = good ? bc : 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) R[(size_t)p * 9 + i] = good ? r[i] : 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) T[(size_t)p * 3 + i] = good ? r[9 + i] : 0.f;
}

// ---- pose remap of the augmentation chain (kd6d_pose_remap) ----------------------------------------------------------
// kd6d/libs/pnp.py's remap_pose, chained as kd6d/libs/augment.py::draw_params chains it: ONE LANE PER INSTANCE, the
// solver above with one observation per corner (n_k = 1, the sums are the observation itself).
struct RemapArgs {
  int n_inst, n_images, n_class;
  const int32_t* inst_img;
  const int32_t* inst_cls;
  const double* src_K;       // (n_images, 9)
  const double* src_R;       // (n_inst, 9)
  const double* src_T;       // (n_inst, 3)
  const float* box;          // (n_class, 8, 3)
  double dst_K[9];
  const double* M_resize;    // (n_images, 6)
  const double* M_ssr;       // (n_images, 6) or nullptr
  float* pose_out;           // (n_inst, 2, 12)
  int32_t* ok_out;           // (n_inst, 2)
};

// one stage: where (R, T) seen through Ks and mapped by M puts the corners -> the pose that puts them there through P.K
__device__ bool remap_stage(const Problem& P, const double* Ks, const double* M, const double* R, const double* T,
                            Pose& out) {
  double n8[8], sx[8], sy[8], sr[8], su[8], sv[8];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double X0 = P.X[k][0], X1 = P.X[k][1], X2 = P.X[k][2];
    const double c0 = R[0] * X0 + R[1] * X1 + R[2] * X2 + T[0];
    const double c1 = R[3] * X0 + R[4] * X1 + R[5] * X2 + T[1];
    const double c2 = R[6] * X0 + R[7] * X1 + R[8] * X2 + T[2];
    const double p0 = Ks[0] * c0 + Ks[1] * c1 + Ks[2] * c2;
    const double p1 = Ks[3] * c0 + Ks[4] * c1 + Ks[5] * c2;
    const double p2 = Ks[6] * c0 + Ks[7] * c1 + Ks[8] * c2;
    const double q0 = M[0] * p0 + M[1] * p1 + M[2] * p2, q1 = M[3] * p0 + M[4] * p1 + M[5] * p2;
    const double u = q0 / (p2 + 1e-8), v = q1 / (p2 + 1e-8);
    fin = fin && isfinite(u) && isfinite(v);
    const double x = P.a[0] * u + P.a[1] * v + P.a[2], y = P.b[0] * u + P.b[1] * v + P.b[2];
    n8[k] = 1.0; sx[k] = x; sy[k] = y; sr[k] = x * x + y * y;
    su[k] = u; sv[k] = v;
  }
  if (!fin || !dlt(P, n8, sx, sy, sr, out)) return false;
  gauss_newton(P, n8, su, sv, out, 20);
#pragma unroll
  for (int i = 0; i < 9; ++i) fin = fin && isfinite(out.R[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) fin = fin && isfinite(out.t[i]);
  return fin;
}

__global__ __launch_bounds__(64) void pose_remap_kernel(RemapArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_inst) return;
  float* out = a.pose_out + (size_t)i * 24;
  int32_t* ok = a.ok_out + (size_t)i * 2;
  const int img = a.inst_img[i], cls = a.inst_cls[i];
  if (img < 0 || img >= a.n_images || cls < 0 || cls >= a.n_class) {
    for (int j = 0; j < 24; ++j) out[j] = 0.f;
    ok[0] = ok[1] = 0;
    return;
  }
  float Kd[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) Kd[j] = (float)a.dst_K[j];
  Problem P;
  const bool valid = load_problem(P, nullptr, 0, a.box + (size_t)cls * 24, Kd);
  double R[9], T[3], Ks[9], M[6];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    R[j] = a.src_R[(size_t)i * 9 + j];
    Ks[j] = a.src_K[(size_t)img * 9 + j];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) T[j] = a.src_T[(size_t)i * 3 + j];
  int good = 0;
#pragma unroll 1                               // one copy of the solver
  for (int stage = 0; stage < 2; ++stage) {
    const double* Ms = stage == 0 ? a.M_resize : a.M_ssr;
    if (Ms) {                                  // stage 2 without M_ssr: a copy of stage 1 (R, T and good as they are)
#pragma unroll
      for (int j = 0; j < 6; ++j) M[j] = Ms[(size_t)img * 6 + j];
      Pose ps;
      good = valid && remap_stage(P, Ks, M, R, T, ps) ? 1 : 0;
      // the result (or, without one, the source pose) rounded to fp32: what is written and what the chain goes on from
#pragma unroll
      for (int j = 0; j < 9; ++j) R[j] = (double)(float)(good ? ps.R[j] : R[j]);
#pragma unroll
      for (int j = 0; j < 3; ++j) T[j] = (double)(float)(good ? ps.t[j] : T[j]);
#pragma unroll
      for (int j = 0; j < 9; ++j) Ks[j] = a.dst_K[j];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) out[stage * 12 + j] = (float)R[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) out[stage * 12 + 9 + j] = (float)T[j];
    ok[stage] = good;
  }
}

int launch(const char* name, int n_problems, const HypArgs& a, int32_t* ok, float* R, float* T, int32_t* n_inliers,
           int32_t* t_cnt_out, void* stream) {
  if (n_problems == 0) return KD6D_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pnp_hyp_kernel, dim3((unsigned)((a.iters + 63) / 64), (unsigned)n_problems), dim3(64), 0, st, a);
  KD6D_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(pnp_pick_kernel, dim3((unsigned)n_problems), dim3(64), 0, st, a.cnt, a.iters,
                     (const float*)a.ws, ok, R, T, n_inliers, t_cnt_out);
  KD6D_CHECK_LAUNCH(name);
  return KD6D_OK;
}

}  // namespace

extern "C" int64_t kd6d_pnp_workspace_floats(int n_problems, int iters) {
  if (n_problems < 0 || iters <= 0) return 0;
  return (int64_t)n_problems * iters * kSlot;
}

extern "C" int kd6d_pnp_ransac(int n_problems, int cap, const int32_t* cnt, const float* kp, const float* box,
                               const float* K, float reproj_err, int iters, uint64_t seed, int32_t* ok, float* R,
                               float* T, int32_t* n_inliers, float* workspace, int64_t workspace_floats,
                               void* stream) {
  KD6D_CHECK_ARG(cnt && kp && box && K && ok && R && T && n_inliers && workspace, "kd6d_pnp_ransac: null pointer");
  KD6D_CHECK_ARG(n_problems >= 0 && n_problems <= 65535, "kd6d_pnp_ransac: n_problems=%d (0 ... 65535)", n_problems);
  KD6D_CHECK_ARG(cap >= 1 && cap <= KD6D_PNP_MAX_CAP, "kd6d_pnp_ransac: cap=%d (1 ... %d)", cap, KD6D_PNP_MAX_CAP);
  KD6D_CHECK_ARG(iters > 0 && iters <= kMaxIters, "kd6d_pnp_ransac: iters=%d (1 ... %d)", iters, kMaxIters);
  KD6D_CHECK_ARG(reproj_err > 0.f && reproj_err < 1e30f, "kd6d_pnp_ransac: reproj_err=%g", (double)reproj_err);
  KD6D_CHECK_ARG(workspace_floats >= kd6d_pnp_workspace_floats(n_problems, iters),
                 "kd6d_pnp_ransac: workspace of %lld floats, needs %lld", (long long)workspace_floats,
                 (long long)kd6d_pnp_workspace_floats(n_problems, iters));
  HypArgs a = {};
  a.cap = cap; a.iters = iters; a.cnt = cnt; a.kp = kp; a.box = box; a.K = K; a.reproj_err = reproj_err;
  a.seed = seed; a.ws = workspace;
  return launch("kd6d_pnp_ransac", n_problems, a, ok, R, T, n_inliers, nullptr, stream);
}

extern "C" int kd6d_teacher_pnp_gate(const float* cls, int n_cls, float threshold, const int32_t* t_row,
                                     int32_t* t_cnt, const float* t_kp, int cap, int batch, const float* kp3d,
                                     int n_class_rows, const float* K, float reproj_err, int iters, uint64_t seed,
                                     float* workspace, int64_t workspace_floats, void* stream) {
  KD6D_CHECK_ARG(cls && t_row && t_cnt && t_kp && kp3d && K && workspace, "kd6d_teacher_pnp_gate: null pointer");
  KD6D_CHECK_ARG(batch >= 0 && batch <= 65535, "kd6d_teacher_pnp_gate: batch=%d (0 ... 65535)", batch);
  KD6D_CHECK_ARG(cap >= 1 && cap <= KD6D_PNP_MAX_CAP, "kd6d_teacher_pnp_gate: cap=%d (1 ... %d)", cap,
                 KD6D_PNP_MAX_CAP);
  KD6D_CHECK_ARG(n_cls >= 1 && n_cls <= 16 && n_cls <= n_class_rows,
                 "kd6d_teacher_pnp_gate: n_cls=%d (1 ... min(16, n_class_rows=%d))", n_cls, n_class_rows);
  KD6D_CHECK_ARG(iters > 0 && iters <= kMaxIters, "kd6d_teacher_pnp_gate: iters=%d (1 ... %d)", iters, kMaxIters);
  KD6D_CHECK_ARG(reproj_err > 0.f && reproj_err < 1e30f, "kd6d_teacher_pnp_gate: reproj_err=%g", (double)reproj_err);
  KD6D_CHECK_ARG(workspace_floats >= kd6d_pnp_workspace_floats(batch, iters),
                 "kd6d_teacher_pnp_gate: workspace of %lld floats, needs %lld", (long long)workspace_floats,
                 (long long)kd6d_pnp_workspace_floats(batch, iters));
  HypArgs a = {};
  a.cap = cap; a.iters = iters; a.cnt = t_cnt; a.kp = t_kp; a.box = kp3d; a.K = K; a.reproj_err = reproj_err;
  a.seed = seed; a.cls = cls; a.t_row = t_row; a.n_cls = n_cls; a.n_class_rows = n_class_rows;
  a.threshold = threshold; a.ws = workspace;
  return launch("kd6d_teacher_pnp_gate", batch, a, nullptr, nullptr, nullptr, nullptr, t_cnt, stream);
}

extern "C" int kd6d_pose_remap(int n_inst, int n_images, int n_class, const int32_t* inst_img, const int32_t* inst_cls,
                               const double* src_K, const double* src_R, const double* src_T, const float* box,
                               const double* dst_K_host, const double* M_resize, const double* M_ssr, float* pose_out,
                               int32_t* ok_out, void* stream) {
  KD6D_CHECK_ARG(inst_img && inst_cls && src_K && src_R && src_T && box && dst_K_host && M_resize && pose_out && ok_out,
                 "kd6d_pose_remap: null pointer");
  KD6D_CHECK_ARG(n_inst > 0 && n_inst <= (1 << 24), "kd6d_pose_remap: n_inst=%d (1 ... %d)", n_inst, 1 << 24);
  KD6D_CHECK_ARG(n_images > 0, "kd6d_pose_remap: n_images=%d (>= 1)", n_images);
  KD6D_CHECK_ARG(n_class > 0, "kd6d_pose_remap: n_class=%d (>= 1)", n_class);
  RemapArgs a = {};
  a.n_inst = n_inst; a.n_images = n_images; a.n_class = n_class; a.inst_img = inst_img; a.inst_cls = inst_cls;
  a.src_K = src_K; a.src_R = src_R; a.src_T = src_T; a.box = box; a.M_resize = M_resize; a.M_ssr = M_ssr;
  a.pose_out = pose_out; a.ok_out = ok_out;
  for (int j = 0; j < 9; ++j) a.dst_K[j] = dst_K_host[j];
  hipLaunchKernelGGL(pose_remap_kernel, dim3((unsigned)((n_inst + 63) / 64)), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  KD6D_CHECK_LAUNCH("kd6d_pose_remap");
  return KD6D_OK;
}
