// Pose errors of the evaluation path on the GPU: libs/utils.py::compute_pose_diff of the reference
// (kd6d/libs/evaluate.py::compute_pose_diff here) for a whole batch of (ground truth, prediction) pairs.
//
// Problem p scores n = vcnt[p] <= max_v <= 1000 vertices m_i of one mesh (verts[voff[p] + vidx[p][i]], or
// verts[voff[p] + i] without an index table) under the poses (Rg, Tg) and (Rp, Tp):
//   err[p][0] = mean_i |Rg m_i + Tg - (Rp m_j + Tp)|,  j = i, or (sym) the j with the smallest such distance
//   err[p][1] = mean_i |pi(Rg m_i + Tg) - pi(Rp m_j + Tp)|,  pi(x) = (K x)_{0,1} / ((K x)_2 + 1e-8)
//
//   pose_err_kernel  ONE WORKGROUP PER PROBLEM, 256 threads.  The predicted set b_j = Rp m_j is staged once in LDS
//                    (float4 per vertex, 16 KB at 1000); lane t owns the ground-truth vertices t, t + 256, ... (at
//                    most 4) and keeps a_i = Rg m_i + (Tg - Tp) in registers.  Differences are a_i - b_j: both terms
//                    are object sized (~100 mm), not camera-frame points (~1000 mm), which keeps an order of magnitude
//                    more of fp32.  In the symmetric case a lane walks j = 0 ... n-1 with one ds_read_b128 at a
//                    wave-uniform address (a broadcast, no bank conflict) per j, against its 4 vertices, keeping a
//                    running (min d^2, j) with a strict `<`: ties go to the lowest j, as np.argmin does.
//
// The two sums are per-lane partials (own vertices in ascending order), a fixed butterfly inside each wave and the
// four wave totals added in wave order: no atomics, nothing depends on the batch around the problem, two launches
// agree bit for bit.
#include <math.h>

#include "kd6d_common.h"

namespace {

constexpr int kMaxV = KD6D_POSE_ERR_MAX_V;   // the reference's subsample size (utils.py:722)
constexpr int kThreads = 256;
constexpr int kOwn = (kMaxV + kThreads - 1) / kThreads;

struct PoseErrArgs {
  int max_v;
  const float* verts;
  const int32_t* voff;
  const int32_t* vcnt;
  const int32_t* vidx;
  const float* K;
  const float* Rg;
  const float* Tg;
  const float* Rp;
  const float* Tp;
  const int32_t* sym;
  float* err;
  int32_t* nn;
};

__device__ __forceinline__ void rot3(const float* R, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = fmaf(R[2], z, fmaf(R[1], y, R[0] * x));
  oy = fmaf(R[5], z, fmaf(R[4], y, R[3] * x));
  oz = fmaf(R[8], z, fmaf(R[7], y, R[6] * x));
}

__device__ __forceinline__ void pinhole(const float* K, float x, float y, float z, float& u, float& v) {
  float p0, p1, p2;
  rot3(K, x, y, z, p0, p1, p2);
  const float w = p2 + 1e-8f;
  u = p0 / w;
  v = p1 / w;
}

__global__ __launch_bounds__(kThreads) void pose_err_kernel(PoseErrArgs a) {
  __shared__ f32x4_t pred[kMaxV];
  __shared__ float wsum[2][kThreads / 64];
  const int p = blockIdx.x;
  const int tid = threadIdx.x;
  const int n = min(max(a.vcnt[p], 0), a.max_v);
  const float* mesh = a.verts + (size_t)a.voff[p] * 3;
  const int32_t* idx = a.vidx ? a.vidx + (size_t)p * a.max_v : nullptr;
  float K[9], Rg[9], Rp[9], Tp[3], dT[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    K[i] = a.K[(size_t)p * 9 + i];
    Rg[i] = a.Rg[(size_t)p * 9 + i];
    Rp[i] = a.Rp[(size_t)p * 9 + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Tp[i] = a.Tp[(size_t)p * 3 + i];
    dT[i] = a.Tg[(size_t)p * 3 + i] - Tp[i];
  }
  const bool sym = a.sym[p] != 0;

  float ax[kOwn], ay[kOwn], az[kOwn];
#pragma unroll
  for (int k = 0; k < kOwn; ++k) {
    const int i = tid + k * kThreads;
    ax[k] = ay[k] = az[k] = 0.f;
    if (i < n) {
      const float* m = mesh + (size_t)(idx ? idx[i] : i) * 3;
      const float mx = m[0], my = m[1], mz = m[2];
      float bx, by, bz;
      rot3(Rp, mx, my, mz, bx, by, bz);
      f32x4_t b = {bx, by, bz, 0.f};
      pred[i] = b;
      rot3(Rg, mx, my, mz, ax[k], ay[k], az[k]);
      ax[k] += dT[0]; ay[k] += dT[1]; az[k] += dT[2];
    }
  }
  __syncthreads();

  int best[kOwn];
#pragma unroll
  for (int k = 0; k < kOwn; ++k) best[k] = tid + k * kThreads;
  if (sym) {
    float bd[kOwn];
#pragma unroll
    for (int k = 0; k < kOwn; ++k) { bd[k] = INFINITY; best[k] = 0; }
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
      const f32x4_t b = pred[j];
#pragma unroll
      for (int k = 0; k < kOwn; ++k) {
        const float dx = ax[k] - b.x, dy = ay[k] - b.y, dz = az[k] - b.z;
        const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const bool lt = d2 < bd[k];
        bd[k] = lt ? d2 : bd[k];
        best[k] = lt ? j : best[k];
      }
    }
  }

  float s3 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < kOwn; ++k) {
    const int i = tid + k * kThreads;
    if (i < n) {
      const f32x4_t b = pred[best[k]];
      const float dx = ax[k] - b.x, dy = ay[k] - b.y, dz = az[k] - b.z;
      s3 += sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
      float ua, va, ub, vb;
      pinhole(K, ax[k] + Tp[0], ay[k] + Tp[1], az[k] + Tp[2], ua, va);
      pinhole(K, b.x + Tp[0], b.y + Tp[1], b.z + Tp[2], ub, vb);
      const float du = ua - ub, dv = va - vb;
      s2 += sqrtf(fmaf(dv, dv, du * du));
    }
    if (a.nn && i < a.max_v) a.nn[(size_t)p * a.max_v + i] = i < n ? best[k] : -1;
  }
  s3 = wave_sum(s3);
  s2 = wave_sum(s2);
  if ((tid & 63) == 0) { wsum[0][tid >> 6] = s3; wsum[1][tid >> 6] = s2; }
  __syncthreads();
  if (tid < 2) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) t += wsum[tid][w];
    a.err[(size_t)p * 2 + tid] = n > 0 ? t / (float)n : 0.f;
  }
}

}  // namespace

extern "C" int kd6d_pose_errors(int n_problems, int max_v, const float* verts, const int32_t* voff, const int32_t* vcnt,
                                const int32_t* vidx, const float* K, const float* Rg, const float* Tg, const float* Rp,
                                const float* Tp, const int32_t* sym, float* err, int32_t* nn, void* stream) {
  KD6D_CHECK_ARG(verts && voff && vcnt && K && Rg && Tg && Rp && Tp && sym && err, "kd6d_pose_errors: null pointer");
  KD6D_CHECK_ARG(n_problems >= 0, "kd6d_pose_errors: n_problems=%d (>= 0)", n_problems);
  KD6D_CHECK_ARG(max_v >= 1 && max_v <= kMaxV, "kd6d_pose_errors: max_v=%d (1 ... %d)", max_v, kMaxV);
  if (n_problems == 0) return KD6D_OK;
  PoseErrArgs a = {max_v, verts, voff, vcnt, vidx, K, Rg, Tg, Rp, Tp, sym, err, nn};
  hipLaunchKernelGGL(pose_err_kernel, dim3((unsigned)n_problems), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  KD6D_CHECK_LAUNCH("kd6d_pose_errors");
  return KD6D_OK;
}
