// BOP pose errors on the GPU: MSSD and MSPD (maximum symmetry-aware surface / projection distance) of a whole batch
// of (ground truth, prediction) pairs -- kd6d/libs/bop_metrics.py::bop_errors_host is the float64 definition.
//
// Problem p scores ALL n = vcnt[p] vertices v_i = verts[voff[p] + i] of one mesh under the poses (Rg, Tg), (Rp, Tp)
// and the symmetry transforms S_s = syms[soff[p] + s] (12 floats: R row-major, then t), s < scnt[p]:
//   err[p][0] = min_s max_i |(Rp v_i + Tp) - (Rg (S_s v_i) + Tg)|                                   (mssd)
//   err[p][1] = min_s max_i |pi(Rp v_i + Tp) - pi(Rg (S_s v_i) + Tg)|,  pi(q) = (K q)_{0,1} / ((K q)_2 + 1e-8)  (mspd)
//
//   bop_max_kernel   ONE WORKGROUP PER (PROBLEM, TILE OF 16 SYMMETRIES), 256 threads, one lane per vertex (vertex t,
//                    t + 256, ... streamed straight from global memory: each is read once per tile and the pool stays
//                    in L2).  The first lanes compose M_s = Rg S_R and c_s = Rg S_t + (Tg - Tp) once per (problem,
//                    symmetry) into LDS (three float4 per symmetry = the rows of [M_s | c_s]); the vertex loop reads
//                    them back with ds_read_b128 at a wave-uniform address (a broadcast: no bank conflict); they do
//                    not depend on the vertex, so the compiler holds the tile in registers across the loop (NS = 16:
//                    244 VGPRs, no scratch, two waves per SIMD -- the loop is VALU-bound, ~45 instructions per
//                    (vertex, symmetry) with the two correctly rounded divisions, and 16 independent chains).  A lane
//                    forms a_s = M_s v + c_s and b = Rp v, the difference a_s - b of two object-sized vectors (the
//                    ~1000 mm translation never meets a ~50 mm vertex in one fp32 sum, as in pose_err.hip), and keeps
//                    2 x NS running maxima of the SQUARED distances in registers.  NS = 1, 2, 4, 8 or 16 is the
//                    tile's symmetry count rounded up (a wave-uniform switch over five instantiations): an
//                    asymmetric object pays for one symmetry, not sixteen; the slots past the count repeat the
//                    tile's first symmetry, which cannot change a minimum.  After the loop one wave_max per slot,
//                    the four wave results through LDS, one sqrt per (problem, symmetry), written to the workspace.
//   bop_min_kernel   ONE WAVE PER PROBLEM: the minimum over the problem's workspace row.
//
// max and min of floats are exact in any order and sqrt is monotonic: no atomics, no accumulators, no cross-workgroup
// barrier; err[p] is a pure function of problem p's own inputs -- independent of the batch, of the order of its
// vertices and of the order of its symmetries, bit for bit.
#include <math.h>

#include "kd6d_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 16;            // symmetries per workgroup

struct BopErrArgs {
  const float* verts;
  const int32_t* voff;
  const int32_t* vcnt;
  const float* syms;
  const int32_t* soff;
  const int32_t* scnt;
  const float* K;
  const float* Rg;
  const float* Tg;
  const float* Rp;
  const float* Tp;
  float* ws;
  int cap;                           // workspace slots per problem
  float* err;
  int n_problems;
};

__device__ __forceinline__ void mul3(const float* R, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = fmaf(R[2], z, fmaf(R[1], y, R[0] * x));
  oy = fmaf(R[5], z, fmaf(R[4], y, R[3] * x));
  oz = fmaf(R[8], z, fmaf(R[7], y, R[6] * x));
}

__device__ __forceinline__ void project(const float* K, float x, float y, float z, float& u, float& v) {
  float p0, p1, p2;
  mul3(K, x, y, z, p0, p1, p2);
  const float w = p2 + 1e-8f;
  u = p0 / w;
  v = p1 / w;
}

// symmetries in use of a problem: scnt <= 0 is the identity alone; more than the workspace row holds are not scored
__device__ __forceinline__ int sym_count(int scnt, int cap) { return min(max(scnt, 1), cap); }

template <int NS>
__device__ __forceinline__ void vertex_loop(const float* mesh, int n, int tid, const float* K, const float* Rp,
                                            const float* Tp, const f32x4_t* tile, float* wmax) {
  float a3[NS], a2[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) a3[s] = a2[s] = 0.f;
  for (int i = tid; i < n; i += kThreads) {
    const float* m = mesh + (size_t)i * 3;
    const float x = m[0], y = m[1], z = m[2];
    float bx, by, bz, ub, vb;
    mul3(Rp, x, y, z, bx, by, bz);
    project(K, bx + Tp[0], by + Tp[1], bz + Tp[2], ub, vb);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const f32x4_t r0 = tile[3 * s], r1 = tile[3 * s + 1], r2 = tile[3 * s + 2];
      const float ax = fmaf(r0.z, z, fmaf(r0.y, y, r0.x * x)) + r0.w;
      const float ay = fmaf(r1.z, z, fmaf(r1.y, y, r1.x * x)) + r1.w;
      const float az = fmaf(r2.z, z, fmaf(r2.y, y, r2.x * x)) + r2.w;
      const float dx = ax - bx, dy = ay - by, dz = az - bz;
      a3[s] = fmaxf(a3[s], fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
      float ua, va;
      project(K, ax + Tp[0], ay + Tp[1], az + Tp[2], ua, va);
      const float du = ua - ub, dv = va - vb;
      a2[s] = fmaxf(a2[s], fmaf(dv, dv, du * du));
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float w3 = wave_max(a3[s]), w2 = wave_max(a2[s]);
    if ((tid & 63) == 0) { wmax[(tid >> 6) * 2 * kTile + s] = w3; wmax[(tid >> 6) * 2 * kTile + kTile + s] = w2; }
  }
}

__global__ __launch_bounds__(kThreads) void bop_max_kernel(BopErrArgs a) {
  __shared__ f32x4_t tile[kTile * 3];
  __shared__ float wmax[kWaves][2 * kTile];
  const int p = blockIdx.x;
  const int tid = threadIdx.x;
  const int ns_all = sym_count(a.scnt[p], a.cap);
  const int s0 = blockIdx.y * kTile;
  if (s0 >= ns_all) return;            // the grid is sized for the largest symmetry set of the batch
  const int ns = min(ns_all - s0, kTile);
  const int n = max(a.vcnt[p], 0);
  const float* mesh = a.verts + (size_t)a.voff[p] * 3;
  float K[9], Rp[9], Tp[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    K[i] = a.K[(size_t)p * 9 + i];
    Rp[i] = a.Rp[(size_t)p * 9 + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) Tp[i] = a.Tp[(size_t)p * 3 + i];

  if (tid < kTile) {
    // slot tid holds symmetry s0 + tid, or (past the tile's count) the tile's first symmetry again
    const int s = s0 + (tid < ns ? tid : 0);
    float S[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    if (a.scnt[p] > 0) {
      const float* src = a.syms + ((size_t)a.soff[p] + s) * 12;
#pragma unroll
      for (int i = 0; i < 12; ++i) S[i] = src[i];
    }
    float Rg[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rg[i] = a.Rg[(size_t)p * 9 + i];
    float M[9], c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        M[3 * r + k] = fmaf(Rg[3 * r + 2], S[6 + k], fmaf(Rg[3 * r + 1], S[3 + k], Rg[3 * r] * S[k]));
      const float rt = fmaf(Rg[3 * r + 2], S[11], fmaf(Rg[3 * r + 1], S[10], Rg[3 * r] * S[9]));
      c[r] = rt + (a.Tg[(size_t)p * 3 + r] - Tp[r]);
      f32x4_t row = {M[3 * r], M[3 * r + 1], M[3 * r + 2], c[r]};
      tile[3 * tid + r] = row;
    }
  }
  __syncthreads();

  if (ns <= 1) vertex_loop<1>(mesh, n, tid, K, Rp, Tp, tile, &wmax[0][0]);
  else if (ns <= 2) vertex_loop<2>(mesh, n, tid, K, Rp, Tp, tile, &wmax[0][0]);
  else if (ns <= 4) vertex_loop<4>(mesh, n, tid, K, Rp, Tp, tile, &wmax[0][0]);
  else if (ns <= 8) vertex_loop<8>(mesh, n, tid, K, Rp, Tp, tile, &wmax[0][0]);
  else vertex_loop<16>(mesh, n, tid, K, Rp, Tp, tile, &wmax[0][0]);
  __syncthreads();
  if (tid < 2 * kTile) {
    const int s = tid & (kTile - 1), which = tid / kTile;
    if (s < ns) {
      float t = wmax[0][tid];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) t = fmaxf(t, wmax[w][tid]);
      a.ws[((size_t)p * a.cap + s0 + s) * 2 + which] = sqrtf(t);
    }
  }
}

__global__ __launch_bounds__(kThreads) void bop_min_kernel(BopErrArgs a) {
  const int p = blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= a.n_problems) return;
  const int ns = sym_count(a.scnt[p], a.cap);
  const float* row = a.ws + (size_t)p * a.cap * 2;
  float e3 = INFINITY, e2 = INFINITY;
  for (int s = lane; s < ns; s += 64) {
    e3 = fminf(e3, row[2 * s]);
    e2 = fminf(e2, row[2 * s + 1]);
  }
  e3 = -wave_max(-e3);
  e2 = -wave_max(-e2);
  if (lane == 0) {
    a.err[(size_t)p * 2] = e3;
    a.err[(size_t)p * 2 + 1] = e2;
  }
}

}  // namespace

extern "C" int64_t kd6d_bop_errors_workspace_floats(int n_problems, int max_scnt) {
  return (int64_t)(n_problems > 0 ? n_problems : 0) * (max_scnt > 1 ? max_scnt : 1) * 2;
}

extern "C" int kd6d_bop_errors(int n_problems, const float* verts, const int32_t* voff, const int32_t* vcnt,
                               const float* syms, const int32_t* soff, const int32_t* scnt, const float* K,
                               const float* Rg, const float* Tg, const float* Rp, const float* Tp, float* workspace,
                               int64_t workspace_floats, float* err, void* stream) {
  KD6D_CHECK_ARG(n_problems >= 0, "kd6d_bop_errors: n_problems=%d (>= 0)", n_problems);
  if (n_problems == 0) return KD6D_OK;
  KD6D_CHECK_ARG(verts && voff && vcnt && syms && soff && scnt && K && Rg && Tg && Rp && Tp && workspace && err,
                 "kd6d_bop_errors: null pointer");
  KD6D_CHECK_ARG(workspace_floats >= 2 * (int64_t)n_problems,
                 "kd6d_bop_errors: workspace of %lld floats, %d problems need at least %lld "
                 "(kd6d_bop_errors_workspace_floats)", (long long)workspace_floats, n_problems, 2LL * n_problems);
  const int64_t cap = workspace_floats / (2 * (int64_t)n_problems);
  const int64_t tiles = (cap + kTile - 1) / kTile;
  KD6D_CHECK_ARG(tiles <= 65535, "kd6d_bop_errors: a workspace row of %lld symmetries (at most %d)", (long long)cap,
                 65535 * kTile);
  BopErrArgs a = {verts, voff, vcnt, syms, soff, scnt, K, Rg, Tg, Rp, Tp, workspace, (int)cap, err, n_problems};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bop_max_kernel, dim3((unsigned)n_problems, (unsigned)tiles), dim3(kThreads), 0, s, a);
  KD6D_CHECK_LAUNCH("kd6d_bop_errors");
  hipLaunchKernelGGL(bop_min_kernel, dim3((unsigned)cdiv(n_problems, kWaves)), dim3(kThreads), 0, s, a);
  KD6D_CHECK_LAUNCH("kd6d_bop_errors");
  return KD6D_OK;
}
