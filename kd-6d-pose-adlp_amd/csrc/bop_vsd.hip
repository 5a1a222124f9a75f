// BOP's VSD (visible surface discrepancy) on the GPU: a depth rasteriser and the per-pixel visibility comparison of a
// whole batch of (ground truth, estimate) pairs -- kd6d/libs/bop_metrics.py::render_depth_host / vsd_errors_host are
// the float64 definitions.
//
// Rasteriser contract (host and kernel alike).  K = [fx s cx; 0 fy cy; 0 0 1].  A vertex X = R v + T with X.z > 0
// projects to u = (fx X.x + s X.y) / X.z + cx, v = fy X.y / X.z + cy; pixel (x, y) has its centre at integer
// coordinates.  A triangle with any vertex at z <= 0 is dropped whole (no near-plane clipping); a triangle whose
// projected area is zero is skipped; both windings are drawn.  A pixel centre is covered when the three edge functions
// all have the sign of the area or are zero (inclusive edges: a closed surface has no cracks).  Its depth is the depth
// of the triangle's plane along the pixel's ray r = K^-1 (x, y, 1): z = (n . X0) / (n . r), n = (X1 - X0) x (X2 - X0),
// clamped to the z range of the three vertices (n . r == 0: the nearest vertex z).  The kernel forms n in the object
// frame, n_o = (v1 - v0) x (v2 - v0), n = R n_o and n . X0 = n_o . v0 + n . T, so that the ~1000 mm translation never
// meets a ~50 mm vertex before the cross product.  The pixel keeps the minimum over the triangles; background = 0.
//
//   vsd_roi_kernel<NB>   ONE WORKGROUP PER ITEM: the bounding box of the projected vertices (z > 0) under the item's NB
//                        poses, widened by one pixel and clipped to the image -> roi[item] = (x0, y0, x1, y1), empty
//                        (x1 < x0) when nothing can be drawn or when an offset, count or frame index of the item lies
//                        outside its pool (such an item is never dereferenced again: its maps and counts stay zero).
//   vsd_tile_kernel<NB>  ONE WORKGROUP PER (ITEM, 64 x 64 TILE OF ITS ROI), 256 threads.  NB z-buffers of the tile live
//                        in LDS (NB x 16 KiB).  The lanes walk the mesh's triangles, one triangle per lane: transform,
//                        project, reject by the bounding box against the tile, rasterise the rest.  A depth is a
//                        positive float, its bit pattern orders like an unsigned integer: the z-test is an LDS
//                        unsigned-integer atomic min (integer LDS atomics are an order of magnitude cheaper here than
//                        float ones, profiles/r04_atomic_rate.md); there is no global z-buffer.  The grid is
//                        (items, tiles of the whole image); the workgroups past an item's own tile count exit
//                        wave-uniformly.  NB == 1 (kd6d_render_depth) writes the tile out.  NB == 2 (kd6d_bop_vsd)
//                        reads the tile of the frame's depth image after the barrier, forms the three distances per
//                        pixel (depth x the length of the pixel's ray), applies the bop19 visibility rule and counts
//                        n_u, n_inter and, per tau, the cost numerator; the counts are summed over the waves in LDS and
//                        added to the problem's int32 counters with integer atomics.
//   vsd_err_kernel       err[p][k] = cost_k / n_u (1 when n_u == 0): one division of two exact integers.
//
// Bitwise property: minima and integer sums are exact in any order.  There is no floating-point atomic and no
// accumulator; counts[p] is a pure function of problem p's own inputs -- the same alone and inside any batch, under any
// order of the mesh's faces and with a face repeated.
#include <math.h>

#include "kd6d_common.h"
#include "kd6d_raster.h"

namespace {

constexpr int kMaxTau = 16;

struct VsdArgs {
  const float* verts;
  const int32_t* faces;
  int n_verts, n_faces;
  const int32_t* voff;
  const int32_t* vcnt;
  const int32_t* foff;
  const int32_t* fcnt;
  const float* K;
  const float* R[2];                     // ground truth, estimate (render: pose, unused)
  const float* T[2];
  const float* diam;
  const int32_t* frame;
  const float* depth;
  int n_img, H, W;
  float delta;
  float tau[kMaxTau];
  int n_tau;
  int32_t* roi;
  int32_t* counts;
  float* err;
  float* out;
  int n;
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <int NB>
__global__ __launch_bounds__(kThreads) void vsd_roi_kernel(VsdArgs a) {
  __shared__ float red[kWaves][4];
  const int p = blockIdx.x;
  const int tid = threadIdx.x;
  const int vo = a.voff[p], vc = a.vcnt[p], fo = a.foff[p], fc = a.fcnt[p];
  bool ok = vo >= 0 && vc >= 1 && (long long)vo + vc <= a.n_verts && fo >= 0 && fc >= 1 && (long long)fo + fc <= a.n_faces;
  if (NB == 2) ok = ok && a.frame[p] >= 0 && a.frame[p] < a.n_img;
  int32_t* roi = a.roi + (size_t)p * 4;
  if (!ok) {                             // wave-uniform: the item's own scalars decide
    if (tid == 0) { roi[0] = 0; roi[1] = 0; roi[2] = -1; roi[3] = -1; }
    return;
  }
  const Cam cam = load_cam(a.K + (size_t)p * 9);
  Pose q[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) q[b] = load_pose(a.R[b], a.T[b], p);
  item_roi<NB>(a.verts + (size_t)vo * 3, vc, cam, q, a.H, a.W, red, roi, tid);
}

// One pose of the mesh into one z-buffer of the tile (ox, oy, w, h): the z-test is an LDS unsigned-integer minimum.
__device__ __forceinline__ void rasterise_depth(const VsdArgs& a, int p, const Cam& cam, const Pose& q, int ox, int oy,
                                                int w, int h, unsigned* zb, int tid) {
  rasterise(a.verts + (size_t)a.voff[p] * 3, a.faces + (size_t)a.foff[p] * 3, a.vcnt[p], a.fcnt[p], a.H, a.W, cam, q, ox,
            oy, w, h, tid, [zb](int i, float z, int) { atomicMin(&zb[i], __float_as_uint(z)); });
}

__device__ __forceinline__ bool visible(float t, float m, float delta) {
  return (t > 0.f && m > 0.f && m - t <= delta) || (t == 0.f && m > 0.f);
}

template <int NB>
__global__ __launch_bounds__(kThreads) void vsd_tile_kernel(VsdArgs a) {
  __shared__ unsigned zb[NB][kTile * kTile];
  __shared__ int cnt[2 + kMaxTau];
  const int p = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t* roi = a.roi + (size_t)p * 4;
  const int x0 = roi[0], y0 = roi[1], x1 = roi[2], y1 = roi[3];
  if (x1 < x0 || y1 < y0) return;
  const int tw = (x1 - x0 + kTile) / kTile, th = (y1 - y0 + kTile) / kTile;
  const int t = blockIdx.y;
  if (t >= tw * th) return;              // the grid is sized for a region of interest as large as the image
  const int ox = x0 + (t % tw) * kTile, oy = y0 + (t / tw) * kTile;
  const int w = min(kTile, x1 + 1 - ox), h = min(kTile, y1 + 1 - oy);
  for (int i = tid; i < NB * kTile * kTile; i += kThreads) (&zb[0][0])[i] = kEmpty;
  if (tid < 2 + kMaxTau) cnt[tid] = 0;
  __syncthreads();
  const Cam cam = load_cam(a.K + (size_t)p * 9);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const Pose q = load_pose(a.R[b], a.T[b], p);
    rasterise_depth(a, p, cam, q, ox, oy, w, h, zb[b], tid);
  }
  __syncthreads();

  if (NB == 1) {
    float* out = a.out + (size_t)p * a.H * a.W;
    for (int i = tid; i < kTile * kTile; i += kThreads) {
      const int lx = i % kTile, ly = i / kTile;
      if (lx < w && ly < h) {
        const unsigned z = zb[0][i];
        out[(size_t)(oy + ly) * a.W + ox + lx] = z == kEmpty ? 0.f : __uint_as_float(z);
      }
    }
    return;
  }

  const float* test = a.depth + (size_t)a.frame[p] * a.H * a.W;
  const float diam = a.diam[p];
  int n_u = 0, n_i = 0, far[kMaxTau];
#pragma unroll
  for (int k = 0; k < kMaxTau; ++k) far[k] = 0;
  for (int i = tid; i < kTile * kTile; i += kThreads) {
    const int lx = i % kTile, ly = i / kTile;
    if (lx >= w || ly >= h) continue;
    const unsigned zg = zb[0][i], ze = zb[NB - 1][i];
    if (zg == kEmpty && ze == kEmpty) continue;          // neither drawn: outside both visibility masks
    const float ry = ((float)(oy + ly) - cam.cy) / cam.fy;
    const float rx = ((float)(ox + lx) - cam.cx - cam.sk * ry) / cam.fx;
    const float len = sqrtf(fmaf(rx, rx, fmaf(ry, ry, 1.f)));
    const float dt = test[(size_t)(oy + ly) * a.W + ox + lx] * len;
    const float dg = zg == kEmpty ? 0.f : __uint_as_float(zg) * len;
    const float de = ze == kEmpty ? 0.f : __uint_as_float(ze) * len;
    const bool vg = visible(dt, dg, a.delta);
    const bool ve = visible(dt, de, a.delta) || (vg && de > 0.f);
    const bool both = vg && ve;
    n_u += (vg || ve) ? 1 : 0;
    n_i += both ? 1 : 0;
    const float ad = fabsf(dg - de);
#pragma unroll
    for (int k = 0; k < kMaxTau; ++k) far[k] += (k < a.n_tau && both && ad >= a.tau[k] * diam) ? 1 : 0;
  }
  const int n_c = n_u - n_i;             // per thread: the sums below are linear
  n_u = wave_sum_i(n_u);
  n_i = wave_sum_i(n_i);
#pragma unroll
  for (int k = 0; k < kMaxTau; ++k) far[k] = wave_sum_i(far[k] + n_c);
  if ((tid & 63) == 0) {
    __hip_atomic_fetch_add(&cnt[0], n_u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(&cnt[1], n_i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
    for (int k = 0; k < kMaxTau; ++k)
      __hip_atomic_fetch_add(&cnt[2 + k], far[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  if (tid < 2 + a.n_tau && cnt[tid] != 0)
    __hip_atomic_fetch_add(&a.counts[(size_t)p * (2 + a.n_tau) + tid], cnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void vsd_err_kernel(VsdArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n * a.n_tau) return;
  const int p = i / a.n_tau, k = i % a.n_tau;
  const int32_t* c = a.counts + (size_t)p * (2 + a.n_tau);
  a.err[i] = c[0] > 0 ? (float)c[2 + k] / (float)c[0] : 1.f;
}

int check_common(const char* who, int n, int n_verts, int n_faces, int H, int W) {
  KD6D_CHECK_ARG(n >= 0 && n <= 0x7fffff00, "%s: n=%d (>= 0)", who, n);
  KD6D_CHECK_ARG(n_verts >= 0 && n_faces >= 0, "%s: pools of %d vertices and %d faces", who, n_verts, n_faces);
  KD6D_CHECK_ARG(H >= 1 && W >= 1 && (long long)cdiv(H, kTile) * cdiv(W, kTile) <= 65535 && (long long)H * W < (1LL << 31),
                 "%s: image of %d x %d pixels", who, W, H);
  return KD6D_OK;
}

}  // namespace

extern "C" int64_t kd6d_bop_vsd_workspace_ints(int n) { return 4 * (int64_t)(n > 0 ? n : 0); }

extern "C" int kd6d_render_depth(int n, const float* verts, int n_verts, const int32_t* faces, int n_faces,
                                 const int32_t* voff, const int32_t* vcnt, const int32_t* foff, const int32_t* fcnt,
                                 const float* K, const float* R, const float* T, int H, int W, int32_t* workspace,
                                 int64_t workspace_ints, float* depth_out, void* stream) {
  if (check_common("kd6d_render_depth", n, n_verts, n_faces, H, W) != KD6D_OK) return KD6D_ERR_ARG;
  if (n == 0) return KD6D_OK;
  KD6D_CHECK_ARG(verts && faces && voff && vcnt && foff && fcnt && K && R && T && workspace && depth_out,
                 "kd6d_render_depth: null pointer");
  KD6D_CHECK_ARG(workspace_ints >= kd6d_bop_vsd_workspace_ints(n), "kd6d_render_depth: workspace of %lld ints, %d items "
                 "need %lld (kd6d_bop_vsd_workspace_ints)", (long long)workspace_ints, n,
                 (long long)kd6d_bop_vsd_workspace_ints(n));
  VsdArgs a = {};
  a.verts = verts; a.faces = faces; a.n_verts = n_verts; a.n_faces = n_faces;
  a.voff = voff; a.vcnt = vcnt; a.foff = foff; a.fcnt = fcnt;
  a.K = K; a.R[0] = a.R[1] = R; a.T[0] = a.T[1] = T;
  a.H = H; a.W = W; a.roi = workspace; a.out = depth_out; a.n = n;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  KD6D_CHECK_ARG(hipMemsetAsync(depth_out, 0, (size_t)n * H * W * sizeof(float), s) == hipSuccess,
                 "kd6d_render_depth: clearing the maps failed");
  hipLaunchKernelGGL(vsd_roi_kernel<1>, dim3((unsigned)n), dim3(kThreads), 0, s, a);
  KD6D_CHECK_LAUNCH("kd6d_render_depth");
  hipLaunchKernelGGL(vsd_tile_kernel<1>, dim3((unsigned)n, (unsigned)(cdiv(H, kTile) * cdiv(W, kTile))), dim3(kThreads),
                     0, s, a);
  KD6D_CHECK_LAUNCH("kd6d_render_depth");
  return KD6D_OK;
}

extern "C" int kd6d_bop_vsd(int n, const float* verts, int n_verts, const int32_t* faces, int n_faces,
                            const int32_t* voff, const int32_t* vcnt, const int32_t* foff, const int32_t* fcnt,
                            const float* K, const float* Rg, const float* Tg, const float* Rp, const float* Tp,
                            const float* diameter, const int32_t* frame, const float* depth, int n_img, int H, int W,
                            float delta, const float* tau_host, int n_tau, int32_t* workspace, int64_t workspace_ints,
                            int32_t* counts, float* err, void* stream) {
  if (check_common("kd6d_bop_vsd", n, n_verts, n_faces, H, W) != KD6D_OK) return KD6D_ERR_ARG;
  KD6D_CHECK_ARG(n_tau >= 1 && n_tau <= kMaxTau, "kd6d_bop_vsd: n_tau=%d (1 ... %d)", n_tau, kMaxTau);
  KD6D_CHECK_ARG(n_img >= 0, "kd6d_bop_vsd: n_img=%d (>= 0)", n_img);
  if (n == 0) return KD6D_OK;
  KD6D_CHECK_ARG(verts && faces && voff && vcnt && foff && fcnt && K && Rg && Tg && Rp && Tp && diameter && frame &&
                 depth && tau_host && workspace && counts && err, "kd6d_bop_vsd: null pointer");
  KD6D_CHECK_ARG(workspace_ints >= kd6d_bop_vsd_workspace_ints(n), "kd6d_bop_vsd: workspace of %lld ints, %d problems "
                 "need %lld (kd6d_bop_vsd_workspace_ints)", (long long)workspace_ints, n,
                 (long long)kd6d_bop_vsd_workspace_ints(n));
  KD6D_CHECK_ARG((long long)n * n_tau < (1LL << 31), "kd6d_bop_vsd: %d problems x %d taus", n, n_tau);
  VsdArgs a = {};
  a.verts = verts; a.faces = faces; a.n_verts = n_verts; a.n_faces = n_faces;
  a.voff = voff; a.vcnt = vcnt; a.foff = foff; a.fcnt = fcnt;
  a.K = K; a.R[0] = Rg; a.R[1] = Rp; a.T[0] = Tg; a.T[1] = Tp;
  a.diam = diameter; a.frame = frame; a.depth = depth; a.n_img = n_img; a.H = H; a.W = W;
  a.delta = delta; a.n_tau = n_tau;
  for (int k = 0; k < n_tau; ++k) a.tau[k] = tau_host[k];
  a.roi = workspace; a.counts = counts; a.err = err; a.n = n;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  KD6D_CHECK_ARG(hipMemsetAsync(counts, 0, (size_t)n * (2 + n_tau) * sizeof(int32_t), s) == hipSuccess,
                 "kd6d_bop_vsd: clearing the counters failed");
  hipLaunchKernelGGL(vsd_roi_kernel<2>, dim3((unsigned)n), dim3(kThreads), 0, s, a);
  KD6D_CHECK_LAUNCH("kd6d_bop_vsd");
  hipLaunchKernelGGL(vsd_tile_kernel<2>, dim3((unsigned)n, (unsigned)(cdiv(H, kTile) * cdiv(W, kTile))), dim3(kThreads),
                     0, s, a);
  KD6D_CHECK_LAUNCH("kd6d_bop_vsd");
  hipLaunchKernelGGL(vsd_err_kernel, dim3((unsigned)cdiv((long long)n * n_tau, kThreads)), dim3(kThreads), 0, s, a);
  KD6D_CHECK_LAUNCH("kd6d_bop_vsd");
  return KD6D_OK;
}
