// Kernel distances (MMD) between weighted point sets, forward value AND gradient in one launch: the `gaussian`,
// `laplacian` and `energy` losses of geomloss.SamplesLoss that the reference's --gtype offers beside `sinkhorn`
// (arguments/argument_kd.py:41, losses/kd_loss.py:26-30).  geomloss 0.2.4 is NOT vendored by the reference; the
// arithmetic restated here is its kernel_samples.py, tensorized path (parity unpinned
// at that boundary).  For x (N,D) with weights a and y (M,D) with weights b, the weights used as given:
//   L        = 1/2 sum_ij a_i a_j k(x_i,x_j) + 1/2 sum_ij b_i b_j k(y_i,y_j) - sum_ij a_i b_j k(x_i,y_j)
//   r2(u,v)  = sum_d (u_d - v_d)^2                                  (direct differences)
//   gaussian : k = exp(-r2 / (2 blur^2))
//   laplacian: k = exp(-sqrt(max(r2 / blur^2, 1e-8)))
//   energy   : k = -sqrt(max(r2, 1e-8))
//   dL/da_i  = sum_j a_j k(x_i,x_j) - sum_j b_j k(x_i,y_j)
//   dL/dx_i  = a_i [ sum_j a_j grad1 k(x_i,x_j) - sum_j b_j grad1 k(x_i,y_j) ]
// grad1 k = 0 where the clamp is active (torch's clamp_min rule: the gradient passes at equality), so coincident
// points -- the diagonal included -- contribute k = -1e-4 (energy) or exp(-1e-4) (laplacian) and no gradient.
//
// Two launchers.  kd6d_kernel_div_fwd_bwd is the KD step's: one workgroup per problem, 8 waves = the 8 keypoints,
// the layouts and the contract of kd6d_sinkhorn_div_fwd_bwd.  kd6d_kernel_dense_fwd_bwd is the counterpart of
// kd6d_sinkhorn_dense_fwd_bwd: one problem, D in {2,4,8,16}, one row per thread, column tiles staged in LDS, the
// pair matrices never materialised.  fp32 VALU only; every sum runs in a fixed order (no atomics).
#include <type_traits>

#include "pointset_small.h"

namespace {

using namespace pointset;
constexpr float kClamp = 1e-8f;

// k and the factor c of its gradient, grad1 k(u,v) = c * (u - v), from r2 = |u - v|^2.
template <int KIND>
__device__ __forceinline__ void pair_terms(float r2, float inv_b2, float& k, float& c) {
  if (KIND == KD6D_KERNEL_GAUSSIAN) {
    k = expf(-0.5f * r2 * inv_b2);
    c = -k * inv_b2;
  } else if (KIND == KD6D_KERNEL_LAPLACIAN) {
    const float s = r2 * inv_b2;
    if (s >= kClamp) {
      const float q = sqrtf(s);
      k = expf(-q);
      c = -k * inv_b2 / q;
    } else {
      k = expf(-1e-4f);
      c = 0.f;
    }
  } else {
    if (r2 >= kClamp) {
      const float q = sqrtf(r2);
      k = -q;
      c = -1.f / q;
    } else {
      k = -1e-4f;
      c = 0.f;
    }
  }
}

// The kernel sums feed a three-term value whose terms nearly cancel when the two measures are alike: they are
// accumulated four columns at a time with a compensated (Kahan) add, so their error stays at the rounding of the
// terms.  The gradient sums are plain: their terms carry signs already.
struct Comp {
  float s = 0.f, c = 0.f;
  __device__ __forceinline__ void add(float v) {
    const float y = v - c, t = s + y;
    c = (t - s) - y;
    s = t;
  }
};

// ---- small sets: the KD step's launch ---------------------------------------------------------------------------
struct WaveLds {
  float px[kCap], py[kCap], a[kCap];   // student points, weights
  float qx[kCap], qy[kCap], b[kCap];   // teacher points, weights
};

// sum_j w_j k(r, c_j) over the n columns in ascending order, four per chunk (three 16-byte LDS broadcasts issued
// together, like lse_row of sinkhorn.hip); with GRAD also sum_j w_j grad1 k(r, c_j).
template <int KIND, bool GRAD>
__device__ __forceinline__ float row_sweep(float rx, float ry, const float* cx, const float* cy, const float* w, int n,
                                           float inv_b2, float& gx, float& gy) {
  Comp S;
  float sx = 0.f, sy = 0.f;
  int j = 0;
  for (; j + 4 <= n; j += 4) {
    const f32x4_t X = *reinterpret_cast<const f32x4_t*>(cx + j);
    const f32x4_t Y = *reinterpret_cast<const f32x4_t*>(cy + j);
    const f32x4_t W = *reinterpret_cast<const f32x4_t*>(w + j);
    float kw[4], tx[4], ty[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float dx = rx - X[t], dy = ry - Y[t];
      float k, c;
      pair_terms<KIND>(dx * dx + dy * dy, inv_b2, k, c);
      kw[t] = W[t] * k;
      if (GRAD) { const float cw = W[t] * c; tx[t] = cw * dx; ty[t] = cw * dy; }
    }
    S.add((kw[0] + kw[1]) + (kw[2] + kw[3]));
    if (GRAD) { sx += (tx[0] + tx[1]) + (tx[2] + tx[3]); sy += (ty[0] + ty[1]) + (ty[2] + ty[3]); }
  }
  for (; j < n; ++j) {
    const float dx = rx - cx[j], dy = ry - cy[j];
    float k, c;
    pair_terms<KIND>(dx * dx + dy * dy, inv_b2, k, c);
    S.add(w[j] * k);
    if (GRAD) { const float cw = w[j] * c; sx += cw * dx; sy += cw * dy; }
  }
  if (GRAD) { gx = sx; gy = sy; }
  return S.s;
}

template <int KIND>
__global__ __launch_bounds__(64 * kWaves) void kernel_small_kernel(
    const float* __restrict__ xs, const float* __restrict__ alpha, const int* __restrict__ s_start,
    const int* __restrict__ s_cnt, const float* __restrict__ yt, const float* __restrict__ beta,
    const int* __restrict__ t_start, const int* __restrict__ t_cnt, float inv_b2, float* __restrict__ loss_img,
    int* __restrict__ valid_img, float* __restrict__ loss_kp, float* __restrict__ gx_out,
    float* __restrict__ galpha_out) {
  __shared__ __attribute__((aligned(16))) WaveLds all[kWaves];
  __shared__ float red[kWaves];

  const Segments sg = small_problem_begin(s_start, s_cnt, t_start, t_cnt, loss_img, valid_img, loss_kp);
  if (sg.skip) return;
  const int s0 = sg.s0, N = sg.N(), t0 = sg.t0, M = sg.M();
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  WaveLds& L = all[wave];
  const int k = wave;  // keypoint
  for (int i = lane; i < N; i += 64) {
    const size_t at = weight_at(s0 + i, k);
    L.px[i] = xs[point_at(at) + 0];
    L.py[i] = xs[point_at(at) + 1];
    L.a[i] = alpha[at];
  }
  for (int j = lane; j < M; j += 64) {
    const size_t at = weight_at(t0 + j, k);
    L.qx[j] = yt[point_at(at) + 0];
    L.qy[j] = yt[point_at(at) + 1];
    L.b[j] = beta[at];
  }
  __syncthreads();

  float part = 0.f;
  for (int i = lane; i < N; i += 64) {           // rows of x over the x columns, then the y columns
    const float rx = L.px[i], ry = L.py[i], a = L.a[i];
    float gxx0, gxx1, gxy0, gxy1;
    const float sxx = row_sweep<KIND, true>(rx, ry, L.px, L.py, L.a, N, inv_b2, gxx0, gxx1);
    const float sxy = row_sweep<KIND, true>(rx, ry, L.qx, L.qy, L.b, M, inv_b2, gxy0, gxy1);
    part += a * (0.5f * sxx - sxy);
    const size_t at = weight_at(s0 + i, k);
    gx_out[point_at(at) + 0] = a * (gxx0 - gxy0);
    gx_out[point_at(at) + 1] = a * (gxx1 - gxy1);
    galpha_out[at] = sxx - sxy;
  }
  for (int j = lane; j < M; j += 64) {           // third sweep: rows of y over the y columns, value only
    float g0, g1;
    const float syy = row_sweep<KIND, false>(L.qx[j], L.qy[j], L.qx, L.qy, L.b, M, inv_b2, g0, g1);
    part += 0.5f * L.b[j] * syy;
  }
  small_problem_finish(part, red, loss_img, valid_img, loss_kp);
}

// ---- dense sets: one problem, D coordinates per point -----------------------------------------------------------
constexpr int kRows = 64;     // rows per workgroup: one wave, one row per lane (16384 rows -> 256 workgroups per sweep)
constexpr int kTile = 128;    // columns per LDS tile

template <int D> struct PointVec { typedef f32x4_t type; static constexpr int W = 4; };
template <> struct PointVec<2> { typedef f32x2_t type; static constexpr int W = 2; };

// one column: returns w k(r, c) and, with GRAD, adds w grad1 k(r, c) to g
template <int KIND, int D, bool GRAD>
__device__ __forceinline__ float dense_col(const float (&xr)[D], const float* cp, float w, float inv_b2, float (&g)[D]) {
  typedef typename PointVec<D>::type vec_t;
  constexpr int VW = PointVec<D>::W;
  float diff[D];
  float r2 = 0.f;
#pragma unroll
  for (int v = 0; v < D / VW; ++v) {
    const vec_t C = *reinterpret_cast<const vec_t*>(cp + v * VW);
#pragma unroll
    for (int t = 0; t < VW; ++t) {
      diff[v * VW + t] = xr[v * VW + t] - C[t];
      r2 += diff[v * VW + t] * diff[v * VW + t];
    }
  }
  float k, c;
  pair_terms<KIND>(r2, inv_b2, k, c);
  if (GRAD) {
    const float cw = w * c;
#pragma unroll
    for (int d = 0; d < D; ++d) g[d] += cw * diff[d];
  }
  return w * k;
}

// sum_j sign w_j k(r, p_j) over the n points of one set, ascending, through LDS tiles shared by the workgroup
template <int KIND, int D, bool GRAD>
__device__ __forceinline__ float dense_sweep(const float (&xr)[D], const float* __restrict__ pts,
                                             const float* __restrict__ wts, int n, float sign, float inv_b2,
                                             float* tile_p, float* tile_w, float (&g)[D]) {
  Comp S;
  for (int c0 = 0; c0 < n; c0 += kTile) {
    const int cnt = min(kTile, n - c0);
    __syncthreads();                               // the previous tile has been read by every row
    for (int e = threadIdx.x; e < cnt * D; e += kRows) tile_p[e] = pts[(size_t)c0 * D + e];
    for (int e = threadIdx.x; e < cnt; e += kRows) tile_w[e] = sign * wts[c0 + e];
    __syncthreads();
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {
      const float k0 = dense_col<KIND, D, GRAD>(xr, tile_p + (j + 0) * D, tile_w[j + 0], inv_b2, g);
      const float k1 = dense_col<KIND, D, GRAD>(xr, tile_p + (j + 1) * D, tile_w[j + 1], inv_b2, g);
      const float k2 = dense_col<KIND, D, GRAD>(xr, tile_p + (j + 2) * D, tile_w[j + 2], inv_b2, g);
      const float k3 = dense_col<KIND, D, GRAD>(xr, tile_p + (j + 3) * D, tile_w[j + 3], inv_b2, g);
      S.add((k0 + k1) + (k2 + k3));
    }
    for (; j < cnt; ++j) S.add(dense_col<KIND, D, GRAD>(xr, tile_p + j * D, tile_w[j], inv_b2, g));
  }
  return S.s;
}

// workgroups [0, nbx): rows of x over the [x | y] columns (value + gradients); [nbx, nbx + nby): rows of y over the y
// columns (value only).  partials[workgroup] = the workgroup's share of L.
template <int KIND, int D>
__global__ __launch_bounds__(kRows) void kernel_dense_kernel(const float* __restrict__ x, const float* __restrict__ alpha,
                                                             const float* __restrict__ y, const float* __restrict__ beta,
                                                             int N, int M, int nbx, float inv_b2,
                                                             float* __restrict__ partials, float* __restrict__ grad_x,
                                                             float* __restrict__ grad_alpha) {
  __shared__ __attribute__((aligned(16))) float tile_p[kTile * D];
  __shared__ float tile_w[kTile];
  const bool on_x = (int)blockIdx.x < nbx;
  const int rows = on_x ? N : M;
  const float* base = on_x ? x : y;
  const float* wrow = on_x ? alpha : beta;
  const int r = (on_x ? (int)blockIdx.x : (int)blockIdx.x - nbx) * kRows + (int)threadIdx.x;
  const bool act = r < rows;
  float xr[D], g[D];
#pragma unroll
  for (int d = 0; d < D; ++d) { xr[d] = act ? base[(size_t)r * D + d] : 0.f; g[d] = 0.f; }
  const float wr = act ? wrow[r] : 0.f;
  float part = 0.f;
  if (on_x) {
    const float sxx = dense_sweep<KIND, D, true>(xr, x, alpha, N, 1.f, inv_b2, tile_p, tile_w, g);
    const float nsxy = dense_sweep<KIND, D, true>(xr, y, beta, M, -1.f, inv_b2, tile_p, tile_w, g);   // = -S_xy
    if (act) {
      part = wr * (0.5f * sxx + nsxy);
      grad_alpha[r] = sxx + nsxy;
#pragma unroll
      for (int d = 0; d < D; ++d) grad_x[(size_t)r * D + d] = wr * g[d];
    }
  } else {
    const float syy = dense_sweep<KIND, D, false>(xr, y, beta, M, 1.f, inv_b2, tile_p, tile_w, g);
    if (act) part = 0.5f * wr * syy;
  }
  part = wave_sum(part);
  if (threadIdx.x == 0) partials[blockIdx.x] = part;
}

// the partials in index order
__global__ void kernel_dense_sum_kernel(const float* __restrict__ partials, int n, float* __restrict__ loss) {
  if (threadIdx.x == 0) {
    Comp S;
    for (int i = 0; i < n; ++i) S.add(partials[i]);
    loss[0] = S.s;
  }
}

// f(std::integral_constant<int, KIND>) for the KD6D_KERNEL_* code `kind`; f(std::integral_constant<int, D>) for D
template <int V> using Const = std::integral_constant<int, V>;
template <class F>
void dispatch_kind(int kind, F f) {
  if (kind == KD6D_KERNEL_GAUSSIAN) f(Const<KD6D_KERNEL_GAUSSIAN>{});
  else if (kind == KD6D_KERNEL_LAPLACIAN) f(Const<KD6D_KERNEL_LAPLACIAN>{});
  else f(Const<KD6D_KERNEL_ENERGY>{});
}
template <class F>
void dispatch_dim(int D, F f) {
  if (D == 2) f(Const<2>{}); else if (D == 4) f(Const<4>{}); else if (D == 8) f(Const<8>{}); else f(Const<16>{});
}

// 1 / blur^2 in double like the reference's python floats; the energy distance has no blur
inline float inv_blur2(int kind, float blur) {
  return kind == KD6D_KERNEL_ENERGY ? 1.f : (float)(1.0 / ((double)blur * (double)blur));
}

}  // namespace

extern "C" int kd6d_kernel_div_fwd_bwd(int kind, const float* xs, const float* alpha, const int32_t* s_start,
                                       const int32_t* s_cnt, const float* yt, const float* beta, const int32_t* t_start,
                                       const int32_t* t_cnt, int n_images, float blur, float* loss_img,
                                       int32_t* valid_img, float* loss_kp, float* grad_xs, float* grad_alpha,
                                       void* stream) {
  if (const int rc = check_small_set_pointers("kd6d_kernel_div_fwd_bwd", xs, alpha, s_start, s_cnt, yt, beta, t_start,
                                              t_cnt, loss_img, valid_img, grad_xs, grad_alpha))
    return rc;
  KD6D_CHECK_ARG(kind >= KD6D_KERNEL_GAUSSIAN && kind <= KD6D_KERNEL_ENERGY, "kd6d_kernel_div_fwd_bwd: unknown kind=%d",
                 kind);
  KD6D_CHECK_ARG(kind == KD6D_KERNEL_ENERGY || blur > 0.f, "kd6d_kernel_div_fwd_bwd: blur=%g (need blur > 0)",
                 (double)blur);
  KD6D_CHECK_ARG(n_images >= 0, "kd6d_kernel_div_fwd_bwd: n_images=%d", n_images);
  if (n_images == 0) return KD6D_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float inv_b2 = inv_blur2(kind, blur);
  dispatch_kind(kind, [&](auto K) {
    hipLaunchKernelGGL(kernel_small_kernel<decltype(K)::value>, dim3(n_images), dim3(64 * kWaves), 0, st, xs, alpha,
                       s_start, s_cnt, yt, beta, t_start, t_cnt, inv_b2, loss_img, valid_img, loss_kp, grad_xs, grad_alpha);
  });
  KD6D_CHECK_LAUNCH("kd6d_kernel_div_fwd_bwd");
  return KD6D_OK;
}

extern "C" int kd6d_kernel_div_max_points(void) { return kCap; }

extern "C" int64_t kd6d_kernel_dense_workspace_floats(int N, int M, int D) {
  (void)D;
  if (N < 1 || M < 1) return 0;
  return (int64_t)cdiv(N, kRows) + cdiv(M, kRows);
}

extern "C" int kd6d_kernel_dense_fwd_bwd(int kind, const float* x, const float* alpha, const float* y, const float* beta,
                                         int N, int M, int D, float blur, float* workspace, int64_t workspace_floats,
                                         float* loss, float* grad_x, float* grad_alpha, void* stream) {
  KD6D_CHECK_ARG(x && alpha && y && beta && workspace && loss && grad_x && grad_alpha,
                 "kd6d_kernel_dense_fwd_bwd: null pointer");
  KD6D_CHECK_ARG(kind >= KD6D_KERNEL_GAUSSIAN && kind <= KD6D_KERNEL_ENERGY, "kd6d_kernel_dense_fwd_bwd: unknown kind=%d",
                 kind);
  KD6D_CHECK_ARG(kind == KD6D_KERNEL_ENERGY || blur > 0.f, "kd6d_kernel_dense_fwd_bwd: blur=%g (need blur > 0)",
                 (double)blur);
  KD6D_CHECK_ARG(N >= 1 && M >= 1, "kd6d_kernel_dense_fwd_bwd: N=%d M=%d (need at least one point per set)", N, M);
  KD6D_CHECK_ARG(D == 2 || D == 4 || D == 8 || D == 16, "kd6d_kernel_dense_fwd_bwd: D=%d (need 2, 4, 8 or 16)", D);
  const int64_t need = kd6d_kernel_dense_workspace_floats(N, M, D);
  KD6D_CHECK_ARG(workspace_floats >= need, "kd6d_kernel_dense_fwd_bwd: workspace_floats=%lld < %lld",
                 (long long)workspace_floats, (long long)need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float inv_b2 = inv_blur2(kind, blur);
  const int nbx = cdiv(N, kRows), nby = cdiv(M, kRows);
  dispatch_kind(kind, [&](auto K) {
    dispatch_dim(D, [&](auto Dc) {
      hipLaunchKernelGGL((kernel_dense_kernel<decltype(K)::value, decltype(Dc)::value>), dim3(nbx + nby), dim3(kRows), 0,
                         st, x, alpha, y, beta, N, M, nbx, inv_b2, workspace, grad_x, grad_alpha);
    });
  });
  KD6D_CHECK_LAUNCH("kd6d_kernel_dense_fwd_bwd");
  hipLaunchKernelGGL(kernel_dense_sum_kernel, dim3(1), dim3(64), 0, st, workspace, (int)need, loss);
  KD6D_CHECK_LAUNCH("kd6d_kernel_dense_fwd_bwd");
  return KD6D_OK;
}
