// The frame of a small-set launch: what kd6d_sinkhorn_div_fwd_bwd (sinkhorn.hip) and kd6d_kernel_div_fwd_bwd
// (kernel_loss.hip) have in common, written once ("The small-set launch contract").
//   * one workgroup of kWaves waves per problem, wave k = keypoint k; at most kCap points per set;
//   * points (rows, 8, 2) and weights (rows, 8); problem b owns student rows [s_start[b], s_start[b] + s_cnt[b]) and
//     teacher rows [t_start[b], t_start[b] + t_cnt[b]);
//   * a problem with an empty set is skipped (valid_img = 0), one with more than kCap points in a set refused
//     (valid_img = -1): loss_img = 0, its loss_kp row zeroed, its gradient rows NOT written;
//   * otherwise valid_img = 1, loss_kp[b][k] = wave k's value, loss_img[b] = their fp32 sum in wave order.
#pragma once
#include "kd6d_common.h"

namespace pointset {

constexpr int kCap = 128;     // max points per set per problem (kd6d_sinkhorn_max_points() = kd6d_kernel_div_max_points())
constexpr int kWaves = 8;     // keypoints per problem

// index of the weight of point `row`, keypoint k, in a (rows, 8) array; of that point's x in a (rows, 8, 2) array (+ 1: y)
__device__ __forceinline__ size_t weight_at(int row, int k) { return (size_t)row * 8 + k; }
__device__ __forceinline__ size_t point_at(size_t weight_index) { return weight_index * 2; }

struct Segments {
  int s0, n, t0, m;
  bool skip;
  // the sizes of a problem that is not skipped: 1 <= N, M <= kCap, said to the compiler (it sizes the row loops by it)
  __device__ __forceinline__ int N() const { __builtin_assume(n > 0); __builtin_assume(n <= kCap); return n; }
  __device__ __forceinline__ int M() const { __builtin_assume(m > 0); __builtin_assume(m <= kCap); return m; }
};

// The segments of problem blockIdx.x.  skip: the problem is empty or oversize, its outputs have been written as above
// and the workgroup must return.
__device__ __forceinline__ Segments small_problem_begin(const int* __restrict__ s_start, const int* __restrict__ s_cnt,
                                                        const int* __restrict__ t_start, const int* __restrict__ t_cnt,
                                                        float* __restrict__ loss_img, int* __restrict__ valid_img,
                                                        float* __restrict__ loss_kp) {
  const int b = blockIdx.x;
  const int s0 = s_start[b], N = s_cnt[b];
  const int t0 = t_start[b], M = t_cnt[b];
  const bool skip = N <= 0 || M <= 0 || N > kCap || M > kCap;
  if (skip) {                                  // empty: the reference skips such an image (loss_libs.py:25-28)
    if (threadIdx.x == 0) { loss_img[b] = 0.f; valid_img[b] = (N <= 0 || M <= 0) ? 0 : -1; }
    if (loss_kp && threadIdx.x < kWaves) loss_kp[b * kWaves + threadIdx.x] = 0.f;
  }
  return {s0, N, t0, M, skip};
}

// part: this lane's share of its wave's (keypoint's) value.  red: kWaves floats of LDS, red_stride apart.
__device__ __forceinline__ void small_problem_finish(float part, float* red, float* __restrict__ loss_img,
                                                     int* __restrict__ valid_img, float* __restrict__ loss_kp,
                                                     int red_stride = 1) {
  const int b = blockIdx.x, wave = threadIdx.x >> 6;
  part = wave_sum(part);
  if ((threadIdx.x & 63) == 0) { red[wave * red_stride] = part; if (loss_kp) loss_kp[b * kWaves + wave] = part; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int w = 0; w < kWaves; ++w) tot += red[w * red_stride];
    loss_img[b] = tot;
    valid_img[b] = 1;
  }
}

// Host: the pointers every small-set entry point needs, all non-null (loss_kp is optional and not among them).
template <class... P>
inline int check_small_set_pointers(const char* entry, P... required) {
  KD6D_CHECK_ARG((... && (required != nullptr)), "%s: null pointer", entry);
  return KD6D_OK;
}

}  // namespace pointset
