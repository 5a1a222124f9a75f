// Device-resident frame cache (train_kd.py / test.py --frame_cache device; kd6d/libs/frame_cache.py): the decoded
// frames, merged instance masks and pose annotations of a whole image list stay in HBM, and a batch is assembled from
// sampler indices by two launches instead of a host decode, a host collate and a pageable upload per batch:
//   kd6d_cache_gather_frames   frames_out[b] = frames[index[b]] (bytes), masks_out[b] = float(masks[index[b]])
//   kd6d_cache_gather_targets  the small fields of a PackedTargets (kd6d/kd_losses.py), written in their packed layout
// Both are pure data movement (no arithmetic beyond uint8 -> float32, which is exact), so what kd6d_dzi_crop and the
// augmentation front-end read is byte for byte what the host loader would have uploaded.
//
// Its own translation unit: nothing here is shared with a kernel of the default path.
//
// kd6d_cache_gather_frames is bound by HBM traffic (read 4 + write 7 bytes per pixel: ~3.4 MB per 480x640 frame).
// Lanes move 16-byte granules.  A frame's byte size need not be a multiple of 16 (and the cache and the batch place
// frame k at k * frame_bytes), so per (source, destination) pair the kernel picks the widest granule BOTH addresses
// can be aligned to -- 16, 4 or 1 byte(s) -- copies the head up to the destination's first aligned granule and the
// tail behind the last one bytewise, and only ever issues naturally aligned accesses inside [base, base + size).
#include "kd6d_common.h"

namespace {

// d[0, nbytes) = ok ? s[0, nbytes) : 0, V-wide where (s - d) is a multiple of sizeof(V) (the caller's choice of V).
template <typename V>
__device__ __forceinline__ void copy_span(const unsigned char* __restrict__ s, unsigned char* __restrict__ d,
                                          size_t nbytes, bool ok, size_t tid, size_t nthreads) {
  size_t head = (size_t)(0 - reinterpret_cast<uintptr_t>(d)) & (sizeof(V) - 1);
  if (head > nbytes) head = nbytes;
  const size_t nv = (nbytes - head) / sizeof(V);
  const size_t tail0 = head + nv * sizeof(V);
  for (size_t i = tid; i < head; i += nthreads) d[i] = ok ? s[i] : (unsigned char)0;
  V* dv = reinterpret_cast<V*>(d + head);
  if (ok) {
    const V* sv = reinterpret_cast<const V*>(s + head);
    for (size_t i = tid; i < nv; i += nthreads) dv[i] = sv[i];
  } else {
    V z;
    memset(&z, 0, sizeof(V));
    for (size_t i = tid; i < nv; i += nthreads) dv[i] = z;
  }
  for (size_t i = tail0 + tid; i < nbytes; i += nthreads) d[i] = ok ? s[i] : (unsigned char)0;
}

// d[0, n) = ok ? float(s[0, n)) : 0.  d is 4-byte aligned; the body stores one 16-byte granule (4 floats) per lane from
// 4 source bytes, read as one word where the source is word aligned at that point and bytewise otherwise.
__device__ __forceinline__ void widen_span(const unsigned char* __restrict__ s, float* __restrict__ d, size_t n, bool ok,
                                           size_t tid, size_t nthreads) {
  size_t head = ((size_t)(0 - reinterpret_cast<uintptr_t>(d)) & 15) >> 2;
  if (head > n) head = n;
  const size_t ng = (n - head) / 4;
  const size_t tail0 = head + ng * 4;
  for (size_t i = tid; i < head; i += nthreads) d[i] = ok ? (float)s[i] : 0.f;
  f32x4_t* dv = reinterpret_cast<f32x4_t*>(d + head);
  if (!ok) {
    const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
    for (size_t g = tid; g < ng; g += nthreads) dv[g] = z;
  } else if ((reinterpret_cast<uintptr_t>(s + head) & 3) == 0) {
    const unsigned* sw = reinterpret_cast<const unsigned*>(s + head);
    for (size_t g = tid; g < ng; g += nthreads) {
      const unsigned w = sw[g];
      const f32x4_t v = {(float)(w & 255u), (float)((w >> 8) & 255u), (float)((w >> 16) & 255u), (float)(w >> 24)};
      dv[g] = v;
    }
  } else {
    const unsigned char* sb = s + head;
    for (size_t g = tid; g < ng; g += nthreads) {
      const f32x4_t v = {(float)sb[g * 4 + 0], (float)sb[g * 4 + 1], (float)sb[g * 4 + 2], (float)sb[g * 4 + 3]};
      dv[g] = v;
    }
  }
  for (size_t i = tail0 + tid; i < n; i += nthreads) d[i] = ok ? (float)s[i] : 0.f;
}

__global__ __launch_bounds__(256) void cache_gather_frames_kernel(
    const unsigned char* __restrict__ frames, const unsigned char* __restrict__ masks, int n, size_t npix,
    const int* __restrict__ index, unsigned char* __restrict__ frames_out, float* __restrict__ masks_out) {
  const int b = blockIdx.y;
  const int idx = index[b];
  const bool ok = idx >= 0 && idx < n;          // an index outside the cache is never dereferenced: the entry is zero-filled
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
  const size_t fbytes = npix * 3;
  unsigned char* fd = frames_out + (size_t)b * fbytes;
  const unsigned char* fs = ok ? frames + (size_t)idx * fbytes : fd;
  const unsigned delta = (unsigned)(reinterpret_cast<uintptr_t>(fs) ^ reinterpret_cast<uintptr_t>(fd));
  // (equal low bits <=> the difference of the two addresses is a multiple of the granule)
  if ((delta & 15u) == 0)
    copy_span<u32x4_t>(fs, fd, fbytes, ok, tid, nthreads);
  else if ((delta & 3u) == 0)
    copy_span<unsigned>(fs, fd, fbytes, ok, tid, nthreads);
  else
    copy_span<unsigned char>(fs, fd, fbytes, ok, tid, nthreads);
  widen_span(ok ? masks + (size_t)idx * npix : nullptr, masks_out + (size_t)b * npix, npix, ok, tid, nthreads);
}

__device__ __forceinline__ int pad4(int v) { return (v + 3) / 4 * 4; }

// One workgroup per batch entry; workgroup 0 also zeroes the padding behind each field.
__global__ __launch_bounds__(256) void cache_gather_targets_kernel(
    const float* __restrict__ table_f, const int* __restrict__ table_i, const float* __restrict__ kp3d, int kp_elems,
    int n, const int* __restrict__ index, int B, const float* __restrict__ bbox_trans, float* __restrict__ flat_f,
    int* __restrict__ flat_i) {
  constexpr int G = KD6D_MAX_GT, ROW_F = KD6D_CACHE_ROW_F, ROW_I = KD6D_CACHE_ROW_I;
  const int b = blockIdx.x, t = threadIdx.x;
  const int idx = index[b];
  const bool ok = idx >= 0 && idx < n;
  const float* rf = ok ? table_f + (size_t)idx * ROW_F : nullptr;     // {K 9, rot G*9, trans G*3}
  const int* ri = ok ? table_i + (size_t)idx * ROW_I : nullptr;       // {n_gt, class_ids G}
  const int o_K = pad4(B * kp_elems), o_bt = o_K + pad4(B * 9), o_rot = o_bt + pad4(B * 6);
  const int o_tr = o_rot + pad4(B * G * 9);
  for (int i = t; i < kp_elems; i += 256) flat_f[(size_t)b * kp_elems + i] = kp3d[i];
  if (t < 9) flat_f[o_K + b * 9 + t] = ok ? rf[t] : 0.f;
  if (t < 6) flat_f[o_bt + b * 6 + t] = bbox_trans[b * 6 + t];
  if (t < G * 9) flat_f[o_rot + b * G * 9 + t] = ok ? rf[9 + t] : 0.f;
  if (t < G * 3) flat_f[o_tr + b * G * 3 + t] = ok ? rf[9 + G * 9 + t] : 0.f;
  const int o_ng = pad4(B * G);
  if (t < G) flat_i[b * G + t] = ok ? ri[1 + t] : 0;
  if (t == 0) flat_i[o_ng + b] = ok ? ri[0] : 0;
  if (b == 0 && t < 4) {
    // the (at most 3) padding elements behind each field; kp3d has none (kp_elems is a multiple of 4)
    if (B * 9 + t < pad4(B * 9)) flat_f[o_K + B * 9 + t] = 0.f;
    if (B * 6 + t < pad4(B * 6)) flat_f[o_bt + B * 6 + t] = 0.f;
    if (B * G * 9 + t < pad4(B * G * 9)) flat_f[o_rot + B * G * 9 + t] = 0.f;
    if (B * G * 3 + t < pad4(B * G * 3)) flat_f[o_tr + B * G * 3 + t] = 0.f;
    if (B * G + t < pad4(B * G)) flat_i[B * G + t] = 0;
    if (B + t < pad4(B)) flat_i[o_ng + B + t] = 0;
  }
}

}  // namespace

extern "C" int kd6d_cache_gather_frames(const uint8_t* frames_u8, const uint8_t* masks_u8, int n, int H, int W,
                                        const int32_t* index_dev, int B, uint8_t* frames_out_u8, float* masks_out_f32,
                                        void* stream) {
  KD6D_CHECK_ARG(frames_u8 && masks_u8 && index_dev && frames_out_u8 && masks_out_f32,
                 "kd6d_cache_gather_frames: null pointer");
  KD6D_CHECK_ARG(n > 0 && B > 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384 && B <= 65535,
                 "kd6d_cache_gather_frames: bad sizes n=%d B=%d H=%d W=%d", n, B, H, W);
  KD6D_CHECK_ARG((reinterpret_cast<uintptr_t>(masks_out_f32) & 3) == 0,
                 "kd6d_cache_gather_frames: masks_out_f32 is not 4-byte aligned");
  const size_t npix = (size_t)H * (size_t)W;
  // 16 bytes per lane and a few granules per lane: 64 workgroups per frame saturate HBM from B = 4 up
  int nb = cdiv((long long)npix * 3, 256 * 16 * 4);
  if (nb > 64) nb = 64;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(cache_gather_frames_kernel, dim3(nb, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     frames_u8, masks_u8, n, npix, index_dev, frames_out_u8, masks_out_f32);
  KD6D_CHECK_LAUNCH("kd6d_cache_gather_frames");
  return KD6D_OK;
}

extern "C" int kd6d_cache_gather_targets(const float* table_f, const int32_t* table_i, const float* kp3d, int kp_elems,
                                         int n, const int32_t* index_dev, int B, const float* bbox_trans,
                                         float* flat_f_out, int32_t* flat_i_out, void* stream) {
  KD6D_CHECK_ARG(table_f && table_i && kp3d && index_dev && bbox_trans && flat_f_out && flat_i_out,
                 "kd6d_cache_gather_targets: null pointer");
  KD6D_CHECK_ARG(n > 0 && B > 0 && B <= 65535 && kp_elems > 0 && kp_elems % 4 == 0 &&
                     (long long)B * kp_elems <= (1ll << 28),
                 "kd6d_cache_gather_targets: bad sizes n=%d B=%d kp_elems=%d", n, B, kp_elems);
  hipLaunchKernelGGL(cache_gather_targets_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), table_f,
                     table_i, kp3d, kp_elems, n, index_dev, B, bbox_trans, flat_f_out, flat_i_out);
  KD6D_CHECK_LAUNCH("kd6d_cache_gather_targets");
  return KD6D_OK;
}
