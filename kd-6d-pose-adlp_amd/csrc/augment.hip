// Train-time augmentation of full uint8 frames on the GPU: the reference's train transform chain
// (libs/train_libs.py:212-238) and its post-transform clean-up (dataset.py:166-176), the stage right
// upstream of the DZI crop (dzi.hip).  kd6d/libs/augment.py draws every scalar parameter on the host
// and runs the launches below in this order:
//
//   kd6d_aug_warp_u8      Resize (M = INTERNAL_K K^-1) and RandomShiftScaleRotate: cv2.warpAffine,
//                         8-bit INTER_LINEAR (border 128) on the frame, INTER_NEAREST (border 0) on the mask
//   kd6d_aug_mask_stats   per image and instance id: area + visible box (to_visible_boxlist / remove_invalids)
//   kd6d_aug_occlude      RandomOcclusion: rectangles from the visible boxes and five host uniforms per slot,
//                         random bytes into the frame, -1 into the mask
//   kd6d_aug_background   RandomBackground (--aug_chain full): mask == 0 pixels take cv2.resize(back, frame size),
//                         8-bit INTER_LINEAR gathered from a pool of backgrounds at their native sizes (in place)
//   kd6d_aug_warp_u8      (RandomShiftScaleRotate, as above)
//   kd6d_aug_hsv          RandomHSV: cv2 8-bit BGR->HSV, float32 scale, truncating store, HSV->BGR (in place)
//   kd6d_aug_sharpen      RandomPencilSharpen (--aug_chain full): box blur on LDS tiles, edge image, two whole-image
//                         min-max normalisations (init + three launches)
//   kd6d_aug_filter       RandomSmooth (cv2.blur, BORDER_REFLECT_101) + RandomNoise + Grayscalize, fused
//   kd6d_aug_relabel      remove_invalids: per-image id lookup table on the mask
//
// The reference chain's eight pixel stages are all here.  One thread per output pixel, all three channels, except in
// kd6d_aug_sharpen (one thread per value, LDS tiles).  The others are HBM / latency bound: plain loads and
// stores, no LDS tiling, no matrix pipe.  Per-pixel randomness (occlusion bytes, Gaussian noise) is a
// counter-based hash of (key, image, pixel, channel): order-free, so the result does not depend on the
// launch shape.  The arithmetic restates OpenCV's documented 8-bit fixed-point scheme (parity unpinned: no
// OpenCV on this project's machines; tests/augment_ref.py holds the same arithmetic in numpy and the GPU tests
// hold the two bit-equal).
#include <math.h>

#include "kd6d_common.h"

namespace {

constexpr int AB_BITS = 10, INTER_BITS = 5;
constexpr int AB_SCALE = 1 << AB_BITS, INTER_TAB = 1 << INTER_BITS;
constexpr int COEF_BITS = 15;                 // INTER_REMAP_COEF_BITS
constexpr int AUG_MAX_ID = KD6D_AUG_MAX_ID;

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// 64 random bits for (key, stream tag, image, pixel, draw); byte c of the occlusion draw is channel c's fill byte
__device__ __forceinline__ unsigned long long pixel_hash(unsigned long long key, unsigned tag, int b, long long pix,
                                                         unsigned draw) {
  const unsigned long long ctr = ((unsigned long long)tag << 60) ^ ((unsigned long long)draw << 56) ^
                                 ((unsigned long long)(unsigned)b << 36) ^ (unsigned long long)pix;
  return splitmix64(key ^ splitmix64(ctr));
}

// ------------------------------------------------------------------------------------------------------------------
// warpAffine, 8-bit bilinear + float nearest.  cv2 inverts the forward matrix in double, steps the source coordinate
// in 1/1024 px (rounded half to even), rounds it to 1/32 px and takes the four taps' 15-bit weights from the
// 32 x 32 table of initInterTab2D: w = (32 - fy, fy) x (32 - fx, fx) * 32 exactly, except entry (0, 0) where 1.0 * 32768
// saturates to 32767 and the adjustment moves the missing unit to the last tap: {32767, 0, 0, 1}.  Out-of-frame taps
// read the border value 128; the sum is rounded (+2^14) >> 15 and saturated.
__global__ __launch_bounds__(256) void warp_u8_kernel(const unsigned char* __restrict__ src,
                                                      const float* __restrict__ src_mask, int H, int W,
                                                      const double* __restrict__ fwd, int Ho, int Wo,
                                                      unsigned char* __restrict__ dst, float* __restrict__ dst_mask) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const double* M = fwd + (size_t)b * 6;
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0.0 ? 1.0 / D : 0.0;
  const double m00 = M[4] * D, m01 = M[1] * -D, m10 = M[3] * -D, m11 = M[0] * D;
  const double b1 = -m00 * M[2] - m01 * M[5];
  const double b2 = -m10 * M[2] - m11 * M[5];
  const unsigned char* fr = src + (size_t)b * H * W * 3;
  const float* mk = src_mask ? src_mask + (size_t)b * H * W : nullptr;
  const long long npix = (long long)Ho * Wo;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
    const int y = (int)(p / Wo), x = (int)(p - (long long)y * Wo);
    const long long ad = (long long)rint(m00 * (double)x * AB_SCALE);
    const long long bd = (long long)rint(m10 * (double)x * AB_SCALE);
    const long long X0 = (long long)rint((m01 * (double)y + b1) * AB_SCALE);
    const long long Y0 = (long long)rint((m11 * (double)y + b2) * AB_SCALE);
    {
      const int rd = AB_SCALE / INTER_TAB / 2;
      const long long X = (X0 + rd + ad) >> (AB_BITS - INTER_BITS), Y = (Y0 + rd + bd) >> (AB_BITS - INTER_BITS);
      const long long sx = X >> INTER_BITS, sy = Y >> INTER_BITS;
      const int fx = (int)(X & (INTER_TAB - 1)), fy = (int)(Y & (INTER_TAB - 1));
      int w[4] = {(INTER_TAB - fy) * (INTER_TAB - fx) * 32, (INTER_TAB - fy) * fx * 32, fy * (INTER_TAB - fx) * 32,
                  fy * fx * 32};
      if (fx == 0 && fy == 0) { w[0] = 32767; w[3] = 1; }
      int acc[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long yy = sy + (k >> 1), xx = sx + (k & 1);
        int px[3] = {128, 128, 128};
        if (xx >= 0 && xx < W && yy >= 0 && yy < H) {
          const unsigned char* q = fr + ((size_t)yy * W + (size_t)xx) * 3;
          px[0] = q[0]; px[1] = q[1]; px[2] = q[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += px[c] * w[k];
      }
      unsigned char* o = dst + ((size_t)b * npix + (size_t)p) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int v = (acc[c] + (1 << (COEF_BITS - 1))) >> COEF_BITS;
        o[c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
      }
    }
    if (mk) {
      const int rd = AB_SCALE / 2;
      const long long X = (X0 + rd + ad) >> AB_BITS, Y = (Y0 + rd + bd) >> AB_BITS;
      float v = 0.f;
      if (X >= 0 && X < W && Y >= 0 && Y < H) v = mk[(size_t)Y * W + (size_t)X];
      dst_mask[(size_t)b * npix + p] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Per (image, id in 1..max_id): {area, xmin, ymin, xmax, ymax} of the pixels whose mask value is exactly id.
// Workgroup partials in LDS (integer atomics), then one global integer atomic per workgroup and field: the result
// does not depend on the order.  Encoded while accumulating so that every field starts at 0 (hipMemsetAsync) and
// merges with add / max: {area, W - xmin, H - ymin, xmax + 1, ymax + 1}; mask_stats_finish_kernel decodes.
constexpr int STATS_PIX_PER_THREAD = 16;

__global__ __launch_bounds__(256) void mask_stats_kernel(const float* __restrict__ masks, int H, int W, int max_id,
                                                         int* __restrict__ stats) {
  __shared__ int s[AUG_MAX_ID * 5];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < max_id * 5; i += 256) s[i] = 0;
  __syncthreads();
  const long long npix = (long long)H * W;
  const float* mk = masks + (size_t)b * npix;
  const long long p0 = (long long)blockIdx.x * 256 * STATS_PIX_PER_THREAD;
  for (int k = 0; k < STATS_PIX_PER_THREAD; ++k) {
    const long long p = p0 + (long long)k * 256 + threadIdx.x;
    if (p >= npix) break;
    const float v = mk[p];
    const int id = (int)v;
    if (!(v == (float)id && id >= 1 && id <= max_id)) continue;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    int* e = s + (id - 1) * 5;
    __hip_atomic_fetch_add(e + 0, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // integer: order-free
    atomicMax(e + 1, W - x);
    atomicMax(e + 2, H - y);
    atomicMax(e + 3, x + 1);
    atomicMax(e + 4, y + 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < max_id * 5; i += 256) {
    const int v = s[i];
    if (v == 0) continue;
    int* g = stats + (size_t)b * max_id * 5 + i;
    if (i % 5 == 0) __hip_atomic_fetch_add(g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else atomicMax(g, v);
  }
}

__global__ void mask_stats_finish_kernel(int B, int H, int W, int max_id, int* __restrict__ stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * max_id) return;
  int* e = stats + (size_t)i * 5;
  if (e[0] == 0) {
    e[1] = e[2] = e[3] = e[4] = 0;          // to_visible_boxlist: [0, 0, 0, 0] for an instance without pixels
  } else {
    e[1] = W - e[1]; e[2] = H - e[2]; e[3] = e[3] - 1; e[4] = e[4] - 1;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// RandomOcclusion (transform.py:257-290) with the host's uniforms u[0..4] per instance slot standing in for
// random.uniform(0, 1), (0.02, 0.7), (0.5, 2.0), (x1, x2), (y1, y2): a + (b - a) * u, random.uniform's own formula.
struct Rect {
  int x0, y0, x1, y1;   // [x0, x1) x [y0, y1); empty when x0 >= x1 or y0 >= y1
};

__device__ double clip_d(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ Rect occlusion_rect(const int* st, const double* u, double prob, int H, int W) {
#pragma clang fp contract(off)
  Rect r = {0, 0, 0, 0};
  const int x1 = st[1], y1 = st[2], x2 = st[3], y2 = st[4];   // int(float(v)) of integer coordinates
  const int bw = x2 - x1, bh = y2 - y1;
  if (!(0.0 + (1.0 - 0.0) * u[0] <= prob && bw > 2 && bh > 2)) return r;
  const double bb_size = (double)(bw * bh);
  const double size = (0.02 + (0.7 - 0.02) * u[1]) * bb_size;
  const double ratio = 0.5 + (2.0 - 0.5) * u[2];
  const int ew = (int)sqrt(size * ratio);
  const int eh = (int)sqrt(size / ratio);
  const double ecx = (double)x1 + (double)(x2 - x1) * u[3];
  const double ecy = (double)y1 + (double)(y2 - y1) * u[4];
  r.x0 = (int)clip_d(ecx - (double)ew / 2 + 0.5, 0.0, (double)(W - 1));
  r.y0 = (int)clip_d(ecy - (double)eh / 2 + 0.5, 0.0, (double)(H - 1));
  r.x1 = (int)clip_d(ecx + (double)ew / 2 + 0.5, 0.0, (double)(W - 1));
  r.y1 = (int)clip_d(ecy + (double)eh / 2 + 0.5, 0.0, (double)(H - 1));
  return r;
}

__global__ __launch_bounds__(256) void occlude_kernel(unsigned char* __restrict__ frames, float* __restrict__ masks,
                                                      int H, int W, const int* __restrict__ stats, int stats_ids,
                                                      const double* __restrict__ uniforms,
                                                      const int* __restrict__ n_inst, double prob,
                                                      unsigned long long key) {
  __shared__ Rect s_r[KD6D_MAX_GT];
  const int b = blockIdx.y;
  const int n = min(n_inst[b], KD6D_MAX_GT);
  if (threadIdx.x < KD6D_MAX_GT) {
    Rect r = {0, 0, 0, 0};
    if ((int)threadIdx.x < n)
      r = occlusion_rect(stats + ((size_t)b * stats_ids + threadIdx.x) * 5,
                         uniforms + ((size_t)b * KD6D_MAX_GT + threadIdx.x) * 5, prob, H, W);
    s_r[threadIdx.x] = r;
  }
  __syncthreads();
  bool any = false;
  for (int i = 0; i < n; ++i) any |= s_r[i].x0 < s_r[i].x1 && s_r[i].y0 < s_r[i].y1;
  if (!any) return;
  const long long npix = (long long)H * W;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    bool hit = false;
    for (int i = 0; i < n; ++i) hit |= x >= s_r[i].x0 && x < s_r[i].x1 && y >= s_r[i].y0 && y < s_r[i].y1;
    if (!hit) continue;
    const unsigned long long h = pixel_hash(key, 1u, b, p, 0u);
    unsigned char* o = frames + ((size_t)b * npix + (size_t)p) * 3;
    o[0] = (unsigned char)(h & 255); o[1] = (unsigned char)((h >> 8) & 255); o[2] = (unsigned char)((h >> 16) & 255);
    masks[(size_t)b * npix + p] = -1.f;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// RandomHSV (utils.py:181-195).  BGR -> HSV is cv2's 8-bit integer path (RGB2HSV_b, hsv_shift 12, hue range 180);
// each channel is scaled in float32, clipped at 179 / 255 only for a factor >= 1, stored with the truncating
// float -> uint8 cast of numpy; HSV -> BGR is cv2's float path on (h, s/255, v/255), then cvRound(x * 255).
__device__ __forceinline__ int cv_round_div(int num_shifted, double den) { return (int)rint((double)num_shifted / den); }

__device__ __forceinline__ unsigned char sat_round_u8(float v) {
  const float r = rintf(v);
  return (unsigned char)(r < 0.f ? 0.f : (r > 255.f ? 255.f : r));
}

__global__ __launch_bounds__(256) void hsv_kernel(unsigned char* __restrict__ frames, int H, int W,
                                                  const float* __restrict__ factors) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const float fa = factors[b * 3 + 0], fb = factors[b * 3 + 1], fc = factors[b * 3 + 2];
  const long long npix = (long long)H * W;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
    unsigned char* px = frames + ((size_t)b * npix + (size_t)p) * 3;
    const int B_ = px[0], G_ = px[1], R_ = px[2];
    // ---- BGR -> HSV, 8-bit ----
    int v = max(max(B_, G_), R_), vmin = min(min(B_, G_), R_);
    const int diff = v - vmin;
    const int vr = v == R_ ? -1 : 0, vg = v == G_ ? -1 : 0;
    const int sdiv = v ? cv_round_div(255 << 12, (double)v) : 0;
    const int hdiv = diff ? cv_round_div(180 << 12, 6.0 * diff) : 0;
    const int s = (diff * sdiv + (1 << 11)) >> 12;
    int h = (vr & (G_ - B_)) + (~vr & ((vg & (B_ - R_ + 2 * diff)) + ((~vg) & (R_ - G_ + 4 * diff))));
    h = (h * hdiv + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    // ---- scale in float32, truncating store ----
    float hf = (float)h * fa, sf = (float)s * fb, vf = (float)v * fc;
    if (!(fa < 1.f)) hf = fminf(hf, 179.f);
    if (!(fb < 1.f)) sf = fminf(sf, 255.f);
    if (!(fc < 1.f)) vf = fminf(vf, 255.f);
    const int h2 = (int)hf, s2 = (int)sf, v2 = (int)vf;   // values in [0, 255]: C cast = numpy's float -> uint8
    // ---- HSV -> BGR, float path ----
    float hh = (float)h2, ss = (float)s2 * (1.f / 255.f), vv = (float)v2 * (1.f / 255.f);
    float bo, go, ro;
    if (ss == 0.f) {
      bo = go = ro = vv;
    } else {
      hh = hh * (6.f / 180.f);
      if (hh < 0.f) { do hh += 6.f; while (hh < 0.f); }
      else if (hh >= 6.f) { do hh -= 6.f; while (hh >= 6.f); }
      int sector = (int)floorf(hh);
      hh = hh - (float)sector;
      if ((unsigned)sector >= 6u) { sector = 0; hh = 0.f; }
      float tab[4];
      tab[0] = vv;
      tab[1] = vv * (1.f - ss);
      tab[2] = vv * (1.f - ss * hh);
      tab[3] = vv * (1.f - ss * (1.f - hh));
      const int sd[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};
      bo = tab[sd[sector][0]]; go = tab[sd[sector][1]]; ro = tab[sd[sector][2]];
    }
    px[0] = sat_round_u8(bo * 255.f);
    px[1] = sat_round_u8(go * 255.f);
    px[2] = sat_round_u8(ro * 255.f);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// RandomSmooth + RandomNoise + Grayscalize, fused (they change no byte when fused: each consumes the previous
// stage's uint8 value of the SAME pixel, only the blur reads neighbours, and it reads the input buffer).
//   blur: cv2.blur (ks, ks), BORDER_REFLECT_101, cvRound(sum / ks^2) (ks^2 odd: no ties) -- ks = 1 is a copy;
//   noise: v + (sigma * n) * 255 in float32, n ~ N(0, 1) by Box-Muller from the pixel hash, clipped to [0, 255],
//          truncated (np.uint8); sigma = 0 skips it;
//   gray:  (1868 B + 9617 G + 4899 R + 8192) >> 14 into all three channels.
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

__global__ __launch_bounds__(256) void filter_kernel(const unsigned char* __restrict__ src,
                                                     unsigned char* __restrict__ dst, int H, int W,
                                                     const int* __restrict__ ksize, const float* __restrict__ sigma,
                                                     int gray, unsigned long long key) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int ks = ksize ? ksize[b] : 1, r = ks / 2;
  const float sg = sigma ? sigma[b] : 0.f;
  const long long npix = (long long)H * W;
  const unsigned char* fr = src + (size_t)b * npix * 3;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    int v[3];
    if (ks <= 1) {
      const unsigned char* q = fr + (size_t)p * 3;
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    } else {
      int sum[3] = {0, 0, 0};
      for (int dy = -r; dy <= r; ++dy) {
        const int yy = reflect101(y + dy, H);
        for (int dx = -r; dx <= r; ++dx) {
          const unsigned char* q = fr + ((size_t)yy * W + (size_t)reflect101(x + dx, W)) * 3;
          sum[0] += q[0]; sum[1] += q[1]; sum[2] += q[2];
        }
      }
      const int area = ks * ks;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (sum[c] + area / 2) / area;
    }
    if (sg > 0.f) {
      const unsigned long long h0 = pixel_hash(key, 2u, b, p, 0u), h1 = pixel_hash(key, 2u, b, p, 1u);
      const unsigned u32[4] = {(unsigned)h0, (unsigned)(h0 >> 32), (unsigned)h1, (unsigned)(h1 >> 32)};
      float n[4];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float u1 = ((float)(u32[2 * k] >> 8) + 1.f) * (1.f / 16777216.f);   // (0, 1]
        const float u2 = (float)(u32[2 * k + 1] >> 8) * (1.f / 16777216.f);        // [0, 1)
        const float rad = sqrtf(-2.f * logf(u1)), th = 6.2831853071795864f * u2;
        n[2 * k] = rad * cosf(th);
        n[2 * k + 1] = rad * sinf(th);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float f = (float)v[c] + (sg * n[c]) * 255.f;
        f = f > 255.f ? 255.f : (f < 0.f ? 0.f : f);
        v[c] = (int)f;
      }
    }
    if (gray) {
      const int g = (1868 * v[0] + 9617 * v[1] + 4899 * v[2] + 8192) >> 14;
      v[0] = v[1] = v[2] = g;
    }
    unsigned char* o = dst + ((size_t)b * npix + (size_t)p) * 3;
    o[0] = (unsigned char)v[0]; o[1] = (unsigned char)v[1]; o[2] = (unsigned char)v[2];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// remove_invalids (poses.py:172-200): mask value id in 1..max_id -> lut[b][id]; anything else (0, the occlusion's -1)
// -> 0, as the reference's fresh zero mask does.
__global__ __launch_bounds__(256) void relabel_kernel(float* __restrict__ masks, int H, int W,
                                                      const float* __restrict__ lut, int max_id) {
  const int b = blockIdx.y;
  const long long npix = (long long)H * W;
  const float* L = lut + (size_t)b * (max_id + 1);
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
    float* m = masks + (size_t)b * npix + p;
    const float v = *m;
    const int id = (int)v;
    *m = (v == (float)id && id >= 1 && id <= max_id) ? L[id] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// RandomBackground (transform.py:130-190, merge_background_mask): a pixel whose mask value is exactly 0 takes the
// pixel of cv2.resize(back, (W, H)), every other pixel keeps its byte (np.uint8(back * (1 - a) + fore * a) with a in
// {0, 1} is that selection).  The resize is computed here, per output pixel, as a four-tap gather from the ragged pool
// of backgrounds at their native sizes; no resized copy exists.  cv2's 8-bit INTER_LINEAR, restated per axis
// (d = output index, n = source extent, N = output extent):
//     f  = float32((d + 0.5) * (double(n) / double(N)) - 0.5)       (double arithmetic, rounded once to float32)
//     s  = floor(f);  f = f - float32(s)                            (float32)
//     s < 0      -> s = 0,     f = 0;      s >= n - 1 -> s = n - 1, f = 0;      taps s and min(s + 1, n - 1)
//     c0 = rint((1 - f) * 2048),  c1 = rint(f * 2048)               (float32, ties to even: the 11-bit coefficients)
// horizontal pass, per source row:   h = p[x0] * a0 + p[x1] * a1                             (int, scaled by 2^11)
// vertical pass:                     out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
// A background of the frame's size has f = 0 everywhere: (2048 * (p * 128)) >> 16 = 4 p, (4 p + 2) >> 2 = p, a copy.
// (cv2 switches an exact 2x downscale to its area path; this restatement stays bilinear at every scale.)
// Bad input is a no-op, never dereferenced: an index outside [0, n_bg) (-1 = "no background"), or a table entry
// with h, w < 1 or off + h * w * 3 > pool_bytes, leaves the image untouched.
constexpr int RESIZE_COEF_BITS = 11;
constexpr int BG_MAX_SIDE = 32768;            // keeps h * w * 3 far inside 64 bits

__device__ __forceinline__ void resize_taps(int d, double scale, int n, int* i0, int* i1, int* c0, int* c1) {
#pragma clang fp contract(off)
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f = f - (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= n - 1) { s = n - 1; f = 0.f; }
  *i0 = s;
  *i1 = s + 1 < n ? s + 1 : n - 1;
  *c0 = (int)rintf((1.f - f) * (float)(1 << RESIZE_COEF_BITS));
  *c1 = (int)rintf(f * (float)(1 << RESIZE_COEF_BITS));
}

__global__ __launch_bounds__(256) void background_kernel(unsigned char* __restrict__ frames,
                                                         const float* __restrict__ masks, int H, int W,
                                                         const unsigned char* __restrict__ pool, long long pool_bytes,
                                                         const long long* __restrict__ bg_off,
                                                         const int* __restrict__ bg_hw, int n_bg,
                                                         const int* __restrict__ bg_index) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int idx = bg_index[b];
  if (idx < 0 || idx >= n_bg) return;
  const int h = bg_hw[idx * 2], w = bg_hw[idx * 2 + 1];
  const long long off = bg_off[idx];
  if (h < 1 || w < 1 || h > BG_MAX_SIDE || w > BG_MAX_SIDE || off < 0 || off > pool_bytes ||
      (long long)h * w * 3 > pool_bytes - off)
    return;
  const unsigned char* bg = pool + off;
  const double sx = (double)w / (double)W, sy = (double)h / (double)H;
  const long long npix = (long long)H * W;
  const float* mk = masks + (size_t)b * npix;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
    if (!(mk[p] == 0.f)) continue;
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    int x0, x1, a0, a1, y0, y1, b0, b1;
    resize_taps(x, sx, w, &x0, &x1, &a0, &a1);
    resize_taps(y, sy, h, &y0, &y1, &b0, &b1);
    const unsigned char* r0 = bg + (size_t)y0 * w * 3;
    const unsigned char* r1 = bg + (size_t)y1 * w * 3;
    unsigned char* o = frames + ((size_t)b * npix + (size_t)p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int h0 = r0[x0 * 3 + c] * a0 + r0[x1 * 3 + c] * a1;
      const int h1 = r1[x0 * 3 + c] * a0 + r1[x1 * 3 + c] * a1;
      o[c] = (unsigned char)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// RandomPencilSharpen (transform.py:111-128) with the reference's dtypes, per image with ks in {5, 7, 9, 11}:
//   s    = cv2.blur(img, (ks, ks))                              filter_kernel's arithmetic (REFLECT_101, rounded mean)
//   edge = img / (float32(s) + 0.01f)   (mode != 0)             float32, IEEE division
//        = img - float32(s)             (mode == 0)
//   e    = uint8(edge * float32(scale) + float32(shift))        cv2.normalize(NORM_MINMAX, 0, 255) of a float32 image:
//          scale = 255 * (max - min > DBL_EPSILON ? 1 / (max - min) : 0),  shift = 0 - min * scale, both in double,
//          applied in float32, truncated
//   v    = img * (1 - alpha) + e * alpha                        float64
//   out  = uint8(v * scale' + shift')                           the same normalisation of v, applied in double, truncated
// ks = 0 (and any size this kernel does not take) copies the image.  The two whole-image extrema need three passes:
//   a  blur, edge, min / max of edge;      b  blur, edge, e (parked in dst), v, min / max of v;      c  out from src, e.
// Passes a and b work on SH_TH x SH_TW tiles: the tile and its reflected halo are staged once in LDS as bytes, the
// ks horizontal sums of every staged row go to a second LDS plane (uint16: at most 11 * 255), and a value's box sum is
// ks reads down that plane -- 2 ks LDS reads per value where filter_kernel issues ks^2 global byte loads.  A thread
// owns one (pixel, channel) VALUE at a time, so consecutive lanes touch consecutive bytes / uint16 of both planes: a
// 32-lane group covers at most 64 contiguous bytes (16 banks) of a row, and the plane of row sums has no padding
// between rows, so a wave that straddles two rows still reads one contiguous run -- no bank is hit twice.
// Extrema: per thread, then wave shuffles, then one LDS slot per wave, then ONE integer atomic min and max per
// workgroup on an order-preserving encoding (float32 edge: sign flip; float64 v >= 0: its bits as uint64).  min / max
// are exact in any order, so the result is a pure function of the image.
constexpr int SH_TW = 32, SH_TH = 32, SH_RMAX = 5;
constexpr int SH_RAW_PITCH = (SH_TW + 2 * SH_RMAX) * 3;      // bytes per staged row
constexpr int SH_ROW_PITCH = SH_TW * 3;                      // uint16 per row of horizontal sums

struct SharpenWs {                   // per image; kd6d_aug_sharpen_ws_bytes = sizeof * B
  unsigned emin, emax;               // encoded float32 extrema of edge
  unsigned long long vmin, vmax;     // bits of the float64 extrema of v (v >= 0)
  unsigned long long pad;
};

__device__ __forceinline__ int sharpen_ks(int ks) { return (ks >= 5 && ks <= 2 * SH_RMAX + 1 && (ks & 1)) ? ks : 0; }

__device__ __forceinline__ unsigned enc_f32(float f) {
  const unsigned u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float dec_f32(unsigned e) {
  return __uint_as_float(e ^ ((e >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// cv2.normalize(NORM_MINMAX, alpha = 0, beta = 255): scale and shift in double
__device__ __forceinline__ void minmax_scale(double mn, double mx, double* scale, double* shift) {
#pragma clang fp contract(off)
  const double d = mx - mn;
  *scale = 255.0 * (d > 2.220446049250313e-16 ? 1.0 / d : 0.0);
  *shift = 0.0 - mn * *scale;
}

__device__ __forceinline__ float sharpen_edge(int img, int blur, bool ratio) {
#pragma clang fp contract(off)
  return ratio ? (float)img / ((float)blur + 0.01f) : (float)img - (float)blur;
}

__device__ __forceinline__ int sharpen_e(float edge, float scale, float shift) {
#pragma clang fp contract(off)
  return (int)(edge * scale + shift) & 255;
}

__device__ __forceinline__ double sharpen_v(int img, int e, double alpha) {
#pragma clang fp contract(off)
  return (double)img * (1.0 - alpha) + (double)e * alpha;
}

template <int PASS, int KS>
__device__ __forceinline__ void sharpen_tile(const unsigned char* __restrict__ fr, unsigned char* __restrict__ out, int H,
                                             int W, bool ratio, double alpha, SharpenWs* __restrict__ ws,
                                             unsigned char* s_raw, unsigned short* s_row, unsigned long long* s_red) {
#pragma clang fp contract(off)
  constexpr int R = KS / 2, AREA = KS * KS;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * SH_TW, y0 = blockIdx.y * SH_TH;
  const int tw = min(SH_TW, W - x0), th = min(SH_TH, H - y0);
  const int cols = tw + 2 * R, rows = th + 2 * R;
  for (int i = tid; i < rows * cols; i += 256) {
    const int ry = i / cols, rx = i - ry * cols;
    const unsigned char* q = fr + ((size_t)reflect101(y0 - R + ry, H) * W + (size_t)reflect101(x0 - R + rx, W)) * 3;
    unsigned char* d = s_raw + ry * SH_RAW_PITCH + rx * 3;
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
  }
  __syncthreads();
  const int vals = tw * 3;
  for (int i = tid; i < rows * vals; i += 256) {
    const int ry = i / vals, j = i - ry * vals;
    const unsigned char* q = s_raw + ry * SH_RAW_PITCH + j;
    int s = 0;
#pragma unroll
    for (int d = 0; d < KS; ++d) s += q[d * 3];
    s_row[ry * SH_ROW_PITCH + j] = (unsigned short)s;
  }
  __syncthreads();
  float scale = 0.f, shift = 0.f;
  if (PASS == 2) {
    double sc, sh;
    minmax_scale((double)dec_f32(ws->emin), (double)dec_f32(ws->emax), &sc, &sh);
    scale = (float)sc; shift = (float)sh;
  }
  float elo = INFINITY, ehi = -INFINITY;
  double vlo = INFINITY, vhi = 0.0;
  for (int i = tid; i < th * vals; i += 256) {
    const int py = i / vals, j = i - py * vals;
    const unsigned short* q = s_row + py * SH_ROW_PITCH + j;
    int s = 0;
#pragma unroll
    for (int d = 0; d < KS; ++d) s += q[d * SH_ROW_PITCH];
    const int blur = (s + AREA / 2) / AREA;
    const int img = s_raw[(py + R) * SH_RAW_PITCH + R * 3 + j];
    const float edge = sharpen_edge(img, blur, ratio);
    if (PASS == 1) {
      elo = fminf(elo, edge); ehi = fmaxf(ehi, edge);
    } else {
      const int e = sharpen_e(edge, scale, shift);
      const double v = sharpen_v(img, e, alpha);
      vlo = fmin(vlo, v); vhi = fmax(vhi, v);
      out[((size_t)(y0 + py) * W + (size_t)x0) * 3 + j] = (unsigned char)e;
    }
  }
  // workgroup extrema: shuffles inside a wave, one LDS slot per wave, one atomic pair per workgroup
  unsigned long long lo, hi;
  if (PASS == 1) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      elo = fminf(elo, __shfl_xor(elo, o, 64));
      ehi = fmaxf(ehi, __shfl_xor(ehi, o, 64));
    }
    lo = enc_f32(elo); hi = enc_f32(ehi);
  } else {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      vlo = fmin(vlo, __shfl_xor(vlo, o, 64));
      vhi = fmax(vhi, __shfl_xor(vhi, o, 64));
    }
    lo = (unsigned long long)__double_as_longlong(vlo); hi = (unsigned long long)__double_as_longlong(vhi);
  }
  if ((tid & 63) == 0) { s_red[(tid >> 6) * 2] = lo; s_red[(tid >> 6) * 2 + 1] = hi; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k) {
      lo = s_red[k * 2] < lo ? s_red[k * 2] : lo;
      hi = s_red[k * 2 + 1] > hi ? s_red[k * 2 + 1] : hi;
    }
    if (PASS == 1) {
      atomicMin(&ws->emin, (unsigned)lo);
      atomicMax(&ws->emax, (unsigned)hi);
    } else {
      atomicMin(&ws->vmin, lo);
      atomicMax(&ws->vmax, hi);
    }
  }
}

template <int PASS>
__global__ __launch_bounds__(256) void sharpen_tile_kernel(const unsigned char* __restrict__ src,
                                                           unsigned char* __restrict__ dst, int H, int W,
                                                           const int* __restrict__ ksize, const int* __restrict__ mode,
                                                           const double* __restrict__ alpha,
                                                           SharpenWs* __restrict__ ws) {
  __shared__ unsigned char s_raw[(SH_TH + 2 * SH_RMAX) * SH_RAW_PITCH];
  __shared__ unsigned short s_row[(SH_TH + 2 * SH_RMAX) * SH_ROW_PITCH];
  __shared__ unsigned long long s_red[8];
  const int b = blockIdx.z;
  const int ks = sharpen_ks(ksize[b]);
  if (ks == 0) return;
  const size_t img = (size_t)b * H * W * 3;
  const bool ratio = mode[b] != 0;
  const double a = alpha[b];
  switch (ks) {
    case 5: sharpen_tile<PASS, 5>(src + img, dst + img, H, W, ratio, a, ws + b, s_raw, s_row, s_red); break;
    case 7: sharpen_tile<PASS, 7>(src + img, dst + img, H, W, ratio, a, ws + b, s_raw, s_row, s_red); break;
    case 9: sharpen_tile<PASS, 9>(src + img, dst + img, H, W, ratio, a, ws + b, s_raw, s_row, s_red); break;
    default: sharpen_tile<PASS, 11>(src + img, dst + img, H, W, ratio, a, ws + b, s_raw, s_row, s_red); break;
  }
}

__global__ void sharpen_init_kernel(SharpenWs* __restrict__ ws, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  ws[b].emin = 0xFFFFFFFFu; ws[b].emax = 0u;
  ws[b].vmin = ~0ull; ws[b].vmax = 0ull; ws[b].pad = 0ull;
}

// pass c: per value, out = uint8(v * scale' + shift') from the source byte and the e parked in dst; ks = 0 copies
__global__ __launch_bounds__(256) void sharpen_store_kernel(const unsigned char* __restrict__ src,
                                                            unsigned char* __restrict__ dst, long long nval,
                                                            const int* __restrict__ ksize,
                                                            const double* __restrict__ alpha,
                                                            const SharpenWs* __restrict__ ws) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const unsigned char* s = src + (size_t)b * nval;
  unsigned char* d = dst + (size_t)b * nval;
  const bool on = sharpen_ks(ksize[b]) != 0;
  double scale = 0.0, shift = 0.0;
  if (on) minmax_scale(__longlong_as_double((long long)ws[b].vmin), __longlong_as_double((long long)ws[b].vmax), &scale, &shift);
  const double a = alpha[b];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nval; i += (long long)gridDim.x * 256) {
    if (!on) { d[i] = s[i]; continue; }
    const double v = sharpen_v(s[i], d[i], a);
    d[i] = (unsigned char)((int)(v * scale + shift) & 255);
  }
}

int grid_x(long long npix) {
  long long nb = (npix + 255) / 256;
  return (int)(nb > 1024 ? 1024 : nb);
}

}  // namespace

#define AUG_CHECK_SIZES(name, B, H, W)                                                                    \
  KD6D_CHECK_ARG((B) > 0 && (B) <= 65535 && (H) > 0 && (W) > 0 && (H) <= 16384 && (W) <= 16384,           \
                 name ": bad sizes B=%d H=%d W=%d", (int)(B), (int)(H), (int)(W))

extern "C" int kd6d_aug_warp_u8(const uint8_t* src, const float* src_mask, int B, int H, int W, const double* fwd_mats,
                                int Ho, int Wo, uint8_t* dst, float* dst_mask, void* stream) {
  KD6D_CHECK_ARG(src && fwd_mats && dst, "kd6d_aug_warp_u8: null pointer");
  KD6D_CHECK_ARG((src_mask == nullptr) == (dst_mask == nullptr), "kd6d_aug_warp_u8: src_mask and dst_mask go together");
  KD6D_CHECK_ARG((const void*)src != (const void*)dst, "kd6d_aug_warp_u8: in-place warp is not supported");
  AUG_CHECK_SIZES("kd6d_aug_warp_u8", B, H, W);
  AUG_CHECK_SIZES("kd6d_aug_warp_u8 (output)", B, Ho, Wo);
  hipLaunchKernelGGL(warp_u8_kernel, dim3(grid_x((long long)Ho * Wo), B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), src, src_mask, H, W, fwd_mats, Ho, Wo, dst, dst_mask);
  KD6D_CHECK_LAUNCH("kd6d_aug_warp_u8");
  return KD6D_OK;
}

extern "C" int kd6d_aug_mask_stats(const float* masks, int B, int H, int W, int max_id, int32_t* stats, void* stream) {
  KD6D_CHECK_ARG(masks && stats, "kd6d_aug_mask_stats: null pointer");
  AUG_CHECK_SIZES("kd6d_aug_mask_stats", B, H, W);
  KD6D_CHECK_ARG(max_id >= 1 && max_id <= KD6D_AUG_MAX_ID, "kd6d_aug_mask_stats: max_id=%d outside 1..%d", max_id,
                 KD6D_AUG_MAX_ID);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(stats, 0, sizeof(int32_t) * 5 * (size_t)B * max_id, st) != hipSuccess) {
    kd6d_set_error("kd6d_aug_mask_stats: hipMemsetAsync failed");
    return KD6D_ERR_LAUNCH;
  }
  const long long npix = (long long)H * W;
  const long long nb = (npix + 256 * STATS_PIX_PER_THREAD - 1) / (256 * STATS_PIX_PER_THREAD);
  hipLaunchKernelGGL(mask_stats_kernel, dim3((unsigned)nb, B), dim3(256), 0, st, masks, H, W, max_id, (int*)stats);
  KD6D_CHECK_LAUNCH("kd6d_aug_mask_stats");
  hipLaunchKernelGGL(mask_stats_finish_kernel, dim3((B * max_id + 63) / 64), dim3(64), 0, st, B, H, W, max_id,
                     (int*)stats);
  KD6D_CHECK_LAUNCH("kd6d_aug_mask_stats (finish)");
  return KD6D_OK;
}

extern "C" int kd6d_aug_occlude(uint8_t* frames, float* masks, int B, int H, int W, const int32_t* stats, int stats_ids,
                                const double* uniforms, const int32_t* n_inst, double prob, uint64_t key,
                                void* stream) {
  KD6D_CHECK_ARG(frames && masks && stats && uniforms && n_inst, "kd6d_aug_occlude: null pointer");
  AUG_CHECK_SIZES("kd6d_aug_occlude", B, H, W);
  KD6D_CHECK_ARG(stats_ids >= KD6D_MAX_GT && stats_ids <= KD6D_AUG_MAX_ID,
                 "kd6d_aug_occlude: stats_ids=%d outside %d..%d", stats_ids, KD6D_MAX_GT, KD6D_AUG_MAX_ID);
  hipLaunchKernelGGL(occlude_kernel, dim3(grid_x((long long)H * W), B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), frames, masks, H, W, (const int*)stats, stats_ids, uniforms,
                     (const int*)n_inst, prob, (unsigned long long)key);
  KD6D_CHECK_LAUNCH("kd6d_aug_occlude");
  return KD6D_OK;
}

extern "C" int kd6d_aug_hsv(uint8_t* frames, int B, int H, int W, const float* factors, void* stream) {
  KD6D_CHECK_ARG(frames && factors, "kd6d_aug_hsv: null pointer");
  AUG_CHECK_SIZES("kd6d_aug_hsv", B, H, W);
  hipLaunchKernelGGL(hsv_kernel, dim3(grid_x((long long)H * W), B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), frames, H, W, factors);
  KD6D_CHECK_LAUNCH("kd6d_aug_hsv");
  return KD6D_OK;
}

extern "C" int kd6d_aug_filter(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* ksize,
                               const float* sigma, int gray, uint64_t key, void* stream) {
  KD6D_CHECK_ARG(src && dst, "kd6d_aug_filter: null pointer");
  KD6D_CHECK_ARG((const void*)src != (const void*)dst, "kd6d_aug_filter: in-place filter is not supported");
  AUG_CHECK_SIZES("kd6d_aug_filter", B, H, W);
  hipLaunchKernelGGL(filter_kernel, dim3(grid_x((long long)H * W), B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), src, dst, H, W, (const int*)ksize, sigma, gray,
                     (unsigned long long)key);
  KD6D_CHECK_LAUNCH("kd6d_aug_filter");
  return KD6D_OK;
}

extern "C" int kd6d_aug_relabel(float* masks, int B, int H, int W, const float* lut, int max_id, void* stream) {
  KD6D_CHECK_ARG(masks && lut, "kd6d_aug_relabel: null pointer");
  AUG_CHECK_SIZES("kd6d_aug_relabel", B, H, W);
  KD6D_CHECK_ARG(max_id >= 1 && max_id <= KD6D_AUG_MAX_ID, "kd6d_aug_relabel: max_id=%d outside 1..%d", max_id,
                 KD6D_AUG_MAX_ID);
  hipLaunchKernelGGL(relabel_kernel, dim3(grid_x((long long)H * W), B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), masks, H, W, lut, max_id);
  KD6D_CHECK_LAUNCH("kd6d_aug_relabel");
  return KD6D_OK;
}

extern "C" int kd6d_aug_background(uint8_t* frames, const float* masks, int B, int H, int W, const uint8_t* pool,
                                   int64_t pool_bytes, const int64_t* bg_off, const int32_t* bg_hw, int n_bg,
                                   const int32_t* bg_index, void* stream) {
  KD6D_CHECK_ARG(frames && masks && pool && bg_off && bg_hw && bg_index, "kd6d_aug_background: null pointer");
  AUG_CHECK_SIZES("kd6d_aug_background", B, H, W);
  KD6D_CHECK_ARG(n_bg >= 1 && pool_bytes >= 3, "kd6d_aug_background: empty pool (n_bg=%d, pool_bytes=%lld)", n_bg,
                 (long long)pool_bytes);
  hipLaunchKernelGGL(background_kernel, dim3(grid_x((long long)H * W), B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), frames, masks, H, W, pool, (long long)pool_bytes,
                     (const long long*)bg_off, (const int*)bg_hw, n_bg, (const int*)bg_index);
  KD6D_CHECK_LAUNCH("kd6d_aug_background");
  return KD6D_OK;
}

extern "C" int64_t kd6d_aug_sharpen_ws_bytes(int B) { return B > 0 ? (int64_t)sizeof(SharpenWs) * B : 0; }

extern "C" int kd6d_aug_sharpen(const uint8_t* src, uint8_t* dst, int B, int H, int W, const int32_t* ksize,
                                const int32_t* mode, const double* alpha, void* ws, int64_t ws_bytes, void* stream) {
  KD6D_CHECK_ARG(src && dst && ksize && mode && alpha && ws, "kd6d_aug_sharpen: null pointer");
  KD6D_CHECK_ARG((const void*)src != (const void*)dst, "kd6d_aug_sharpen: in-place sharpen is not supported");
  AUG_CHECK_SIZES("kd6d_aug_sharpen", B, H, W);
  KD6D_CHECK_ARG(ws_bytes >= kd6d_aug_sharpen_ws_bytes(B), "kd6d_aug_sharpen: workspace of %lld bytes, %lld needed",
                 (long long)ws_bytes, (long long)kd6d_aug_sharpen_ws_bytes(B));
  KD6D_CHECK_ARG(((uintptr_t)ws & 7) == 0, "kd6d_aug_sharpen: workspace must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SharpenWs* w = reinterpret_cast<SharpenWs*>(ws);
  hipLaunchKernelGGL(sharpen_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, w, B);
  KD6D_CHECK_LAUNCH("kd6d_aug_sharpen (init)");
  const dim3 tiles((W + SH_TW - 1) / SH_TW, (H + SH_TH - 1) / SH_TH, B);
  hipLaunchKernelGGL(sharpen_tile_kernel<1>, tiles, dim3(256), 0, st, src, dst, H, W, (const int*)ksize,
                     (const int*)mode, alpha, w);
  KD6D_CHECK_LAUNCH("kd6d_aug_sharpen (edge extrema)");
  hipLaunchKernelGGL(sharpen_tile_kernel<2>, tiles, dim3(256), 0, st, src, dst, H, W, (const int*)ksize,
                     (const int*)mode, alpha, w);
  KD6D_CHECK_LAUNCH("kd6d_aug_sharpen (blend extrema)");
  const long long nval = (long long)H * W * 3;
  hipLaunchKernelGGL(sharpen_store_kernel, dim3(grid_x(nval), B), dim3(256), 0, st, src, dst, nval, (const int*)ksize,
                     alpha, (const SharpenWs*)w);
  KD6D_CHECK_LAUNCH("kd6d_aug_sharpen (store)");
  return KD6D_OK;
}
