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
//   kd6d_aug_hsv          RandomHSV: cv2 8-bit BGR->HSV, float32 scale, truncating store, HSV->BGR (in place)
//   kd6d_aug_filter       RandomSmooth (cv2.blur, BORDER_REFLECT_101) + RandomNoise + Grayscalize, fused
//   kd6d_aug_relabel      remove_invalids: per-image id lookup table on the mask
//
// One thread per output pixel, all three channels.  Everything is HBM / latency bound: plain loads and
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
