// Training frames on the GPU: a colour rasteriser that draws n_frames full frames of up to KD6D_MAX_GT shaded objects
// each over a background, with the visible-instance mask (and, optionally, the depth) of every frame --
// kd6d/libs/render.py::render_frames_host is the float64 definition.
//
// Coverage and depth are the rasteriser contract of bop_vsd.hip, bit for bit: both units walk the triangles with
// kd6d_raster.h.  Owner of a pixel: the triangle of the smallest depth; among triangles whose depth at the pixel is
// bit-equal, the lowest (slot g, face index f).  Colour of a pixel from its owner (vertices v0 v1 v2, camera z Z0 Z1 Z2,
// projected edge functions E01 E12 E20 of the pixel centre, times the sign of the area):
//     b0 = E12 / Z0, b1 = E20 / Z1, b2 = E01 / Z2                   perspective-correct barycentric weights ...
//     albedo_c = (b0 c0 + b1 c1 + b2 c2) / (b0 + b1 + b2)           ... of the vertex colours (vcol, uint8 RGB)
//     n = R normalize((v1 - v0) x (v2 - v0)), negated when n . X0 > 0 (it then points away from the camera)
//     shade = ambient + (1 - ambient) max(0, n . light)
//     out_c = clamp(floor(albedo_c shade + 0.5), 0, 255), written BGR; mask = g + 1
// A pixel without an owner takes backgrounds[bg_index[frame]] (zeros when the index is outside the pool), mask 0, depth 0.
//
//   frames_roi_kernel   ONE WORKGROUP PER ITEM: validates the item (offsets and counts inside the pools, fcnt < 2^28,
//                       frame in [0, n_frames), slot in [0, KD6D_MAX_GT)), writes its region of interest and enters it
//                       into slot_item[frame][slot] with an integer atomic min: of several items that claim one slot
//                       the lowest item index is drawn.  An invalid item is never dereferenced again.
//   frames_tile_kernel  ONE WORKGROUP PER (FRAME, 64 x 64 TILE OF THE IMAGE), 256 threads, a depth and an owner buffer in
//                       LDS (2 x 16 KiB).  Pass 1: every object whose region of interest meets the tile is rasterised, the
//                       z-test an LDS unsigned-integer atomic min on the depth's bits.  Barrier.  Pass 2: the same walk
//                       (the same code, hence the same bits) does an atomic min of the packed owner id g << 28 | f
//                       wherever the triangle's depth equals the winner's.  Barrier.  Resolve: one pixel per lane.
//
// Bitwise property: two integer minima decide everything, so a frame is a pure function of its own inputs -- the same in
// any batch, under any order of the items, of a mesh's faces (where no two distinct faces tie) and with a face repeated.
// No float atomics, no global z-buffer.
#include <math.h>

#include "kd6d_common.h"
#include "kd6d_raster.h"

namespace {

constexpr int kMaxGt = KD6D_MAX_GT;
constexpr int kFaceBits = 28;
static_assert(kMaxGt == 4, "the owner id keeps 4 bits for the slot and the resolve selects among 4 items");

struct FramesArgs {
  const float* verts;
  const int32_t* faces;
  const uint8_t* vcol;
  int n_verts, n_faces;
  const int32_t* voff;
  const int32_t* vcnt;
  const int32_t* foff;
  const int32_t* fcnt;
  const int32_t* item_frame;
  const int32_t* item_slot;
  const float* R;
  const float* T;
  const float* K;
  const float* light;
  const float* ambient;
  const int32_t* bg_index;
  const uint8_t* backgrounds;
  int n_bg, n_frames, n_items, H, W;
  int32_t* roi;
  int32_t* slot_item;
  uint8_t* frames;
  uint8_t* masks;
  float* depth;
};

__global__ __launch_bounds__(kThreads) void frames_roi_kernel(FramesArgs a) {
  __shared__ float red[kWaves][4];
  const int p = blockIdx.x;
  const int tid = threadIdx.x;
  const int vo = a.voff[p], vc = a.vcnt[p], fo = a.foff[p], fc = a.fcnt[p];
  const int fr = a.item_frame[p], g = a.item_slot[p];
  const bool ok = vo >= 0 && vc >= 1 && (long long)vo + vc <= a.n_verts && fo >= 0 && fc >= 1 &&
                  (long long)fo + fc <= a.n_faces && fc < (1 << kFaceBits) && fr >= 0 && fr < a.n_frames && g >= 0 &&
                  g < kMaxGt;
  int32_t* roi = a.roi + (size_t)p * 4;
  if (!ok) {                             // wave-uniform: the item's own scalars decide
    if (tid == 0) { roi[0] = 0; roi[1] = 0; roi[2] = -1; roi[3] = -1; }
    return;
  }
  const Cam cam = load_cam(a.K + (size_t)fr * 9);
  const Pose q = load_pose(a.R, a.T, p);
  item_roi<1>(a.verts + (size_t)vo * 3, vc, cam, &q, a.H, a.W, red, roi, tid);
  if (tid == 0) atomicMin(&a.slot_item[(size_t)fr * kMaxGt + g], p);
}

__device__ __forceinline__ unsigned char to_level(float c) { return (unsigned char)fminf(fmaxf(floorf(c + 0.5f), 0.f), 255.f); }

__global__ __launch_bounds__(kThreads) void frames_tile_kernel(FramesArgs a) {
  __shared__ unsigned zb[kTile * kTile];
  __shared__ unsigned ob[kTile * kTile];
  const int fr = blockIdx.x;
  const int tid = threadIdx.x;
  const int tw = (a.W + kTile - 1) / kTile;
  const int ox = ((int)blockIdx.y % tw) * kTile, oy = ((int)blockIdx.y / tw) * kTile;
  const int w = min(kTile, a.W - ox), h = min(kTile, a.H - oy);
  for (int i = tid; i < kTile * kTile; i += kThreads) { zb[i] = kEmpty; ob[i] = kEmpty; }
  const Cam cam = load_cam(a.K + (size_t)fr * 9);
  int item[kMaxGt];
#pragma unroll
  for (int g = 0; g < kMaxGt; ++g) {     // wave-uniform: the frame's own table and the items' regions decide
    int p = a.slot_item[(size_t)fr * kMaxGt + g];
    if (p < 0 || p >= a.n_items) p = -1;
    if (p >= 0) {
      const int32_t* roi = a.roi + (size_t)p * 4;
      if (roi[2] < roi[0] || roi[3] < roi[1] || roi[2] < ox || roi[0] > ox + w - 1 || roi[3] < oy || roi[1] > oy + h - 1)
        p = -1;
    }
    item[g] = p;
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < kMaxGt; ++g) {
    const int p = item[g];
    if (p < 0) continue;
    const Pose q = load_pose(a.R, a.T, p);
    rasterise(a.verts + (size_t)a.voff[p] * 3, a.faces + (size_t)a.foff[p] * 3, a.vcnt[p], a.fcnt[p], a.H, a.W, cam, q, ox,
              oy, w, h, tid, [](int i, float z, int) { atomicMin(&zb[i], __float_as_uint(z)); });
  }
  __syncthreads();
  // INVARIANT: this second instance of rasterise() must form the very bits of z the first one did, or a covered pixel
  // finds no owner and falls to the background.  Every product-sum of the walk is an explicit fmaf except
  // `px - cam.cx - cam.sk * ry`, which the compiler may contract; it has to decide alike in both instances (it does: one
  // expression, one use).  tests/test_render_frames_gpu.py pins it: mask > 0 equals depth > 0 on every case, and the depth
  // equals kd6d_render_depth's bit for bit.  (Switching contraction off inside rasterise() would change kd6d_bop_vsd's bits.)
#pragma unroll
  for (int g = 0; g < kMaxGt; ++g) {
    const int p = item[g];
    if (p < 0) continue;
    const Pose q = load_pose(a.R, a.T, p);
    rasterise(a.verts + (size_t)a.voff[p] * 3, a.faces + (size_t)a.foff[p] * 3, a.vcnt[p], a.fcnt[p], a.H, a.W, cam, q, ox,
              oy, w, h, tid, [g](int i, float z, int f) {
                if (zb[i] == __float_as_uint(z)) atomicMin(&ob[i], ((unsigned)g << kFaceBits) | (unsigned)f);
              });
  }
  __syncthreads();

  const int bi = a.bg_index[fr];
  const uint8_t* bg = (bi >= 0 && bi < a.n_bg) ? a.backgrounds + (size_t)bi * a.H * a.W * 3 : nullptr;
  const float lx = a.light[(size_t)fr * 3], ly = a.light[(size_t)fr * 3 + 1], lz = a.light[(size_t)fr * 3 + 2];
  const float amb = a.ambient[fr];
  for (int i = tid; i < kTile * kTile; i += kThreads) {
    const int tx = i % kTile, ty = i / kTile;
    if (tx >= w || ty >= h) continue;
    const int x = ox + tx, y = oy + ty;
    const size_t pix = (size_t)fr * a.H * a.W + (size_t)y * a.W + x;
    const unsigned own = ob[i];
    if (own == kEmpty) {
      const size_t src = ((size_t)y * a.W + x) * 3;
      a.frames[pix * 3] = bg ? bg[src] : 0;
      a.frames[pix * 3 + 1] = bg ? bg[src + 1] : 0;
      a.frames[pix * 3 + 2] = bg ? bg[src + 2] : 0;
      a.masks[pix] = 0;
      if (a.depth) a.depth[pix] = 0.f;
      continue;
    }
    const int g = (int)(own >> kFaceBits), f = (int)(own & ((1u << kFaceBits) - 1));
    const int p = item[0] * (g == 0) + item[1] * (g == 1) + item[2] * (g == 2) + item[3] * (g == 3);
    const Pose q = load_pose(a.R, a.T, p);
    const float* mesh = a.verts + (size_t)a.voff[p] * 3;
    const uint8_t* col = a.vcol + (size_t)a.voff[p] * 3;
    const int32_t* tri = a.faces + ((size_t)a.foff[p] + f) * 3;
    const int i0 = tri[0], i1 = tri[1], i2 = tri[2];         // an owner passed the index check of the walk
    const float* m0 = mesh + (size_t)i0 * 3;
    const float* m1 = mesh + (size_t)i1 * 3;
    const float* m2 = mesh + (size_t)i2 * 3;
    const float ax = m0[0], ay = m0[1], az = m0[2];
    float X0, Y0, Z0, X1, Y1, Z1, X2, Y2, Z2, u0, v0, u1, v1, u2, v2;
    rot3(q.R, ax, ay, az, X0, Y0, Z0);
    rot3(q.R, m1[0], m1[1], m1[2], X1, Y1, Z1);
    rot3(q.R, m2[0], m2[1], m2[2], X2, Y2, Z2);
    X0 += q.T[0]; Y0 += q.T[1]; Z0 += q.T[2];
    X1 += q.T[0]; Y1 += q.T[1]; Z1 += q.T[2];
    X2 += q.T[0]; Y2 += q.T[1]; Z2 += q.T[2];
    project(cam, X0, Y0, Z0, u0, v0);
    project(cam, X1, Y1, Z1, u1, v1);
    project(cam, X2, Y2, Z2, u2, v2);
    const float e01x = u1 - u0, e01y = v1 - v0, e12x = u2 - u1, e12y = v2 - v1, e20x = u0 - u2, e20y = v0 - v2;
    const float area = fmaf(e01x, v2 - v0, -(e01y * (u2 - u0)));
    const float sg = area > 0.f ? 1.f : -1.f;
    const float px = (float)x, py = (float)y;
    const float w01 = fmaf(e01x, py - v0, -(e01y * (px - u0))) * sg;
    const float w12 = fmaf(e12x, py - v1, -(e12y * (px - u1))) * sg;
    const float w20 = fmaf(e20x, py - v2, -(e20y * (px - u2))) * sg;
    float b0 = w12 / Z0, b1 = w20 / Z1, b2 = w01 / Z2;
    float bs = b0 + b1 + b2;
    if (!(bs > 0.f)) { b0 = b1 = b2 = 1.f; bs = 3.f; }      // all three edge functions zero: no weight to form
    const float bx = m1[0] - ax, by = m1[1] - ay, bz = m1[2] - az;
    const float cx = m2[0] - ax, cy = m2[1] - ay, cz = m2[2] - az;
    const float nox = fmaf(by, cz, -(bz * cy)), noy = fmaf(bz, cx, -(bx * cz)), noz = fmaf(bx, cy, -(by * cx));
    float nx, ny, nz;
    rot3(q.R, nox, noy, noz, nx, ny, nz);
    const float d = fmaf(noz, az, fmaf(noy, ay, nox * ax)) + fmaf(nz, q.T[2], fmaf(ny, q.T[1], nx * q.T[0]));
    const float len = sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx)));
    float ndl = fmaf(nz, lz, fmaf(ny, ly, nx * lx)) / len;
    if (d > 0.f) ndl = -ndl;
    const float shade = amb + (1.f - amb) * fmaxf(ndl, 0.f);            // a NaN (zero normal) shades as ambient
    const uint8_t* c0 = col + (size_t)i0 * 3;
    const uint8_t* c1 = col + (size_t)i1 * 3;
    const uint8_t* c2 = col + (size_t)i2 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float alb = fmaf(b2, (float)c2[c], fmaf(b1, (float)c1[c], b0 * (float)c0[c])) / bs;
      a.frames[pix * 3 + (2 - c)] = to_level(alb * shade);              // vcol is RGB, a frame is BGR
    }
    a.masks[pix] = (uint8_t)(g + 1);
    if (a.depth) a.depth[pix] = __uint_as_float(zb[i]);
  }
}

}  // namespace

extern "C" int64_t kd6d_render_frames_workspace_ints(int n_frames, int n_items) {
  return 4 * (int64_t)(n_items > 0 ? n_items : 0) + kMaxGt * (int64_t)(n_frames > 0 ? n_frames : 0);
}

extern "C" int kd6d_render_frames(int n_frames, int n_items, const float* verts, int n_verts, const int32_t* faces,
                                  int n_faces, const uint8_t* vcol, const int32_t* voff, const int32_t* vcnt,
                                  const int32_t* foff, const int32_t* fcnt, const int32_t* item_frame,
                                  const int32_t* item_slot, const float* R, const float* T, const float* K,
                                  const float* light, const float* ambient, const int32_t* bg_index,
                                  const uint8_t* backgrounds, int n_bg, int H, int W, int32_t* workspace,
                                  int64_t workspace_ints, uint8_t* frames_out, uint8_t* masks_out, float* depth_out,
                                  void* stream) {
  KD6D_CHECK_ARG(n_frames >= 0 && n_frames <= 0x1fffffff && n_items >= 0 && n_items <= 0x7f000000,
                 "kd6d_render_frames: %d frames, %d items", n_frames, n_items);
  KD6D_CHECK_ARG(n_verts >= 0 && n_faces >= 0 && n_bg >= 0, "kd6d_render_frames: pools of %d vertices, %d faces and %d "
                 "backgrounds", n_verts, n_faces, n_bg);
  KD6D_CHECK_ARG(H >= 1 && W >= 1 && (long long)cdiv(H, kTile) * cdiv(W, kTile) <= 65535 && (long long)H * W < (1LL << 31),
                 "kd6d_render_frames: image of %d x %d pixels", W, H);
  if (n_frames == 0) return KD6D_OK;
  KD6D_CHECK_ARG(K && light && ambient && bg_index && workspace && frames_out && masks_out && (n_bg == 0 || backgrounds),
                 "kd6d_render_frames: null pointer");
  KD6D_CHECK_ARG(n_items == 0 || (verts && faces && vcol && voff && vcnt && foff && fcnt && item_frame && item_slot && R && T),
                 "kd6d_render_frames: null pointer");
  KD6D_CHECK_ARG(workspace_ints >= kd6d_render_frames_workspace_ints(n_frames, n_items), "kd6d_render_frames: workspace of "
                 "%lld ints, %d frames and %d items need %lld (kd6d_render_frames_workspace_ints)",
                 (long long)workspace_ints, n_frames, n_items,
                 (long long)kd6d_render_frames_workspace_ints(n_frames, n_items));
  FramesArgs a = {};
  a.verts = verts; a.faces = faces; a.vcol = vcol; a.n_verts = n_verts; a.n_faces = n_faces;
  a.voff = voff; a.vcnt = vcnt; a.foff = foff; a.fcnt = fcnt; a.item_frame = item_frame; a.item_slot = item_slot;
  a.R = R; a.T = T; a.K = K; a.light = light; a.ambient = ambient; a.bg_index = bg_index;
  a.backgrounds = backgrounds; a.n_bg = n_bg; a.n_frames = n_frames; a.n_items = n_items; a.H = H; a.W = W;
  a.roi = workspace; a.slot_item = workspace + 4 * (size_t)n_items;
  a.frames = frames_out; a.masks = masks_out; a.depth = depth_out;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  KD6D_CHECK_ARG(hipMemsetAsync(a.slot_item, 0x7f, (size_t)n_frames * kMaxGt * sizeof(int32_t), s) == hipSuccess,
                 "kd6d_render_frames: clearing the slot table failed");
  if (n_items > 0) {
    hipLaunchKernelGGL(frames_roi_kernel, dim3((unsigned)n_items), dim3(kThreads), 0, s, a);
    KD6D_CHECK_LAUNCH("kd6d_render_frames");
  }
  hipLaunchKernelGGL(frames_tile_kernel, dim3((unsigned)n_frames, (unsigned)(cdiv(H, kTile) * cdiv(W, kTile))),
                     dim3(kThreads), 0, s, a);
  KD6D_CHECK_LAUNCH("kd6d_render_frames");
  return KD6D_OK;
}
