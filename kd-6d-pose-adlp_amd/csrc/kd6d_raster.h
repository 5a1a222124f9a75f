// The tiled rasteriser shared by bop_vsd.hip (depth, VSD counts) and render_frames.hip (colour, visible mask): camera,
// pose, projection, the per-item region of interest and the triangle walk.  The contract is the one stated at the head
// of bop_vsd.hip and in kd6d/libs/bop_metrics.py; every expression below is the one those kernels were tested with --
// the walk hands each covered pixel to a sink, so that both units form coverage and depth with the same arithmetic.
#pragma once
#include <math.h>

#include "kd6d_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 64;                // the tile is kTile x kTile pixels
constexpr unsigned kEmpty = 0xffffffffu;

struct Pose {
  float R[9], T[3];
};

struct Cam {
  float fx, sk, cx, fy, cy;
};

__device__ __forceinline__ Cam load_cam(const float* K) { return {K[0], K[1], K[2], K[4], K[5]}; }

__device__ __forceinline__ Pose load_pose(const float* R, const float* T, int p) {
  Pose q;
#pragma unroll
  for (int i = 0; i < 9; ++i) q.R[i] = R[(size_t)p * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) q.T[i] = T[(size_t)p * 3 + i];
  return q;
}

__device__ __forceinline__ void rot3(const float* R, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = fmaf(R[2], z, fmaf(R[1], y, R[0] * x));
  oy = fmaf(R[5], z, fmaf(R[4], y, R[3] * x));
  oz = fmaf(R[8], z, fmaf(R[7], y, R[6] * x));
}

__device__ __forceinline__ void project(const Cam& c, float X, float Y, float Z, float& u, float& v) {
  u = fmaf(c.sk, Y, c.fx * X) / Z + c.cx;
  v = c.fy * Y / Z + c.cy;
}

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

// float pixel bound -> int, safe for infinities and NaN (clamped to [-2, limit + 1] first)
__device__ __forceinline__ int to_px(float x, int limit) { return (int)fminf(fmaxf(x, -2.f), (float)limit + 1.f); }

// Region of interest of one item (the whole workgroup calls this): the bounding box of the vc vertices `mesh` projected
// (z > 0) under the NB poses q, widened by one pixel and clipped to the image -> roi = (x0, y0, x1, y1), empty
// (x1 < x0) when nothing can be drawn.  red: kWaves x 4 floats of LDS.
template <int NB>
__device__ __forceinline__ void item_roi(const float* mesh, int vc, const Cam& cam, const Pose* q, int H, int W,
                                         float (*red)[4], int32_t* roi, int tid) {
  float lo_u = INFINITY, lo_v = INFINITY, hi_u = -INFINITY, hi_v = -INFINITY;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    for (int i = tid; i < vc; i += kThreads) {
      const float* m = mesh + (size_t)i * 3;
      float X, Y, Z, u, v;
      rot3(q[b].R, m[0], m[1], m[2], X, Y, Z);
      X += q[b].T[0]; Y += q[b].T[1]; Z += q[b].T[2];
      if (Z > 0.f) {
        project(cam, X, Y, Z, u, v);
        lo_u = fminf(lo_u, u); hi_u = fmaxf(hi_u, u);
        lo_v = fminf(lo_v, v); hi_v = fmaxf(hi_v, v);
      }
    }
  }
  lo_u = wave_min(lo_u); lo_v = wave_min(lo_v); hi_u = wave_max(hi_u); hi_v = wave_max(hi_v);
  if ((tid & 63) == 0) { red[tid >> 6][0] = lo_u; red[tid >> 6][1] = lo_v; red[tid >> 6][2] = hi_u; red[tid >> 6][3] = hi_v; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      lo_u = fminf(lo_u, red[w][0]); lo_v = fminf(lo_v, red[w][1]);
      hi_u = fmaxf(hi_u, red[w][2]); hi_v = fmaxf(hi_v, red[w][3]);
    }
    // one pixel wider than the box: a tile test never decides coverage, the edge functions do
    const int x0 = max(to_px(floorf(lo_u), W) - 1, 0), y0 = max(to_px(floorf(lo_v), H) - 1, 0);
    const int x1 = min(to_px(ceilf(hi_u), W) + 1, W - 1), y1 = min(to_px(ceilf(hi_v), H) + 1, H - 1);
    const bool none = !(lo_u <= hi_u) || x1 < x0 || y1 < y0;
    roi[0] = x0; roi[1] = y0; roi[2] = none ? x0 - 1 : x1; roi[3] = none ? y0 - 1 : y1;
  }
}

// One pose of a mesh (vc vertices `mesh`, fc triangles `tri`) over the tile (ox, oy, w, h) of an H x W image: a triangle
// per lane.  sink(i, z, f): pixel i = (y - oy) * kTile + (x - ox) of the tile is covered by triangle f at depth z.
template <class Sink>
__device__ __forceinline__ void rasterise(const float* mesh, const int32_t* tri, int vc, int fc, int H, int W,
                                          const Cam& cam, const Pose& q, int ox, int oy, int w, int h, int tid,
                                          Sink sink) {
  for (int f = tid; f < fc; f += kThreads) {
    const int i0 = tri[(size_t)f * 3], i1 = tri[(size_t)f * 3 + 1], i2 = tri[(size_t)f * 3 + 2];
    if ((unsigned)i0 >= (unsigned)vc || (unsigned)i1 >= (unsigned)vc || (unsigned)i2 >= (unsigned)vc) continue;
    const float* m0 = mesh + (size_t)i0 * 3;
    const float* m1 = mesh + (size_t)i1 * 3;
    const float* m2 = mesh + (size_t)i2 * 3;
    const float ax = m0[0], ay = m0[1], az = m0[2];
    float X0, Y0, Z0, X1, Y1, Z1, X2, Y2, Z2;
    rot3(q.R, ax, ay, az, X0, Y0, Z0);
    rot3(q.R, m1[0], m1[1], m1[2], X1, Y1, Z1);
    rot3(q.R, m2[0], m2[1], m2[2], X2, Y2, Z2);
    X0 += q.T[0]; Y0 += q.T[1]; Z0 += q.T[2];
    X1 += q.T[0]; Y1 += q.T[1]; Z1 += q.T[2];
    X2 += q.T[0]; Y2 += q.T[1]; Z2 += q.T[2];
    if (!(Z0 > 0.f && Z1 > 0.f && Z2 > 0.f)) continue;
    float u0, v0, u1, v1, u2, v2;
    project(cam, X0, Y0, Z0, u0, v0);
    project(cam, X1, Y1, Z1, u1, v1);
    project(cam, X2, Y2, Z2, u2, v2);
    const float lu = fminf(u0, fminf(u1, u2)), hu = fmaxf(u0, fmaxf(u1, u2));
    const float lv = fminf(v0, fminf(v1, v2)), hv = fmaxf(v0, fmaxf(v1, v2));
    const int xa = max(to_px(ceilf(lu), W), ox), xb = min(to_px(floorf(hu), W), ox + w - 1);
    const int ya = max(to_px(ceilf(lv), H), oy), yb = min(to_px(floorf(hv), H), oy + h - 1);
    if (xa > xb || ya > yb) continue;
    const float e01x = u1 - u0, e01y = v1 - v0, e12x = u2 - u1, e12y = v2 - v1, e20x = u0 - u2, e20y = v0 - v2;
    const float area = fmaf(e01x, v2 - v0, -(e01y * (u2 - u0)));
    if (!(area != 0.f)) continue;        // zero area, or NaN
    const float sg = area > 0.f ? 1.f : -1.f;
    // the plane: n_o in the object frame, n = R n_o, n . X0 = n_o . v0 + n . T
    const float bx = m1[0] - ax, by = m1[1] - ay, bz = m1[2] - az;
    const float cx = m2[0] - ax, cy = m2[1] - ay, cz = m2[2] - az;
    const float nox = fmaf(by, cz, -(bz * cy)), noy = fmaf(bz, cx, -(bx * cz)), noz = fmaf(bx, cy, -(by * cx));
    float nx, ny, nz;
    rot3(q.R, nox, noy, noz, nx, ny, nz);
    const float d = fmaf(noz, az, fmaf(noy, ay, nox * ax)) + fmaf(nz, q.T[2], fmaf(ny, q.T[1], nx * q.T[0]));
    const float zlo = fminf(Z0, fminf(Z1, Z2)), zhi = fmaxf(Z0, fmaxf(Z1, Z2));
    for (int y = ya; y <= yb; ++y) {
      const float py = (float)y;
      const float ry = (py - cam.cy) / cam.fy;
      for (int x = xa; x <= xb; ++x) {
        const float px = (float)x;
        const float w0 = fmaf(e01x, py - v0, -(e01y * (px - u0))) * sg;
        const float w1 = fmaf(e12x, py - v1, -(e12y * (px - u1))) * sg;
        const float w2 = fmaf(e20x, py - v2, -(e20y * (px - u2))) * sg;
        if (!(w0 >= 0.f && w1 >= 0.f && w2 >= 0.f)) continue;
        const float rx = (px - cam.cx - cam.sk * ry) / cam.fx;
        const float den = fmaf(nx, rx, fmaf(ny, ry, nz));
        float z = den != 0.f ? d / den : zlo;
        z = fminf(fmaxf(z, zlo), zhi);   // a NaN takes zlo
        sink((y - oy) * kTile + (x - ox), z, f);
      }
    }
  }
}

}  // namespace
