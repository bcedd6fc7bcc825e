// The sphere ray-caster's pieces, shared by every kernel that draws the joint-action spheres (render.hip: render_spheres_kernel;
// replay_render.hip: replay_render_kernel) so that their pixels agree bit for bit: the eye-space set-up of a view's spheres in LDS, the ray
// cast, the per-pixel shading loop and the byte composites.  genima_hip.h (gn_render_spheres) states the arithmetic.  Files that include
// this are built with -ffp-contract=off: the blend is numpy's unfused f64 multiply / multiply / add, truncated.
#pragma once
#include "common.h"
#include "image_convert.h"

constexpr int MAX_SPHERES = 8;
constexpr int CAM_FLOATS = 18;     // fx fy cx cy | pose 3x4 row-major | znear zfar
constexpr int SPHERE_FLOATS = 16;  // pose 3x4 row-major | radius | factor r g b

struct SphereLds {
  float c[3];     // centre in eye space (camera at the origin, looking down -z, y up)
  float r, r2, inv_r;
  float m[9];     // eye space -> the sphere's frame: Rs^T Rc, row-major
  float f[3];     // base colour factor
  int tex;        // atlas layer, clamped
  int x0, x1, y0, y1;  // inclusive pixel rectangle that holds the silhouette (conservative)
};

// the sphere atlas uint8 [T, th, tw, 4]
struct SphereAtlas {
  const uint8_t* atlas;
  int T, th, tw;
};

__device__ __forceinline__ int wrap(int i, int n) {
  i %= n;
  return i < 0 ? i + n : i;
}

// one sphere of a view into eye space (f64), with its bounding rectangle in a W x H image; tex: its atlas layer, clamped here
__device__ __forceinline__ void sphere_to_lds(SphereLds& d, const float* __restrict__ cam, const float* __restrict__ sp, int tex, int T, int W, int H) {
  const float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
  double Rc[9], Rs[9], o[3], c[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rc[i * 3 + j] = cam[4 + i * 4 + j], Rs[i * 3 + j] = sp[i * 4 + j];
    o[i] = cam[4 + i * 4 + 3], c[i] = sp[i * 4 + 3];
  }
  double ce[3];
  for (int i = 0; i < 3; ++i) {  // Rc^T (c - o)
    ce[i] = Rc[0 * 3 + i] * (c[0] - o[0]) + Rc[1 * 3 + i] * (c[1] - o[1]) + Rc[2 * 3 + i] * (c[2] - o[2]);
    d.c[i] = (float)ce[i];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) d.m[i * 3 + j] = (float)(Rs[0 * 3 + i] * Rc[0 * 3 + j] + Rs[1 * 3 + i] * Rc[1 * 3 + j] + Rs[2 * 3 + i] * Rc[2 * 3 + j]);
  const double r = sp[12];
  d.r = (float)r, d.r2 = (float)(r * r), d.inv_r = (float)(1.0 / r);
  d.f[0] = sp[13], d.f[1] = sp[14], d.f[2] = sp[15];
  d.tex = tex < 0 ? 0 : (tex >= T ? T - 1 : tex);
  // every point of the sphere has x in [cx - r, cx + r] and depth in [zc - r, zc + r]: bound x / depth, project, pad a pixel
  const double zc = -ce[2];
  int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
  if (zc + r <= 0.0 || !(r > 0.0)) {
    x0 = 1, x1 = 0;  // wholly behind the camera: never hit
  } else if (zc - r > 1e-9) {
    const double lo_d = zc - r, hi_d = zc + r;
    const double xa = ce[0] - r, xb = ce[0] + r, ya = ce[1] - r, yb = ce[1] + r;
    const double dx0 = xa / (xa < 0.0 ? lo_d : hi_d), dx1 = xb / (xb > 0.0 ? lo_d : hi_d);
    const double dy0 = ya / (ya < 0.0 ? lo_d : hi_d), dy1 = yb / (yb > 0.0 ? lo_d : hi_d);
    const double ua = (double)cx + (double)fx * dx0, ub = (double)cx + (double)fx * dx1;  // u = cx + fx dx, v = cy - fy dy (signed fx, fy)
    const double va = (double)cy - (double)fy * dy0, vb = (double)cy - (double)fy * dy1;
    const double W1 = W, H1 = H;
    x0 = (int)fmin(fmax(floor(fmin(ua, ub)) - 1.0, 0.0), W1), x1 = (int)fmin(fmax(ceil(fmax(ua, ub)) + 1.0, -1.0), W1 - 1.0);
    y0 = (int)fmin(fmax(floor(fmin(va, vb)) - 1.0, 0.0), H1), y1 = (int)fmin(fmax(ceil(fmax(va, vb)) + 1.0, -1.0), H1 - 1.0);
  }
  d.x0 = x0, d.x1 = x1, d.y0 = y0, d.y1 = y1;
}

// colour of one ray: the nearest front hit's factor * bilinear texel / 255, white on a miss
__device__ __forceinline__ void cast(const SphereLds* __restrict__ sph, int n, const SphereAtlas& k, float dx, float dy, float znear, float zfar,
                                     float& cr, float& cg, float& cb) {
  const float a = dx * dx + dy * dy + 1.0f;
  float best_t = 3.0e38f, tq = 0.0f;  // tq = t - b/a of the winner
  int best = -1;
  float ex = 0.0f, ey = 0.0f, ez = 0.0f;
  for (int s = 0; s < n; ++s) {
    const SphereLds& sp = sph[s];
    const float b = dx * sp.c[0] + dy * sp.c[1] - sp.c[2];
    const float q = b / a;
    const float px = sp.c[0] - q * dx, py = sp.c[1] - q * dy, pz = sp.c[2] + q;  // centre minus its foot on the ray: perpendicular, small
    const float disc = sp.r2 - (px * px + py * py + pz * pz);
    if (disc < 0.0f) continue;
    const float h = sqrtf(disc / a);
    const float t = q - h;  // eye-space depth -z of the front intersection (dz = -1)
    if (!(t > 0.0f) || t < znear || t > zfar || !(t < best_t)) continue;
    best_t = t, best = s, tq = -h, ex = px, ey = py, ez = pz;
  }
  if (best < 0) {
    cr = cg = cb = 1.0f;
    return;
  }
  const SphereLds& sp = sph[best];
  // hit - centre = (t - q) d - (c - q d)
  const float hx = tq * dx - ex, hy = tq * dy - ey, hz = -tq - ez;
  const float lx = sp.m[0] * hx + sp.m[1] * hy + sp.m[2] * hz;
  const float ly = sp.m[3] * hx + sp.m[4] * hy + sp.m[5] * hz;
  const float u = (lx * sp.inv_r + 1.0f) * 0.5f, v = (ly * sp.inv_r + 1.0f) * 0.5f;
  const float x = u * (float)k.tw - 0.5f, y = v * (float)k.th - 0.5f;  // y counts rows from the texture's BOTTOM row
  const float xf = floorf(x), yf = floorf(y);
  const float wx = x - xf, wy = y - yf;
  const int i0 = wrap((int)xf, k.tw), i1 = wrap((int)xf + 1, k.tw);
  const int j0 = k.th - 1 - wrap((int)yf, k.th), j1 = k.th - 1 - wrap((int)yf + 1, k.th);
  const uchar4* __restrict__ tex = reinterpret_cast<const uchar4*>(k.atlas) + (long)sp.tex * k.th * k.tw;
  const uchar4 t00 = tex[j0 * k.tw + i0], t01 = tex[j0 * k.tw + i1], t10 = tex[j1 * k.tw + i0], t11 = tex[j1 * k.tw + i1];
  const float w00 = (1.0f - wx) * (1.0f - wy), w01 = wx * (1.0f - wy), w10 = (1.0f - wx) * wy, w11 = wx * wy;
  cr = sp.f[0] * ((w00 * t00.x + w01 * t01.x + w10 * t10.x + w11 * t11.x) / 255.0f);
  cg = sp.f[1] * ((w00 * t00.y + w01 * t01.y + w10 * t10.y + w11 * t11.y) / 255.0f);
  cb = sp.f[2] * ((w00 * t00.z + w01 * t01.z + w10 * t10.z + w11 * t11.z) / 255.0f);
}

__device__ __forceinline__ uint8_t to_u8(float c) { return (uint8_t)fminf(fmaxf(rintf(255.0f * c), 0.0f), 255.0f); }

// the rendered colour of pixel (px, py) of a view whose n spheres are in sph: white outside every bounding rectangle, without casting a ray
__device__ __forceinline__ void shade_pixel(const SphereLds* __restrict__ sph, int n, const SphereAtlas& k, const float* __restrict__ cam, int samples, int px,
                                            int py, uint8_t& r8, uint8_t& g8, uint8_t& b8) {
  const float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], znear = cam[16], zfar = cam[17];
  bool near = false;
  for (int s = 0; s < n; ++s) near |= px >= sph[s].x0 && px <= sph[s].x1 && py >= sph[s].y0 && py <= sph[s].y1;
  r8 = 255, g8 = 255, b8 = 255;
  if (near) {
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    const int ns = samples;
    for (int i = 0; i < ns; ++i) {
      // samples = 4: (0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875)
      const float ox = ns == 1 ? 0.5f : (i == 0 ? 0.375f : i == 1 ? 0.875f : i == 2 ? 0.125f : 0.625f);
      const float oy = ns == 1 ? 0.5f : 0.125f + 0.25f * (float)i;
      const float u = (float)px + ox, v = (float)py + oy;
      float cr, cg, cb;
      cast(sph, n, k, (u - cx) / fx, (cy - v) / fy, znear, zfar, cr, cg, cb);
      ar += cr, ag += cg, ab += cb;
    }
    const float inv = 1.0f / (float)ns;
    r8 = to_u8(ar * inv), g8 = to_u8(ag * inv), b8 = to_u8(ab * inv);
  }
}

// numpy: uint8 * float -> float64, added, cast back to uint8 (truncation)
__device__ __forceinline__ uint8_t blend_u8(uint8_t p, uint8_t t, double blend, double one_minus) {
  return (uint8_t)(int)__dadd_rn(__dmul_rn((double)p, blend), __dmul_rn((double)t, one_minus));
}

__device__ __forceinline__ void store_f16_pixel(f16* __restrict__ o, uint8_t r, uint8_t g, uint8_t b, float mul, float add) {
  const f16 z = (f16)0.0f;
  *reinterpret_cast<f16x8*>(o) = f16x8{u8_to_f16_value(r, mul, add), u8_to_f16_value(g, mul, add), u8_to_f16_value(b, mul, add), z, z, z, z, z};
}
