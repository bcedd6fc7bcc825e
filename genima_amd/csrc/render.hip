// Joint-action sphere renderer (render/joint_marker.py + the composite of render/render_data.py:282-307): an analytic ray-caster for
// the flat-shaded textured spheres the reference draws with pyrender, and the white-keyed composite over the RGB frame / the alpha
// blend over a random texture, in ONE launch per batch of views.  genima_hip.h (gn_render_spheres) states the arithmetic.
//
// Shape: blockIdx.z = view, a block is 64 x 4 pixels (a wave = 64 consecutive pixels of one row: 1 KiB of contiguous 16-byte stores
// on the f16 NHWC-8 output).  The first `count` threads of a block bring the view's spheres into eye space (f64, once per block) and
// leave them in LDS with their bounding rectangles; a pixel outside every rectangle is white without casting a ray.  No scratch, no
// atomics.  Built with -ffp-contract=off: the blend is numpy's unfused f64 multiply / multiply / add, truncated.
#include "common.h"
#include "image_convert.h"

namespace {

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

struct KParams {
  const float* cams;
  const float* spheres;
  const int32_t* tex_index;
  const int32_t* count;
  const uint8_t* atlas;
  const uint8_t* bg;
  const uint8_t* bg2;
  const double* blend;
  const int32_t* tile_index;
  const uint8_t* const* bg_frames;
  uint8_t* full;
  uint8_t* rnd;
  uint8_t* occupied;
  f16* full_f16;
  f16* rnd_f16;
  int S, H, W, T, th, tw, samples, bg_tiled, n_tiled;
  float full_mul, full_add, rnd_mul, rnd_add;
};

__device__ __forceinline__ int wrap(int i, int n) {
  i %= n;
  return i < 0 ? i + n : i;
}

// colour of one ray: the nearest front hit's factor * bilinear texel / 255, white on a miss
__device__ __forceinline__ void cast(const SphereLds* __restrict__ sph, int n, const KParams& k, float dx, float dy, float znear, float zfar,
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

// numpy: uint8 * float -> float64, added, cast back to uint8 (truncation)
__device__ __forceinline__ uint8_t blend_u8(uint8_t p, uint8_t t, double blend, double one_minus) {
  return (uint8_t)(int)__dadd_rn(__dmul_rn((double)p, blend), __dmul_rn((double)t, one_minus));
}

__device__ __forceinline__ void store_f16_pixel(f16* __restrict__ o, uint8_t r, uint8_t g, uint8_t b, float mul, float add) {
  const f16 z = (f16)0.0f;
  *reinterpret_cast<f16x8*>(o) = f16x8{u8_to_f16_value(r, mul, add), u8_to_f16_value(g, mul, add), u8_to_f16_value(b, mul, add), z, z, z, z, z};
}

__global__ __launch_bounds__(256) void render_spheres_kernel(const KParams k) {
  __shared__ SphereLds sph[MAX_SPHERES];
  const int view = blockIdx.z;
  const float* __restrict__ cam = k.cams + (long)view * CAM_FLOATS;
  const float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], znear = cam[16], zfar = cam[17];
  int n = k.count[view];
  n = n < 0 ? 0 : (n > k.S ? k.S : n);
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if (tid < n) {
    const float* __restrict__ sp = k.spheres + ((long)view * k.S + tid) * SPHERE_FLOATS;
    double Rc[9], Rs[9], o[3], c[3];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Rc[i * 3 + j] = cam[4 + i * 4 + j], Rs[i * 3 + j] = sp[i * 4 + j];
      o[i] = cam[4 + i * 4 + 3], c[i] = sp[i * 4 + 3];
    }
    SphereLds& d = sph[tid];
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
    const int t = k.tex_index[(long)view * k.S + tid];
    d.tex = t < 0 ? 0 : (t >= k.T ? k.T - 1 : t);
    // every point of the sphere has x in [cx - r, cx + r] and depth in [zc - r, zc + r]: bound x / depth, project, pad a pixel
    const double zc = -ce[2];
    int x0 = 0, x1 = k.W - 1, y0 = 0, y1 = k.H - 1;
    if (zc + r <= 0.0 || !(r > 0.0)) {
      x0 = 1, x1 = 0;  // wholly behind the camera: never hit
    } else if (zc - r > 1e-9) {
      const double lo_d = zc - r, hi_d = zc + r;
      const double xa = ce[0] - r, xb = ce[0] + r, ya = ce[1] - r, yb = ce[1] + r;
      const double dx0 = xa / (xa < 0.0 ? lo_d : hi_d), dx1 = xb / (xb > 0.0 ? lo_d : hi_d);
      const double dy0 = ya / (ya < 0.0 ? lo_d : hi_d), dy1 = yb / (yb > 0.0 ? lo_d : hi_d);
      const double ua = (double)cx + (double)fx * dx0, ub = (double)cx + (double)fx * dx1;  // u = cx + fx dx, v = cy - fy dy (signed fx, fy)
      const double va = (double)cy - (double)fy * dy0, vb = (double)cy - (double)fy * dy1;
      const double W1 = k.W, H1 = k.H;
      x0 = (int)fmin(fmax(floor(fmin(ua, ub)) - 1.0, 0.0), W1), x1 = (int)fmin(fmax(ceil(fmax(ua, ub)) + 1.0, -1.0), W1 - 1.0);
      y0 = (int)fmin(fmax(floor(fmin(va, vb)) - 1.0, 0.0), H1), y1 = (int)fmin(fmax(ceil(fmax(va, vb)) + 1.0, -1.0), H1 - 1.0);
    }
    d.x0 = x0, d.x1 = x1, d.y0 = y0, d.y1 = y1;
  }
  __syncthreads();

  const int px = blockIdx.x * 64 + threadIdx.x, py = blockIdx.y * 4 + threadIdx.y;
  if (px >= k.W || py >= k.H) return;
  // where the view sits in the tiled [n_tiled, 2H, 2W, .] tensors: image tile / 4, row (tile % 4) / 2, column tile % 2 (genima_amd/tiling.py)
  const bool tiled_io = k.bg_tiled || k.full_f16 || k.rnd_f16;
  long tpix = 0;
  if (tiled_io) {
    const int tile = k.tile_index ? k.tile_index[view] : view;
    if (tile < 0 || tile >= 4 * k.n_tiled) return;  // a bad index writes nothing
    tpix = (((long)(tile >> 2) * 2 + ((tile >> 1) & 1)) * k.H + py) * (2L * k.W) + (long)(tile & 1) * k.W + px;
  }
  const long pix = ((long)view * k.H + py) * k.W + px;

  bool near = false;
  for (int s = 0; s < n; ++s) near |= px >= sph[s].x0 && px <= sph[s].x1 && py >= sph[s].y0 && py <= sph[s].y1;
  uint8_t r8 = 255, g8 = 255, b8 = 255;
  if (near) {
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    const int ns = k.samples;
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
  const bool white = r8 == 255 && g8 == 255 && b8 == 255;  // render_data.py keys on the COLOUR, not on coverage
  if (k.occupied) k.occupied[pix] = white ? 0 : 1;

  const long bpix = (k.bg_tiled ? tpix : pix) * 3;
  if (k.full || k.full_f16) {
    uint8_t fr = r8, fg = g8, fb = b8;
    if (white) {
      // bg_frames: the tiled frames lie anywhere on the device (the DataLoader's frame cache), one pointer per tiled image
      const uint8_t* __restrict__ bgp = k.bg_frames ? k.bg_frames[tpix / (4L * k.H * k.W)] + (tpix % (4L * k.H * k.W)) * 3 : k.bg + bpix;
      fr = bgp[0], fg = bgp[1], fb = bgp[2];
    }
    if (k.full) k.full[pix * 3] = fr, k.full[pix * 3 + 1] = fg, k.full[pix * 3 + 2] = fb;
    if (k.full_f16) store_f16_pixel(k.full_f16 + tpix * 8, fr, fg, fb, k.full_mul, k.full_add);
  }
  if (k.rnd || k.rnd_f16) {
    uint8_t tr = k.bg2[bpix], tg = k.bg2[bpix + 1], tb = k.bg2[bpix + 2];
    if (!white) {
      const double bl = k.blend[view], om = 1.0 - bl;
      tr = blend_u8(r8, tr, bl, om), tg = blend_u8(g8, tg, bl, om), tb = blend_u8(b8, tb, bl, om);
    }
    if (k.rnd) k.rnd[pix * 3] = tr, k.rnd[pix * 3 + 1] = tg, k.rnd[pix * 3 + 2] = tb;
    if (k.rnd_f16) store_f16_pixel(k.rnd_f16 + tpix * 8, tr, tg, tb, k.rnd_mul, k.rnd_add);
  }
}

}  // namespace

extern "C" int32_t gn_render_spheres(gn_ctx* ctx, const gn_render_desc* d) {
  GN_REQUIRE(ctx && d, "gn_render_spheres: null context or descriptor");
  GN_REQUIRE(d->B > 0 && d->B <= 65535 && d->S > 0 && d->S <= MAX_SPHERES && d->H > 0 && d->W > 0, "gn_render_spheres: bad B / S / H / W (S <= %d)", MAX_SPHERES);
  GN_REQUIRE(d->samples == 1 || d->samples == 4, "gn_render_spheres: samples must be 1 or 4");
  GN_REQUIRE(d->cams && d->spheres && d->tex_index && d->count && d->atlas && d->T > 0 && d->th > 0 && d->tw > 0, "gn_render_spheres: missing inputs");
  GN_REQUIRE(((uintptr_t)d->atlas & 3) == 0, "gn_render_spheres: atlas must be 4-byte aligned");
  const bool want_full = d->full || d->full_f16, want_rnd = d->rnd || d->rnd_f16;
  GN_REQUIRE(want_full || want_rnd || d->occupied, "gn_render_spheres: no output requested");
  GN_REQUIRE(!want_full || d->bg || d->bg_frames, "gn_render_spheres: full needs bg (or bg_frames)");
  GN_REQUIRE(!d->bg_frames || d->bg_tiled, "gn_render_spheres: bg_frames are tiled frames (bg_tiled)");
  GN_REQUIRE(!want_rnd || (d->bg2 && d->blend), "gn_render_spheres: rnd needs bg2 and blend");
  const bool tiled = d->bg_tiled || d->full_f16 || d->rnd_f16;
  GN_REQUIRE(!tiled || (d->n_tiled > 0 && (d->tile_index || d->B <= 4 * (int64_t)d->n_tiled)), "gn_render_spheres: tiled tensors need n_tiled >= B / 4 (or tile_index)");
  GN_REQUIRE((((uintptr_t)d->full_f16 | (uintptr_t)d->rnd_f16) & 15) == 0, "gn_render_spheres: f16 outputs must be 16-byte aligned");
  KParams k;
  k.cams = d->cams, k.spheres = d->spheres, k.tex_index = d->tex_index, k.count = d->count, k.atlas = d->atlas;
  k.bg = d->bg, k.bg2 = d->bg2, k.blend = d->blend, k.tile_index = d->tile_index, k.bg_frames = d->bg_frames;
  k.full = d->full, k.rnd = d->rnd, k.occupied = d->occupied, k.full_f16 = (f16*)d->full_f16, k.rnd_f16 = (f16*)d->rnd_f16;
  k.S = d->S, k.H = d->H, k.W = d->W, k.T = d->T, k.th = d->th, k.tw = d->tw, k.samples = d->samples, k.bg_tiled = d->bg_tiled, k.n_tiled = d->n_tiled;
  k.full_mul = d->full_mul, k.full_add = d->full_add, k.rnd_mul = d->rnd_mul, k.rnd_add = d->rnd_add;
  hipLaunchKernelGGL(render_spheres_kernel, dim3((d->W + 63) / 64, (d->H + 3) / 4, d->B), dim3(64, 4), 0, ctx->stream, k);
  GN_LAUNCH_CHECK();
  return GN_OK;
}
