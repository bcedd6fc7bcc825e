// Joint-action sphere renderer (render/joint_marker.py + the composite of render/render_data.py:282-307): an analytic ray-caster for
// the flat-shaded textured spheres the reference draws with pyrender, and the white-keyed composite over the RGB frame / the alpha
// blend over a random texture, in ONE launch per batch of views.  genima_hip.h (gn_render_spheres) states the arithmetic.
//
// Shape: blockIdx.z = view, a block is 64 x 4 pixels (a wave = 64 consecutive pixels of one row: 1 KiB of contiguous 16-byte stores
// on the f16 NHWC-8 output).  The first `count` threads of a block bring the view's spheres into eye space (f64, once per block) and
// leave them in LDS with their bounding rectangles; a pixel outside every rectangle is white without casting a ray.  No scratch, no
// atomics.  Built with -ffp-contract=off: the blend is numpy's unfused f64 multiply / multiply / add, truncated.
#include "render_common.h"

namespace {

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

__global__ __launch_bounds__(256) void render_spheres_kernel(const KParams k) {
  __shared__ SphereLds sph[MAX_SPHERES];
  const int view = blockIdx.z;
  const float* __restrict__ cam = k.cams + (long)view * CAM_FLOATS;
  int n = k.count[view];
  n = n < 0 ? 0 : (n > k.S ? k.S : n);
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if (tid < n) sphere_to_lds(sph[tid], cam, k.spheres + ((long)view * k.S + tid) * SPHERE_FLOATS, k.tex_index[(long)view * k.S + tid], k.T, k.W, k.H);
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

  uint8_t r8, g8, b8;
  shade_pixel(sph, n, SphereAtlas{k.atlas, k.T, k.th, k.tw}, cam, k.samples, px, py, r8, g8, b8);
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
