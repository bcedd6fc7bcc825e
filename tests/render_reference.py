"""A numpy restatement of the sphere renderer's arithmetic (include/genima_hip.h: gn_render_spheres) and of the reference's composite
(render/render_data.py:282-307), written from the reference's two files and the kernel's contract, not from the kernel: world-space rays,
one sphere at a time, float64 throughout.  The intersection is written through the foot of the perpendicular (dist^2 first, then the
depth), because the exclusion rule is stated on dist^2 and the float32 run of the same statements needs a form without the quadratic's
cancellation; the kernel uses the same textbook form in eye space, so what pins geometry, orientation and depth order independently
are the known answers of tests/test_render_cpu.py.  ``dtype=np.float32`` runs the same statements in single precision -- what any f32
implementation may legitimately differ by -- and ``exclusion`` marks the pixels where that difference can change a decision."""
import numpy as np

SAMPLE_OFFSETS = {1: ((0.5, 0.5),), 4: ((0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875))}
EXCLUDE_REL = 1e-4  # |dist^2 - r^2| <= EXCLUDE_REL r^2 (silhouette) or a bilinear coordinate within EXCLUDE_REL texels of a texel centre


def render(cam, spheres, tex_index, count, atlas, H, W, samples=4, dtype=np.float64):
    """cam [18], spheres [S, 16], tex_index [S], count, atlas uint8 [T, th, tw, 4] (the kernel's packed inputs, any float type) ->
    (uint8 [H, W, 3] render, white where nothing was drawn; bool [H, W] exclusion mask)."""
    f = dtype
    cam = np.asarray(cam).astype(f)
    fx, fy, cx, cy = cam[:4]
    pose = cam[4:16].reshape(3, 4)
    R, o = pose[:, :3], pose[:, 3]
    znear, zfar = cam[16], cam[17]
    th, tw = atlas.shape[1:3]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    acc = np.zeros((H, W, 3), f)
    excluded = np.zeros((H, W), bool)
    for ox, oy in SAMPLE_OFFSETS[samples]:
        u, v = xs.astype(f) + f(ox), ys.astype(f) + f(oy)
        de = np.stack([(u - cx) / fx, (cy - v) / fy, -np.ones_like(u)], -1)  # camera looks down -z, y up; signed fx, fy
        d = de @ R.T
        a = (d * d).sum(-1)
        best_t = np.full((H, W), np.inf, f)
        colour = np.ones((H, W, 3), f)  # a miss is white
        texel_edge = np.zeros((H, W), bool)
        for s in range(int(count)):
            sp = np.asarray(spheres[s]).astype(f)
            Ps = sp[:12].reshape(3, 4)
            Rs, c, r, factor = Ps[:, :3], Ps[:, 3], sp[12], sp[13:16]
            oc = c - o
            q = (d * oc).sum(-1) / a
            perp = oc - q[..., None] * d
            dist2 = (perp * perp).sum(-1)
            excluded |= np.abs(dist2 - r * r) <= f(EXCLUDE_REL) * r * r
            disc = r * r - dist2
            t = q - np.sqrt(np.maximum(disc, 0) / a)  # the front intersection; dz = -1 in eye space, so t is the eye depth -z
            hit = (disc >= 0) & (t > 0) & (t >= znear) & (t <= zfar) & (t < best_t)
            p = ((o + t[..., None] * d) - c) @ Rs  # Rs^T (hit - c)
            uu, vv = (p[..., 0] / r + 1) / 2, (p[..., 1] / r + 1) / 2
            x, y = uu * tw - f(0.5), vv * th - f(0.5)  # y counts rows from the texture's bottom row
            x0, y0 = np.floor(x), np.floor(y)
            wx, wy = (x - x0)[..., None], (y - y0)[..., None]
            i0, i1 = x0.astype(np.int64) % tw, (x0.astype(np.int64) + 1) % tw
            j0, j1 = th - 1 - y0.astype(np.int64) % th, th - 1 - (y0.astype(np.int64) + 1) % th
            T = atlas[int(tex_index[s])][..., :3].astype(f)
            texel = (T[j0, i0] * (1 - wx) + T[j0, i1] * wx) * (1 - wy) + (T[j1, i0] * (1 - wx) + T[j1, i1] * wx) * wy
            colour = np.where(hit[..., None], factor * texel / f(255), colour)
            edge = (np.abs(x - np.rint(x)) <= EXCLUDE_REL) | (np.abs(y - np.rint(y)) <= EXCLUDE_REL)
            texel_edge = np.where(hit, edge, texel_edge)
            best_t = np.where(hit, t, best_t)
        excluded |= texel_edge
        acc += colour
    img = np.clip(np.rint(f(255) * (acc / f(samples))), 0, 255).astype(np.uint8)
    return img, excluded


def composite(render_u8, rgb, texture=None, blend=None):
    """render_data.py:282-307, literally: -> (full, rnd or None, occupied)."""
    render_u8 = np.array(render_u8)
    render_rnd_bg = np.array(render_u8)
    white_space = np.all(render_u8 == [255, 255, 255], axis=-1)
    occupied_space = np.any(render_u8 != [255, 255, 255], axis=-1)
    render_u8[white_space] = rgb[white_space]
    if texture is None:
        return render_u8, None, occupied_space
    render_rnd_bg[white_space] = texture[white_space]
    render_rnd_bg[occupied_space] = render_rnd_bg[occupied_space] * blend + texture[occupied_space] * (1 - blend)
    return render_u8, render_rnd_bg, occupied_space


def scene(seed, B=8, H=256, W=256, scales=(3.0, 8.0, 6.5, 6.5, 6.5), radius=0.01, S=4, flip_sign=True):
    """The GPU test's views: render.yaml's geometry (256^2, the five camera scales, radius 0.01, znear 1e-5, zfar 3), random camera poses,
    1-4 spheres per view placed in front of the camera 0.3-1.5 m away inside the frustum, random sphere orientations, every texture used.
    RLBench-style negative fx / fy on every second view.  -> the packed kernel inputs (numpy)."""
    rng = np.random.RandomState(seed)

    def rot():
        q = rng.randn(4)
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    cams, sph = np.zeros((B, 18), np.float32), np.zeros((B, S, 16), np.float32)
    tex, count = np.zeros((B, S), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        fl = 0.5 * W / np.tan(np.radians(rng.uniform(20, 35)))
        sign = -1.0 if (flip_sign and b % 2) else 1.0
        Rc, oc = rot(), rng.uniform(-1, 1, 3)
        cams[b, :4] = (sign * fl, sign * fl, W / 2 + rng.uniform(-3, 3), H / 2 + rng.uniform(-3, 3))
        cams[b, 4:16] = np.concatenate([Rc, oc[:, None]], 1).reshape(-1)
        cams[b, 16:] = (1e-5, 3.0)
        count[b] = 1 + (b + seed) % 4
        for s in range(count[b]):
            depth = rng.uniform(0.3, 1.5)
            e = np.array([rng.uniform(-0.8, 0.8) * depth * (W / 2) / fl, rng.uniform(-0.8, 0.8) * depth * (H / 2) / fl, -depth])
            sph[b, s, :12] = np.concatenate([rot(), (Rc @ e + oc)[:, None]], 1).reshape(-1)
            sph[b, s, 12] = radius * scales[(b + s) % len(scales)]
            sph[b, s, 13:] = (0.60392156862, 0.86274509803, 1.0) if (b + s) % 3 else (1.0, 1.0, 0.0)
            tex[b, s] = (b * S + s) % 5
    return {"cams": cams, "spheres": sph, "tex_index": tex, "count": count}
