"""The host half of ``DataLoader(view_augment=...)``, no device: ``perturb.sample_tables`` and ``perturb.draw(rng=)``, and the loader's
draw key over a hand-made tree (``tiled_rgb`` PNGs written with PIL plus ``save_traj``): a sample's tables depend on (seed, epoch, dataset
index) and on nothing else."""
import os
import pickle

import numpy as np
import pytest
from PIL import Image

from genima_amd import data as D
from genima_amd import perturb as P
from genima_amd import render as R
from genima_amd.pipeline import HashTokenizer

TEXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sphere_textures")
NAMES = ["wrist", "front", "right_shoulder", "left_shoulder"]
BOTH = P.parse("camera_pose+light_color")
EYE = np.eye(3).reshape(9)


def _cams(seed=3):
    """Four plausible f32 camera rows: RLBench's negative focal lengths, a rotation each."""
    rng = np.random.default_rng(seed)
    cams = np.zeros((4, 18), np.float32)
    for v in range(4):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cams[v, :4] = (-351.6, -351.6, 128.0, 128.0)
        cams[v, 4:16] = np.concatenate([q, rng.normal(size=(3, 1))], axis=1).reshape(-1)
        cams[v, 16:] = (1e-5, 3.0)
    return cams


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_sample_tables_repeats_for_a_key_and_differs_between_keys_and_epochs():
    cams = _cams()
    a, b = P.sample_tables(BOTH, cams, NAMES, (4, 1, 7)), P.sample_tables(BOTH, cams, NAMES, (4, 1, 7))
    assert a[3] is True and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:3], b[:3]))
    assert a[0].dtype == np.float32 and a[0].shape == (4, 18) and a[1].dtype == np.float64 and a[1].shape == (4, 9) and a[2].shape == (4, 6)
    for key in ((4, 1, 8), (4, 2, 7), (5, 1, 7)):  # another sample, another epoch, another seed
        c = P.sample_tables(BOTH, cams, NAMES, key)
        assert not np.array_equal(a[1], c[1]) and not np.array_equal(a[2], c[2]) and not np.array_equal(a[0], c[0]), key
    assert np.array_equal(_bits(a[1]), _bits(P.homography(cams, a[0])))
    assert (a[2] == a[2][0]).all() and (a[2][0, :3] >= 0.5).all() and (a[2][0, :3] <= 1.0).all() and not a[2][0, 3:].any()  # one light for the four views
    assert not np.array_equal(_bits(cams), _bits(a[0])) and np.array_equal(cams, _cams()), "the input table was written"


def test_the_wrist_keeps_its_bits_and_the_exact_identity_under_camera_pose():
    cams = _cams()
    cams[0, 5] = -0.0  # a negative zero survives
    new, M, colour, applied = P.sample_tables(P.parse("camera_pose"), cams, NAMES, (0, 0, 0))
    assert applied and np.array_equal(_bits(new[0]), _bits(cams[0])) and np.array_equal(_bits(M[0]), _bits(EYE))
    for v in (1, 2, 3):
        assert not np.array_equal(new[v], cams[v]) and not np.array_equal(M[v], EYE)
        assert np.array_equal(_bits(new[v, [0, 1, 2, 3, 7, 11, 15, 16, 17]]), _bits(cams[v, [0, 1, 2, 3, 7, 11, 15, 16, 17]]))  # the centre stays: a pure turn
    assert np.array_equal(colour, np.tile([[1.0, 1, 1, 0, 0, 0]], (4, 1)))


def test_prob_zero_gives_identities_and_consumes_the_same_first_draw():
    cams = _cams()
    new, M, colour, applied = P.sample_tables(BOTH, cams, NAMES, (1, 2, 3), prob=0.0)
    assert applied is False and np.array_equal(_bits(new), _bits(cams)) and new is not cams
    assert np.array_equal(_bits(M), _bits(np.tile(EYE, (4, 1)))) and np.array_equal(colour, np.tile([[1.0, 1, 1, 0, 0, 0]], (4, 1)))
    # the coin is drawn first whatever prob is: a prob just above the coin applies exactly what prob = 1 applies
    coin = np.random.default_rng([1, 2, 3]).random()
    full = P.sample_tables(BOTH, cams, NAMES, (1, 2, 3), prob=1.0)
    above, below = P.sample_tables(BOTH, cams, NAMES, (1, 2, 3), prob=np.nextafter(coin, 1.0)), P.sample_tables(BOTH, cams, NAMES, (1, 2, 3), prob=coin)
    assert above[3] is True and below[3] is False
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(full[:3], above[:3]))
    # and the values are draw()'s on the generator that has given the coin
    rng = np.random.default_rng([1, 2, 3])
    rng.random()
    d = P.draw(BOTH, 1, NAMES, rng=rng)
    want = P.perturb_cams(cams, P.rotation(d["pitch"][0], d["yaw"][0], d["roll"][0]), d["zoom"][0], np.stack([d["shift_x"][0], d["shift_y"][0]], axis=-1))
    assert np.array_equal(_bits(full[0]), _bits(np.ascontiguousarray(want))) and np.array_equal(full[2][0], np.concatenate([d["gain"][0], d["offset"][0]]))
    for bad in (dict(prob=1.5), dict(prob=-0.1), dict(key=(1, -2)), dict(key=())):
        with pytest.raises(ValueError):
            P.sample_tables(BOTH, cams, NAMES, **dict(dict(key=(1, 2)), **bad))


def test_draw_without_rng_returns_what_it_returned_before():
    p = P.Perturbation("x", pitch=(-0.1, 0.1), zoom=(0.9, 1.1), shift_x=2.0, cameras=("front",), gain=((0.5, 1.0),) * 3, offset=((-3.0, 3.0),) * 3)
    E, seed = 3, 11
    got = P.draw(p, E, NAMES, seed=seed)
    rng = np.random.default_rng(seed)  # the written order: six camera keys of size (E, V), then gain r g b and offset r g b of size (E,)
    cam = {k: rng.uniform(*getattr(p, k), size=(E, 4)) for k in P.CAMERA_KEYS}
    off = np.array([n != "front" for n in NAMES])
    for k, ident in zip(P.CAMERA_KEYS, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0)):
        cam[k][:, off] = ident
        assert np.array_equal(_bits(got[k]), _bits(cam[k])), k
    gain = np.stack([rng.uniform(lo, hi, size=(E,)) for lo, hi in p.gain], axis=1)
    offset = np.stack([rng.uniform(lo, hi, size=(E,)) for lo, hi in p.offset], axis=1)
    assert np.array_equal(_bits(got["gain"]), _bits(gain)) and np.array_equal(_bits(got["offset"]), _bits(offset))
    again = P.draw(p, E, NAMES, seed=seed, rng=np.random.default_rng(seed))  # a generator given is asked in the same order
    assert all(np.array_equal(_bits(got[k]), _bits(again[k])) for k in got)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """One episode of six steps: constant-colour 512 x 512 ``tiled_rgb`` frames and the synthetic trajectory.  -> (dataset, RenderConfig)."""
    root = str(tmp_path_factory.mktemp("view_augment"))
    cfg, traj, _ = R.synthetic_episode(6, 7, TEXTURES)
    base = os.path.join(root, "open_box", "variation0")
    ep = os.path.join(base, "episodes", "episode0")
    os.makedirs(os.path.join(ep, "tiled_rgb"))
    with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
        pickle.dump(["open the box"], f)
    for ts in range(6):
        Image.fromarray(np.full((512, 512, 3), 20 * ts, np.uint8)).save(os.path.join(ep, "tiled_rgb", f"{ts}.png"))
    R.save_traj(os.path.join(ep, "traj.npz"), traj)
    ds = D.RLBenchDataset(root, tasks="open_box", num_demos=1, image_type="tiled_rgb", conditioning_image_type="tiled_rgb")
    assert len(ds) == 5  # the tiled reader drops the last frame
    return ds, cfg


def _tables(loader, epochs=1):
    """-> per epoch {dataset index: [(M, colour, cams), ...]}: the dataset index of a row is read from the loader's own batches."""
    out = []
    for _ in range(epochs):
        order = [i for ix in loader._batches() for i in ix]
        got, k = {}, 0
        for batch in loader:
            v = batch["render_views"]
            assert v["M"].dtype.is_floating_point and tuple(v["M"].shape[1:]) == (4, 9) and tuple(v["colour"].shape[1:]) == (4, 6)
            assert v["cams"].shape[0] == 4 * v["M"].shape[0]
            for j in range(v["M"].shape[0]):
                got.setdefault(order[k], []).append((v["M"][j].numpy().copy(), v["colour"][j].numpy().copy(), v["cams"][4 * j:4 * j + 4].numpy().copy()))
                k += 1
        assert k == len(order)
        out.append(got)
    return out


def test_loader_refusals(tree):
    ds, cfg = tree
    tok = HashTokenizer(1024)
    with pytest.raises(ValueError, match="no camera to turn and no target to re-draw"):
        D.DataLoader(ds, 2, tok, 512, view_augment="camera_pose")
    src = R.TrajectorySource(cfg)
    for prob in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="view_augment_prob"):
            D.DataLoader(ds, 2, tok, 512, render_targets=src, view_augment="camera_pose", view_augment_prob=prob)
    with pytest.raises(ValueError):
        D.DataLoader(ds, 2, tok, 512, render_targets=src, view_augment="camera:wobble=1")
    assert "M" not in next(iter(D.DataLoader(ds, 2, tok, 512, render_targets=src)))["render_views"]  # off by default


def test_loader_draw_depends_on_seed_epoch_and_index_alone(tree):
    ds, cfg = tree
    tok = HashTokenizer(1024)
    src = R.TrajectorySource(cfg)
    clean = {i: np.stack([v[0] for v in src.views(ds.examples[i]["conditioning_image"])]) for i in range(len(ds))}
    before = {i: [tuple(a.copy() if isinstance(a, np.ndarray) else a for a in v) for v in src.views(ds.examples[i]["conditioning_image"])] for i in range(len(ds))}
    kw = dict(render_targets=src, view_augment=BOTH, seed=3)
    ref = _tables(D.DataLoader(ds, 2, tok, 512, **kw), epochs=2)
    for e, got in enumerate(ref):
        assert sorted(got) == list(range(len(ds)))
        for i, rows in got.items():
            new, M, colour, applied = P.sample_tables(BOTH, clean[i], NAMES, (3, e, i))
            assert applied and np.array_equal(_bits(rows[0][0]), _bits(M)) and np.array_equal(_bits(rows[0][1]), _bits(colour))
            assert np.array_equal(_bits(rows[0][2]), _bits(new))
    assert all(not np.array_equal(ref[0][i][0][0], ref[1][i][0][0]) for i in range(len(ds))), "the epochs repeat each other"
    # another batch size, a prefetching producer, decode workers, a host cache and a separate augmentation seed of the same value
    for other in (dict(batch=3), dict(batch=3, prefetch=0), dict(batch=2, decode_workers=3), dict(batch=2, cache="host"), dict(batch=1, view_augment_seed=3, seed=9)):
        o = dict(kw, **other)
        got = _tables(D.DataLoader(ds, o.pop("batch"), tok, 512, **o))[0]
        for i in range(len(ds)):
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[i][0], ref[0][i][0])), (other, i)
    # two ranks: every sample, the ones the data-parallel tail repeats included, gets the draw it gets alone
    seen = {}
    for rank in (0, 1):
        for i, rows in _tables(D.DataLoader(ds, 2, tok, 512, rank=rank, world=2, **kw))[0].items():
            seen.setdefault(i, []).extend(rows)
    assert sorted(seen) == list(range(len(ds))) and sum(len(r) for r in seen.values()) == 8  # 5 samples completed to 2 ranks x 2 batches x 2
    for i, rows in seen.items():
        for row in rows:
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(row, ref[0][i][0])), i
    assert _tables(D.DataLoader(ds, 2, tok, 512, **dict(kw, view_augment_seed=4)))[0][0][0][0].tolist() != ref[0][0][0][0].tolist()
    # the memoised views are what they were
    for i, views in before.items():
        for a, b in zip(views, src.views(ds.examples[i]["conditioning_image"])):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), i


def test_loader_prob_zero_hands_over_the_clean_tables(tree):
    ds, cfg = tree
    tok = HashTokenizer(1024)
    src = R.TrajectorySource(cfg)
    plain = next(iter(D.DataLoader(ds, 2, tok, 512, render_targets=src, seed=1)))["render_views"]
    off = next(iter(D.DataLoader(ds, 2, tok, 512, render_targets=src, seed=1, view_augment="camera_pose", view_augment_prob=0.0)))["render_views"]
    assert np.array_equal(_bits(off["cams"].numpy()), _bits(plain["cams"].numpy()))
    assert np.array_equal(off["M"].numpy(), np.tile(EYE, (2, 4, 1))) and np.array_equal(off["colour"].numpy(), np.tile([1.0, 1, 1, 0, 0, 0], (2, 4, 1)))
    for k in ("spheres", "tex_index", "count"):
        assert np.array_equal(off[k].numpy(), plain[k].numpy())
