"""The DataLoader's frame cache and decode workers (genima_amd/data.py) without a GPU: cached and fanned-out loaders yield the batches of the
plain loader, every file is decoded once within the budget and on every use beyond it, and decoding errors still reach the consumer."""
import os
import pickle
import random

import numpy as np
import pytest
import torch
from PIL import Image

from genima_amd import data as D
from genima_amd.pipeline import HashTokenizer

R = 16
FRAME = R * R * 3


def _tree(root):
    """One task, 3 episodes x (8 + 1) frames: 24 tiled examples, 48 distinct files.  Episode 0 is stored at R x R (no resize), the others
    larger and not square (Resize + CenterCrop run)."""
    rng = np.random.RandomState(0)
    base = os.path.join(root, "open_box", "variation0")
    os.makedirs(os.path.join(base, "episodes"))
    with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
        pickle.dump(["open the box"], f)
    for e, size in enumerate(((R, R), (24, 40), (33, 20))):
        for kind in ("rgb", "rgb_rendered"):
            d = os.path.join(base, "episodes", f"episode{e}", kind)
            os.makedirs(d)
            for i in range(9):
                Image.fromarray(rng.randint(0, 256, size + (3,), dtype=np.uint8)).save(os.path.join(d, f"{i}.png"))
    return D.RLBenchDataset(root, tasks="open_box", num_demos=3)


def _epochs(loader, n=3, seed=11):
    random.seed(seed)  # tokenize_captions draws from python's global stream (proportion_empty_prompts)
    return [[{k: v.clone() for k, v in b.items()} for b in loader] for _ in range(n)]


def _assert_same(got, want):
    assert len(got) == len(want)
    for eg, ew in zip(got, want):
        assert len(eg) == len(ew)
        for bg, bw in zip(eg, ew):
            assert set(bg) == set(bw) == {"pixel_values_u8", "conditioning_pixel_values_u8", "input_ids"}
            for k in bw:
                assert bg[k].dtype == bw[k].dtype and torch.equal(bg[k], bw[k]), k


@pytest.fixture()
def count_decodes(monkeypatch):
    calls = []
    real = D.resize_center_crop_u8

    def counting(im, resolution):
        calls.append(resolution)
        return real(im, resolution)
    monkeypatch.setattr(D, "resize_center_crop_u8", counting)
    return calls


@pytest.mark.parametrize("world,rank,pep", [(1, 0, 0.0), (2, 0, 0.0), (2, 1, 0.0), (1, 0, 0.5)])
def test_host_cache_yields_the_uncached_batches(tmp_path, world, rank, pep):
    ds = _tree(str(tmp_path))
    assert len(ds) == 24
    tok = HashTokenizer(1024)
    kw = dict(seed=3, rank=rank, world=world, proportion_empty_prompts=pep)
    # 24 examples in batches of 5: a partial last batch at world 1, a wrap-around tail (30 slots for 24 examples) at world 2
    want = _epochs(D.DataLoader(ds, 5, tok, R, **kw))
    cached = D.DataLoader(ds, 5, tok, R, cache="host", **kw)
    _assert_same(_epochs(cached), want)
    assert [b["input_ids"].shape[0] for b in want[0]] == ([5, 5, 5, 5, 4] if world == 1 else [5, 5, 5])
    assert len(cached) == len(want[0]) and cached.cache.hits > 0
    if pep:
        empty = tok([""], max_length=tok.model_max_length, padding="max_length", truncation=True, return_tensors="pt").input_ids[0]
        rows = [r for e in want for b in e for r in b["input_ids"]]
        n_empty = sum(bool(torch.equal(r, empty)) for r in rows)
        assert 0 < n_empty < len(rows)  # the draw happened, and the cached loader reproduced it row for row (above)


@pytest.mark.parametrize("cache", [None, "host"])
def test_decode_workers_yield_the_same_batches(tmp_path, cache):
    ds = _tree(str(tmp_path))
    tok = HashTokenizer(1024)
    kw = dict(seed=5, proportion_empty_prompts=0.5, cache=cache)
    want = _epochs(D.DataLoader(ds, 5, tok, R, decode_workers=1, **kw))
    fan = D.DataLoader(ds, 5, tok, R, decode_workers=4, **kw)
    assert fan.decode_workers == 4 and D.DataLoader(ds, 5, tok, R, decode_workers=1000).decode_workers == 16
    _assert_same(_epochs(fan), want)
    _assert_same(_epochs(D.DataLoader(ds, 5, tok, R, decode_workers=4, prefetch=0, **kw)), want)


def test_every_file_is_decoded_once_within_the_budget(tmp_path, count_decodes):
    ds = _tree(str(tmp_path))
    tok = HashTokenizer(1024)
    want = _epochs(D.DataLoader(ds, 5, tok, R, seed=3))
    assert len(count_decodes) == 3 * 48  # no cache: every use decodes
    del count_decodes[:]
    for world, n_files in ((1, 48), (2, 48)):  # world 2: both ranks share one cache, the wrapped tail repeats frames
        cache = D.FrameCache("host", cache_bytes=48 * FRAME, chunk_bytes=10 * FRAME)  # five chunks, the last one cut to 8 frames
        loaders = [D.DataLoader(ds, 5, tok, R, seed=3, rank=r, world=world, cache=cache) for r in range(world)]
        got = [_epochs(ld) for ld in loaders]
        if world == 1:
            _assert_same(got[0], want)
        assert len(count_decodes) == n_files == len(cache) == cache.decodes
        assert cache.nbytes == 48 * FRAME == cache.allocated_bytes <= cache.cache_bytes
        del count_decodes[:]
        cache.clear()
        assert len(cache) == 0 and cache.nbytes == 0 and cache.hits == cache.misses == cache.decodes == 0


def test_a_file_used_in_both_roles_is_stored_once(tmp_path, count_decodes):
    ds = _tree(str(tmp_path))
    for e in ds.examples:
        e["conditioning_image"] = e["image"]
    tok = HashTokenizer(1024)
    ld = D.DataLoader(ds, 5, tok, R, seed=3, cache="host")
    for b in ld:
        assert torch.equal(b["pixel_values_u8"], b["conditioning_pixel_values_u8"])
    assert len(ld.cache) == 24 == len(count_decodes)


def test_budget_of_n_frames_caches_n_and_decodes_the_rest_every_time(tmp_path, count_decodes):
    ds = _tree(str(tmp_path))
    tok = HashTokenizer(1024)
    want = _epochs(D.DataLoader(ds, 5, tok, R, seed=3))
    del count_decodes[:]
    N = 13
    ld = D.DataLoader(ds, 5, tok, R, seed=3, cache="host", cache_bytes=N * FRAME + FRAME // 2)
    _assert_same(_epochs(ld), want)
    assert len(ld.cache) == N and ld.cache.nbytes == N * FRAME <= ld.cache.cache_bytes
    # N files once, the other 48 - N in each of the three epochs
    assert len(count_decodes) == N + 3 * (48 - N) == ld.cache.decodes
    assert ld.cache.hits == 2 * N


def test_device_cache_batches_name_slots_without_touching_a_device(tmp_path, count_decodes):
    """The producer's half of cache="device" needs no GPU: slots, pending uploads and staging frames are host data."""
    ds = _tree(str(tmp_path))
    tok = HashTokenizer(1024)
    N = 20
    ld = D.DataLoader(ds, 4, tok, R, seed=3, cache="device", cache_bytes=N * FRAME, prefetch=0)
    want = [b for b in D.DataLoader(ds, 4, tok, R, seed=3, prefetch=0)]
    seen = {}
    for b, w in zip(ld, want):
        assert b["frame_slots"].shape == (8, 2) and b["frame_slots"].dtype == torch.int64 and torch.equal(b["input_ids"], w["input_ids"])
        flat = torch.cat([w["pixel_values_u8"], w["conditioning_pixel_values_u8"]])
        pending = {(c, i): t for c, i, t in b["frame_uploads"]}
        for (c, i), frame in zip(b["frame_slots"].tolist(), flat):
            if c < 0:
                assert torch.equal(b["frame_staging_u8"][i], frame)
            else:
                seen.setdefault((c, i), pending.get((c, i)))
                assert seen[(c, i)] is not None and torch.equal(seen[(c, i)], frame)  # nothing was uploaded, so every slot is still pending
    assert len(ld.cache) == N == len(seen) and len(count_decodes) == 48 + 48


def test_a_truncated_png_still_surfaces_in_the_consumer(tmp_path):
    ds = _tree(str(tmp_path))
    tok = HashTokenizer(1024)
    bad = ds.examples[7]["image"]
    with open(bad, "rb") as f:
        head = f.read()[:60]
    with open(bad, "wb") as f:
        f.write(head)
    for kw in (dict(), dict(cache="host"), dict(cache="host", decode_workers=4), dict(cache="device", prefetch=0), dict(decode_workers=4)):
        ld = D.DataLoader(ds, 5, tok, R, seed=3, shuffle=False, **kw)
        with pytest.raises(Exception) as ei:
            for _ in ld:
                pass
        assert not isinstance(ei.value, (AssertionError, KeyError, AttributeError)), ei.value
        if ld.cache is not None:  # the failed batch gave its slots back: nothing half-filled stays addressable
            assert all(os.path.exists(k[0]) and k[0] != bad for k in ld.cache._index)
            assert len(ld.cache) == 10  # the first batch's 5 + 5 frames
