"""-m gpu: the device frame cache of the training DataLoader -- ``gn_gather_u8_to_f16`` against ``gn_image_u8_to_f16`` bit for bit, its
argument checks, ``to_device`` on device-cache batches (all misses, all hits, over the budget) against the uncached batches, and a
ControlNet fine-tune fed from the cache against one fed without it."""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

from genima_amd import configs, schema, weights
from genima_amd import data as D
from genima_amd.pipeline import HashTokenizer

pytestmark = pytest.mark.gpu


def _frames_in_chunks(n, pixels, seed, offset=0):
    """n random uint8 [pixels, 3] frames spread over three separately allocated device 'chunks' at 4-byte aligned strides (+ offset)."""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (n, pixels, 3), generator=g, dtype=torch.uint8)
    k = min(256, pixels)
    frames[0, :k, 0] = torch.arange(k, dtype=torch.uint8)  # every byte value at least once (pixels >= 256)
    stride = (pixels * 3 + 3) // 4 * 4
    chunks = [torch.zeros(offset + stride * n, dtype=torch.uint8, device="cuda") for _ in range(3)]
    addr = []
    for i in range(n):
        c, k = chunks[i % 3], (i * 7) % n  # scattered: neither chunk nor slot follows the batch order
        c[offset + k * stride: offset + k * stride + pixels * 3] = frames[i].reshape(-1).cuda()
        addr.append(c.data_ptr() + offset + k * stride)
    return frames, chunks, addr


@pytest.mark.parametrize("mul,add", [(2.0, -1.0), (1.0, 0.0)])
@pytest.mark.parametrize("cpad", [8, 4])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("pixels", [999, 4100, 1030])  # 999 = 3 mod 4 and under one block of 1024; 4100: five blocks, the last partial; 1030 = 2 mod 4
def test_gather_is_bit_equal_to_image_u8_to_f16(engine, mul, add, cpad, B, pixels):
    frames, chunks, addr = _frames_in_chunks(B, pixels, seed=B * 10000 + pixels)
    order = list(range(B))
    if B > 1:
        order[-1] = order[0]  # a repeated pointer (the data-parallel tail wraps round)
    ptrs = torch.tensor([addr[i] for i in order], dtype=torch.int64).cuda()
    got = engine.gather_u8_to_f16(ptrs, (pixels, 1), cpad, mul, add)
    want = engine.image_u8_to_f16(frames[order].reshape(B, pixels, 1, 3).cuda(), cpad, mul, add)
    assert got.shape == want.shape == (B, pixels, 1, cpad) and got.dtype == torch.float16
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert float(got[..., 3:].abs().max()) == 0.0


def test_gather_reads_a_frame_that_is_not_dword_aligned(engine):
    frames, chunks, addr = _frames_in_chunks(3, 1030, seed=5, offset=1)
    got = engine.gather_u8_to_f16(torch.tensor(addr, dtype=torch.int64).cuda(), (1030, 1), 8, 2.0, -1.0)
    want = engine.image_u8_to_f16(frames.reshape(3, 1030, 1, 3).cuda(), 8, 2.0, -1.0)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_gather_rejects_bad_arguments_without_launching(engine):
    frames, chunks, addr = _frames_in_chunks(2, 64, seed=1)
    ptrs = torch.tensor(addr, dtype=torch.int64).cuda()
    out = torch.full((2 * 64 * 8 + 8,), 7.0, dtype=torch.float16, device="cuda")
    call = lambda src, o, B, px, cpad: int(engine.lib.gn_gather_u8_to_f16(engine._ctx, src, o, B, px, cpad, 1.0, 0.0))  # noqa: E731
    p, o = ptrs.data_ptr(), out.data_ptr()
    for args in ((None, o, 2, 64, 8), (p, None, 2, 64, 8), (p, o, 0, 64, 8), (p, o, -1, 64, 8), (p, o, 70000, 64, 8), (p, o, 2, 0, 8),
                 (p, o, 2, 64, 2), (p, o, 2, 64, 9), (p, o + 2, 2, 64, 8)):
        assert call(*args) != 0, args
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(p, o, 2, 64, 8) == 0  # ... and the good call goes through
    torch.cuda.synchronize()
    assert bool((out[:2 * 64 * 8] != 7.0).all()) and bool((out[2 * 64 * 8:] == 7.0).all())


def _tree(root, n_eps=2, n_frames=7, size=(96, 80)):
    rng = np.random.RandomState(1)
    base = os.path.join(root, "open_box", "variation0")
    os.makedirs(os.path.join(base, "episodes"))
    with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
        pickle.dump(["open the box"], f)
    for e in range(n_eps):
        for kind in ("rgb", "rgb_rendered"):
            d = os.path.join(base, "episodes", f"episode{e}", kind)
            os.makedirs(d)
            for i in range(n_frames):
                Image.fromarray(rng.randint(0, 256, size + (3,), dtype=np.uint8)).save(os.path.join(d, f"{i}.png"))
    return D.RLBenchDataset(root, tasks="open_box", num_demos=n_eps)


def _same(a, b):
    assert set(a) == set(b) == {"pixel_values", "conditioning_pixel_values", "input_ids"}
    for k in ("pixel_values", "conditioning_pixel_values"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype == torch.float16 and a[k].is_cuda
        assert torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k
    assert torch.equal(a["input_ids"], b["input_ids"])


@pytest.mark.parametrize("world,rank,n_examples,bs", [(1, 0, 12, 5), (2, 1, 3, 4)])
def test_to_device_on_cache_batches_equals_the_uncached_batches(engine, tmp_path, world, rank, n_examples, bs):
    ds = _tree(str(tmp_path))  # 12 examples, 24 files
    # world 2: 3 examples in batches of 4 on 2 ranks -- 8 slots, so the wrapped tail names the same frame twice within a batch
    del ds.examples[n_examples:]
    tok, R = HashTokenizer(1024), 64
    fb = R * R * 3
    kw = dict(seed=2, rank=rank, world=world, shuffle=world == 1)
    plain = D.DataLoader(ds, bs, tok, R, **kw)
    cached = D.DataLoader(ds, bs, tok, R, cache=D.FrameCache("device", cache_bytes=64 * fb, chunk_bytes=5 * fb), **kw)  # frames in several chunks
    n_files = 2 * n_examples
    for epoch in range(3):
        before = cached.cache.decodes
        for hb, cb in zip(plain, cached):
            assert "frame_slots" in cb and "pixel_values_u8" not in cb
            if world == 2:
                assert len({tuple(s) for s in cb["frame_slots"].tolist()}) < 2 * bs  # a repeated frame
            _same(D.to_device(engine, cb), D.to_device(engine, hb))
        # epoch 1: every file misses once; afterwards everything is gathered from the device chunks
        assert cached.cache.decodes - before == (n_files if epoch == 0 else 0)
    assert len(cached.cache) == n_files and len(cached.cache._chunks[R]) == (n_files + 4) // 5 and not cached.cache._pending
    assert all(c.is_cuda for c in cached.cache._chunks[R])


def test_to_device_over_the_budget_mixes_hits_uploads_and_staging(engine, tmp_path):
    ds = _tree(str(tmp_path))
    tok, R = HashTokenizer(1024), 64
    fb = R * R * 3
    plain = D.DataLoader(ds, 4, tok, R, seed=4)
    cached = D.DataLoader(ds, 4, tok, R, seed=4, cache="device", cache_bytes=9 * fb + 100)  # 9 of 24 files fit
    staged_beside_uploads = staged_beside_hits = False
    for epoch in range(2):
        for hb, cb in zip(plain, cached):
            staged = int((cb["frame_slots"][:, 0] < 0).sum())
            staged_beside_uploads |= staged > 0 and len(cb["frame_uploads"]) > 0
            staged_beside_hits |= staged > 0 and epoch == 1 and staged < 8
            assert (cb["frame_staging_u8"] is None) == (staged == 0)
            _same(D.to_device(engine, cb), D.to_device(engine, hb))
    assert len(cached.cache) == 9 and cached.cache.nbytes == 9 * fb <= cached.cache.cache_bytes
    assert cached.cache.decodes == 9 + 2 * 15 and cached.cache.hits == 9
    assert staged_beside_uploads and staged_beside_hits


def test_trainer_fed_from_the_device_cache_reproduces_the_uncached_losses(engine, tmp_path, monkeypatch):
    from genima_amd.packing import pack_state_dict
    from genima_amd.scheduler import DDPMScheduler
    from genima_amd.training import ControlNetTrainer

    ds = _tree(str(tmp_path), n_eps=2, n_frames=4, size=(300, 300))  # 6 examples
    fam = configs.family("tiny")
    tok = HashTokenizer(fam["text"]["vocab_size"])
    calls = []
    real = D.resize_center_crop_u8
    monkeypatch.setattr(D, "resize_center_crop_u8", lambda im, res: (calls.append(res), real(im, res))[1])

    def run(**kw):
        synth = lambda sch, s: weights.synth_state_dict(sch, s)  # noqa: E731
        tr = ControlNetTrainer(engine, fam["unet"], fam["controlnet"], pack_state_dict(synth(schema.unet_schema(fam["unet"]), 1), "cuda"),
                               synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-4)
        tr.attach_frozen(fam["vae"], pack_state_dict(synth(schema.vae_schema(fam["vae"]), 3), "cuda"), fam["text"],
                         pack_state_dict(synth(schema.clip_text_schema(fam["text"]), 4), "cuda"), DDPMScheduler(), seed=5,
                         augmentations="crop,colorjitter")
        loader = D.DataLoader(ds, 2, tok, 256, shuffle=True, seed=0, **kw)
        losses, decodes = [], []
        for _ in range(2):
            n0 = len(calls)
            for batch in loader:
                losses.append(float(tr.train_step(batch)))
            decodes.append(len(calls) - n0)
        return losses, decodes

    want, d0 = run()
    got, d1 = run(cache="device")
    assert d0 == [12, 12] and d1 == [12, 0]  # the cached loader decodes nothing in epoch 2
    assert len(want) == 6 and all(np.isfinite(want)) and len(set(want)) > 1
    assert got == want, (got, want)  # bit-identical loss sequences
