"""-m gpu: guarded segments of a recorded program (gn_program_begin_segment / end_segment / set_segment_enabled): the prompt-only work (text
tower + cross-attention K / V) and the record-time constants (time shifts) are replayed once per prompt / once per program.  Everything here
compares against the unguarded program (GN_HOIST=0) bit for bit: the same kernels write the same buffers, only less often."""
import numpy as np
import pytest
import torch

from genima_amd import configs, weights
from genima_amd._lib import GenimaHipError
from genima_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _ids(V, B, variant):
    """[B, 77] int32 prompt ids: variant 0 / 1 = two different prompts, 2 = prompt 0 with ONE row of the batch changed."""
    ids = torch.zeros(B, 77, dtype=torch.int32)
    base = 320 if variant != 1 else 400
    ids[:, :14] = torch.tensor([V - 2] + [base + i for i in range(12)] + [V - 1], dtype=torch.int32)
    if variant == 2:
        ids[B - 1, 3] = 17
    return ids


# same prompt x3, a different prompt, the first prompt again, then a change in one row only of a B > 1 batch
SEQUENCE = (0, 0, 0, 1, 0, 2)


def _kernel_ops(E):
    return sum(1 for m in E.meta if m["kind"] != "stream")


def _run_sequence(pipe, B, HW, steps, lat, img, device_ids, output_type, seq):
    """-> (per-call outputs, per-call kernel ops issued, the program)."""
    V = pipe.text_encoder.config["vocab_size"]
    outs, issued = [], []
    for variant in seq:
        ids = _ids(V, B, variant)
        if device_ids:
            ids = ids.cuda()
        out = pipe(prompt_ids=ids, image=img, latents=lat, num_inference_steps=steps, guidance_scale=0.0, output_type=output_type).images
        outs.append(out.cpu().numpy())
        issued.append(pipe.program(B, HW, HW, steps).engine.last_run_ops)
    return outs, issued, pipe.program(B, HW, HW, steps)


def _both_settings(monkeypatch, pipe, B, HW, steps, graph, device_ids, seq=SEQUENCE):
    img = torch.from_numpy(weights.counter_bytes(3, "ctrl", B * HW * HW * 3).reshape(B, HW, HW, 3))
    lat = torch.randn(B, 4, HW // 8, HW // 8, generator=torch.Generator().manual_seed(2)).half()
    res = {}
    for hoist in ("1", "0"):
        monkeypatch.setenv("GN_HOIST", hoist)
        pipe.enable_hip_graph(graph)  # (drops the recorded programs: the next call records with this setting)
        res[hoist] = {ot: _run_sequence(pipe, B, HW, steps, lat, img, device_ids, ot, seq) for ot in ("pt", "latent")}
    return res


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("device_ids", [False, True])
def test_tiny_sequence_is_bit_equal_and_skips(monkeypatch, graph, device_ids):
    from genima_amd.pipeline import StableDiffusionControlNetPipeline

    pipe = StableDiffusionControlNetPipeline.from_synthetic(configs.family("tiny"), seed=20)
    pipe.to("cuda")
    B, HW, steps = 2, 128, 3
    res = _both_settings(monkeypatch, pipe, B, HW, steps, graph, device_ids)
    for ot in ("pt", "latent"):
        on, off = res["1"][ot][0], res["0"][ot][0]
        for i, (a, b) in enumerate(zip(on, off)):
            assert np.array_equal(a, b), f"{ot} of call {i} differs between GN_HOIST=1 and 0"
        assert not np.array_equal(on[2], on[3]), "the second prompt must give another image (else this test proves nothing)"
        assert not np.array_equal(on[4], on[5]), "one changed row must change the output"
    # proof that skips happen: kernel ops issued per call
    _, issued, io = res["1"]["pt"]
    E = io.engine
    full, p, c = _kernel_ops(E), E.segments["prompt"]["kernel_ops"], E.segments["constants"]["kernel_ops"]
    assert p > 10 and c >= 8, (p, c)
    first = full - c if graph else full  # under hipGraph the constants ran with the warm-up replay in front of the capture
    assert issued == [first, full - p - c, full - p - c, full - c, full - c, full - c], (issued, full, p, c)
    # GN_HOIST=0: every call replays everything; the recorded program itself is the same
    _, issued0, io0 = res["0"]["pt"]
    assert issued0 == [full] * len(SEQUENCE)
    assert io0.engine.num_ops == E.num_ops
    assert [(m["kind"], m.get("shape")) for m in io0.engine.meta] == [(m["kind"], m.get("shape")) for m in E.meta]
    assert all(s["enabled"] for s in E.segments.values()), "the wrapper leaves every segment enabled for direct replays"


def test_explicit_range_ignores_the_flags():
    from genima_amd.pipeline import StableDiffusionControlNetPipeline

    pipe = StableDiffusionControlNetPipeline.from_synthetic(configs.family("tiny"), seed=20)
    pipe.to("cuda")
    B, HW, steps = 1, 128, 2
    V = pipe.text_encoder.config["vocab_size"]
    img = torch.from_numpy(weights.counter_bytes(3, "ctrl", B * HW * HW * 3).reshape(B, HW, HW, 3))
    pipe(prompt_ids=_ids(V, B, 0), image=img, num_inference_steps=steps, guidance_scale=0.0, output_type="pt")
    io = pipe.program(B, HW, HW, steps)
    E = io.engine
    seg = E.segments["prompt"]
    i = seg["first"]
    assert E.meta[i]["kind"] == "embedding"
    emb = E.buffers["clip/emb"]
    want = emb.clone()
    n_ops, full = E.num_ops, _kernel_ops(E)
    E.set_segment("prompt", False)
    emb.zero_()
    E.run()  # full replay: the segment is skipped, the zeroed buffer stays as it is
    E.synchronize()
    assert E.last_run_ops == full - seg["kernel_ops"]
    assert not emb.any()
    E.run(i, i + 1)  # an explicit range runs what it names
    E.synchronize()
    assert torch.equal(emb, want)
    assert E.last_run_ops == full - seg["kernel_ops"], "a partial replay does not touch the full-replay counter"
    E.run(0, E.num_ops)  # the whole program named explicitly: every op
    E.set_segment("prompt", True)
    E.run()
    E.synchronize()
    assert E.last_run_ops == full and E.num_ops == n_ops


def test_liveness_assertion_fires_on_an_aliased_buffer():
    E = Engine("cuda", record=True)
    x = torch.zeros(4, 16, 8, dtype=torch.float16, device="cuda")
    with E.segment("s"):
        E.scale_pad(x, 1.0, 8, name="kept")
    E.scale_pad(x, 1.0, 8, name="other")  # another buffer: fine
    with pytest.raises(GenimaHipError, match="segment 's'"):
        E.scale_pad(x, 2.0, 8, name="kept")  # the same named buffer, rewritten by an op outside the segment
    E2 = Engine("cuda", record=True)
    E2.scale_pad(x, 1.0, 8, name="early")
    with pytest.raises(GenimaHipError, match="outside it writes"):
        with E2.segment("s"):
            E2.scale_pad(x, 2.0, 8, name="early")  # the op in front would run again and the skipped segment would not restore it
    with pytest.raises(GenimaHipError, match="do not nest"):
        with E2.segment("a"):
            with E2.segment("b"):
                pass


def test_bytes_changed_entry_point():
    E = Engine("cuda", record=True)
    for n in (77, 2 * 77, 8 * 77, 4):  # 308 bytes = 19 x 16 + a 12-byte tail
        live = torch.arange(n, dtype=torch.int32, device="cuda")
        key = f"k{n}"
        assert E.changed(live, key) is True, "the first comparison has nothing to compare with"
        assert E.changed(live, key) is False
        live[n - 1] += 1  # the last word (in the tail where there is one)
        assert E.changed(live, key) is True
        assert E.changed(live, key) is False, "the snapshot is brought up to date by the comparing pass"
        live[0] = -5
        assert E.changed(live, key) is True
        E.forget(key)
        assert E.changed(live, key) is True


def test_act_tiled_sequence_is_bit_equal(monkeypatch):
    from genima_amd.act import GenimaACT

    fam = configs.family("tiny")
    B = 2
    Vc = fam["act_text"]["vocab_size"]
    tiled = torch.from_numpy(weights.counter_bytes(9, "act", B * 128 * 128 * 3).reshape(B, 128, 128, 3)).cuda()
    state = torch.randn(B, 1, fam["act"]["state_dim"], generator=torch.Generator().manual_seed(7)).cuda()

    def toks(variant):
        t = torch.zeros(B, 1, 77, dtype=torch.int32)
        t[:, 0, :5] = torch.tensor([Vc - 2, 5 + variant, 6, 7, Vc - 1], dtype=torch.int32)
        return t

    for device_tokens in (False, True):
        res = {}
        for hoist in ("1", "0"):
            monkeypatch.setenv("GN_HOIST", hoist)
            agent = GenimaACT(fam["act"], None, fam["act_text"], None, device="cuda", seed=0)
            outs, issued = [], []
            for variant in (0, 0, 0, 1, 0):
                t = toks(variant).cuda() if device_tokens else toks(variant)
                a = agent.act_tiled(tiled, state, t)
                outs.append(a.float().cpu().numpy())
                issued.append(next(iter(agent._progs.values())).engine.last_run_ops)
            res[hoist] = (outs, issued, next(iter(agent._progs.values())).engine)
        for i, (a, b) in enumerate(zip(res["1"][0], res["0"][0])):
            assert np.array_equal(a, b), f"actions of call {i} differ between GN_HOIST=1 and 0"
        assert not np.array_equal(res["1"][0][2], res["1"][0][3]), "other tokens must give other actions"
        E = res["1"][2]
        full, t_ops = _kernel_ops(E), E.segments["task_text"]["kernel_ops"]
        assert t_ops > 10
        assert res["1"][1] == [full, full - t_ops, full - t_ops, full, full], (res["1"][1], full, t_ops)
        assert res["0"][1] == [full] * 5


def test_changed_controlnet_weights_run_the_segments_again():
    """load_state_dict re-packs (a new pack generation, so a new program whose segments all run); the validation path builds its pipeline
    around the live modules with another ControlNet.  Either way a call with an unchanged prompt equals a freshly built pipeline's."""
    from genima_amd.host import ControlNetModel
    from genima_amd.pipeline import StableDiffusionControlNetPipeline
    from genima_amd.validation import validation_pipeline

    fam = configs.family("tiny")
    B, HW, steps = 1, 128, 2
    img = torch.from_numpy(weights.counter_bytes(3, "ctrl", B * HW * HW * 3).reshape(B, HW, HW, 3))
    lat = torch.randn(B, 4, HW // 8, HW // 8, generator=torch.Generator().manual_seed(2)).half()

    def call(p, ids):
        return p(prompt_ids=ids, image=img, latents=lat, num_inference_steps=steps, guidance_scale=0.0, output_type="pt").images.cpu().numpy()

    pipe = StableDiffusionControlNetPipeline.from_synthetic(fam, seed=20)
    pipe.to("cuda")
    ids = _ids(pipe.text_encoder.config["vocab_size"], B, 0)
    a0 = call(pipe, ids)
    assert np.array_equal(a0, call(pipe, ids))
    sd = pipe.controlnet.state_dict()
    g = torch.Generator().manual_seed(5)
    new = {k: (v + 0.05 * torch.randn(v.shape, generator=g) if (".attn2.to_k." in k or ".attn2.to_v." in k or "time_emb_proj" in k) else v)
           for k, v in sd.items()}
    pipe.controlnet.load_state_dict(new)
    a1 = call(pipe, ids)  # same prompt, new K / V and time-shift weights
    fresh = StableDiffusionControlNetPipeline.from_synthetic(fam, seed=20)
    fresh.controlnet.load_state_dict(new)
    fresh.to("cuda")
    want = call(fresh, ids)
    assert np.array_equal(a1, want)
    assert not np.array_equal(a0, a1), "the changed weights must show in the output"
    # in-place edits of packed weights have no generation to bump: weights_changed() runs every segment again
    io = pipe.program(B, HW, HW, steps)
    call(pipe, ids)
    pipe.weights_changed()
    call(pipe, ids)
    assert io.engine.last_run_ops == _kernel_ops(io.engine)
    # trainer -> validation: a pipeline around the live modules, one ControlNet after the other, same prompt
    for cn_sd in (sd, new):
        vp = validation_pipeline(pipe.vae, pipe.text_encoder, pipe.tokenizer, pipe.unet, ControlNetModel(fam["controlnet"], cn_sd), "euler_discrete")
        ref = validation_pipeline(fresh.vae, fresh.text_encoder, fresh.tokenizer, fresh.unet, ControlNetModel(fam["controlnet"], cn_sd), "euler_discrete")
        for _ in range(2):
            assert np.array_equal(call(vp, ids), call(ref, ids))


@pytest.mark.parametrize("graph", [False, True])
def test_sd_turbo_single_b1_is_bit_equal(monkeypatch, graph):
    from genima_amd.pipeline import StableDiffusionControlNetPipeline

    pipe = StableDiffusionControlNetPipeline.from_synthetic(configs.family("sd-turbo"), seed=0, gen_device=torch.device("cuda"))
    pipe.to("cuda")
    for m in (pipe.vae, pipe.text_encoder, pipe.unet, pipe.controlnet):
        m._sd = None
    res = _both_settings(monkeypatch, pipe, 1, 256, 5, graph, True, seq=SEQUENCE[:5])
    for ot in ("pt", "latent"):
        for i, (a, b) in enumerate(zip(res["1"][ot][0], res["0"][ot][0])):
            assert np.array_equal(a, b), f"{ot} of call {i} differs between GN_HOIST=1 and 0"
    _, issued, io = res["1"]["pt"]
    E = io.engine
    full, p, c = _kernel_ops(E), E.segments["prompt"]["kernel_ops"], E.segments["constants"]["kernel_ops"]
    assert issued[1] == full - p - c and issued[3] == full - c, (issued, full, p, c)
