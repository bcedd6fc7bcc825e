"""-m gpu: every Engine method that can record, op by op -- the recorded launch (``Engine(record=True)`` + ``run()``) against the eager launch of
the same arguments, bit for bit.  A recorded op carries its arguments from ``gn_program_add_*`` to the replay; an argument that arrives in
another position, or through a narrower type, changes the bytes, so every case below keeps the arguments of its op distinct from their
neighbours (C != C2, ld != C, sigma != sigma_next, four different sizes, ...).  Then the same ops as ONE program (stream replay, then
hipGraph capture + launch), a fork / main / join section against the same ops without the markers, and a recorded op the launch refuses.

Nothing here has a tolerance: both sides run the same kernel on the same inputs."""
import pytest
import torch

from genima_amd import _lib
from genima_amd._lib import ACT_GELU, ACT_SILU, GenimaHipError
from genima_amd.engine import Engine

pytestmark = pytest.mark.gpu

F16, F32, I32, U8 = torch.float16, torch.float32, torch.int32, torch.uint8


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _h(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=_g(seed)) * scale).to(F16).cuda()


def _u8(*shape, seed):
    return torch.randint(0, 256, shape, generator=_g(seed), dtype=torch.int32).to(U8).cuda()


class Case:
    """``build()`` -> the input tensors (made once per session); ``emit(E, t, name)`` -> the op's outputs on engine E.  ``mutable``: the inputs
    the op writes (in-place ops, an explicit destination, the ensemble's state) -- every engine gets its own copy, restored between replays."""

    def __init__(self, build, emit, mutable=()):
        self.build, self.emit, self.mutable = build, emit, tuple(mutable)


def _ensemble_case(dtype):
    B, T, A, ld, K, h = 2, 6, 5, 8, 4, 3  # A < ld, h < T, K > 1 (>= ceil(T / h)), all six different

    def build():
        chunk = (torch.rand(B, T, ld, generator=_g(60)) * 4.0 - 2.0).to(dtype)
        chunk[..., A:] = 1000.0  # pad columns: an average that read them would show
        return dict(chunk=chunk.cuda(), steps=torch.tensor([3, 10], dtype=I32).cuda(), reset=torch.tensor([0, 1], dtype=U8).cuda(),
                    state=torch.zeros(int(_lib.load().gn_action_ensemble_state_bytes(B, T, A, K)), dtype=U8, device="cuda"))

    def emit(E, t, name):
        out = E.action_ensemble(t["chunk"], t["state"], t["steps"], t["reset"], h, K, 0.02, A=A, name=name)
        return [out, t["state"]]

    return Case(build, emit, mutable=("state",))


def _copy4d_emit(E, t, name):
    # 2 x 3 x 4 x 5 runs of 8 elements, gathered from one spread layout into another (offsets = 8 * (i0 + 2 i1 + 6 i2 + 24 i3): disjoint)
    return [E.copy4d(t["src"], t["dst"], (2, 3, 4, 5), (960, 320, 80, 16), (8, 16, 48, 192), 8)]


def _film_emit(E, t, name):
    fb = t["fb"]  # gamma | beta | unused columns of one [2, 48] feature buffer: ld_film 48 != C 16
    return [E.film(t["x"], fb[:, :16], fb[:, 16:32], 3, ACT_SILU, name=name)]  # rows 6, rows_per_film 3


def _attention_build():
    B, heads, Nq, Nk, D = 2, 2, 40, 24, 64
    v = _h(B, Nk, heads * D, seed=52)
    vt = torch.zeros(B, heads * D, 64, dtype=F16, device="cuda")
    vt[:, :, :Nk] = v.transpose(1, 2)
    return dict(q=_h(B, Nq, heads * D, seed=50), k=_h(B, Nk, heads * D, seed=51), vt=vt)


CASES = {
    "timestep_embedding": Case(lambda: dict(t=torch.tensor([1.0, 250.5, 999.0]).cuda()),
                               lambda E, t, name: [E.timestep_embedding(t["t"], 16, True, 0.5, name=name)]),
    "scale_pad": Case(lambda: dict(x=_h(5, 6, seed=1)), lambda E, t, name: [E.scale_pad(t["x"], 0.37, 16, name=name)]),
    # C 5 of ld1 12, C2 3 of ld2 20, Cpad 16 > C + C2
    "scale_cat_pad": Case(lambda: dict(x=_h(7, 12, seed=2), x2=_h(7, 20, seed=3)),
                          lambda E, t, name: [E.scale_cat_pad(t["x"], 5, t["x2"], 3, 16, 0.5, -1.75, name=name)]),
    "euler_step": Case(lambda: dict(x=_h(9, 4, seed=4), eps=_h(9, 8, seed=5)),  # C 4, ld_eps 8
                       lambda E, t, name: [E.euler_step(t["x"], t["eps"], 2.5, 1.25)], mutable=("x",)),
    "add_noise": Case(lambda: dict(x0=_h(3, 40, seed=6), noise=_h(3, 40, seed=7), a=torch.tensor([0.9, 0.5, 0.1]).cuda(),
                                   b=torch.tensor([0.2, 0.6, 0.95]).cuda()),
                      lambda E, t, name: [E.add_noise(t["x0"], t["noise"], t["a"], t["b"], name=name)]),
    "image_u8_to_f16": Case(lambda: dict(img=_u8(2, 5, 3, 3, seed=8)), lambda E, t, name: [E.image_u8_to_f16(t["img"], 8, 2.0, -1.0, name=name)]),
    "image_f16_to_u8": Case(lambda: dict(x=_h(2, 5, 3, 8, seed=9)), lambda E, t, name: [E.image_f16_to_u8(t["x"], name=name)]),
    "image_normalize_u8": Case(lambda: dict(img=_u8(2, 5, 3, 3, seed=10)),
                               lambda E, t, name: [E.image_normalize_u8(t["img"], (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 8, name=name)]),
    "add": Case(lambda: dict(a=_h(104, seed=11), b=_h(104, seed=12)), lambda E, t, name: [E.add(t["a"], t["b"], name=name)]),
    "add_multi": Case(lambda: dict(a0=_h(8, seed=13), b0=_h(8, seed=14), a1=_h(24, seed=15), b1=_h(24, seed=16), a2=_h(40, seed=17), b2=_h(40, seed=18)),
                      lambda E, t, name: E.add_multi([(t["a0"], t["b0"]), (t["a1"], t["b1"]), (t["a2"], t["b2"])], name=name)),
    "act": Case(lambda: dict(x=_h(48, seed=19)), lambda E, t, name: [E.act(t["x"], ACT_GELU, name=name)]),
    "film": Case(lambda: dict(x=_h(6, 16, seed=20), fb=_h(2, 48, seed=21)), _film_emit),
    "embedding": Case(lambda: dict(ids=torch.tensor([[4, 0, 10], [7, 7, 2]], dtype=I32).cuda(), tok=_h(11, 8, seed=22), pos=_h(3, 8, seed=23)),
                      lambda E, t, name: [E.embedding(t["ids"], t["tok"], t["pos"], name=name)]),  # B 2, L 3, D 8
    "softmax_rows": Case(lambda: dict(x=_h(5, 24, seed=24)),  # 16 columns of rows 24 wide: ld != cols
                         lambda E, t, name: [E.softmax_rows(t["x"][:, :16], 0.7), t["x"]], mutable=("x",)),
    "gather_rows": Case(lambda: dict(x=_h(2, 3, 8, seed=25), idx=torch.tensor([2, 1], dtype=I32).cuda()),
                        lambda E, t, name: [E.gather_rows(t["x"], t["idx"], name=name)]),
    "argmax_rows": Case(lambda: dict(x=torch.randint(-50, 50, (5, 7), generator=_g(26), dtype=I32).cuda()),
                        lambda E, t, name: [E.argmax_rows(t["x"], name=name)]),
    "copy4d": Case(lambda: dict(src=_h(2048, seed=27), dst=torch.zeros(1024, dtype=F16, device="cuda")), _copy4d_emit, mutable=("dst",)),
    "maxpool3x3s2": Case(lambda: dict(x=_h(2, 5, 7, 8, seed=28)), lambda E, t, name: [E.maxpool3x3s2(t["x"], name=name)]),
    "layernorm": Case(lambda: dict(x=_h(5, 24, seed=29), g=_h(24, seed=30), b=_h(24, seed=31)),
                      lambda E, t, name: [E.layernorm(t["x"], t["g"], t["b"], 1e-3, name=name)]),
    "tiny_block": Case(lambda: dict(x=_h(1, 5, 7, 64, seed=32), **{f"w{k}": _h(64, 576, seed=33 + k, scale=576 ** -0.5) for k in range(3)},
                                    **{f"b{k}": _h(64, seed=36 + k) for k in range(3)}),
                       lambda E, t, name: [E.tiny_block(t["x"], [t["w0"], t["w1"], t["w2"]], [t["b0"], t["b1"], t["b2"]], name=name)]),
    "action_ensemble": _ensemble_case(F32),
    "action_ensemble_f16": _ensemble_case(F16),
    "linear": Case(lambda: dict(x=_h(10, 64, seed=40), w=_h(24, 64, seed=41, scale=0.125), b=_h(24, seed=42)),
                   lambda E, t, name: [E.linear(t["x"], t["w"], t["b"], act=ACT_SILU, name=name)]),
    "groupnorm": Case(lambda: dict(x=_h(2, 35, 32, seed=43), g=_h(32, seed=44), b=_h(32, seed=45)),
                      lambda E, t, name: [E.groupnorm(t["x"], t["g"], t["b"], 4, 1e-5, act=ACT_SILU, name=name)]),
    "attention": Case(_attention_build, lambda E, t, name: [E.attention(t["q"], t["k"], t["vt"], 2, Nk=24, name=name)]),
}

_built = {}


def _inputs(name):
    """The case's inputs, built once and left unchanged: engines get clones of what the op writes."""
    if name not in _built:
        _built[name] = CASES[name].build()
    return _built[name]


def _own(name):
    base = _inputs(name)
    return {k: (v.clone() if k in CASES[name].mutable else v) for k, v in base.items()}


def _engine(record):
    E = Engine("cuda:0", record=record)
    E.autotune = False  # both sides take the tune table's plan (or the library's heuristic) for the one Linear: no race at record time
    return E


def _same(got, want, what):
    assert len(got) == len(want) and len(got) > 0, what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        assert torch.equal(a, b), f"{what}: output {i} differs ({int((a != b).sum())} of {a.numel()} elements)"


@pytest.mark.parametrize("name", list(CASES))
def test_recorded_op_equals_eager_op(name):
    case = CASES[name]
    E, R = _engine(False), _engine(True)
    eager = case.emit(E, _own(name), name)
    E.synchronize()
    rec = case.emit(R, _own(name), name)
    assert R.num_ops == 1 == len(R.meta), "one Engine call records one op"
    R.run()
    R.synchronize()
    _same(rec, eager, name)


def test_one_program_replays_the_same_by_stream_and_by_graph():
    """All the ops above in one program: ``run()``, then ``capture()`` + ``launch()`` from restored inputs and scrubbed outputs."""
    side = torch.cuda.Stream()
    R = _engine(True)
    R.use_stream(side)
    with torch.cuda.stream(side):
        owned = {name: _own(name) for name in CASES}
        per_case = {name: case.emit(R, owned[name], name) for name, case in CASES.items()}
        assert R.num_ops == len(CASES) == len(R.meta)
        outs = [o for v in per_case.values() for o in v]
        mutable = [(owned[name][k], _inputs(name)[k]) for name, case in CASES.items() for k in case.mutable]
        R.run()
        side.synchronize()
        first = {name: [o.clone() for o in v] for name, v in per_case.items()}
        for mine, base in mutable:  # what the ops wrote in place goes back to its first value (the ensemble states: zero) ...
            mine.copy_(base)
        in_place = {mine.data_ptr() for mine, _ in mutable}
        for o in outs:  # ... and every other output is scrubbed: the launch has to write it again
            if o.data_ptr() not in in_place:
                o.zero_()
        R.capture()
        R.launch()
        side.synchronize()
        _same(outs, [o for v in first.values() for o in v], "hipGraph launch vs stream replay")
        assert R.last_run_ops == len(CASES)
    E = _engine(False)
    for name, case in CASES.items():  # and both were what the eager ops give
        _same(first[name], case.emit(E, _own(name), name), f"program vs eager: {name}")


def test_fork_main_join_section_gives_the_same_bytes():
    a, b, x = _inputs("add")["a"], _inputs("add")["b"], _inputs("act")["x"]
    side = torch.cuda.Stream()
    got = {}
    for markers in (True, False):
        R = _engine(True)
        R.use_stream(side)
        with torch.cuda.stream(side):
            if markers:
                R.fork()
            s = R.add(a, b, name="s")
            if markers:
                R.main()
            y = R.act(x, ACT_GELU, name="y")
            if markers:
                R.join()
            assert R.num_ops == (5 if markers else 2) == len(R.meta), "a stream marker is one op of the list"
            R.run()
            side.synchronize()
            assert R.last_run_ops == 2, "markers are not kernel ops"
            got[markers] = [s.clone(), y.clone()]
    _same(got[True], got[False], "fork / main / join vs plain")
    E = _engine(False)
    _same(got[True], [E.add(a, b), E.act(x, ACT_GELU)], "fork / main / join vs eager")


def test_refused_op_names_its_index_and_leaves_the_program_usable():
    """gn_softmax_rows refuses 12 columns on the host (a multiple of 8 is required) and launches nothing: the replay stops there, the error
    names op 1, and explicit ranges over the good ops still run."""
    a, b, x = _inputs("add")["a"], _inputs("add")["b"], _inputs("act")["x"]
    R = _engine(True)
    s = R.add(a, b, name="s")
    bad = torch.zeros(4, 12, dtype=F16, device="cuda")
    R.softmax_rows(bad, 1.0)
    y = R.act(x, ACT_GELU, name="y")
    y.zero_()
    with pytest.raises(GenimaHipError, match=r"\bop 1\b.*gn_softmax_rows"):
        R.run()
    R.synchronize()
    assert not bool(y.any()), "nothing behind the refused op ran"
    s.zero_()
    R.run(0, 1)
    R.run(2, 3)
    R.synchronize()
    E = _engine(False)
    _same([s, y], [E.add(a, b), E.act(x, ACT_GELU)], "ranges around the refused op")
    with pytest.raises(GenimaHipError, match=r"\bop 1\b"):
        R.run()
