"""Micro-benchmark of the patch-resident 3x3 conv with fused GroupNorm-apply + SiLU (csrc/conv_gn.hip) against the gn_groupnorm_fwd +
gn_gemm launches it replaces, on the VAE decoder's shapes at B = 8 tiled 512^2 (run on the GPU box).

`python tools/bench_conv_gn.py patch [out.txt]`: the race of the 64-channel-group patch conv (csrc/conv_patch.hip) against the
GroupNorm launch + the tune table's gn_gemm on the UNet / ControlNet ResNet conv shapes at B = 8 (64 x 64 -> 320 and 32 x 32 -> 640 channels,
concatenated inputs as their two sources), the contenders alternating in one process; the table decides engine.CONV_PATCH_SHAPES."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd._lib import ACT_SILU  # noqa: E402
from genima_amd.engine import Engine  # noqa: E402

E = Engine("cuda:0", autotune=True)
B = int(os.environ.get("B", "8"))


def timeit(fn, iters=10):
    for _ in range(3):
        fn()
    a, e = E.event(), E.event()
    E.event_record(a)
    for _ in range(iters):
        fn()
    E.event_record(e)
    return E.event_elapsed_ms(a, e) / iters * 1000.0


def race_patch(out_path=None):
    """name, H, C1, C2, Cout: conv1 / conv2 of the encoder blocks, conv1 of the up blocks (skip concat)."""
    shapes = [(64, 320, 0, 320), (64, 320, 320, 320), (64, 640, 320, 320), (32, 640, 0, 640), (32, 320, 0, 640), (32, 640, 640, 640), (32, 1280, 640, 640),
              (32, 640, 320, 640)]
    lines = [f"# B={B}; us per launch, median of 5 rounds of 20, contenders alternating; gn = GroupNorm+SiLU launch, st = statistics-only GroupNorm,",
             "# gemm = gn_gemm (tune table) on the normalised tensor, p = gn_conv3x3_patch on the same tensor, pgn = gn_conv3x3_patch on the raw",
             "# tensor(s) with GroupNorm + SiLU inside the patch",
             "# HxW Cin(C1+C2)->Cout | gn gemm gn+gemm | p p/gemm | st pgn st+pgn (st+pgn)/(gn+gemm)"]
    for H, C1, C2, Cout in shapes:
        Cin = C1 + C2
        x = torch.randn(B, H, H, C1, device="cuda").half()
        x2 = torch.randn(B, H, H, C2, device="cuda").half() if C2 else None
        w = (torch.randn(Cout, 9 * Cin, device="cuda") * (9 * Cin) ** -0.5).half()
        bias, gamma, beta = torch.randn(Cout, device="cuda").half(), torch.ones(Cin, device="cuda").half(), torch.zeros(Cin, device="cuda").half()
        shift = torch.randn(B, 4 * Cout, device="cuda").half()[:, Cout:2 * Cout]
        n = torch.empty(B, H, H, Cin, device="cuda", dtype=torch.float16)
        y0, y1 = (torch.empty(B, H, H, Cout, device="cuda", dtype=torch.float16) for _ in range(2))
        st = E.groupnorm_stats(x, gamma, beta, 32, 1e-5, x2=x2)
        fns = {"gn": lambda: E.groupnorm(x, gamma, beta, 32, 1e-5, act=ACT_SILU, x2=x2, out=n),
               "gemm": lambda: E.conv2d(n, w, bias, shift=shift, ldshift=4 * Cout, out=y0),
               "st": lambda: E.groupnorm_stats(x, gamma, beta, 32, 1e-5, x2=x2),
               "pgn": lambda: E.conv2d_patch(x, st, w, bias, x2=x2, shift=shift, ldshift=4 * Cout, out=y1),
               "p": lambda: E.conv2d_patch(n, None, w, bias, shift=shift, ldshift=4 * Cout, act=0, out=y1)}
        t = {k: [] for k in fns}
        for _ in range(5):
            for k, fn in fns.items():
                t[k].append(timeit(fn, iters=20))
        m = {k: sorted(v)[2] for k, v in t.items()}
        fl = 2.0 * B * H * H * Cout * 9 * Cin
        lines.append(f"{H}x{H} {Cin}({C1}+{C2})->{Cout} | {m['gn']:6.1f} {m['gemm']:7.1f} ({fl / m['gemm'] / 1e6:5.0f} TF/s) {m['gn'] + m['gemm']:7.1f} | {m['p']:7.1f} "
                     f"({fl / m['p'] / 1e6:5.0f} TF/s) {m['p'] / m['gemm']:5.3f}x | {m['st']:6.1f} {m['pgn']:7.1f} {m['st'] + m['pgn']:7.1f} {(m['st'] + m['pgn']) / (m['gn'] + m['gemm']):5.3f}x")
        print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if len(sys.argv) > 1 and sys.argv[1] == "patch":
    race_patch(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)

for H, Cin, Cout in [tuple(int(v) for v in t.split("x")) for t in os.environ.get("SHAPES", "512x128x8,512x128x128,512x256x128,256x256x256,256x512x256,128x512x512,64x512x512,64x384x384").split(",")]:
    x = torch.randn(B, H, H, Cin, device="cuda").half()
    w = (torch.randn(Cout, 9 * Cin, device="cuda") * (9 * Cin) ** -0.5).half()
    bias, gamma, beta = torch.randn(Cout, device="cuda").half(), torch.ones(Cin, device="cuda").half(), torch.zeros(Cin, device="cuda").half()
    n, y0, y1 = torch.empty_like(x), torch.empty(B, H, H, Cout, device="cuda", dtype=torch.float16), torch.empty(B, H, H, Cout, device="cuda", dtype=torch.float16)
    st = E.groupnorm_stats(x, gamma, beta, 32, 1e-6)
    fl = 2.0 * B * H * H * Cout * 9 * Cin
    t_gn = timeit(lambda: E.groupnorm(x, gamma, beta, 32, 1e-6, act=ACT_SILU, out=n))
    t_cv = timeit(lambda: E.conv2d(n, w, bias, out=y0))
    t_st = timeit(lambda: E.groupnorm_stats(x, gamma, beta, 32, 1e-6))
    t_fu = timeit(lambda: E.conv2d_gn(x, st, w, bias, out=y1))
    t_pl = timeit(lambda: E.conv2d_gn(x, None, w, bias, act=0, out=y1))
    print(f"B={B} {H}x{H} {Cin}->{Cout}: GN {t_gn:7.1f} + conv {t_cv:7.1f} ({fl / t_cv / 1e6:6.1f} TF/s) = {t_gn + t_cv:7.1f} us | stats {t_st:6.1f} + conv_gn {t_fu:7.1f} "
          f"({fl / t_fu / 1e6:6.1f} TF/s) = {t_st + t_fu:7.1f} us | patch conv without GN {t_pl:7.1f} us", flush=True)
