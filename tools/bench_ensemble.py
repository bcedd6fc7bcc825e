"""B = 1 controller call (full-size ACT, ``act_tiled`` on a 512 x 512 tile) with and without the action-ensemble op
(``GenimaACT.set_execution(5, True)``), alternating in one process: 9 blocks of 60 individually synchronised calls per setting, the op-less
call as baseline; then the op alone (HIP events around a replay of that one op of the recorded program).

    python tools/bench_ensemble.py [--out profiles/ensemble_b1_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from genima_amd import configs, weights
from genima_amd.act import GenimaACT

fam = configs.family("sd-turbo")
ccfg = dict(configs.TINY_ACT_CLIP_TEXT, projection_dim=512)
agent = GenimaACT(fam["act"], None, ccfg, None, device="cuda", seed=0)
B = 1
tiled = torch.from_numpy(weights.counter_bytes(9, "act", B * 512 * 512 * 3).reshape(B, 512, 512, 3)).cuda()
state = torch.randn(B, 1, fam["act"]["state_dim"], generator=torch.Generator().manual_seed(7)).cuda()
Vc = ccfg["vocab_size"]
toks = torch.zeros(B, 1, 77, dtype=torch.int32)
toks[:, 0, :5] = torch.tensor([Vc - 2, 5, 6, 7, Vc - 1], dtype=torch.int32)

def block(n, step0):
    ts = []
    for i in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.act_tiled(tiled, state, toks, step=step0 + 5 * i)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)

res = {"off": [], "on": []}
for mode in ("off", "on"):  # record + warm both programs
    agent.set_execution(5, True) if mode == "on" else agent.set_execution()
    block(10, 0)
for r in range(9):
    for mode in ("off", "on"):
        agent.set_execution(5, True) if mode == "on" else agent.set_execution()
        block(3, 0)
        res[mode].append(block(60, 15))
out = {m: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), blocks=v) for m, v in res.items()}
out["delta_us"] = (out["on"]["median_ms"] - out["off"]["median_ms"]) * 1e3
# the op alone, from the recorded program (HIP events around a replay of its one op)
io = [p for p in agent._progs.values() if p.exec is not None][0]
E = io.engine
e0, e1 = E.event(), E.event()
n = E.num_ops
one = []
for _ in range(50):
    E.event_record(e0); E.run(n - 1, n); E.event_record(e1)
    one.append(E.event_elapsed_ms(e0, e1) * 1e3)
out["op_alone_us_median"] = statistics.median(one)
out["ops"] = n
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ensemble_b1_timing.json"))
args = ap.parse_args()
out["device"] = torch.cuda.get_device_name(0)
out["what"] = "GenimaACT.act_tiled, B = 1, full-size ACT, ms per synchronised call: medians of 9 alternating blocks of 60 calls; op_alone: one op replayed between HIP events"
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps({k: v for k, v in out.items() if k not in ("off", "on")}), {m: (out[m]["median_ms"], out[m]["min_ms"], out[m]["max_ms"]) for m in ("off", "on")})
