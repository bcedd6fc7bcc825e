"""In-call tile tuning of the recorded inference programs.

The shipped tile table (genima_amd/gemm_tune_gfx950.json) was filled by ISOLATED races: a shape's candidates run back to back in a hot loop,
operands resident in L2 / MALL, the chip's clock wherever that loop leaves it.  DESIGN.md (round 3) records that such a race does not rank
tiles the way the call does (a re-race flipped 236 entries and made the call slower).  This tool times the candidates where they run:

  for each gn_gemm shape of the recorded program (largest share of the call first)
      shortlist: an isolated race over every valid tile (and K splits of the best two)
      for each shortlisted plan: patch it into EVERY op of that shape (gn_program_set_gemm_plan), replay the whole program op by op
          (cold weights, the producer's output in cache, the neighbours' clock state), sum the HIP-event time of that shape's ops
      keep a challenger only if it beats the incumbent by --margin in two interleaved comparisons

and finally checks the call's wall time before / after; the winners go into the tile table (and gpurun_out/gemm_tune_gfx950.json).
A tile never changes the summation order along K; a changed K split does (deterministically), which the parity tests' tolerances cover.

    python tools/incall_tune.py [--workloads tiled_b8,tiled_b1,single_b1] [--top 40] [--margin 0.03]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (synthetic inputs, workloads)
from genima_amd import configs, engine as engine_mod  # noqa: E402
from genima_amd._lib import GEMM_PP, GEMM_PPP, GEMM_REG, GemmDesc, check, gemm_tiles  # noqa: E402
from genima_amd.engine import ACT_GEGLU, OUT_ROWMAJOR, Engine  # noqa: E402



def gemm_ops(E):
    """-> {tune key: [(op index, desc, on_side)]} of the recorded program."""
    out, side = {}, False
    for i in range(E.num_ops):
        m = E.meta[i]
        if m["kind"] == "stream":
            side = m.get("op") == "fork"
            continue
        d = GemmDesc()
        if E.lib.gn_program_get_gemm(E._prog, i, C.byref(d)) != 0:
            continue
        if d.fp8 or d.up_phases or d.accumulate or d.norm_out.y or d.norm_in.stats or d.sink.stats:  # (round 5: the reduce-side GroupNorm needs a K split,
            continue                                                                            #  the bridge's tails / A path their own tiles: not raced here)
        out.setdefault(Engine._tune_key(d), []).append((i, d, side))
    return out


def valid_plans(d):
    fam = {t: c.family for t, c in gemm_tiles().items()}
    if d.act == ACT_GEGLU:  # (the persistent ping-pong tile has not been raced in the call for GEGLU)
        tiles = [t for t, c in gemm_tiles().items() if c.geglu and c.family != GEMM_PPP]
    else:
        tiles = list(fam)
    if d.ln_c1:  # the LDS-DMA kernels carry the LayerNorm fold; tile 24 stays out of this race as it always has
        tiles = [t for t in tiles if fam[t] not in (GEMM_REG, GEMM_PP) and t != 24]
    if d.k_append:  # the appended 1x1 segment lives in the LDS-DMA loaders
        tiles = [t for t in tiles if fam[t] != GEMM_REG]
    return tiles


def splits_ok(d):
    return d.K >= 1024 and d.act != ACT_GEGLU and d.out_mode == OUT_ROWMAJOR and d.batch <= 1 and not d.out2 and not d.ln_c1


class Tuner:
    def __init__(self, E, margin):
        self.E, self.margin = E, margin
        self.ops = gemm_ops(E)
        self.ws = {}  # per stream: a scratch buffer large enough for every plan tried on it
        self.force_tiles = ()

    def workspace(self, side, nbytes):
        cur = self.ws.get(side)
        if cur is None or cur.numel() * 4 < nbytes:
            cur = torch.empty(max(nbytes // 4 + 64, 1 << 20), dtype=torch.float32, device=self.E.device)
            self.ws[side] = cur
            self.E._keep.append(cur)
        return cur.data_ptr()

    def set_plan(self, key, plan):
        tile, sk = plan % 100, plan // 100
        for i, d, side in self.ops[key]:
            t = GemmDesc.from_buffer_copy(d)
            t.tile, t.splitk = tile, sk
            nb = int(self.E.lib.gn_gemm_workspace_bytes(C.byref(t)))
            ws = self.workspace(side, nb) if nb > 0 else None
            check(self.E.lib.gn_program_set_gemm_plan(self.E._prog, i, tile, sk, ws), "gn_program_set_gemm_plan")

    def time_key(self, key, reps=2):
        """Replay the program op by op; -> min over reps of the summed time of this key's ops (ms)."""
        E = self.E
        idx = [i for i, _, _ in self.ops[key]]
        evs = [(E.event(), E.event()) for _ in idx]
        best = float("inf")
        for _ in range(reps):
            pos = 0
            for (e0, e1), i in zip(evs, idx):
                if i > pos:
                    E.run(pos, i)
                E.event_record(e0)
                E.run(i, i + 1)
                E.event_record(e1)
                pos = i + 1
            E.run(pos, E.num_ops)
            E.synchronize()
            best = min(best, sum(E.event_elapsed_ms(a, b) for a, b in evs))
        for a, b in evs:
            E.lib.gn_event_destroy(a)
            E.lib.gn_event_destroy(b)
        return best

    def profile_all(self):
        """One op-by-op replay with events around every gn_gemm op -> {key: summed ms}."""
        E = self.E
        where = sorted((i, k) for k, lst in self.ops.items() for i, _, _ in lst)
        evs, pos = [], 0
        E.run(0, E.num_ops)  # warm
        for i, k in where:
            if i > pos:
                E.run(pos, i)
            e0, e1 = E.event(), E.event()
            E.event_record(e0)
            E.run(i, i + 1)
            E.event_record(e1)
            evs.append((k, e0, e1))
            pos = i + 1
        E.run(pos, E.num_ops)
        E.synchronize()
        out = {k: 0.0 for k in self.ops}
        for k, a, b in evs:
            out[k] += E.event_elapsed_ms(a, b)
            E.lib.gn_event_destroy(a)
            E.lib.gn_event_destroy(b)
        return out

    def isolated(self, d, plan, side):
        E = self.E
        t = GemmDesc.from_buffer_copy(d)
        t.tile, t.splitk = plan % 100, plan // 100
        nb = int(E.lib.gn_gemm_workspace_bytes(C.byref(t)))
        t.workspace = self.workspace(side, nb) if nb > 0 else None
        e0, e1 = E.event(), E.event()
        check(E.lib.gn_gemm(E._ctx, C.byref(t)), "gn_gemm(race)")
        E.event_record(e0)
        for _ in range(3):
            check(E.lib.gn_gemm(E._ctx, C.byref(t)), "gn_gemm(race)")
        E.event_record(e1)
        ms = E.event_elapsed_ms(e0, e1)
        E.lib.gn_event_destroy(e0)
        E.lib.gn_event_destroy(e1)
        return ms

    def shortlist(self, key, incumbent, keep=5):
        _, d, side = self.ops[key][0]
        raced = sorted((self.isolated(d, t, side), t) for t in valid_plans(d))
        plans = [t for _, t in raced[:keep]]
        # tiles the isolated race cannot judge (deep rings: their point is the COLD weight stream of the call) always reach the in-call race
        forced = [t for t in self.force_tiles if t in valid_plans(d)]
        plans += forced
        if forced and splits_ok(d):
            plans += [t + 100 * sk for t in forced for sk in sorted({incumbent // 100, 2, 4}) if sk > 0 and sk * 512 <= d.K]
        if splits_ok(d):
            spl = []
            for t in plans[:2] + ([incumbent % 100] if incumbent % 100 else []):
                for sk in (1, 2, 3, 4, 6, 8):
                    if sk * 512 <= d.K:
                        spl.append((self.isolated(d, t + 100 * sk, side), t + 100 * sk))
            plans += [p for _, p in sorted(spl)[:4]]
        seen, out = set(), []
        for p in plans:
            if p not in seen and p != incumbent:
                seen.add(p)
                out.append(p)
        return out

    def tune(self, top):
        E = self.E
        base = self.profile_all()
        order = sorted(self.ops, key=lambda k: -base[k])[:top]
        total = sum(base.values())
        print(f"{len(self.ops)} gn_gemm shapes, {sum(len(v) for v in self.ops.values())} ops, {total:.2f} ms op-by-op; tuning the top {len(order)}", flush=True)
        changes = {}
        for key in order:
            _, d0, _ = self.ops[key][0]
            inc = int(d0.tile) + 100 * int(d0.splitk)
            cands = self.shortlist(key, inc)
            t_inc = self.time_key(key)
            best, t_best = inc, t_inc
            for p in cands:
                self.set_plan(key, p)
                t = self.time_key(key)
                if t < t_best:
                    best, t_best = p, t
            if best != inc and t_best < (1.0 - self.margin) * t_inc:
                # confirm: incumbent and challenger once more, interleaved
                self.set_plan(key, inc)
                t_inc2 = self.time_key(key)
                self.set_plan(key, best)
                t_best2 = self.time_key(key)
                if t_best2 < (1.0 - self.margin) * min(t_inc, t_inc2):
                    changes[key] = (inc, best, min(t_inc, t_inc2), min(t_best, t_best2), len(self.ops[key]))
                    print(f"  {key}: plan {inc} -> {best}   {min(t_inc, t_inc2):.3f} -> {min(t_best, t_best2):.3f} ms over {len(self.ops[key])} ops", flush=True)
                    continue
            self.set_plan(key, inc)
        return changes


def call_ms(pipe, ids, img, lat, steps, dev, calls=10):
    for _ in range(2):
        pipe(prompt_ids=ids, image=img, latents=lat, num_inference_steps=steps, guidance_scale=0.0, output_type="pt")
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        pipe(prompt_ids=ids, image=img, latents=lat, num_inference_steps=steps, guidance_scale=0.0, output_type="pt")
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return 1000.0 * ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="tiled_b8")
    ap.add_argument("--family", default="sd-turbo")
    ap.add_argument("--top", type=int, default=40)
    ap.add_argument("--margin", type=float, default=0.03)
    ap.add_argument("--force-tiles", default="", help="comma-separated tiles that always enter the in-call race")
    ap.add_argument("--denoise-steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "incall_tune.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    from genima_amd.pipeline import StableDiffusionControlNetPipeline

    pipe = StableDiffusionControlNetPipeline.from_synthetic(configs.family(args.family), seed=0, gen_device=dev)
    pipe.to(dev)
    for m in (pipe.vae, pipe.text_encoder, pipe.unet, pipe.controlnet):
        m._sd = None
    torch.cuda.empty_cache()
    pipe.enable_hip_graph(False)
    report = {}
    table = engine_mod._tune_table()
    for wl in args.workloads.split(","):
        B, H, W, desc = bench.WORKLOADS[wl]
        ids, img, lat = bench.synthetic_inputs(pipe, B, H, W, dev, 0)
        before = call_ms(pipe, ids, img, lat, args.denoise_steps, dev)
        io = pipe.program(B, H, W, args.denoise_steps)
        tuner = Tuner(io.engine, args.margin)
        tuner.force_tiles = tuple(int(t) for t in args.force_tiles.split(",") if t.strip())
        changes = tuner.tune(args.top)
        after = call_ms(pipe, ids, img, lat, args.denoise_steps, dev)
        print(f"{wl}: call {before:.2f} -> {after:.2f} ms with {len(changes)} plans changed", flush=True)
        if after < before:
            for key, (inc, best, *_rest) in changes.items():
                table[key] = best
            engine_mod._tune_dirty[0] = True
        else:  # the per-op sums lied about the call: leave the table alone
            print(f"{wl}: no gain on the call -- table unchanged", flush=True)
        report[wl] = {"workload": desc, "call_ms_before": before, "call_ms_after": after,
                      "changes": {k: {"from": v[0], "to": v[1], "ms_before": v[2], "ms_after": v[3], "ops": v[4]} for k, v in changes.items()}}
    engine_mod.save_tune_table()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
