"""The GEMM planner and the autotuner's candidate lists over a corpus of descriptors, without a GPU.

The corpus is every key of genima_amd/gemm_tune_gfx950.json (as it stood when the fixture was written; the fixture keeps the keys), each
turned into a gn_gemm_desc with fake aligned pointers (the planner never dereferences them), in several variants (GEGLU, fp8, ln_c1,
k_append, norm_in, up_phases, batch > 1, operands too large for the LDS-DMA loaders) and crossed with requested tiles 0 .. 25 and K splits.  For each descriptor it records

  tile   the tile that runs (from the GN_GEMM_LOG_FALLBACK=1 lines; the requested tile when none is logged; -1 for tile 0, the heuristic)
  ws     gn_gemm_workspace_bytes (encodes the K split, and tile 0's choice where it splits K or runs tile 25)
  valid  gn_gemm_plan_valid

and Engine._race_candidates (what _autotune races, in order) with an empty table and with the shipped entry plus GN_RETUNE challengers.

    python tests/golden/gemm_plan_sweep.py --write           # (re)write tests/golden/gemm_plan_golden.npz
    python tests/golden/gemm_plan_sweep.py --out sweep.npz   # sweep the corpus of the committed fixture

GN_GEMM_LOG_FALLBACK=1 must be set in the environment (the library reads it once); GN_LIB_PATH picks another library build.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from genima_amd import _lib  # noqa: E402
from genima_amd.engine import Engine  # noqa: E402

GOLDEN = os.path.join(HERE, "gemm_plan_golden.npz")
NUM_TILES = 25  # the tiles of the library the fixture was written against
VARIANTS = ("base", "geglu", "fp8", "ln", "ln_geglu", "k_append", "norm_in16", "norm_in64", "norm_in256", "norm_in1024", "up_phases", "batch2",
            "big", "big_geglu", "big_k_append")  # big: W beyond the 32-bit buffer offsets of the LDS-DMA loaders
CHALLENGERS = [15, 25, 7, 16, 3, 19]


def desc_of(key: str, variant: str) -> _lib.GemmDesc:
    f = key.split("|")
    conv, M, N, K, C1, C2, KH, stride, ups, act, out_mode, res = (int(v) for v in f[:12])
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.act, d.out_mode, d.out_scale = M, N, K, act, out_mode, 1.0
    d.a, d.w, d.out, d.bias = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    d.lda, d.ldw, d.ldo, d.rows_per_batch = K, K, N, M
    if res:
        d.residual, d.ldr = 0x50000000, N
    if conv:
        wo = 1
        while (2 * wo) * (2 * wo) <= M and M % (2 * wo) == 0:
            wo *= 2
        d.conv, d.B, d.Ho, d.Wo, d.C1, d.C2, d.KH, d.KW, d.stride, d.upsample2x = 1, 1, M // wo, wo, C1, C2, KH, KH, stride, ups
        d.H, d.W = max(1, d.Ho * stride // (2 if ups else 1)), max(1, wo * stride // (2 if ups else 1))
        if C2:
            d.a2 = 0x60000000
    flags = f[12:]
    for s in flags:
        if s.startswith("b"):
            d.batch = int(s[1:])
        elif s == "acc":
            d.accumulate = 1
        elif s == "fp8":
            d.fp8 = 1
        elif s.startswith("o2"):
            d.out2, d.split_n = 0x90000000, int(s[2:])
        elif s == "ln":
            d.ln_c1, d.ln_eps = 0x70000000, 1e-5
        elif s == "ka":
            d.k_append = 1
        elif s == "gn":
            d.norm_in.rows_per_sample = 64
    if variant in ("geglu", "ln_geglu", "big_geglu"):
        d.act = 5
    if variant == "fp8":
        d.fp8 = 1
    if variant in ("ln", "ln_geglu"):
        d.ln_c1, d.ln_eps = 0x70000000, 1e-5
    if variant in ("k_append", "big_k_append") or d.k_append:
        d.k_append, d.a2 = 1, 0x60000000
        if not d.C2:
            d.C2 = 64
        d.lda2 = d.C2
    if variant.startswith("norm_in") or "gn" in flags:
        ct = (d.C1 if d.k_append else d.C1 + d.C2) if d.conv else (d.K - d.C2 if d.k_append else d.K)
        n = d.norm_in
        n.stats, n.gamma, n.beta, n.eps, n.groups = 0x80000000, 0xA0000000, 0xB0000000, 1e-5, 32
        n.cpg = max(1, ct // 32)
        if variant.startswith("norm_in"):
            n.rows_per_sample = int(variant[7:])
        n.samples = max(1, M // max(1, n.rows_per_sample))
    if variant == "up_phases":
        d.batch, d.up_phases, d.out_row_width = 4, 1, max(1, d.Wo)
    if variant == "batch2":
        d.batch = 2
    if variant.startswith("big"):
        d.ldw = ((1 << 31) // N + 8) // 8 * 8
    return d


def plans(variant):
    """(tile, splitk) requested: the plain problems cross every tile with every K split, the variants every tile unsplit and two splits."""
    sks = range(9) if variant == "base" else (0, 2, 5)
    return [(t, s) for t in range(NUM_TILES + 1) for s in sks]


def sweep(keys):
    lib = _lib.load()
    tiles, ws, valid = [], [], []
    log = tempfile.TemporaryFile()
    saved = os.dup(2)
    sys.stderr.flush()
    os.dup2(log.fileno(), 2)
    try:
        i = 0
        for key in keys:
            for variant in VARIANTS:
                d = desc_of(key, variant)
                for t, s in plans(variant):
                    d.tile, d.splitk = t, s
                    os.write(2, b"#%d\n" % i)
                    ws.append(int(lib.gn_gemm_workspace_bytes(C.byref(d))))
                    valid.append(int(lib.gn_gemm_plan_valid(C.byref(d))))
                    tiles.append(t if t > 0 else -1)
                    i += 1
    finally:
        os.dup2(saved, 2)
        os.close(saved)
    log.seek(0)
    cur = -1
    for line in log.read().decode().splitlines():
        if line.startswith("#"):
            cur = int(line[1:])
        elif line.startswith("[gn_gemm] tile "):
            tiles[cur] = int(line.split(" requested, ")[1].split(" runs")[0])
    return np.array(tiles, np.int8), np.array(ws, np.int64), np.array(valid, np.int8)


def candidates(keys, table):
    """-> one flat array of every candidate list, each ended by -1: per key and variant, the race of a new shape, then the re-race
    of the shipped entry against CHALLENGERS."""
    out = []
    for key in keys:
        for variant in VARIANTS:
            d = desc_of(key, variant)
            out += Engine._race_candidates(d, key, {}, []) + [-1]
            out += Engine._race_candidates(d, key, {key: table.get(key, 18)}, CHALLENGERS) + [-1]
    return np.array(out, np.int16)


def tile_shapes(header):
    """bm x bn of every tile from the kCfg initializer of csrc/gemm_common.h (as written when the fixture was made)."""
    import re

    src = open(header).read()
    body = src[src.index("kCfg[] = {"):]
    body = body[:body.index("};")]
    return np.array([(int(a), int(b)) for a, b in re.findall(r"\{(\d+),\s*(\d+),", body)], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write the fixture from the current library and tune table")
    ap.add_argument("--out", help="sweep the fixture's corpus and save the results here")
    args = ap.parse_args()
    if os.environ.get("GN_GEMM_LOG_FALLBACK") != "1":
        sys.exit("set GN_GEMM_LOG_FALLBACK=1")
    if args.write:
        with open(os.path.join(ROOT, "genima_amd", "gemm_tune_gfx950.json")) as f:
            table = {k: int(v) for k, v in json.load(f).items()}
        keys = sorted(k for k in table if not k.startswith("wg|"))  # (wg: the weight-gradient kernels of gemm_tn.hip, another table)
        shapes = tile_shapes(os.path.join(ROOT, "genima_amd", "csrc", "gemm_common.h"))
        assert len(shapes) == NUM_TILES, len(shapes)
        out, plans_of = GOLDEN, np.array([table[k] for k in keys], np.int32)
    else:
        g = np.load(GOLDEN)
        keys, plans_of, shapes = [str(k) for k in g["keys"]], g["plans"], g["tile_bmn"]
        table = dict(zip(keys, (int(p) for p in plans_of)))
        out = args.out
    tiles, ws, valid = sweep(keys)
    np.savez_compressed(out, keys=np.array(keys), plans=plans_of, tile_bmn=shapes, tile=tiles, ws=ws, valid=valid,
                        cands=candidates(keys, table))
    print(f"{len(tiles)} descriptors, {int((tiles >= 0).sum())} with a known tile -> {out}")


if __name__ == "__main__":
    main()
