"""-m "not gpu": the GEMM planner (the tile that runs, the K split, gn_gemm_plan_valid) and the autotuner's candidate lists over the corpus of
tests/golden/gemm_plan_sweep.py agree with the fixture that script recorded (tests/golden/gemm_plan_golden.npz; rewritten only where a change
of the plan is intended), and the library's tile export agrees with the tile shapes recorded there."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from genima_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_plan_golden.npz")


def test_tile_export_matches_the_recorded_shapes():
    g = np.load(GOLDEN)
    tiles = _lib.gemm_tiles()
    assert list(tiles) == list(range(1, len(g["tile_bmn"]) + 1))
    assert [(c.bm, c.bn) for c in tiles.values()] == [tuple(r) for r in g["tile_bmn"].tolist()]
    assert _lib.load().gn_gemm_tile_info(len(tiles) + 1, C.byref(_lib.GemmTile())) != 0


def test_planner_workspace_and_autotune_candidates_match_the_fixture(tmp_path):
    out = str(tmp_path / "sweep.npz")
    env = dict(os.environ, GN_GEMM_LOG_FALLBACK="1")  # read once per process: a fresh interpreter
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "gemm_plan_sweep.py"), "--out", out], env=env, check=True, timeout=600)
    g, n = np.load(GOLDEN), np.load(out)
    for field in ("tile", "ws", "valid", "cands"):
        bad = np.flatnonzero(g[field] != n[field]) if g[field].shape == n[field].shape else [-1]
        assert len(bad) == 0, f"{field}: {len(bad)} descriptors differ from the fixture (first {bad[:5]})"
