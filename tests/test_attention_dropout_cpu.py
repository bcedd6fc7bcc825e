"""The attention dropout mask and its host side without a GPU: the numpy restatement (tests/attention_dropout_ref.py) against the known
answers of the formula (include/genima_hip.h, gn_attn_dropout), the binding's threshold / descriptor, the mask's statistics, and the ACT
trainer's per-call seed function."""
import numpy as np
import pytest

import attention_dropout_ref as DR
from genima_amd import _lib
from genima_amd.act_training import attn_call_seed


@pytest.mark.parametrize("seed,bh,i,j,r", DR.KNOWN_ANSWERS, ids=lambda x: hex(x) if isinstance(x, int) and x > 999 else str(x))
def test_known_answers(seed, bh, i, j, r):
    assert int(DR.hash_r(seed, bh, i, j)[0]) == r


def test_thresholds_and_descriptor():
    assert DR.threshold(0.1) == 429496729 and DR.threshold(0.5) == 2147483648 and DR.threshold(0.0) == 0
    for p in (0.0, 0.1, 0.3, 0.5, 0.999999999999):
        assert _lib.attn_dropout_threshold(p) == DR.threshold(p) <= 2 ** 32 - 1
    d = _lib.attn_dropout_desc(0.1, 0x0123456789ABCDEF)
    assert (d.threshold, d.seed_lo, d.seed_hi) == (429496729, 0x89ABCDEF, 0x01234567) and d.inv_keep == np.float32(1.0 / 0.9)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            _lib.attn_dropout_threshold(bad)
    for name in ("gn_attention_dropout_fwd", "gn_attention_dropout_bwd", "gn_attention_dropout_apply"):
        assert name in _lib.SIGNATURES
    import ctypes as C
    assert C.sizeof(_lib.AttnDropout) == 16


@pytest.mark.parametrize("seed", DR.KNOWN_SEEDS, ids=hex)
def test_p_zero_keeps_everything(seed):
    assert DR.keep_mask(seed, 0.0, 4, 40, 72).all()


def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize("p", DR.PS)
@pytest.mark.parametrize("seed", DR.KNOWN_SEEDS, ids=hex)
def test_rate_and_neighbour_correlation(seed, p):
    """16 x 264 x 264 elements: the keep rate within 4 sigma of 1 - p, the correlation of neighbours along j, i and bh within 4 / sqrt(n)
    (the formula's own figures on these seeds: <= 1.9 sigma, <= 2.5 / sqrt(n))."""
    keep = DR.keep_mask(seed, p, 16, 264, 264)
    n = keep.size
    t = DR.threshold(p) / 2.0 ** 32  # the drop probability the 32-bit threshold really gives
    z = (keep.mean() - (1 - t)) / np.sqrt(t * (1 - t) / n)
    cj, ci, cb = _corr(keep[:, :, :-1], keep[:, :, 1:]), _corr(keep[:, :-1], keep[:, 1:]), _corr(keep[:-1], keep[1:])
    print(f"seed {seed:#x} p {p}: rate z {z:+.2f}; corr * sqrt(n) along j {cj * np.sqrt(n):+.2f}, i {ci * np.sqrt(n):+.2f}, bh {cb * np.sqrt(n):+.2f}")
    assert abs(z) <= 4.0
    for c in (cj, ci, cb):
        assert abs(c) <= 4.0 / np.sqrt(n)


def test_trainer_seeds_are_distinct_and_reproducible():
    """Distinct seeds for every (step 0..2, call index) pair -- the full ACT update makes 4 + 4 + 2 * 6 = 20 attention calls -- and for
    another trainer seed; the same trainer seed gives the same seeds.  64-bit values."""
    for ts in (0, 3, 2 ** 63 + 5):
        seeds = [attn_call_seed(ts, step, idx) for step in range(3) for idx in range(20)]
        assert len(set(seeds)) == len(seeds) and all(0 <= s < 2 ** 64 for s in seeds)
        assert seeds == [attn_call_seed(ts, step, idx) for step in range(3) for idx in range(20)]
        assert any(s >> 32 for s in seeds), "the high word is used"
    assert not set(attn_call_seed(0, s, i) for s in range(3) for i in range(20)) & set(attn_call_seed(1, s, i) for s in range(3) for i in range(20))
