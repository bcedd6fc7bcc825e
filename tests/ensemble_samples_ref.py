"""float64 restatement of the sample-combined ensembling rule of include/genima_hip.h (gn_action_ensemble_samples_f16), written from the rule:
R sampled chunks per row are combined into one -- their mean, or their medoid (the sample with the smallest summed L1 distance to all the
others over every element alike, the lowest index on a tie) -- and the combined chunk goes into tests/ensemble_ref.py's EnsembleRef as the new
chunk.  ``spread`` is the mean over samples and elements of |sample - combined|.
"""
import numpy as np

from ensemble_ref import EnsembleRef

RULES = ("mean", "medoid")


def medoid_distances(x):
    """x [R, ...] -> f64 [R]: D_r = sum_q d(r, q), d(r, q) = sum over every element of |x_r - x_q|.  Each pair's distance is summed once and
    used for both of its samples, so what is equal by symmetry (R = 2: D_0 = D_1 = d(0, 1); two identical samples) is equal in these numbers."""
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    R = len(x)
    d = np.zeros((R, R))
    for r in range(R):
        for q in range(r + 1, R):
            d[r, q] = d[q, r] = np.abs(x[r] - x[q]).sum()
    return np.array([sum(d[r, q] for q in range(R)) for r in range(R)])  # added in the order q = 0 .. R - 1


def medoid_margin(x):
    """-> (ties, margin): the samples whose D equals the smallest one exactly (the pick is the lowest of them), and (D_next - D_best) / D_best
    for the smallest D that is larger (inf where there is none or D_best is 0)."""
    D = medoid_distances(x)
    best = D.min()
    ties = [r for r in range(len(D)) if D[r] == best]
    rest = D[D > best]
    return ties, (np.inf if rest.size == 0 or best == 0.0 else float((rest.min() - best) / best))


TIE_CALL = 4  # sample_chunks: the call whose row 0 holds two identical best samples (1 and 2) where R >= 3


def sample_chunks(B, R, T, A, ld, seed, n=30):
    """n calls of R sampled chunks per row, f32 [n, B, R, T, ld] holding f16-representable values; the pad columns hold 60000 (f16 has no 1e30),
    which would wreck any sum that read them.  A sample is one base chunk in [-2, 2] plus s_r times a noise field the samples SHARE plus a
    small field of its own (0.004): the scales s_r = 0.05 (1 + k), k a permutation of 0 .. R - 1 that turns with the call and the row, are
    clearly different, so the summed distances D_r are set by the scales -- the medoid is the sample of the median scale, with a margin of
    tens of per cent for R >= 3 -- and not by the draw.  R = 2 is a tie by symmetry (pick 0), R = 1 has nothing to compare."""
    g = np.random.RandomState(seed)
    x = np.zeros((n, B, R, T, ld), dtype=np.float32)
    for c in range(n):
        for b in range(B):
            base, shared = g.uniform(-2, 2, (T, ld)), g.uniform(-1, 1, (T, ld))
            scales = 0.05 * (1 + np.roll(np.arange(R), c + b))
            if c == TIE_CALL and b == 0 and R >= 3:
                scales = 0.05 * np.array([5, 3, 3, 1, 4][:R] if R > 3 else [5, 3, 3])
            for r in range(R):
                x[c, b, r] = base + scales[r] * shared + 0.004 * g.uniform(-1, 1, (T, ld))
            if c == TIE_CALL and b == 0 and R >= 3:
                x[c, b, 2] = x[c, b, 1]
    x = x.astype(np.float16).astype(np.float32)
    x[..., A:] = 60000.0
    return x


def combine(x, rule):
    """x [R, T, A] -> (combined f64 [T, A], pick (-1 under mean), spread)."""
    x = np.asarray(x, dtype=np.float64)
    if rule == "mean":
        pick, c = -1, x.sum(axis=0) / len(x)
    elif rule == "medoid":
        pick = int(np.argmin(medoid_distances(x)))  # argmin: the first of equal minima
        c = x[pick]
    else:
        raise ValueError(rule)
    return c, pick, float(np.abs(x - c[None]).sum() / len(x) / c.size)


class EnsembleSamplesRef:
    def __init__(self, B, R, T, A, K, h, m=0.01, rule="mean"):
        self.B, self.R, self.A, self.rule = B, R, A, rule
        self.ens = EnsembleRef(B, T, A, K, h, m)

    def __call__(self, chunk, steps, reset=None, picks=None):
        """chunk [B, R, T, >= A] -> (f64 [B, h, A], picks int [B], spreads f64 [B]).  ``picks``: under medoid, the samples to take instead of
        the f64 medoids (inputs that keep no margin between two D_r: the caller checks the picks it passes)."""
        chunk = np.asarray(chunk, dtype=np.float64)[..., : self.A]
        assert chunk.shape[:2] == (self.B, self.R)
        parts = [combine(chunk[b], self.rule) for b in range(self.B)]
        if picks is not None and self.rule == "medoid":
            parts = [(chunk[b, int(picks[b])], int(picks[b]), float(np.abs(chunk[b] - chunk[b, int(picks[b])][None]).mean())) for b in range(self.B)]
        out = self.ens(np.stack([p[0] for p in parts]), steps, reset)
        return out, np.array([p[1] for p in parts]), np.array([p[2] for p in parts])


def replay_table(chunks, first_tr, h, temporal_agg, m, rule):
    """The open-loop side (gn_openloop_exec_actions_samples): chunks [R, N, T, >= A], first_tr [N] -> (f64 [N, A], picks [N]): every episode is
    run through EnsembleSamplesRef with a call every h steps after a reset; transition n's action is the row of its step in the call covering it."""
    chunks = np.asarray(chunks, dtype=np.float64)
    R, N, T, A = chunks.shape
    K = -(-T // h) if temporal_agg else 1
    out, picks = np.zeros((N, A)), np.zeros(N, dtype=np.int64)
    for n in range(N):
        picks[n] = combine(chunks[:, n], rule)[1]
    for f in sorted(set(int(v) for v in first_tr)):
        rows = [n for n in range(N) if int(first_tr[n]) == f]
        ref = EnsembleSamplesRef(1, R, T, A, K, h, m, rule)
        for t in range(0, len(rows), h):
            got, _, _ = ref(chunks[:, f + t][None], [t], [t == 0])
            for j in range(min(h, len(rows) - t)):
                out[f + t + j] = got[0, j]
    return out, picks
