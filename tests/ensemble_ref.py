"""float64 restatement of the temporal-ensembling rule of include/genima_hip.h (gn_action_ensemble), written from the rule and not from the
kernel: per batch row a plain list of (start, chunk) pairs, newest last; no ring, no slots.

  * a call at environment step t appends (t, chunk) and keeps the last ``K`` pairs of the row;
  * the action of a target step s in [t, t + h) averages every kept chunk with 0 <= s - start < T, the i-th of them (i = 0: the one that has
    been there longest) weighing exp(-m i);
  * a reset empties the row's list before the new pair goes in.
"""
import numpy as np


class EnsembleRef:
    def __init__(self, B, T, A, K, h, m=0.01):
        self.B, self.T, self.A, self.K, self.h, self.m = B, T, A, K, h, float(m)
        self.rows = [[] for _ in range(B)]

    def __call__(self, chunk, steps, reset=None):
        """chunk [B, T, >= A] (any float dtype), steps [B] ints, reset [B] bools -> f64 [B, h, A]."""
        chunk = np.asarray(chunk, dtype=np.float64)[:, :, : self.A]
        out = np.zeros((self.B, self.h, self.A), dtype=np.float64)
        for b in range(self.B):
            if reset is not None and reset[b]:
                self.rows[b] = []
            t = int(steps[b])
            self.rows[b] = (self.rows[b] + [(t, chunk[b].copy())])[-self.K:]
            for j in range(self.h):
                s = t + j
                covering = [c[s - start] for start, c in self.rows[b] if 0 <= s - start < self.T]
                w = np.exp(-self.m * np.arange(len(covering), dtype=np.float64))
                out[b, j] = (w[:, None] * np.stack(covering)).sum(0) / w.sum()
        return out
