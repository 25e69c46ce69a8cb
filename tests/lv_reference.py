"""A numpy restatement of include/msig_lv.h and of live.py's host logic, written from the definitions and sharing no code with
either: a ring is a plain array filled row by row with i % R, a window is read back row by row, the bookkeeping is a loop over single
samples, and the alarms are read off the whole raw state vector.  Also the recording generator and the member models of the live
tests (the generator restates tests/test_recording_gpu.py's, which is a test module and is not imported)."""
import numpy as np

MAX_C = 16
NAMES8 = ["chest_ECG", "chest_EDA", "chest_Resp", "chest_Temp", "chest_ACC_x", "wrist_BVP", "chest_EMG", "wrist_EDA"]
# column 1 is the one under log1p (positive, heavy-tailed); 3 and 4 have mean >> spread; 6 is exactly constant
COLS = {"3of8": [5, 1, 4], "1of8": [3], "8of8": [7, 2, 0, 3, 1, 6, 5, 4]}


def mask_of(cols):
    return sum(1 << c for c, col in enumerate(cols) if NAMES8[col] == "chest_EDA")


def recording(Ln, seed):
    """(Ln, 8) float64 with a slow drift, so that a range of windows has statistics of its own."""
    rs = np.random.RandomState(seed)
    spread = 0.5 + rs.rand(8)
    sig = rs.randn(Ln, 8) * spread + rs.randn(8) + 0.7 * spread * np.sin(2 * np.pi * np.arange(Ln) / Ln)[:, None]
    sig[:, 1] = np.exp(0.8 * rs.randn(Ln) + 0.5 * np.sin(2 * np.pi * np.arange(Ln) / Ln)) + 0.1
    sig[:, 3] = 33.0 + 0.05 * rs.randn(Ln) + 0.03 * np.arange(Ln) / Ln
    sig[:, 4] = 0.9 + 0.02 * rs.randn(Ln)
    sig[:, 6] = 0.75
    return np.ascontiguousarray(sig)


def count(L, T, S):
    return 0 if L < T else (L - T) // S + 1


class Ring:
    """A ring of R rows filled sample by sample: sample i in row i % R."""

    def __init__(self, R, C_all, fill=np.nan):
        self.R, self.rows, self.written = R, np.full((R, C_all), fill, dtype=np.float64), 0

    def push(self, chunk):
        for row in chunk:
            self.rows[self.written % self.R] = row
            self.written += 1

    def window(self, n, T, S):
        """(T, C_all): samples [n S, n S + T); refuses what is not there."""
        assert n * S + T <= self.written and n * S >= self.written - self.R
        return np.stack([self.rows[i % self.R] for i in range(n * S, n * S + T)])


def normalised(win, cols, log1p_mask, mean, inv):
    """(C, T) float32 of a (T, C_all) window: (float)((v - mean) * inv) in float64."""
    v = win[:, cols].astype(np.float64)
    for c in range(len(cols)):
        if (log1p_mask >> c) & 1:
            v[:, c] = np.log1p(v[:, c])
    return np.ascontiguousarray(((v - np.asarray(mean)) * np.asarray(inv)).astype(np.float32).T)


def bookkeeping(n_push, written, next_window, pending, R, T, S, warm):
    """A push of n_push samples, one sample at a time: the segments [(length, statistics due, windows handed out)] of the greedy
    rule — a sample is appended unless it would overwrite one that a window not yet handed out needs (or the segment is a whole
    ring already: one append takes R rows at most); then the statistics are taken
    (if the head is complete and they are pending) and the complete windows handed out, and the next segment begins."""
    head = (warm - 1) * S + T if warm else 0
    out, left = [], n_push
    while left > 0:
        a = 0
        while left > 0 and a < R and written + 1 - R <= next_window * S:        # row (written % R) still holds sample written - R
            written, left, a = written + 1, left - 1, a + 1
        assert a > 0
        due = pending and written >= head
        pending = pending and not due
        wins = []
        if not pending:
            while next_window * S + T <= written:
                wins.append(next_window)
                next_window += 1
        out.append((a, due, wins))
    return out, written, next_window, pending


def raw_state(smoothed, on, off):
    raw, cur = [], False
    for v in smoothed:
        if cur:
            if v <= off:
                cur = False
        elif v >= on:
            cur = True
        raw.append(cur)
    return raw


def alarms(smoothed, on, off, min_on):
    """[(kind, window, start_window)] by the live rule, from the whole raw state vector: a maximal run [a, b) of at least min_on
    windows raises an onset at a + min_on - 1 and, if it ends before the stream does, an offset at b."""
    raw = raw_state(smoothed, on, off)
    out, n, N = [], 0, len(raw)
    while n < N:
        if raw[n]:
            a = n
            while n < N and raw[n]:
                n += 1
            if n - a >= min_on:
                out.append(("onset", a + min_on - 1, a))
                if n < N:
                    out.append(("offset", n, a))
        else:
            n += 1
    return out


def models(kind, Cin, K, M, device, seed=5):
    """Randomly initialised members (never trained), in eval mode."""
    import torch
    from multimodalsignal_amd.models import CnnGruAttentionModel, CnnGruModel
    cls = CnnGruAttentionModel if kind == "cnn_gru_attention" else CnnGruModel
    out = []
    for r in range(M):
        torch.manual_seed(seed + r)
        out.append(cls(Cin, K).to(device).eval())
    return out
