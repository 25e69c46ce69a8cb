"""Helpers of the mixed-rate tests (tests/test_mixed_rate_gpu.py): the stream set, raw recordings per stream, and the ORACLE — the offline
assembly formed with the existing single-rate call, msig_rs_resample, one stream at a time, truncated to the slowest stream and laid side
by side (a stream at the output rate is its raw rows).  tests/test_resample_gpu.py ties msig_rs_resample to the np.longdouble
restatement (tests/rs_reference.py); nothing here goes through include/msig_mx.h or through MixedResampler.apply.  The pool class drives
msig_mx_lv_push through the C ABI with its own integer bookkeeping (a raw count per stream, the row bound of lv_reference's rule)."""
import ctypes as C

import numpy as np
import torch

import lv_reference as R
from multimodalsignal_amd import _lib as L
from multimodalsignal_amd.resample import FirResampler, MixedResampler, Stream

FS = 64.0
NAMES8 = R.NAMES8
# a permuted order of NAMES8: 4 columns at 700 Hz (chest_EDA, the one under log1p, among them), 1 at 32 Hz, 1 at 64 Hz, 2 at 4 Hz
STREAMS = (("chest", 700, ("chest_Resp", "chest_EDA", "chest_EMG", "chest_ECG")), ("acc", 32, ("chest_ACC_x",)), ("bvp", 64, ("wrist_BVP",)),
           ("slow", 4, ("wrist_EDA", "chest_Temp")))
ORDER = [c for _n, _f, cols in STREAMS for c in cols]          # the columns of a ring row


def resampler(device):
    return MixedResampler([Stream(n, f, list(cols)) for n, f, cols in STREAMS], FS, device=device)


def cols_of(key):
    """lv_reference.COLS[key], which indexes NAMES8, as columns of a ring row in ORDER, and the log1p mask (chest_EDA)."""
    cols = [ORDER.index(NAMES8[c]) for c in R.COLS[key]]
    return cols, sum(1 << i for i, c in enumerate(cols) if ORDER[c] == "chest_EDA")


def raw_streams(mx, n_out, seed):
    """{name: (n_g, ncols_g) float64}: per stream lv_reference.recording at the stream's length, its own columns of it (so a column
    keeps its regime: chest_EDA positive and heavy-tailed, chest_Temp and chest_ACC_x far from zero, chest_EMG constant), every stream
    a little longer than n_out outputs need, each by another amount."""
    out = {}
    for i, g in enumerate(mx.streams):
        n = g.max_rows(n_out + 3 * i) + (i % 2)
        out[g.name] = np.ascontiguousarray(R.recording(n, seed + 101 * i)[:, [NAMES8.index(c) for c in g.columns]])
    return out


def stream_outputs(mx, dev, device):
    """{name: (count_g, ncols_g) device tensor}: every stream resampled on its own by msig_rs_resample (the identity: its raw rows)."""
    out = {}
    st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    for g in mx.streams:
        x = dev[g.name]
        if g.identity:
            out[g.name] = x.clone()
            continue
        r = FirResampler(g.fs, FS, device)
        n = r.out_count(x.shape[0])
        y = torch.empty((n, g.ncols), dtype=torch.float64, device=device)
        L.check(L.lib().msig_rs_resample(x.data_ptr(), x.shape[0], g.ncols, *r.ratio_args(), y.data_ptr(), n, st), "msig_rs_resample")
        out[g.name] = y
    return out


def assembly(mx, dev, device):
    """(n_out, C_all) device tensor: stream_outputs truncated to the slowest stream, side by side in ORDER."""
    ys = stream_outputs(mx, dev, device)
    n = min(y.shape[0] for y in ys.values())
    return torch.cat([ys[g.name][:n] for g in mx.streams], dim=1).contiguous()


class MxPool:
    """A caller-owned pool of `slots` rings and tail blocks filled with 0x5A and the host's raw counts, a count per (session, stream)."""

    def __init__(self, mx, Rn, slots, sessions, device, pad=0):
        self.mx, self.R, self.slots, self.device, self.pad = mx, Rn, slots, device, pad
        self.C_all = mx.C_all
        self.mem = torch.full((slots, Rn * self.C_all * 8 + pad), 0x5A, dtype=torch.uint8, device=device)
        self.tails = torch.full((slots, mx.tail_doubles * 8 + pad), 0x5A, dtype=torch.uint8, device=device)
        self.groups = mx.groups()
        self.raw = {k: [0] * len(mx.streams) for k in sessions}

    def args(self):
        return self.mem.data_ptr(), self.slots, self.R, self.mem.shape[1], self.C_all

    def tail_args(self):
        return self.tails.data_ptr(), self.tails.shape[1], self.mx.h.data_ptr(), self.groups, len(self.mx.streams)

    def counts(self, k):
        return [g.out_count(n) for g, n in zip(self.mx.streams, self.raw[k])]

    def written(self, k):
        return min(self.counts(k))

    def push(self, chunks, missing=False):
        """chunks: [(session, stream index, (n, ncols) device rows)] — ONE msig_mx_lv_push, the chunks back to back in one staging
        buffer (`missing`: no staging buffer)."""
        n = len(chunks)
        staging = torch.cat([x.reshape(-1) for _k, _g, x in chunks]) if n > 1 else chunks[0][2].reshape(-1).contiguous()
        rc = L.lib().msig_mx_lv_push(*self.args(), *self.tail_args(), (C.c_int32 * n)(*[k for k, _g, _x in chunks]),
                                     (C.c_int32 * n)(*[g for _k, g, _x in chunks]), (C.c_int64 * n)(*[self.raw[k][g] for k, g, _x in chunks]),
                                     (C.c_int64 * n)(*[int(x.shape[0]) for _k, _g, x in chunks]), n, None if missing else staging.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        L.check(rc, "msig_mx_lv_push")
        for k, g, x in chunks:
            self.raw[k][g] += int(x.shape[0])

    def ring(self, k):
        return self.mem[k, :self.R * self.C_all * 8].view(torch.float64).view(self.R, self.C_all).cpu().numpy()

    def tail(self, k, gi):
        g = self.mx.streams[gi]
        t = self.tails[k, :self.mx.tail_doubles * 8].view(torch.float64)
        return t[g.tail_off:g.tail_off + g.tail_rows * g.ncols].view(g.tail_rows, g.ncols).cpu().numpy()
