"""Synthetic WESAD-shaped data (the real dataset is not redistributable and is absent from
the reference tree).  Writes the on-disk format preprocess.py:217-222
produces — ``{sid}_X.npy`` (N,T,C_all) float64, ``{sid}_y.npy`` raw protocol labels
{1,2,3,4}, ``_channel_names.txt`` — with a class-dependent planted signal so that
training has something to learn."""
from pathlib import Path

import numpy as np

CHANNELS6 = ["chest_ECG", "chest_EDA", "chest_Resp", "chest_EMG", "wrist_BVP", "wrist_EDA"]
ALL_SUBJECTS = [f"S{i}" for i in range(2, 18) if i != 12]          # main.py:67


def subject_window_counts(n_subjects, windows_per_subject, spread, seed=42):
    """Per-subject window counts: `windows_per_subject` +- `spread` (WESAD recordings differ in length by a few minutes, so the
    reference's per-subject `.npy` files differ by a few windows, dataset.py:17-27); spread 0 = equal sizes."""
    if not spread:
        return [int(windows_per_subject)] * n_subjects
    rs = np.random.RandomState(seed + 7919)
    return [int(windows_per_subject + v) for v in rs.randint(-spread, spread + 1, size=n_subjects)]


def make_synthetic_wesad(out_dir, subjects=ALL_SUBJECTS, windows_per_subject=270, T=3840, channels=CHANNELS6,
                         seed=42, fs=64.0, difficulty=1.0, window_spread=0):
    """`difficulty` >= 1 shrinks the class-dependent effects by 1/difficulty while the per-window,
    label-independent variability stays, so classes overlap more (1.0 is almost separable).
    `window_spread` > 0: subject i gets windows_per_subject +- window_spread windows (subject_window_counts)."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    rs = np.random.RandomState(seed)
    C = len(channels)
    t = np.arange(T) / fs
    a = 1.0 / float(difficulty)
    # protocol mix of WESAD: baseline ~20 min, TSST ~10, amusement ~6.5, meditation 2x7
    probs = np.array([20.0, 10.0, 6.5, 14.0])
    probs /= probs.sum()
    counts = subject_window_counts(len(subjects), windows_per_subject, window_spread, seed)
    for si, sid in enumerate(subjects):
        n = counts[si]
        y = rs.choice([1, 2, 3, 4], size=n, p=probs)
        gain = 0.7 + 0.6 * rs.rand(C)                  # subject-specific scale / offset (what the z-score removes)
        offs = rs.randn(C)
        x = rs.randn(n, T, C)
        stress = (y == 2).astype(np.float64)[:, None]
        hr = 1.1 + 0.30 * a * stress + 0.12 * rs.randn(n, 1)                  # heart-rate like rhythm (Hz), jittered per window
        x[:, :, 0] += 1.5 * np.sin(2 * np.pi * hr * t[None, :] + rs.rand(n, 1) * 6.28)
        if C > 1:
            level = 1.0 + 0.5 * a * stress + 0.35 * rs.randn(n, 1)           # tonic EDA level, positive
            x[:, :, 1] = np.abs(x[:, :, 1]) * 0.2 + np.abs(level) + 0.0015 * a * t[None, :] * stress
        if C > 2:
            br = 0.25 + 0.06 * a * stress + 0.04 * rs.randn(n, 1)
            x[:, :, 2] += np.sin(2 * np.pi * br * t[None, :])
        for c in range(3, C):
            x[:, :, c] += 0.3 * a * stress * np.sin(2 * np.pi * (0.5 + 0.1 * c) * t[None, :])
        x = x * gain[None, None, :] + offs[None, None, :]
        if C > 1:
            x[:, :, 1] = np.abs(x[:, :, 1]) + 0.05
        np.save(out / f"{sid}_X.npy", x.astype(np.float64))
        np.save(out / f"{sid}_y.npy", y.astype(np.int64))
    (out / "_channel_names.txt").write_text("\n".join(channels) + "\n")
    return out


def make_synthetic_recording(phases, fs=64.0, channels=CHANNELS6, seed=42, difficulty=1.0, block_s=60.0, gaps=None):
    """ONE continuous recording with make_synthetic_wesad's planted effects, piecewise per protocol phase: `phases` is a list of
    (raw label 1..4, seconds).  Returns (sig (L, C) float64, phase table) — the table one dict per phase with its raw label, its
    first and one-past-last sample and the same in seconds.

    What make_synthetic_wesad draws per window (heart and breathing rate, tonic EDA level) is drawn here per `block_s` seconds of a
    phase and held; the two rhythms' frequencies are integrated over the whole recording, so their phase is continuous across
    blocks and protocol phases; the EDA ramp of the stress class rises over the first `block_s` seconds of a stress phase and
    stays.  Subject gain and offset are one draw for the recording.  The draws are this function's own (RandomState(seed)):
    make_synthetic_wesad's stream and files do not depend on it.
    `gaps` (default None: no sample is missing): a parse_synthetic_gaps spec of samples to set to NaN afterwards (plant_gaps)."""
    phases = [(int(lab), float(sec)) for lab, sec in phases]
    if not phases or any(lab not in (1, 2, 3, 4) or not sec > 0 for lab, sec in phases):
        raise ValueError(f"phases must be a non-empty list of (raw label 1..4, seconds > 0), got {phases!r}")
    rs = np.random.RandomState(seed)
    C = len(channels)
    a = 1.0 / float(difficulty)
    lens = [int(round(sec * fs)) for _, sec in phases]
    L = int(sum(lens))
    table, at = [], 0
    for (lab, _), n in zip(phases, lens):
        table.append({"label": lab, "start": at, "end": at + n, "start_s": at / fs, "end_s": (at + n) / fs})
        at += n
    gain = 0.7 + 0.6 * rs.rand(C)
    offs = rs.randn(C)
    x = rs.randn(L, C)
    t = np.arange(L) / fs
    stress, hr, level, br, ramp = (np.zeros(L) for _ in range(5))
    blk = max(1, int(round(block_s * fs)))
    for row in table:
        s = 1.0 if row["label"] == 2 else 0.0
        for b0 in range(row["start"], row["end"], blk):
            b1 = min(b0 + blk, row["end"])
            hr[b0:b1] = 1.1 + 0.30 * a * s + 0.12 * rs.randn()
            level[b0:b1] = 1.0 + 0.5 * a * s + 0.35 * rs.randn()
            br[b0:b1] = 0.25 + 0.06 * a * s + 0.04 * rs.randn()
        stress[row["start"]:row["end"]] = s
        ramp[row["start"]:row["end"]] = np.minimum(t[row["start"]:row["end"]] - row["start_s"], block_s)
    x[:, 0] += 1.5 * np.sin(2 * np.pi * np.cumsum(hr) / fs + rs.rand() * 6.28)
    if C > 1:
        x[:, 1] = np.abs(x[:, 1]) * 0.2 + np.abs(level) + 0.0015 * a * ramp * stress
    if C > 2:
        x[:, 2] += np.sin(2 * np.pi * np.cumsum(br) / fs)
    for c in range(3, C):
        x[:, c] += 0.3 * a * stress * np.sin(2 * np.pi * (0.5 + 0.1 * c) * t)
    x = x * gain[None, :] + offs[None, :]
    if C > 1:
        x[:, 1] = np.abs(x[:, 1]) + 0.05
    x = np.ascontiguousarray(x, dtype=np.float64)
    if gaps is not None:
        plant_gaps(x, gaps, fs, seed)
    return x, table


SYNTHETIC_GAPS_FORMS = ("comma-separated drop=RATE (each sample of each channel missing with probability RATE in [0, 1)), "
                        "channel=INDEX:START_S:SECONDS (one channel off for a span), all=START_S:SECONDS (every channel off for a span) and, "
                        "with mixed-rate streams, stream=NAME:START_S:SECONDS (one stream off for a span); channel=, all= and stream= may repeat")


def parse_synthetic_gaps(spec) -> dict:
    """--synthetic-gaps SPEC -> {"drop": rate, "channel": [(index, start_s, seconds), ...], "all": [(start_s, seconds), ...],
    "stream": [(name, start_s, seconds), ...]}."""
    out = {"drop": 0.0, "channel": [], "all": [], "stream": []}
    try:
        for item in str(spec).split(","):
            key, _, val = item.partition("=")
            if key == "stream":
                name, _, span = val.partition(":")
                nums = [float(v) for v in span.split(":")]
                if not name or len(nums) != 2 or not (nums[0] >= 0 and nums[1] > 0):
                    raise ValueError
                out["stream"].append((name, nums[0], nums[1]))
                continue
            nums = [float(v) for v in val.split(":")]
            if key == "drop" and len(nums) == 1 and 0.0 <= nums[0] < 1.0:
                out["drop"] = nums[0]
            elif key == "channel" and len(nums) == 3 and nums[0] == int(nums[0]) and nums[0] >= 0 and nums[1] >= 0 and nums[2] > 0:
                out["channel"].append((int(nums[0]), nums[1], nums[2]))
            elif key == "all" and len(nums) == 2 and nums[0] >= 0 and nums[1] > 0:
                out["all"].append((nums[0], nums[1]))
            else:
                raise ValueError
    except ValueError:
        raise ValueError(f"--synthetic-gaps takes {SYNTHETIC_GAPS_FORMS}, got {spec!r}") from None
    return out


def gap_spans(spec, fs, L, stream=None) -> list:
    """The all-channel spans of a gaps spec as sorted, merged (first sample, one past last) pairs inside [0, L); with `stream`, a
    stream's name, the spans in which that stream is off: the all-channel spans and its own stream= spans."""
    g = parse_synthetic_gaps(spec)
    both = g["all"] + [(a, d) for name, a, d in g["stream"] if stream is not None and name == stream]
    spans = sorted((min(L, int(round(a * fs))), min(L, int(round((a + d) * fs)))) for a, d in both)
    out = []
    for a, b in spans:
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        elif b > a:
            out.append((a, b))
    return out


def plant_gaps(x, spec, fs, seed=42, streams=False):
    """Sets the samples a gaps spec names to NaN, in place.  The dropped samples are this function's own draws
    (RandomState(seed + 7919)), so the recording's values do not depend on the spec.  stream= spans belong to mixed-rate streams
    (make_synthetic_streams plants them, with streams=True here): a single-rate recording has no streams and refuses them."""
    g = parse_synthetic_gaps(spec)
    L, C = x.shape
    if g["stream"] and not streams:
        raise ValueError("--synthetic-gaps stream=NAME:START_S:SECONDS goes with mixed-rate streams (--streams)")
    if any(c >= C for c, _a, _d in g["channel"]):
        raise ValueError(f"--synthetic-gaps names a channel outside 0..{C - 1}")
    if g["drop"] > 0:
        x[np.random.RandomState(seed + 7919).rand(L, C) < g["drop"]] = np.nan
    for c, a, d in g["channel"]:
        x[int(round(a * fs)):int(round((a + d) * fs)), c] = np.nan
    for a, b in gap_spans(spec, fs, L):
        x[a:b, :] = np.nan
    return x


def make_synthetic_streams(phases, streams, fs=64.0, channels=CHANNELS6, seed=42, difficulty=1.0, block_s=60.0, gaps=None):
    """make_synthetic_recording as mixed-rate streams: `streams` is a list of resample.Stream (name, fs, columns — each column one
    of `channels`).  Returns ({name: (n, ncols) float64 at the stream's rate}, phase table in samples at `fs`, the monitor's rate).

    make_synthetic_recording is called once per distinct rate with the same seed, and each stream keeps its columns of the
    recording at its rate.  The planted phase effects — the stress terms of the rhythms' rates, of the EDA level and ramp and of the
    modulation, in seconds, and the subject's gain and offset — are the same at every rate.  The NOISE draws differ between rates:
    the generator draws a recording's per-sample noise first, so the per-block draws that follow it (a block's own heart rate, level
    and breathing rate around the planted ones) differ too, and a column at 4 Hz is not the 700 Hz column decimated.
    `gaps`: drop=, channel= (an index into `channels`) and all= are planted at every rate; stream=NAME:START_S:SECONDS sets that
    stream's rows of the span to NaN."""
    channels = list(channels)
    unknown = [c for st in streams for c in st.columns if c not in channels]
    if unknown:
        raise ValueError(f"the synthetic recording has the channels {channels}; the streams name {unknown}")
    spec = parse_synthetic_gaps(gaps) if gaps is not None else None
    if spec is not None and any(name not in [st.name for st in streams] for name, _a, _d in spec["stream"]):
        raise ValueError(f"--synthetic-gaps names a stream outside {[st.name for st in streams]}")
    at_rate, table = {}, None
    for st in streams:
        if st.fs not in at_rate:
            x, t = make_synthetic_recording(phases, fs=st.fs, channels=channels, seed=seed, difficulty=difficulty, block_s=block_s)
            if gaps is not None:
                plant_gaps(x, gaps, st.fs, seed, streams=True)
            at_rate[st.fs] = x
            table = t if table is None else table
    out = {}
    for st in streams:
        x = np.ascontiguousarray(at_rate[st.fs][:, [channels.index(c) for c in st.columns]])
        if gaps is not None:
            for a, b in gap_spans(gaps, st.fs, x.shape[0], stream=st.name):
                x[a:b, :] = np.nan
        out[st.name] = x
    return out, [dict(row, start=row["start_s"] * fs, end=row["end_s"] * fs) for row in table]
