"""Label-free entropy-minimisation adaptation to the test subject after LOSO (TENT; include/msig_tt.h).

``--adapt-bn`` re-estimates the BatchNorm running statistics of a finished fold on its new wearer's unlabelled windows and moves no
parameter.  This is the label-free method that does: every weight stays frozen except the BatchNorm scale and shift (``params="bn"``;
``"bn+gate"`` adds ChannelAttention's two matrices, ``"all"`` frees everything), and those descend the Shannon entropy of the
model's own predictions on the subject's windows (Wang et al., ICLR 2021) — with ``diversity`` > 0 less that weight times the entropy
of the batch's mean prediction (information maximisation, Liang et al., ICML 2020), which guards against collapse onto one class.
The model runs in EVAL mode throughout: running-statistic BatchNorm (the model's own, or AdaBN's when a job brings ``bn_state``),
no dropout, so a prediction never depends on its batch companions; the batch-statistic form of TENT is out of scope.

It reads the test subject's unlabelled windows: transductive, as ``--adapt-bn`` and the pipeline's per-subject z-score are.
Whether it helps on real WESAD is NOT known: the synthetic set has no subject shift by construction and cannot decide.

Nothing of the run is touched: the adapter works on COPIES of each model's parameters; the model, ``best_model.pt`` and every other
output stay as they are (``model.adapt_entropy(x, inplace=True)`` is the one call that loads the result into a model).
"""
from __future__ import annotations

import ctypes as C
import json
import math
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .adapt import SYNTHETIC_NOTE, batch_plan
from .calibrate import summarise
from .runtime import Arenas, make_batch, workspace_need
from .trainer import accuracy_and_weighted_f1

TT_ABI_VERSION = 1     # include/msig_tt.h MSIG_TT_ABI_VERSION
TT_MAX_BATCH = 2048    # msig_tt.h MSIG_TT_MAX_BATCH: rows of one step
TT_STATS = 36          # msig_tt.h MSIG_TT_STATS: fp64 statistics of one model
TT_S_ENT, TT_S_ROWS, TT_S_HQ, TT_S_STEPS, TT_S_P, TT_S_PRED = 0, 1, 2, 3, 4, 20      # msig_tt.h MSIG_TT_S_*
NPARAM = 28            # msig.h MSIG_NPARAM
P_GATE_W1, P_GATE_W2, P_BN1_G, P_BN1_B, P_BN2_G, P_BN2_B = 0, 1, 3, 4, 6, 7          # msig.h enum msig_param
SELECT_BN = (1 << P_BN1_G) | (1 << P_BN1_B) | (1 << P_BN2_G) | (1 << P_BN2_B)        # msig_tt.h MSIG_TT_SELECT_BN
SELECT_GATE = (1 << P_GATE_W1) | (1 << P_GATE_W2)                                    # MSIG_TT_SELECT_GATE
SELECT_ALL = (1 << NPARAM) - 1                                                       # MSIG_TT_SELECT_ALL
SELECT = {"bn": SELECT_BN, "bn+gate": SELECT_BN | SELECT_GATE, "all": SELECT_ALL}
ORDERS = ("shuffled", "recorded")
BETAS, EPS = (0.9, 0.999), 1e-8


class Tt(C.Structure):
    """msig_tt of include/msig_tt.h."""
    _fields_ = [("kind", C.c_int32), ("select", C.c_uint32), ("diversity", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("weight_decay", C.c_float), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("stats", C.c_void_p)]


_bound = None


def lib() -> C.CDLL:
    """libmsig_hip.so with include/msig_tt.h's calls bound (argument types as _lib.py binds the other headers'); a library that
    lacks them, or whose msig_tt differs from the mirror above, is an error — there is no fallback."""
    global _bound
    lb = L.lib()
    if _bound is lb:
        return lb
    vp, f, i32, i64 = C.c_void_p, C.c_float, C.c_int32, C.c_int64
    lb.msig_tt_abi_version.restype = C.c_int
    lb.msig_tt_struct_bytes.restype = i64
    if lb.msig_tt_abi_version() != TT_ABI_VERSION or lb.msig_tt_struct_bytes() != C.sizeof(Tt):
        raise RuntimeError(f"{L.LIB_PATH} has msig_tt.h ABI {lb.msig_tt_abi_version()} with msig_tt of {lb.msig_tt_struct_bytes()} bytes; this "
                           f"binding is {TT_ABI_VERSION} with {C.sizeof(Tt)}: rebuild the library")
    lb.msig_tt_objective.argtypes = [vp, i32, i32, f, vp, vp, vp]
    lb.msig_tt_objective_multi.argtypes = [vp, i32, i32, f, vp, vp, C.POINTER(L.Multi), vp]
    lb.msig_tt_adam.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_uint32, f, f, f, f, f, i64, vp]
    lb.msig_tt_adam_multi.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_uint32, f, f, f, f, i64, C.POINTER(L.Multi), vp]
    lb.msig_tt_step.argtypes = [C.POINTER(L.Batch), C.POINTER(Tt), f, i64, vp]
    lb.msig_tt_step_multi.argtypes = [C.POINTER(L.Batch), C.POINTER(L.Multi), C.POINTER(Tt), i64, vp]
    for name in ("msig_tt_objective", "msig_tt_objective_multi", "msig_tt_adam", "msig_tt_adam_multi", "msig_tt_step", "msig_tt_step_multi"):
        getattr(lb, name).restype = C.c_int
    _bound = lb
    return lb


# ---- settings -----------------------------------------------------------------------------------------------------------------------
def check_settings(lr=1e-3, epochs=1, diversity=0.0, batch=64, params="bn", seed=0, order="shuffled") -> dict:
    """The settings of an adaptation after their checks (ValueError): lr >= 0 and finite, epochs >= 1, diversity >= 0 and finite,
    batch in 1..TT_MAX_BATCH, params one of SELECT, order one of ORDERS."""
    def number(v, what):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"adapt_entropy {what} must be a number, got {v!r}") from None
        if not (0.0 <= v < math.inf):               # NaN fails both comparisons
            raise ValueError(f"adapt_entropy {what} must be finite and >= 0, got {v!r}")
        return v
    lr, diversity = number(lr, "lr"), number(diversity, "diversity")
    for v, what, lo, hi in ((epochs, "epochs", 1, 1 << 20), (batch, "batch", 1, TT_MAX_BATCH)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not (lo <= int(v) <= hi):
            raise ValueError(f"adapt_entropy {what} must be an integer in {lo}..{hi}, got {v!r}")
    if params not in SELECT:
        raise ValueError(f"adapt_entropy params must be one of {', '.join(SELECT)}, got {params!r}")
    if order not in ORDERS:
        raise ValueError(f"adapt_entropy order must be one of {', '.join(ORDERS)}, got {order!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or int(seed) < 0:
        raise ValueError(f"adapt_entropy seed must be a non-negative integer, got {seed!r}")
    return dict(lr=lr, epochs=int(epochs), diversity=diversity, batch=int(batch), params=params, seed=int(seed), order=order)


def parse_flag(value: Optional[str]) -> dict:
    """--adapt-entropy [LR[:EPOCHS[:DIVERSITY]]] -> {lr, epochs, diversity}; None or "" = the defaults.  ValueError on anything else."""
    out = dict(lr=1e-3, epochs=1, diversity=0.0)
    if value is None or value == "":
        return out
    parts = str(value).split(":")
    if len(parts) > 3 or any(p.strip() == "" for p in parts):
        raise ValueError(f"expected LR[:EPOCHS[:DIVERSITY]], got {value!r}")
    try:
        out["lr"] = float(parts[0])
        if len(parts) > 1:
            out["epochs"] = int(parts[1])
        if len(parts) > 2:
            out["diversity"] = float(parts[2])
    except ValueError:
        raise ValueError(f"expected LR[:EPOCHS[:DIVERSITY]] with a number, an integer and a number, got {value!r}") from None
    check_settings(**out)
    return out


def epoch_order(n: int, seed: int, epoch: int, order: str = "shuffled") -> np.ndarray:
    """The order in which epoch `epoch` of a subject with `n` windows visits them: a permutation that is a function of (n, seed,
    epoch) alone, or the recording order.  Recording order is class-blocked by protocol phase — single-class batches, under which
    entropy minimisation collapses fastest — which is why shuffled is the default."""
    if order == "recorded":
        return np.arange(n, dtype=np.int64)
    return np.random.default_rng([int(seed), int(epoch)]).permutation(n).astype(np.int64)


def selected_keys(engine, params: str) -> List[str]:
    """The state_dict names of the tensors `params` lets move, for the engine's model kind."""
    return [k for i, k in engine.keys if (SELECT[params] >> i) & 1]


class EntropyAdapter(Arenas):
    """Adapts one model, or several as a fold batch (one set of launches per batch for all of them), by entropy minimisation.

    jobs: dicts with
        model     the fold's model (CnnGruAttentionModel / CnnGruModel, either depth), on the GPU
        x         (N, C, T) float32 device tensor: the new subject's windows, unlabelled
        y         optional (N,) labels: run() then also reports accuracy and weighted F1 before and after on the same windows, and
                  the steps report the online CrossEntropy (the labels never reach the objective: the same bits with and without)
        bn_state  optional 96 floats: running statistics to adapt under instead of the model's own (adapt.BnAdapter's adapted_state)
    The jobs of an adapter share the model kind, depth, C, K and T, and either all or none bring `y`; N is per job.
    batched=False runs one msig_tt_step per job instead of one msig_tt_step_multi per group: the same bits.

    run() returns one dict per job (see there).  adapted_params(i) is job i's adapted flat parameters (a view of the working copy),
    adapted_tensors(i) the tensors the selection let move, under the reference's state_dict names."""

    def __init__(self, jobs: Sequence[dict], lr=1e-3, epochs=1, diversity=0.0, batch=64, params="bn", seed=0, order="shuffled",
                 batched: bool = True, eval_batch: int = 1024):
        if not (1 <= len(jobs) <= L.MAX_FOLDS):
            raise ValueError(f"1..{L.MAX_FOLDS} folds per adapter")
        self.settings = check_settings(lr, epochs, diversity, batch, params, seed, order)
        self.jobs, self.batched = list(jobs), bool(batched)
        self.engines = [j["model"].engine() for j in self.jobs]
        e0, x0 = self.engines[0], self.jobs[0]["x"]
        for j, e in zip(self.jobs, self.engines):
            x = j["x"]
            if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] != e.C or x.shape[0] < 1:
                raise ValueError(f"expected a non-empty float32 (N, {e.C}, T) GPU tensor, got {x.dtype} {tuple(x.shape)} on {x.device}")
            if (e.kind, e.gru_layers, e.C, e.K, e.n_flat, x.shape[2]) != (e0.kind, e0.gru_layers, e0.C, e0.K, e0.n_flat, x0.shape[2]):
                raise ValueError("the folds of an adapter share the model kind, depth, channels, classes and window length")
            if j.get("y") is not None and tuple(j["y"].shape) != (x.shape[0],):
                raise ValueError(f"expected ({x.shape[0]},) labels, got {tuple(j['y'].shape)}")
            if j.get("bn_state") is not None and j["bn_state"].numel() != L.BN_STATE_FLOATS:
                raise ValueError(f"bn_state holds {L.BN_STATE_FLOATS} floats, got {j['bn_state'].numel()}")
        with_y = [j.get("y") is not None for j in self.jobs]
        if any(with_y) and not all(with_y):
            raise ValueError("either every job of an adapter brings labels or none does (a fold batch shares its descriptor)")
        self.labelled = all(with_y)
        self.kind, self.C, self.K, self.T = e0.kind, e0.C, e0.K, int(x0.shape[2])
        self.sizes = [int(j["x"].shape[0]) for j in self.jobs]
        self.batch = max(1, min(self.settings["batch"], max(self.sizes)))
        self.eval_batch = max(1, int(eval_batch))
        self.plan = batch_plan(self.sizes, self.batch)
        self.ws_bytes = workspace_need(sorted({b for _, b, _ in self.plan}), self.C, self.T, self.K, True)      # kept for a backward: the training layout
        flat = e0.n_flat * 4
        super().__init__(len(self.jobs), e0.device, [("params", flat), ("grads", flat), ("exp_avg", flat), ("exp_avg_sq", flat),
                                                     ("bn_state", L.BN_STATE_FLOATS * 4), ("bn_count", 16), ("x", self.batch * self.C * self.T * 4),
                                                     ("y", self.batch * 8), ("ws", self.ws_bytes), ("stats", TT_STATS * 8), ("acc", 16)])
        self.objective: List[List[float]] = [[] for _ in self.jobs]      # per job, per epoch: the mean objective
        self.online: List[List[dict]] = [[] for _ in self.jobs]          # per job, per epoch: the steps' own CrossEntropy and accuracy (labelled)
        self._ran = False

    # ---- descriptors ------------------------------------------------------------------------------------------------------------
    def _desc(self, B: int, slot: int = 0) -> L.Batch:
        """The descriptor of a step on B windows in arena `slot` (the *_multi call is given arena 0's): eval mode, kept for a backward."""
        b = make_batch(B, self.C, self.T, self.K, *(self.ptr(r, slot) for r in ("x", "params", "bn_state", "bn_count", "ws")), self.ws_bytes,
                       self.engines[0].gru_layers, labels=self.ptr("y", slot) if self.labelled else None, grads=self.ptr("grads", slot),
                       loss_acc=self.ptr("acc", slot) if self.labelled else None)
        b.keep_for_backward = 1
        return b

    def _tt(self, slot: int = 0) -> Tt:
        t = Tt()
        t.kind, t.select, t.diversity = L.FT_KINDS[self.kind], SELECT[self.settings["params"]], self.settings["diversity"]
        t.beta1, t.beta2, t.eps, t.weight_decay = BETAS[0], BETAS[1], EPS, 0.0
        t.exp_avg, t.exp_avg_sq, t.stats = self.ptr("exp_avg", slot), self.ptr("exp_avg_sq", slot), self.ptr("stats", slot)
        return t

    # ---- the adaptation -----------------------------------------------------------------------------------------------------------
    def adapt(self):
        """`epochs` passes over every job's windows in steps of `batch`, on copies of the models' parameters and state."""
        lb, st, s = lib(), self.stream(), self.settings
        for k, (j, eng) in enumerate(zip(self.jobs, self.engines)):
            if getattr(eng, "scatter", None) is not None:
                eng.scatter()                                       # the one-layer model: its parameters into the padded layout
            self.view(k, "params", torch.float32).copy_(eng.params)
            src = j.get("bn_state")
            self.view(k, "bn_state", torch.float32).copy_(eng.bn_state if src is None else src.to(torch.float32).reshape(-1))
            self.view(k, "bn_count", torch.int64)[:2].copy_(eng.bn_count)
            for r in ("grads", "exp_avg", "exp_avg_sq"):
                self.view(k, r).zero_()
        steps = [0] * self.n
        wf = self.C * self.T
        for epoch in range(s["epochs"]):
            order = [torch.from_numpy(epoch_order(n, s["seed"], epoch, s["order"])).to(self.device) for n in self.sizes]
            for k in range(self.n):
                self.view(k, "stats").zero_()
                self.view(k, "acc").zero_()
            for i, b, slots in self.plan:
                for k in slots:
                    idx = order[k][i:i + b]
                    self.view(k, "x", torch.float32)[:b * wf].copy_(self.jobs[k]["x"].index_select(0, idx).reshape(-1))
                    if self.labelled:
                        self.view(k, "y", torch.int64)[:b].copy_(self.jobs[k]["y"].to(torch.int64).index_select(0, idx))
                    steps[k] += 1
                if self.batched:
                    m = self.multi(slots, lr=[s["lr"]] * len(slots), steps=[steps[k] for k in slots])
                    L.check(lb.msig_tt_step_multi(C.byref(self._desc(b)), C.byref(m), C.byref(self._tt()), 1, st), "msig_tt_step_multi")
                else:
                    for k in slots:
                        L.check(lb.msig_tt_step(C.byref(self._desc(b, k)), C.byref(self._tt(k)), s["lr"], steps[k], st), "msig_tt_step")
            for k in range(self.n):
                v = self.view(k, "stats", torch.float64).cpu().numpy()
                self.objective[k].append(float(v[TT_S_ENT] / v[TT_S_ROWS] - s["diversity"] * v[TT_S_HQ] / v[TT_S_STEPS]))
                if self.labelled:
                    a = self.view(k, "acc", torch.float64).cpu().numpy()
                    self.online[k].append({"cross_entropy": float(a[0] / self.sizes[k]), "accuracy": float(a[1] / self.sizes[k])})
        self._ran = True

    def _evaluate(self, eng, params_ptr: Optional[int], bn_state: torch.Tensor, x):
        """(predictions, per-window prediction entropy in fp64) of fresh eval-mode forwards of the model over all windows, with
        `params_ptr` (None: its own) and `bn_state`."""
        pred, ent = [], []
        for i in range(0, x.shape[0], self.eval_batch):
            xb = x[i:i + self.eval_batch]
            b = eng._batch(xb, None, False, 0.0, 0, 0)
            if params_ptr is not None:
                b.params = params_ptr
            b.bn_state = bn_state.data_ptr()
            b.loss_acc = None
            eng.forward_desc(b)
            pred.append(eng.region("PRED", torch.int32, (xb.shape[0],)).clone())
            lp = torch.log_softmax(eng.region("LOGITS", torch.float32, (xb.shape[0], self.K)).to(torch.float64), dim=1)
            ent.append(-(lp.exp() * lp).sum(dim=1))
        return torch.cat(pred).cpu().numpy().astype(np.int64), torch.cat(ent).cpu().numpy()

    def run(self) -> List[dict]:
        """One dict per job: n; entropy {before, after}: the mean prediction entropy over ALL windows by fresh eval forwards; shares
        {before, after}: the predicted-class shares, the collapse indicator — reported, never hidden; flipped: windows whose
        prediction changed; objective: the per-epoch mean objective from the steps' statistics; with `y` before / after
        {accuracy, f1_score} and online: the steps' own CrossEntropy and accuracy per epoch.  `before` is the model as it stands;
        a job that brought `bn_state` also reports `start` (accuracy, f1_score, entropy, shares under those statistics)."""
        if not self._ran:
            self.adapt()
        out = []
        share = lambda p: [float(v) for v in np.bincount(p, minlength=self.K) / max(len(p), 1)]
        for k, (j, eng) in enumerate(zip(self.jobs, self.engines)):
            x = j["x"]
            p0, h0 = self._evaluate(eng, None, eng.bn_state, x)
            p1, h1 = self._evaluate(eng, self.ptr("params", k), self.view(k, "bn_state", torch.float32), x)
            r = {"n": self.sizes[k], "entropy": {"before": float(h0.mean()), "after": float(h1.mean())},
                 "shares": {"before": share(p0), "after": share(p1)}, "flipped": int((p0 != p1).sum()), "objective": list(self.objective[k])}
            y = None if j.get("y") is None else j["y"].cpu().numpy().astype(np.int64)
            score = lambda p: dict(zip(("accuracy", "f1_score"), accuracy_and_weighted_f1(y, p)))
            if y is not None:
                r.update(before=score(p0), after=score(p1), online=list(self.online[k]))
            if j.get("bn_state") is not None:
                ps, hs = self._evaluate(eng, None, j["bn_state"].to(torch.float32).reshape(-1).contiguous(), x)
                r["start"] = dict(score(ps) if y is not None else {}, entropy=float(hs.mean()), shares=share(ps))
            out.append(r)
        return out

    def adapted_params(self, slot: int) -> torch.Tensor:
        """Job `slot`'s adapted parameters in the flat layout (a view of the adapter's working copy)."""
        if not self._ran:
            self.adapt()
        return self.view(slot, "params", torch.float32)

    def adapted_tensors(self, slot: int) -> dict:
        """The tensors the selection let move, adapted, under the reference's state_dict names and in its shapes."""
        eng, flat = self.engines[slot], self.adapted_params(slot)
        if getattr(eng, "scatter", None) is not None:
            views = eng.small_views(flat.index_select(0, eng.index))
        else:
            views = eng.named_param_views(flat)
        return {k: views[k].clone() for k in selected_keys(eng, self.settings["params"]) if k in views}


# ---- the adaptation table of a run --------------------------------------------------------------------------------------------------
def settings_of(cfg) -> dict:
    """The settings of a configuration (--adapt-entropy ...), as entropy_adaptation.txt / .json name them."""
    s = dict(cfg["adapt_entropy"])
    s.update(params=cfg.get("adapt_entropy_params", "bn"), batch=int(cfg.get("adapt_entropy_batch", 64)), order="shuffled", seed=0)
    if cfg.get("adapt_bn") is not None:
        s["adabn_alpha"] = float(cfg["adapt_bn"])
    return s


def format_entropy(table: dict, settings: Optional[dict] = None, synthetic: bool = False) -> str:
    three = any("start" in f for f in table["folds"])
    lines = ["Label-free entropy-minimisation adaptation (TENT): every weight frozen but the selected tensors, which descend the entropy "
             "of the model's own predictions on the test subject's unlabelled windows (transductive, as the per-subject z-score is); "
             "eval-mode BatchNorm throughout; all columns on the SAME windows; difference = adapted - LOSO",
             "Whether this helps on real WESAD is not known."]
    if three:
        lines.append("With --adapt-bn the adaptation starts from the AdaBN statistics: LOSO, AdaBN, AdaBN + entropy.")
    if settings:
        lines.append("settings: " + ", ".join(f"{k} = {v}" for k, v in settings.items()))
    if synthetic:
        lines.append("NOTE: " + SYNTHETIC_NOTE + ".")
    mid = f" {'AdaBN acc':>10}" if three else ""
    midf = f" {'AdaBN F1':>9}" if three else ""
    lines += ["", f"  {'subject':<10} {'n':>6} {'LOSO acc':>10}{mid} {'adapt acc':>10} {'diff':>9}   {'LOSO F1':>9}{midf} {'adapt F1':>9} {'diff':>9}   "
                  f"{'entropy':>8} {'->':>8} {'flipped':>8}   predicted-class shares before -> after"]
    for f in table["folds"]:
        b, a, s = f["before"], f["after"], f.get("start")
        ma = f" {s['accuracy']:>10.4f}" if three and s else (f" {'':>10}" if three else "")
        mf = f" {s['f1_score']:>9.4f}" if three and s else (f" {'':>9}" if three else "")
        sh = lambda v: "[" + " ".join(f"{p:.2f}" for p in v) + "]"
        lines.append(f"  {f['subject']:<10} {f.get('n', 0):>6} {b['accuracy']:>10.4f}{ma} {a['accuracy']:>10.4f} {a['accuracy'] - b['accuracy']:>+9.4f}   "
                     f"{b['f1_score']:>9.4f}{mf} {a['f1_score']:>9.4f} {a['f1_score'] - b['f1_score']:>+9.4f}   "
                     f"{f['entropy']['before']:>8.4f} {f['entropy']['after']:>8.4f} {f['flipped']:>8}   {sh(f['shares']['before'])} -> {sh(f['shares']['after'])}")
    lines.append("")
    for m, label in (("accuracy", "accuracy"), ("f1_score", "weighted F1")):
        sm = table["summary"][m]
        adabn = ""
        if three:
            v = np.array([f["start"][m] for f in table["folds"] if "start" in f], dtype=np.float64)
            adabn = f"   AdaBN {v.mean():.4f} ± {v.std():.4f}"
        lines.append(f"  {label}: LOSO {sm['before']['mean']:.4f} ± {sm['before']['std']:.4f}{adabn}   adapted {sm['after']['mean']:.4f} ± "
                     f"{sm['after']['std']:.4f}   mean paired difference {sm['difference']['mean']:+.4f} ± {sm['difference']['std']:.4f}   "
                     f"adapted wins {table['wins'][m]} of {table['n_folds']} folds, ties {table['ties'][m]}, losses {table['losses'][m]}")
    return "\n".join(lines) + "\n"


def write_entropy_adaptation(run_output_dir, folds: Sequence[dict], settings: Optional[dict] = None, synthetic: bool = False) -> Path:
    """entropy_adaptation.json (calibrate.summarise of the folds' before / after + settings) and entropy_adaptation.txt."""
    run_output_dir = Path(run_output_dir)
    table = summarise(folds)
    doc = dict(table, settings=dict(settings or {}))
    if synthetic:
        doc["note"] = SYNTHETIC_NOTE
    (run_output_dir / "entropy_adaptation.json").write_text(json.dumps(doc, indent=1))
    path = run_output_dir / "entropy_adaptation.txt"
    path.write_text(format_entropy(table, settings, synthetic), encoding="utf-8")
    return path
