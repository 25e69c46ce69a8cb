"""What an entropy-minimisation step (include/msig_tt.h) costs beside a plain train step, and what the whole
--adapt-entropy pass costs beside the LOSO it follows.

  steps   msig_tt_step at B = 64 (C = 6, T = 3840, K = 2) against msig_train_step, and msig_tt_step_multi over 15 folds against
          msig_train_step_multi, through the C ABI on buffers of their own.  The variants take turns run by run — three runs of 200
          steps each after a warm-up, every run timed by device events — so drift of the clocks hits them alike.  The fold batch of
          adaptation steps is timed with msig_multi.form_folds = 1 (what tta.EntropyAdapter passes: every fold keeps its stand-alone
          bits) and with form_folds = 15 (the train step's own choice of backward GRU form).
          --train-only times the train steps alone and makes no msig_tt call: with MSIG_LIB pointing at the PARENT commit's library
          it is the parent's msig_train_step[_multi] on the same machine in the same session.
  pass    the synthetic 15-fold LOSO through the driver, every fold's best_model.pt reloaded, and the adaptation of the 15 test
          subjects (all their windows, the flag's defaults) as ONE fold batch and as 15 single-model adaptations: median of
          --repeat host-timed, device-synchronised runs after a warm-up, building the adapter and copying the windows included.

    python tools/entropy_adapt_timing.py --work WORKDIR > profiles/entropy_adapt_timing.log
"""
import argparse
import contextlib
import ctypes as C
import re
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from multimodalsignal_amd import _lib as L                      # noqa: E402
from multimodalsignal_amd.runtime import Arenas, make_batch     # noqa: E402

Cc, T, K, B, NF = 6, 3840, 2, 64, 15
BETAS, EPS = (0.9, 0.999), 1e-8


class Bench(Arenas):
    def __init__(self, n, dev):
        self.n_flat = L.param_layout(Cc, K)[-1]
        self.ws_bytes = L.workspace_layout(B, Cc, T, K, True)[-1]
        flat = self.n_flat * 4
        super().__init__(n, dev, [("params", flat), ("grads", flat), ("exp_avg", flat), ("exp_avg_sq", flat), ("bn_state", 96 * 4), ("bn_count", 16),
                                  ("x", B * Cc * T * 4), ("y", B * 8), ("ws", self.ws_bytes), ("stats", 36 * 8), ("acc", 16)])
        g = torch.Generator().manual_seed(0)
        for s in range(n):
            self.view(s, "params", torch.float32).copy_(torch.randn(self.n_flat, generator=g) * 0.05)
            bn = self.view(s, "bn_state", torch.float32)
            bn[16:32] = 1.0
            bn[64:96] = 1.0
            self.view(s, "x", torch.float32).copy_(torch.randn(B * Cc * T, generator=g))
            self.view(s, "y", torch.int64).copy_(torch.randint(0, K, (B,), generator=g))
        self.step = 0

    def desc(self, training):
        b = make_batch(B, Cc, T, K, *(self.ptr(r) for r in ("x", "params", "bn_state", "bn_count", "ws")), self.ws_bytes, 2, training=training,
                       dropout_thr=128 if training else 0, labels=self.ptr("y"), grads=self.ptr("grads"), loss_acc=self.ptr("acc"))
        b.keep_for_backward = 0 if training else 1
        b.key_gru, b.key_head = 12345 + self.step, 54321 + self.step
        return b

    def train(self, form_folds=None):
        lib, st = L.lib(), self.stream()
        self.step += 1
        b = self.desc(True)
        if self.n == 1:
            L.check(lib.msig_train_step(C.byref(b), self.ptr("exp_avg"), self.ptr("exp_avg_sq"), 1e-4, *BETAS, EPS, 1e-4, self.step, st), "msig_train_step")
        else:
            m = self.multi(range(self.n), key_gru=[b.key_gru + s for s in range(self.n)], key_head=[b.key_head + s for s in range(self.n)],
                           lr=[1e-4] * self.n)
            m.form_folds = self.n if form_folds is None else form_folds
            L.check(lib.msig_train_step_multi(C.byref(b), C.byref(m), self.ptr("exp_avg"), self.ptr("exp_avg_sq"), *BETAS, EPS, 1e-4, self.step, st),
                    "msig_train_step_multi")

    def adapt(self, form_folds=1):
        from multimodalsignal_amd import tta
        lib, st = tta.lib(), self.stream()
        self.step += 1
        b, t = self.desc(False), tta.Tt()
        t.kind, t.select, t.diversity = 0, tta.SELECT_BN, 0.0
        t.beta1, t.beta2, t.eps, t.weight_decay = BETAS[0], BETAS[1], EPS, 0.0
        t.exp_avg, t.exp_avg_sq, t.stats = self.ptr("exp_avg"), self.ptr("exp_avg_sq"), self.ptr("stats")
        if self.n == 1:
            L.check(lib.msig_tt_step(C.byref(b), C.byref(t), 1e-4, self.step, st), "msig_tt_step")
        else:
            m = self.multi(range(self.n), lr=[1e-4] * self.n)
            m.form_folds = form_folds
            L.check(lib.msig_tt_step_multi(C.byref(b), C.byref(m), C.byref(t), self.step, st), "msig_tt_step_multi")


def run_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(fns, steps, runs, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            out[k].append(run_ms(fn, steps))
    return out


def report(title, times, base):
    print(title)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        extra = "" if k == base or base not in med else f"   {med[k] / med[base]:.3f} x {base}"
        print(f"  {k:<44} median {med[k]:.4f} ms per step   runs " + " ".join(f"{t:.4f}" for t in v) + extra)


def steps_section(dev, args):
    print(f"library: {L.LIB_PATH.name}" + ("   (train steps only: no msig_tt call is made)" if args.train_only else ""))
    print(f"B = {B}, C = {Cc}, T = {T}, K = {K}; {args.runs} runs of {args.steps} steps per variant after {args.warmup} warm-up steps, device events, "
          f"variants alternating run by run")
    one = Bench(1, dev)
    fns = {"msig_train_step": one.train}
    if not args.train_only:
        fns["msig_tt_step"] = one.adapt
    report("single model:", alternate(fns, args.steps, args.runs, args.warmup), "msig_train_step")
    assert bool(torch.isfinite(one.view(0, "params", torch.float32)).all())
    del one
    many = Bench(NF, dev)
    fns = {f"msig_train_step_multi ({NF} folds)": many.train}
    if not args.train_only:
        fns[f"msig_tt_step_multi ({NF} folds, form_folds = 1)"] = lambda: many.adapt(1)
        fns[f"msig_tt_step_multi ({NF} folds, form_folds = {NF})"] = lambda: many.adapt(NF)
    report(f"fold batch of {NF}:", alternate(fns, args.steps, args.runs, args.warmup), f"msig_train_step_multi ({NF} folds)")
    assert bool(torch.isfinite(many.view(NF - 1, "params", torch.float32)).all())
    if not args.train_only:
        L.profile_enable(True)
        try:
            for _ in range(20):
                many.adapt(1)
            torch.cuda.synchronize()
            rep = L.profile_report()
        finally:
            L.profile_enable(False)
        print("the two launches the step adds, mean of 20 fold-batch steps (the library's per-kernel events): "
              + ", ".join(f"{k} {1e3 * rep[k][1] / rep[k][0]:.1f} us" for k in ("tt_objective", "tt_adam")))
        print(f"launches per fold-batch adaptation step: {sum(v[0] for v in rep.values()) // 20}")


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def pass_section(dev, args):
    from multimodalsignal_amd import main as M
    from multimodalsignal_amd.dataset import WesadDataset
    from multimodalsignal_amd.models import CnnGruAttentionModel
    from multimodalsignal_amd.synth import ALL_SUBJECTS, CHANNELS6, make_synthetic_wesad
    from multimodalsignal_amd.tta import EntropyAdapter
    data = make_synthetic_wesad(args.work / "data")
    with contextlib.redirect_stdout(sys.stderr):             # the driver's own log lines stay out of the report
        M.main(["--synthetic", str(data), "--epochs", str(args.epochs), "--out", str(args.work / "out")])
    run = sorted((args.work / "out").glob("*/run_*"))[-1]
    wall = float(re.search(r"LOSO wall-clock: ([0-9.]+) s", (run / "cv_summary.txt").read_text(encoding="utf-8")).group(1))
    with open(data / "_channel_names.txt") as f:
        names = [ln.strip() for ln in f if ln.strip()]
    jobs = []
    for s in ALL_SUBJECTS:
        sd = torch.load(run / f"fold_test_on_{s}" / "best_model.pt", weights_only=True)
        C_, K_ = int(sd["cnn_encoder.0.weight"].shape[1]), int(sd["classifier.3.bias"].numel())
        model = CnnGruAttentionModel(C_, K_).to(dev)
        model.load_state_dict(sd)
        x, y = WesadDataset(data, [s], list(CHANNELS6)[:C_], names, classification_mode=M.CLASSIFICATION_MODE).device_tensors(dev)
        jobs.append(dict(model=model.eval(), x=x.contiguous(), y=y))
    eb = M.EVAL_BATCH_SIZE
    batch = timed(lambda: EntropyAdapter(jobs, eval_batch=eb).adapt(), args.repeat)
    single = timed(lambda: [EntropyAdapter([j], eval_batch=eb).adapt() for j in jobs], args.repeat)
    whole = timed(lambda: EntropyAdapter(jobs, eval_batch=eb).run(), args.repeat)
    res = EntropyAdapter(jobs, eval_batch=eb).run()
    n = sum(r["n"] for r in res)
    print(f"synthetic LOSO: {len(jobs)} folds, epochs budget {args.epochs}, C = {jobs[0]['x'].shape[1]}, T = {jobs[0]['x'].shape[2]}, "
          f"{n} test windows in all; adaptation at the flag's defaults (lr 1e-3, 1 epoch, diversity 0, batch 64, BatchNorm scale and shift)")
    print(f"LOSO wall-clock (cv_summary.txt): {wall:.2f} s")
    for label, (med, lo, hi) in (("one fold batch of 15", batch), ("15 single-model adaptations", single),
                                 ("one fold batch of 15 with the before / after evaluation (run())", whole)):
        print(f"adaptation, {label}: median {med * 1e3:.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}; {args.repeat} runs after a warm-up) "
              f"= {100 * med / wall:.3f} % of the LOSO wall-clock")
    print(f"fold batch / single: {batch[0] / single[0]:.3f}")
    mean = lambda key, sub: sum(r[key][sub] for r in res) / len(res)
    d_acc = [r["after"]["accuracy"] - r["before"]["accuracy"] for r in res]
    print(f"on the synthetic set (no subject shift by construction; says nothing about real WESAD): accuracy {mean('before', 'accuracy'):.4f} -> "
          f"{mean('after', 'accuracy'):.4f} (per-fold difference min {min(d_acc):+.4f} max {max(d_acc):+.4f}), mean prediction entropy "
          f"{mean('entropy', 'before'):.4f} -> {mean('entropy', 'after'):.4f}, {sum(r['flipped'] for r in res)} of {n} predictions flipped")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--work", type=Path, default=None, help="directory for the synthetic LOSO of the `pass` section (omitted: that section is skipped)")
    ap.add_argument("--train-only", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}")
    steps_section(dev, args)
    if args.work is not None and not args.train_only:
        pass_section(dev, args)


if __name__ == "__main__":
    main()
