"""What label-free BatchNorm adaptation (adapt.BnAdapter) costs beside the LOSO it follows.

Runs the synthetic 15-fold LOSO through the driver, reloads every fold's best_model.pt and times the adaptation of the 15 test
subjects (all their windows, alpha = 1) two ways: as ONE fold batch (one BnAdapter over 15 jobs) and as 15 single-model adaptations
one after the other.  Each figure is the median of `--repeat` runs after one warm-up, device-synchronised, and includes building
the adapter (its arenas) and copying the windows in.  The LOSO wall-clock is the driver's own (cv_summary.txt).

    python tools/adapt_bn_timing.py --work /tmp/adapt_bn_timing [--epochs 20] > profiles/adapt_bn_timing.log
"""
import argparse
import re
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from multimodalsignal_amd import main as M                      # noqa: E402
from multimodalsignal_amd.adapt import BnAdapter                # noqa: E402
from multimodalsignal_amd.dataset import WesadDataset           # noqa: E402
from multimodalsignal_amd.models import CnnGruAttentionModel    # noqa: E402
from multimodalsignal_amd.synth import ALL_SUBJECTS, CHANNELS6, make_synthetic_wesad      # noqa: E402


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--work", type=Path, required=True)
    ap.add_argument("--epochs", type=int, default=M.EPOCHS)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    data = make_synthetic_wesad(args.work / "data")
    M.main(["--synthetic", str(data), "--epochs", str(args.epochs), "--out", str(args.work / "out")])
    run = sorted((args.work / "out").glob("*/run_*"))[-1]
    wall = float(re.search(r"LOSO wall-clock: ([0-9.]+) s", (run / "cv_summary.txt").read_text(encoding="utf-8")).group(1))
    with open(data / "_channel_names.txt") as f:
        names = [ln.strip() for ln in f if ln.strip()]
    jobs = []
    for s in ALL_SUBJECTS:
        sd = torch.load(run / f"fold_test_on_{s}" / "best_model.pt", weights_only=True)
        C_, K = int(sd["cnn_encoder.0.weight"].shape[1]), int(sd["classifier.3.bias"].numel())
        model = CnnGruAttentionModel(C_, K).to(dev)
        model.load_state_dict(sd)
        x, y = WesadDataset(data, [s], list(CHANNELS6)[:C_], names, classification_mode=M.CLASSIFICATION_MODE).device_tensors(dev)
        jobs.append(dict(model=model.eval(), x=x.contiguous(), y=y))
    eb = M.EVAL_BATCH_SIZE
    batch = timed(lambda: BnAdapter(jobs, eval_batch=eb).adapt(), args.repeat)
    single = timed(lambda: [BnAdapter([j], eval_batch=eb).adapt() for j in jobs], args.repeat)
    res = BnAdapter(jobs, eval_batch=eb).run()
    n = sum(r["n"] for r in res)
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"synthetic LOSO: {len(jobs)} folds, epochs budget {args.epochs}, C = {jobs[0]['x'].shape[1]}, T = {jobs[0]['x'].shape[2]}, "
          f"{n} test windows in all, eval batch {eb}")
    print(f"LOSO wall-clock (cv_summary.txt): {wall:.2f} s")
    for label, (med, lo, hi) in (("one fold batch of 15", batch), ("15 single-model adaptations", single)):
        print(f"adaptation, {label}: median {med * 1e3:.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}; {args.repeat} runs after a warm-up) "
              f"= {100 * med / wall:.3f} % of the LOSO wall-clock")
    print(f"fold batch / single: {batch[0] / single[0]:.3f}")
    d_acc = [r["after"]["accuracy"] - r["before"]["accuracy"] for r in res]
    print(f"accuracy LOSO -> adapted on the synthetic set (no subject shift by construction; says nothing about real WESAD): "
          f"mean {sum(r['before']['accuracy'] for r in res) / len(res):.4f} -> {sum(r['after']['accuracy'] for r in res) / len(res):.4f}, "
          f"per-fold difference min {min(d_acc):+.4f} max {max(d_acc):+.4f}")


if __name__ == "__main__":
    main()
