"""Per-kernel dispatch statistics from a `rocprofv3 --kernel-trace` database (rocpd SQLite): count, mean / median / min duration
in microseconds, and the grid, grouped by kernel name and grid size (one batch size per grid).

    python tools/kernel_trace_stats.py RESULTS.db [NAME_SUBSTRING ...]
"""
import sqlite3
import statistics
import sys


def main():
    db, pats = sys.argv[1], sys.argv[2:]
    con = sqlite3.connect(db)
    groups = {}
    for name, dur, gx, gz in con.execute("select name, duration, grid_x, grid_z from kernels"):
        if pats and not any(p in name for p in pats):
            continue
        groups.setdefault((name.split("(")[0], gx, gz), []).append(dur / 1e3)
    print(f"{'kernel':<48} {'grid_x':>10} {'n':>5} {'mean_us':>10} {'median_us':>10} {'min_us':>10}")
    for (name, gx, gz), d in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
        print(f"{name[:48]:<48} {gx:>10} {len(d):>5} {statistics.mean(d):>10.2f} {statistics.median(d):>10.2f} {min(d):>10.2f}")


if __name__ == "__main__":
    main()
