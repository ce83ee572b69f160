"""What posterior rows cost by the scaled probability-space sweeps beside the log-space ones, and how far the rows lie
apart (profiles/posterior_scaled/probe.txt).  Measured, not gated.

One MI355X, one process.  The C3 database (20 000 profiles) against one 1 kbp query, every profile once, multi-hit, on a
float and on a double DB: posterior_pairs_scaled by dcp_gpu_posterior_scaled_kernel_ms and posterior_pairs by
dcp_gpu_posterior_kernel_ms (HIP events around the rounds' launches, the combining kernel included) in the same process,
alternating; one warm-up and three timed runs each, medians and spans (max - min).  Then the same by core size: 1 - 64,
65 - 256, 257 - 1 024 and wider, with the redo count.  Beside the times: the largest |scaled - log space| over the three
rows and on the two alt scores.

    python profiles/posterior_scaled/probe.py [--nprof N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench  # noqa: E402
from seq_windows_probe import med, sample_profiles  # noqa: E402

CLASSES = ((1, 64), (65, 256), (257, 1024), (1025, 4096))


def span(v):
    return max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_scaled", "probe.txt"))
    args = ap.parse_args()
    dcp = bench.load_product()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = np.asarray(bench.core_sizes_for("c3", args.nprof))
    query = np.random.default_rng(19).integers(0, 4, 1000, dtype=np.uint8)
    say(f"C3 database: {len(sizes)} profiles, core sizes {int(sizes.min())} .. {int(sizes.max())} (sum {int(sizes.sum())}),"
        f" one query of {len(query)} nt, every profile once, multi-hit")
    for precision in (32, 64):
        profs = sample_profiles(dcp, sizes, precision)
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs([query])
        say(f"f{precision} DB")
        whole = np.arange(len(sizes), dtype=np.uint32)
        lists = [("all", whole)] + [(f"{lo} - {hi}", whole[(sizes >= lo) & (sizes <= hi)]) for lo, hi in CLASSES]
        for name, pr in lists:
            if len(pr) == 0:
                continue
            sq = np.zeros(len(pr), np.uint32)
            new, old = [], []
            for it in range(4):
                got = sc.posterior_pairs_scaled(sq, pr)
                new.append(sc.posterior_scaled_kernel_ms)
                redo = sc.last_posterior_scaled_redo_pairs
                ref = sc.posterior_pairs(sq, pr)
                old.append(sc.posterior_kernel_ms)
            assert np.isfinite(got[4]).all() and np.isfinite(got[5]).all() and not np.isnan(got[3]).any()
            gcell = float(sizes[pr].sum()) * len(query) / 1e9
            f, o = med(new[1:]), med(old[1:])
            faster = o - f > span(new[1:]) + span(old[1:])
            say(f"  {name:>12}: {len(pr):6d} pairs, {gcell:7.3f} Gcell, redo {redo};  scaled {f:8.2f} ms (span {span(new[1:]):5.2f});"
                f"  log space {o:8.2f} ms (span {span(old[1:]):5.2f});  ratio {o / f:5.2f},"
                f" faster by more than the spans: {'yes' if faster else 'NO'}")
            d = [float(np.abs(got[i] - ref[i]).max()) for i in (1, 2, 3, 4, 5)]
            say(f"  {'':>12}  largest |scaled - log space|: begin {d[0]:.3e}, end {d[1]:.3e}, core {d[2]:.3e}, alt_fwd {d[3]:.3e},"
                f" alt_bwd {d[4]:.3e}; largest |alt_fwd - alt_bwd| {float(np.abs(got[4] - got[5]).max()):.3e}")
        sc.close()
        del profs

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
