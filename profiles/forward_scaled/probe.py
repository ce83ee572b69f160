"""What the scaled probability-space Forward sweep costs beside the log-space one, and how far its scores lie from it
(profiles/forward_scaled/probe.txt).  Measured, not gated.

One MI355X, one process.
1. Pair list: the C3 database (20 000 profiles) against one 1 kbp query, every profile once, multi-hit, on a float and
   on a double DB: forward_pairs_scaled by dcp_gpu_forward_scaled_kernel_ms and forward_pairs by
   dcp_gpu_forward_kernel_ms (HIP events around the launches) in the same process, alternating; one warm-up and three
   timed runs each, medians and spans (max - min).  Then the same by core size: 1 - 64, 65 - 256, 257 - 1 024 and wider,
   with the redo count.  Beside the times: the largest |scaled - log space| on both scores, and for a float DB the
   allowance A = n(L, M) (delta + 2^-51) of the pair where the distance is largest (tests/test_forward_scaled.py).
2. Calibration: the 200 x 100 nt dense scan of DESIGN 23 on a float DB by forward_dense_scaled beside forward_dense
   (forward_dense_kernel_ms), the same schedule.

    python profiles/forward_scaled/probe.py [--nprof N] [--out FILE]
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


def recorded_delta():
    with open(os.path.join(ROOT, "profiles", "forward_scaled", "factor_delta.txt")) as f:
        for line in f:
            if line.startswith("delta "):
                return float(line.split()[1])
    raise SystemExit("no delta recorded")


def span(v):
    return max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_scaled", "probe.txt"))
    args = ap.parse_args()
    dcp = bench.load_product()
    delta = recorded_delta()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = np.asarray(bench.core_sizes_for("c3", args.nprof))
    query = np.random.default_rng(19).integers(0, 4, 1000, dtype=np.uint8)
    say(f"C3 database: {len(sizes)} profiles, core sizes {int(sizes.min())} .. {int(sizes.max())} (sum {int(sizes.sum())}),"
        f" one query of {len(query)} nt, every profile once, multi-hit; factor rule delta {delta:.4e}")
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
                sn, sa = sc.forward_pairs_scaled(sq, pr)
                new.append(sc.forward_scaled_kernel_ms)
                redo = sc.last_forward_scaled_redo_pairs
                ln, la = sc.forward_pairs(sq, pr)
                old.append(sc.forward_kernel_ms)
            assert np.isfinite(sa).all() and np.isfinite(sn).all() and np.isfinite(la).all()
            gcell = float(sizes[pr].sum()) * len(query) / 1e9
            f, o = med(new[1:]), med(old[1:])
            faster = o - f > span(new[1:]) + span(old[1:])
            say(f"  {name:>12}: {len(pr):6d} pairs, {gcell:7.3f} Gcell, redo {redo};  scaled {f:8.2f} ms (span {span(new[1:]):5.2f}) ="
                f" {gcell / f * 1e3:7.2f} Gcell/s;  log space {o:8.2f} ms (span {span(old[1:]):5.2f}) = {gcell / o * 1e3:6.2f} Gcell/s;"
                f"  ratio {o / f:5.2f}, faster by more than the spans: {'yes' if faster else 'NO'}")
            dn, da = np.abs(sn - ln), np.abs(sa - la)
            i = int(np.argmax(da))
            line = f"  {'':>12}  largest |scaled - log space|: null {dn.max():.3e}, alt {da.max():.3e} (profile of {int(sizes[pr[i]])} nodes"
            if precision == 32:
                n = len(query) * (int(sizes[pr[i]]) + 2) + 2
                line += f": n = {n}, A = {n * (delta + 2.0 ** -51):.3e}"
            else:
                line += f": 2^-32 (|x| + 1) = {2.0 ** -32 * (abs(la[i]) + 1.0):.3e}"
            say(line + ")")
        sc.close()
        del profs

    # the calibration of DESIGN 23: 200 random sequences of 100 nt against the C3 database, a float DB
    profs = sample_profiles(dcp, sizes, 32)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.random_seqs(200, 100, 2027)
    new, old = [], []
    for it in range(4):
        sc.forward_dense_scaled()
        new.append(sc.forward_dense_kernel_ms())
        redo = sc.last_forward_scaled_redo_pairs
        got = sc.forward_scores()
        sc.forward_dense()
        old.append(sc.forward_dense_kernel_ms())
        ref = sc.forward_scores()
    fin = np.isfinite(ref[1])
    assert np.array_equal(fin, np.isfinite(got[1]))
    gcell = float(sizes.sum()) * 200 * 100 / 1e9
    f, o = med(new[1:]), med(old[1:])
    say(f"calibration, f32 DB, 200 x 100 nt dense ({gcell:.1f} Gcell), redo {redo}: forward_dense_scaled {f / 1e3:7.3f} s (span"
        f" {span(new[1:]) / 1e3:.3f}) = {gcell / f * 1e3:7.2f} Gcell/s;  forward_dense {o / 1e3:7.3f} s (span {span(old[1:]) / 1e3:.3f}) ="
        f" {gcell / o * 1e3:6.2f} Gcell/s;  ratio {o / f:5.2f};  largest |scaled - log space| alt {np.abs(got[1][fin] - ref[1][fin]).max():.3e}")
    sc.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
