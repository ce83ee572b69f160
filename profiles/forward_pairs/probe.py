"""What Forward scores of a pair list cost (profiles/forward_pairs/probe.txt).  Measured, not gated.

One MI355X, one process.  The C3 database (20 000 profiles) against one 1 kbp query as a pair list, every profile once,
on a float and on a double DB: forward_pairs by dcp_gpu_forward_kernel_ms (HIP events around the launches), beside
scan_pairs of the same list by last_scan_ms; one warm-up and three timed runs each, medians.  Then the same split by
core size: 1 - 64, 65 - 256, 257 - 1 024 and larger.

For the record, in the planted world of tests/test_scan_pairs.py: alt - null by Forward and by Viterbi for the two
planted pairs, and the largest value among the other pairs.

    python profiles/forward_pairs/probe.py [--nprof N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from seq_windows_probe import med, sample_profiles  # noqa: E402

CLASSES = ((1, 64), (65, 256), (257, 1024), (1025, 4096))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_pairs", "probe.txt"))
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
            fwd, vit = [], []
            for it in range(4):
                null, alt = sc.forward_pairs(sq, pr)
                fwd.append(sc.forward_kernel_ms)
                sc.scan_pairs(sq, pr, True, False, float("-inf"))
                vit.append(sc.last_scan_ms)
            assert np.isfinite(alt).all() and np.isfinite(null).all()
            gcell = float(sizes[pr].sum()) * len(query) / 1e9
            f, v = med(fwd[1:]), med(vit[1:])
            say(f"  {name:>12}: {len(pr):6d} pairs, {gcell:7.3f} Gcell;  forward_pairs {f:9.2f} ms = {gcell / f * 1e3:7.2f} Gcell/s;"
                f"  scan_pairs {v:8.2f} ms = {gcell / v * 1e3:7.1f} Gcell/s;  Forward / Viterbi time {f / v:6.1f}")
        sc.close()
        del profs

    # the planted world of tests/test_scan_pairs.py: queries 5 and 6 carry the genes of profiles 1 and 5
    from oracle_py import Oracle
    from test_scan_pairs import pair_world
    for precision in (32, 64):
        profs, seqs, nl, al = pair_world(dcp, Oracle(precision), precision)[:4]
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs(seqs)
        sq = np.arange(len(seqs), dtype=np.uint32).repeat(len(profs))
        pr = np.tile(np.arange(len(profs), dtype=np.uint32), len(seqs))
        null, alt = sc.forward_pairs(sq, pr)
        sc.close()
        with np.errstate(invalid="ignore"):
            fwd = (alt - null).reshape(len(seqs), len(profs))
            vit = np.asarray(al, np.float64) - np.asarray(nl, np.float64)
        say(f"planted world, f{precision}: alt - null by Forward / by Viterbi")
        rest = np.ones(fwd.shape, bool)
        for q, p in ((5, 1), (6, 5)):
            rest[q, p] = False
            say(f"  planted (query {q}, {len(seqs[q])} nt; profile {p}, {profs[p].core_size} nodes): {fwd[q, p]:9.3f} / {vit[q, p]:9.3f}")
        rest[:, -1] = False  # the profile with positive MD / DD is no probability model
        fin = rest & np.isfinite(fwd) & np.isfinite(vit)
        say(f"  largest among the other {int(fin.sum())} finite pairs: {fwd[fin].max():9.3f} / {vit[fin].max():9.3f}")

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
