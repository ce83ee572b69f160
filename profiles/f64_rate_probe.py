"""Rate of the f64 row sweep (viterbi64_kernel) beside the f32 row sweep on the same C2-sized job:
1 000 profiles (bench.py's c2 core sizes, 100..300 nodes) x 1 000 queries x 300 nt, multi-hit.
Each kernel: one warm-up scan, then `--reps` timed scans (HIP events around the scan's launches).
Prints one JSON line.  python profiles/f64_rate_probe.py [--nprof 1000 --nq 1000 --qlen 300 --reps 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import _load_product  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=1000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--qlen", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dcp = _load_product()
    sizes = bench.core_sizes_for("c2", a.nprof)
    seqs = list(bench.make_queries(0, a.nq, a.qlen))
    out = {"nprof": a.nprof, "nq": a.nq, "qlen": a.qlen}
    cfg = dcp.ProteinCfg(dcp.ENTRY_DIST_OCCUPANCY, 0.01)
    for prec in (32, 64):
        profs = [dcp.ProteinProfile.sample(0xC2 + p, int(sizes[p]), cfg, precision=prec) for p in range(a.nprof)]
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs(seqs)
        ms = []
        for r in range(a.reps + 1):
            sc.scan(True, False, 10.0, keep_scores=False, kernel=dcp.KERNEL_ROWSWEEP)
            if r:
                ms.append(sc.last_scan_ms)
        cells = sc.cells
        out[f"f{prec}_ms"] = ms
        out[f"f{prec}_gcells"] = cells / (min(ms) * 1e-3) / 1e9
        out[f"f{prec}_hits"] = int(len(sc.hits()))
        sc.close()
    out["cells"] = int(cells)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
