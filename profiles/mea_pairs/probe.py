"""What the posterior-decoded alignment of a pair list costs beside its posterior rows and its Forward scores
(profiles/mea_pairs/probe.txt).  Measured, not gated.

One MI355X, one process.  The C3 database (20 000 profiles) against one 1 kbp query as a pair list, every profile once
(the list of profiles/forward_pairs/probe.py), on a float and on a double DB: mea_pairs by dcp_gpu_mea_kernel_ms beside
posterior_pairs by dcp_gpu_posterior_kernel_ms and forward_pairs by dcp_gpu_forward_kernel_ms (HIP events around the
launches), the three calls alternating; one warm-up and three timed runs each, medians and the three runs' spread; the
rounds the matrices' budget makes of the list and the bytes a cell they imply.

--product DIR measures the package in DIR instead of the repository's (a build of another commit); a library without
mea_pairs gets the other two alone: that is how the parent commit's forward_pairs and posterior_pairs are held beside
this one's.

    python profiles/mea_pairs/probe.py [--nprof N] [--product DIR] [--out FILE]
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench  # noqa: E402
from seq_windows_probe import med, sample_profiles  # noqa: E402

CELL_BYTES, ROW_BYTES, BUDGET = 34, 88, 8 << 30  # csrc/dcp_gpu.hip: kMeaCellBytes, kMeaRowBytes, the default budget


def load(product):
    if not product:
        return bench.load_product()
    path = os.path.join(product, "__init__.py")
    spec = importlib.util.spec_from_file_location("deciphon_old_amd", path, submodule_search_locations=[product])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["deciphon_old_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def rounds_of(sizes, L):
    """the rounds of consecutive pairs dcp_gpu_mea_pairs makes of the list under the default budget"""
    n, used = 1, 0
    for M in sizes:
        need = (L + 1) * (int(M) * CELL_BYTES + ROW_BYTES)
        if used and used + need > BUDGET:
            n, used = n + 1, 0
        used += need
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=20000)
    ap.add_argument("--product", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mea_pairs", "probe.txt"))
    args = ap.parse_args()
    dcp = load(args.product)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = np.asarray(bench.core_sizes_for("c3", args.nprof))
    query = np.random.default_rng(19).integers(0, 4, 1000, dtype=np.uint8)
    say(f"C3 database: {len(sizes)} profiles, core sizes {int(sizes.min())} .. {int(sizes.max())} (sum {int(sizes.sum())}),"
        f" one query of {len(query)} nt, every profile once, multi-hit")
    gcell = float(sizes.sum()) * len(query) / 1e9
    cells = float(sizes.sum()) * (len(query) + 1)
    for precision in (32, 64):
        profs = sample_profiles(dcp, sizes, precision)
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs([query])
        has = hasattr(sc, "mea_pairs")
        pr = np.arange(len(sizes), dtype=np.uint32)
        sq = np.zeros(len(pr), np.uint32)
        fwd, post, mea, wall = [], [], [], []
        for it in range(4):
            null, alt = sc.forward_pairs(sq, pr)
            fwd.append(sc.forward_kernel_ms)
            sc.posterior_pairs(sq, pr)
            post.append(sc.posterior_kernel_ms)
            if has:
                t0 = time.perf_counter()
                paths, posts, gain, afwd = sc.mea_pairs(sq, pr)
                wall.append((time.perf_counter() - t0) * 1e3)
                mea.append(sc.mea_kernel_ms)
        f, p = med(fwd[1:]), med(post[1:])
        say(f"f{precision} DB: {len(pr)} pairs, {gcell:.3f} Gcell")
        say(f"  forward_pairs   {f:9.2f} ms (runs {min(fwd[1:]):.2f} .. {max(fwd[1:]):.2f}) = {gcell / f * 1e3:6.2f} Gcell/s")
        say(f"  posterior_pairs {p:9.2f} ms (runs {min(post[1:]):.2f} .. {max(post[1:]):.2f}) = {gcell / p * 1e3:6.2f} Gcell/s;"
            f"  posterior / Forward time {p / f:5.2f}")
        if has:
            m = med(mea[1:])
            assert np.array_equal(afwd.view(np.uint64), alt.view(np.uint64))
            nsteps = sum(len(x) for x in paths)
            say(f"  mea_pairs       {m:9.2f} ms (runs {min(mea[1:]):.2f} .. {max(mea[1:]):.2f}) = {gcell / m * 1e3:6.2f} Gcell/s;"
                f"  mea / posterior time {m / p:5.2f};  the call, copies and host work included, {med(wall[1:]):.0f} ms")
            say(f"  {rounds_of(sizes, len(query))} rounds of at most {BUDGET >> 30} GiB: {CELL_BYTES} bytes a cell and {ROW_BYTES} a row,"
                f" {(cells * CELL_BYTES + len(pr) * (len(query) + 1) * ROW_BYTES) / 1e9:.1f} GB in all; {nsteps} steps;"
                f" alt_fwd has forward_pairs' bits; mean gain {float(np.mean(gain[np.isfinite(gain)])):.1f} of {len(query)} bases")
        else:
            say("  (no mea_pairs in this build)")
        sc.close()
        del profs

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
