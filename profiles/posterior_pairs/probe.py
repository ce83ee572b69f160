"""What the posterior rows of a pair list cost beside its Forward scores (profiles/posterior_pairs/probe.txt,
DESIGN.md 20).  Measured, not gated.

One MI355X, one process.  The C3 database (20 000 profiles) against one 1 kbp query as a pair list, every profile once
(the list of profiles/forward_pairs/probe.py), on a float and on a double DB: posterior_pairs by
dcp_gpu_posterior_kernel_ms beside forward_pairs by dcp_gpu_forward_kernel_ms (HIP events around the launches), the two
calls alternating; one warm-up and three timed runs each, medians and the three runs' spread.

--product DIR measures the package in DIR instead of the repository's (a build of another commit); a library without
posterior_pairs gets forward_pairs alone: that is how the parent commit's forward_pairs is held beside this one's.

    python profiles/posterior_pairs/probe.py [--nprof N] [--product DIR] [--out FILE]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench  # noqa: E402
from seq_windows_probe import med, sample_profiles  # noqa: E402


def load(product):
    if not product:
        return bench.load_product()
    path = os.path.join(product, "__init__.py")
    spec = importlib.util.spec_from_file_location("deciphon_old_amd", path, submodule_search_locations=[product])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["deciphon_old_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprof", type=int, default=20000)
    ap.add_argument("--product", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_pairs", "probe.txt"))
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
    for precision in (32, 64):
        profs = sample_profiles(dcp, sizes, precision)
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs([query])
        has = hasattr(sc, "posterior_pairs")
        pr = np.arange(len(sizes), dtype=np.uint32)
        sq = np.zeros(len(pr), np.uint32)
        fwd, post = [], []
        for it in range(4):
            null, alt = sc.forward_pairs(sq, pr)
            fwd.append(sc.forward_kernel_ms)
            if has:
                row_off, begin, end, core, afwd, abwd = sc.posterior_pairs(sq, pr)
                post.append(sc.posterior_kernel_ms)
        f = med(fwd[1:])
        say(f"f{precision} DB: {len(pr)} pairs, {gcell:.3f} Gcell")
        say(f"  forward_pairs   {f:9.2f} ms (runs {min(fwd[1:]):.2f} .. {max(fwd[1:]):.2f}) = {gcell / f * 1e3:6.2f} Gcell/s")
        if has:
            p = med(post[1:])
            fin = np.isfinite(afwd)
            gap = float(np.max(np.abs(abwd[fin] - afwd[fin]) / (np.abs(afwd[fin]) + 1.0)))
            assert np.array_equal(afwd.view(np.uint64), alt.view(np.uint64))
            say(f"  posterior_pairs {p:9.2f} ms (runs {min(post[1:]):.2f} .. {max(post[1:]):.2f}) = {gcell / p * 1e3:6.2f} Gcell/s;"
                f"  posterior / Forward time {p / f:5.2f}")
            say(f"  {int(row_off[-1])} rows; alt_fwd has forward_pairs' bits; largest |alt_bwd - alt_fwd| / (|alt_fwd| + 1) {gap:.2e};"
                f" expected domains per pair: mean {float(begin.sum()) / len(pr):.3f}")
        else:
            say("  (no posterior_pairs in this build)")
        sc.close()
        del profs

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
