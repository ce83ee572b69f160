"""What it costs to find a pair list's posterior envelopes on the device, beside copying the posterior rows out and
finding them on the host (profiles/envelope_pairs/probe.txt).  Measured, not gated.

One MI355X, one process.  The C3 database (20 000 profiles) against one 1 kbp query, every profile once, multi-hit, on a
float and on a double DB, hi = 0.5, lo = 0.1.  Two routes over the same list, alternating, one warm-up and three timed
runs each, medians and spans (max - min):

  rows route      posterior_pairs_scaled, then the Python loop of posterior_envelopes over the core rows (the only route
                  before envelope_pairs: its intervals are those of hi = lo = 0.5, without peak or sums).  With
                  --parent DIR it runs from a built checkout of the parent commit at DIR, loaded beside this build in
                  the same process, with a DB of its own of the same profiles; without, from this build, whose sweeps'
                  and combining kernel's objects are the parent's byte for byte and whose round loop is the parent's
                  behind a sink argument.
  envelope route  envelope_pairs(scaled=True), from the test-hooks build of this tree: the same objects but the
                  driver's, which there also reports the envelope kernels' own event time.

Per route: wall time of the whole route, the event-timed launches (posterior_scaled_kernel_ms beside envelope_kernel_ms,
and of the latter the envelope kernels' own part), the bytes copied to the host, the number of envelopes.

--big: a second line -- a list whose rows the rows route cannot hold in host memory on this box: pairs of the 1 kbp query
against the smallest profile, as many as make 24 bytes a row exceed MemAvailable (/proc/meminfo) at run time, unless
that is more than --big-max-rows rows (then the line says so and nothing runs).  Only the envelope route runs it.

    python profiles/envelope_pairs/probe.py [--nprof N] [--parent DIR] [--big] [--big-max-rows R] [--out FILE]
"""
import argparse
import importlib.util
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bench  # noqa: E402
from seq_windows_probe import med, sample_profiles  # noqa: E402

HI, LO = 0.5, 0.1


def span(v):
    return max(v) - min(v)


def mem_available():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) * 1024
    return 0


def load_parent(root):
    """the package of another checkout, under a name of its own; it loads its own libdcp_hip.so"""
    path = os.path.join(root, "deciphon-old_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location("deciphon_old_amd_parent", path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["deciphon_old_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--nprof", type=int, default=20000)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--big-max-rows", type=float, default=1.2e11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envelope_pairs", "probe.txt"))
    args = ap.parse_args()
    dcp = bench.load_product()
    old = load_parent(args.parent) if args.parent else dcp
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = np.asarray(bench.core_sizes_for("c3", args.nprof))
    query = np.random.default_rng(19).integers(0, 4, 1000, dtype=np.uint8)
    say(f"C3 database: {len(sizes)} profiles, core sizes {int(sizes.min())} .. {int(sizes.max())} (sum {int(sizes.sum())}),"
        f" one query of {len(query)} nt, every profile once, multi-hit, hi {HI}, lo {LO}")
    say("rows route from " + ("a build of the parent commit" if args.parent else "this build") + "; arguments: "
        + (" ".join(a for a in sys.argv[1:] if a != args.parent and a != args.out) or "none"))
    assert not args.parent or not hasattr(old.Scanner, "envelope_pairs")
    for precision in (32, 64):
        profs = sample_profiles(dcp, sizes, precision)
        sc = dcp.Scanner(0, lib=dcp.load_testhooks())
        sc.upload_db(profs)
        sc.upload_seqs([query])
        if args.parent:
            old_profs = sample_profiles(old, sizes, precision)
            osc = old.Scanner(0)
            osc.upload_db(old_profs)
            osc.upload_seqs([query])
        else:
            osc = sc
        say(f"f{precision} DB")
        pr = np.arange(len(sizes), dtype=np.uint32)
        sq = np.zeros(len(pr), np.uint32)
        wall_a, wall_b, ms_a, ms_b, ms_own, wall_loop = [], [], [], [], [], []
        for it in range(4):
            t0 = time.perf_counter()
            row_off, begin, end, core, fwd, bwd = osc.posterior_pairs_scaled(sq, pr)
            t1 = time.perf_counter()
            o = row_off.astype(np.int64)
            runs = [old.posterior_envelopes(core[o[i]:o[i + 1]], HI) for i in range(len(pr))]
            t2 = time.perf_counter()
            wall_a.append(t2 - t0), wall_loop.append(t2 - t1), ms_a.append(osc.posterior_scaled_kernel_ms)
            redo = osc.last_posterior_scaled_redo_pairs
            t0 = time.perf_counter()
            env_off, env, efwd, ebwd = sc.envelope_pairs(sq, pr, hi=HI, lo=LO)
            wall_b.append(time.perf_counter() - t0), ms_b.append(sc.envelope_kernel_ms), ms_own.append(sc.test_envelope_records_kernel_ms)
        assert np.array_equal(fwd.view(np.uint64), efwd.view(np.uint64)) and np.array_equal(bwd.view(np.uint64), ebwd.view(np.uint64))
        # the device's records on the host's rows: intervals, peak and core_max in bits
        for i in np.random.default_rng(1).choice(len(pr), 500, replace=False):
            want = dcp.posterior_envelope_records(begin[o[i]:o[i + 1]], end[o[i]:o[i + 1]], core[o[i]:o[i + 1]], HI, LO)
            got = env[int(env_off[i]):int(env_off[i + 1])]
            assert all(got[f].tobytes() == want[f].tobytes() for f in ("begin", "end", "peak", "core_max")), i
        nrows = int(row_off[-1])
        bytes_a = 24 * nrows + 16 * len(pr)
        bytes_b = 4 * len(pr) + 48 * len(env) + 16 * len(pr)
        wa, wb, ka, kb = wall_a[1:], wall_b[1:], ms_a[1:], ms_b[1:]
        say(f"  rows route:     wall {med(wa) * 1e3:8.1f} ms (span {span(wa) * 1e3:6.1f}), of it the Python loop {med(wall_loop[1:]) * 1e3:7.1f} ms;"
            f"  launches {med(ka):8.2f} ms (span {span(ka):5.2f});  {bytes_a / 1e6:8.1f} MB to the host;"
            f"  {sum(len(r) for r in runs)} intervals at hi = lo = {HI}; redo {redo}")
        say(f"  envelope route: wall {med(wb) * 1e3:8.1f} ms (span {span(wb) * 1e3:6.1f});  launches {med(kb):8.2f} ms (span {span(kb):5.2f}),"
            f" of them the envelope kernels {med(ms_own[1:]):6.3f} ms;  {bytes_b / 1e6:8.3f} MB to the host;  {len(env)} envelopes"
            f" in {int((np.diff(env_off.astype(np.int64)) > 0).sum())} pairs")
        extra = med(kb) - med(ka)
        say(f"  launches: envelope route - rows route = {extra:+.2f} ms, the rows route's span {span(ka):.2f} ms:"
            f" within it: {'yes' if extra <= span(ka) else 'NO'};  wall: envelope route below the rows route:"
            f" {'yes' if med(wb) < med(wa) else 'NO'} ({med(wa) / med(wb):.2f} times)")

        if args.big and precision == 32:
            L = len(query)
            avail = mem_available()
            npairs = int(avail // (24 * (L + 1))) + 1000
            rows = npairs * (L + 1)
            say(f"  a list the rows route cannot hold: MemAvailable {avail / 2**30:.1f} GiB, so {npairs} pairs of a {L} nt query"
                f" against the smallest profile ({int(sizes.min())} nodes): {rows:.3e} rows, {24 * rows / 2**30:.1f} GiB of rows")
            if rows > args.big_max_rows:
                say(f"    not run: more than --big-max-rows {args.big_max_rows:.2e} rows")
            else:
                small = int(np.argmin(sizes))
                stop = threading.Event()

                def beat():
                    t = time.perf_counter()
                    while not stop.wait(60):
                        print(f"    ... {time.perf_counter() - t:.0f} s", flush=True)

                th = threading.Thread(target=beat, daemon=True)
                th.start()
                t0 = time.perf_counter()
                env_off, env, efwd, ebwd = sc.envelope_pairs(np.zeros(npairs, np.uint32), np.full(npairs, small, np.uint32), hi=HI, lo=LO)
                wall = time.perf_counter() - t0
                stop.set()
                say(f"    envelope route: wall {wall:.1f} s, launches {sc.envelope_kernel_ms / 1e3:.1f} s, of them the envelope kernels"
                    f" {sc.test_envelope_records_kernel_ms:.1f} ms; {len(env)} envelopes, {(4 * npairs + 48 * len(env) + 16 * npairs) / 1e6:.1f} MB"
                    f" to the host; device rounds within 1 GiB of row records")
        sc.close()
        if args.parent:
            osc.close()
            del old_profs
        del profs

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
