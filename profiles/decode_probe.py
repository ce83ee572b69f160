#!/usr/bin/env python3
"""What the decode of hit paths costs on the host and on the device, on the mixed-length job of
profiles/r04/host_scan_probe.txt section 3: 3 000 sequences of 100 nt .. 10 kbp against the C3-shaped database of
20 000 profiles (about 4 000 hits, about 6 M path steps).

Compiles profiles/decode_probe.c against the float host library and runs it with the process bound to 2 and to 16
CPUs (the product rows' OpenMP team is sized by the CPUs the process may run on).  Each run prints four jobs: host
decode and device decode (scan_cfg.device_decode), each with the database loaded and with it resident; "device decode"
is the wall time of dcp_gpu_decode_paths over the job's passes, "product rows" the rows phase of scan_run_source.
The host-decode jobs run the code path of the commit before the feature unchanged (the flag defaults to off).

    python profiles/decode_probe.py [--profiles 20000] [--seqs 3000] [--cpus 2,16] [--out profiles/decode_paths/probe.txt]

Not part of the tests; needs an MI355X."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "deciphon-old_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiles", type=int, default=20000)
    ap.add_argument("--seqs", type=int, default=3000)
    ap.add_argument("--cpus", default="2,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "decode_probe")
        subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "profiles", "decode_probe.c"), "-o", exe, "-L", LIBDIR, "-ldeciphon_host",
                               "-ldcp_hip", "-lm", "-fopenmp", "-Wl,-rpath," + LIBDIR])
        db = os.path.join(tmp, "probe.dcp")
        mine = sorted(os.sched_getaffinity(0))
        for n in [int(x) for x in args.cpus.split(",")]:
            cpus = set(mine[:n])
            lines.append("== %d CPUs%s" % (len(cpus), "" if len(cpus) == n else " (the process may run on no more)"))
            out = subprocess.run([exe, db, str(args.profiles), str(args.seqs)], stdout=subprocess.PIPE, text=True, check=True,
                                 preexec_fn=lambda: os.sched_setaffinity(0, cpus)).stdout
            lines += out.splitlines()
            print("\n".join(lines[-len(out.splitlines()) - 1:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
