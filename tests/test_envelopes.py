"""Envelope records from posterior rows on the host: dcp_posterior_envelope_records (the twin of the device kernels of
tests/test_envelopes_gpu.py), and dcp_envelopes_regions, which hands envelopes to cut_regions.  CPU only.

The yardstick is a plain numpy restatement of the two-threshold rule written here (restate): intervals, peak and
core_max are decided by comparisons and must agree in bits.  A sum of n doubles, added in any order, lies within
(n - 1) 2^-53 sum|term| of the exact sum: every sum, the twin's here and the device's in tests/test_envelopes_gpu.py, is
held to that against the exact sum in rational arithmetic (sums_within); and two such sums of the same terms are held to
n 2^-52 sum|term| of each other (sums_agree), the bound between device and twin."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_both_strands import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (2, 1), (2, 7), (5, 30), (64, 100), (65, 60), (40, 333))  # tests/test_posterior_pairs.py's (M, L)
EXACT = ("pair", "begin", "end", "peak", "core_max")
SUMS = (("core_sum", 2, 1), ("begin_sum", 0, 0), ("end_sum", 1, 1))  # field, row, offset of base i's term in the row


def restate(begin, end, core, hi, lo, min_len, pair=0):
    """[(pair, b, e, peak, core_max, core terms, begin terms, end terms)] of the kept runs, in order"""
    L = len(core) - 1
    above = np.zeros(L + 2, bool)
    above[1:L + 1] = core[1:] >= lo  # above[i + 1]: base i is in a run
    starts = np.nonzero(above[1:] & ~above[:-1])[0]
    ends = np.nonzero(~above[1:] & above[:-1])[0]
    out = []
    for b, e in zip(starts.tolist(), ends.tolist()):
        vals = core[b + 1:e + 1]
        if e - b < min_len or not vals.max() >= hi:
            continue
        peak = b + int(np.argmax(vals))  # (argmax: the first of equals)
        out.append((pair, b, e, peak, core[peak + 1], vals, begin[b:e], end[b + 1:e + 1]))
    return out


def sums_within(rec, want, what=""):
    """each of the record's three sums within (n - 1) 2^-53 sum|term| of the exact sum of the run's own n terms, in
    rational arithmetic: the bound of a sum in any order, and nothing more; the worst ratio"""
    worst = 0.0
    n = want[2] - want[1]
    for (name, _, _), terms in zip(SUMS, want[5:]):
        assert len(terms) == n
        exact = sum((Fraction(float(x)) for x in terms), Fraction(0))
        bound = Fraction(n - 1, 2 ** 53) * sum((abs(Fraction(float(x))) for x in terms), Fraction(0))
        err = abs(Fraction(float(rec[name])) - exact)
        assert err <= bound, (what, name, float(rec[name]), float(exact), float(err), float(bound))
        worst = max(worst, float(err / bound) if bound else 0.0)
    return worst


def sums_agree(rec, other, want, what=""):
    """two records of the same run, their sums in different orders: each pair of sums within n 2^-52 sum|term| of each
    other, n the run's length, the terms the run's own (want: restate's tuple); the worst ratio"""
    worst = 0.0
    n = want[2] - want[1]
    for (name, _, _), terms in zip(SUMS, want[5:]):
        bound = Fraction(n, 2 ** 52) * sum((abs(Fraction(float(x))) for x in terms), Fraction(0))
        err = abs(Fraction(float(rec[name])) - Fraction(float(other[name])))
        assert err <= bound, (what, name, float(rec[name]), float(other[name]), float(err), float(bound))
        worst = max(worst, float(err / bound) if bound else 0.0)
    return worst


def same_records(got, wants, what=""):
    """records against restate's tuples: the exact fields in bits, each sum within the any-order bound of the exact sum"""
    assert len(got) == len(wants), (what, len(got), len(wants))
    for k, (rec, want) in enumerate(zip(got, wants)):
        assert tuple(int(rec[f]) for f in EXACT[:4]) == tuple(int(x) for x in want[:4]), (what, k, rec, want[:4])
        assert bits(np.array([rec["core_max"]])) == bits(np.array([want[4]], np.float64)), (what, k)
        sums_within(rec, want, (what, k))


def exact_fields(env):
    return [env[f].tobytes() for f in EXACT]


def random_rows(rng, L, style):
    """rows [L + 1] whose core row has runs: smooth bumps, noise, or plateaus of equal values"""
    begin, end = rng.random(L + 1) * 0.1, rng.random(L + 1) * 0.1
    if style == "noise":
        core = rng.random(L + 1)
    elif style == "plateau":
        core = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], L + 1)
    else:
        x = np.arange(L + 1)
        core = np.clip(np.sin(x / 7.0 + rng.random() * 6) * 0.6 + 0.4 + rng.normal(0, 0.05, L + 1), 0.0, 1.0)
    core[0] = 0.0
    end[0] = 0.0
    return begin, end, core


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 200])
def test_against_posterior_envelopes_and_the_restatement_on_random_rows(dcp, L):
    rng = np.random.default_rng(2600 + L)
    for style in ("bumps", "noise", "plateau"):
        for _ in range(6):
            begin, end, core = random_rows(rng, L, style)
            for hi, min_len in ((0.5, 1), (0.25, 3), (0.9, 1), (0.0, 1), (1.5, 1)):
                env = dcp.posterior_envelope_records(begin, end, core, hi, None, min_len)
                assert env.dtype == dcp.ENVELOPE_DTYPE and env.itemsize == 48
                assert [(int(r["begin"]), int(r["end"])) for r in env] == dcp.posterior_envelopes(core, hi, min_len)
                same_records(env, restate(begin, end, core, hi, hi, min_len), (L, style, hi, min_len))
            for hi, lo, min_len in ((0.5, 0.1, 1), (0.9, 0.25, 2), (0.75, 0.5, 1), (1.0, 0.0, 1), (0.5, -1.0, 1)):
                env = dcp.posterior_envelope_records(begin, end, core, hi, lo, min_len)
                same_records(env, restate(begin, end, core, hi, lo, min_len), (L, style, hi, lo, min_len))


@pytest.mark.parametrize("M,L", SHAPES)
def test_against_posterior_envelopes_on_the_posterior_shapes(dcp, oracle64, M, L):
    from test_posterior_pairs import case
    for multi in (True, False):
        t8, em, ei, en, xt, seq = case(oracle64, M, L, multi)
        begin, end, core, fwd, bwd = dcp.posterior_tables(t8, em, ei, en, xt, seq)
        for thr in (0.5, 0.1, 0.9, float(np.median(core[1:]))):
            for min_len in (1, 3):
                env = dcp.posterior_envelope_records(begin, end, core, thr, None, min_len)
                assert [(int(r["begin"]), int(r["end"])) for r in env] == dcp.posterior_envelopes(core, thr, min_len)
                same_records(env, restate(begin, end, core, thr, thr, min_len), (M, L, multi, thr, min_len))
        lo = float(np.quantile(core[1:], 0.3))
        hi = float(np.quantile(core[1:], 0.8))
        same_records(dcp.posterior_envelope_records(begin, end, core, hi, lo), restate(begin, end, core, hi, lo, 1), (M, L, multi))


def rows_of(core_bases):
    """rows [L + 1] around the given per-base core values; begin and end are distinct known values"""
    core = np.concatenate([[0.0], np.asarray(core_bases, np.float64)])
    L = len(core) - 1
    begin = (np.arange(L + 1) + 1) / 1024.0
    end = (np.arange(L + 1) + 1) / 4096.0
    end[0] = 0.0
    return begin, end, core


def test_edge_rows(dcp):
    rec = dcp.posterior_envelope_records
    # all above: one run over everything; its sums are the rows'
    b, e, c = rows_of([0.75] * 10)  # (every value and every sum below is exact in binary)
    env = rec(b, e, c, 0.5)
    assert [(r["begin"], r["end"], r["peak"]) for r in env] == [(0, 10, 0)] and env[0]["pair"] == 0
    assert env[0]["core_sum"] == np.sum(c[1:]) and env[0]["begin_sum"] == np.sum(b[:10]) and env[0]["end_sum"] == np.sum(e[1:])
    # all below
    assert len(rec(b, e, c, 0.9)) == 0
    # a run to the last base, and one that never reaches hi
    b, e, c = rows_of([0.0, 0.3, 0.3, 0.0, 0.2, 0.6, 0.8, 0.8])
    env = rec(b, e, c, 0.5, 0.1)
    assert [(r["begin"], r["end"], r["peak"], r["core_max"]) for r in env] == [(4, 8, 6, 0.8)]
    assert env[0]["begin_sum"] == np.sum(b[4:8]) and env[0]["end_sum"] == np.sum(e[5:9])
    assert [(r["begin"], r["end"]) for r in rec(b, e, c, 0.3, 0.1)] == [(1, 3), (4, 8)]
    # min_len at a run's length and one above
    assert [(r["begin"], r["end"]) for r in rec(b, e, c, 0.3, 0.1, 2)] == [(1, 3), (4, 8)]
    assert [(r["begin"], r["end"]) for r in rec(b, e, c, 0.3, 0.1, 3)] == [(4, 8)]
    assert [(r["begin"], r["end"]) for r in rec(b, e, c, 0.3, 0.1, 4)] == [(4, 8)]
    assert len(rec(b, e, c, 0.3, 0.1, 5)) == 0
    # cap one short: the count is true, the first cap are written
    n = C.c_uint(99)
    out = np.zeros(2, dcp.ENVELOPE_DTYPE)
    out["pair"][1] = 77
    P = lambda a: a.ctypes.data  # noqa: E731
    assert dcp.lib.dcp_posterior_envelope_records(P(b), P(e), P(c), 8, 0.3, 0.1, 1, P(out), 1, C.byref(n)) == 0
    assert n.value == 2 and (out[0]["begin"], out[0]["end"]) == (1, 3) and out["pair"][1] == 77 and out["end"][1] == 0
    # values of -1e-17, as 1 - (a sum that rounds past 1) leaves them, with lo = 0: they are in no run
    b, e, c = rows_of([0.4, -1e-17, 0.0, 0.6, -1e-17, -1e-17, 0.0])
    env = rec(b, e, c, 0.5, 0.0)
    assert [(r["begin"], r["end"], r["peak"]) for r in env] == [(2, 4, 3)]
    assert [(r["begin"], r["end"]) for r in rec(b, e, c, 0.0, 0.0)] == [(0, 1), (2, 4), (6, 7)]
    same_records(rec(b, e, c, 0.0, 0.0), restate(b, e, c, 0.0, 0.0, 1))
    # equal maxima: the first; -0.0 equals 0.0
    b, e, c = rows_of([0.5, 0.9, 0.2, 0.9, 0.9])
    assert rec(b, e, c, 0.5, 0.1)[0]["peak"] == 1
    b, e, c = rows_of([-0.0, 0.0, -0.0])
    env = rec(b, e, c, 0.0, 0.0)
    assert env[0]["peak"] == 0 and np.signbit(env[0]["core_max"])
    # a NaN is in no run
    b, e, c = rows_of([0.6, float("nan"), 0.6])
    assert [(r["begin"], r["end"]) for r in rec(b, e, c, 0.5)] == [(0, 1), (2, 3)]
    # no bases at all
    assert len(rec(np.zeros(1), np.zeros(1), np.zeros(1))) == 0


def test_refusals_write_nothing(dcp):
    b, e, c = rows_of([0.7] * 10)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    out = np.zeros(4, dcp.ENVELOPE_DTYPE)
    out["pair"] = 77
    n = C.c_uint(99)
    nan = float("nan")

    def run(b_=b, e_=e, c_=c, L=10, hi=0.5, lo=0.5, out_=out, cap=4, n_=n):
        return dcp.lib.dcp_posterior_envelope_records(P(b_), P(e_), P(c_), L, hi, lo, 1, P(out_), cap, None if n_ is None else C.byref(n_))

    for change in (dict(hi=nan), dict(lo=nan), dict(hi=nan, lo=nan), dict(hi=0.2, lo=0.3), dict(b_=None), dict(e_=None),
                   dict(c_=None), dict(out_=None), dict(n_=None)):
        assert run(**change) == dcp.RC_EINVAL, change
        assert n.value == 99 and (out["pair"] == 77).all() and not out["end"].any(), change
    assert run(out_=None, cap=0) == 0 and n.value == 1  # counting needs no array
    assert run(b_=None, e_=None, c_=None, L=0) == 0 and n.value == 0  # nor do no rows
    assert run() == 0 and n.value == 1 and out["pair"][0] == 0 and (out["pair"][1:] == 77).all()
    for bad in (dict(hi=nan), dict(lo=nan), dict(hi=0.1, lo=0.2)):
        with pytest.raises(dcp.DcpError):
            dcp.posterior_envelope_records(b, e, c, **bad)
    with pytest.raises(dcp.DcpError):
        dcp.posterior_envelope_records(b, e[:-1], c)


def envelopes(dcp, recs):
    env = np.zeros(len(recs), dcp.ENVELOPE_DTYPE)
    for k, (pair, b, e) in enumerate(recs):
        env[k]["pair"], env[k]["begin"], env[k]["end"], env[k]["peak"] = pair, b, e, b
    return env


def test_envelopes_regions(dcp):
    seq_idx = np.array([2, 0, 2, 1], np.uint32)  # the list's sequences; pair 2 repeats pair 0's
    seq_len = np.array([50, 7, 100], np.uint32)
    env = envelopes(dcp, [(0, 10, 20), (0, 0, 100), (1, 3, 50), (3, 0, 7), (2, 95, 100), (1, 0, 1)])
    src, begin, length, pair = dcp.envelopes_regions(env, seq_idx, seq_len)
    assert src.dtype == begin.dtype == length.dtype == pair.dtype == np.uint32
    assert src.tolist() == [2, 2, 0, 1, 2, 0] and pair.tolist() == [0, 0, 1, 3, 2, 1]
    assert begin.tolist() == [10, 0, 3, 0, 95, 0] and length.tolist() == [10, 100, 47, 7, 5, 1]
    # a flank: clipped at both ends
    src, begin, length, pair = dcp.envelopes_regions(env, seq_idx, seq_len, flank=5)
    assert begin.tolist() == [5, 0, 0, 0, 90, 0] and length.tolist() == [20, 100, 50, 7, 10, 6]
    # larger than every sequence: the whole sequence, also at the largest flank there is
    for flank in (1000, 2 ** 32 - 1):
        src, begin, length, pair = dcp.envelopes_regions(env, seq_idx, seq_len, flank=flank)
        assert not begin.any() and length.tolist() == [100, 100, 50, 7, 100, 50]
    # none
    assert all(len(a) == 0 for a in dcp.envelopes_regions(envelopes(dcp, []), seq_idx, seq_len))

    # refusals write nothing
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    outs = [np.full(len(env), 9, np.uint32) for _ in range(4)]

    def run(env_=env, sq=seq_idx, npairs=4, sl=seq_len, nseqs=3, outs_=outs):
        return dcp.lib.dcp_envelopes_regions(P(env_), len(env), P(sq), npairs, P(sl), nseqs, 2, *[P(o) for o in outs_])

    def bad(k, **fields):
        e = env.copy()
        for f, v in fields.items():
            e[k][f] = v
        return e

    for change in (dict(env_=bad(5, pair=4)), dict(npairs=3), dict(nseqs=2), dict(env_=bad(4, end=101)),
                   dict(env_=bad(5, begin=1)), dict(env_=bad(5, begin=2)), dict(env_=None), dict(sq=None), dict(sl=None),
                   dict(outs_=[None] + outs[1:]), dict(outs_=outs[:3] + [None]),
                   dict(sq=np.array([2, 0, 3, 1], np.uint32))):
        assert run(**change) == dcp.RC_EINVAL, change
        assert all((o == 9).all() for o in outs), change
    assert run() == 0 and outs[0].tolist() == [2, 2, 0, 1, 2, 0]
    with pytest.raises(dcp.DcpError):
        dcp.envelopes_regions(bad(0, end=10), seq_idx, seq_len)


def test_envelopes_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_envelopes.c with the host model alone (no device code) under ASan + UBSan, as a program of its
    own."""
    obj, exe = str(tmp_path / "asan_envelopes.o"), str(tmp_path / "asan_envelopes")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_envelopes.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_envelopes ok" in r.stdout
