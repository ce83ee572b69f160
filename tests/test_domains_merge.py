"""dcp_domains_locate and dcp_domains_merge (csrc/dcp_model.cpp; locate_domains / merge_domains): pure host arithmetic,
checked on the CPU.

locate: against a Python restatement, over cut and uncut batches of one and two strands, windows at offset 0, at an odd
phase and anchored at the source's end, domains that touch either end of their resident sequence, and the refusals.
merge: hand-made cases for every clause of the rule, then 20 000 random domains against the rule restated as the
plain quadratic loop.  tests/c/asan_domains.c drives both calls under ASan + UBSan in a stand-alone program."""
import os
import subprocess
import time

import numpy as np
import pytest

from test_c_host import ROOT


def domains(dcp, intervals):
    d = np.zeros(len(intervals), dcp.DOMAIN_DTYPE)
    for j, (b, e) in enumerate(intervals):
        d[j]["seq_begin"], d[j]["seq_end"] = b, e
    return d


def py_locate(res_idx, dom, res_len, per_strand, win_src, win_off):
    out = []
    for r, d in zip(res_idx, dom):
        i, minus, L = r % per_strand, r >= per_strand, int(res_len[r])
        b, e = int(d["seq_begin"]), int(d["seq_end"])
        if minus:
            b, e = L - e, L - b
        off = int(win_off[i]) if win_src is not None else 0
        out.append((int(win_src[i]) if win_src is not None else i, off + b, off + e, int(minus)))
    return out


def py_merge(src, minus, profile, begin, end, odds):
    """the rule as stated: one global order, a candidate against every kept member of its group"""
    n = len(src)
    order = sorted(range(n), key=lambda j: (-odds[j], -(int(end[j]) - int(begin[j])), j))
    keep = np.zeros(n, bool)
    kept = {}
    for j in order:
        group = kept.setdefault((int(src[j]), bool(minus[j]), int(profile[j])), [])
        b, e = int(begin[j]), int(end[j])
        ok = True
        for kb, ke in group:
            ov = min(e, ke) - max(b, kb)
            if ov > 0 and 2 * ov > min(e - b, ke - kb):
                ok = False
                break
        if ok:
            group.append((b, e))
            keep[j] = True
    return keep


# ---- locate ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("cut", [False, True])
def test_locate_equals_the_restatement(dcp, strands, cut):
    rng = np.random.default_rng(150 + strands + 2 * cut)
    # a 5 000-nt source in windows of 2 048 every 1 023 (offsets 0, 1 023: odd phase, ..., 2 952: anchored), a source
    # shorter than the window, and a 2 049-nt one (windows at 0 and 1)
    lens = [5000, 700, 2049]
    if cut:
        starts = [dcp.window_starts(L, 2048, 1023) for L in lens]
        assert starts[0].tolist() == [0, 1023, 2046, 2952] and starts[2].tolist() == [0, 1]
        win_src = np.concatenate([np.full(len(s), q, np.uint32) for q, s in enumerate(starts)])
        win_off = np.concatenate(starts).astype(np.uint32)
        res_len = np.concatenate([np.full(len(s), min(L, 2048), np.uint32) for L, s in zip(lens, starts)])
    else:
        win_src = win_off = None
        res_len = np.array(lens, np.uint32)
    per = len(res_len)
    res_len = np.tile(res_len, strands)
    res_idx, iv = [], []
    for r in range(per * strands):
        L = int(res_len[r])
        iv += [(0, L), (0, 1), (L - 1, L), (0, 0), (L, L)]  # the whole sequence, either end, empty ones at the ends
        iv += [tuple(sorted(rng.integers(0, L + 1, 2).tolist())) for _ in range(5)]
        res_idx += [r] * 10
    dom = domains(dcp, iv)
    got = dcp.locate_domains(res_idx, dom, res_len, per, strands, win_src, win_off)
    assert [a.dtype for a in got] == [np.uint32, np.uint64, np.uint64, np.uint8]
    assert list(zip(*[a.tolist() for a in got])) == py_locate(res_idx, dom, res_len, per, win_src, win_off)
    if strands == 2:  # a plus-strand interval and its mirror image on the minus strand are the same bases of the source
        L = int(res_len[0])
        s, b, e, m = dcp.locate_domains([0, per], domains(dcp, [(10, 40), (L - 40, L - 10)]), res_len, per, 2, win_src, win_off)
        assert s[0] == s[1] and b[0] == b[1] and e[0] == e[1] and m.tolist() == [0, 1]


def test_locate_offsets_need_64_bits(dcp):
    got = dcp.locate_domains([0], domains(dcp, [(5, 100)]), [100], 1, 1, [3], [2 ** 32 - 50])
    assert [int(a[0]) for a in got] == [3, 2 ** 32 - 45, 2 ** 32 + 50, 0]


def test_locate_refusals(dcp):
    dom, lens = domains(dcp, [(0, 10), (5, 20)]), np.array([20, 30, 20, 30], np.uint32)
    ok = lambda **kw: dcp.locate_domains(kw.get("res", [0, 3]), kw.get("dom", dom), kw.get("lens", lens), kw.get("per", 2),
                                         kw.get("strands", 2), kw.get("ws"), kw.get("wo"))
    assert ok()[3].tolist() == [0, 1]
    for bad in (dict(res=[0, 4]), dict(dom=domains(dcp, [(0, 21), (0, 1)])), dict(dom=domains(dcp, [(11, 10), (0, 1)])),
                dict(strands=3, lens=np.zeros(6, np.uint32)), dict(strands=0, lens=np.zeros(0, np.uint32)),
                dict(res=[0]), dict(lens=lens[:3]), dict(ws=[0], wo=[0])):
        with pytest.raises(dcp.DcpError) as e:
            ok(**bad)
        assert e.value.rc == dcp.RC_EINVAL, bad
    # the raw call writes nothing when it refuses
    import ctypes as C
    res = np.array([0, 4], np.uint32)
    src, b, e_, m = np.full(2, 9, np.uint32), np.full(2, 9, np.uint64), np.full(2, 9, np.uint64), np.full(2, 9, np.uint8)
    rc = dcp.lib.dcp_domains_locate(res.ctypes.data, dom.ctypes.data, 2, lens.ctypes.data, 2, 2, None, None, src.ctypes.data,
                                    b.ctypes.data, e_.ctypes.data, m.ctypes.data)
    assert rc == dcp.RC_EINVAL and (src == 9).all() and (b == 9).all() and (e_ == 9).all() and (m == 9).all()
    assert dcp.lib.dcp_domains_locate(None, None, 0, None, 0, 0, None, None, None, None, None, None) == 0
    assert dcp.DOMAIN_DTYPE.itemsize == 48 and C.sizeof(C.c_uint32) * 12 == 48


# ---- merge -------------------------------------------------------------------------------------------------------


def merge(dcp, rows):
    """rows: (src, minus, profile, begin, end, odds)"""
    cols = list(zip(*rows)) if rows else [[]] * 6
    return dcp.merge_domains(*cols).tolist()


def test_merge_disjoint_domains_are_all_kept(dcp):
    assert merge(dcp, [(0, 0, 0, 0, 100, 5.0), (0, 0, 0, 100, 200, 1.0), (0, 0, 0, 300, 301, -4.0)]) == [True, True, True]


def test_merge_exact_duplicates_keep_the_lower_index(dcp):
    assert merge(dcp, [(0, 0, 0, 10, 100, 7.5), (0, 0, 0, 10, 100, 7.5), (0, 0, 0, 10, 100, 7.5)]) == [True, False, False]
    assert merge(dcp, [(0, 0, 0, 10, 100, 7.5), (0, 0, 0, 10, 100, 8.5)]) == [False, True]  # the odds go first
    assert merge(dcp, [(0, 0, 0, 10, 99, 7.5), (0, 0, 0, 10, 100, 7.5)]) == [False, True]  # then the length


def test_merge_a_stump_inside_a_whole_copy_is_dropped(dcp):
    # the issue's numbers: the 83-nt stump of a 900-nt gene (odds 63.7 against 800.6), seen once beside two whole copies
    rows = [(0, 1, 2, 4013, 4096, 63.7), (0, 1, 2, 4013, 4912, 800.6), (0, 1, 2, 4013, 4912, 800.6)]
    assert merge(dcp, rows) == [False, True, False]
    # ranked by the raw core scores (-53.55 against -409.71) the stump would win and remove both whole copies
    assert merge(dcp, [r[:5] + (c,) for r, c in zip(rows, (-53.55, -409.71, -409.71))]) == [True, False, False]


def test_merge_half_is_kept_half_plus_one_is_dropped(dcp):
    assert merge(dcp, [(0, 0, 0, 0, 100, 2.0), (0, 0, 0, 50, 150, 1.0)]) == [True, True]    # ov 50 of 100
    assert merge(dcp, [(0, 0, 0, 0, 100, 2.0), (0, 0, 0, 49, 149, 1.0)]) == [True, False]   # ov 51
    assert merge(dcp, [(0, 0, 0, 0, 1000, 2.0), (0, 0, 0, 990, 1010, 1.0)]) == [True, True]  # ov 10 of the shorter's 20
    assert merge(dcp, [(0, 0, 0, 0, 1000, 2.0), (0, 0, 0, 989, 1010, 1.0)]) == [True, False]  # ov 11 of 21
    assert merge(dcp, [(0, 0, 0, 0, 1000, 1.0), (0, 0, 0, 989, 1010, 2.0)]) == [False, True]  # whichever ranks first stays
    assert merge(dcp, [(0, 0, 0, 0, 101, 2.0), (0, 0, 0, 50, 151, 1.0)]) == [True, False]   # 51 of 101: 102 > 101


def test_merge_groups_never_interact(dcp):
    same = (10, 100, 1.0)
    assert merge(dcp, [(0, 0, 0) + same, (0, 1, 0) + same, (0, 0, 1) + same, (1, 0, 0) + same]) == [True] * 4
    assert merge(dcp, [(0, 0, 0) + same, (0, 1, 0) + same, (0, 5, 0) + same]) == [True, True, False]  # any non-zero is minus


def test_merge_a_chain_in_which_the_middle_one_loses(dcp):
    # A [0, 100) and C [120, 220) do not overlap; B [40, 180) overlaps both by more than half of them.  B loses to A,
    # so C, which only B would have removed, survives.
    assert merge(dcp, [(0, 0, 0, 0, 100, 3.0), (0, 0, 0, 40, 180, 2.0), (0, 0, 0, 120, 220, 1.0)]) == [True, False, True]
    # and if B ranks first it removes both
    assert merge(dcp, [(0, 0, 0, 0, 100, 2.0), (0, 0, 0, 40, 180, 3.0), (0, 0, 0, 120, 220, 1.0)]) == [False, True, False]


def test_merge_nothing_and_the_refusals(dcp):
    assert merge(dcp, []) == []
    for rows in ([(0, 0, 0, 0, 10, float("nan"))], [(0, 0, 0, 0, 10, 1.0), (0, 0, 0, 5, 5, 1.0)],
                 [(0, 0, 0, 0, 10, 1.0), (0, 0, 0, 6, 5, 1.0)]):
        with pytest.raises(dcp.DcpError) as e:
            merge(dcp, rows)
        assert e.value.rc == dcp.RC_EINVAL
    assert merge(dcp, [(0, 0, 0, 0, 10, float("inf")), (0, 0, 0, 0, 10, float("-inf"))]) == [True, False]  # infinities rank


def test_merge_20000_random_domains(dcp):
    rng = np.random.default_rng(20000)
    n = 20000
    src, minus, profile = rng.integers(0, 4, n), rng.integers(0, 2, n), rng.integers(0, 25, n)
    begin = rng.integers(0, 200_000, n)
    end = begin + rng.integers(1, 1500, n)
    odds = np.round(rng.normal(100, 80, n))  # whole numbers: many exact ties
    want = py_merge(src, minus, profile, begin, end, odds)
    t0 = time.perf_counter()
    got = dcp.merge_domains(src, minus, profile, begin, end, odds)
    dt = time.perf_counter() - t0
    assert np.array_equal(got, want) and 0 < got.sum() < n
    assert dt < 0.5, dt  # one sort and neighbourhood look-ups: about 10 ms; a quadratic loop over 20 000 takes seconds
    # one group, everything piled up: still the rule, still fast
    src[:] = minus[:] = profile[:] = 0
    begin = rng.integers(0, 3000, n)
    end = begin + rng.integers(1, 1500, n)
    t0 = time.perf_counter()
    got = dcp.merge_domains(src, minus, profile, begin, end, odds)
    dt = time.perf_counter() - t0
    assert np.array_equal(got, py_merge(src, minus, profile, begin, end, odds))
    assert dt < 0.5, dt


def test_domains_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_domains.c with the host model alone (no device code) under ASan + UBSan, as a program of its own."""
    obj, exe = str(tmp_path / "asan_domains.o"), str(tmp_path / "asan_domains")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_domains.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_domains ok" in r.stdout
