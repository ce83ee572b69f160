"""dcp_domains_regions and dcp_domains_locate_regions (csrc/dcp_model.cpp; domain_regions / locate_domains_regions): pure
host arithmetic, checked on the CPU.

regions: hand-made cases for every clause of the rule, the refusals, the counting call, then 20 000 random domains
against the rule restated in Python.  locate: against a restatement, both strands, a region at offset 0 and one ending
at its source's last base.  tests/c/asan_regions.c drives both calls under ASan + UBSan in a stand-alone program.

Premises, on the oracle: the planted world of test_seq_windows cut 1 024 / 512 reports the 899-nt minus-strand gene in
pieces only, the merge leaves more than one of them, the rule joins every copy's pieces into one region, and each
region's slice scanned alone gives one domain from node 1 to node M."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_both_strands import bits, np_revcomp, oracle_lrt
from test_c_host import ROOT
from test_domains_merge import domains, py_merge
from test_path_domains import restate
from test_seq_windows import PLANT_L, PLANT_M, hand_cut, planted_world, py_starts

PRECISIONS = (32, 64)
REGION_CUT = (1024, 512)  # the planted world under it: the 899-nt gene lies wholly in no window
REGION_FLANK = 30


def py_regions(src, minus, profile, begin, end, src_len, max_gap=0, flank=0):
    """the rule as stated: (reg_of, [(src, minus, profile, begin, len, nparts)])"""
    n = len(src)
    order = sorted(range(n), key=lambda j: (int(src[j]), bool(minus[j]), int(profile[j]), int(begin[j]), int(end[j]), j))
    reg_of, regs, cur = [0] * n, [], None
    for j in order:
        key = (int(src[j]), int(bool(minus[j])), int(profile[j]))
        b, e = int(begin[j]), int(end[j])
        if cur is not None and cur["key"] == key and b <= cur["hi"] + max_gap:
            cur["hi"] = max(cur["hi"], e)
            cur["n"] += 1
        else:
            cur = dict(key=key, lo=b, hi=e, n=1)
            regs.append(cur)
        reg_of[j] = len(regs) - 1
    out = []
    for r in regs:
        lo = r["lo"] - min(r["lo"], flank)
        hi = min(r["hi"] + flank, int(src_len[r["key"][0]]))
        out.append(r["key"] + (lo, hi - lo, r["n"]))
    return reg_of, out


def regions(dcp, rows, src_len, max_gap=0, flank=0):
    """rows: (src, minus, profile, begin, end) -> (reg_of list, region tuples)"""
    cols = list(zip(*rows)) if rows else [[]] * 5
    reg_of, reg = dcp.domain_regions(*cols, src_len, max_gap, flank)
    assert reg_of.dtype == np.uint32 and reg.dtype == dcp.REGION_DTYPE
    return reg_of.tolist(), [tuple(int(v) for v in r) for r in reg]


def both(dcp, rows, src_len, max_gap=0, flank=0):
    got = regions(dcp, rows, src_len, max_gap, flank)
    cols = list(zip(*rows))
    assert got == py_regions(*cols, src_len, max_gap, flank)
    return got


# ---- the rule ------------------------------------------------------------------------------------------------------


def test_a_gap_of_exactly_max_gap_joins_and_one_more_does_not(dcp):
    rows = [(0, 0, 0, 10, 100), (0, 0, 0, 150, 200)]
    assert both(dcp, rows, [1000], max_gap=50) == ([0, 0], [(0, 0, 0, 10, 190, 2)])
    assert both(dcp, rows, [1000], max_gap=49) == ([0, 1], [(0, 0, 0, 10, 90, 1), (0, 0, 0, 150, 50, 1)])
    # max_gap 0: touching intervals join, a gap of one base does not
    assert both(dcp, [(0, 0, 0, 10, 100), (0, 0, 0, 100, 200)], [1000])[1] == [(0, 0, 0, 10, 190, 2)]
    assert len(both(dcp, [(0, 0, 0, 10, 100), (0, 0, 0, 101, 200)], [1000])[1]) == 2
    # the largest gap there is: hi + max_gap is taken in 64 bits and beyond
    assert both(dcp, rows, [1000], max_gap=2 ** 64 - 1) == ([0, 0], [(0, 0, 0, 10, 190, 2)])


def test_containment_keeps_the_largest_end(dcp):
    # [10, 500) holds [20, 30); [400, 600) joins on the first one's end, not on the contained one's
    rows = [(0, 0, 0, 20, 30), (0, 0, 0, 400, 600), (0, 0, 0, 10, 500)]
    assert both(dcp, rows, [1000]) == ([0, 0, 0], [(0, 0, 0, 10, 590, 3)])
    rows = [(0, 0, 0, 10, 500), (0, 0, 0, 20, 30), (0, 0, 0, 31, 40), (0, 0, 0, 501, 502)]
    assert both(dcp, rows, [1000]) == ([0, 0, 0, 1], [(0, 0, 0, 10, 490, 3), (0, 0, 0, 501, 1, 1)])


def test_equal_begins_and_input_order(dcp):
    rows = [(0, 0, 0, 300, 400), (0, 0, 0, 10, 90), (0, 0, 0, 10, 20), (0, 0, 0, 10, 90)]
    assert both(dcp, rows, [1000]) == ([1, 0, 0, 0], [(0, 0, 0, 10, 80, 3), (0, 0, 0, 300, 100, 1)])


def test_flanks_are_clipped_at_both_ends_of_the_source(dcp):
    rows = [(0, 0, 0, 5, 100), (0, 0, 0, 900, 995), (1, 0, 0, 0, 50)]
    assert both(dcp, rows, [1000, 50], flank=10)[1] == [(0, 0, 0, 0, 110, 1), (0, 0, 0, 890, 110, 1), (1, 0, 0, 0, 50, 1)]
    assert both(dcp, rows, [1000, 50], flank=5)[1] == [(0, 0, 0, 0, 105, 1), (0, 0, 0, 895, 105, 1), (1, 0, 0, 0, 50, 1)]
    assert both(dcp, rows, [1000, 50], flank=2 ** 32 - 1)[1] == [(0, 0, 0, 0, 1000, 1), (0, 0, 0, 0, 1000, 1), (1, 0, 0, 0, 50, 1)]
    # the flank plays no part in the clustering
    assert both(dcp, [(0, 0, 0, 10, 100), (0, 0, 0, 101, 200)], [1000], flank=50)[1] == [(0, 0, 0, 0, 150, 1), (0, 0, 0, 51, 199, 1)]


def test_groups_never_interact_and_regions_come_out_in_order(dcp):
    same = (10, 100)
    rows = [(1, 0, 0) + same, (0, 0, 1) + same, (0, 1, 0) + same, (0, 0, 0) + same, (0, 5, 0) + same]
    reg_of, reg = both(dcp, rows, [200, 200], max_gap=1000)
    assert reg == [(0, 0, 0, 10, 90, 1), (0, 0, 1, 10, 90, 1), (0, 1, 0, 10, 90, 2), (1, 0, 0, 10, 90, 1)]
    assert reg_of == [3, 1, 2, 0, 2]  # any non-zero is minus


def test_nothing_and_the_refusals(dcp):
    assert regions(dcp, [], [100]) == ([], [])
    assert regions(dcp, [], []) == ([], [])
    for rows, lens in (([(0, 0, 0, 5, 5)], [100]), ([(0, 0, 0, 6, 5)], [100]), ([(0, 0, 0, 5, 101)], [100]),
                       ([(1, 0, 0, 5, 10)], [100]), ([(0, 0, 0, 5, 10)], []), ([(0, 0, 0, 5, 10), (0, 0, 0, 2 ** 40, 2 ** 40 + 1)], [100])):
        with pytest.raises(dcp.DcpError) as e:
            regions(dcp, rows, lens)
        assert e.value.rc == dcp.RC_EINVAL, rows
    with pytest.raises(dcp.DcpError):
        dcp.domain_regions([0], [0], [0], [1, 2], [3], [100])
    assert regions(dcp, [(0, 0, 0, 0, 100)], [100]) == ([0], [(0, 0, 0, 0, 100, 1)])  # the whole source


def raw_regions(dcp, rows, lens, cap, null=(), nregions=True):
    src, minus, profile, begin, end = (np.array(col, t) for col, t in
                                       zip(zip(*rows), (np.uint32, np.uint8, np.uint32, np.uint64, np.uint64)))
    lens = np.array(lens, np.uint32)
    reg_of = np.full(len(rows), 9, np.uint32)
    outs = [np.full(max(cap, 1), 9, t) for t in (np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32)]
    n = C.c_uint(77)
    ptr = lambda name, a: None if name in null else a.ctypes.data
    rc = dcp.lib.dcp_domains_regions(ptr("src", src), ptr("minus", minus), ptr("profile", profile), ptr("begin", begin),
                                     ptr("end", end), len(rows), ptr("src_len", lens), len(lens), 0, 0, ptr("reg_of", reg_of),
                                     *[ptr("out%d" % i, a) for i, a in enumerate(outs)], cap, C.byref(n) if nregions else None)
    untouched = (reg_of == 9).all() and all((a == 9).all() for a in outs)
    return rc, n.value, untouched


def test_the_raw_call_counts_first_and_writes_nothing_when_it_refuses(dcp):
    rows = [(0, 0, 0, 10, 20), (0, 0, 0, 30, 40), (0, 1, 0, 30, 40)]
    for cap in (0, 1, 2):
        assert raw_regions(dcp, rows, [100], cap) == (dcp.RC_ENOMEM, 3, True)
    assert raw_regions(dcp, rows, [100], 0, null=["out%d" % i for i in range(6)]) == (dcp.RC_ENOMEM, 3, True)  # the counting call
    rc, n, untouched = raw_regions(dcp, rows, [100], 3)
    assert (rc, n, untouched) == (0, 3, False)
    assert raw_regions(dcp, rows, [100], 5)[:2] == (0, 3)
    for name in ("src", "minus", "profile", "begin", "end", "src_len", "reg_of", "out0", "out1", "out2", "out3", "out4", "out5"):
        assert raw_regions(dcp, rows, [100], 3, null=[name]) == (dcp.RC_EINVAL, 77, True), name
    assert raw_regions(dcp, rows, [100], 3, nregions=False)[0] == dcp.RC_EINVAL
    assert raw_regions(dcp, rows[:2] + [(0, 0, 0, 50, 101)], [100], 3) == (dcp.RC_EINVAL, 77, True)
    n = C.c_uint(77)
    assert dcp.lib.dcp_domains_regions(None, None, None, None, None, 0, None, 0, 0, 0, None, None, None, None, None, None, None,
                                       0, C.byref(n)) == 0 and n.value == 0


def test_20000_random_domains(dcp):
    rng = np.random.default_rng(20016)
    n = 20000
    src_len = rng.integers(150_000, 200_000, 4)
    src, minus, profile = rng.integers(0, 4, n), rng.integers(0, 2, n) * rng.integers(1, 200, n), rng.integers(0, 25, n)
    begin = rng.integers(0, 140_000, n)
    end = np.minimum(begin + rng.integers(1, 1500, n), src_len[src])
    for max_gap, flank in ((0, 0), (0, 30), (100, 5000), (1, 2 ** 31)):
        reg_of, reg = dcp.domain_regions(src, minus, profile, begin, end, src_len, max_gap, flank)
        want_of, want = py_regions(src, minus, profile, begin, end, src_len, max_gap, flank)
        assert reg_of.tolist() == want_of and [tuple(int(v) for v in r) for r in reg] == want, (max_gap, flank)
        assert 200 <= len(reg) < n and int(reg["nparts"].sum()) == n
        assert np.array_equal(np.bincount(reg_of, minlength=len(reg)), reg["nparts"])
        # every domain lies in its region
        r = reg[reg_of]
        assert (r["begin"] <= begin).all() and (end <= r["begin"].astype(np.int64) + r["len"]).all()
    # one group, everything piled up
    src[:] = minus[:] = profile[:] = 0
    begin = rng.integers(0, 3000, n)
    end = begin + rng.integers(1, 1500, n)
    assert regions(dcp, list(zip(src, minus, profile, begin, end)), src_len) == py_regions(src, minus, profile, begin, end, src_len)


# ---- locate on regions ---------------------------------------------------------------------------------------------


def py_locate_regions(res_idx, dom, res_len, reg_src, reg_begin, reg_minus):
    out = []
    for r, d in zip(res_idx, dom):
        L, b, e = int(res_len[r]), int(d["seq_begin"]), int(d["seq_end"])
        if reg_minus[r]:
            b, e = L - e, L - b
        out.append((int(reg_src[r]), int(reg_begin[r]) + b, int(reg_begin[r]) + e, int(bool(reg_minus[r]))))
    return out


def test_locate_regions_equals_the_restatement(dcp):
    rng = np.random.default_rng(1600)
    src_len = [5000, 700]
    # a region at offset 0, one ending at its source's last base, the whole of a source, odd phases: each on both strands
    reg = [(0, 0, 100), (0, 4900, 100), (1, 0, 700), (0, 1023, 33), (1, 699, 1), (0, 17, 2048)]
    reg_src = [s for s, _, _ in reg] * 2
    reg_begin = [b for _, b, _ in reg] * 2
    res_len = [n for _, _, n in reg] * 2
    reg_minus = [0] * len(reg) + [7] * len(reg)
    assert all(b + n <= src_len[s] for s, b, n in reg)
    res_idx, iv = [], []
    for r, L in enumerate(res_len):
        iv += [(0, L), (0, 1), (L - 1, L), (0, 0), (L, L)] + [tuple(sorted(rng.integers(0, L + 1, 2).tolist())) for _ in range(5)]
        res_idx += [r] * 10
    dom = domains(dcp, iv)
    got = dcp.locate_domains_regions(res_idx, dom, res_len, reg_src, reg_begin, reg_minus)
    assert [a.dtype for a in got] == [np.uint32, np.uint64, np.uint64, np.uint8]
    assert list(zip(*[a.tolist() for a in got])) == py_locate_regions(res_idx, dom, res_len, reg_src, reg_begin, reg_minus)
    # a plus interval and its mirror image on the minus twin of the region are the same bases of the source
    s, b, e, m = dcp.locate_domains_regions([5, 11], domains(dcp, [(10, 40), (2048 - 40, 2048 - 10)]), res_len, reg_src, reg_begin, reg_minus)
    assert s[0] == s[1] == 0 and b[0] == b[1] == 27 and e[0] == e[1] == 57 and m.tolist() == [0, 1]
    # begin + len needs more than 32 bits
    got = dcp.locate_domains_regions([0], domains(dcp, [(5, 100)]), [100], [3], [2 ** 32 - 50], [1])
    assert [int(a[0]) for a in got] == [3, 2 ** 32 - 50, 2 ** 32 + 45, 1]


def test_locate_regions_refusals(dcp):
    dom = domains(dcp, [(0, 10), (5, 20)])
    ok = lambda **kw: dcp.locate_domains_regions(kw.get("res", [0, 1]), kw.get("dom", dom), kw.get("lens", [20, 30]), [0, 0],
                                                 [0, 50], kw.get("minus", [0, 1]))
    assert ok()[3].tolist() == [0, 1]
    for bad in (dict(res=[0, 2]), dict(dom=domains(dcp, [(0, 21), (0, 1)])), dict(dom=domains(dcp, [(11, 10), (0, 1)])),
                dict(res=[0]), dict(lens=[20]), dict(minus=[0])):
        with pytest.raises(dcp.DcpError) as e:
            ok(**bad)
        assert e.value.rc == dcp.RC_EINVAL, bad
    res, lens = np.array([0, 2], np.uint32), np.array([20, 30], np.uint32)
    rs, rb, rm = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint8)
    src, b, e_, m = np.full(2, 9, np.uint32), np.full(2, 9, np.uint64), np.full(2, 9, np.uint64), np.full(2, 9, np.uint8)
    call = lambda r, s: dcp.lib.dcp_domains_locate_regions(r, dom.ctypes.data, 2, lens.ctypes.data, 2, rs.ctypes.data, rb.ctypes.data,
                                                           rm.ctypes.data, s, b.ctypes.data, e_.ctypes.data, m.ctypes.data)
    assert call(res.ctypes.data, src.ctypes.data) == dcp.RC_EINVAL
    assert call(None, src.ctypes.data) == dcp.RC_EINVAL and call(res.ctypes.data, None) == dcp.RC_EINVAL
    assert (src == 9).all() and (b == 9).all() and (e_ == 9).all() and (m == 9).all()
    assert dcp.lib.dcp_domains_locate_regions(None, None, 0, None, 0, None, None, None, None, None, None, None) == 0


def test_regions_under_asan_ubsan(tmp_path):
    """CPU: tests/c/asan_regions.c with the host model alone (no device code) under ASan + UBSan, as a program of its own."""
    obj, exe = str(tmp_path / "asan_regions.o"), str(tmp_path / "asan_regions")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "c", "asan_regions.c"),
                           "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + san +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "deciphon-old_amd", "csrc"), obj,
                           os.path.join(ROOT, "deciphon-old_amd", "csrc", "dcp_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_regions ok" in r.stdout


# ---- premises on the oracle ----------------------------------------------------------------------------------------

_PREMISE = {}


def oracle_domains(orc, oprof, seq):
    """the records of the oracle's multi-hit Viterbi path of seq against oprof"""
    oprof.setup(len(seq), True, False)
    t8, em, ei, en, xt = oprof.export()
    _, al, apath, _ = orc.dp_tables_path(t8, em, ei, en, xt, bytes(seq))
    total, recs, cores, nulls = restate(*apath, seq, t8, em, ei, en, xt)
    assert bits(total) == bits(orc.np(al))
    return recs, cores, nulls


def planted_regions(dcp, orc, precision):
    """The planted world cut REGION_CUT, both strands, multi-hit, LRT >= 10, on the oracle: every domain located on the
    source (the restated locate), its odds, and the regions of the restated rule.  Computed once per precision."""
    if precision not in _PREMISE:
        _, oprofs, seq, _ = planted_world(dcp, orc, precision)
        cut = hand_cut([seq], *REGION_CUT)
        W = len(cut)
        starts = py_starts(PLANT_L, *REGION_CUT)
        res = cut + [np_revcomp(s) for s in cut]
        lrt = oracle_lrt(orc, oprofs, res)
        rows = []
        for r, p in zip(*np.nonzero(lrt >= 10.0)):
            recs, cores, nulls = oracle_domains(orc, oprofs[p], res[r])
            for rec, c, n in zip(recs, cores, nulls):
                L, b, e, minus = len(res[r]), rec["seq_begin"], rec["seq_end"], int(r >= W)
                if minus:
                    b, e = L - e, L - b
                rows.append(dict(profile=int(p), minus=minus, begin=starts[r % W] + b, end=starts[r % W] + e, res=int(r),
                                 first=rec["node_first"], last=rec["node_last"], odds=float(c) - float(n)))
        col = lambda k: np.array([row[k] for row in rows])
        src = np.zeros(len(rows), np.uint32)
        reg_of, reg = py_regions(src, col("minus"), col("profile"), col("begin"), col("end"), [PLANT_L], 0, REGION_FLANK)
        # each region's slice (reverse-complemented for a minus one) scanned alone: its domains, located on the source
        final = []
        for _, minus, p, b, n, _ in reg:
            piece = seq[b:b + n]
            recs, _, _ = oracle_domains(orc, oprofs[p], np_revcomp(piece) if minus else piece)
            final.append([(b + n - rec["seq_end"], b + n - rec["seq_begin"], rec["node_first"], rec["node_last"]) if minus else
                          (b + rec["seq_begin"], b + rec["seq_end"], rec["node_first"], rec["node_last"]) for rec in recs])
        _PREMISE[precision] = (rows, reg_of, reg, W, final)
    return _PREMISE[precision]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_premise_windows_report_the_long_gene_in_pieces_and_the_rule_joins_them(dcp, oracle32, oracle64, precision):
    orc = oracle64 if precision == 64 else oracle32
    rows, reg_of, reg, W, final = planted_regions(dcp, orc, precision)
    assert py_starts(PLANT_L, *REGION_CUT)[-1] + REGION_CUT[0] == PLANT_L and W == 11
    long_gene = [row for row in rows if row["profile"] == 2]
    # 1. no located domain of profile 2 spans the model
    assert long_gene and all(row["minus"] == 1 for row in long_gene)
    assert not any(row["first"] == 1 and row["last"] == PLANT_M[2] for row in long_gene)
    # 2. after the merge more than one domain of it is left
    col = lambda k: np.array([row[k] for row in rows])
    src = np.zeros(len(rows), np.uint32)
    keep = py_merge(src, col("minus"), col("profile"), col("begin"), col("end"), col("odds"))
    assert sum(1 for j in np.flatnonzero(keep) if rows[j]["profile"] == 2) > 1
    # 3. the rule gives exactly three regions, one per planted copy; the library's rule is the restated one
    got_of, got = dcp.domain_regions(src, col("minus"), col("profile"), col("begin"), col("end"), [PLANT_L], 0, REGION_FLANK)
    assert got_of.tolist() == reg_of and [tuple(int(v) for v in r) for r in got] == reg
    assert [(r[2], r[1]) for r in reg] == [(0, 0), (1, 0), (2, 1)]
    assert sum(r[5] for r in reg) == len(rows) and reg[2][5] == len(long_gene) > 1
    if precision == 32:  # what the issue observed
        assert [(r[3] + REGION_FLANK, r[3] + r[4] - REGION_FLANK, r[5]) for r in reg] == [(1112, 1232, 2), (2512, 2902, 3), (4013, 4912, 4)]
    # 4. each region's slice (reverse-complemented for the minus one) has exactly one domain, node 1 to node M
    for (_, minus, p, b, n, _), doms in zip(reg, final):
        assert len(doms) == 1 and doms[0][2:] == (1, PLANT_M[p]), (p, doms)
        assert b <= doms[0][0] < doms[0][1] <= b + n
