"""The scaled probability-space Forward sweep where pairs leave the double range: the exits of forward_scaled_kernel and
forward_scaled_wide_kernel (csrc/dcp_forward_scaled.hip), finish_pair's own, and the redo list that run_scaled_sweeps
and rerun_scaled_redo (csrc/dcp_gpu.hip) hand to the log-space kernels; DESIGN section 24.

The promise under test: no NaN or +inf score is ever returned; a pair whose values leave the double range is rerun in
log space and has forward_pairs' bits; every other pair's bits do not depend on what else is in the call.

One world, defined here, for the CPU part and the GPU part:

  profiles   ordinary      pfam_like_params at 1, 64, 65, 128, 129, 256, 257, 513 nodes: both sides of every class edge
             overflow      positive delete chains (MD = +0.7, DD = v on nodes 1 .. M - 1) whose sum of DD is above 745:
                           (33, 24), (64, 12), (65, 12), (128, 6), (129, 6), (256, 3), (257, 3), (513, 1.5).  The chain
                           multiplies up past the double range in the first row that holds mass
             near edge     the same with a sum of DD below 700: (64, 11), (128, 5.5), (256, 2.7); they stay in range
             epsilon 0     (64, 12) and (256, 3) with epsilon 0: no mass before row 3, none at all where L mod 3 != 0
             late exit     IM = -inf and II = +v at every node, at 7, 70, 130, 260 nodes (one per class): the insert ring
                           grows by e^v a row and nothing feeds it back into what the rescaling looks at, so Q leaves the
                           range after some rows, each v at another row.  (An emission score above 709.8 cannot be had:
                           from_params normalises the codon, insert and null tables, so no emission exceeds 0.)
  queries    random, L = 1, 2, 3, 4, 6, 12, 40
  lever rows copies of the 12-nt and of the 1-nt query whose special transitions are those of their length, multi-hit,
             with: nothing; one of SB, SN, NB, EB, EJ, EC, RR, ET, CT = 710; ET = CT = 710; ET = 709.5 (a float-rule case:
             t > 708; never on a double DB's device run); SB = SN = -705; ET = CT = -705; RR = -705

CPU (the premises; oracle tables, both factor rules, bands 4 and 64): restate_scaled of tests/test_forward_scaled.py
says where the rule ends a pair, by the twin's checks in the twin's order; the twin's verdict is the restatement's on
every pair; in range the twin is within the project's allowances of forward_tables; forward_tables is finite on every
flagged pair but epsilon 0 with L mod 3 != 0; the exits seen are row 0, row 1, row 3, a late row at each phase of the
unroll by five, the finish, and R alone; RR = -705 is flagged at band 4 and in range at band 64 somewhere.

GPU (per precision): every (copy, profile) pair through forward_pairs_scaled at the default band and at band 4; the
unflagged pairs alone; one and three wavefronts behind their bad pairs; four classes on one redo list; the dense scan
with the lever rows set; the pairs near the edge that stay in range, at bands 4, 8 and 64.

Allowances, the project's own: device against scaled twin 2^-32 (|x| + 1); against forward_pairs the same on a double DB
and A = (L (M + 2) + 2)(delta + 2^-51) on a float DB; rerun pairs: bit equality."""
import numpy as np
import pytest

import test_forward_chain_premises as pr
import test_forward_scaled as fs
from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, refused
from test_forward_dense import full_list, same_matrices
from test_forward_pairs import NEG_INF, PRECISIONS, device_tables, within, worst, xtrans_of
from test_gpu_parity import pfam_like_params

XT = ("RR", "SB", "SN", "NN", "NB", "ET", "EC", "CC", "CT", "EB", "EJ", "JJ", "JB")  # xtrans order
BANDS = (4, 64)

# ---- the world ------------------------------------------------------------------------------------------------------
ORDINARY_M = (1, 64, 65, 128, 129, 256, 257, 513)
OVERFLOW = ((33, 24.0), (64, 12.0), (65, 12.0), (128, 6.0), (129, 6.0), (256, 3.0), (257, 3.0), (513, 1.5))  # (M, DD)
NEAR_EDGE = ((64, 11.0), (128, 5.5), (256, 2.7))
EPS0 = ((64, 12.0), (256, 3.0))
LATE_M = (7, 70, 130, 260)
LATE_II = (96.0, 108.0, 124.0, 142.0, 170.0)  # rows 10, 9, 8, 7, 6 on the 12-nt and the 40-nt query: every phase
FAMILIES = ("ordinary", "overflow", "near", "eps0", "late")
QUERY_L = (1, 2, 3, 4, 6, 12, 40)
LEVER_L = (12, 1)
LEVERS = (("none", {}),) + tuple((n + "710", {n: 710.0}) for n in ("SB", "SN", "NB", "EB", "EJ", "EC", "RR", "ET", "CT")) + (
    ("ET=CT710", {"ET": 710.0, "CT": 710.0}), ("ET709.5", {"ET": 709.5}), ("SB=SN-705", {"SB": -705.0, "SN": -705.0}),
    ("ET=CT-705", {"ET": -705.0, "CT": -705.0}), ("RR-705", {"RR": -705.0}))
FLOAT_RULE_ONLY = "ET709.5"  # 708 < t < 709.78: +inf by the float rule, a finite factor in double
DD_SUM_OUT, DD_SUM_IN = 745.0, 700.0  # the margins of the chains' verdicts
XT_OUT, XT_IN = 709.9, 709.0  # and of the special transitions', on a double DB


def world_specs():
    """[(family, M, v, epsilon)] in the order of the DB"""
    return ([("ordinary", M, None, pr.EPS) for M in ORDINARY_M] + [("overflow", M, v, pr.EPS) for M, v in OVERFLOW] +
            [("near", M, v, pr.EPS) for M, v in NEAR_EDGE] + [("eps0", M, v, 0.0) for M, v in EPS0] +
            [("late", M, v, pr.EPS) for M in LATE_M for v in LATE_II])


def params(spec):
    """(null, match, trans) of from_params, as chain_params("positive", ..) builds its chains"""
    family, M, v = spec[:3]
    null, match, trans = pfam_like_params(np.random.default_rng(7000 + M), M)
    trans = trans.copy()
    if family in ("overflow", "near", "eps0"):
        trans[1:M, 2] = np.float32(0.7)
        trans[1:M, 6] = np.float32(v)
    elif family == "late":
        trans[:, 3] = -np.inf  # IM: nothing comes back from the insert states
        trans[:, 4] = np.float32(v)  # II
    return null, match, trans


def copies(precision=None):
    """[(L, lever name)]: the resident batch.  A double DB leaves out the float-rule case"""
    out = [(L, "none") for L in QUERY_L] + [(L, name) for name, _ in LEVERS for L in LEVER_L]
    return [c for c in out if not (precision == 64 and c[1] == FLOAT_RULE_ONLY)]


def query(L):
    return np.random.default_rng(70 + L).integers(0, 4, L, dtype=np.uint8)


def lever_row(xt, name):
    """the special transitions xt of a length with the lever's values in place"""
    xt = np.array(xt)
    for which, value in dict(LEVERS)[name].items():
        xt[XT.index(which)] = value
    return xt


def size_class(M):
    return 0 if M <= 64 else 1 if M <= 128 else 2 if M <= 256 else 3


def exit_kind(spec, ex, names):
    """what the coverage assertions count: None in range"""
    if ex is None:
        return None
    if ex == ("finish",):
        return "finish"
    if names == ["PR"]:
        return "R alone"
    if spec[0] == "late" and ex[1] > 5 and set(names) <= {"P", "Q"}:
        return "late%d" % (ex[1] % 5)  # the phase of the unroll by five
    return "row%d" % ex[1]


LATE_KINDS = tuple("late%d" % ph for ph in range(5))


# ---- CPU: the premises --------------------------------------------------------------------------------------------------
def test_the_world_is_what_the_docstring_says_and_its_verdicts_have_margins():
    specs = world_specs()
    assert len(specs) == 8 + 8 + 3 + 2 + 4 * 5 and len(copies()) == 7 + 2 * 15 and len(copies(64)) == len(copies()) - 2
    assert sorted({size_class(M) for M in ORDINARY_M}) == sorted({size_class(M) for M in LATE_M}) == [0, 1, 2, 3]
    assert sorted({size_class(M) for M, _ in OVERFLOW}) == [0, 1, 2, 3] and all(M <= 513 for _, M, _, _ in specs)
    for spec in specs:
        family, M, v, eps = spec
        trans = np.asarray(params(spec)[2], np.float64)
        if family in ("overflow", "eps0"):
            assert float(trans[1:M, 6].sum()) > DD_SUM_OUT, spec
        elif family == "near":
            assert 0.0 < float(trans[1:M, 6].sum()) < DD_SUM_IN, spec
        elif family == "late":
            assert np.isneginf(trans[:, 3]).all() and (trans[:, 4] == v).all()
    for name, lever in LEVERS:  # a double DB takes exp from another libm on each side: nothing of its world is near 709.78
        for value in lever.values():
            assert value >= XT_OUT or value <= XT_IN or name == FLOAT_RULE_ONLY, name
    assert XT_IN < 709.78 < XT_OUT and 708.0 < dict(LEVERS)[FLOAT_RULE_ONLY]["ET"] < XT_OUT


_CPU = {}


def f32_rounded(a):
    return np.asarray(a, np.float32).astype(np.float64)


def cpu_pair(dcp, orc, p, c):
    """forward_tables, the twin per (float factors, band) and the restatement per band of profile p x copy c"""
    key = (orc.np, p, c)
    if key not in _CPU:
        spec, (L, lever) = world_specs()[p], copies()[c]
        if ("tabs", orc.np, p) not in _CPU:
            prof = orc.new(*params(spec), ENTRY_DIST_OCCUPANCY, spec[3])
            prof.setup(1, True, False)
            _CPU["tabs", orc.np, p] = prof.export()[:4]
        tabs, seq = _CPU["tabs", orc.np, p], query(L)
        xt = lever_row(dcp.xtrans64(L, True, False), lever)
        tabs32, xt32 = tuple(f32_rounded(t) for t in tabs), f32_rounded(xt)  # what a float DB would hold
        out = {"ft": dcp.forward_tables(*tabs, xt, seq), "ft32": dcp.forward_tables(*tabs32, xt32, seq), "tw": {}, "rs": {}}
        for band in BANDS:
            out["tw"][False, band] = dcp.forward_scaled_tables(*tabs, xt, seq, band=band)
            out["tw"][True, band] = dcp.forward_scaled_tables(*tabs32, xt32, seq, float_factors=True, band=band)
            out["rs"][band] = fs.restate_scaled(*tabs, xt, seq, band, where=True)
        out["args"] = (tabs, xt, seq)
        _CPU[key] = out
    return _CPU[key]


@pytest.mark.parametrize("family", FAMILIES)
def test_twin_restatement_and_forward_tables_on_every_pair(dcp, oracle64, family):
    specs, cps = world_specs(), copies()
    far = {(f32, band): 0.0 for f32 in (False, True) for band in BANDS}
    counts = {"pairs": 0, "flagged": 0}
    for p, spec in enumerate(specs):
        if spec[0] != family:
            continue
        M = spec[1]
        for c, (L, lever) in enumerate(cps):
            r = cpu_pair(dcp, oracle64, p, c)
            where = (spec, L, lever)
            counts["pairs"] += 1
            for band in BANDS:
                n, a, s, sR, ex, names = r["rs"][band]
                tn, ta, oor = r["tw"][False, band]
                assert oor == (ex is not None), (where, band, ex, names)  # the twin's verdict is the restatement's
                fn, fa, foor = r["tw"][True, band]
                assert foor == (True if lever == FLOAT_RULE_ONLY else oor), (where, band)
                if not oor:
                    assert bits(np.array([tn, ta])).tolist() == bits(np.array([n, a])).tolist(), (where, band)
                    far[False, band] = max(far[False, band], worst([tn, ta], r["ft"]))
                    assert within([tn, ta], r["ft"]), (where, band, (tn, ta), r["ft"])
                if not foor:
                    if np.isfinite(r["ft32"]).all():
                        far[True, band] = max(far[True, band], float(np.max(np.abs(np.array([fn, fa]) - np.array(r["ft32"])))) /
                                              fs.allowance_f32(L, M))
                    assert fs.within_f32([fn, fa], r["ft32"], L, M), (where, band, (fn, fa), r["ft32"])
                if oor or foor:
                    counts["flagged"] += 1
                    no_path = spec[3] == 0.0 and L % 3 != 0
                    assert no_path or np.isfinite(r["ft"]).all(), (where, r["ft"])
                if exit_kind(spec, ex, names) in LATE_KINDS:
                    tabs, xt, seq = r["args"]
                    # at band 4 it has rescaled by then, and was fine up to the row before
                    assert band != 4 or s != 0, (where, band)
                    assert band != 4 or lever != "none" or not dcp.forward_scaled_tables(*tabs, xt, seq[:ex[1] - 1], band=band)[2], where
    print("%s: %d pairs, %d flagged verdicts; worst in range: double factors %s of 2^-32 (|x| + 1), float factors %s of A" % (
        family, counts["pairs"], counts["flagged"], {b: "%.3e" % (far[False, b] * 2.0 ** 32) for b in BANDS},
        {b: "%.3e" % far[True, b] for b in BANDS}))
    assert counts["pairs"] == len(cps) * sum(s[0] == family for s in specs)


def test_the_exits_seen_cover_every_kind_and_one_flag_depends_on_the_band(dcp, oracle64):
    specs, cps = world_specs(), copies()
    seen = {band: {} for band in BANDS}
    band_dependent = []
    for p, spec in enumerate(specs):
        for c, (L, lever) in enumerate(cps):
            r = cpu_pair(dcp, oracle64, p, c)
            for band in BANDS:
                ex, names = r["rs"][band][4:]
                kind = exit_kind(spec, ex, names)
                if kind:
                    seen[band].setdefault(kind, []).append((spec, L, lever))
                if kind == "R alone":  # PR is the only non-finite value of its row: RR = 710, or at band 4 the ring slot of RR = -705
                    assert names == ["PR"] and (lever == "RR710" or (lever, band) == ("RR-705", 4)), (spec, L, lever, band)
            if r["tw"][False, 4][2] != r["tw"][False, 64][2]:
                band_dependent.append((spec, L, lever, r["tw"][False, 4][2]))
    for band in BANDS:
        print("band %d: %s" % (band, {k: len(v) for k, v in sorted(seen[band].items())}))
        assert {"row0", "row1", "row3", "finish", "R alone"} <= set(seen[band]), band
        assert any(w[2] == "RR710" for w in seen[band]["R alone"])
        assert set(LATE_KINDS) <= set(seen[band]), band  # a late row at each phase of the unroll by five
        for M in LATE_M:  # and in every class
            assert set(LATE_KINDS) <= {k for k, v in seen[band].items() if any(w[0][1] == M for w in v)}, (band, M)
        assert all(w[0][0] == "eps0" and w[1] >= 3 for w in seen[band]["row3"] if w[2] == "none")  # the first row with mass
    print("flagged under one band only:", band_dependent)
    # an upward rescaling by 2^1022 can push an older ring slot past the range: band 4 flags what band 64 does not
    assert any(lever == "RR-705" and at4 for _, _, lever, at4 in band_dependent)
    # the float-rule case is a case: in range with double factors somewhere
    assert any(not cpu_pair(dcp, oracle64, p, c)["tw"][False, 64][2] for p in range(len(specs))
               for c, (L, lever) in enumerate(cps) if lever == FLOAT_RULE_ONLY)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
_DEV = {}


class World:
    pass


def device_world(dcp, precision):
    """the world on the device's own tables: per band the scaled twin's (null, alt, out_of_range) matrices [copy, profile]
    and the exit kind of every flagged pair (the restatement, double factors); computed once"""
    if precision not in _DEV:
        W = World()
        W.precision, W.specs, W.copies = precision, world_specs(), copies(precision)
        W.profs = [dcp.ProteinProfile.from_params(*params(s), dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, s[3]),
                                                  "%s%d_%s" % s[:3], precision=precision) for s in W.specs]
        assert [p.core_size for p in W.profs] == [s[1] for s in W.specs]
        W.seqs = [query(L) for L, _ in W.copies]
        W.xt = np.stack([lever_row(xtrans_of(dcp, precision, L, True, False), lever) for L, lever in W.copies])
        assert W.xt.dtype == (np.float64 if precision == 64 else np.float32)
        sc = loaded(dcp, W)
        W.tabs = device_tables(dcp, sc, W.profs, precision, pr.EPS)
        sc.close()
        if precision == 32:  # a float DB's insert and null tables are the host's expansion, at the profile's own epsilon
            for p, s in enumerate(W.specs):
                if s[3] != pr.EPS:
                    W.tabs[p] = W.tabs[p][:2] + (dcp.frame_table_host(W.profs[p].insert_dist, s[3]),
                                                 dcp.frame_table_host(W.profs[p].null_dist, s[3]))
        for p, s in enumerate(W.specs):  # the device holds the world the premises are about
            t8 = np.asarray(W.tabs[p][0], np.float64)
            if s[0] in ("overflow", "eps0"):
                assert float(t8[5, 1:].sum()) > DD_SUM_OUT
            elif s[0] == "near":
                assert 0.0 < float(t8[5, 1:].sum()) < DD_SUM_IN
            elif s[0] == "late":
                assert np.isneginf(t8[2]).all() and (t8[7][:-1] == s[2]).all()  # IM, II (the last node has no insert state)
        W.tabs = [tuple(np.ascontiguousarray(t, np.float64) for t in tab) for tab in W.tabs]  # promoted once, not per call
        W.twin = {band: twin_matrices(dcp, W, band) for band in BANDS}
        # the exit kinds, for the coverage assertions: of every profile with a plain query and of the ordinary profiles
        # with every lever row (the other flagged pairs count for no kind)
        W.kind = {}
        shape = (len(W.copies), len(W.profs))
        W.kind[64] = np.full(shape, None, object)
        for c, p in zip(*np.nonzero(W.twin[64][2])):
            if W.copies[c][1] == "none" or W.specs[p][0] == "ordinary":
                W.kind[64][c, p] = kind_of(W, c, p, 64)
        W.kind[4] = W.kind[64].copy()
        for c, p in zip(*np.nonzero(W.twin[4][2] != W.twin[64][2])):
            W.kind[4][c, p] = kind_of(W, c, p, 4) if W.twin[4][2][c, p] else None
        _DEV[precision] = W
    return _DEV[precision]


def twin_matrices(dcp, W, band):
    shape = (len(W.copies), len(W.profs))
    n, a, oor = np.full(shape, np.nan), np.full(shape, np.nan), np.zeros(shape, bool)
    for c in range(shape[0]):
        for p in range(shape[1]):
            gn, ga, flag = dcp.forward_scaled_tables(*W.tabs[p], W.xt[c], W.seqs[c], float_factors=W.precision == 32, band=band)
            oor[c, p] = flag
            if not flag:
                n[c, p], a[c, p] = gn, ga
    return n, a, oor


def kind_of(W, c, p, band):
    ex, names = fs.restate_scaled(*W.tabs[p], np.asarray(W.xt[c], np.float64), W.seqs[c], band, where=True)[4:]
    if ex is None:  # flagged by the float rule alone
        assert W.precision == 32 and W.copies[c][1] == FLOAT_RULE_ONLY
        return "finish"
    return exit_kind(W.specs[p], ex, names)


def loaded(dcp, W, hooks=False):
    sc = dcp.Scanner(0, lib=dcp.load_testhooks()) if hooks else dcp.Scanner(0)
    sc.upload_db(W.profs)
    sc.upload_seqs(W.seqs)
    (sc.set_xtrans64 if W.precision == 64 else sc.set_xtrans)(W.xt)
    return sc


def same_bits(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def check_list(W, band, sq, pp, got, ref, redone, title):
    """forward_pairs_scaled's (null, alt) of a list against the twin at that band and against forward_pairs' of the same
    list: the redone set is the twin's flagged set and has forward_pairs' bits, every other pair is within the allowances,
    no NaN, -inf exactly where forward_pairs has it"""
    tn, ta, oor = (m[sq, pp] for m in W.twin[band])
    flagged = oor
    for g, r in zip(got, ref):
        assert not np.isnan(g).any() and not np.isnan(r).any()
        assert np.array_equal(g == NEG_INF, r == NEG_INF) and not (g == np.inf).any()
    print("%s f%d band %d: %d pairs, %d flagged by the twin, %d redone; in range vs twin: null %.3e alt %.3e of (|x| + 1)" % (
        title, W.precision, band, len(sq), int(flagged.sum()), redone, worst(got[0][~flagged], tn[~flagged]),
        worst(got[1][~flagged], ta[~flagged])))
    assert redone == int(flagged.sum())
    assert np.array_equal(bits(got[0][flagged]), bits(ref[0][flagged])) and np.array_equal(bits(got[1][flagged]), bits(ref[1][flagged]))
    assert within(got[0][~flagged], tn[~flagged]) and within(got[1][~flagged], ta[~flagged])
    ix = np.nonzero(~flagged)[0]
    if W.precision == 64:
        print("  vs forward_pairs: null %.3e alt %.3e of (|x| + 1)" % (worst(got[0][ix], ref[0][ix]), worst(got[1][ix], ref[1][ix])))
        assert within(got[0][ix], ref[0][ix]) and within(got[1][ix], ref[1][ix])
    else:
        far = 0.0
        for i in ix:
            L, M = len(W.seqs[sq[i]]), W.specs[pp[i]][1]
            for g, r in zip(got, ref):
                if np.isfinite(r[i]):
                    far = max(far, abs(g[i] - r[i]) / fs.allowance_f32(L, M))
        print("  vs forward_pairs: the worst distance is %.3e of its A" % far)
        for i in ix:
            L, M = len(W.seqs[sq[i]]), W.specs[pp[i]][1]
            for g, r in zip(got, ref):
                assert fs.within_f32(g[i:i + 1], r[i:i + 1], L, M), (W.copies[sq[i]], W.specs[pp[i]], g[i], r[i])


def kinds_by_class(W, band, sq, pp):
    out = {}
    for q, p in zip(sq, pp):
        if W.kind[band][q, p]:
            out.setdefault(W.kind[band][q, p], set()).add(size_class(W.specs[p][1]))
    return out


def check_coverage(W, band, sq, pp):
    """each exit kind in each class that can take it: lever rows reach all classes, chains their own, late exits all"""
    got = kinds_by_class(W, band, sq, pp)
    print("f%d band %d, classes per exit kind: %s" % (W.precision, band, {k: sorted(v) for k, v in sorted(got.items())}))
    for kind in ("row0", "row1", "finish", "R alone") + LATE_KINDS:
        assert got.get(kind) == {0, 1, 2, 3}, (band, kind, got.get(kind))
    assert got.get("row3") >= {size_class(M) for M, _ in EPS0}
    for cls in range(4):  # the chains themselves, with no lever: row 1 in their own class
        assert any(W.kind[band][q, p] == "row1" and W.copies[q][1] == "none" and W.specs[p][0] == "overflow" and
                   size_class(W.specs[p][1]) == cls for q, p in zip(sq, pp))
    levers = {W.copies[q][1] for q, p in zip(sq, pp) if W.kind[band][q, p] and W.specs[p][0] == "ordinary"}
    assert levers >= {name for name, _ in LEVERS if "710" in name}


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_exit_in_every_class(dcp, precision):
    W = device_world(dcp, precision)
    sq, pp = fs.shuffled(len(W.copies), len(W.profs), 29)
    for band in (64, 4):
        sc = loaded(dcp, W, hooks=band != 64)
        if band != 64:
            sc.test_set_forward_scale_band(band)
        got = sc.forward_pairs_scaled(sq, pp)
        redone = sc.last_forward_scaled_redo_pairs
        ref = sc.forward_pairs(sq, pp)
        sc.close()
        check_list(W, band, sq, pp, got, ref, redone, "every pair")
        check_coverage(W, band, sq, pp)
    differ = W.twin[4][2] != W.twin[64][2]
    print("flagged under one band only: %s" % [(W.copies[c], W.specs[p]) for c, p in zip(*np.nonzero(differ))])
    assert any(W.copies[c][1] == "RR-705" for c, p in zip(*np.nonzero(differ)))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bits_without_the_neighbours(dcp, precision):
    W = device_world(dcp, precision)
    sq, pp = fs.shuffled(len(W.copies), len(W.profs), 29)
    good = ~W.twin[64][2][sq, pp]
    sc = loaded(dcp, W)
    every = sc.forward_pairs_scaled(sq, pp)
    assert sc.last_forward_scaled_redo_pairs == int((~good).sum()) > 0
    alone = sc.forward_pairs_scaled(sq[good], pp[good])
    assert sc.last_forward_scaled_redo_pairs == 0
    sc.close()
    assert same_bits(alone, (every[0][good], every[1][good]))


def index_of(W, spec=None, copy=None):
    return W.specs.index(spec) if spec else W.copies.index(copy)


def pair_cost(W, q, p):
    """the driver runs a class's pairs by falling rows x chunks, equals in list order"""
    return len(W.seqs[q]) * -(-W.specs[p][1] // pr.WIDE_CHUNK)


def bad_good_lists(W):
    """per class a list bad, good, bad, good, .. in the order the driver runs it (costs never rise), the good pairs in
    turn wider and narrower than the bad pair before them where the class has both.  The bad pairs: a late exit at each
    of the five phases, the overflowing chains, the epsilon-0 chain where there is one, and lever rows on an ordinary
    profile: R alone, the finish, row 0."""
    q12, q6, q4 = (index_of(W, copy=(L, "none")) for L in (12, 6, 4))
    lists = []
    for cls in range(4):
        ordinary = [index_of(W, s) for s in W.specs if s[0] == "ordinary" and size_class(s[1]) == cls]
        bads = [(q12, index_of(W, s)) for s in W.specs if s[0] == "late" and size_class(s[1]) == cls]
        bads += [(q12, index_of(W, s)) for s in W.specs if s[0] in ("overflow", "eps0") and size_class(s[1]) == cls]
        bads += [(index_of(W, copy=(12, lever)), p) for lever, p in zip(("RR710", "ET710", "SB710", "EC710"), ordinary * 2)]
        pairs = []
        for i, (q, p) in enumerate(bads):
            M = W.specs[p][1]
            wider, narrower = [g for g in ordinary if W.specs[g][1] > M], [g for g in ordinary if W.specs[g][1] < M]
            pick = (wider or narrower) if i % 2 == 0 else (narrower or wider)
            pairs += [(q, p), (q12, pick[0] if pick else ordinary[0])]
        if cls == 3:  # by hand, at falling costs: 257 nodes behind a bad 513-node pair and 513 behind a bad 257-node pair
            o257, o513 = index_of(W, ("ordinary", 257, None, pr.EPS)), index_of(W, ("ordinary", 513, None, pr.EPS))
            c257, c513 = index_of(W, ("overflow", 257, 3.0, pr.EPS)), index_of(W, ("overflow", 513, 1.5, pr.EPS))
            pairs = [(q12, c513), (q12, o257)]  # 36, then 24 each
            for s in W.specs:
                if s[0] == "late" and size_class(s[1]) == 3:
                    pairs += [(q12, index_of(W, s)), (q12, o257)]
            for lever in ("RR710", "ET710", "SB710", "EC710"):
                pairs += [(index_of(W, copy=(12, lever)), o257), (q12, o257)]
            pairs += [(q12, c257), (q6, o513), (q4, c513), (q6, o257)]  # 24, 18, 12, 12
            pairs += [(index_of(W, copy=(1, "RR710")), o513), (index_of(W, copy=(1, "none")), o257)]  # 3, 2
        lists.append(pairs)
    return lists


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_wavefront_after_its_bad_pair(dcp, precision):
    W = device_world(dcp, precision)
    oor = W.twin[64][2]
    lists = bad_good_lists(W)
    for cls, pairs in enumerate(lists):  # premises of the lists
        flags = [bool(oor[q, p]) for q, p in pairs]
        costs = [pair_cost(W, q, p) for q, p in pairs]
        assert costs == sorted(costs, reverse=True) and all(size_class(W.specs[p][1]) == cls for _, p in pairs)
        assert flags.count(True) >= 8 and all(flags[i] != flags[i + 1] for i in range(len(flags) - 1)), (cls, flags)
        assert any(flags[i] and not flags[i + 1] for i in range(len(flags) - 1))
        kinds = {W.kind[64][q, p] for q, p in pairs}
        assert kinds >= set(LATE_KINDS) | {"row0", "row1", "finish", "R alone"}, (cls, kinds)
        for i in range(len(pairs) - 1):  # each phase's bad pair has a good pair right behind it
            if W.kind[64][pairs[i]] in LATE_KINDS:
                assert not flags[i + 1], (cls, i)
    widths = [[W.specs[p][1] for _, p in pairs] for pairs in lists]
    assert any(a == 257 and b == 513 for a, b in zip(widths[3], widths[3][1:])) and any(a == 513 and b == 257 for a, b in zip(widths[3], widths[3][1:]))
    mixed = [pairs[i] for i in range(max(map(len, lists))) for pairs in lists if i < len(pairs)]
    sc = loaded(dcp, W, hooks=True)
    for pairs in lists + [mixed]:
        sq, pp = np.array([q for q, _ in pairs]), np.array([p for _, p in pairs])
        sc.test_set_forward_waves(0)
        base = sc.forward_pairs_scaled(sq, pp)
        redone = sc.last_forward_scaled_redo_pairs
        check_list(W, 64, sq, pp, base, sc.forward_pairs(sq, pp), redone, "bad, good, ..")
        for cap in (1, 3):
            sc.test_set_forward_waves(cap)
            got = sc.forward_pairs_scaled(sq, pp)
            assert same_bits(got, base), (cap, [i for i in range(len(sq)) if bits(got[1])[i] != bits(base[1])[i]])
            assert sc.last_forward_scaled_redo_pairs == redone
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_four_classes_on_one_redo_list(dcp, precision):
    W = device_world(dcp, precision)
    oor = W.twin[64][2]
    lists = bad_good_lists(W)
    mixed = [pairs[i] for i in range(max(map(len, lists))) for pairs in lists if i < len(pairs)]
    twice = next(qp for qp in lists[1] if oor[qp])  # one flagged pair three times more, apart from one another
    for at in (3, len(mixed) // 2, len(mixed)):
        mixed.insert(at, twice)
    sq, pp = np.array([q for q, _ in mixed]), np.array([p for _, p in mixed])
    flagged = oor[sq, pp]
    assert {size_class(W.specs[p][1]) for p in pp[flagged]} == {0, 1, 2, 3}
    assert flagged.sum() > 16 and (~flagged).sum() > 16 and (flagged[:-1] != flagged[1:]).sum() > 16  # they interleave
    sc = loaded(dcp, W)
    got = sc.forward_pairs_scaled(sq, pp)
    redone = sc.last_forward_scaled_redo_pairs
    ref = sc.forward_pairs(sq, pp)
    check_list(W, 64, sq, pp, got, ref, redone, "four classes")
    same = [i for i in range(len(mixed)) if mixed[i] == twice]
    assert len(same) == 4 and len({int(b) for b in bits(got[1])[same]}) == 1 and len({int(b) for b in bits(got[0])[same]}) == 1
    again = sc.forward_pairs_scaled(sq, pp)
    assert same_bits(again, got) and sc.last_forward_scaled_redo_pairs == redone
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_dense_scan_with_lever_rows(dcp, precision):
    W = device_world(dcp, precision)
    B, P = len(W.copies), len(W.profs)
    sc = loaded(dcp, W, hooks=True)
    sq, pp = full_list(sc)
    want = tuple(m.reshape(B, P) for m in sc.forward_pairs_scaled(sq, pp))
    flagged = W.twin[64][2]
    assert sc.last_forward_scaled_redo_pairs == int(flagged.sum())
    sc.forward_dense()
    log_space = sc.forward_scores()
    for npairs in (1, 7, P + 1, 0):
        for cap in (0, 1):
            sc.test_set_dense_round(npairs)
            sc.test_set_forward_waves(cap)
            sc.forward_dense_scaled()
            got = sc.forward_scores()
            assert same_matrices(got, want), (precision, npairs, cap)
            assert sc.last_forward_scaled_redo_pairs == int(flagged.sum()), (npairs, cap)
    # every flagged entry has the log-space scan's bits: whole rows of them where a lever flags every profile
    whole = [c for c in range(B) if flagged[c].all()]
    assert {W.copies[c][1] for c in whole} >= {"SB710", "SN710"} and not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    for g, w in zip(got, log_space):
        assert np.array_equal(bits(g[flagged]), bits(w[flagged])) and np.array_equal(bits(g[whole]), bits(w[whole]))
    assert not same_matrices(got, log_space)
    sc.test_set_dense_round(7)
    sc.test_set_forward_waves(0)
    sc.test_set_forward_scale_band(4)
    want4 = tuple(m.reshape(B, P) for m in sc.forward_pairs_scaled(sq, pp))
    assert sc.last_forward_scaled_redo_pairs == int(W.twin[4][2].sum())
    sc.forward_dense_scaled()
    assert same_matrices(sc.forward_scores(), want4) and sc.last_forward_scaled_redo_pairs == int(W.twin[4][2].sum())
    sc.test_set_dense_round(0)
    sc.test_set_forward_scale_band(0)
    # explicit transitions set afterwards void the matrices
    (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(W.xt)
    refused(dcp, sc, sc.forward_scores)
    assert not sc.forward_dense_is_scaled
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_near_the_edge_and_in_range(dcp, precision):
    W = device_world(dcp, precision)
    low = [c for c, (L, lever) in enumerate(W.copies) if "-705" in lever]
    near = [p for p, s in enumerate(W.specs) if s[0] == "near"]
    calm = [p for p, s in enumerate(W.specs) if s[0] in ("ordinary", "near")]

    def stay(c, p):  # the premise, from the twin: in range at every band
        return not (W.twin[4][2][c, p] or W.twin[64][2][c, p] or
                    dcp.forward_scaled_tables(*W.tabs[p], W.xt[c], W.seqs[c], float_factors=precision == 32, band=8)[2])

    pairs = [(c, p) for p in near for c in range(len(W.copies)) if stay(c, p)] + [(c, p) for c in low for p in calm if stay(c, p)]
    assert len(low) == 6 and len(near) == 3
    for p in near:  # each chain with a plain query of every length, each lever row on every calm profile's class
        assert sum(1 for c, q in pairs if q == p and W.copies[c][1] == "none") >= len(QUERY_L)
    for name in {W.copies[c][1] for c in low}:  # (RR = -705 on 12 nt is flagged at band 4: the 1-nt copy stands for it)
        assert {size_class(W.specs[p][1]) for c, p in pairs if W.copies[c][1] == name} == {0, 1, 2, 3}, name
    sq, pp = np.array([c for c, _ in pairs]), np.array([p for _, p in pairs])
    sc = loaded(dcp, W, hooks=True)
    base = sc.forward_pairs_scaled(sq, pp)
    redone = sc.last_forward_scaled_redo_pairs
    check_list(W, 64, sq, pp, base, sc.forward_pairs(sq, pp), redone, "near the edge")
    assert redone == 0 and np.isfinite(base[1]).all()
    for band in (4, 8):
        sc.test_set_forward_scale_band(band)
        got = sc.forward_pairs_scaled(sq, pp)
        assert sc.last_forward_scaled_redo_pairs == 0 and same_bits(got, base), band
    sc.test_set_forward_scale_band(0)
    sc.close()
