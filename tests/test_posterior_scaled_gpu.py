"""The scaled probability-space Backward sweep and posterior rows on the device: dcp_gpu_posterior_pairs_scaled /
Scanner.posterior_pairs_scaled (csrc/dcp_backward_scaled.hip, the row-storing variant of csrc/dcp_forward_scaled.hip;
DESIGN section 25).  The CPU half is tests/test_posterior_scaled.py.

The references are the scaled host twin on the tables the device holds and posterior_pairs on the device, never the code
under test.  Allowances (X: tests/test_posterior_pairs.py's, A: tests/test_forward_scaled.py's allowance_f32):
  device against the scaled twin, either DB           scores 2^-32 (|x| + 1)   rows 4 x 2^-32 (X + 1)
  device against posterior_pairs, double DB           the same
  device against posterior_pairs, float DB            scores A absolute        rows 2 A + 4 x 2^-32 (X + 1)
(the last two are the scaled twin's allowances against dcp_posterior_tables, which posterior_pairs is held to).
alt_fwd has forward_pairs_scaled's bits on the same list; a rerun pair has posterior_pairs' bits."""
import numpy as np
import pytest

import test_forward_chain_premises as pr
import test_forward_pairs as fp
import test_forward_scaled_range as rg
import test_posterior_pairs as tp
from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, np_revcomp, refused
from test_forward_pairs import FLAGS, NEG_INF, PRECISIONS, WORLD_L, WORLD_M, device_tables, within, worst, xtrans_of
from test_forward_scaled import allowance_f32, shuffled
from test_posterior_pairs import same_bits, unpack

_TWIN = {}


def twin_of(dcp, precision, tabs, xt, seq):
    """the scaled twin's (begin, end, core, alt_fwd, alt_bwd, X) on the device's tables, or None if it flags the pair"""
    got = dcp.posterior_scaled_tables(*tabs, xt, seq, float_factors=precision == 32)
    if got[5]:
        return None
    begin, end, core, fwd, bwd = got[:5]
    X = abs(fwd) if np.isfinite(fwd) else 0.0
    if np.isfinite(fwd):  # f + beta = a + log(posterior), as tests/test_posterior_pairs.py's twin_rows reads it back
        for row in (begin, end):
            pos = row[row > 0.0]
            if len(pos):
                X = max(X, float(np.max(np.abs(fwd + np.log(pos)))))
    return begin, end, core, fwd, bwd, X


def world_twin(dcp, precision, orc64, multi, h3):
    key = (precision, multi, h3)
    if key not in _TWIN:
        profs, seqs, tabs = fp.world(dcp, precision, orc64)[:3]
        _TWIN[key] = {(q, p): twin_of(dcp, precision, tabs[p], xtrans_of(dcp, precision, len(s), multi, h3), s)
                      for q, s in enumerate(seqs) for p in range(len(profs))}
    return _TWIN[key]


def check_against_posterior_pairs(precision, got, ref, sq, pp, seqs, profs, skip=()):
    """posterior_pairs of the same list at the allowance of the DB kind; the worst rows |d|"""
    (rows, fwd, bwd), (rrows, rfwd, rbwd) = got, ref
    assert np.array_equal(np.isfinite(fwd), np.isfinite(rfwd)) and np.array_equal(np.isfinite(bwd), np.isfinite(rbwd))
    assert not np.isnan(fwd).any() and not np.isnan(bwd).any()
    d_worst = 0.0
    for i in range(len(sq)):
        if i in skip:
            continue
        X = abs(rfwd[i]) if np.isfinite(rfwd[i]) else 0.0  # at most the pair's X: a tighter allowance
        A = allowance_f32(len(seqs[sq[i]]), profs[pp[i]].core_size) if precision == 32 else 0.0
        if precision == 64:
            assert within([fwd[i]], [rfwd[i]]) and within([bwd[i]], [rbwd[i]]), (i, fwd[i], rfwd[i])
        elif np.isfinite(rfwd[i]):
            assert abs(fwd[i] - rfwd[i]) <= A and abs(bwd[i] - rbwd[i]) <= A, (i, fwd[i], rfwd[i], A)
        for g, w in zip(rows[i], rrows[i]):
            assert g.shape == w.shape and not np.isnan(g).any()
            d = float(np.max(np.abs(g - w)))
            d_worst = max(d_worst, d)
            assert d <= 2.0 * A + tp.rows_allow(X), (i, d, A, X)
    return d_worst


@pytest.mark.gpu
@pytest.mark.parametrize("multi,h3", FLAGS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_class_edges_against_the_twin_and_posterior_pairs(dcp, oracle64, precision, multi, h3):
    profs, seqs = fp.world(dcp, precision, oracle64)[:2]
    assert {64, 65, 128, 129, 256, 257, 512, 513} <= set(WORLD_M) and {1, 5, 6, 333} <= set(WORLD_L)
    assert (513 + 255) // 256 == 3  # a three-chunk width
    twin = world_twin(dcp, precision, oracle64, multi, h3)
    assert all(t is not None for t in twin.values())  # the twin flags none of them
    sq, pp = shuffled(len(seqs), len(profs), 19)
    sc = fp.loaded(dcp, precision)
    assert sc.posterior_scaled_kernel_ms < 0
    res = sc.posterior_pairs_scaled(sq, pp, multi, h3)
    assert sc.posterior_scaled_kernel_ms > 0 and sc.last_posterior_scaled_redo_pairs == 0
    ref = sc.posterior_pairs(sq, pp, multi, h3)
    fs = sc.forward_pairs_scaled(sq, pp, multi, h3)
    sc.close()
    assert res[0].tolist() == ref[0].tolist()
    rows, fwd, bwd = unpack(res)
    assert np.array_equal(bits(fwd), bits(fs[1]))  # one sweep: forward_pairs_scaled's bits
    ws, wr = tp.check_against(rows, fwd, bwd, [twin[q, p] for q, p in zip(sq, pp)], (precision, multi, h3))
    d = check_against_posterior_pairs(precision, (rows, fwd, bwd), unpack(ref), sq, pp, seqs, profs)
    print("scaled device vs scaled twin f%d multi %d h3 %d: scores %.3e, rows %.3e of (X + 1); vs posterior_pairs: rows |d| %.3e" % (
        precision, multi, h3, ws, wr, d))
    assert np.isfinite(fwd).sum() > len(sq) // 2
    for (b, e, c), a in zip(rows, fwd):
        assert e[0] == 0.0 and c[0] == 0.0
        if a == NEG_INF:
            assert not b.any() and not e.any() and not c.any()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bands_wavefront_caps_and_budgets_change_no_bit(dcp, oracle64, precision):
    profs, seqs = fp.world(dcp, precision, oracle64)[:2]
    sc = fp.loaded(dcp, precision, dcp.load_testhooks())
    sq, pp = shuffled(len(seqs), len(profs), 19)
    base = sc.posterior_pairs_scaled(sq, pp)
    assert sc.last_posterior_scaled_redo_pairs == 0
    for band in (4, 8):  # the wide class's work-area rings too
        sc.test_set_forward_scale_band(band)
        assert same_bits(sc.posterior_pairs_scaled(sq, pp), base), band
        assert sc.last_posterior_scaled_redo_pairs == 0
    sc.test_set_forward_scale_band(0)
    ix = {M: i for i, M in enumerate(WORLD_M)}
    q = WORLD_L.index(100)
    pairs = [(q, ix[1100]), (q, ix[257]), (q, ix[1100]), (q, ix[2]), (q, ix[513])]
    pairs += [(8, ix[512]), (7, ix[64]), (8, ix[129]), (5, ix[1100]), (8, len(WORLD_M)), (6, ix[256]), (0, ix[63]), (3, ix[128])]
    sq, pp = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    base = sc.posterior_pairs_scaled(sq, pp)
    for cap in (3, 1, 0):
        sc.test_set_forward_waves(cap)
        assert same_bits(sc.posterior_pairs_scaled(sq, pp), base), cap
    # 80 bytes of records a row: rounds of a few pairs, rounds of one pair (every pair of 100 or 333 nt alone), one round
    for budget in (250 * 80, 20 * 80, 1, 0):
        sc.test_set_posterior_budget(budget)
        assert same_bits(sc.posterior_pairs_scaled(sq, pp), base), budget
    sc.test_set_posterior_budget(250 * 80)
    sc.test_set_forward_waves(1)
    assert same_bits(sc.posterior_pairs_scaled(sq, pp), base)
    sc.close()


def redo_world(dcp, orc64, precision):
    """normal profiles of every class with the 2 000-node positive chain and an insert-loop profile of
    tests/test_forward_scaled_range.py's late family (IM = -inf, II = +96, 70 nodes) among them; the flagged indices"""
    profs, seqs = fp.world(dcp, precision, orc64)[:2]
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
    big = dcp.ProteinProfile.from_params(*pr.chain_params("positive", 2000), cfg, "POS2000", precision=precision)
    loop = dcp.ProteinProfile.from_params(*rg.params(("late", 70, 96.0, pr.EPS)), cfg, "LOOP70", precision=precision)
    keep = [WORLD_M.index(M) for M in (2, 64, 129, 256, 513)]
    mine = [profs[i] for i in keep[:2]] + [big] + [profs[i] for i in keep[2:4]] + [loop] + [profs[keep[4]]]
    qs = [seqs[WORLD_L.index(L)] for L in (6, 17, 100)]
    return mine, qs, (2, 5)


def twin_flags(dcp, sc, mine, qs, precision, sq, pp):
    tabs = device_tables(dcp, sc, mine, precision, float(np.float32(0.01)))
    return np.array([twin_of(dcp, precision, tabs[p], xtrans_of(dcp, precision, len(qs[q]), True, False), qs[q]) is None
                     for q, p in zip(sq, pp)])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_redo_of_flagged_pairs(dcp, oracle64, precision):
    mine, qs, bad = redo_world(dcp, oracle64, precision)
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    sc.upload_db(mine)
    sc.upload_seqs(qs)
    sq, pp = shuffled(len(qs), len(mine), 5)
    flagged = twin_flags(dcp, sc, mine, qs, precision, sq, pp)
    # the twin flags the chain on every query and the loop where the query is long enough for it to multiply up
    assert flagged[pp == bad[0]].all() and flagged[(pp == bad[1]) & (sq == 2)].all() and not flagged[~np.isin(pp, bad)].any()
    res = sc.posterior_pairs_scaled(sq, pp)
    assert sc.last_posterior_scaled_redo_pairs == int(flagged.sum()) >= 4
    ref = sc.posterior_pairs(sq, pp)
    rows, fwd, bwd = unpack(res)
    rrows, rfwd, rbwd = unpack(ref)
    assert not np.isnan(res[1]).any() and not np.isnan(res[2]).any() and not np.isnan(res[3]).any()
    for i in np.nonzero(flagged)[0]:  # flagged pairs have posterior_pairs' bits
        assert same_bits(rows[i], rrows[i]) and bits(fwd[i:i + 1]) == bits(rfwd[i:i + 1]) and bits(bwd[i:i + 1]) == bits(rbwd[i:i + 1]), i
    assert np.isfinite(rfwd[flagged]).all()
    check_against_posterior_pairs(precision, (rows, fwd, bwd), (rrows, rfwd, rbwd), sq, pp, qs, mine)
    # ... and the others the bits they have without the flagged ones in the list
    orows, ofwd, obwd = unpack(sc.posterior_pairs_scaled(sq[~flagged], pp[~flagged]))
    assert sc.last_posterior_scaled_redo_pairs == 0
    keep = np.nonzero(~flagged)[0]
    assert all(same_bits(orows[n], rows[i]) for n, i in enumerate(keep))
    assert np.array_equal(bits(ofwd), bits(fwd[keep])) and np.array_equal(bits(obwd), bits(bwd[keep]))

    # one wavefront runs bad, good, bad, good pairs, and the same pair appears twice in the list
    sq2, pp2 = np.array([2, 2, 2, 2, 2, 2]), np.array([bad[0], 1, bad[1], 3, bad[0], 1])
    whole = unpack(sc.posterior_pairs_scaled(sq2, pp2))
    assert sc.last_posterior_scaled_redo_pairs == 3
    sc.test_set_forward_waves(1)
    one = unpack(sc.posterior_pairs_scaled(sq2, pp2))
    assert sc.last_posterior_scaled_redo_pairs == 3
    want = unpack(sc.posterior_pairs(sq2, pp2))
    for i in range(6):
        assert same_bits(one[0][i], whole[0][i]) and bits(one[2][i:i + 1]) == bits(whole[2][i:i + 1])
        if pp2[i] in bad:
            assert same_bits(one[0][i], want[0][i]) and bits(one[1][i:i + 1]) == bits(want[1][i:i + 1])
    assert same_bits(one[0][0], one[0][4]) and same_bits(one[0][1], one[0][5])
    # a flagged pair on a round boundary: rounds of one pair, and of two (101 rows each, 80 bytes a row)
    for budget in (1, 2 * 101 * 80):
        sc.test_set_posterior_budget(budget)
        got = unpack(sc.posterior_pairs_scaled(sq2, pp2))
        assert sc.last_posterior_scaled_redo_pairs == 3
        assert all(same_bits(got[0][i], one[0][i]) for i in range(6)) and same_bits(got[1:], one[1:]), budget
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_batches_transitions_and_refusals(dcp, oracle64, precision):
    profs, seqs, tabs = fp.world(dcp, precision, oracle64)[:3]

    def wants(sq, pp, seq_of, xt_of):
        return [twin_of(dcp, precision, tabs[p], xt_of(q), seq_of(q)) for q, p in zip(sq, pp)]

    std = lambda s: xtrans_of(dcp, precision, len(s), True, False)  # noqa: E731
    sc = dcp.Scanner(0)
    refused(dcp, sc, lambda: sc.posterior_pairs_scaled([0], [0]))  # no DB
    sc.upload_db(profs)
    refused(dcp, sc, lambda: sc.posterior_pairs_scaled([0], [0]))  # no batch
    sc.upload_seqs(seqs)
    row_off, begin, end, core, fwd, bwd = sc.posterior_pairs_scaled([], [])
    assert row_off.tolist() == [0] and begin.shape == fwd.shape == (0,) and sc.posterior_scaled_kernel_ms < 0
    with pytest.raises(dcp.DcpError) as e:
        sc.posterior_pairs_scaled([0, len(seqs), 99], [0, 0, 99])
    assert e.value.rc == dcp.RC_EINVAL and "pair 1 " in str(e.value)
    refused(dcp, sc, lambda: sc.posterior_pairs_scaled([0, 1], [0]))
    # capacity and null outputs: refused, everything untouched
    sq, pp = np.array([8, 5], np.uint32), np.array([0, 3], np.uint32)
    need = len(seqs[8]) + len(seqs[5]) + 2
    off = np.full(3, 7, np.uint64)
    rows = [np.full(need, 1.5) for _ in range(3)]
    fwd, bwd = np.full(2, 2.5), np.full(2, 2.5)
    call = sc._lib.dcp_gpu_posterior_pairs_scaled
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def run(sq_=sq, pp_=pp, off_=off, rows_=rows, cap=need, fwd_=fwd, bwd_=bwd):
        return call(sc._c, 1, 0, P(sq_), P(pp_), 2, P(off_), P(rows_[0]), P(rows_[1]), P(rows_[2]), cap, P(fwd_), P(bwd_))

    def untouched():
        return off.tolist() == [7, 7, 7] and all((r == 1.5).all() for r in rows) and (fwd == 2.5).all() and (bwd == 2.5).all()

    assert run(cap=need - 1) == dcp.RC_EINVAL and untouched()
    assert str(need) in sc._lib.dcp_gpu_last_error(sc._c).decode()
    for change in (dict(sq_=None), dict(pp_=None), dict(off_=None), dict(rows_=[None, rows[1], rows[2]]),
                   dict(rows_=[rows[0], rows[1], None]), dict(fwd_=None), dict(bwd_=None), dict(sq_=np.array([8, 99], np.uint32))):
        assert run(**change) == dcp.RC_EINVAL and untouched(), change
    assert sc.posterior_scaled_kernel_ms < 0 and sc.posterior_kernel_ms < 0
    assert run() == 0 and off.tolist() == [0, len(seqs[8]) + 1, need] and np.isfinite(fwd).all() and not (rows[0] == 1.5).any()
    assert sc.posterior_scaled_kernel_ms > 0 and sc.posterior_kernel_ms < 0  # posterior_pairs' clock is its own
    # a list with duplicates comes back in list order
    sq, pp = np.array([7, 8, 7, 7, 3, 8]), np.array([11, 4, 11, 11, 0, 4])
    rows_, fwd_, bwd_ = unpack(sc.posterior_pairs_scaled(sq, pp))
    tp.check_against(rows_, fwd_, bwd_, wants(sq, pp, lambda q: seqs[q], lambda q: std(seqs[q])), precision)
    assert same_bits(rows_[0], rows_[2]) and same_bits(rows_[0], rows_[3]) and same_bits(rows_[1], rows_[5])
    # explicit transitions in the DB's precision are honoured, those of the other refused
    xt = np.stack([xtrans_of(dcp, precision, len(s) + 50, False, False) for s in seqs])
    (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(xt)
    sq, pp = np.array([8, 7, 4, 8, 2]), np.array([12, 9, 5, 11, 1])
    rows_, fwd_, bwd_ = unpack(sc.posterior_pairs_scaled(sq, pp, True, False))
    tp.check_against(rows_, fwd_, bwd_, wants(sq, pp, lambda q: seqs[q], lambda q: xt[q]), precision)
    other = np.stack([xtrans_of(dcp, 96 - precision, len(s), True, False) for s in seqs])
    (sc.set_xtrans if precision == 64 else sc.set_xtrans64)(other)
    refused(dcp, sc, lambda: sc.posterior_pairs_scaled(sq, pp))
    sc.close()

    # both strands, windows
    sc = fp.loaded(dcp, precision)
    n = len(seqs)
    sc.add_reverse_strand()
    sq, pp = np.array([n + 8, n + 7, 8, n + 5]), np.array([9, 12, 9, 2])
    strand = lambda q: np_revcomp(seqs[q % n]) if q >= n else seqs[q % n]  # noqa: E731
    rows_, fwd_, bwd_ = unpack(sc.posterior_pairs_scaled(sq, pp))
    tp.check_against(rows_, fwd_, bwd_, wants(sq, pp, strand, lambda q: std(seqs[q % n])), precision)
    sc.upload_seqs([seqs[8], seqs[7]])
    sc.cut_windows(64, 40)
    sq, pp = np.arange(sc.nseqs), np.arange(sc.nseqs) % len(profs)
    rows_, fwd_, bwd_ = unpack(sc.posterior_pairs_scaled(sq, pp))
    assert sc.nseqs > 2
    tp.check_against(rows_, fwd_, bwd_, wants(sq, pp, sc.fetch_seq, lambda q: std(sc.fetch_seq(q))), precision)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nothing_else_moves(dcp, oracle64, precision):
    fp.world(dcp, precision, oracle64)
    sc = fp.loaded(dcp, precision)
    sq, pp = np.array([8, 7, 6, 8, 3]), np.array([11, 3, 0, 12, 9])

    def flat(x):
        if isinstance(x, (tuple, list)):
            return [flat(v) for v in x]
        return np.ascontiguousarray(x).tobytes()

    sc.scan(True, False, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    sc.forward_dense(False, False)

    def state():
        return (flat(sc.scores()), sc.hits().tobytes(), sc.cells, sc.last_scan_launches, flat(sc.forward_pairs(sq, pp)),
                flat(sc.forward_pairs_scaled(sq, pp)), flat(sc.posterior_pairs(sq, pp)), flat(sc.forward_scores()),
                flat(sc.mea_pairs(sq, pp)), sc.forward_dense_is_scaled)

    before = state()
    assert len(sc.hits()) > 0
    ms = sc.posterior_kernel_ms
    got = sc.posterior_pairs_scaled(sq, pp, False, False)  # other flags than the scan's
    assert np.isfinite(got[4]).all() and sc.posterior_scaled_kernel_ms > 0
    assert sc.posterior_kernel_ms == ms  # posterior_pairs' clock is its own
    assert state() == before
    sc.close()
