"""Posterior envelopes of a pair list found on the device: the envelope kernels alone, through the test-hooks build's
dcp_gpu_test_envelopes_of_rows on rows made here, and dcp_gpu_envelope_pairs, in both precisions.

The reference is the host twin (dcp_posterior_envelope_records, tests/test_envelopes.py checks it on the CPU against a
numpy restatement) applied to the same rows: rows made here, or the rows posterior_pairs / posterior_pairs_scaled return
for the same list.  env_off, pair, begin, end, peak and core_max must agree in bits; each of the three sums is a run's own
n = end - begin terms added in another order: |device - twin| <= n 2^-52 sum|term| is asserted for every record
(test_envelopes.sums_agree), and the device's sum is also held to (n - 1) 2^-53 sum|term| of the exact sum
(test_envelopes.sums_within), the bound of any order of addition."""
import numpy as np
import pytest

import test_forward_pairs as fp
from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, refused
from test_envelopes import EXACT, exact_fields, restate, same_records, sums_agree
from test_forward_pairs import FLAGS, NEG_INF, PRECISIONS, xtrans_of
from test_gpu_parity import pfam_like_params, planted_query
from test_posterior_pairs import same_bits, unpack

HI, LO = 0.5, 0.1
SUM_FIELDS = ("core_sum", "begin_sum", "end_sum")


# ---- the kernel alone: rows made here ----------------------------------------------------------------------------
def rows_with_runs(rng, L, runs, peak=True):
    """rows [L + 1]: core in [LO, HI) on the runs' bases and below LO elsewhere, one value >= HI per run if `peak`"""
    begin, end, core = rng.random(L + 1) * 0.2, rng.random(L + 1) * 0.2, rng.random(L + 1) * LO * 0.99
    for s, e in runs:
        core[s + 1:e + 1] = LO + rng.random(e - s) * (HI - LO) * 0.99
        if peak:
            core[s + 1 + rng.integers(0, e - s)] = HI + rng.random() * (1.0 - HI)
    core[0] = end[0] = 0.0
    return begin, end, core


def synthetic_pairs():
    """[(begin, end, core)]: the run patterns at which the wavefront's chunks of 64 bases can go wrong"""
    rng = np.random.default_rng(2626)
    pairs = []
    for L in (1, 63, 64, 65, 127, 128, 129, 200):
        # random rows, all ones, all zeros, a run to the last base
        pairs.append((rng.random(L + 1) * 0.2, rng.random(L + 1) * 0.2, np.concatenate([[0.0], rng.random(L)])))
        pairs.append(rows_with_runs(rng, L, [(0, L)]))
        pairs.append(rows_with_runs(rng, L, []))
        pairs.append(rows_with_runs(rng, L, [(L - min(L, 4), L)]))
    for edge in (64, 128):  # every run that ends at lane 63, starts at lane 0 or spans the chunk edge
        for s in range(edge - 4, edge + 3):
            for e in range(s + 1, edge + 7):
                L = (edge + 1, edge + 63, 200)[(s + e) % 3]
                pairs.append(rows_with_runs(rng, max(L, e), [(s, e)], peak=(s * e) % 5 != 0))
    pairs.append(rows_with_runs(rng, 200, [(30, 170)]))  # a run over three chunks
    pairs.append(rows_with_runs(rng, 200, [(64 + 2 * k, 65 + 2 * k) for k in range(32)]))  # 32 one-base runs in a chunk
    pairs.append(rows_with_runs(rng, 129, [(2 * k, 2 * k + 1) for k in range(64)]))
    b, e, c = rows_with_runs(rng, 129, [(50, 80)], peak=False)  # the only value >= hi in the run's second chunk
    c[70 + 1] = 0.9
    pairs.append((b, e, c))
    b, e, c = rows_with_runs(rng, 129, [(50, 80)], peak=False)  # two equal maxima, one per chunk: the first
    c[60 + 1] = c[70 + 1] = 0.9
    pairs.append((b, e, c))
    b, e, c = rows_with_runs(rng, 200, [(10, 150)], peak=False)  # three equal maxima, the largest of its chunk each
    c[20 + 1] = c[100 + 1] = c[130 + 1] = 0.75
    pairs.append((b, e, c))
    b, e, c = rows_with_runs(rng, 129, [(60, 64), (64 + 3, 64 + 9)])  # min_len: runs of 4 and 6 bases at a chunk's end
    pairs.append((b, e, c))
    b, e, c = rows_with_runs(rng, 65, [])  # -1e-17 as 1 - (a sum past 1) leaves it, for lo = 0
    c[1:] = np.where(rng.random(65) < 0.5, -1e-17, 0.0)
    c[64] = 0.7
    pairs.append((b, e, c))
    while len(pairs) < 320:  # and random rows of random lengths
        L = int(rng.integers(1, 260))
        runs, at = [], 0
        while True:
            s = at + int(rng.integers(1, 60))
            e = s + int(rng.integers(1, 90))
            if e > L:
                break
            runs.append((s, e))
            at = e
        pairs.append(rows_with_runs(rng, L, runs, peak=bool(rng.integers(0, 2))))
    return pairs


def packed(pairs, order):
    """(row_off, begin, end, core) of the pairs in the given order"""
    off = np.concatenate([[0], np.cumsum([len(pairs[i][2]) for i in order])]).astype(np.uint64)
    return (off,) + tuple(np.concatenate([pairs[i][k] for i in order]) for k in range(3))


def twin_list(dcp, rows, hi, lo, min_len):
    """(env_off, records) of the host twin over a list of (begin, end, core), pair = the list index"""
    off, recs = [0], []
    for i, (b, e, c) in enumerate(rows):
        r = dcp.posterior_envelope_records(b, e, c, hi, lo, min_len)
        r["pair"] = i
        recs.append(r)
        off.append(off[-1] + len(r))
    return np.array(off, np.uint64), np.concatenate(recs) if recs else np.zeros(0, dcp.ENVELOPE_DTYPE)


def against_twin(dcp, got_off, got, rows, hi, lo, min_len, what=""):
    """device records against the twin's on the same rows: offsets and exact fields in bits both ways, every sum within
    n 2^-52 sum|term| of the twin's and within (n - 1) 2^-53 sum|term| of the exact sum of the run's own terms; returns
    the twin's records"""
    want_off, want = twin_list(dcp, rows, hi, lo, min_len)
    assert got_off.dtype == np.uint64 and np.array_equal(got_off, want_off), (what, got_off.tolist()[:20], want_off.tolist()[:20])
    assert got.dtype == dcp.ENVELOPE_DTYPE and len(got) == len(want)
    assert exact_fields(got) == exact_fields(want), what  # the same bytes: device -> twin and twin -> device
    for i, (b, e, c) in enumerate(rows):
        mine, twin = got[int(got_off[i]):int(got_off[i + 1])], want[int(want_off[i]):int(want_off[i + 1])]
        runs = restate(b, e, c, hi, lo, min_len, pair=i)
        same_records(mine, runs, (what, i))
        for k, run in enumerate(runs):
            sums_agree(mine[k], twin[k], run, (what, i, k))
    return want


@pytest.fixture(scope="module")
def hooked(dcp):
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    yield sc
    sc.close()


@pytest.mark.gpu
def test_the_kernel_alone_on_every_run_pattern(dcp, hooked):
    pairs = synthetic_pairs()
    assert len(pairs) >= 300
    order = list(range(len(pairs)))
    off, env = hooked.test_envelopes_of_rows(*packed(pairs, order), HI, LO, 1)
    want = against_twin(dcp, off, env, pairs, HI, LO, 1, "in order")
    assert len(env) > 200 and (env["end"] > 64).any() and ((env["begin"] < 64) & (env["end"] > 64)).any()
    worst = max(abs(float(g[f]) - float(w[f])) / max(abs(float(w[f])), 1e-300) for g, w in zip(env, want) for f in SUM_FIELDS)
    print("the sums against the twin's: largest relative difference %.3e over %d records" % (worst, len(env)))
    # other thresholds: lo == hi, lo = 0 (the -1e-17 row), nothing reaches hi, everything above lo
    for hi, lo in ((HI, HI), (LO, LO), (HI, 0.0), (0.0, 0.0), (2.0, LO), (HI, -1.0)):
        o, v = hooked.test_envelopes_of_rows(*packed(pairs, order), hi, lo, 1)
        against_twin(dcp, o, v, pairs, hi, lo, 1, (hi, lo))
        if lo == hi:
            for i, (b, e, c) in enumerate(pairs):
                mine = v[int(o[i]):int(o[i + 1])]
                assert [(int(r["begin"]), int(r["end"])) for r in mine] == dcp.posterior_envelopes(c, hi, 1)
    # min_len at a run's length and one above
    for min_len in (0, 4, 5, 6, 7, 1000):
        o, v = hooked.test_envelopes_of_rows(*packed(pairs, order), HI, LO, min_len)
        against_twin(dcp, o, v, pairs, HI, LO, min_len, min_len)
        assert min_len == 0 or not len(v) or (v["end"] - v["begin"]).min() >= min_len
    lens = (env["end"] - env["begin"]).tolist()
    assert 4 in lens and 6 in lens  # so 4 -> 5 and 6 -> 7 each drop runs


@pytest.mark.gpu
def test_the_kernel_alone_shuffled_repeated_and_with_few_wavefronts(dcp, hooked):
    pairs = synthetic_pairs()
    rng = np.random.default_rng(27)
    order = rng.permutation(len(pairs)).tolist()
    order += order[:7] + [order[0]] * 3  # pairs listed twice, and one four times, behind each other too
    rows = [pairs[i] for i in order]
    base_off, base = hooked.test_envelopes_of_rows(*packed(pairs, order), HI, LO, 1)
    against_twin(dcp, base_off, base, rows, HI, LO, 1, "shuffled")
    try:
        for cap in (1, 3, 64, 0):  # one wavefront takes every pair in turn: an open run must not reach the next pair
            hooked.test_set_forward_waves(cap)
            off, env = hooked.test_envelopes_of_rows(*packed(pairs, order), HI, LO, 1)
            assert np.array_equal(off, base_off) and env.tobytes() == base.tobytes(), cap
            off, env = hooked.test_envelopes_of_rows(*packed(pairs, order), HI, LO, 5)
            against_twin(dcp, off, env, rows, HI, LO, 5, cap)
    finally:
        hooked.test_set_forward_waves(0)
    # a list whose first offset is not 0
    off4 = packed(pairs, order[:40])
    o, v = hooked.test_envelopes_of_rows(off4[0] + np.uint64(5), *[np.concatenate([np.full(5, 0.9), a]) for a in off4[1:]], HI, LO, 1)
    against_twin(dcp, o, v, rows[:40], HI, LO, 1, "offset")


@pytest.mark.gpu
def test_the_hook_refuses_and_reports_the_need(dcp, hooked):
    pairs = synthetic_pairs()[:40]
    off, b, e, c = packed(pairs, range(len(pairs)))
    want_off, want = twin_list(dcp, pairs, HI, LO, 1)
    need = len(want)
    out = np.zeros(need, dcp.ENVELOPE_DTYPE)
    out["pair"] = 77
    eo = np.full(len(pairs) + 1, 7, np.uint64)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    nan = float("nan")

    def run(off_=off, b_=b, e_=e, c_=c, n=len(pairs), hi=HI, lo=LO, out_=out, cap=need, eo_=eo):
        return hooked._lib.dcp_gpu_test_envelopes_of_rows(hooked._c, P(off_), P(b_), P(e_), P(c_), n, hi, lo, 1, P(out_), cap, P(eo_))

    flat = off.copy()
    flat[3] = flat[2]  # a pair without a row
    for change in (dict(hi=nan), dict(lo=nan), dict(hi=LO, lo=HI), dict(off_=None), dict(b_=None), dict(e_=None), dict(c_=None),
                   dict(out_=None), dict(eo_=None), dict(off_=flat)):
        assert run(**change) == dcp.RC_EINVAL, change
        assert (eo == 7).all() and (out["pair"] == 77).all(), change
    assert run(cap=need - 1) == dcp.RC_ENOMEM and np.array_equal(eo, want_off) and (out["pair"] == 77).all()
    eo[:] = 7
    assert run(n=0) == 0 and eo[0] == 0 and (eo[1:] == 7).all()
    assert run() == 0 and np.array_equal(eo, want_off) and exact_fields(out) == exact_fields(want)


# ---- the call: the world of tests/test_forward_pairs.py and planted genes ---------------------------------------------
_WORLD = {}
PLANT = ((63, 0, 9), (64, 0, 10), (65, 0, 15), (128, 1, 20), (129, 1, 30), (200, 1, 40))  # (query length, gene, its first base)
PLANT_M = (15, 30)


def env_world(dcp, precision, orc32, orc64):
    """fp.world's profiles and queries, two small profiles and six queries of 63 .. 200 nt that carry a gene of one of
    them; the planted (query, profile) pairs"""
    if precision not in _WORLD:
        profs, seqs = fp.world(dcp, precision, orc64)[:2]
        rng = np.random.default_rng(2600 + precision)
        orc = orc64 if precision == 64 else orc32
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
        params = [pfam_like_params(rng, M) for M in PLANT_M]
        mine = list(profs) + [dcp.ProteinProfile.from_params(*prm, cfg, f"ENV{i}", precision=precision) for i, prm in enumerate(params)]
        genes = [planted_query(rng, orc.new(*prm, ENTRY_DIST_OCCUPANCY, 0.01), M, flank=0) for prm, M in zip(params, PLANT_M)]
        qs, planted = list(seqs), []
        for L, g, at in PLANT:
            q = rng.integers(0, 4, L, dtype=np.uint8)
            q[at:at + len(genes[g])] = genes[g]
            planted.append((len(qs), len(profs) + g, at, at + len(genes[g])))
            qs.append(q)
        _WORLD[precision] = (mine, qs, planted)
    return _WORLD[precision]


def loaded(dcp, precision, lib=None):
    mine, qs = _WORLD[precision][:2]
    sc = dcp.Scanner(0, lib=lib) if lib else dcp.Scanner(0)
    sc.upload_db(mine)
    sc.upload_seqs(qs)
    return sc


def every_pair(mine, qs, seed):
    every = [(q, p) for q in range(len(qs)) for p in range(len(mine))]
    order = np.random.default_rng(seed).permutation(len(every))
    return np.array([every[i][0] for i in order]), np.array([every[i][1] for i in order])


def against_rows(dcp, got, res, hi=HI, lo=LO, min_len=1, what=""):
    """envelope_pairs' result against the twin on a posterior call's result for the same list, and the scores' bits"""
    off, env, fwd, bwd = got
    rows, rfwd, rbwd = unpack(res)
    assert np.array_equal(bits(fwd), bits(rfwd)) and np.array_equal(bits(bwd), bits(rbwd)), what
    return against_twin(dcp, off, env, rows, hi, lo, min_len, what)


@pytest.mark.gpu
@pytest.mark.parametrize("multi,h3", FLAGS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_pair_against_the_twin_on_the_rows(dcp, oracle32, oracle64, precision, multi, h3):
    mine, qs, planted = env_world(dcp, precision, oracle32, oracle64)
    sq, pr = every_pair(mine, qs, 26)
    sc = loaded(dcp, precision, dcp.load_testhooks())  # (the hooks build: for the envelope kernels' own clock)
    assert sc.envelope_kernel_ms < 0 and sc.test_envelope_records_kernel_ms < 0  # none has run
    res = sc.posterior_pairs(sq, pr, multi, h3)
    # the condition on the inputs, first: on posterior_pairs' own rows the twin finds an envelope for every planted pair,
    # which overlaps the gene, and one of them crosses base 64
    rows = unpack(res)[0]
    crossing = 0
    for q, p, g0, g1 in planted:
        i = int(np.nonzero((sq == q) & (pr == p))[0][0])
        env = dcp.posterior_envelope_records(*rows[i], HI, LO)
        assert len(env) >= 1 and any(min(int(r["end"]), g1) > max(int(r["begin"]), g0) for r in env), (q, p, env)
        crossing += sum(int(r["begin"]) < 64 < int(r["end"]) for r in env)
    assert crossing >= 1
    got = sc.envelope_pairs(sq, pr, multi, h3, HI, LO, scaled=False)
    assert sc.envelope_kernel_ms > 0 and 0 < sc.test_envelope_records_kernel_ms < sc.envelope_kernel_ms
    want = against_rows(dcp, got, res, what=("log", precision, multi, h3))
    res_s = sc.posterior_pairs_scaled(sq, pr, multi, h3)
    got_s = sc.envelope_pairs(sq, pr, multi, h3, HI, LO)  # scaled is the default
    against_rows(dcp, got_s, res_s, what=("scaled", precision, multi, h3))
    sc.close()
    print("f%d multi %d h3 %d: %d pairs, %d envelopes, %d cross base 64 in the planted pairs" % (precision, multi, h3, len(sq),
                                                                                              len(want), crossing))
    # a pair without a path has rows of 0: no envelope
    for i in np.nonzero(got[2] == NEG_INF)[0]:
        assert got[0][i] == got[0][i + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_knobs_change_no_bit(dcp, oracle32, oracle64, precision):
    mine, qs, planted = env_world(dcp, precision, oracle32, oracle64)
    sq, pr = every_pair(mine, qs, 27)
    keep = np.concatenate([np.arange(60), [int(np.nonzero((sq == q) & (pr == p))[0][0]) for q, p, _, _ in planted]])
    sq, pr = sq[keep], pr[keep]
    sc = loaded(dcp, precision, dcp.load_testhooks())
    try:
        for scaled in (True, False):
            res = (sc.posterior_pairs_scaled if scaled else sc.posterior_pairs)(sq, pr)
            base = sc.envelope_pairs(sq, pr, hi=HI, lo=LO, scaled=scaled)
            against_rows(dcp, base, res, what=("base", scaled))
            assert len(base[1]) >= len(planted)
            # lo == hi: posterior_envelopes' intervals, pair by pair
            off, env, _, _ = got = sc.envelope_pairs(sq, pr, hi=HI, scaled=scaled)
            against_rows(dcp, got, res, HI, HI, what=("lo == hi", scaled))
            for i, (b, e, c) in enumerate(unpack(res)[0]):
                mine_ = env[int(off[i]):int(off[i + 1])]
                assert [(int(r["begin"]), int(r["end"])) for r in mine_] == dcp.posterior_envelopes(c, HI)
            # 80 bytes of records a row: rounds of a few pairs, of one pair, and a budget no pair fits
            for budget in (700 * 80, 20 * 80, 1, 0):
                sc.test_set_posterior_budget(budget)
                got = sc.envelope_pairs(sq, pr, hi=HI, lo=LO, scaled=scaled)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base)), (budget, scaled)
            for cap in (1, 3, 0):
                sc.test_set_forward_waves(cap)
                got = sc.envelope_pairs(sq, pr, hi=HI, lo=LO, scaled=scaled)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base)), (cap, scaled)
            sc.test_set_posterior_budget(700 * 80)
            sc.test_set_forward_waves(1)
            got = sc.envelope_pairs(sq, pr, hi=HI, lo=LO, min_len=3, scaled=scaled)
            against_rows(dcp, got, res, HI, LO, 3, what=("rounds of one wavefront", scaled))
            sc.test_set_posterior_budget(0)
            sc.test_set_forward_waves(0)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_redo_pairs_have_the_log_space_rows_envelopes(dcp, oracle64, precision):
    from test_forward_scaled import shuffled
    from test_posterior_scaled_gpu import redo_world
    mine, qs, bad = redo_world(dcp, oracle64, precision)
    sc = dcp.Scanner(0)
    sc.upload_db(mine)
    sc.upload_seqs(qs)
    sq, pp = shuffled(len(qs), len(mine), 5)
    res_s = sc.posterior_pairs_scaled(sq, pp)
    redone = sc.last_posterior_scaled_redo_pairs
    assert redone >= 4
    res = sc.posterior_pairs(sq, pp)
    for hi, lo in ((HI, LO), (1e-3, 1e-6)):
        got = sc.envelope_pairs(sq, pp, hi=hi, lo=lo)
        assert sc.last_posterior_scaled_redo_pairs == redone
        against_rows(dcp, got, res_s, hi, lo, what="scaled rows")
        # the flagged profiles' pairs: the envelopes of posterior_pairs' rows
        off, env = got[:2]
        rows = unpack(res)[0]
        n = 0
        for i in np.nonzero(np.isin(pp, bad) & np.array([same_bits(a, b) for a, b in zip(unpack(res_s)[0], rows)]))[0]:
            want = dcp.posterior_envelope_records(*rows[i], hi, lo)
            want["pair"] = i
            assert exact_fields(env[int(off[i]):int(off[i + 1])]) == exact_fields(want)
            n += 1
        assert n >= 4
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lists_refusals_and_capacity(dcp, oracle32, oracle64, precision):
    mine, qs, planted = env_world(dcp, precision, oracle32, oracle64)
    sc = dcp.Scanner(0)
    refused(dcp, sc, lambda: sc.envelope_pairs([0], [0]))  # no DB
    sc.upload_db(mine)
    refused(dcp, sc, lambda: sc.envelope_pairs([0], [0]))  # no batch
    sc.upload_seqs(qs)
    # empty, single, duplicates
    off, env, fwd, bwd = sc.envelope_pairs([], [])
    assert off.tolist() == [0] and off.dtype == np.uint64 and env.shape == fwd.shape == bwd.shape == (0,)
    assert sc.envelope_kernel_ms < 0
    q, p, g0, g1 = planted[3]
    got = sc.envelope_pairs([q], [p], hi=HI, lo=LO)
    against_rows(dcp, got, sc.posterior_pairs_scaled([q], [p]), what="single")
    assert len(got[1]) >= 1 and sc.envelope_kernel_ms > 0
    sq = np.array([q, planted[5][0], q, q, 3, planted[5][0]], np.uint32)
    pr = np.array([p, planted[5][1], p, p, 0, planted[5][1]], np.uint32)
    off, env, fwd, bwd = got = sc.envelope_pairs(sq, pr, hi=HI, lo=LO)
    against_rows(dcp, got, sc.posterior_pairs_scaled(sq, pr), what="duplicates")
    per = [env[int(off[i]):int(off[i + 1])] for i in range(len(sq))]
    assert [r["pair"].tolist() for r in per] == [[i] * len(r) for i, r in enumerate(per)]  # listed twice: reported twice
    for f in EXACT[1:] + SUM_FIELDS:
        assert per[0][f].tobytes() == per[2][f].tobytes() == per[3][f].tobytes() and per[1][f].tobytes() == per[5][f].tobytes()
    for bad_ in (lambda: sc.envelope_pairs([0, len(qs)], [0, 0]), lambda: sc.envelope_pairs([0, 1], [0, len(mine)]),
                 lambda: sc.envelope_pairs([0, 1], [0]), lambda: sc.envelope_pairs(sq, pr, hi=float("nan")),
                 lambda: sc.envelope_pairs(sq, pr, hi=HI, lo=float("nan")), lambda: sc.envelope_pairs(sq, pr, hi=LO, lo=HI)):
        refused(dcp, sc, bad_)

    # the raw call: capacity one short, each null pointer
    need = len(env)
    assert need >= 4
    out = np.zeros(need, dcp.ENVELOPE_DTYPE)
    out["pair"] = 77
    eo = np.full(len(sq) + 1, 7, np.uint64)
    f2, b2 = np.full(len(sq), 2.5), np.full(len(sq), 2.5)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    nan = float("nan")

    def run(sq_=sq, pr_=pr, n=len(sq), hi=HI, lo=LO, out_=out, cap=need, eo_=eo, f_=f2, b_=b2):
        return sc._lib.dcp_gpu_envelope_pairs(sc._c, 1, 0, 1, P(sq_), P(pr_), n, hi, lo, 1, P(out_), cap, P(eo_), P(f_), P(b_))

    def untouched(offsets=True):
        return (not offsets or (eo == 7).all()) and (out["pair"] == 77).all() and (f2 == 2.5).all() and (b2 == 2.5).all()

    for change in (dict(sq_=None), dict(pr_=None), dict(out_=None), dict(eo_=None), dict(f_=None), dict(b_=None), dict(hi=nan),
                   dict(lo=nan), dict(hi=LO, lo=HI), dict(sq_=np.array([q, 99, q, q, 3, q], np.uint32))):
        assert run(**change) == dcp.RC_EINVAL and untouched(), change
        assert len(sc._lib.dcp_gpu_last_error(sc._c)) > 0
    assert run(cap=need - 1) == dcp.RC_ENOMEM and untouched(offsets=False) and np.array_equal(eo, off)
    assert str(need) in sc._lib.dcp_gpu_last_error(sc._c).decode()
    eo[:] = 7
    assert run(out_=None, cap=0) == dcp.RC_ENOMEM and untouched(offsets=False) and np.array_equal(eo, off)  # counting needs no array
    eo[:] = 7
    assert run(n=0) == 0 and eo[0] == 0 and (eo[1:] == 7).all() and untouched(offsets=False)
    assert run() == 0 and np.array_equal(eo, off) and out.tobytes() == env.tobytes()
    assert np.array_equal(bits(f2), bits(fwd)) and np.array_equal(bits(b2), bits(bwd))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_other_batches_and_transitions(dcp, oracle32, oracle64, precision):
    mine, qs, planted = env_world(dcp, precision, oracle32, oracle64)
    n = len(qs)
    plq = [q for q, _, _, _ in planted]
    plp = [p for _, p, _, _ in planted]

    def check(sc, sq, pr, what, at_least=1):
        for scaled in (True, False):
            res = (sc.posterior_pairs_scaled if scaled else sc.posterior_pairs)(sq, pr)
            got = sc.envelope_pairs(sq, pr, hi=HI, lo=LO, scaled=scaled)
            against_rows(dcp, got, res, what=(what, scaled))
            assert len(got[1]) >= at_least, what

    # an epsilon = 0 profile: no path where the length is no multiple of three, rows of 0
    eps0 = dcp.ProteinProfile.sample(77, 70, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.0), "EPS0", precision=precision)
    sc = dcp.Scanner(0)
    sc.upload_db([mine[3], eps0, mine[plp[0]], mine[plp[3]]])
    sc.upload_seqs(qs)
    sq, pr = np.arange(n).repeat(4), np.tile(np.arange(4), n)
    check(sc, sq, pr, "eps 0", 2)
    off, env, fwd, bwd = sc.envelope_pairs(sq, pr, hi=HI, lo=LO)
    for q, s in enumerate(qs):
        if len(s) % 3:
            assert fwd[4 * q + 1] == NEG_INF and off[4 * q + 1] == off[4 * q + 2]
    off0 = sc.envelope_pairs(sq, pr, hi=0.0, lo=0.0)[0]  # lo <= 0: rows of 0 are one run over the sequence
    assert all(off0[4 * q + 2] - off0[4 * q + 1] == 1 for q, s in enumerate(qs) if len(s) % 3)
    sc.close()

    # both strands: resident n + q is the reverse complement of q
    sc = loaded(dcp, precision)
    sc.add_reverse_strand()
    check(sc, np.array(plq + [n + q for q in plq] + [n + 8, 8]), np.array(plp + plp + [9, 9]), "strands", len(planted))
    sc.close()
    # windows
    sc = loaded(dcp, precision)
    sc.cut_windows(100, 50)
    nw = sc.nseqs
    check(sc, np.arange(nw).repeat(2), np.tile(np.array(plp[2:4]), nw), "windows")
    sc.close()
    # regions cut out of the batch
    sc = loaded(dcp, precision)
    sc.cut_regions([plq[5], plq[5], plq[3], 8], [0, 20, 10, 100], [200, 150, 100, 150], [0, 1, 0, 1])
    check(sc, np.array([0, 1, 2, 3, 1]), np.array([plp[5], plp[5], plp[3], 6, 0]), "regions")
    sc.close()
    # explicit transitions
    sc = loaded(dcp, precision)
    xt = np.stack([xtrans_of(dcp, precision, len(s) + 50, False, False) for s in qs])
    (sc.set_xtrans64 if precision == 64 else sc.set_xtrans)(xt)
    check(sc, np.array(plq + [8, 7]), np.array(plp + [12, 9]), "explicit transitions", len(planted))
    other = np.stack([xtrans_of(dcp, 96 - precision, len(s), True, False) for s in qs])
    (sc.set_xtrans if precision == 64 else sc.set_xtrans64)(other)
    refused(dcp, sc, lambda: sc.envelope_pairs(plq, plp))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nothing_else_moves(dcp, oracle32, oracle64, precision):
    mine, qs, planted = env_world(dcp, precision, oracle32, oracle64)
    sc = loaded(dcp, precision)
    sc.scan(True, False, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    sq, pr = every_pair(mine, qs, 28)
    sq, pr = sq[:40], pr[:40]

    def state():
        nl, al = sc.scores()
        mea = sc.mea_pairs(sq[:6], pr[:6])
        return dict(scores=(bits(nl).copy(), bits(al).copy()), hits=sc.hits().tobytes(), cells=sc.cells,
                    launches=sc.last_scan_launches, dense=tuple(bits(a).copy() for a in sc.forward_scores()),
                    fwd=tuple(bits(a) for a in sc.forward_pairs(sq, pr, False, False)),
                    post=tuple(a.tobytes() for a in sc.posterior_pairs(sq, pr, False, False)),
                    post_s=tuple(a.tobytes() for a in sc.posterior_pairs_scaled(sq, pr, False, False)),
                    mea=(b"".join(p.tobytes() for p in mea[0]), b"".join(p.tobytes() for p in mea[1]), mea[2].tobytes(),
                         mea[3].tobytes()))

    sc.forward_dense(True, False)
    before = state()
    for scaled in (True, False):
        got = sc.envelope_pairs(sq, pr, True, True, HI, LO, scaled=scaled)  # other flags than the scan's
        assert len(got[0]) == len(sq) + 1
    after = state()
    for k in before:
        a, b = before[k], after[k]
        same = all(x == y if isinstance(x, bytes) else np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else a == b
        assert same, k
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_envelopes_into_the_rescoring_chain(dcp, oracle32, oracle64, precision):
    """the planted world of tests/test_scan_pairs.py: the 333-nt query carries the 64-node profile's gene in bases
    [70, 262), the 1 000-nt one the 300-node profile's from base 50 on"""
    from test_scan_pairs import PAIR_M, pair_world
    profs, seqs = pair_world(dcp, oracle64 if precision == 64 else oracle32, precision)[:2]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sq, pr = np.array([5, 6, 5, 2]), np.array([1, 5, 0, 1])
    off, env, fwd, bwd = sc.envelope_pairs(sq, pr, hi=HI, lo=LO)
    lens = np.array([len(s) for s in seqs])
    for i, (g0, g1) in enumerate(((70, 70 + 3 * PAIR_M[1]), (50, 50 + 3 * PAIR_M[5]))):
        mine = env[int(off[i]):int(off[i + 1])]
        assert len(mine) >= 1 and sum(max(0, min(int(r["end"]), g1) - max(int(r["begin"]), g0)) for r in mine) > 0, (i, mine)
        print("planted gene [%d, %d) f%d: envelopes %s, expected domains %s" % (
            g0, g1, precision, [(int(r["begin"]), int(r["end"])) for r in mine], [float(r["begin_sum"]) for r in mine]))
    assert len(env) >= 2
    flank = 12
    src, begin, length, pair = dcp.envelopes_regions(env, sq, lens, flank)
    assert src.tolist() == sq[env["pair"]].tolist() and pair.tolist() == env["pair"].tolist()
    assert begin.tolist() == np.maximum(env["begin"].astype(np.int64) - flank, 0).tolist()
    assert (begin + length).tolist() == np.minimum(env["end"].astype(np.int64) + flank, lens[src]).tolist()
    sc.cut_regions(src, begin, length, np.zeros(len(env), np.uint8))
    assert sc.regions == len(env)
    msrc, mbegin, mminus = sc.region_map()  # the envelope's source and first base
    assert msrc.tolist() == src.tolist() and mbegin.tolist() == begin.tolist() and not mminus.any()
    prof_of = pr[pair]
    null, alt = sc.forward_pairs_scaled(np.arange(len(env)), prof_of, multi_hits=False)
    assert np.isfinite(null).all() and np.isfinite(alt).all()
    assert ((alt - null)[:int(off[2])] > 0).any()  # a planted gene's envelope scores above the null model
    sc.close()
    # the same substrings cut on the host and uploaded: the same bits
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs([seqs[s][b:b + n] for s, b, n in zip(src.tolist(), begin.tolist(), length.tolist())])
    null2, alt2 = sc.forward_pairs_scaled(np.arange(len(env)), prof_of, multi_hits=False)
    sc.close()
    assert np.array_equal(bits(null), bits(null2)) and np.array_equal(bits(alt), bits(alt2))
