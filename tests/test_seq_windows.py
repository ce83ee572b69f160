"""Windows: the rule on the host (dcp_seq_window_count / _start / _plan), and window_words_kernel (csrc/dcp_seqs.hip)
behind dcp_gpu_seqs_cut_windows / Scanner.cut_windows on the device.

CPU: the rule against a plain Python restatement, its coverage properties, its refusals, the plan's overflow.
GPU:
  1. the words of every window, bit for bit, against the host packing of the numpy slice (pad words and the bits
     behind the last base included), all-T sequences and their neighbours among them;
  2. a batch cut on the device scans to the bits of the same windows uploaded as sequences, on every kernel and flag set,
     also with the reverse strand added behind the cut;
  3. a planted gene is found in every window that wholly contains it, with the bits, path and product row of the slice
     uploaded alone, on either strand;
  4. the contract's refusals, explicit transitions and ranged scans over windows, the return to uncut."""
import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, hit_fields, host_words, kernels_of, np_revcomp, oracle_lrt, refused, world
from test_gpu_parity import pfam_like_params, planted_query

EDGE_L = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 100, 1000, 10007)
PRECISIONS = (32, 64)


def edge_windows(L):
    return sorted({w for w in (1, 5, 15, 16, 17, 32, 33, 48, 100, L - 1, L, L + 1) if w >= 1})


def edge_steps(window):
    return sorted({s for s in (1, 15, 16, 17, window - 1, window) if 1 <= s <= window})


def py_count(L, window, step):
    return 1 if L <= window else 1 + -(-(L - window) // step)


def py_starts(L, window, step):
    return [0] if L <= window else [min(i * step, L - window) for i in range(py_count(L, window, step))]


def py_map(lens, window, step):
    src, off = [], []
    for q, L in enumerate(lens):
        st = py_starts(int(L), window, step)
        src += [q] * len(st)
        off += st
    return np.array(src, np.uint32), np.array(off, np.uint32)


# ---- CPU ---------------------------------------------------------------------------------------------------------


def test_rule_equals_the_restatement_and_covers_every_base(dcp):
    for L in EDGE_L:
        for window in edge_windows(L):
            for step in edge_steps(window):
                where = (L, window, step)
                want = py_starts(L, window, step)
                assert dcp.window_count(L, window, step) == len(want) == py_count(L, window, step), where
                got = dcp.window_starts(L, window, step)
                assert got.dtype == np.uint32 and got.tolist() == want, where
                wl = min(L, window)
                assert got[0] == 0 and int(got[-1]) + wl == L, where  # the last window ends at L
                d = np.diff(got.astype(np.int64))
                # consecutive starts rise by at most step <= window: with the two ends above no base is left out
                assert (d >= 1).all() and (d <= step).all(), where
                # one past the last index stays anchored
                assert dcp.lib.dcp_seq_window_start(L, window, step, len(want)) == want[-1], where


def test_plan_equals_the_restatement(dcp):
    lens = np.array(EDGE_L, np.uint32)
    for window in (1, 5, 15, 16, 17, 32, 33, 48, 100, 999, 1000, 1001, 10006, 10007, 10008):
        for step in edge_steps(window):
            cnt = [py_count(int(L), window, step) for L in lens]
            words = sum(c * (min(int(L), window) // 16 + 3) for c, L in zip(cnt, lens))
            assert dcp.window_plan(lens, window, step) == (sum(cnt), words), (window, step)
    assert dcp.window_plan(np.zeros(0, np.uint32), 5, 5) == (0, 0)


def test_bad_rules_are_refused(dcp):
    lens = np.array([10, 20], np.uint32)
    for window, step in ((0, 0), (0, 1), (5, 0), (5, 6), (1, 2)):
        assert dcp.lib.dcp_seq_window_count(100, window, step) == 0
        assert dcp.lib.dcp_seq_window_start(100, window, step, 1) == 0
        for call in (lambda: dcp.window_starts(100, window, step), lambda: dcp.window_count(100, window, step),
                     lambda: dcp.window_plan(lens, window, step)):
            with pytest.raises(dcp.DcpError) as e:
                call()
            assert e.value.rc == dcp.RC_EINVAL


def test_plan_refuses_what_passes_32_bits(dcp):
    import ctypes as C
    big = np.full(70000, 1 << 20, np.uint32)
    nwin, nwords = C.c_uint64(0), C.c_uint64(0)
    # 70 000 x 2^20 windows of one base: the count itself passes 2^32 - 1; the totals still come back in 64 bits
    rc = dcp.lib.dcp_seq_window_plan(big.ctypes.data, len(big), 1, 1, C.byref(nwin), C.byref(nwords))
    assert rc == dcp.RC_EINVAL and nwin.value == 70000 << 20 and nwords.value == 3 * (70000 << 20)
    with pytest.raises(dcp.DcpError):
        dcp.window_plan(big, 1, 1)
    # 1 500 x 2^20: the windows fit, their words (3 each) do not
    rc = dcp.lib.dcp_seq_window_plan(big.ctypes.data, 1500, 1, 1, C.byref(nwin), C.byref(nwords))
    assert rc == dcp.RC_EINVAL and nwin.value == 1500 << 20 < 2 ** 32 <= nwords.value == 3 * (1500 << 20)
    # 1 365 x 2^20: both fit (3 x 1365 x 2^20 = 2^32 - 2^20)
    assert dcp.window_plan(big[:1365], 1, 1) == (1365 << 20, 3 * (1365 << 20))
    # sequences left uncut (window >= L) cost what they cost resident: 60 000 of them fit, 70 000 do not
    assert dcp.window_plan(big[:60000], 1 << 20, 1) == (60000, 60000 * ((1 << 16) + 3))
    with pytest.raises(dcp.DcpError):
        dcp.window_plan(big, 1 << 20, 1)
    # lengths of 2^32 - 1: the count is 64-bit arithmetic
    top = np.full(3, 2 ** 32 - 1, np.uint32)
    assert dcp.window_count(2 ** 32 - 1, 1, 1) == 2 ** 32 - 1
    assert dcp.window_starts(2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 2).tolist() == [0, 1]
    with pytest.raises(dcp.DcpError):
        dcp.window_plan(top, 1, 1)


# ---- GPU: words --------------------------------------------------------------------------------------------------

_WORD_SEQS = []


def word_seqs():
    """The edge lengths, every all-T sequence between two random ones in the word array, and the other way round."""
    if not _WORD_SEQS:
        rng = np.random.default_rng(1414)
        for L in EDGE_L:
            _WORD_SEQS.append(rng.integers(0, 4, L, dtype=np.uint8))
            if L in (1, 16, 17, 33, 49, 100, 1000):
                _WORD_SEQS.append(np.full(L, 3, np.uint8))
        _WORD_SEQS.append(rng.integers(0, 4, 50, dtype=np.uint8))
    return _WORD_SEQS


def check_words(sc, seqs, window, step):
    src, off = sc.window_map()
    wsrc, woff = py_map([len(s) for s in seqs], window, step)
    assert np.array_equal(src, wsrc) and np.array_equal(off, woff), (window, step)
    assert sc.nseqs == len(src) and sc.windows == (window, step) and sc.strands == 1
    for i in range(len(src)):
        s = seqs[src[i]]
        want = host_words(s[off[i]:off[i] + window])
        got = sc.test_seq_words(i)
        assert np.array_equal(got, want), (window, step, i, int(src[i]), int(off[i]), [hex(x) for x in got], [hex(x) for x in want])
    return src, off


WORD_WINDOWS = (1, 5, 15, 16, 17, 32, 33, 48, 49, 50, 100, 999, 1000, 1001)  # the fixed ones, and L - 1, L, L + 1 of 16, 49, 1000


@pytest.mark.gpu
@pytest.mark.parametrize("window", WORD_WINDOWS)
def test_words_of_every_window(dcp, window):
    """One batch, one cut per step: every resident window's raw words against the host packing of its slice.  (A
    sequence joins a cut only where it gives at most 1 200 windows -- each is fetched on its own -- so the 10 007-nt one
    is cut by steps of 15 and more.)"""
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    for step in edge_steps(window):
        seqs = [s for s in word_seqs() if py_count(len(s), window, step) <= 1200]
        assert len(seqs) >= len(word_seqs()) - 1
        sc.upload_seqs(seqs)
        assert sc.windows is None
        sc.cut_windows(window, step)
        check_words(sc, seqs, window, step)
    sc.close()


@pytest.mark.gpu
def test_phases_anchors_and_a_long_sequence(dcp):
    """What the cases above must contain, stated: starts at phases 0, 1 and 15 of a word, an anchored last window at an
    odd phase, an all-T source and the neighbours of one; then one 2^16-nt sequence cut 1 000 / 999 between two all-T
    ones, and fetch_seq of every window."""
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    seqs = word_seqs()
    sc.upload_seqs(seqs)
    sc.cut_windows(33, 17)
    src, off = check_words(sc, seqs, 33, 17)
    assert {0, 1, 15} <= {int(o) & 15 for o in off}
    lens = np.array([len(s) for s in seqs])
    last = np.r_[src[1:] != src[:-1], True] & (lens[src] > 33)
    assert (off[last] == lens[src[last]] - 33).all() and any(int(o) & 1 for o in off[last])  # L = 100: 67
    allt = [q for q, s in enumerate(seqs) if (s == 3).all() and len(s) > 33]
    assert allt and all(not (seqs[q - 1] == 3).all() and not (seqs[q + 1] == 3).all() for q in allt)
    for i in range(len(src)):
        assert np.array_equal(sc.fetch_seq(i), seqs[src[i]][off[i]:off[i] + 33]), i
    rng = np.random.default_rng(65536)
    long = [np.full(40, 3, np.uint8), rng.integers(0, 4, 1 << 16, dtype=np.uint8), np.full(1001, 3, np.uint8)]
    sc.upload_seqs(long)
    sc.cut_windows(1000, 999)
    src, off = check_words(sc, long, 1000, 999)
    assert len(src) == 1 + 66 + 2 and off[66] == 65536 - 1000 and off[65] == 64 * 999
    for i in (0, 1, 2, 65, 66, 67, 68):
        assert np.array_equal(sc.fetch_seq(i), long[src[i]][off[i]:off[i] + 1000]), i
    sc.close()


@pytest.mark.gpu
def test_a_batch_of_short_sequences_keeps_its_words(dcp):
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    seqs = [s for s in word_seqs() if len(s) <= 1000]
    sc.upload_seqs(seqs)
    before = [sc.test_seq_words(q) for q in range(len(seqs))]
    for window, step in ((1000, 1), (1000, 1000), (4096, 17)):
        sc.upload_seqs(seqs)
        sc.cut_windows(window, step)
        assert sc.nseqs == len(seqs) and sc.windows == (window, step)
        src, off = sc.window_map()
        assert src.tolist() == list(range(len(seqs))) and not off.any()
        for q in range(len(seqs)):
            assert np.array_equal(sc.test_seq_words(q), before[q]), q
    sc.close()


# ---- GPU: the bits of a batch cut by hand ------------------------------------------------------------------------

SAME_BITS_CASES = [(32, 1), (32, 2), (32, 3), (64, 1), (64, 4)]  # (precision, dcp_scan_params.kernel)
CUT = (100, 64)  # the strands tests' world under it: 1 .. 100-nt windows, 156 of the 10 007-nt query


def hand_cut(seqs, window, step):
    return [s[o:o + window] for s in seqs for o in py_starts(len(s), window, step)]


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("multi_hits", [False, True])
@pytest.mark.parametrize("precision,kernel", SAME_BITS_CASES)
def test_same_bits_as_a_hand_cut_batch(dcp, precision, kernel, multi_hits, both):
    """Scan A: n queries + cut_windows (+ add_reverse_strand).  Scan B: the windows (and their reverse complements)
    through upload_seqs."""
    profs, seqs = world(dcp, precision)
    cut = hand_cut(seqs, *CUT)
    a, b = dcp.Scanner(0), dcp.Scanner(0)
    a.upload_db(profs)
    b.upload_db(profs)
    a.upload_seqs(seqs)
    a.cut_windows(*CUT)
    if both:
        a.add_reverse_strand()
        cut = cut + [np_revcomp(s) for s in cut]
    b.upload_seqs(cut)
    assert a.nseqs == b.nseqs == len(cut) and a.strands == (2 if both else 1)
    assert a.cells == b.cells and a.algorithmic_bytes == b.algorithmic_bytes
    for h3 in (False, True):
        for thr in (10.0, 0.0):
            a.scan(multi_hits, h3, thr, kernel=kernel)
            b.scan(multi_hits, h3, thr, kernel=kernel)
            where = (precision, kernel, multi_hits, h3, thr, both)
            for x, y in zip(a.scores(), b.scores()):
                assert np.array_equal(bits(x), bits(y)), where
            assert hit_fields(a.hits()) == hit_fields(b.hits()), where
            assert a.last_scan_redo_pairs == b.last_scan_redo_pairs, where
            assert a.last_scan_kernel == b.last_scan_kernel == kernel, where
            if kernel == dcp.KERNEL_QLANE64:
                assert a.last_scan_query_plan == b.last_scan_query_plan, where
    a.close()
    b.close()


# ---- GPU: a planted gene -----------------------------------------------------------------------------------------

PLANT_SEED = {32: 5100, 64: 5200}  # the premise holds for every containing window of either precision (checked on the CPU)
PLANT_M = (40, 130, 300)
PLANT_AT = (1100, 2500, 4000)  # profile 2's copy is planted on the minus strand
PLANT_L, PLANT_WINDOW, PLANT_STEP = 6000, 2048, 1024

_PLANTED = {}


def planted_world(dcp, oracle, precision):
    """Pfam-like profiles, their oracle twins, and one 6 000-nt sequence with a copy of each: profiles 0 and 1 forward,
    profile 2 as its reverse complement.  Also (profile, window, strand) of every window that wholly contains a copy."""
    if precision not in _PLANTED:
        rng = np.random.default_rng(PLANT_SEED[precision])
        params = [pfam_like_params(rng, M) for M in PLANT_M]
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
        profs = [dcp.ProteinProfile.from_params(*prm, cfg, f"PLANT{i}", precision=precision) for i, prm in enumerate(params)]
        oprofs = [oracle.new(*prm, ENTRY_DIST_OCCUPANCY, 0.01) for prm in params]
        seq = rng.integers(0, 4, PLANT_L, dtype=np.uint8)
        inside = []
        starts = py_starts(PLANT_L, PLANT_WINDOW, PLANT_STEP)
        for p, (M, at) in enumerate(zip(PLANT_M, PLANT_AT)):
            gene = planted_query(rng, oprofs[p], M, flank=12)
            minus = p == 2
            seq[at:at + len(gene)] = np_revcomp(gene) if minus else gene
            inside += [(p, i, minus) for i, o in enumerate(starts) if o <= at and at + len(gene) <= o + PLANT_WINDOW]
        _PLANTED[precision] = (profs, oprofs, seq, inside)
    return _PLANTED[precision]


def test_the_planted_world_has_what_the_test_needs(dcp, oracle32):
    _, _, seq, inside = planted_world(dcp, oracle32, 32)
    assert py_starts(PLANT_L, PLANT_WINDOW, PLANT_STEP) == [0, 1024, 2048, 3072, 3952]  # the last one anchored
    assert sorted(inside) == [(0, 0, False), (0, 1, False), (1, 1, False), (1, 2, False), (2, 3, True), (2, 4, True)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_premise_every_containing_window_hits_on_the_oracle(dcp, oracle32, oracle64, precision):
    """CPU: every window that wholly contains a planted copy hits that profile (on the strand the copy is on, and not
    on the other one), for the seeds kept above."""
    oracle = oracle64 if precision == 64 else oracle32
    _, oprofs, seq, inside = planted_world(dcp, oracle, precision)
    cut = hand_cut([seq], PLANT_WINDOW, PLANT_STEP)
    fwd = oracle_lrt(oracle, oprofs, cut)
    rev = oracle_lrt(oracle, oprofs, [np_revcomp(s) for s in cut])
    for p, i, minus in inside:
        hit, other = (rev, fwd) if minus else (fwd, rev)
        assert hit[i, p] >= 10.0, (p, i, hit[i, p])
        assert not other[i, p] >= 10.0, (p, i, other[i, p])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_planted_gene_is_found_in_every_window_that_contains_it(dcp, oracle32, oracle64, precision):
    oracle = oracle64 if precision == 64 else oracle32
    profs, _, seq, inside = planted_world(dcp, oracle, precision)
    cut = hand_cut([seq], PLANT_WINDOW, PLANT_STEP)
    W = len(cut)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    # every slice (and its reverse complement) uploaded alone: the bits, paths and rows the windows must reproduce
    want = {}
    for p, i, minus in inside:
        alone = np_revcomp(cut[i]) if minus else cut[i]
        sc.upload_seqs([alone])
        sc.scan(True, False, 10.0)
        own = [h.copy() for h in sc.hits() if h["profile_idx"] == p]
        assert len(own) == 1  # the premise on the device
        paths, _ = sc.trace_paths(np.array(own), True, False)
        row = profs[p].prod_row(alone, paths[0], 3, 77, own[0]["alt_loglik"], own[0]["null_loglik"])
        want[(p, i, minus)] = (own[0], paths[0], row)
    sc.upload_seqs([seq])
    sc.cut_windows(PLANT_WINDOW, PLANT_STEP)
    assert sc.nseqs == W
    sc.scan(True, False, 10.0)
    plus = {(int(h["seq_idx"]), int(h["profile_idx"])) for h in sc.hits()}
    assert {(i, p) for p, i, minus in inside if not minus} <= plus
    assert not any((i, p) in plus for p, i, minus in inside if minus)  # the minus-strand copy is invisible so far
    sc.add_reverse_strand()
    assert sc.nseqs == 2 * W and sc.window_map()[1].tolist() == py_starts(PLANT_L, PLANT_WINDOW, PLANT_STEP)
    for kernel in kernels_of(dcp, precision):
        sc.scan(True, False, 10.0, kernel=kernel)
        got = {(int(h["seq_idx"]), int(h["profile_idx"])): h.copy() for h in sc.hits()}
        assert {k for k in got if k[0] < W} == plus
        for (p, i, minus), (own, _, _) in want.items():
            h = got[(W + i if minus else i, p)]
            assert bits(h["null_loglik"]) == bits(own["null_loglik"]), (kernel, p, i)
            assert bits(h["alt_loglik"]) == bits(own["alt_loglik"]), (kernel, p, i)
    keys = sorted(want)
    hits = np.array([got[(W + i if minus else i, p)] for p, i, minus in keys])
    paths, alt = sc.trace_paths(hits, True, False)
    for k, key in enumerate(keys):
        own, want_path, want_row = want[key]
        p, i, minus = key
        assert np.array_equal(paths[k], want_path), key
        assert bits(alt[k]) == bits(own["alt_loglik"]), key
        bases = sc.fetch_seq(int(hits[k]["seq_idx"]))
        assert np.array_equal(bases, np_revcomp(cut[i]) if minus else cut[i]), key
        assert profs[p].prod_row(bases, paths[k], 3, 77, hits[k]["alt_loglik"], hits[k]["null_loglik"]) == want_row, key
    sc.close()


# ---- GPU: contract -----------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_contract(dcp, precision):
    profs, seqs = world(dcp, precision)
    seqs = seqs[:12] + [seqs[18]]  # 1 .. 47 nt, and the 1 000-nt query
    n = len(seqs)
    window, step = 48, 31
    cut = hand_cut(seqs, window, step)
    W = len(cut)
    assert W > n
    sc = dcp.Scanner(0)

    def state():
        return sc.nseqs, sc.strands, sc.windows

    def message(call, *words):
        with pytest.raises(dcp.DcpError) as e:
            call()
        assert e.value.rc == dcp.RC_EINVAL and all(w in str(e.value) for w in words), str(e.value)

    # no batch resident (and no DB)
    message(lambda: sc.cut_windows(window, step), "no sequences resident")
    assert state() == (0, 0, None)
    refused(dcp, sc, sc.window_map)
    sc.upload_seqs(seqs)
    sc.cut_windows(window, step)  # no DB resident: sequences only
    assert state() == (W, 1, (window, step))
    sc.upload_db(profs)
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    want = [bits(x).copy() for x in sc.scores()]

    def same_scan(k=None):
        sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
        for x, y in zip(sc.scores(), want):
            assert np.array_equal(bits(x)[:k], y[:k])

    # the batch already cut
    message(lambda: sc.cut_windows(window, step), "already cut")
    assert state() == (W, 1, (window, step))
    same_scan()
    # a bad rule, on a cut batch and on an uncut one
    sc.upload_seqs(cut)
    assert state() == (W, 1, None)  # the next upload clears the state
    refused(dcp, sc, sc.window_map)
    for bad in ((0, 0), (0, 1), (5, 0), (5, 6)):
        message(lambda: sc.cut_windows(*bad), "window")
        assert state() == (W, 1, None)
    same_scan()
    # both strands already resident
    sc.upload_seqs(cut[:W // 2])
    sc.add_reverse_strand()
    message(lambda: sc.cut_windows(window, step), "both strands", "first")
    assert state() == (2 * (W // 2), 2, None)
    same_scan(W // 2)
    # explicit transitions in force, in the precision of the DB
    derived = (dcp.xtrans64 if precision == 64 else dcp.xtrans)
    rows = lambda ss: np.stack([derived(len(s), True, False) for s in ss])
    sc.upload_seqs(cut)
    sc.set_xtrans(rows(cut))
    message(lambda: sc.cut_windows(window, step), "explicit special transitions")
    assert state() == (W, 1, None)
    sc.scan(False, True, 10.0, kernel=dcp.KERNEL_ROWSWEEP)  # the flags are ignored: the explicit rows still hold
    for x, y in zip(sc.scores(), want):
        assert np.array_equal(bits(x), y)
    # set_xtrans after the cut takes W rows
    sc.upload_seqs(seqs)
    sc.cut_windows(window, step)
    refused(dcp, sc, lambda: sc.set_xtrans(rows(seqs)))
    sc.set_xtrans(rows(cut))
    sc.scan(False, True, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    for x, y in zip(sc.scores(), want):
        assert np.array_equal(bits(x), y)
    # a ranged scan over windows
    sc.upload_seqs(seqs)
    sc.cut_windows(window, step)
    keep_all = -1e30
    sc.scan(True, False, keep_all)
    fn, fa = sc.scores()
    fh = sc.hits()
    for kernel in kernels_of(dcp, precision):
        for q0, q1 in ((n - 2, W), (3, n + 5)):
            sc.scan(True, False, keep_all, q_range=(q0, q1), kernel=kernel)
            gn, ga = sc.scores()
            assert np.array_equal(bits(gn[q0:q1]), bits(fn[q0:q1])) and np.array_equal(bits(ga[q0:q1]), bits(fa[q0:q1]))
            sel = fh[(fh["seq_idx"] >= q0) & (fh["seq_idx"] < q1)]
            assert len(sel) > 0 and hit_fields(sc.hits()) == hit_fields(sel), (kernel, q0, q1)
    # the supported order: cut, then the reverse strand; the next upload returns the context to uncut
    sc.add_reverse_strand()
    assert state() == (2 * W, 2, (window, step)) and len(sc.window_map()[0]) == W
    short = np.zeros(W, np.uint32)
    assert sc._lib.dcp_gpu_seqs_window_map(sc._c, short.ctypes.data, short.ctypes.data, W - 1) == dcp.RC_ENOMEM and not short.any()
    message(lambda: sc.cut_windows(window, step), "both strands")
    sc.upload_seqs(seqs)
    assert state() == (n, 1, None)
    sc.cut_windows(window, step)
    same_scan()
    sc.close()
