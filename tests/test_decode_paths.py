"""The decode of hit paths on the device (dcp_gpu_decode_paths) and its host companions
dcp_profile_codon_joint / dcp_prod_format_row_codes.

The agreement rule of every GPU comparison -- device code d against the host's dcp_profile_decode codon h:
  * I, N, J, C, R steps: d == h, always (the device multiplies the host's own exp() values);
  * M steps: d == h, or codon_joint(d) >= codon_joint(h) * (1 - 2^-40), both evaluated on the host.  The two exp()
    implementations differ by a few units in the last place, every term of the formula is a product of at most three
    such values and the sums have only non-negative terms: a joint moves by about 2^-48, 2^-40 leaves 256x and is
    far below any gap that is not a tie;
  * M steps with d != h are counted and printed and may be at most 1 in 1 000 of a test's M steps.

Near-ties of the tests' own inputs, counted on the CPU before any GPU run with codon_joint over all 64 codons
(`python tests/test_decode_paths.py` prints them): M steps whose runner-up lies within 2^-40 of the best --
  every word, every state kind   float profiles: 0 of 20 460 M steps    double profiles: 0 of 20 460
  real paths (oracle's paths)    float profiles: 0 of 388 M steps       double profiles: 0 of 388
so with these seeds the rule's second branch has nothing to hide: every M step is expected to agree exactly."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY

gpu = pytest.mark.gpu
R, S, N, B, E, J, CC, T = [(3 << 14) | i for i in range(8)]
MUTE = 0xFF
TIE = 1.0 - 2.0 ** -40


def I_(k):
    return (1 << 14) | k


def D_(k):
    return (2 << 14) | k


# ---- inputs --------------------------------------------------------------------------------------------------------
WORD_SIZES = [65, 1, 513, 2, 64]  # core sizes 1, 2, 64, 65, 513, uploaded unsorted: the dist-row map is not the identity
WORD_SEEDS = [11, 12, 24, 21, 21]  # chosen for no near-tie M step (see above): synonymous codons tie exactly under other seeds


def all_words():
    """The 1 364 words of length 1..5 in code order (first base most significant)."""
    out = []
    for ln in range(1, 6):
        for v in range(4 ** ln):
            out.append(np.array([(v >> (2 * (ln - 1 - i))) & 3 for i in range(ln)], np.uint8))
    return out


def word_states(M):
    """M1, a middle node, M_last, I2 (I1 of a one-node profile), N, J, C, R."""
    return [1, (M + 1) // 2, M, I_(min(2, M)), N, J, CC, R]


def word_profiles(dcp, precision):
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)

    def one(seed, M):
        if M >= 2:
            return dcp.ProteinProfile.sample(seed, M, cfg, "W%d" % M, precision=precision)
        # protein_profile_sample asserts core_size >= 2: the one-node profile from random parameters of its own
        rng = np.random.default_rng(seed)
        norm = lambda x: x - np.logaddexp.reduce(x, axis=-1, keepdims=True)  # noqa: E731
        trans = np.log(rng.random((M + 1, 7)) + 0.05)
        trans[0, 6] = trans[M, 2] = trans[M, 6] = -np.inf
        trans[:, 0:3], trans[:, 3:5] = norm(trans[:, 0:3]), norm(trans[:, 3:5])
        return dcp.ProteinProfile.from_params(norm(np.log(rng.random(20) + 0.05)), norm(np.log(rng.random((M, 20)) + 0.05)),
                                              trans, cfg, "W%d" % M, precision=precision)

    return [one(s, m) for s, m in zip(WORD_SEEDS, WORD_SIZES)]


def word_paths(dcp):
    """One 6 372-nt sequence = all words back to back, and per (profile, state) one 1 364-step path tiling it."""
    words = all_words()
    seq = np.concatenate(words)
    lens = np.array([len(w) for w in words], np.uint8)
    hits, paths = [], []
    for p, M in enumerate(WORD_SIZES):
        for sid in word_states(M):
            st = np.zeros(len(words), dcp.STEP_DTYPE)
            st["state_id"], st["seqlen"] = sid, lens
            hits.append((0, p))
            paths.append(st)
    return seq, np.array(hits, [("seq_idx", np.uint32), ("profile_idx", np.uint32)]), paths


def host_codes(prof, seq, path):
    """dcp_profile_decode of every step: 16a + 4b + c, MUTE for a step that emits nothing."""
    out = np.full(len(path), MUTE, np.uint8)
    pos = 0
    for i, (sid, ln) in enumerate(zip(path["state_id"].tolist(), path["seqlen"].tolist())):
        if ln:
            c = prof.decode(seq[pos:pos + ln], sid)
            out[i] = 16 * "ACGT".index(c[0]) + 4 * "ACGT".index(c[1]) + "ACGT".index(c[2])
        pos += ln
    return out


def check_rule(prof, seq, path, dev, host):
    """The agreement rule; returns (M steps, M steps with d != h)."""
    sid, ln = path["state_id"].astype(np.int64), path["seqlen"].astype(np.int64)
    assert dev.shape == host.shape == sid.shape
    assert np.array_equal(dev[ln == 0], np.full(int((ln == 0).sum()), MUTE, np.uint8))
    assert np.all(dev[ln > 0] < 64)
    is_m = (ln > 0) & ((sid >> 14) == 0)
    start = np.cumsum(ln) - ln
    diff = np.nonzero(dev != host)[0]
    for i in diff:
        assert is_m[i], "step %d (state 0x%x): device %d, host %d -- only M steps may differ" % (i, sid[i], dev[i], host[i])
        frag = seq[start[i]:start[i] + ln[i]]
        jd, jh = prof.codon_joint(frag, int(sid[i]), int(dev[i])), prof.codon_joint(frag, int(sid[i]), int(host[i]))
        assert jd >= jh * TIE, "step %d: joint of the device's codon %r < the host's %r" % (i, jd, jh)
    return int(is_m.sum()), len(diff)


def near_ties(prof, seq, path):
    """(M steps, M steps whose runner-up joint lies within 2^-40 of the best): codon_joint over all 64 codons."""
    pos = n = close = 0
    for sid, ln in zip(path["state_id"].tolist(), path["seqlen"].tolist()):
        if ln and (sid >> 14) == 0:
            j = sorted(prof.codon_joint(seq[pos:pos + ln], sid, c) for c in range(64))
            n += 1
            close += j[-2] >= j[-1] * TIE
        pos += ln
    return n, close


# real paths: lengths {1, 5, 16, 17, 33, 300} and two sequences with planted two-domain hits
REAL_SIZES = [40, 64, 65, 130]


def real_params():
    import test_gpu_parity as tp

    rng = np.random.default_rng(2024)
    return [tp.pfam_like_params(rng, M) for M in REAL_SIZES]


def real_profiles(dcp, precision):
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)
    return [dcp.ProteinProfile.from_params(*prm, cfg, accession="R%d" % i, precision=precision)
            for i, prm in enumerate(real_params())]


def consensus_dna(prof):
    """The most likely codon of every match state, from the profile's own match dists."""
    md = np.asarray(prof.match_dist, np.float64).reshape(prof.core_size, 129)[:, 4:].reshape(-1, 5, 5, 5)[:, :4, :4, :4]
    best = md.reshape(prof.core_size, 64).argmax(axis=1)
    return np.stack([best >> 4, (best >> 2) & 3, best & 3], axis=1).astype(np.uint8).reshape(-1)


def real_seqs(dcp):
    rng = np.random.default_rng(77)
    profs = real_profiles(dcp, 32)
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in (1, 5, 16, 17, 33, 300)]
    for p in (1, 3):  # two domains of the same profile: J between them, N in front, C behind
        dom = consensus_dna(profs[p])
        seqs.append(np.concatenate([rng.integers(0, 4, 23, dtype=np.uint8), dom, rng.integers(0, 4, 31, dtype=np.uint8), dom,
                                    rng.integers(0, 4, 19, dtype=np.uint8)]))
    return seqs


# ---- CPU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [32, 64])
def test_codon_joint_argmax_is_decode(dcp, oracle64, precision):
    """All 1 364 words x states {M1, M_last, I, N, R} of one sampled profile per precision: the LAST maximiser of
    codon_joint over the 64 codons is dcp_profile_decode's codon (its `v >= best` loop); for the double profile
    log(joint) equals the oracle's log-domain codon_lprob to 1e-10 relative (measured maximum 5.2e-16)."""
    M = 7
    # the oracle takes the reference's float literal for epsilon in either build: the same double here
    prof = dcp.ProteinProfile.sample(5, M, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01))), precision=precision)
    op = oracle64.sample(5, M, ENTRY_DIST_OCCUPANCY, 0.01) if precision == 64 else None
    worst = 0.0
    codons = ["ACGT"[c >> 4] + "ACGT"[(c >> 2) & 3] + "ACGT"[c & 3] for c in range(64)]
    for w in all_words():
        for sid in (1, M, I_(2), N, R):
            j = np.array([prof.codon_joint(w, sid, c) for c in range(64)])
            last = 63 - int(np.argmax(j[::-1]))
            assert codons[last] == prof.decode(w, sid), (w, sid)
            if op is not None:
                for c in range(64):
                    want = op.codon_lprob(bytes(w), sid, codons[c])
                    if j[c] > 0.0:
                        worst = max(worst, abs(np.log(j[c]) - want) / abs(want))
                    else:
                        assert want == -np.inf
    print("max relative difference of log(joint) to the oracle: %.3g" % worst)
    assert worst <= 1e-10


def test_codon_joint_refuses_what_decode_refuses(dcp):
    prof = dcp.ProteinProfile.sample(5, 3, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01))
    for frag, sid, codon in (("ACG", S, "AAA"), ("ACG", D_(1), "AAA"), ("ACG", 4, "AAA"), ("ACGTAC", 1, "AAA"), ("", 1, "AAA")):
        with pytest.raises(dcp.DcpError):
            prof.codon_joint(frag, sid, codon)
    with pytest.raises(dcp.DcpError):
        prof.codon_joint(np.array([0, 1], np.uint8), 1, np.array([0, 4, 0], np.uint8))
    assert prof.codon_joint("ACG", 1, "ACG") == prof.codon_joint("ACG", 1, 0 * 16 + 1 * 4 + 2) > 0.0


def golden_rows(dcp, oracle64):
    """(profile, sequence ids, steps) of the committed goldens' inputs: the reference's own test sequence and profile
    (tests/golden/reference_protein_profile.json) and cases of tests/golden/oracle_scores.json, with the oracle's paths."""
    import json
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ref = json.load(open(os.path.join(here, "reference_protein_profile.json")))
    gold = json.load(open(os.path.join(here, "oracle_scores.json")))
    todo = [(ref["seed"], ref["core_size"], ENTRY_DIST_OCCUPANCY, ref["epsilon"], ref["multi_hits"], ref["hmmer3_compat"], ref["seq"])]
    for case in gold["cases"][::6]:
        for s in gold["seqs"][:4]:
            todo.append((case["seed"], case["core_size"], case["entry_dist"], case["epsilon"], case["multi_hits"],
                         case["hmmer3_compat"], s))
    from oracle_py import encode
    for seed, M, entry, eps, multi, h3, text in todo:
        op = oracle64.sample(seed, M, entry, eps)
        seq = encode(text)
        op.setup(len(seq), multi, h3)
        rc, _, path = op.viterbi(1, seq)
        if rc or not path:
            continue
        for precision in (32, 64):
            prof = dcp.ProteinProfile.sample(seed, M, dcp.ProteinCfg(entry, eps), precision=precision)
            yield prof, np.frombuffer(seq, np.uint8), np.array([(s, l, 0) for s, l in path], dcp.STEP_DTYPE)


def test_prod_row_with_codes_is_prod_row(dcp, oracle64):
    n = 0
    for prof, seq, steps in golden_rows(dcp, oracle64):
        codes = host_codes(prof, seq, steps)
        assert (codes == MUTE).sum() == (steps["seqlen"] == 0).sum() >= 2
        want = prof.prod_row(seq, steps, scan_id=3, seq_id=9, alt_loglik=-1.5, null_loglik=-2.5)
        assert prof.prod_row(seq, steps, scan_id=3, seq_id=9, alt_loglik=-1.5, null_loglik=-2.5, codes=codes) == want
        n += 1
        if n == 1:
            with pytest.raises(dcp.DcpError):  # a wrong number of codes
                prof.prod_row(seq, steps, codes=codes[:-1])
            with pytest.raises(dcp.DcpError):
                prof.prod_row(seq, steps, codes=np.append(codes, MUTE))
            emit = int(np.nonzero(steps["seqlen"] > 0)[0][0])
            bad = codes.copy()
            bad[emit] = MUTE  # DCP_CODE_MUTE on an emitting step
            with pytest.raises(dcp.DcpError):
                prof.prod_row(seq, steps, codes=bad)
            bad[emit] = 64  # no codon
            with pytest.raises(dcp.DcpError):
                prof.prod_row(seq, steps, codes=bad)
            bad = codes.copy()
            bad[0] = 5  # a codon on the mute S step
            with pytest.raises(dcp.DcpError):
                prof.prod_row(seq, steps, codes=bad)
            # the C call itself returns -1
            buf = C.create_string_buffer(4096)
            st = np.ascontiguousarray(steps)
            bad[0], bad[emit] = MUTE, MUTE
            assert dcp.lib.dcp_prod_format_row_codes(buf, 4096, 0, 0, b"x", b"dna", 0.0, 0.0, b"protein", b"0", prof._h,
                                                     seq.ctypes.data, len(seq), st.ctypes.data, len(st), bad.ctypes.data) == -1
    assert n >= 10


# ---- GPU -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def word_case(dcp):
    """The every-word inputs and, per precision, the profiles and the host's codes of every path (computed once)."""
    seq, hits, paths = word_paths(dcp)
    case = {"seq": seq, "hits": hits, "paths": paths}
    for precision in (32, 64):
        profs = word_profiles(dcp, precision)
        case[precision] = (profs, [host_codes(profs[int(h["profile_idx"])], seq, p) for h, p in zip(hits, paths)])
    return case


VARIANTS = {"float-two-layout": (32, False, {}), "float-one-layout-keep": (32, True, {"one_layout": True}),
            "float-host-expanded-keep": (32, True, {"expand_on_host": True}), "double-keep": (64, True, {})}


@gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_word_every_state_kind(dcp, word_case, variant):
    precision, keep, flags = VARIANTS[variant]
    profs, want = word_case[precision]
    sc = dcp.Scanner(0)
    try:
        sc.keep_dists(keep)
        sc.upload_db(profs, **flags)
        assert sc.has_dists and sc.precision == precision
        sc.upload_seqs([word_case["seq"]])
        got = sc.decode_paths(word_case["hits"], word_case["paths"])
    finally:
        sc.close()
    m = diff = 0
    for h, path, d, w in zip(word_case["hits"], word_case["paths"], got, want):
        a, b = check_rule(profs[int(h["profile_idx"])], word_case["seq"], path, d, w)
        m, diff = m + a, diff + b
    print("%s: %d of %d M steps differ from the host" % (variant, diff, m))
    assert m == 3 * 1364 * len(WORD_SIZES) and diff * 1000 <= m


@gpu
@pytest.mark.parametrize("precision", [32, 64])
def test_real_paths_both_strands(dcp, precision):
    profs, seqs = real_profiles(dcp, precision), real_seqs(dcp)
    sc = dcp.Scanner(0)
    try:
        sc.keep_dists(True)
        sc.upload_db(profs)
        sc.upload_seqs(seqs)
        sc.add_reverse_strand()
        sc.scan(True, False, 10.0)
        hits = sc.hits()
        resident = [sc.fetch_seq(q) for q in range(2 * len(seqs))]
        m = diff = rows = 0
        kinds = {False: set(), True: set()}  # emitting states met: "M", "I", or the special state's id
        for null_model in (False, True):
            paths, _ = sc.trace_paths(hits, True, False, null_model=null_model)
            codes = sc.decode_paths(hits, paths)
            for h, path, d in zip(hits, paths, codes):
                prof, seq = profs[int(h["profile_idx"])], resident[int(h["seq_idx"])]
                w = host_codes(prof, seq, path)
                a, b = check_rule(prof, seq, path, d, w)
                m, diff = m + a, diff + b
                for sid in set(path["state_id"][path["seqlen"] > 0].tolist()):
                    kinds[null_model].add({0: "M", 1: "I", 3: sid}[sid >> 14])
                if b == 0:
                    assert prof.prod_row(seq, path, codes=d) == prof.prod_row(seq, path)
                    rows += 1
    finally:
        sc.close()
    print("precision %d: %d hits, %d of %d M steps differ from the host" % (precision, len(hits), diff, m))
    assert len(hits) >= 2 and rows >= 1 and diff * 1000 <= m
    assert {"M", N, J, CC} <= kinds[False] and kinds[True] == {R}  # two-domain alt paths; null paths are R steps


@gpu
def test_round_edge(dcp):
    """2^20 + 3 one-base N steps cross the round of 2^20 emitting steps; the next path lies wholly behind it."""
    prof = dcp.ProteinProfile.sample(3, 2, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01))
    L = (1 << 20) + 3
    rng = np.random.default_rng(5)
    long_seq, short_seq = rng.integers(0, 4, L, dtype=np.uint8), np.array([0, 3, 2, 2, 1, 0, 3], np.uint8)
    table = np.array([host_codes(prof, np.array([b], np.uint8), np.array([(N, 1, 0)], dcp.STEP_DTYPE))[0] for b in range(4)])
    long_path = np.zeros(L, dcp.STEP_DTYPE)
    long_path["state_id"], long_path["seqlen"] = N, 1
    short_path = np.array([(S, 0, 0), (B, 0, 0), (1, 3, 0), (D_(2), 0, 0), (E, 0, 0), (CC, 4, 0), (T, 0, 0)], dcp.STEP_DTYPE)
    idx = np.dtype([("seq_idx", np.uint32), ("profile_idx", np.uint32)])
    sc = dcp.Scanner(0)
    try:
        sc.upload_db([prof])
        sc.upload_seqs([long_seq, short_seq])
        assert sc.decode_paths(np.zeros(0, idx), []) == []  # npaths == 0
        one = sc.decode_paths(np.array([(0, 0)], idx), [long_path])
        two = sc.decode_paths(np.array([(0, 0), (1, 0)], idx), [long_path, short_path])
        empty = sc.decode_paths(np.array([(1, 0), (1, 0)], idx), [short_path[:0], short_path])
    finally:
        sc.close()
    assert np.array_equal(one[0], table[long_seq])
    assert np.array_equal(two[0], table[long_seq])
    want = host_codes(prof, short_seq, short_path)
    assert np.array_equal(two[1], want) and np.array_equal(empty[1], want) and len(empty[0]) == 0
    assert list(want == MUTE) == [True, True, False, True, True, False, True]


def raw_decode(dcp, sc, hits, paths):
    """dcp_gpu_decode_paths with a sentinel-filled output: (rc, message, codes)."""
    off = np.zeros(len(paths) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in paths])
    steps = np.ascontiguousarray(np.concatenate(paths), dcp.STEP_DTYPE)
    out = np.full(int(off[-1]), 0xA5, np.uint8)
    sq, pr = np.ascontiguousarray(hits["seq_idx"], np.uint32), np.ascontiguousarray(hits["profile_idx"], np.uint32)
    rc = sc._lib.dcp_gpu_decode_paths(sc._c, sq.ctypes.data, pr.ctypes.data, len(paths), steps.ctypes.data, off.ctypes.data,
                                      out.ctypes.data)
    return rc, sc._lib.dcp_gpu_last_error(sc._c).decode(), out


@gpu
def test_refusals_leave_the_output_untouched(dcp):
    idx = np.dtype([("seq_idx", np.uint32), ("profile_idx", np.uint32)])
    M, L = 3, 12
    seq = np.array([0, 1, 2, 3, 3, 2, 1, 0, 0, 2, 1, 3], np.uint8)
    good = np.array([(S, 0, 0), (N, 1, 0), (B, 0, 0), (1, 3, 0), (I_(1), 2, 0), (2, 3, 0), (D_(3), 0, 0), (E, 0, 0), (CC, 3, 0),
                     (T, 0, 0)], dcp.STEP_DTYPE)
    assert int(good["seqlen"].sum()) == L

    def changed(i, sid=None, ln=None):
        p = good.copy()
        if sid is not None:
            p["state_id"][i] = sid
        if ln is not None:
            p["seqlen"][i] = ln
        return p

    one = np.array([(0, 0)], idx)
    for precision in (32, 64):
        prof = dcp.ProteinProfile.sample(8, M, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01), precision=precision)
        want = host_codes(prof, seq, good)
        sc = dcp.Scanner(0)
        try:
            # keep off: a one-layout float DB and a double DB release their dists as before, the tables are the same
            flags = {"one_layout": True} if precision == 32 else {}
            sc.upload_db([prof], **flags)
            sc.upload_seqs([seq])
            assert not sc.has_dists
            bytes_off = sc.table_bytes
            rc, msg, out = raw_decode(dcp, sc, one, [good])
            assert rc == dcp.RC_EINVAL and "dcp_gpu_db_keep_dists" in msg and np.all(out == 0xA5)
            sc.keep_dists(True)
            assert not sc.has_dists  # the setting speaks of later uploads
            sc.upload_db([prof], **flags)
            assert sc.has_dists and sc.table_bytes == bytes_off
            rc, msg, out = raw_decode(dcp, sc, one, [good])
            assert rc == 0 and np.array_equal(out, want)
            bad = [("no state", changed(3, sid=M + 1), one), ("no state", changed(4, sid=I_(0)), one),
                   ("no state", changed(1, sid=(3 << 14) | 8), one), ("seqlen 6", changed(3, ln=6), one),
                   ("seqlen 0", changed(1, ln=0), one), ("mute state with seqlen 1", changed(2, ln=1), one),
                   ("emit 13 bases", changed(8, ln=4), one), ("sequence 1 is not resident", good, np.array([(1, 0)], idx)),
                   ("profile 1 is not resident", good, np.array([(0, 1)], idx))]
            for what, path, hit in bad:
                rc, msg, out = raw_decode(dcp, sc, hit, [path])
                assert rc == dcp.RC_EINVAL and what in msg and np.all(out == 0xA5), (what, rc, msg)
                rc, msg, out = raw_decode(dcp, sc, one, [good])  # the next valid call is correct
                assert rc == 0 and np.array_equal(out, want), what
            # keep off again: the dists are gone as before
            sc.keep_dists(False)
            sc.upload_db([prof], **flags)
            assert not sc.has_dists and sc.table_bytes == bytes_off
        finally:
            sc.close()
    # without a batch, and a default two-layout float DB (it keeps its dists anyway)
    sc = dcp.Scanner(0)
    try:
        prof = dcp.ProteinProfile.sample(8, M, dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01))
        rc, msg, out = raw_decode(dcp, sc, one, [good])
        assert rc == dcp.RC_EINVAL and "no profile DB" in msg and np.all(out == 0xA5)
        sc.upload_db([prof])
        assert sc.has_dists
        rc, msg, out = raw_decode(dcp, sc, one, [good])
        assert rc == dcp.RC_EINVAL and "no sequences" in msg and np.all(out == 0xA5)
    finally:
        sc.close()


# ---- the near-tie counts of the docstring ----------------------------------------------------------------------------
def _count_near_ties():
    from conftest import load_product
    from oracle_py import Oracle

    dcp = load_product()
    seq, hits, paths = word_paths(dcp)
    for precision in (32, 64):
        profs = word_profiles(dcp, precision)
        n = close = 0
        for h, p in zip(hits, paths):
            a, b = near_ties(profs[int(h["profile_idx"])], seq, p)
            n, close = n + a, close + b
        print("every word, precision %d: %d of %d M steps have a runner-up within 2^-40" % (precision, close, n))
    # real paths: the oracle's Viterbi paths of the pairs it keeps (LRT >= 10), both strands, alt and null model
    seqs = real_seqs(dcp)
    both = seqs + [dcp.revcomp(s) for s in seqs]
    for precision in (32, 64):
        orc = Oracle(precision)
        profs = real_profiles(dcp, precision)
        n = close = nhits = 0
        for prm, prof in zip(real_params(), profs):
            cv = np.float64 if precision == 64 else np.float32
            op = orc.new(*[np.asarray(x, cv) for x in prm], ENTRY_DIST_OCCUPANCY, 0.01)
            for s in both:
                op.setup(len(s), True, False)
                _, nl, npath = op.viterbi(0, bytes(s))
                rc, al, apath = op.viterbi(1, bytes(s))
                if rc or not np.isfinite(al) or -2 * (nl - al) < 10.0:
                    continue
                nhits += 1
                for path in (apath, npath):
                    a, b = near_ties(prof, s, np.array([(x, y, 0) for x, y in path], dcp.STEP_DTYPE))
                    n, close = n + a, close + b
        print("real paths, precision %d: %d hits, %d of %d M steps have a runner-up within 2^-40" % (precision, nhits, close, n))


if __name__ == "__main__":
    _count_near_ties()
