"""The oracle's traceback on given tables (orc_dp_tables_path, orc_path_score_tables), checked on the CPU.

The device's paths are compared with orc_dp_tables_path step for step (tests/test_trace_paths.py), so that walk must
itself be exactly orc_viterbi's: fed the tables the oracle's own model exports, it gives the generic Viterbi's alt
and null paths and scores bit for bit, ties included (first maximum in the order the model wires its transitions,
the shortest fragment first).  The fixtures are chosen to make ties and long paths: identical nodes, uniform entry,
periodic queries, the all-zero special transitions of a profile never set up, and multi-domain queries whose paths
cross long runs of delete states (longer than any 2L + c M estimate of their length).
"""
import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM, ORC_ENOMEM, encode

FLAGS = [(True, False), (False, False), (True, True)]
T_STATE, S_STATE = (3 << 14) | 7, (3 << 14) | 1


def norm(x):
    return x - np.logaddexp.reduce(x, axis=-1, keepdims=True)


def pfam_like_params(rng, M):
    """Peaked match distributions and Pfam-like transitions (MM ~ 0.95): a query of each node's best codon is a hit."""
    null = norm(np.log(rng.random(20) + 0.5)).astype(np.float32)
    match = np.log(rng.random((M, 20)) * 0.02 + 1e-3)
    match[np.arange(M), rng.integers(0, 20, M)] = np.log(0.8)
    match = norm(match).astype(np.float32)
    trans = np.tile(np.log(np.array([0.95, 0.025, 0.025, 0.6, 0.4, 0.6, 0.4])), (M + 1, 1))
    trans[0, 6] = -np.inf
    trans[M, 2] = trans[M, 6] = -np.inf
    trans[:, 0:3] = norm(trans[:, 0:3])
    trans[:, 3:5] = norm(trans[:, 3:5])
    with np.errstate(invalid="ignore"):
        dm = norm(trans[:, 5:7])
    trans[:, 5:7] = np.where(np.isnan(dm), trans[:, 5:7], dm)
    return null, match, trans.astype(np.float32)


def gapped_params(rng, M=1000):
    """pfam_like_params, but nodes 11 .. M-10 are crossed by deletes: MM/MI/MD 0.5/0.01/0.49 out of nodes 10 .. M-11,
    DM/DD 0.001/0.999 out of 11 .. M-11 (rows normalised, every log-probability <= 0)."""
    null, match, trans = pfam_like_params(rng, M)
    trans = trans.astype(np.float64)
    trans[10:M - 10, 0:3] = np.log([0.5, 0.01, 0.49])
    trans[11:M - 10, 5:7] = np.log([0.001, 0.999])
    return null, match, trans.astype(np.float32)


def best_codons(oprof, nodes):
    out = []
    for k in nodes:
        best, arg = -np.inf, None
        for c in range(64):
            frag = bytes([(c >> 4) & 3, (c >> 2) & 3, c & 3])
            lp, _ = oprof.decode(frag, k + 1)
            if lp > best:
                best, arg = lp, frag
        out.append(arg)
    return b"".join(out)


def gapped_query(rng, oprof, copies, M=1000):
    """`copies` domains, each the best codons of nodes 1..10 and M-9..M behind 6 random nt; 6 more at the end"""
    dom = best_codons(oprof, list(range(10)) + list(range(M - 10, M)))
    parts = []
    for _ in range(copies):
        parts += [rng.integers(0, 4, 6, dtype=np.uint8).tobytes(), dom]
    parts.append(rng.integers(0, 4, 6, dtype=np.uint8).tobytes())
    return b"".join(parts)


def identical_node_params(M, seed=5):
    """every node alike (same match row, same transitions): E(j) ties across k, and with uniform entry so do paths
    that enter and leave at different nodes"""
    rng = np.random.default_rng(seed)
    null, match, _ = pfam_like_params(rng, 1)
    _, _, trans = pfam_like_params(rng, M)  # its rows are alike but for the first's and the last's missing edges
    return null, np.tile(match[0], (M, 1)), trans


def flat_params(M):
    """null, insert and match distributions alike (every log-odds 0): with one node (uniform entry costs 0) and the
    LOG1 special transitions, N, E and J reach B with the same value"""
    _, _, trans = pfam_like_params(np.random.default_rng(M), M)
    return np.zeros(20, np.float32), np.zeros((M, 20), np.float32), trans


def free_delete_params(M):
    """identical nodes whose delete runs cost nothing beyond entering and leaving them (MM/MI/MD 0.01/0.01/0.98,
    DM 0.5, DD = 0): a longer run ties with a shorter one, so D_k's two candidates tie"""
    null, match, trans = identical_node_params(M)
    trans = trans.astype(np.float64)
    trans[1:M, 0:3] = np.log([0.01, 0.01, 0.98])
    trans[1:M, 5:7] = [np.log(0.5), 0.0]
    return null, match, trans.astype(np.float32)


def bits(x):
    return np.float32(x).view(np.uint32)


def as_path(states_lens):
    st, ln = states_lens
    return list(zip(st.tolist(), ln.tolist()))


def check_pair(orc, prof, seq, setup=None):
    """orc_dp_tables_path on the profile's exported tables == orc_viterbi, paths and scores in bits; the path scorer
    gives the alt path the alt score's bits.  Returns the alt path."""
    if setup is not None:
        assert prof.setup(len(seq), *setup) == 0
    t8, em, ei, en, xt = prof.export()
    rc, ll, want = prof.viterbi(1, seq)
    rc0, ll0, want0 = prof.viterbi(0, seq)
    assert rc == 0 and rc0 == 0
    nl, al, apath, npath = orc.dp_tables_path(t8, em, ei, en, xt, seq)
    assert bits(al) == bits(ll) and bits(nl) == bits(ll0), (al, ll, nl, ll0)
    assert as_path(apath) == want
    assert as_path(npath) == want0
    if want:
        assert bits(orc.path_score_tables(t8, em, ei, en, xt, seq, *apath)) == bits(al)
    assert bits(orc.path_score_tables(t8, em, ei, en, xt, seq, *npath, alt=False)) == bits(nl)
    return want


def sampled(orc, M, entry, seed):
    if M == 1:  # orc_profile_sample starts at two nodes
        return orc.new(*pfam_like_params(np.random.default_rng(seed), 1), entry)
    return orc.sample(seed, M, entry, 0.01)


@pytest.mark.parametrize("M", [1, 2, 3, 5, 17, 64, 65, 130, 300])
def test_walk_on_exported_tables_is_the_generic_viterbi(oracle32, M):
    rng = np.random.default_rng(100 + M)
    lens = list(range(1, 10)) + [20, 61, 150 if M > 100 else 333]
    for entry in (ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM):
        prof = sampled(oracle32, M, entry, M + entry)
        for L in lens:
            seq = rng.integers(0, 4, L, dtype=np.uint8).tobytes()
            for multi, h3 in FLAGS:
                path = check_pair(oracle32, prof, seq, (multi, h3))
                assert path[0] == (S_STATE, 0) and path[-1] == (T_STATE, 0)
                assert sum(l for _, l in path) == L


def test_walk_on_planted_hits(oracle32):
    """one- and two-domain planted queries: paths through M, I and D of many nodes"""
    rng = np.random.default_rng(7)
    for M in (40, 129, 257):
        prof = oracle32.new(*pfam_like_params(rng, M))
        dom = best_codons(prof, range(M))
        for seq in (dom, rng.integers(0, 4, 30, dtype=np.uint8).tobytes() + dom[: 3 * M // 2] + dom[3 * M // 2 + 7:],
                    dom + rng.integers(0, 4, 11, dtype=np.uint8).tobytes() + dom):
            for multi, h3 in FLAGS:
                path = check_pair(oracle32, prof, seq, (multi, h3))
                assert sum(1 for s, _ in path if s >> 14 == 0) >= M // 2


@pytest.mark.parametrize("M", [1, 2, 3, 8, 40, 300])
def test_ties_of_identical_nodes(oracle32, M):
    """Identical nodes, uniform entry, periodic queries: many alignments score exactly alike, and the walk must take
    the generic Viterbi's among them.  A one-codon query makes it explicit: entering at node k, emitting the codon and
    leaving for E scores the same for every k, and E takes the first wired edge, M_M -> E."""
    null, match, trans = identical_node_params(M)
    prof = oracle32.new(null, match, trans, ENTRY_DIST_UNIFORM)
    codon = best_codons(prof, [0])
    seqs = [codon, codon * 2, codon * 7, b"\x00\x01" * 11, b"\x02" * 9, (codon + b"\x03") * 5,
            bytes(np.random.default_rng(M).integers(0, 4, 90, dtype=np.uint8))]
    for seq in seqs:
        for multi, h3 in FLAGS:
            check_pair(oracle32, prof, seq, (multi, h3))
        check_pair(oracle32, prof, seq)  # and with the specials as left by the last setup of another length
    prof.setup(3, False, False)
    t8, em, ei, en, xt = prof.export()
    _, al, apath, _ = oracle32.dp_tables_path(t8, em, ei, en, xt, codon)
    got = as_path(apath)
    assert got[-3:] == [(M, 3), ((3 << 14) | 4, 0), (T_STATE, 0)]  # node M: E's first candidate wins the tie
    assert sum(1 for s, _ in got if s >> 14 == 0) == 1
    # the tie is real: the same alignment through node 1 scores the same bits
    alt_path = [(s if s >> 14 else 1, l) for s, l in got]
    assert bits(oracle32.path_score_tables(t8, em, ei, en, xt, codon, *zip(*alt_path))) == bits(al)


def test_ties_into_b_and_along_delete_runs(oracle32):
    """exact ties of B's candidates (a flat one-node profile without setup) and of D's (free delete runs)"""
    rng = np.random.default_rng(13)
    prof = oracle32.new(*flat_params(1), ENTRY_DIST_UNIFORM)
    for L in (1, 2, 3, 5, 8, 13, 40):
        check_pair(oracle32, prof, rng.integers(0, 4, L, dtype=np.uint8).tobytes())
    for M in (5, 40, 130):
        prof = oracle32.new(*free_delete_params(M), ENTRY_DIST_UNIFORM)
        codon = best_codons(prof, [0])
        deletes = 0
        for seq in (codon * 4, codon * 12, (codon + b"\x01") * 6, rng.integers(0, 4, 70, dtype=np.uint8).tobytes()):
            for flags in FLAGS:
                deletes += sum(s >> 14 == 2 for s, _ in check_pair(oracle32, prof, seq, flags))
        assert deletes > 0


def test_all_zero_special_transitions(oracle32):
    """A profile never set up keeps LOG1 = 0 on every special transition: N, E and J reach B alike, E -> T and C -> T
    alike."""
    rng = np.random.default_rng(11)
    for M in (1, 2, 9, 64, 200):
        prof = sampled(oracle32, M, ENTRY_DIST_OCCUPANCY if M % 2 else ENTRY_DIST_UNIFORM, 30 + M)
        assert not prof.export()[4][1:].any()
        for L in (1, 2, 4, 7, 30, 151):
            check_pair(oracle32, prof, rng.integers(0, 4, L, dtype=np.uint8).tobytes())
    null, match, trans = identical_node_params(12)
    prof = oracle32.new(null, match, trans, ENTRY_DIST_UNIFORM)
    for seq in (b"\x01" * 12, b"\x00\x03\x02" * 10):
        check_pair(oracle32, prof, seq)


@pytest.mark.parametrize("copies", [3, 8])
def test_paths_through_long_delete_runs(oracle32, copies):
    """k planted copies of nodes 1..10 and 991..1000 of a 1 000-node profile whose middle is crossed by deletes: a
    k-domain hit of about 1 000 steps per domain, longer than the 2L + 2M + 16 steps the device's paths were sized at
    and, with 8 copies, than 2L + 3M + 16 (where Profile.viterbi starts and must now retry at the true count) and the
    4(L + M) + 64 steps the device's walk once stopped at."""
    rng = np.random.default_rng(1000 + copies)
    prof = oracle32.new(*gapped_params(rng))
    seq = gapped_query(rng, prof, copies)
    L, M = len(seq), 1000
    prof.setup(L, True, False)
    path = check_pair(oracle32, prof, seq)
    assert len(path) > 2 * L + 2 * M + 16
    if copies == 8:
        assert len(path) > 2 * L + 3 * M + 16 and len(path) > 4 * (L + M) + 64
    assert sum(1 for s, _ in path if s == (3 << 14) | 3) == copies  # one B per domain
    assert sum(1 for s, _ in path if s >> 14 == 2) == copies * 980
    _, ll0, _ = prof.viterbi(0, seq, False)
    _, ll, _ = prof.viterbi(1, seq, False)
    assert -2 * (ll0 - ll) >= 10  # a real hit
    # the raw call reports the shortfall with the true count
    import ctypes as C
    st, ln, n = np.zeros(16, np.uint16), np.zeros(16, np.uint8), C.c_uint(16)
    out = oracle32.fl()
    rc = oracle32.lib.orc_viterbi(prof.h, 1, seq, L, C.byref(out), st.ctypes.data, ln.ctypes.data, C.byref(n))
    assert rc == ORC_ENOMEM and n.value == len(path)


def host_test_gapped_profile(orc):
    """the 1 000-node profile tests/c/test_scan_host.c builds (long_multi_domain_paths), in the oracle"""
    M, f = 1000, lambda x: np.float32(np.log(np.float32(x)))
    amino = "ACDEFGHIKLMNPQRSTVWY"
    null = np.full(20, f(1 / 20), np.float32)
    match = np.full((M, 20), f(0.01), np.float32)
    for k in range(M):
        match[k, amino.index("W" if k % 3 == 0 else "M")] = f(0.81)
    trans = np.zeros((M + 1, 7), np.float32)
    for i in range(M + 1):
        t = [f(0.95), f(0.025), f(0.025), f(0.6), f(0.4), f(0.6), f(0.4)]
        if 10 <= i < M - 10:
            t[0:3] = [f(0.5), f(0.01), f(0.49)]
        if 11 <= i < M - 10:
            t[5:7] = [f(0.001), f(0.999)]
        if i == 0:
            t[6], t[5] = -np.inf, 0.0
        if i == M:
            t[2], t[6], t[0], t[5] = -np.inf, -np.inf, f(0.975), 0.0
        trans[i] = t
    dom = "".join("TGG" if k % 3 == 0 else "ATG" for k in list(range(10)) + list(range(M - 10, M)))
    return orc.new(null, match, trans, ENTRY_DIST_OCCUPANCY, 0.01), dom


def test_step_counts_pinned_in_the_c_host_test(oracle32):
    """tests/c/test_scan_host.c checks imm_dp_viterbi's and scan_run_local's step counts of its gapped queries against
    3 016 and 8 036: the oracle's, on the same profile"""
    prof, dom = host_test_gapped_profile(oracle32)
    for copies, want in ((3, 3016), (8, 8036)):
        seq = encode(("ACGTAC" + dom) * copies + "GATTAC")
        prof.setup(len(seq), True, False)
        assert len(check_pair(oracle32, prof, seq)) == want


def test_path_score_tables_rejects_what_is_not_a_path(oracle32):
    rng = np.random.default_rng(3)
    prof = oracle32.new(*pfam_like_params(rng, 20))
    seq = best_codons(prof, range(20))
    prof.setup(len(seq), True, False)
    t8, em, ei, en, xt = prof.export()
    _, al, (st, ln), (nst, nln) = oracle32.dp_tables_path(t8, em, ei, en, xt, seq)
    score = lambda s, l, alt=True: oracle32.path_score_tables(t8, em, ei, en, xt, seq, s, l, alt)
    assert bits(score(st, ln)) == bits(al)
    assert np.isnan(score(st[1:], ln[1:]))            # no S
    assert np.isnan(score(st[:-1], ln[:-1]))          # no T
    m = int(np.flatnonzero(st >> 14 == 0)[3])
    assert np.isnan(score(np.delete(st, m), np.delete(ln, m)))  # a node skipped (and the query not covered)
    st2 = st.copy()
    st2[m] += 1                                       # M_k -> M_{k+2}: no such edge
    assert np.isnan(score(st2, ln))
    ln2 = ln.copy()
    ln2[m] = 6
    assert np.isnan(score(st, ln2))
    assert np.isnan(score(st, ln, alt=False)) and np.isnan(score(nst, nln, alt=True))


def test_double_precision_build(oracle64):
    """the f64 oracle has the same walk"""
    rng = np.random.default_rng(64)
    for M in (1, 7, 90):
        prof = sampled(oracle64, M, ENTRY_DIST_OCCUPANCY, M)
        for L in (1, 5, 9, 80):
            seq = rng.integers(0, 4, L, dtype=np.uint8).tobytes()
            prof.setup(L, True, False)
            t8, em, ei, en, xt = prof.export()
            rc, ll, want = prof.viterbi(1, seq)
            nl, al, apath, _ = oracle64.dp_tables_path(t8, em, ei, en, xt, seq)
            assert al == ll and as_path(apath) == want
            assert oracle64.path_score_tables(t8, em, ei, en, xt, seq, *apath) == al
