"""Device tracebacks (dcp_gpu_trace_paths) step for step against the oracle's walk on the device's own tables.

For every pair traced, hit or not, orc_dp_tables_path is fed the tables the device holds (transitions, the match
table read back from the device, the host's insert and null tables, the special transitions of the pair) and its path
must equal the device's step for step; the score the trace recomputes must equal the scan's in bits, and the
oracle's.  tests/test_trace_oracle.py proves that walk equal to orc_viterbi's, ties included, on the CPU.
"""
import ctypes as C

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM
from test_trace_oracle import (FLAGS, best_codons, flat_params, free_delete_params, gapped_params, gapped_query,
                               identical_node_params, pfam_like_params)

pytestmark = pytest.mark.gpu

CLASS_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 192, 256, 257, 384, 385, 512, 513, 768, 1024, 1025, 2048, 2049, 4096]


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scanner(dcp):
    s = dcp.Scanner(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def hooks_scanner(dcp):
    s = dcp.Scanner(0, lib=dcp.load_testhooks())
    yield s
    s.test_set_trace_mode(0, 0)
    s.close()


def build(dcp, orc, params, entry=ENTRY_DIST_OCCUPANCY, eps=0.01):
    cfg = dcp.ProteinCfg(entry, eps)
    return [dcp.ProteinProfile.from_params(*prm, cfg) for prm in params], [orc.new(*prm, entry, eps) for prm in params]


class Tables:
    """the tables of each resident profile as the device holds them (what oracle_dp_on_product_tables feeds)"""

    def __init__(self, dcp, sc, profiles, eps=0.01):
        eps = float(np.float32(eps))
        self.t = [(p.trans8, sc.match_table(i), dcp.frame_table_host(p.insert_dist, eps),
                   dcp.frame_table_host(p.null_dist, eps)) for i, p in enumerate(profiles)]


def trace_and_check(dcp, orc, sc, tabs, seqs, pairs, multi, h3, xt=None, null_model=False, trace=None):
    """traces `pairs` [(q, p)] (in that order) and checks every path and score; returns the paths"""
    nl, al = sc.scores()
    hits = np.array([(q, p, nl[q, p], al[q, p]) for q, p in pairs], dcp.HIT_DTYPE)
    paths, got = (trace or sc.trace_paths)(hits, multi, h3, null_model)
    assert len(paths) == len(pairs)
    for (q, p), path, g in zip(pairs, paths, got):
        seq = bytes(seqs[q])
        x = xt[q] if xt is not None else dcp.xtrans(len(seq), multi, h3)
        t8, em, ei, en = tabs.t[p]
        onl, oal, apath, npath = orc.dp_tables_path(t8, em, ei, en, x, seq)
        want_score, want = (onl, npath) if null_model else (oal, apath)
        scan = nl[q, p] if null_model else al[q, p]
        assert bits(g) == bits(scan) == bits(want_score), (q, p, g, scan, want_score)
        assert np.array_equal(path["state_id"], want[0]) and np.array_equal(path["seqlen"], want[1]), (
            q, p, len(path), len(want[0]))
        assert int(path["seqlen"].sum()) == len(seq)
    return paths


def finite_pairs(sc, nseqs, nprof, rng=None):
    _, al = sc.scores()
    pairs = [(q, p) for q in range(nseqs) for p in range(nprof) if np.isfinite(al[q, p])]
    if rng is not None:
        pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    return pairs


def size_class_queries(rng, oprofs, sizes, long_nt):
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in range(1, 10)]
    seqs += [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(20, 400, 4)]
    flank = lambda n: rng.integers(0, 4, n, dtype=np.uint8).tobytes()
    for i in (2, 8, 12):  # one-domain planted hits, and a two-domain one
        seqs.append(np.frombuffer(flank(20) + best_codons(oprofs[i], range(sizes[i])) + flank(9), np.uint8))
    d = best_codons(oprofs[5], range(sizes[5]))
    seqs.append(np.frombuffer(flank(5) + d + flank(40) + d + flank(3), np.uint8))
    seqs.append(rng.integers(0, 4, long_nt, dtype=np.uint8))
    return seqs


@pytest.mark.parametrize("multi,h3,on_host", [(True, False, True), (False, False, False), (True, True, True)])
def test_size_class_edges(dcp, oracle32, scanner, multi, h3, on_host):
    """every size-class edge, queries of 1 .. 9 nt up to 2.5 kbp and planted one- and two-domain hits: every pair
    with a finite score, hit or not, traced in a shuffled order"""
    rng = np.random.default_rng(17 + 2 * int(multi) + int(h3))
    params = [pfam_like_params(rng, M) for M in CLASS_EDGES]
    profiles, oprofs = build(dcp, oracle32, params)
    seqs = size_class_queries(rng, oprofs, CLASS_EDGES, 2500)
    scanner.upload_db(profiles, expand_on_host=on_host)
    scanner.upload_seqs(seqs)
    scanner.scan(multi, h3, 10.0)
    pairs = finite_pairs(scanner, len(seqs), len(profiles), rng)
    assert len(pairs) > 300
    paths = trace_and_check(dcp, oracle32, scanner, Tables(dcp, scanner, profiles), seqs, pairs, multi, h3)
    # the planted pairs went through their domains
    for q, p in ((13, 2), (14, 8), (15, 12), (16, 5)):
        path = paths[pairs.index((q, p))]
        nb = int(np.sum(path["state_id"] == ((3 << 14) | 3)))
        assert np.sum(path["state_id"] >> 14 == 0) >= CLASS_EDGES[p] // 2
        assert nb >= (2 if q == 16 and multi else 1)


@pytest.mark.parametrize("one_layout,on_host", [(False, True), (True, True), (True, False)])
def test_table_layouts(dcp, oracle32, scanner, one_layout, on_host):
    """many small profiles share table rows (their ldk is the group's, not their own width), a one-layout DB, and
    tables expanded on the device against the host"""
    rng = np.random.default_rng(5 + int(one_layout) + 2 * int(on_host))
    sizes = [int(m) for m in rng.integers(1, 64, 24)] + [3, 96, 128, 200, 300, 640]
    params = [pfam_like_params(rng, M) for M in sizes]
    profiles, oprofs = build(dcp, oracle32, params)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (1, 4, 7, 9, 40, 130, 601)]
    seqs.append(np.frombuffer(best_codons(oprofs[3], range(sizes[3])) * 2, np.uint8))
    scanner.upload_db(profiles, expand_on_host=on_host, one_layout=one_layout)
    scanner.upload_seqs(seqs)
    tabs = Tables(dcp, scanner, profiles)
    for multi, h3 in FLAGS:
        scanner.scan(multi, h3, 10.0)
        trace_and_check(dcp, oracle32, scanner, tabs, seqs, finite_pairs(scanner, len(seqs), len(profiles), rng),
                        multi, h3)


def test_explicit_special_transitions(dcp, oracle32, scanner):
    """special transitions never set up (LOG1 = 0: N, E and J tie into B), stale, E -> B free, N -> B closed,
    arbitrary: the trace walks on the pair's own"""
    rng = np.random.default_rng(91)
    sizes = [1, 2, 77, 129, 300]
    params = [pfam_like_params(rng, M) for M in sizes]
    profiles, oprofs = build(dcp, oracle32, params)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (3, 8, 50, 200, 260, 90)]
    seqs += [np.frombuffer(best_codons(oprofs[2], range(77)) * 2, np.uint8)] * 2
    xt = np.zeros((len(seqs), 13), np.float32)       # 0, 6: never set up
    xt[1] = dcp.xtrans(5000, True, False)             # stale
    xt[2] = dcp.xtrans(len(seqs[2]), False, False)
    xt[3] = -rng.random(13).astype(np.float32) * 3    # arbitrary
    xt[4] = dcp.xtrans(len(seqs[4]), True, False)
    xt[4, 9] = 0.0                                    # E -> B free
    xt[5] = dcp.xtrans(len(seqs[5]), True, False)
    xt[5, 4] = -np.inf                                # N -> B closed: only S -> B enters
    xt[7] = dcp.xtrans(len(seqs[7]), True, True)
    scanner.upload_db(profiles, expand_on_host=True)
    scanner.upload_seqs(seqs)
    scanner.set_xtrans(xt)
    scanner.scan(True, False, 10.0)
    trace_and_check(dcp, oracle32, scanner, Tables(dcp, scanner, profiles), seqs,
                    finite_pairs(scanner, len(seqs), len(profiles), rng), True, False, xt=xt)


@pytest.mark.parametrize("multi,h3", FLAGS)
def test_tie_heavy_fixtures(dcp, oracle32, scanner, multi, h3):
    """identical nodes with uniform entry and periodic queries: alignments at different nodes score alike to the bit,
    and the device must take the oracle's among them"""
    rng = np.random.default_rng(23)
    sizes = [1, 2, 3, 40, 64, 65, 129, 300, 513]
    params = [identical_node_params(M, seed=M) for M in sizes]
    profiles, oprofs = build(dcp, oracle32, params, ENTRY_DIST_UNIFORM)
    codon = best_codons(oprofs[0], [0])
    seqs = [np.frombuffer(s, np.uint8) for s in (codon, codon * 2, codon * 9, b"\x00\x01" * 11, b"\x02" * 9,
                                                 (codon + b"\x03") * 13, codon * 200)]
    seqs.append(rng.integers(0, 4, 150, dtype=np.uint8))
    scanner.upload_db(profiles, expand_on_host=True)
    scanner.upload_seqs(seqs)
    scanner.scan(multi, h3, 10.0)
    paths = trace_and_check(dcp, oracle32, scanner, Tables(dcp, scanner, profiles), seqs,
                            [(q, p) for q in range(len(seqs)) for p in range(len(profiles))], multi, h3)
    if not multi:  # one codon: E's first candidate (M_M) wins the tie of entering and leaving at any node
        for p, M in enumerate(sizes):
            st = paths[p]["state_id"]
            assert list(st[-3:]) == [M, (3 << 14) | 4, (3 << 14) | 7]


def test_ties_into_b_and_along_delete_runs(dcp, oracle32, scanner):
    """a flat one-node profile under LOG1 special transitions (N, E and J tie into B) and free delete runs (D_k's two
    candidates tie), with the specials never set up and set up for each flag"""
    rng = np.random.default_rng(29)
    sizes = [1, 1, 5, 40, 130, 257]
    params = [flat_params(1)] + [free_delete_params(M) for M in sizes[1:]]
    profiles, oprofs = build(dcp, oracle32, params, ENTRY_DIST_UNIFORM)
    codon = best_codons(oprofs[2], [0])
    seqs = [np.frombuffer(s, np.uint8) for s in (codon, codon * 4, codon * 12, (codon + b"\x01") * 6, codon * 90)]
    seqs += [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (1, 2, 5, 8, 13, 70)]
    scanner.upload_db(profiles, expand_on_host=True)
    scanner.upload_seqs(seqs)
    tabs = Tables(dcp, scanner, profiles)
    pairs = [(q, p) for q in range(len(seqs)) for p in range(len(profiles))]
    for multi, h3 in FLAGS:
        scanner.scan(multi, h3, 10.0)
        trace_and_check(dcp, oracle32, scanner, tabs, seqs, pairs, multi, h3)
    xt = np.zeros((len(seqs), 13), np.float32)
    scanner.set_xtrans(xt)
    scanner.scan(True, False, 10.0)
    trace_and_check(dcp, oracle32, scanner, tabs, seqs, pairs, True, False, xt=xt)


def test_null_model_paths(dcp, oracle32, scanner):
    rng = np.random.default_rng(31)
    sizes = [1, 64, 300]
    profiles, _ = build(dcp, oracle32, [pfam_like_params(rng, M) for M in sizes])
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (1, 2, 3, 4, 5, 6, 9, 33, 400, 3001)]
    scanner.upload_db(profiles, expand_on_host=True)
    scanner.upload_seqs(seqs)
    scanner.scan(True, False, 10.0)
    trace_and_check(dcp, oracle32, scanner, Tables(dcp, scanner, profiles), seqs,
                    [(q, p) for q in range(len(seqs)) for p in range(len(profiles))], True, False, null_model=True)


def test_budgets_modes_order_and_duplicates(dcp, oracle32, hooks_scanner):
    """a trace budget so small that every hit takes its own round of launches, the trace kernel's own forward loop
    (mode 1), the caller's order kept and duplicate hits"""
    sc = hooks_scanner
    rng = np.random.default_rng(41)
    sizes = [1, 65, 129, 257, 513, 1025, 2049]
    params = [pfam_like_params(rng, M) for M in sizes]
    profiles, oprofs = build(dcp, oracle32, params)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (1, 7, 64, 333)]
    seqs.append(np.frombuffer(best_codons(oprofs[3], range(257)) * 2, np.uint8))
    sc.upload_db(profiles, expand_on_host=True)
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0)
    pairs = finite_pairs(sc, len(seqs), len(profiles), rng)
    pairs = pairs + pairs[:7] + [pairs[3]] * 3
    tabs = Tables(dcp, sc, profiles)
    try:
        for mode, budget in ((0, 1), (1, 0), (1, 1 << 16), (0, 0)):
            sc.test_set_trace_mode(mode, budget)
            trace_and_check(dcp, oracle32, sc, tabs, seqs, pairs, True, False)
    finally:
        sc.test_set_trace_mode(0, 0)


@pytest.mark.parametrize("own_forward", [0, 1])
def test_paths_through_long_delete_runs(dcp, oracle32, hooks_scanner, own_forward):
    """3 and 8 planted copies of nodes 1..10 and 991..1000 of a 1 000-node profile crossed by deletes: paths of
    3 016 and 8 036 steps, longer than the 2L + 2M + 16 a hit's capacity is first sized at and (8 copies) than the
    walk's old 4(L + M) + 64 guard.  They used to fail the whole call (DCP_EFAIL)."""
    sc = hooks_scanner
    rng = np.random.default_rng(1003)
    params = gapped_params(rng)
    profiles, oprofs = build(dcp, oracle32, [params])
    seqs = [np.frombuffer(gapped_query(rng, oprofs[0], c), np.uint8) for c in (3, 8)]
    seqs.append(rng.integers(0, 4, 300, dtype=np.uint8))
    sc.upload_db(profiles, expand_on_host=True)
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0)
    hits = sc.hits()
    assert [(int(h["seq_idx"]), int(h["profile_idx"])) for h in hits][:2] == [(0, 0), (1, 0)]
    try:
        sc.test_set_trace_mode(own_forward, 0)
        paths = trace_and_check(dcp, oracle32, sc, Tables(dcp, sc, profiles), seqs, [(0, 0), (2, 0), (1, 0)], True,
                                False)
    finally:
        sc.test_set_trace_mode(0, 0)
    for path, copies in ((paths[0], 3), (paths[2], 8)):
        L = len(seqs[0 if copies == 3 else 1])
        assert len(path) > 2 * L + 2 * 1000 + 16
        assert int(np.sum(path["state_id"] >> 14 == 2)) == 980 * copies


def test_small_step_capacity_reports_the_needed_total(dcp, oracle32, scanner):
    rng = np.random.default_rng(51)
    profiles, oprofs = build(dcp, oracle32, [pfam_like_params(rng, M) for M in (20, 300)])
    seqs = [rng.integers(0, 4, 90, dtype=np.uint8), np.frombuffer(best_codons(oprofs[1], range(300)), np.uint8)]
    scanner.upload_db(profiles, expand_on_host=True)
    scanner.upload_seqs(seqs)
    scanner.scan(True, False, 10.0)
    nl, al = scanner.scores()
    hits = np.array([(q, p, nl[q, p], al[q, p]) for q in range(2) for p in range(2)], dcp.HIT_DTYPE)
    paths, _ = scanner.trace_paths(hits)
    total = sum(len(p) for p in paths)
    for cap in (0, 1, total - 1):
        off = np.zeros(len(hits) + 1, np.uint32)
        steps = np.zeros(max(cap, 1), dcp.STEP_DTYPE)
        rc = scanner._lib.dcp_gpu_trace_paths(scanner._c, hits.ctypes.data, len(hits), 1, 0, 0, steps.ctypes.data,
                                              cap, off.ctypes.data, None)
        assert rc == dcp.RC_ENOMEM and off[-1] == total
        assert list(np.diff(off)) == [len(p) for p in paths]
    off = np.zeros(len(hits) + 1, np.uint32)
    steps = np.zeros(total, dcp.STEP_DTYPE)
    assert scanner._lib.dcp_gpu_trace_paths(scanner._c, hits.ctypes.data, len(hits), 1, 0, 0, steps.ctypes.data,
                                            total, off.ctypes.data, None) == 0
    assert np.array_equal(steps, np.concatenate(paths))


def free_device_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipSetDevice(0) == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_one_hit_whose_work_area_exceeds_2_32_floats(dcp, oracle32, scanner):
    """M = 4096 against 360 kbp: 3 (L + 1) 4096 + 5 (L + 1) = 4.42e9 floats (17.7 GB) of work area for one hit.  Its
    path must be a path of the device's tables whose score, summed step by step in the DP's float order, is the
    scan's to the bit, and it must cover the query."""
    if free_device_bytes() < 24 << 30:
        pytest.skip("less than 24 GiB of free device memory")
    rng = np.random.default_rng(4096)
    profiles, oprofs = build(dcp, oracle32, [pfam_like_params(rng, 4096)])
    L = 360_000
    assert 3 * (L + 1) * 4096 + 5 * (L + 1) > 1 << 32
    dom = np.frombuffer(best_codons(oprofs[0], range(4096)), np.uint8)
    seq = rng.integers(0, 4, L, dtype=np.uint8)
    seq[100_000:100_000 + dom.size] = dom
    seq[250_000:250_000 + dom.size] = dom
    scanner.upload_db(profiles, expand_on_host=True)
    scanner.upload_seqs([seq])
    scanner.scan(True, False, 10.0)
    nl, al = scanner.scores()
    hits = np.array([(0, 0, nl[0, 0], al[0, 0])], dcp.HIT_DTYPE)
    (path,), got = scanner.trace_paths(hits)
    t8, em, ei, en = Tables(dcp, scanner, profiles).t[0]
    xt = dcp.xtrans(L, True, False)
    score = oracle32.path_score_tables(t8, em, ei, en, xt, bytes(seq), path["state_id"], path["seqlen"])
    assert bits(got[0]) == bits(al[0, 0]) == bits(score)
    assert int(path["seqlen"].sum()) == L
    assert int(np.sum(path["state_id"] == ((3 << 14) | 3))) >= 2  # both planted domains
