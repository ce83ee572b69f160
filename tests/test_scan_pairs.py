"""dcp_gpu_scan_pairs / Scanner.scan_pairs: the row-sweep kernels of both precisions over a pair list the host wrote.

GPU, per precision: a DB with a profile on every edge of the size classes and launch groups and one flagged (positive
MD / DD) profile, queries of 1 .. 1 000 nt, two of them carrying a planted gene.  One KERNEL_ROWSWEEP scan with dense
scores is the reference: scan_pairs at threshold -inf returns, as a multiset, exactly the listed pairs whose dense
scores are finite, with the dense bits; at threshold 10 the full scan's hits restricted to the list.  Then the
accounting, the refusals with their messages, explicit transitions, and a normal scan behind a pair scan.

End to end, in the planted world cut 1 024 / 512 (test_domain_regions' premise): windows, domains, domain_regions,
cut_regions, scan_pairs, trace, path_domains, locate_domains -- one domain per region from node 1 to node M, where the
premise found it, with the bits, path and product row of the region's slice uploaded alone."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits, np_revcomp, refused
from test_domain_regions import REGION_CUT, REGION_FLANK, planted_regions
from test_gpu_parity import pfam_like_params, planted_query
from test_seq_windows import PLANT_M, planted_world

PRECISIONS = (32, 64)
PAIR_M = (1, 64, 65, 128, 129, 300, 513, 1100)  # and a flagged profile of 90 nodes behind them
PAIR_L = (1, 2, 3, 17, 100, 333, 1000)
# capacities of the float row sweep's size classes (64 R W nodes) and of the double row sweep's launch groups
CLASS_CAPS = {32: (64, 128, 192, 256, 320, 384, 448, 512, 768, 1024, 1536, 2048, 3072, 4096), 64: (64, 128, 256, 4096)}
NEG_INF = float("-inf")
_WORLD = {}


def pair_world(dcp, orc, precision):
    """(profiles, queries, dense null, dense alt, hits at threshold 10) -- the reference scan runs once per precision"""
    if precision not in _WORLD:
        rng = np.random.default_rng(1700 + precision)
        params = [pfam_like_params(rng, M) for M in PAIR_M]
        null, match, trans = pfam_like_params(rng, 90)
        trans = trans.copy()
        trans[1:90, 2] = np.float32(0.7)  # MD > 0: the delete states decide E(j)
        trans[1:90, 6] = np.float32(0.4)
        params.append((null, match, trans))
        cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))
        profs = [dcp.ProteinProfile.from_params(*prm, cfg, f"PAIR{i}", precision=precision) for i, prm in enumerate(params)]
        seqs = [rng.integers(0, 4, L, dtype=np.uint8) for L in PAIR_L]
        # the 333-nt query carries the 64-node profile's gene, the 1 000-nt one the 300-node profile's
        for q, p, flank in ((5, 1, 70), (6, 5, 50)):
            gene = planted_query(rng, orc.new(*params[p], ENTRY_DIST_OCCUPANCY, 0.01), PAIR_M[p], flank=flank)
            seqs[q][:len(gene)] = gene
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs(seqs)
        sc.scan(True, False, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
        nl, al = sc.scores()
        every = sc.hits()
        sc.scan(True, False, 10.0, keep_scores=False, kernel=dcp.KERNEL_ROWSWEEP)
        _WORLD[precision] = (profs, seqs, nl, al, every, sc.hits().copy(), sc.cells)
        sc.close()
    return _WORLD[precision]


def records(h):
    return sorted(zip(h["seq_idx"].tolist(), h["profile_idx"].tolist(), bits(h["null_loglik"]).tolist(), bits(h["alt_loglik"]).tolist()))


def dense_records(nl, al, pairs, thr=NEG_INF):
    out = []
    for q, p in pairs:
        n, a = nl[q, p], al[q, p]
        with np.errstate(invalid="ignore", over="ignore"):
            lrt = -2 * (n - a)
        if np.isfinite(n) and np.isfinite(a) and np.isfinite(lrt) and lrt >= thr:
            out.append((q, p, int(bits(nl[q:q + 1, p])[0]), int(bits(al[q:q + 1, p])[0])))
    return sorted(out)


def pair_lists(precision):
    nq, npf = len(PAIR_L), len(PAIR_M) + 1
    rng = np.random.default_rng(5)
    every = [(q, p) for q in range(nq) for p in range(npf)]
    shuffled = [every[i] for i in rng.permutation(len(every))]
    sizes = PAIR_M + (90,)
    cls = [min(k for k, cap in enumerate(CLASS_CAPS[precision]) if M <= cap) for M in sizes]
    per_class = [(4 + k % 3, cls.index(k)) for k in sorted(set(cls))]  # the class's first profile, queries of 100 .. 1 000 nt
    return dict(all=shuffled, per_class=per_class, single=[(5, 1)], duplicate=[(6, 5), (4, 7), (6, 5), (6, 5)], empty=[])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["all", "per_class", "single", "duplicate", "empty"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pairs_have_the_dense_bits(dcp, oracle32, oracle64, precision, which):
    profs, seqs, nl, al, every, hits10, full_cells = pair_world(dcp, oracle64 if precision == 64 else oracle32, precision)
    pairs = pair_lists(precision)[which]
    if which == "all":  # the reference itself: every pair with finite scores is a hit at -inf, and most pairs have them
        assert records(every) == dense_records(nl, al, sorted(pairs)) and len(every) > len(pairs) // 2
    if which == "per_class":
        assert len(pairs) == (6 if precision == 32 else 4)  # 1 | 64, 65 | 128 | 90, 129, 300, 513, 1 100; the launch groups
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    sq, pr = [q for q, _ in pairs], [p for _, p in pairs]
    sc.scan_pairs(sq, pr, True, False, NEG_INF)
    want = dense_records(nl, al, pairs)
    assert records(sc.hits()) == want and (len(want) == len(pairs) or which == "all"), which
    # the accounting of a pair scan
    cells = sum(profs[p].core_size * len(seqs[q]) for q, p in pairs)
    assert sc.cells == cells and sc.last_scan_kernel == dcp.KERNEL_ROWSWEEP and sc.last_scan_redo_pairs == 0
    assert sc.algorithmic_bytes == sum(20 * profs[p].core_size * len(seqs[q]) + 32 * (profs[p].core_size + 1) + len(seqs[q]) + 8
                                       for q, p in pairs)
    nclasses = len({min(k for k, cap in enumerate(CLASS_CAPS[precision]) if profs[p].core_size <= cap) for _, p in pairs})
    assert sc.last_scan_launches == nclasses
    if precision == 32:
        infos = sc.launch_infos()
        assert len(infos) == nclasses and sum(i["cells"] for i in infos) == cells
        assert sorted(64 * i["R"] * i["W"] for i in infos) == sorted({min(cap for cap in CLASS_CAPS[32] if profs[p].core_size <= cap) for _, p in pairs})
    refused(dcp, sc, sc.scores)  # no dense matrix
    # threshold 10: the full scan's hits restricted to the list (a listed hit as often as it is listed)
    sc.scan_pairs(sq, pr, True, False, 10.0)
    sel = dense_records(nl, al, pairs, 10.0)
    assert records(sc.hits()) == sel
    assert sorted(set(sel)) == [r for r in records(hits10) if r[:2] in set(pairs)]
    if which in ("all", "single", "duplicate"):
        assert len(sel) >= (2 if which != "single" else 1)
    # the other flags, against the scan of the same flags
    if which == "all":
        for multi, h3 in ((False, False), (True, True)):
            sc.scan(multi, h3, NEG_INF, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
            fn, fa = sc.scores()
            sc.scan_pairs(sq, pr, multi, h3, NEG_INF)
            assert records(sc.hits()) == dense_records(fn, fa, pairs), (multi, h3)
    # a normal scan behind a pair scan is what it was
    sc.scan(True, False, 10.0, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    gn, ga = sc.scores()
    assert np.array_equal(bits(gn), bits(nl)) and np.array_equal(bits(ga), bits(al))
    assert records(sc.hits()) == records(hits10) and sc.cells == full_cells
    if precision == 32:
        assert sum(i["cells"] for i in sc.launch_infos()) == full_cells
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_transitions_and_an_asynchronous_scan(dcp, oracle32, oracle64, precision):
    profs, seqs, nl, al, every, hits10, _ = pair_world(dcp, oracle64 if precision == 64 else oracle32, precision)
    pairs = pair_lists(precision)["all"]
    sq, pr = np.array([q for q, _ in pairs], np.uint32), np.array([p for _, p in pairs], np.uint32)
    sc = dcp.Scanner(0)

    def message(call, *words):
        with pytest.raises(dcp.DcpError) as e:
            call()
        assert e.value.rc == dcp.RC_EINVAL and all(w in str(e.value) for w in words), str(e.value)

    def raw(keep_scores=0, kernel=0):
        prm = dcp.ScanParams(1, 0, 10.0, keep_scores, kernel)
        sc._check(sc._lib.dcp_gpu_scan_pairs(sc._c, C.byref(prm), sq.ctypes.data, pr.ctypes.data, len(sq)))

    message(lambda: sc.scan_pairs(sq, pr), "no profile DB")
    sc.upload_db(profs)
    message(lambda: sc.scan_pairs(sq, pr), "no sequences")
    sc.upload_seqs(seqs)
    sc.scan(True, False, 10.0, keep_scores=True, kernel=dcp.KERNEL_ROWSWEEP)
    message(lambda: raw(keep_scores=1), "keep_scores")
    for kernel in (2, 3, 4, -1):
        message(lambda: raw(kernel=kernel), "kernel")
    bad = sq.copy()
    bad[3] = bad[9] = len(seqs)
    message(lambda: sc.scan_pairs(bad, pr), "pair 3 ")
    bad = pr.copy()
    bad[11] = len(profs)
    message(lambda: sc.scan_pairs(sq, bad), "pair 11 ")
    with pytest.raises(dcp.DcpError):
        sc.scan_pairs(sq, pr[:-1])
    # every refusal left the last scan as it was
    gn, ga = sc.scores()
    assert np.array_equal(bits(gn), bits(nl)) and records(sc.hits()) == records(hits10)
    raw(kernel=1)  # the row sweep by name
    sc.sync()
    assert records(sc.hits()) == dense_records(nl, al, pairs, 10.0)
    # transitions of the other precision are refused, as the scans refuse them
    other = np.stack([(dcp.xtrans if precision == 64 else dcp.xtrans64)(len(s), True, False) for s in seqs])
    if precision == 64:
        sc.set_xtrans(other.astype(np.float32))
        message(lambda: sc.scan_pairs(sq, pr), "float")
    else:
        sc.set_xtrans64(other)
        message(lambda: sc.scan_pairs(sq, pr), "double")
    # explicit transitions apply per sequence and the flags are then ignored, as in a scan
    derived = dcp.xtrans64 if precision == 64 else dcp.xtrans
    sc.upload_seqs(seqs)
    sc.set_xtrans(np.stack([derived(len(s), True, False) for s in seqs]))
    sc.scan_pairs(sq, pr, False, True, NEG_INF)
    assert records(sc.hits()) == dense_records(nl, al, pairs)
    # asynchronous: the call returns with the scan enqueued; the fetch completes it.  And the caller's threshold of a
    # double DB is the one in force
    sc.upload_seqs(seqs)
    sc.scan_pairs(sq, pr, True, False, 10.0, sync=False)
    assert records(sc.hits()) == dense_records(nl, al, pairs, 10.0)
    sc.close()


# ---- end to end ----------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_end_to_end_in_the_planted_world(dcp, oracle32, oracle64, precision):
    orc = oracle64 if precision == 64 else oracle32
    profs, _, seq, _ = planted_world(dcp, orc, precision)
    _, _, want_reg, W, final = planted_regions(dcp, orc, precision)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    # 1, 2: windows of both strands, hits, paths, domains, located
    sc.upload_seqs([seq])
    sc.cut_windows(*REGION_CUT)
    sc.add_reverse_strand()
    assert sc.nseqs == 2 * W
    sc.scan(True, False, 10.0)
    hits = sc.hits()
    paths, _ = sc.trace_paths(hits, True, False)
    dom, _, _, _, _ = sc.path_domains(hits, paths, True, False)
    src, begin, end, minus = sc.locate_domains(hits, dom)
    profile = hits["profile_idx"][dom["path"]]
    # 3: the rule gives the premise's three regions
    reg_of, reg = dcp.domain_regions(src, minus, profile, begin, end, [len(seq)], 0, REGION_FLANK)
    assert [tuple(int(v) for v in r)[:5] for r in reg] == [r[:5] for r in want_reg]
    assert len(reg) == 3 and int(reg["nparts"].sum()) == len(dom) and np.array_equal(np.bincount(reg_of), reg["nparts"])
    long_gene = dom[profile == 2]
    assert len(long_gene) > 1 and not ((long_gene["node_first"] == 1) & (long_gene["node_last"] == PLANT_M[2])).any()
    # every slice uploaded alone: the bits, paths and rows the regions must reproduce
    alone = {}
    for i, r in enumerate(reg):
        piece = seq[r["begin"]:r["begin"] + r["len"]]
        piece = np_revcomp(piece) if r["minus"] else piece
        sc.upload_seqs([piece])
        sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
        own = [h.copy() for h in sc.hits() if h["profile_idx"] == r["profile"]]
        assert len(own) == 1
        own_paths, _ = sc.trace_paths(np.array(own), True, False)
        row = profs[r["profile"]].prod_row(piece, own_paths[0], 3, 77, own[0]["alt_loglik"], own[0]["null_loglik"])
        alone[i] = (piece, own[0], own_paths[0], row)
    # 4: the source again, the regions cut out of it, each scored against its profile
    sc.upload_seqs([seq])
    sc.cut_regions(reg["src"], reg["begin"], reg["len"], reg["minus"])
    assert sc.regions == 3 and [a.tolist() for a in sc.region_map()] == [reg[k].tolist() for k in ("src", "begin", "minus")]
    sc.scan_pairs(np.arange(3), reg["profile"], True, False, 10.0)
    hits = sc.hits()
    assert hits["seq_idx"].tolist() == [0, 1, 2] and hits["profile_idx"].tolist() == reg["profile"].tolist()
    assert sc.cells == sum(int(r["len"]) * PLANT_M[r["profile"]] for r in reg)
    # 5: one domain per region, from node 1 to node M, on the strand and source interval of the premise
    paths, alt = sc.trace_paths(hits, True, False)
    dom, dom_off, core, null, total = sc.path_domains(hits, paths, True, False)
    assert dom_off.tolist() == [0, 1, 2, 3] and np.array_equal(bits(total), bits(hits["alt_loglik"]))
    src, begin, end, minus = sc.locate_domains(hits, dom)
    pure = dcp.locate_domains_regions(hits["seq_idx"][dom["path"]], dom, reg["len"], reg["src"], reg["begin"], reg["minus"])
    assert all(np.array_equal(a, b) for a, b in zip(pure, (src, begin, end, minus)))
    for i, r in enumerate(reg):
        assert (int(dom[i]["node_first"]), int(dom[i]["node_last"])) == (1, PLANT_M[r["profile"]]), i
        assert [(int(begin[i]), int(end[i]), 1, PLANT_M[r["profile"]])] == final[i] and src[i] == 0 and minus[i] == r["minus"], i
        # 6: scores, paths and product rows are those of the slice uploaded alone
        piece, own, own_path, row = alone[i]
        assert bits(hits[i]["null_loglik"]) == bits(own["null_loglik"]) and bits(hits[i]["alt_loglik"]) == bits(own["alt_loglik"]), i
        assert np.array_equal(paths[i], own_path) and bits(alt[i]) == bits(own["alt_loglik"]), i
        bases = sc.fetch_seq(i)
        assert np.array_equal(bases, piece), i
        assert profs[r["profile"]].prod_row(bases, paths[i], 3, 77, hits[i]["alt_loglik"], hits[i]["null_loglik"]) == row, i
    sc.close()
