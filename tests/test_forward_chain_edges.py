"""forward_kernel / forward_wide_kernel (csrc/dcp_forward.hip) and backward_kernel / backward_wide_kernel
(csrc/dcp_posterior.hip) where the delete chain carries weight: the device against the host twin in the worlds of
tests/test_forward_chain_premises.py (runs on a real MI355X).

The worlds -- delete-heavy profiles of 64, 128, 256 (a full class R = 1, 2, 4: lane 63 holds real nodes), 257, 513,
1100 and 4096 nodes (16 chunks); positive-chain profiles of 64, 256, 600; delete-heavy profiles severed at a lane boundary
in the middle of the wave, inside lane 63 and at a chunk's first column; two epsilon-0 profiles; queries of 1, 6, 12 and
40 nt -- are defined there, once, and so is why they are needed: in the pfam-like world of tests/test_forward_pairs.py a
delete run of n nodes weighs 0.4^n, and what the far steps of the cross-lane scan and the carry from chunk to chunk bring
in lies below the allowance.

Per precision, multi-hit: forward_pairs and posterior_pairs on EVERY (query, profile), in a shuffled list, against
dcp.forward_tables / dcp.posterior_tables on the tables the device holds, under the project's allowances unchanged --
2^-32 (|x| + 1) on the scores, 4 x 2^-32 (X + 1) on the rows (within and device_tables of tests/test_forward_pairs.py,
check_against and rows_allow of tests/test_posterior_pairs.py); no NaN anywhere, -inf by equality; epsilon-0 pairs with
L mod 3 != 0 give -inf twice and all-zero rows; alt_bwd within the allowance of alt_fwd; posterior_pairs' Forward score
the bits of forward_pairs'.  With the hooks build a list of a 4096-node, a 257-node, a severed 1100-node and a 64-node
pair behind one another gives the uncapped bits with the wavefront cap at 1 and at 3 and with the posterior budget at
one pair's rows.

Why these tests could fail (asserted on the CPU in tests/test_forward_chain_premises.py, on the oracle's f64 tables of
the same profiles): each of the six scan steps left out, and each chunk carry cut (Forward: D, M of the chunk's last node
into the chain, its M, I, D into the next P; Backward: the carried bD, bP), moves the alt score of the delete-heavy
profiles of 64, 128, 256, 513 and 1100 nodes by at least 2^-26 (|x| + 1) -- 64 times what is allowed here; the
positive-chain profiles meet that for step o = 32; the severed profiles differ from the unsevered ones by more than that.
The host twins lie within the allowance of that emulation.  Measured minima of |delta| / (|x| + 1): scan steps 2^-23.6
Forward, 2^-25.9 Backward (1100 nodes x 6 nt, o = 32; at the other sizes 2^-21.2 at the least); chunk carries 2^-24.3
Forward (the insert state's carry alone, 1100 nodes x 12 nt; 2^-19.0 at the least for the others), 2^-15.4 Backward;
positive chain, o = 32: 2^-1.2; severed: 2^-13.5.  So a kernel with one of these knock-outs as its bug could not pass.

Measured maxima of |delta| / (|x| + 1), device against host twin, float / double DB (the test prints them per family;
DESIGN sections 19 and 20 record them): scores 2.3e-16 / 2.4e-16 delete-heavy and severed, 6.7e-15 / 6.7e-15 positive
chain, 1.5e-16 / 1.2e-16 epsilon 0; rows, of (X + 1), 3.9e-16 / 2.4e-16, 5.5e-15 / 5.1e-15, 8.6e-17 / 8.6e-17."""
import numpy as np
import pytest

import test_forward_chain_premises as pr
from oracle_py import ENTRY_DIST_OCCUPANCY
from test_both_strands import bits
from test_forward_pairs import PRECISIONS, device_tables, within, worst, xtrans_of
from test_posterior_pairs import check_against, same_bits, twin_rows, unpack

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
FAMILIES = ("delete", "positive", "severed", "eps0")
_WORLD = {}


def chain_world(dcp, precision):
    """specs, profiles, queries, and per (q, p) the host twin on the tables the device holds: (null, alt) of
    forward_tables and (begin, end, core, alt_fwd, alt_bwd, X) of posterior_tables; computed once"""
    if precision not in _WORLD:
        specs = pr.world_specs()
        profs = [dcp.ProteinProfile.from_params(*pr.chain_params(fam, M, k), dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, eps),
                                                "%s%d_%s" % (fam, M, k), precision=precision) for fam, M, k, eps in specs]
        assert [p.core_size for p in profs] == [s[1] for s in specs]
        seqs = pr.world_queries()
        sc = dcp.Scanner(0)
        sc.upload_db(profs)
        sc.upload_seqs(seqs)
        tabs = device_tables(dcp, sc, profs, precision, pr.EPS)
        if precision == 32:  # a float DB's insert and null tables are the host's expansion, at the profile's own epsilon
            for p, (fam, M, k, eps) in enumerate(specs):
                if eps != pr.EPS:
                    tabs[p] = tabs[p][:2] + (dcp.frame_table_host(profs[p].insert_dist, eps),
                                             dcp.frame_table_host(profs[p].null_dist, eps))
        sc.close()
        for p, (fam, M, k, eps) in enumerate(specs):  # the device holds the world the premises are about
            t8 = np.asarray(tabs[p][0], np.float64)
            assert t8.shape == (8, M) and tabs[p][1].shape[1] == M
            if fam == "severed":
                assert np.isneginf(t8[[4, 5], k]).all() and np.isfinite(t8[[4, 5], k - 1]).all()  # MD_k, DD_k
            if fam == "positive":
                assert (t8[[4, 5], 1:] > 0).all()
        fwd, post = {}, {}
        for q, s in enumerate(seqs):
            xt = xtrans_of(dcp, precision, len(s), True, False)
            for p in range(len(profs)):
                fwd[q, p] = dcp.forward_tables(*tabs[p], xt, s)
                post[q, p] = twin_rows(dcp, tabs[p], xt, s)
                assert bits(np.array([post[q, p][3]])) == bits(np.array([fwd[q, p][1]]))  # one sweep, stated once
        _WORLD[precision] = (specs, profs, seqs, fwd, post)
    return _WORLD[precision]


def loaded(dcp, precision, lib=None):
    profs, seqs = _WORLD[precision][1:3]
    sc = dcp.Scanner(0, lib=lib) if lib else dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    return sc


def index_of(specs, fam, M, k=None):
    return specs.index((fam, M, k, 0.0 if fam == "eps0" else pr.EPS))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_pair_against_the_host_twin(dcp, precision):
    specs, profs, seqs, ref_f, ref_p = chain_world(dcp, precision)
    every = [(q, p) for q in range(len(seqs)) for p in range(len(profs))]
    order = np.random.default_rng(13).permutation(len(every))
    sq, pp = np.array([every[i][0] for i in order]), np.array([every[i][1] for i in order])
    sc = loaded(dcp, precision)
    gn, ga = sc.forward_pairs(sq, pp)
    res = sc.posterior_pairs(sq, pp)
    sc.close()
    rows, fwd, bwd = unpack(res)
    assert [len(r[0]) for r in rows] == [len(seqs[q]) + 1 for q in sq]
    for a in (gn, ga, fwd, bwd) + tuple(res[1:4]):
        assert not np.isnan(a).any()
    assert np.array_equal(bits(fwd), bits(ga))  # one sweep: the bits of forward_pairs
    fam = np.array([specs[p][0] for p in pp])
    for f in FAMILIES:
        ix = np.nonzero(fam == f)[0]
        assert len(ix) == len(seqs) * sum(s[0] == f for s in specs)
        fn, fa = np.array([ref_f[sq[i], pp[i]][0] for i in ix]), np.array([ref_f[sq[i], pp[i]][1] for i in ix])
        wants = [ref_p[sq[i], pp[i]] for i in ix]
        # print each figure before it is asserted
        wb = worst(bwd[ix], [w[4] for w in wants])
        wr = max((float(np.max(np.abs(np.asarray(g) - np.asarray(w)))) / (want[5] + 1.0)
                  for i, want in zip(ix, wants) for g, w in zip(rows[i], want[:3])), default=0.0)
        print("device vs host twin f%d %s, %d pairs: Forward null %.3e alt %.3e, Backward alt %.3e, alt_bwd vs alt_fwd %.3e, "
              "rows %.3e of (X + 1)" % (precision, f, len(ix), worst(gn[ix], fn), worst(ga[ix], fa), wb,
                                        worst(bwd[ix], fwd[ix]), wr))
        assert within(gn[ix], fn) and within(ga[ix], fa), f
        check_against([rows[i] for i in ix], fwd[ix], bwd[ix], wants, (precision, f))  # and alt_bwd within alt_fwd's allowance
        if f == "eps0":
            for i in ix:
                if len(seqs[sq[i]]) % 3:  # no path emits the sequence in codons alone
                    assert gn[i] == NEG_INF and ga[i] == NEG_INF and fwd[i] == NEG_INF and bwd[i] == NEG_INF
                    assert not any(r.any() for r in rows[i])
                else:
                    assert np.isfinite([gn[i], ga[i], bwd[i]]).all()
        else:
            assert np.isfinite(gn[ix]).all() and np.isfinite(ga[ix]).all() and np.isfinite(bwd[ix]).all()
    for (b, e, c), a in zip(rows, fwd):
        assert e[0] == 0.0 and c[0] == 0.0
        if a == NEG_INF:
            assert not b.any() and not e.any() and not c.any()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_few_wavefronts_and_one_pairs_budget_change_no_bit(dcp, precision):
    """a 4096-node pair, a 257-node pair, a severed 1100-node pair and a 64-node pair behind one another, twice: one
    wavefront takes all wide pairs one after the other in a work area sized by the widest; three stride; rounds of one
    pair's rows"""
    specs, profs, seqs, ref_f, ref_p = chain_world(dcp, precision)
    q1, q6, q12, q40 = range(4)
    four = (index_of(specs, "delete", 4096), index_of(specs, "delete", 257), index_of(specs, "severed", 1100, 512),
            index_of(specs, "delete", 64))
    pairs = list(zip((q40, q12, q40, q6), four)) + list(zip((q6, q40, q1, q40), four))
    sq, pp = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    sc = loaded(dcp, precision, dcp.load_testhooks())
    base_f, base_p = sc.forward_pairs(sq, pp), sc.posterior_pairs(sq, pp)
    rows, fwd, bwd = unpack(base_p)
    assert within(base_f[0], [ref_f[a, b][0] for a, b in pairs]) and within(base_f[1], [ref_f[a, b][1] for a, b in pairs])
    check_against(rows, fwd, bwd, [ref_p[a, b] for a, b in pairs], precision)
    assert np.array_equal(bits(fwd), bits(base_f[1]))
    for cap in (1, 3):
        sc.test_set_forward_waves(cap)
        assert same_bits(sc.forward_pairs(sq, pp), base_f), cap
        assert same_bits(sc.posterior_pairs(sq, pp), base_p), cap
    sc.test_set_forward_waves(0)
    sc.test_set_posterior_budget(80 * (40 + 1))  # 80 bytes of records a row: a 40-nt pair's rows, no more
    assert same_bits(sc.posterior_pairs(sq, pp), base_p)
    sc.test_set_forward_waves(1)
    assert same_bits(sc.posterior_pairs(sq, pp), base_p)
    sc.close()
