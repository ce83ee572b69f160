"""viterbi64_qlane_kernel (kernel 4 on a double DB) through PACKED batch plans, in bits.

Kernel 4 runs the plan dcp_plan_query_slots makes for the scanned range's lengths: 64-query groups packed into the four
wavefront slots of a block, a slot sweeping its groups one after the other per tile, each group in its own region of
the slot's plane columns and to its own longest member.  The shapes here are the smallest at which that can go wrong:
a slot with several groups, a partial group behind another one, empty slots, more tasks than resident blocks (so
consecutive tasks of a block have different slot lists), the redo path from a group that is second in its slot,
ranged scans (which plan the range's own queries) and explicit special transitions.

Every test ASSERTS THE PLAN before it trusts the scan, twice: from dcp_plan_query_slots on the sorted lengths (its
shape: blocks, groups per slot, plane rows) and from Scanner.last_scan_query_plan after a kernel-4 scan, which must
agree with the planner on blocks, rows and plane rows.  The comparisons are test_f64_qlane.py's: as uint64 against
kernel 1 on the same context over all pairs, and against the oracle's orc_dp_tables in double on the DB's own tables
over the pairs the CPU can afford."""
import numpy as np
import pytest

from oracle_py import B_STATE, ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM
from test_f64_bits import Tables64, u64
from test_f64_edges import FLAGS, make_profiles, planted_family
from test_f64_qlane import all_pairs, check4, same_hits, scan_all
from test_f64_scan import random_params
from test_query_slots import plan

pytestmark = pytest.mark.gpu


def groups_per_slot(p):
    return np.diff(p["slot_first"].astype(np.int64)).tolist()


def slot_groups(p):
    """[[(first, n, rowbase, lmax), ...] per slot]"""
    sf = p["slot_first"]
    return [[tuple(int(v) for v in g) for g in p["groups"][sf[s]:sf[s + 1]]] for s in range(len(sf) - 1)]


def planned(dcp, sc, seqs, q_range=None, mh=True, h3=False):
    """The planner's plan of the range's lengths, and a kernel-4 scan of the range that must report that plan."""
    q0, q1 = q_range or (0, len(seqs))
    p = plan(dcp, [len(s) for s in seqs[q0:q1]])
    sc.scan(mh, h3, 10.0, keep_scores=False, q_range=q_range, kernel=dcp.KERNEL_QLANE64)
    assert sc.last_scan_kernel == dcp.KERNEL_QLANE64
    got = sc.last_scan_query_plan
    assert got == dict(nblocks=p["nb"], sum_block_rows=p["cost"], plane_rows=p["plane_rows"],
                       max_groups_per_slot=max(groups_per_slot(p))), (got, p["nb"], p["cost"], p["plane_rows"])
    return p


def sorted_position(seqs, q, q_range=None):
    """where query q stands in the (stable) length order of the range"""
    q0, q1 = q_range or (0, len(seqs))
    order = np.argsort([len(s) for s in seqs[q0:q1]], kind="stable")
    return int(np.nonzero(order == q - q0)[0][0])


def band(rng, n, lo, hi):
    lens = rng.integers(lo, hi + 1, n)
    lens[0] = hi
    return lens.tolist()


def random_seqs(rng, lens):
    return [rng.integers(0, 4, int(L), dtype=np.uint8) for L in lens]


def test_groups_share_a_slot(dcp, oracle64):
    """330 queries in six length bands: one block whose slots hold 1, 2, 2 and 1 groups, the 10-query partial group
    behind another one at plane row 44, the groups' longest members at every residue mod 5 (the ring's turns run
    0 .. 4 rows past them).  One tile, partial last tiles and every launch group; all four flag combinations."""
    rng = np.random.default_rng(330)
    lens = (band(rng, 64, 150, 205) + band(rng, 64, 36, 41) + band(rng, 64, 30, 34) + band(rng, 64, 15, 22) +
            band(rng, 64, 5, 13) + band(rng, 10, 1, 3))
    lens = [lens[i] for i in rng.permutation(len(lens))]
    seqs = random_seqs(rng, lens)
    sizes = [1, 4, 5, 9, 64, 65, 129, 257, 513]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    profs, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes],
                             [(ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2] for i in range(len(sizes))])
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    p = planned(dcp, sc, seqs)
    slots = slot_groups(p)
    assert p["nb"] == 1 and groups_per_slot(p) == [1, 2, 2, 1]
    assert sum(len(s) >= 2 for s in slots) >= 2
    partial = [(i, g) for s in slots for i, g in enumerate(s) if g[1] < 64]
    assert len(partial) == 1 and partial[0][0] == 1 and partial[0][1][1] == 10 and partial[0][1][2] == 44
    assert sorted(g[3] % 5 for s in slots for g in s) == [0, 1, 2, 3, 3, 4]  # 205, 41, 22, 3, 13, 34
    tabs = Tables64(sc, profs)
    # the oracle: the partial group, and a dozen queries of every other group
    by_len = np.argsort(lens, kind="stable")
    some = by_len[:10].tolist() + [int(q) for g0 in range(10, 330, 64) for q in rng.choice(by_len[g0:g0 + 64], 12, False)]
    for i, (mh, h3) in enumerate(FLAGS):
        check4(dcp, oracle64, sc, tabs, seqs, all_pairs(some, range(len(profs))), mh, h3, thr=(10.0, 0.0)[i % 2])
    sc.close()


def test_deeper_slots_empty_slots_and_idle_lanes(dcp, oracle64):
    """600 queries of 1-60 nt: one block with slots of 3, 3, 2 and 2 groups.  One 7-nt query: a block with three empty
    slots, which only take part in the barriers.  257 queries of one length: a second block whose only group has one
    query and 63 idle lanes."""
    rng = np.random.default_rng(2)
    sizes = [3, 37, 100, 260]
    profs, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes],
                             [ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY] * 2)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    batches = [(random_seqs(rng, np.random.default_rng(3).integers(1, 61, 600)), 1, [3, 3, 2, 2]),
               (random_seqs(rng, [7]), 1, [1, 0, 0, 0]),
               (random_seqs(rng, [33] * 257), 2, [1, 1, 1, 1, 1, 0, 0, 0])]
    for seqs, nb, gps in batches:
        sc.upload_seqs(seqs)
        p = planned(dcp, sc, seqs)
        assert p["nb"] == nb and sorted(groups_per_slot(p)[:4], reverse=True) == gps[:4], groups_per_slot(p)
        assert groups_per_slot(p)[4:] == gps[4:]
        tabs = Tables64(sc, profs)
        qs = rng.choice(len(seqs), min(len(seqs), 40), replace=False).tolist()
        for mh in (True, False):
            check4(dcp, oracle64, sc, tabs, seqs, all_pairs(qs, range(len(sizes))), mh, False, thr=0.0)
    sc.close()


class SomeTables64(Tables64):
    """Tables64 of a few resident profiles only"""

    def __init__(self, sc, profiles, which):
        self.t = [None] * len(profiles)
        for p in which:
            ei, en = sc.insert_null_tables64(p)
            self.t[p] = (profiles[p].parts64()[0], sc.match_table(p), ei, en)


def test_more_tasks_than_resident_blocks(dcp, oracle64):
    """600 profiles of 1-12 nodes x 700 queries of 1-60 nt in two plan blocks: 1 200 tasks for a grid of at most 512
    blocks, so a block runs tasks of both plan blocks, with different slot lists, one after the other."""
    rng = np.random.default_rng(1)
    ndist, nprof = 40, 600
    sizes = list(range(1, 13)) + rng.integers(1, 13, ndist - 12).tolist()
    base, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes],
                            [(ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY)[i % 2] for i in range(ndist)])
    of = rng.permutation(np.arange(nprof) % ndist)
    profs = [base[i] for i in of]
    seqs = random_seqs(rng, np.random.default_rng(1).integers(1, 61, 700))
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    p = planned(dcp, sc, seqs)
    assert p["nb"] == 2 and nprof * p["nb"] > 512
    assert groups_per_slot(p)[:4] != groups_per_slot(p)[4:] and max(groups_per_slot(p)) >= 2
    ps = rng.choice(nprof, 12, replace=False).tolist()
    tabs = SomeTables64(sc, profs, ps)
    qs = rng.choice(len(seqs), 60, replace=False).tolist()
    check4(dcp, oracle64, sc, tabs, seqs, all_pairs(qs, ps), True, False, thr=0.0)
    sc.close()


def planted_batch(oracle64, rng):
    """Planted multi-copy queries of a 10-node profile in the bands of a batch like test_groups_share_a_slot's, ten
    times as long, and those of the 257-node family in the long band.  Returns (seqs, own pairs, feedback pairs,
    the index of the 10-node family's k = 2 back-to-back query)."""
    fams = [planted_family(oracle64, M) for M in (10, 257)]
    bands = [(600, 4750), (340, 430), (230, 300), (140, 215), (60, 125)]
    members = [[] for _ in bands]
    for p, f in enumerate(fams):
        for k, spaced, s in f[2]:
            b = next(i for i, (lo, hi) in enumerate(bands) if lo <= len(s) <= hi)
            members[b].append((s, p, k, spaced))
    seqs = []
    for (lo, hi), m in zip(bands, members):
        top = min(hi, 1000)  # the random members of the long band stay short: the oracle scores some of them
        fill = random_seqs(rng, [top] + rng.integers(lo, top + 1, 64 - len(m) - 1).tolist())
        seqs += m + [(s, None, 0, False) for s in fill]
    seqs += [(s, None, 0, False) for s in random_seqs(rng, rng.integers(1, 31, 10))]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    own = [(q, p) for q, (_, p, _, _) in enumerate(seqs) if p is not None]
    k2 = next(q for q, (_, p, k, spaced) in enumerate(seqs) if p == 0 and k == 2 and not spaced)
    seqs = [s for s, _, _, _ in seqs]
    feedback = []
    for q, p in own:  # the premise, on the oracle's own best path (CPU)
        fams[p][1].setup(len(seqs[q]), True, False)
        rc, ll, path = fams[p][1].viterbi(1, bytes(seqs[q]))
        assert rc == 0 and np.isfinite(ll)
        if [s for s, _ in path].count(B_STATE) > 1:
            feedback.append((q, p))
    assert len(feedback) == 16  # k = 2 .. 5, back to back and spaced, of both families
    return fams, seqs, own, feedback, k2


def test_redo_from_a_shared_slot(dcp, oracle64):
    """Pairs whose best path re-enters B leave through the redo lists from wherever their group stands: the 10-node
    family's k = 2 query sits in a group that is SECOND in its slot, the 257-node family's queries in the long group
    that has a slot to itself.  Then the lists capped at three pairs (test-hooks build): the scan is repeated with the
    row sweep, and that scan has no plan."""
    rng = np.random.default_rng(410)
    fams, seqs, own, feedback, k2 = planted_batch(oracle64, rng)
    profs, _ = make_profiles(dcp, oracle64, [f[0] for f in fams], [ENTRY_DIST_OCCUPANCY] * 2)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    p = planned(dcp, sc, seqs)
    slots = slot_groups(p)
    assert p["nb"] == 1 and sorted(groups_per_slot(p)) == [1, 1, 2, 2]
    assert (k2, 0) in feedback
    at = sorted_position(seqs, k2)
    second = [g for s in slots for g in s[1:]]
    assert any(first <= at < first + n and rowbase > 0 for first, n, rowbase, _ in second), (at, slots)
    long_group = [s for s in slots if len(s) == 1 and s[0][3] > 3000]
    assert len(long_group) == 1
    for q, pr in own:
        if pr == 1:
            assert long_group[0][0][0] <= sorted_position(seqs, q) < long_group[0][0][0] + 64
    tabs = Tables64(sc, profs)
    short = [q for q, s in enumerate(seqs) if len(s) <= 215]
    opairs = sorted(set(own) | {(q, 0) for q, _ in own} | set(all_pairs(rng.choice(short, 40, False).tolist(), range(2))))
    npairs = len(seqs) * len(profs)
    for mh, h3 in ((True, False), (True, True)):
        redo, gn, ga = check4(dcp, oracle64, sc, tabs, seqs, opairs, mh, h3)
        assert 0 < redo < npairs, redo
        if not h3:
            assert redo >= len(feedback)
            for q, pr in own:
                assert -2 * (gn[q, pr] - ga[q, pr]) > 10.0
    sc.close()

    hk = dcp.Scanner(0, lib=dcp.load_testhooks())
    hk.upload_db(profs)
    hk.upload_seqs(seqs)
    rn, ra, rh = scan_all(hk, dcp.KERNEL_ROWSWEEP, True, False)
    hk.test_set_redo_cap(3)
    on, oa, oh = scan_all(hk, dcp.KERNEL_QLANE64, True, False)
    assert hk.last_scan_kernel == dcp.KERNEL_ROWSWEEP
    with pytest.raises(dcp.DcpError) as e:
        hk.last_scan_query_plan
    assert e.value.rc == dcp.RC_EINVAL
    assert np.array_equal(u64(on), u64(rn)) and np.array_equal(u64(oa), u64(ra)) and same_hits(oh, rh)
    hk.test_set_redo_cap(0)
    n2, a2, h2 = scan_all(hk, dcp.KERNEL_QLANE64, True, False)
    assert hk.last_scan_kernel == dcp.KERNEL_QLANE64 and hk.last_scan_query_plan["nblocks"] == 1
    assert np.array_equal(u64(n2), u64(rn)) and np.array_equal(u64(a2), u64(ra)) and same_hits(h2, rh)
    hk.close()


def test_ranged_scans_and_explicit_transitions(dcp, oracle64):
    """A resident batch of 1 000 queries of 1-120 nt: a ranged scan plans the RANGE's own queries -- (100, 700) as two
    blocks with shared slots -- and gives the full scan's bits.  Explicit special transitions in double, equal to the
    flag-derived rows and the LOG1 rows (all zero: N, E and J tie into B): kernel 1's bits."""
    rng = np.random.default_rng(4)
    lens = np.where(rng.random(1000) < 0.5, rng.integers(100, 121, 1000), rng.integers(1, 121, 1000))
    seqs = random_seqs(np.random.default_rng(44), lens)
    sizes = [3, 37, 100, 260]
    profs, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in sizes],
                             [ENTRY_DIST_UNIFORM, ENTRY_DIST_OCCUPANCY] * 2)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    tabs = Tables64(sc, profs)
    full = planned(dcp, sc, seqs)
    gn, ga, h = scan_all(sc, dcp.KERNEL_QLANE64, True, False, 0.0)
    ranges = ((100, 700), (0, 257), (999, 1000))
    for r in ranges:
        p = planned(dcp, sc, seqs, q_range=r)
        assert (p["nb"], p["cost"]) != (full["nb"], full["cost"])
        if r == (100, 700):
            assert p["nb"] == 2 and max(groups_per_slot(p)) >= 2
        qs = rng.choice(np.arange(*r), min(r[1] - r[0], 25), replace=False).tolist()
        _, n1, a1 = check4(dcp, oracle64, sc, tabs, seqs, all_pairs(qs, range(len(sizes))), True, False, thr=0.0, q_range=r)
        assert np.array_equal(u64(n1[r[0]:r[1]]), u64(gn[r[0]:r[1]])) and np.array_equal(u64(a1[r[0]:r[1]]), u64(ga[r[0]:r[1]]))
    # explicit rows equal to the flag-derived ones: check4 (the oracle derives them from the flags), the flag unset
    r = (100, 700)
    sc.set_xtrans64(np.stack([dcp.xtrans64(len(s), True, False) for s in seqs]))
    planned(dcp, sc, seqs, q_range=r, mh=False)
    gn4, ga4, h4 = scan_all(sc, dcp.KERNEL_QLANE64, False, False, 0.0, q_range=r)
    gn1, ga1, h1 = scan_all(sc, dcp.KERNEL_ROWSWEEP, False, False, 0.0, q_range=r)
    assert np.array_equal(u64(gn4[r[0]:r[1]]), u64(gn1[r[0]:r[1]])) and np.array_equal(u64(ga4[r[0]:r[1]]), u64(ga1[r[0]:r[1]]))
    assert np.array_equal(u64(gn4[r[0]:r[1]]), u64(gn[r[0]:r[1]])) and np.array_equal(u64(ga4[r[0]:r[1]]), u64(ga[r[0]:r[1]]))
    assert same_hits(h4, h1)
    sc.set_xtrans64(np.zeros((len(seqs), 13)))
    planned(dcp, sc, seqs, q_range=r)
    gn4, ga4, h4 = scan_all(sc, dcp.KERNEL_QLANE64, True, False, 0.0, q_range=r)
    assert sc.last_scan_redo_pairs > 0  # E -> B and J -> B are free
    gn1, ga1, h1 = scan_all(sc, dcp.KERNEL_ROWSWEEP, True, False, 0.0, q_range=r)
    assert np.array_equal(u64(gn4[r[0]:r[1]]), u64(gn1[r[0]:r[1]])) and np.array_equal(u64(ga4[r[0]:r[1]]), u64(ga1[r[0]:r[1]]))
    assert same_hits(h4, h1)
    sc.close()


def test_last_scan_query_plan(dcp, oracle64):
    """The accessor: DCP_EINVAL before the first scan, after a kernel-1 scan and on a float DB; a uniform batch of
    1 000 queries of 300 nt plans as before the packing -- four blocks, one group per slot."""
    def einval(sc):
        with pytest.raises(dcp.DcpError) as e:
            sc.last_scan_query_plan
        assert e.value.rc == dcp.RC_EINVAL

    rng = np.random.default_rng(6)
    sc = dcp.Scanner(0)
    sc.upload_db([dcp.ProteinProfile.sample(3, 40)])
    sc.upload_seqs(["ACGTACGTACGTAAAGGG", "GATTACA"])
    einval(sc)
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_QLANE)
    einval(sc)
    sc.close()

    profs, _ = make_profiles(dcp, oracle64, [random_params(rng, M) for M in (5, 70)], [ENTRY_DIST_OCCUPANCY] * 2)
    seqs = random_seqs(rng, [300] * 1000)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    einval(sc)
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    einval(sc)
    sc.scan(True, False, 10.0)  # kernel 0 on a double DB is the row sweep
    assert sc.last_scan_kernel == dcp.KERNEL_ROWSWEEP
    einval(sc)
    p = planned(dcp, sc, seqs)
    assert p["nb"] == 4 and groups_per_slot(p) == [1] * 16
    assert sc.last_scan_query_plan == dict(nblocks=4, sum_block_rows=4 * 310, plane_rows=310, max_groups_per_slot=1)
    rn, ra, rh = scan_all(sc, dcp.KERNEL_ROWSWEEP, True, False)
    einval(sc)
    gn, ga, h = scan_all(sc, dcp.KERNEL_QLANE64, True, False)
    assert np.array_equal(u64(gn), u64(rn)) and np.array_equal(u64(ga), u64(ra)) and same_hits(h, rh)
    sc.close()
