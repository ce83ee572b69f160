"""The three query-lane kernels (viterbi_qlane_kernel, viterbi_qlane2_kernel, viterbi_qlane_w3_kernel) at their
structural edges, one family of cases per edge (runs on a real MI355X).

Every case goes through ONE helper (check_case), so none is weaker than another: for every scoring mode of the case and
for KERNEL_QLANE (the three-wavefront kernel up to 64 queries, the 256-lane single-stage kernel above) and KERNEL_QLANE2
(two stages), `null` and `alt` of EVERY pair equal the oracle's float32 recursion fed the device's own tables
(test_gpu_parity.oracle_dp_on_product_tables) as uint32, and the hit list equals the reference's filter on those scores
(isfinite(lrt) and not lrt < thr, lrt = float32(-2) * (null - alt)) record for record, scores in bits.  The threshold
is the median of the oracle's finite LRTs, so about half of a case's pairs are published as hits.  Nothing is sampled.
(Queries -- or profiles -- that are copies of one another are scored once by the oracle; that they are copies, and
that a copied profile's device table is its source's, is asserted.)

Where a case depends on how the batch is packed, the plan is asserted first (test_qlane_edge_plans: the same
assertions run on the CPU).

edge (dcp_qlane.hip / dcp_gpu.hip)                                   reached by
  Lwave = 1, 2, 3 < kRingSkew (consumer start of the LDS ring)       B (plan: one group, lmax = Lwave), C short_behind_long
  Lwave mod 5, Lwave < 5 (remainder rows, 5-slot history)            B: Lwave = 1 .. 45
  16-row ring: wrap, producer back-pressure                          B: Lwave = 15, 16, 17, 31, 32, 33, 79 .. 81, 159 .. 161
  rowbase != 0, every even residue mod 16                            C (plan: long_alone has all eight)
  lane L << Lwave (results captured at row L, `at_end`)              B mixed (a lane of 1 nt in every group), D
  park row rowbase + Lwave + 8, the next group's region              C (groups packed back to back), T = 2, 3, 4, 13
  tiles T = 1 .. 5 and many, M mod 8 = 1 .. 7                        A: M = 1 .. 34, 39 .. 41, ... 4096
  two-stage: T = 1, T = 2, odd T (final_stage, idle stage)           A, B (T = 1, 2, 3, 4), C (T = 13)
  nq = 1, 63, 64, 65, ... lanes without a query, empty slots         D (plan: partial group, slots with g0 == g1)
  w3 with 1, 2, 3, 4 tasks (idle slots of a 3-slot block)            D: 1 .. 4 profiles x nq <= 64
  tasks > resident blocks (a block's second task)                    E
  one-layout DB (stage_tile_image<G, true>) at the tile edges        F = A's DB in an order of its own, one_layout
  window extremes AAAAA / TTTTT (largest gather offsets, code 1363)  A's queries
  uni-hit with hmmer3_compat                                         every family's modes include (False, True)
"""
import numpy as np
import pytest
import torch  # before the product's library: both bring a HIP runtime, and torch must see the device too

import test_gpu_parity as tp
import test_qlane_edge_plans as pl
from oracle_py import ENTRY_DIST_OCCUPANCY, ENTRY_DIST_UNIFORM
from test_query_slots import plan

pytestmark = pytest.mark.gpu

MODES4 = [(True, False), (False, False), (True, True), (False, True)]
MODES2 = [(True, False), (False, True)]
PAIRS = {}  # family -> pairs compared against the oracle (per kernel scan), printed per test


@pytest.fixture(scope="module")
def scanner(dcp):
    s = dcp.Scanner(0)
    yield s
    s.close()


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def first_copies(seqs):
    """src[i] = index of the first query identical to query i."""
    seen, src = {}, []
    for i, s in enumerate(seqs):
        src.append(seen.setdefault(bytes(s), i))
    return np.array(src)


def where(dcp, seqs, profiles, q0, q1, kernel, mode, q, p):
    """What the helper's assertion messages name: kernel, mode, profile size, query, the query's group (Lwave, rowbase)."""
    lens = np.array([len(s) for s in seqs[q0:q1]], np.uint32)
    slots = 1 if (kernel == dcp.KERNEL_QLANE and q1 - q0 <= 64) else 4
    pn = plan(dcp, lens, slots)
    pos = int(np.nonzero(np.argsort(lens, kind="stable") == q - q0)[0][0])
    g = [g for g in pn["groups"] if g[0] <= pos < g[0] + g[1]][0]
    name = {dcp.KERNEL_QLANE: "qlane" + ("(w3)" if slots == 1 else ""), dcp.KERNEL_QLANE2: "qlane2"}[kernel]
    return "kernel %s (multi, h3) = %s profile %d (M = %d) query %d (L = %d) lane %d of a group with Lwave = %d at rowbase %d" % (
        name, mode, p, profiles[p].core_size, q, len(seqs[q]), pos - int(g[0]), int(g[3]), int(g[2]))


def oracle_for(dcp, oracle32, scanner, profiles, seqs, mode, on_host, xt, prof_src, cache):
    """[nseq, nprof] null / alt of the oracle on the device's tables; distinct queries x distinct profiles are scored."""
    nprof = len(profiles)
    prof_src = np.arange(nprof) if prof_src is None else np.asarray(prof_src)
    up = np.unique(prof_src)
    assert np.array_equal(up, np.arange(len(up)))  # the sources come first in the caller's order
    tables = {}
    for p in np.nonzero(prof_src != np.arange(nprof))[0]:  # a copy's device table is its source's
        s = int(prof_src[p])
        if s not in tables:
            tables[s] = u32(scanner.match_table(s))
        assert np.array_equal(u32(scanner.match_table(int(p))), tables[s]), (p, s)
    uprofs = [profiles[p] for p in up]
    if xt is not None:
        on = np.zeros((len(seqs), len(up)), np.float32)
        oa = np.zeros_like(on)
        for p, prof in enumerate(uprofs):
            em = scanner.match_table(p)
            eps = tp.prof_eps[id(prof)]
            ei = dcp.frame_table_host(prof.insert_dist, eps)
            en = dcp.frame_table_host(prof.null_dist, eps)
            for q, s in enumerate(seqs):
                rc, on[q, p], oa[q, p] = oracle32.dp_tables(prof.trans8, em, ei, en, xt[q], bytes(s))
                assert rc == 0
        return on[:, prof_src], oa[:, prof_src]
    rows = cache.setdefault(mode, {})
    new = [seqs[i] for i in np.unique(first_copies(seqs)) if bytes(seqs[i]) not in rows]
    if new:
        n, a = tp.oracle_dp_on_product_tables(dcp, oracle32, scanner, uprofs, new, mode[0], mode[1], on_host)
        for i, s in enumerate(new):
            rows[bytes(s)] = (n[i], a[i])
    on = np.stack([rows[bytes(s)][0] for s in seqs])
    oa = np.stack([rows[bytes(s)][1] for s in seqs])
    return on[:, prof_src], oa[:, prof_src]


def check_case(dcp, oracle32, scanner, family, profiles, batches, modes, on_host, one_layout=False, xt=None, prof_src=None,
               q_range=None, want_redo=None):
    """The one check of this file (module docstring).  batches: lists of queries scanned in turn against one upload of
    the DB (the oracle scores each distinct query once); xt: explicit special transitions [nseq, 13] of the single batch;
    q_range: scan that range only.  Returns {(batch, mode, kernel): (null, alt, hits)}."""
    scanner.upload_db(profiles, expand_on_host=on_host, one_layout=one_layout)
    assert scanner.one_layout == one_layout
    out, cache = {}, {}
    sum_m = sum(p.core_size for p in profiles)
    for b, seqs in enumerate(batches):
        scanner.upload_seqs(seqs)
        if xt is not None:
            assert len(batches) == 1
            scanner.set_xtrans(xt)
        q0, q1 = q_range or (0, len(seqs))
        for mode in modes:
            on, oa = oracle_for(dcp, oracle32, scanner, profiles, seqs, mode, on_host, xt, prof_src, cache)
            with np.errstate(invalid="ignore"):
                lrt = np.float32(-2) * (on - oa)
            fin = np.isfinite(lrt[q0:q1])
            thr = np.sort(lrt[q0:q1][fin])[fin.sum() // 2] if fin.any() else np.float32(0)
            with np.errstate(invalid="ignore"):
                hit = np.isfinite(lrt) & ~(lrt < thr)
            hit[:q0], hit[q1:] = False, False
            wq, wp = np.nonzero(hit)  # row-major: sorted by (seq_idx, profile_idx) like dcp_gpu_fetch_hits
            for kernel in (dcp.KERNEL_QLANE, dcp.KERNEL_QLANE2):
                scanner.scan(mode[0], mode[1], float(thr), keep_scores=True, kernel=kernel, q_range=q_range)
                assert scanner.last_scan_kernel == kernel
                infos = scanner.launch_infos()
                assert infos[0]["W"] == 0 and infos[0]["cells"] == sum_m * sum(len(s) for s in seqs[q0:q1])
                assert all(li["cells"] == 0 for li in infos[1:])
                gn, ga = scanner.scores()
                bad = np.argwhere((u32(gn[q0:q1]) != u32(on[q0:q1])) | (u32(ga[q0:q1]) != u32(oa[q0:q1])))
                if len(bad):
                    q, p = int(bad[0][0]) + q0, int(bad[0][1])
                    raise AssertionError("%s batch %d: %d of %d pairs differ; first: %s: device null %r alt %r, oracle %r %r" % (
                        family, b, len(bad), (q1 - q0) * len(profiles), where(dcp, seqs, profiles, q0, q1, kernel, mode, q, p),
                        gn[q, p], ga[q, p], on[q, p], oa[q, p]))
                hits = scanner.hits()
                same = len(hits) == len(wq) and np.array_equal(hits["seq_idx"], wq) and np.array_equal(hits["profile_idx"], wp) \
                    and np.array_equal(u32(hits["null_loglik"]), u32(on[wq, wp])) and np.array_equal(u32(hits["alt_loglik"]), u32(oa[wq, wp]))
                if not same:
                    got = {(int(h["seq_idx"]), int(h["profile_idx"])) for h in hits}
                    diff = sorted(got ^ set(zip(wq.tolist(), wp.tolist())))
                    q, p = diff[0] if diff else (int(hits["seq_idx"][0]), int(hits["profile_idx"][0]))
                    raise AssertionError("%s batch %d: hit list differs (%d records, %d wanted, threshold %r); first: %s" % (
                        family, b, len(hits), len(wq), thr, where(dcp, seqs, profiles, q0, q1, kernel, mode, q, p)))
                if want_redo is not None:
                    assert want_redo(scanner.last_scan_redo_pairs, mode), (family, b, mode, scanner.last_scan_redo_pairs)
                out[(b, mode, kernel)] = (gn[q0:q1].copy(), ga[q0:q1].copy(), hits.copy())
            PAIRS[family] = PAIRS.get(family, 0) + (q1 - q0) * len(profiles)
    print("%s: %d pairs per kernel against the oracle so far" % (family, PAIRS[family]))
    return out


def pfam_profiles(dcp, rng, sizes):
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)
    params = [tp.pfam_like_params(rng, M) for M in sizes]
    profiles = [dcp.ProteinProfile.from_params(*prm, cfg) for prm in params]
    for p in profiles:
        tp.prof_eps[id(p)] = cfg.epsilon
    return profiles, params


def rand_of(rng, lens):
    return [rng.integers(0, 4, int(L), dtype=np.uint8) for L in lens]


# ---- A: tiles, F: one layout, G: modes ---------------------------------------------------------------------------
A_SIZES = list(range(1, 35)) + [39, 40, 41, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096]
A_SAMPLED = (3, 7, 24, 64, 129, 1025)  # ProteinProfile.sample with uniform entry; the others pfam_like_params
A_PLANTED = (8, 9, 16, 17, 257)
A_LENGTHS = list(range(1, 13)) + [15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 100]
_family_a = {}


def family_a(dcp, oracle32):
    if _family_a:
        return _family_a["v"]
    rng = np.random.default_rng(8101)
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)
    profiles, oprofs = [], {}
    for M in A_SIZES:
        if M in A_SAMPLED:
            profiles += tp.make_profiles(dcp, [(8100 + M, M, ENTRY_DIST_UNIFORM, 0.01)])
            continue
        prm = tp.pfam_like_params(rng, M)
        profiles.append(dcp.ProteinProfile.from_params(*prm, cfg))
        tp.prof_eps[id(profiles[-1])] = cfg.epsilon
        if M in A_PLANTED:
            oprofs[M] = oracle32.new(*prm, ENTRY_DIST_OCCUPANCY, 0.01)
    seqs = rand_of(rng, A_LENGTHS)
    for M in A_PLANTED:  # two one-domain and two two-domain queries: redo lists and the dirty flag at tile edges
        one = lambda: tp.planted_query(rng, oprofs[M], M, flank=3)
        seqs += [one(), one(), np.concatenate([one(), one()]), np.concatenate([one(), one()])]
    seqs += [np.zeros(33, np.uint8), np.full(33, 3, np.uint8), np.tile(np.arange(4, dtype=np.uint8), 9)[:33]]
    assert len(seqs) <= 64
    twice = seqs + [seqs[i] for i in rng.permutation(len(seqs))]  # past 64: KERNEL_QLANE runs its 256-lane kernel
    assert len(twice) > 64
    # F: a caller order of its own in which profiles of M mod 8 != 0 are neighbours
    order = rng.permutation(len(A_SIZES))
    ms = np.array(A_SIZES)[order]
    assert ((ms[:-1] % 8 != 0) & (ms[1:] % 8 != 0)).sum() >= 20
    _family_a["v"] = (profiles, seqs, twice, order)
    return _family_a["v"]


@pytest.mark.parametrize("mode", MODES4 + ["xtrans"], ids=lambda m: m if isinstance(m, str) else "multi%d-h3%d" % m)
def test_a_tiles_and_f_one_layout(dcp, oracle32, scanner, mode):
    """A: M = 1 .. 34, 39 .. 41 and both sides of 64 .. 4096 (every M mod 8; T = 1 .. 5 and many, both parities: FIRST &&
    LAST, the two-stage kernel's T = 1 where stage 1 never sweeps, T = 2, odd T with an idle stage in the last step and
    `final_stage`; every redo size class) against queries of 1 .. 12, 15 .. 18, 31 .. 33, 47 .. 49, 100 nt, planted one- and
    two-domain queries (redo lists, `dirty` at tile edges), AAAAA / TTTTT (window extremes: the largest gather offsets,
    code 1363 the last row of a tile image) and (ACGT)^n; once as a batch of at most 64 queries (w3 under KERNEL_QLANE)
    and once replicated past 64.  F: the same DB in another caller order, one_layout (stage_tile_image<G, true> gathers a
    last, partial tile next to a neighbour's first columns): the oracle's bits again, and the two-layout scan's.
    G: all four (multi, h3), and explicit special transitions with E -> B free, which keep the redo path on in a
    uni-hit scan."""
    profiles, seqs, twice, order = family_a(dcp, oracle32)
    if mode == "xtrans":
        xt = np.stack([dcp.xtrans(len(s), True, False) for s in seqs])
        xt[:, 9] = 0.0  # E -> B for free: every pair re-enters the core
        modes, batches = [(False, False)], [seqs]
        redo = lambda n, m: n > 0
    else:
        xt, modes, batches = None, [mode], [seqs, twice]
        redo = lambda n, m: (n >= len(A_PLANTED)) if m[0] else n == 0
    on_host = mode in ((True, False), (True, True))
    two = check_case(dcp, oracle32, scanner, "A", profiles, batches, modes, on_host, xt=xt, want_redo=redo)
    one = check_case(dcp, oracle32, scanner, "F", [profiles[i] for i in order], batches, modes, on_host, one_layout=True, xt=xt,
                     want_redo=redo)
    inv = np.argsort(order)
    for key, (n, a, h) in one.items():
        assert np.array_equal(u32(n[:, inv]), u32(two[key][0])) and np.array_equal(u32(a[:, inv]), u32(two[key][1])), key
        assert len(h) == len(two[key][2])


# ---- B: the rows of a group --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES4, ids=lambda m: "multi%d-h3%d" % m)
def test_b_rows_of_a_group(dcp, oracle32, scanner, mode):
    """Lwave = 1, 2, 3 (< kRingSkew: need0 = rowbase + min(Lwave, kRingSkew)), every Lwave mod 5 from 1 on (the four
    guarded remainder rows, the 5-slot register history), 15 .. 17, 31 .. 33 and on (the 16-row ring's wrap, slot
    (row - 1) % 16, the producer held back at last > seen + kRD) -- asserted from the plan: one group per slot whose
    lmax is the case's Lwave.  Batches of exactly 64 (one wavefront) and 128 queries, all of Lwave nt, then with lane i
    of 1 + i % Lwave nt, longest last: lanes far past their own length, results captured at row L (`at_end`).
    Profiles of 5, 12, 20, 29 nodes: T = 1, 2, 3, 4."""
    rng = np.random.default_rng(8200)
    profiles, _ = pfam_profiles(dcp, rng, pl.B_CORE_SIZES)
    for Lwave in pl.B_LWAVES:
        batches = []
        for mixed in (False, True):
            big = rand_of(rng, pl.b_lens(Lwave, 128, mixed))
            small = big[:63] + [big[127]] if mixed else big[:64]
            assert [len(s) for s in small] == pl.b_lens(Lwave, 64, mixed).tolist()
            batches += [small, big]
            pl.assert_b_plan(dcp, Lwave, 64, mixed, 1)
            pl.assert_b_plan(dcp, Lwave, 64, mixed, 4)
            pl.assert_b_plan(dcp, Lwave, 128, mixed, 4)
        check_case(dcp, oracle32, scanner, "B", profiles, batches, [mode], on_host=bool(Lwave % 2))


# ---- C: groups sharing a slot ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES2, ids=lambda m: "multi%d-h3%d" % m)
@pytest.mark.parametrize("name", list(pl.C_BATCHES) + ["ranged"])
def test_c_groups_sharing_a_slot(dcp, oracle32, scanner, name, mode):
    """rowbase != 0 (ring slots and flags count PLANE rows, rowbase + j; `off` starts at rowbase * NT; the park row
    rowbase + Lwave + 8 lies below the next group's region): batches whose plan -- asserted -- has one to eight groups
    per slot, every even rowbase residue mod 16, a long group alone in its slot next to slots of many short ones, groups
    of Lwave 1, 2, 3 swept behind a long group of their slot; and a ranged scan, which re-plans for its own queries.
    T = 1, 2, 3, 4, 13."""
    rng = np.random.default_rng(8300)
    profiles, _ = pfam_profiles(dcp, rng, pl.C_CORE_SIZES)
    q_range = None
    if name == "ranged":
        name, q0, q1 = pl.C_RANGE
        q_range = (q0, q1)
        pl.assert_c_plan(dcp, pl.c_lens(name)[q0:q1], pl.C_RANGE_SHAPE)
    pl.assert_c_plan(dcp, pl.c_lens(name), pl.C_SHAPES[name])
    seqs = rand_of(rng, pl.c_lens(name))
    check_case(dcp, oracle32, scanner, "C", profiles, [seqs], [mode], on_host=not mode[0], q_range=q_range)


# ---- D: fill -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES2, ids=lambda m: "multi%d-h3%d" % m)
def test_d_fill(dcp, oracle32, scanner, mode):
    """nq = 1, 2, 63, 64, 65 .. 513 queries of 1 .. 60 nt: lanes without a query (g.has), the partial group holding the
    shortest queries, slots without a group (g0 == g1) -- asserted from the plan -- against 1, 2, 3 and 4 profiles: under
    KERNEL_QLANE with nq <= 64 that is the three-wavefront kernel with fewer tasks than a block's three slots, as many,
    and one more (nblocks = (nblocks + 2) / 3 * 3: idle slots, scratch sized per slot)."""
    rng = np.random.default_rng(8400)
    profiles, _ = pfam_profiles(dcp, rng, (3, 8, 9, 21))
    pool = rand_of(rng, pl.D_POOL)
    for nq in pl.D_NQ:
        pl.assert_d_plan(dcp, nq)
    for k in (1, 2, 3, 4):
        check_case(dcp, oracle32, scanner, "D", profiles[:k], [pool[:nq] for nq in pl.D_NQ], [mode], on_host=bool(k % 2))


# ---- E: more tasks than resident blocks ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES2, ids=lambda m: "multi%d-h3%d" % m)
def test_e_more_tasks_than_resident_blocks(dcp, oracle32, scanner, mode):
    """A scan has nprof x (blocks of the plan) tasks, pulled from task_counter by a persistent grid of 3 x num_cus
    three-wavefront slots, 2 x num_cus single-stage or num_cus two-stage blocks: with 3 x num_cus + 7 profiles of 1 .. 16
    nodes (sizes in random caller order: tasks are handed out biggest first) x 64 queries (w3, two-stage) and x 300
    queries (two blocks per profile; single-stage, two-stage) blocks take a second and third task and reuse their LDS,
    planes and ring flags."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(8500)
    sizes = rng.permutation(np.repeat(np.arange(1, 17), 2))
    base, _ = pfam_profiles(dcp, rng, [int(m) for m in sizes])
    nprof = 3 * cus + 7
    src = np.concatenate([np.arange(len(base)), rng.integers(0, len(base), nprof - len(base))])
    profiles = [base[i] for i in src]
    batches = [rand_of(rng, pl.e_lens(64)), rand_of(rng, pl.e_lens(300))]
    for nq, slots, resident in ((64, 1, 3 * cus), (64, 4, cus), (300, 4, 2 * cus), (300, 4, cus)):
        assert nprof * pl.assert_e_plan(dcp, nq, slots)["nb"] > resident
    assert 2 * nprof > 3 * cus  # the two-stage grid's blocks take a third task
    check_case(dcp, oracle32, scanner, "E", profiles, batches, [mode], on_host=mode[0], prof_src=src)
