"""Domains: domains_kernel (csrc/dcp_domains.hip) behind dcp_gpu_path_domains / ...64 and Scanner.path_domains, and the
whole way from a cut batch to merged genes.

The reference of every number is `restate` below: the three sums of include/dcp_gpu.h in numpy scalars of the DB's
precision, one step after the other, and the record fields, on the tables the device itself holds (Scanner.match_table,
the profile's trans8, frame_table_host of its insert and null dists; for a double DB insert_null_tables64 and
parts64).  Everything is compared in bits.

CPU (premises; they use the restatements alone and pass without the feature):
  * the restatement's total is orc_path_score_tables, bit for bit, on the oracle's own paths and tables;
  * the planted world of tests/test_seq_windows.py, cut 2 048 / 1 024 on both strands, gives seven domains of which
    three survive the merge by odds -- and the wrong ones survive a merge by the raw core score.
GPU:
  1. parity on Viterbi paths over every table layout (rows shared four and two at a time, the one-wavefront classes, a
     multi-wavefront class, a one-layout DB; in double both sides of a segment), with M, I, D steps, frame shifts, one
     and two domains, null paths;
  2. hand-made paths whose B and E fall on the edges of the kernel's 64-step trips, a domain over three trips,
     fragments that straddle a 16-base word;
  3. explicit special transitions, a second call after a new upload;
  4. the refusals, each with its message, the outputs untouched and the last scan's bits as they were;
  5. end to end in the planted world: upload, cut, reverse strand, scan, hits, trace, domains, locate, merge."""
import ctypes as C

import numpy as np
import pytest

from oracle_py import (B_STATE, C_STATE, E_STATE, ENTRY_DIST_OCCUPANCY, J_STATE, N_STATE, R_STATE, S_STATE,
                       T_STATE)
from test_both_strands import bits, np_revcomp, oracle_lrt
from test_domains_merge import py_locate, py_merge
from test_gpu_parity import pfam_like_params, planted_query
from test_seq_windows import PLANT_L, PLANT_STEP, PLANT_WINDOW, hand_cut, planted_world, py_starts

PRECISIONS = (32, 64)
WORD_OFF = (0, 4, 20, 84, 340)
FIELDS = ("path", "step_begin", "step_end", "seq_begin", "seq_end", "node_first", "node_last", "n_match", "n_insert",
          "n_delete", "n_shift", "reserved")
# rows of trans8 (csrc/dcp_host.h) and of the 13 special transitions
T_ENTRY, T_MM, T_IM, T_DM, T_MD, T_DD, T_MI, T_II = range(8)
X_RR, X_SB, X_SN, X_NN, X_NB, X_ET, X_EC, X_CC, X_CT, X_EB, X_EJ, X_JJ, X_JB = range(13)


def M_(k):
    return k


def I_(k):
    return (1 << 14) | k


def D_(k):
    return (2 << 14) | k


def edge(t8, xt, prev, cur):
    """The transition prev -> cur as the loop of orc_path_score_tables takes it (oracle/oracle.c), None if the model
    graph has no such edge."""
    pkind, pk, kind, x = prev >> 14, prev & 0x3FFF, cur >> 14, cur & 0x3FFF
    k = x - 1
    if kind == 0:
        if prev == B_STATE:
            return t8[T_ENTRY, k]
        if k > 0 and pk == k and pkind < 3:
            return t8[(T_MM, T_IM, T_DM)[pkind], k]
        return None
    if kind == 1:
        return t8[(T_MI, T_II)[pkind], k] if pk == k + 1 and pkind < 2 else None
    if kind == 2:
        return t8[T_MD if pkind == 0 else T_DD, k] if k > 0 and pk == k and pkind in (0, 2) else None
    if cur == E_STATE:
        return t8.dtype.type(0) if pkind == 0 or (pkind == 2 and pk >= 2) else None
    row = {(R_STATE, R_STATE): X_RR, (S_STATE, N_STATE): X_SN, (N_STATE, N_STATE): X_NN, (S_STATE, B_STATE): X_SB,
           (N_STATE, B_STATE): X_NB, (E_STATE, B_STATE): X_EB, (J_STATE, B_STATE): X_JB, (E_STATE, J_STATE): X_EJ,
           (J_STATE, J_STATE): X_JJ, (E_STATE, C_STATE): X_EC, (C_STATE, C_STATE): X_CC, (E_STATE, T_STATE): X_ET,
           (C_STATE, T_STATE): X_CT}.get((prev, cur))
    return None if row is None else xt[row]


def restate(states, lens, seq, t8, em, ei, en, xt, path=0):
    """(total, [record dict], [core], [null]) of one path: the contract of dcp_gpu_path_domains, one scalar operation
    of the tables' precision per line, in step order."""
    real = t8.dtype.type
    xt = np.asarray(xt, t8.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        s, pos = real(0), 0
        recs, cores, nulls = [], [], []
        cur = None
        for i, (sid, ln) in enumerate(zip((int(v) for v in states), (int(v) for v in lens))):
            kind, x = sid >> 14, sid & 0x3FFF
            t = real(0) if i == 0 else edge(t8, xt, int(states[i - 1]), sid)
            assert t is not None, (i, hex(int(states[i - 1])), hex(sid))
            if ln:
                code = WORD_OFF[ln - 1]
                v = 0
                for b in seq[pos:pos + ln]:
                    v = (v << 2) | int(b)
                code += v
                e = em[code, x - 1] if kind == 0 else ei[code] if kind == 1 else en[code]
                n_i = en[code]
            if i > 0:
                s = s + t
            if ln:
                s = s + e
            if sid == B_STATE:
                cur = dict(path=path, step_begin=i, seq_begin=pos, node_first=0, node_last=0, n_match=0, n_insert=0,
                           n_delete=0, n_shift=0, reserved=0)
                c, n = real(0), real(0)
            elif cur is not None:
                c = c + t
                if ln:
                    c = c + e
                    n = n + n_i
                if int(states[i - 1]) == B_STATE:
                    cur["node_first"] = x
                if kind < 3:
                    cur[("n_match", "n_insert", "n_delete")[kind]] += 1
                    cur["n_shift"] += kind < 2 and ln != 3
                if sid == E_STATE:
                    cur.update(step_end=i, seq_end=pos, node_last=int(states[i - 1]) & 0x3FFF)
                    recs.append(cur)
                    cores.append(c)
                    nulls.append(n)
                    cur = None
            pos += ln
        assert cur is None and pos == len(seq)
        assert all(type(v) is real for v in [s] + cores + nulls)
    return s, recs, cores, nulls


def rec_tuple(r):
    return tuple(int(r[f]) for f in FIELDS)


# ---- CPU: premises -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("precision", PRECISIONS)
def test_premise_the_restated_total_is_the_oracle_s_path_score(oracle32, oracle64, precision):
    orc = oracle64 if precision == 64 else oracle32
    rng = np.random.default_rng(precision)
    domains = 0
    for M in (1, 5, 40, 130):
        prof = orc.new(*pfam_like_params(rng, M))
        gene = planted_query(rng, prof, M, flank=7)
        body = gene[7:-7]
        seqs = [gene, np.delete(gene, 7 + 3 * (M // 2) + 1), np.concatenate([gene, rng.integers(0, 4, 30, dtype=np.uint8), body]),
                rng.integers(0, 4, 1, dtype=np.uint8), rng.integers(0, 4, 5, dtype=np.uint8)]
        for seq in seqs:
            for multi, h3 in ((True, False), (False, False), (True, True)):
                assert prof.setup(len(seq), multi, h3) == 0
                t8, em, ei, en, xt = prof.export()
                nl, al, apath, npath = orc.dp_tables_path(t8, em, ei, en, xt, bytes(seq))
                if len(apath[0]):
                    total, recs, cores, nulls = restate(*apath, seq, t8, em, ei, en, xt)
                    assert bits(total) == bits(orc.np(al)) == bits(orc.np(orc.path_score_tables(t8, em, ei, en, xt, bytes(seq), *apath)))
                    assert len(recs) == int((apath[0] == B_STATE).sum())
                    for r in recs:
                        assert apath[0][r["step_begin"]] == B_STATE and apath[0][r["step_end"]] == E_STATE
                        assert r["n_match"] >= 1 and r["seq_begin"] < r["seq_end"]
                    domains += len(recs)
                total, recs, _, _ = restate(*npath, seq, t8, em, ei, en, xt)
                assert not recs and bits(total) == bits(orc.np(nl))
                assert bits(total) == bits(orc.np(orc.path_score_tables(t8, em, ei, en, xt, bytes(seq), *npath, alt=False)))
    assert domains > 40


PLANT_WANT = {32: [(0, 0, 1112, 1232, 0), (1, 0, 2512, 2902, 1), (2, 1, 4013, 4912, 3)],   # (profile, minus, begin, end, window)
              64: [(0, 0, 1112, 1232, 0), (1, 0, 2512, 2902, 1), (2, 1, 4012, 4912, 3)]}


def planted_cpu_domains(dcp, orc, precision):
    """every domain of every oracle hit (LRT >= 10, multi-hit) of the planted world's ten resident sequences"""
    _, oprofs, seq, _ = planted_world(dcp, orc, precision)
    cut = hand_cut([seq], PLANT_WINDOW, PLANT_STEP)
    W = len(cut)
    res = cut + [np_revcomp(s) for s in cut]
    lrt = oracle_lrt(orc, oprofs, res)
    rows = []
    for r, p in zip(*np.nonzero(lrt >= 10.0)):
        oprofs[p].setup(len(res[r]), True, False)
        t8, em, ei, en, xt = oprofs[p].export()
        _, al, apath, _ = orc.dp_tables_path(t8, em, ei, en, xt, bytes(res[r]))
        total, recs, cores, nulls = restate(*apath, res[r], t8, em, ei, en, xt)
        assert bits(total) == bits(orc.np(al))
        rows += [(int(r), int(p), rec, c, n) for rec, c, n in zip(recs, cores, nulls)]
    return rows, W, [len(s) for s in res]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_premise_the_planted_world_has_seven_domains_and_three_genes(dcp, oracle32, oracle64, precision):
    orc = oracle64 if precision == 64 else oracle32
    rows, W, res_len = planted_cpu_domains(dcp, orc, precision)
    assert len(rows) == 7
    starts = py_starts(PLANT_L, PLANT_WINDOW, PLANT_STEP)
    where = py_locate([r for r, *_ in rows], [rec for _, _, rec, _, _ in rows], res_len, W, [0] * W, starts)
    src, begin, end, minus = (np.array(col) for col in zip(*where))
    profile = np.array([p for _, p, *_ in rows])
    core = np.array([float(c) for *_, c, _ in rows])
    odds = np.array([float(c) - float(n) for *_, c, n in rows])
    # each planted copy once from each of the two windows that wholly contain it: the same interval, the same bits
    twins = {}
    for j, (r, p, rec, c, n) in enumerate(rows):
        twins.setdefault((p, int(minus[j]), int(begin[j]), int(end[j])), []).append((int(bits(c)[0]), int(bits(n)[0])))
    assert sorted(len(v) for v in twins.values()) == [1, 2, 2, 2]
    assert all(len(set(v)) == 1 for v in twins.values())
    (stump,) = [k for k, v in twins.items() if len(v) == 1]
    assert stump[:2] == (2, 1) and stump[3] == 4096 and stump[3] - stump[2] in (83, 84)  # cut by window 2's edge
    keep = py_merge(src, minus, profile, begin, end, odds)
    got = sorted((int(profile[j]), int(minus[j]), int(begin[j]), int(end[j]), rows[j][0] % W) for j in np.flatnonzero(keep))
    assert got == PLANT_WANT[precision]
    # by the raw core score -- a log-likelihood, negative and falling with length -- the stump outranks the whole gene
    j = [k for k in range(7) if (int(begin[k]), int(end[k])) == stump[2:]][0]
    whole = [k for k in range(7) if profile[k] == 2 and k != j]
    assert core[j] > max(core[whole]) and odds[j] < min(odds[whole])
    wrong = py_merge(src, minus, profile, begin, end, core)
    assert wrong[j] and not wrong[whole].any()


# ---- GPU: plumbing -----------------------------------------------------------------------------------------------


def cfg_of(dcp):
    return dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, float(np.float32(0.01)))


def device_tables(dcp, sc, profs):
    """[(trans8, match, insert, null)] as the resident DB holds them, in its precision"""
    if sc.precision == 64:
        out = []
        for p, prof in enumerate(profs):
            ei, en = sc.insert_null_tables64(p)
            out.append((prof.parts64()[0], sc.match_table(p), ei, en))
        return out
    eps = float(np.float32(0.01))
    return [(np.array(p.trans8, np.float32), sc.match_table(i), dcp.frame_table_host(p.insert_dist, eps),
             dcp.frame_table_host(p.null_dist, eps)) for i, p in enumerate(profs)]


def derived_xt(dcp, precision, L, multi, h3):
    return (dcp.xtrans64 if precision == 64 else dcp.xtrans)(L, multi, h3)


def hits_of(dcp, sc, pairs):
    nl, al = sc.scores()
    return np.array([(q, p, nl[q, p], al[q, p]) for q, p in pairs], dcp.HIT64_DTYPE if sc.precision == 64 else dcp.HIT_DTYPE)


def check_against_restatement(dcp, sc, tabs, seqs, hits, paths, multi, h3, xt_rows=None):
    """path_domains of (hits, paths) against `restate`, every field and every bit; returns the call's result"""
    dom, dom_off, core, null, total = sc.path_domains(hits, paths, multi, h3)
    assert dom.dtype == dcp.DOMAIN_DTYPE and dom_off.dtype == np.uint32 and len(dom_off) == len(paths) + 1
    assert core.dtype == null.dtype == total.dtype == (np.float64 if sc.precision == 64 else np.float32)
    assert dom_off[0] == 0 and dom_off[-1] == len(dom) == len(core) == len(null) and len(total) == len(paths)
    for h, path in enumerate(paths):
        q, p = int(hits[h]["seq_idx"]), int(hits[h]["profile_idx"])
        xt = xt_rows[q] if xt_rows is not None else derived_xt(dcp, sc.precision, len(seqs[q]), multi, h3)
        want_total, recs, cores, nulls = restate(path["state_id"], path["seqlen"], seqs[q], *tabs[p], xt, path=h)
        lo, hi = int(dom_off[h]), int(dom_off[h + 1])
        where = (h, q, p, len(path))
        assert [rec_tuple(d) for d in dom[lo:hi]] == [rec_tuple(r) for r in recs], where
        assert np.array_equal(bits(core[lo:hi]), bits(np.array(cores, core.dtype))), where
        assert np.array_equal(bits(null[lo:hi]), bits(np.array(nulls, core.dtype))), where
        assert bits(total[h:h + 1]) == bits(want_total), (where, total[h], want_total)
        for d in dom[lo:hi]:
            assert path["state_id"][d["step_begin"]] == B_STATE and path["state_id"][d["step_end"]] == E_STATE
    return dom, dom_off, core, null, total


# ---- GPU: parity on Viterbi paths ----------------------------------------------------------------------------------

PARITY_M = (1, 5, 40, 64, 65, 128, 129, 300, 513)
_PARITY = {}


def parity_world(dcp, orc, precision):
    """Per profile: the planted consensus; one base removed mid-gene; one codon removed; three random codons inserted;
    two copies 60 nt apart.  Then random sequences of 1 and 5 nt.  `own`: (sequence, profile, copies) of the planted."""
    if precision not in _PARITY:
        rng = np.random.default_rng(1500 + precision)
        params = [pfam_like_params(rng, M) for M in PARITY_M]
        profs = [dcp.ProteinProfile.from_params(*prm, cfg_of(dcp), f"DOM{i}", precision=precision) for i, prm in enumerate(params)]
        seqs, own = [], []
        for p, (M, prm) in enumerate(zip(PARITY_M, params)):
            gene = planted_query(rng, orc.new(*prm, ENTRY_DIST_OCCUPANCY, 0.01), M, flank=12)
            mid = 12 + 3 * (M // 2)
            variants = [gene, np.delete(gene, mid + 1), np.delete(gene, [mid, mid + 1, mid + 2]),
                        np.insert(gene, mid, rng.integers(0, 4, 9, dtype=np.uint8)),
                        np.concatenate([gene[:-12], rng.integers(0, 4, 60, dtype=np.uint8), gene[12:]])]
            for v, s in enumerate(variants):
                own.append((len(seqs), p, 2 if v == 4 else 1))
                seqs.append(np.ascontiguousarray(s, np.uint8))
        short = [len(seqs), len(seqs) + 1]
        seqs += [rng.integers(0, 4, 1, dtype=np.uint8), rng.integers(0, 4, 5, dtype=np.uint8)]
        _PARITY[precision] = (profs, seqs, own, short)
    return _PARITY[precision]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["float", "float-one-layout", "double"])
def test_parity_on_viterbi_paths(dcp, oracle32, oracle64, variant):
    precision = 64 if variant == "double" else 32
    profs, seqs, own, short = parity_world(dcp, oracle64 if precision == 64 else oracle32, precision)
    sc = dcp.Scanner(0)
    sc.upload_db(profs, one_layout=variant == "float-one-layout")
    assert sc.one_layout == (variant == "float-one-layout")
    sc.upload_seqs(seqs)
    tabs = device_tables(dcp, sc, profs)
    seen = dict(match=0, insert=0, delete=0, shift=0, two=0, none=0)
    for multi in (True, False):
        sc.scan(multi, False, -1e30)
        _, al = sc.scores()
        pairs = [(q, p) for q, p, copies in own if multi or copies == 1] + [(q, p) for q in short for p in range(len(profs))]
        pairs = [(q, p) for q, p in pairs if np.isfinite(al[q, p])]
        assert len(pairs) >= (len(own) if multi else len(own) * 4 // 5)
        hits = hits_of(dcp, sc, pairs)
        paths, alt = sc.trace_paths(hits, multi, False)
        dom, dom_off, core, null, total = check_against_restatement(dcp, sc, tabs, seqs, hits, paths, multi, False)
        # the path's total is the traceback's score and the hit's
        assert np.array_equal(bits(total), bits(alt)) and np.array_equal(bits(total), bits(hits["alt_loglik"]))
        per_path = np.diff(dom_off.astype(np.int64))
        assert per_path.tolist() == [int((path["state_id"] == B_STATE).sum()) for path in paths]
        if not multi:
            assert per_path.max() <= 1
        seen["match"] += int(dom["n_match"].sum())
        seen["insert"] += int(dom["n_insert"].sum())
        seen["delete"] += int(dom["n_delete"].sum())
        seen["shift"] += int(dom["n_shift"].sum())
        seen["two"] += int((per_path >= 2).sum())
        # null paths: no domains, the total is the hit's null score
        npaths, nalt = sc.trace_paths(hits, multi, False, null_model=True)
        ndom, ndom_off, _, _, ntotal = check_against_restatement(dcp, sc, tabs, seqs, hits, npaths, multi, False)
        assert len(ndom) == 0 and not ndom_off.any()
        assert np.array_equal(bits(ntotal), bits(hits["null_loglik"])) and np.array_equal(bits(ntotal), bits(nalt))
        # alt and null paths in one call
        mixed = [paths[i] if i % 2 else npaths[i] for i in range(len(paths))]
        check_against_restatement(dcp, sc, tabs, seqs, hits, mixed, multi, False)
    assert all(seen[k] > 0 for k in ("match", "insert", "delete", "shift", "two")), seen
    assert sc.path_domains_kernel_ms > 0
    sc.close()


# ---- GPU: hand-made paths ----------------------------------------------------------------------------------------


def hand_path(dcp, a, ni, c, nlen=(1,), mlen=(3, 3, 3, 3, 3)):
    """S, N x a, B, M1, I1 x ni, M2 .. M5, E, C x c, T: a + ni + c + 9 steps, B at step a + 1, E at step a + ni + 7"""
    states = [S_STATE] + [N_STATE] * a + [B_STATE, M_(1)] + [I_(1)] * ni + [M_(k) for k in (2, 3, 4, 5)] + [E_STATE]
    states += [C_STATE] * c + [T_STATE]
    lens = [0] + [nlen[i % len(nlen)] for i in range(a)] + [0, mlen[0]] + [3] * ni + list(mlen[1:]) + [0] + [1] * c + [0]
    path = np.zeros(len(states), dcp.STEP_DTYPE)
    path["state_id"], path["seqlen"] = states, lens
    return path


HAND_CASES = [
    # (a, ni, c): the step counts around one and two trips
    (20, 0, 34), (20, 0, 35), (20, 0, 36), (20, 0, 98), (20, 0, 99), (20, 0, 100),
    # B the last step of a trip / the first of the next; the same for E
    (62, 0, 3), (63, 0, 3), (56, 0, 3), (57, 0, 3), (56, 0, 0), (57, 0, 0), (0, 0, 70),
    # B and E both on trip edges: 63 / 127, 64 / 128, 63 / 128
    (62, 58, 3), (63, 58, 3), (62, 59, 0),
    # a domain over three trips: B at 60, E at 130
    (59, 64, 5),
]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hand_made_paths_at_the_trip_edges(dcp, oracle32, oracle64, precision):
    orc = oracle64 if precision == 64 else oracle32
    rng = np.random.default_rng(640 + precision)
    prof = dcp.ProteinProfile.from_params(*pfam_like_params(rng, 5), cfg_of(dcp), "HAND", precision=precision)
    paths = [hand_path(dcp, *case) for case in HAND_CASES]
    assert sorted(len(p) for p in paths[:6]) == [63, 64, 65, 127, 128, 129]
    # fragments of five bases starting at phases 12 .. 15 of a word (behind a N steps of one base), and N steps of every length
    paths += [hand_path(dcp, a, 2, 4, mlen=(5, 4, 5, 2, 1)) for a in (12, 13, 14, 15, 28, 31)]
    paths += [hand_path(dcp, 70, 3, 9, nlen=(1, 2, 3, 4, 5), mlen=(5, 5, 5, 5, 5))]
    straddle = 0
    for p in paths:
        start = np.cumsum(p["seqlen"].astype(np.int64)) - p["seqlen"]
        straddle += int(((start % 16) + p["seqlen"] > 16).sum())
    assert straddle >= 8
    seqs = [rng.integers(0, 4, int(p["seqlen"].sum()), dtype=np.uint8) for p in paths]
    sc = dcp.Scanner(0)
    sc.upload_db([prof])
    sc.upload_seqs(seqs)
    tabs = device_tables(dcp, sc, [prof])
    hits = np.zeros(len(paths), dcp.HIT64_DTYPE if precision == 64 else dcp.HIT_DTYPE)
    hits["seq_idx"] = np.arange(len(paths))
    dom, dom_off, core, null, total = check_against_restatement(dcp, sc, tabs, seqs, hits, paths, True, False)
    assert np.diff(dom_off).tolist() == [1] * len(paths)
    for h, (a, ni, c) in enumerate(HAND_CASES):
        assert (int(dom[h]["step_begin"]), int(dom[h]["step_end"])) == (a + 1, a + ni + 7)
        assert (int(dom[h]["n_match"]), int(dom[h]["n_insert"]), int(dom[h]["seq_begin"])) == (5, ni, a)
    for h, path in enumerate(paths):
        xt = derived_xt(dcp, precision, len(seqs[h]), True, False)
        want = orc.path_score_tables(*tabs[0], xt, bytes(seqs[h]), path["state_id"], path["seqlen"])
        assert bits(total[h:h + 1]) == bits(orc.np(want)), (h, total[h], want)
    sc.close()


# ---- GPU: explicit special transitions, a second upload ----------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_explicit_transitions_and_a_second_upload(dcp, oracle32, oracle64, precision):
    profs, seqs, own, _ = parity_world(dcp, oracle64 if precision == 64 else oracle32, precision)
    pick = [(q, p) for q, p, copies in own if PARITY_M[p] in (5, 65, 300)]
    sub = sorted({q for q, _ in pick})
    batch = [seqs[q] for q in sub]
    pairs = [(sub.index(q), p) for q, p in pick]
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs(batch)
    tabs = device_tables(dcp, sc, profs)
    sc.scan(True, False, -1e30)
    hits = hits_of(dcp, sc, pairs)
    paths, _ = sc.trace_paths(hits, True, False)
    base = check_against_restatement(dcp, sc, tabs, batch, hits, paths, True, False)
    # explicit rows: those of uni-hit mode under a call that says multi-hit -- the rows hold, the flags are ignored
    rows = np.stack([derived_xt(dcp, precision, len(s), False, False) for s in batch])
    sc.set_xtrans(rows)
    sc.scan(True, False, -1e30)
    xhits = hits_of(dcp, sc, pairs)
    xpaths, xalt = sc.trace_paths(xhits, True, False)
    got = check_against_restatement(dcp, sc, tabs, batch, xhits, xpaths, True, False, xt_rows=rows)
    assert np.array_equal(bits(got[4]), bits(xalt)) and not np.array_equal(bits(got[4]), bits(base[4]))
    # the same paths, other rows: the sums move with the rows
    rows2 = rows.copy()
    rows2[:, X_NB] -= 1.0
    sc.set_xtrans(rows2)
    moved = check_against_restatement(dcp, sc, tabs, batch, xhits, xpaths, True, False, xt_rows=rows2)
    assert not np.array_equal(bits(moved[4]), bits(got[4])) and np.array_equal(bits(moved[2]), bits(got[2]))
    # a new upload: the derived transitions again, other sequences behind the same indices
    batch2 = [s for s in reversed(batch)]
    sc.upload_seqs(batch2)
    n = len(batch2)
    pairs2 = [(n - 1 - q, p) for q, p in pairs]
    sc.scan(True, False, -1e30)
    hits2 = hits_of(dcp, sc, pairs2)
    paths2, alt2 = sc.trace_paths(hits2, True, False)
    again = check_against_restatement(dcp, sc, tabs, batch2, hits2, paths2, True, False)
    assert np.array_equal(bits(again[4]), bits(alt2)) and np.array_equal(bits(again[4]), bits(base[4]))
    assert np.array_equal(bits(again[2]), bits(base[2])) and np.array_equal(bits(again[3]), bits(base[3]))
    sc.close()


# ---- GPU: refusals -----------------------------------------------------------------------------------------------


def raw_domains(dcp, sc, hits, paths, cap, f64=None, total=True):
    """the C call on sentinel-filled outputs: (rc, message, outputs, untouched)"""
    f64 = sc.precision == 64 if f64 is None else f64
    real = np.float64 if f64 else np.float32
    n = len(paths)
    sq = np.ascontiguousarray(hits["seq_idx"], np.uint32)
    pr = np.ascontiguousarray(hits["profile_idx"], np.uint32)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in paths])
    steps = np.ascontiguousarray(np.concatenate(paths), dcp.STEP_DTYPE)
    dom = np.full(max(cap, 1) * 12, 0xABABABAB, np.uint32)
    dom_off = np.full(n + 1, 0xABABABAB, np.uint32)
    core, null, tot = np.full(max(cap, 1), -7.5, real), np.full(max(cap, 1), -7.5, real), np.full(n, -7.5, real)
    call = sc._lib.dcp_gpu_path_domains64 if f64 else sc._lib.dcp_gpu_path_domains
    rc = call(sc._c, sq.ctypes.data, pr.ctypes.data, n, steps.ctypes.data, off.ctypes.data, 1, 0, dom.ctypes.data, cap,
              dom_off.ctypes.data, core.ctypes.data, null.ctypes.data, tot.ctypes.data if total else None)
    untouched = ((dom == 0xABABABAB).all() and (dom_off[:n] == 0xABABABAB).all() and (core == -7.5).all()
                 and (null == -7.5).all() and (tot == -7.5).all())
    return rc, sc._lib.dcp_gpu_last_error(sc._c).decode(), (dom, dom_off, core, null, tot), untouched


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_everything_untouched(dcp, precision):
    rng = np.random.default_rng(404 + precision)
    prof = dcp.ProteinProfile.from_params(*pfam_like_params(rng, 5), cfg_of(dcp), "REF", precision=precision)
    good = hand_path(dcp, 4, 1, 3)
    L = int(good["seqlen"].sum())
    seqs = [rng.integers(0, 4, L, dtype=np.uint8), rng.integers(0, 4, L - 3, dtype=np.uint8)]
    hit_t = dcp.HIT64_DTYPE if precision == 64 else dcp.HIT_DTYPE
    one = np.zeros(1, hit_t)
    sc = dcp.Scanner(0)
    sc.upload_db([prof])
    # no batch resident
    rc, msg, _, untouched = raw_domains(dcp, sc, one, [good], 4)
    assert rc == dcp.RC_EINVAL and "no sequences resident" in msg and untouched
    sc.upload_seqs(seqs)
    sc.scan(True, False, -1e30)
    before = [bits(x).copy() for x in sc.scores()]
    rc, msg, out, _ = raw_domains(dcp, sc, one, [good], 4)
    assert rc == 0 and out[1].tolist() == [0, 1], msg

    def variant(edit):
        st, ln = good["state_id"].tolist(), good["seqlen"].tolist()
        st, ln = edit(st, ln)
        p = np.zeros(len(st), dcp.STEP_DTYPE)
        p["state_id"], p["seqlen"] = st, ln
        return p

    b = good["state_id"].tolist().index(B_STATE)
    m4 = good["state_id"].tolist().index(M_(4))
    e = good["state_id"].tolist().index(E_STATE)
    on_seq1 = np.zeros(1, hit_t)
    on_seq1["seq_idx"] = 1
    cases = [
        # M3 -> M5: the kernel's finding (the path is three bases short: sequence 1 has them)
        (on_seq1, variant(lambda st, ln: (st[:m4] + st[m4 + 1:], ln[:m4] + ln[m4 + 1:])), ("step %d" % m4, "M3 -> M5", "no edge")),
        # D1: no delete state at node 1
        (one, variant(lambda st, ln: (st[:b + 1] + [D_(1)] + st[b + 1:], ln[:b + 1] + [0] + ln[b + 1:])), ("step %d" % (b + 1), "B -> D1", "no edge")),
        # N -> M1 (the B moved into M4's place): the first of a path's bad edges is the one named
        (on_seq1, variant(lambda st, ln: (st[:b] + st[b + 1:m4] + [B_STATE] + st[m4 + 1:], ln[:b] + ln[b + 1:m4] + [0] + ln[m4 + 1:])),
         ("step %d" % b, "N -> M1", "no edge")),
        # a path that stops short of the sequence
        (one, variant(lambda st, ln: (st[:1] + st[2:], ln[:1] + ln[2:])), ("emit %d bases" % (L - 1), "sequence 0 has %d" % L)),
        # an alt path without T
        (one, variant(lambda st, ln: (st[:-1], ln[:-1])), ("ends with T",)),
        # a B without an E, and a second B before the E
        (one, variant(lambda st, ln: (st[:e] + st[e + 1:], ln[:e] + ln[e + 1:])), ("B without an E",)),
        (one, variant(lambda st, ln: (st[:b + 1] + [B_STATE] + st[b + 1:], ln[:b + 1] + [0] + ln[b + 1:])), ("a B before the E",)),
        # an E without a B, R in an alt path, a null path that is not all R, an emitting state that emits nothing, a
        # state of a larger profile
        (one, variant(lambda st, ln: (st[:b] + st[b + 1:], ln[:b] + ln[b + 1:])), ("E without a B",)),
        (one, variant(lambda st, ln: (st[:1] + [R_STATE] + st[2:], ln)), ("R in an alt path",)),
        (one, variant(lambda st, ln: ([R_STATE] + st[2:], [1] + ln[2:])), ("null path",)),
        (one, variant(lambda st, ln: (st[:e] + [C_STATE] + st[e + 1:], ln)), ("an emitting state with seqlen 0",)),
        (one, variant(lambda st, ln: (st[:m4] + [M_(6)] + st[m4 + 1:], ln)), ("no state of a profile of 5 nodes",)),
    ]
    for hits, path, words in cases:
        rc, msg, _, untouched = raw_domains(dcp, sc, hits, [path], 4)
        assert rc == dcp.RC_EINVAL and untouched, (msg, words)
        assert all(w in msg for w in words), (msg, words)
    # the first bad (path, step) of several is the one named
    bad = cases[1][1]
    rc, msg, _, untouched = raw_domains(dcp, sc, np.zeros(3, hit_t), [good, bad, bad], 4)
    assert rc == dcp.RC_EINVAL and untouched and "path 1, step %d" % (b + 1) in msg
    # a capacity too small: the need in dom_off[npaths], nothing else
    three = np.zeros(3, hit_t)
    rc, msg, out, untouched = raw_domains(dcp, sc, three, [good] * 3, 2)
    assert rc == dcp.RC_ENOMEM and untouched and out[1][3] == 3 and "3 domains" in msg
    rc, msg, out, _ = raw_domains(dcp, sc, three, [good] * 3, 3, total=False)  # total_out may be NULL
    assert rc == 0 and out[1].tolist() == [0, 1, 2, 3] and (out[4] == -7.5).all()
    assert np.array_equal(bits(out[2][:1]), bits(out[2][1:2])) and np.array_equal(bits(out[2][:1]), bits(out[2][2:3]))
    # Scanner.path_domains retries at the true count: 2 n domains are its first guess, here there are 3 n
    triple = variant(lambda st, ln: (st[:e + 1] + ([J_STATE] + st[b:e + 1]) * 2 + st[e + 1:], ln[:e + 1] + ([3] + ln[b:e + 1]) * 2 + ln[e + 1:]))
    long_seq = rng.integers(0, 4, int(triple["seqlen"].sum()), dtype=np.uint8)
    # a precision mismatch
    rc, msg, _, untouched = raw_domains(dcp, sc, one, [good], 4, f64=precision != 64)
    assert rc == dcp.RC_EINVAL and untouched and ("double" in msg and "float" in msg)
    # null pointers
    sq = np.zeros(1, np.uint32)
    call = sc._lib.dcp_gpu_path_domains64 if precision == 64 else sc._lib.dcp_gpu_path_domains
    assert call(sc._c, None, sq.ctypes.data, 1, None, None, 1, 0, None, 0, None, None, None, None) == dcp.RC_EINVAL
    assert "null" in sc._lib.dcp_gpu_last_error(sc._c).decode()
    # no paths: fine, nothing written
    assert call(sc._c, None, None, 0, None, None, 1, 0, None, 0, None, None, None, None) == 0
    # the last scan is as it was
    for x, y in zip(sc.scores(), before):
        assert np.array_equal(bits(x), y)
    sc.upload_seqs([long_seq])
    dom, dom_off, core, null, total = sc.path_domains(one, [triple], True, False)
    assert len(dom) == 3 and dom_off.tolist() == [0, 3] and dom["n_match"].tolist() == [5, 5, 5]
    sc.close()


# ---- GPU: end to end -----------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_end_to_end_in_the_planted_world(dcp, oracle32, oracle64, precision):
    orc = oracle64 if precision == 64 else oracle32
    profs, _, seq, inside = planted_world(dcp, orc, precision)
    sc = dcp.Scanner(0)
    sc.upload_db(profs)
    sc.upload_seqs([seq])
    sc.cut_windows(PLANT_WINDOW, PLANT_STEP)
    sc.add_reverse_strand()
    W = sc.nseqs // 2
    sc.scan(True, False, 10.0)
    hits = sc.hits()
    paths, alt = sc.trace_paths(hits, True, False)
    dom, dom_off, core, null, total = sc.path_domains(hits, paths, True, False)
    assert np.array_equal(bits(total), bits(alt)) and np.array_equal(bits(total), bits(hits["alt_loglik"]))
    src, begin, end, minus = sc.locate_domains(hits, dom)
    res = hits["seq_idx"][dom["path"]]
    profile = hits["profile_idx"][dom["path"]]
    # the context's maps are the pure call's
    wsrc, woff = sc.window_map()
    pure = dcp.locate_domains(res, dom, np.full(2 * W, PLANT_WINDOW), W, 2, wsrc, woff)
    assert all(np.array_equal(a, b) for a, b in zip(pure, (src, begin, end, minus)))
    assert not src.any() and np.array_equal(minus, res >= W)
    # every planted copy from each of the two windows that wholly contain it: one interval, the same bits
    copies = {}
    for j in range(len(dom)):
        copies.setdefault((int(profile[j]), int(minus[j]), int(begin[j]), int(end[j])), []).append(j)
    for p, b, e, m, _ in [(p, b, e, m, w) for p, m, b, e, w in PLANT_WANT[precision]]:
        js = copies[(p, m, b, e)]
        assert sorted((int(res[j]) % W, int(res[j]) >= W) for j in js) == sorted((i, mi) for pp, i, mi in inside if pp == p)
        assert len({(int(bits(core[j:j + 1])[0]), int(bits(null[j:j + 1])[0])) for j in js}) == 1
    odds = core.astype(np.float64) - null.astype(np.float64)
    keep = dcp.merge_domains(src, minus, profile, begin, end, odds)
    got = sorted((int(profile[j]), int(minus[j]), int(begin[j]), int(end[j]), int(res[j]) % W) for j in np.flatnonzero(keep))
    assert got == PLANT_WANT[precision]
    # the stump of profile 2 at window 2's edge, if the device reports that hit, is dropped
    stumps = [j for j in range(len(dom)) if profile[j] == 2 and int(end[j]) == 4096]
    assert not keep[stumps].any()
    assert np.array_equal(keep, py_merge(src, minus, profile, begin, end, odds))
    sc.close()
