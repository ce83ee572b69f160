"""Regions: region_words_kernel (csrc/dcp_seqs.hip) behind dcp_gpu_seqs_cut_regions / Scanner.cut_regions.

GPU:
  1. the words of every region, bit for bit, against the host packing of the numpy slice (its reverse complement for
     a minus region), pad words and the bits behind the last base included -- over begins and ends at every phase of a
     word, minus regions whose lower neighbours are real non-zero bases, regions touching either end of their source,
     whole sources on both strands (the minus ones word for word add_reverse_strand's), an all-T source between
     random ones, overlapping, repeated and shuffled regions, and a 2^16-nt source;
  2. a batch of regions scans to the bits of the same slices uploaded by hand, on every kernel and flag set;
  3. the contract: every refusal leaves the batch untouched, add_reverse_strand and cut_windows are refused after the
     cut, an upload clears the state."""
import numpy as np
import pytest

from test_both_strands import bits, hit_fields, host_words, np_revcomp, refused, world

PRECISIONS = (32, 64)
REGION_LENS = (1, 15, 16, 17, 31, 32, 33, 100)
_SOURCES = []


def sources():
    """[0] 64 nt, [1] 65 nt, [2] 79 nt (L & 15 = 0, 1, 15), [3] 300 nt without a single A (every neighbour of a region is
    a non-zero base), [4] random, [5] all T, [6] random, [7] 2^16 nt, [8] one base."""
    if not _SOURCES:
        rng = np.random.default_rng(1616)
        _SOURCES.extend(rng.integers(0, 4, L, dtype=np.uint8) for L in (64, 65, 79))
        _SOURCES.append(rng.integers(1, 4, 300, dtype=np.uint8))
        _SOURCES.append(rng.integers(0, 4, 200, dtype=np.uint8))
        _SOURCES.append(np.full(177, 3, np.uint8))
        _SOURCES.append(rng.integers(0, 4, 200, dtype=np.uint8))
        _SOURCES.append(rng.integers(0, 4, 1 << 16, dtype=np.uint8))
        _SOURCES.append(rng.integers(1, 4, 1, dtype=np.uint8))
    return _SOURCES


def region_list():
    """(src, begin, len, minus) rows, shuffled"""
    seqs = sources()
    rows = []
    # begins at phases 0, 1, 15 (and in later words) x every length x both strands, in the source without an A: the
    # ends then fall on phases 0, 1, 15 too (begin 15 + len 1, begin 0 + len 17, begin 0 + len 15 ...)
    for begin in (0, 1, 15, 16, 17, 31, 47, 160):
        for n in REGION_LENS:
            rows += [(3, begin, n, 0), (3, begin, n, 1)]
    # regions ending at the source's last base, for L & 15 = 0, 1, 15, and starting at its first
    for s in (0, 1, 2, 3, 5):
        L = len(seqs[s])
        for n in REGION_LENS:
            if n <= L:
                rows += [(s, L - n, n, 0), (s, L - n, n, 1), (s, 0, n, 1), (s, 0, n, 0)]
    # whole sources on both strands, the all-T one and its neighbours among them; the one-base source
    for s in range(len(seqs)):
        rows += [(s, 0, len(seqs[s]), 0), (s, 0, len(seqs[s]), 1)]
    # the long source: far from its start, across many words, at odd phases, ending at its last base
    L = 1 << 16
    rows += [(7, 40001, 3000, 1), (7, 40001, 3000, 0), (7, L - 1001, 1001, 1), (7, 65519, 17, 1), (7, 1, L - 1, 1), (7, 15, 4097, 0)]
    # overlapping and repeated ones
    rows += [(4, 10, 100, 0), (4, 50, 100, 0), (4, 50, 100, 1), (4, 10, 100, 0), (6, 33, 33, 1), (6, 33, 33, 1)]
    order = np.random.default_rng(61).permutation(len(rows))
    return [rows[i] for i in order]


def slice_of(seqs, row):
    s, b, n, minus = row
    piece = seqs[s][b:b + n]
    return np_revcomp(piece) if minus else piece


def test_the_region_list_holds_what_the_kernel_can_get_wrong():
    """CPU: the cases the words test must contain, stated."""
    seqs, rows = sources(), region_list()
    assert [len(s) & 15 for s in seqs[:3]] == [0, 1, 15] and not (seqs[3] == 0).any() and (seqs[5] == 3).all()
    assert not (seqs[4] == 3).all() and not (seqs[6] == 3).all()
    assert {0, 1, 15} <= {b & 15 for _, b, _, _ in rows} and set(REGION_LENS) <= {n for _, _, n, _ in rows}
    inner = [(b, n) for s, b, n, minus in rows if s == 3 and minus and b > 0 and b + n < 300]
    assert {0, 1, 15} <= {(b + n) & 15 for b, n in inner}  # below `begin` lie real non-zero bases
    assert any(minus and b == 0 for _, b, _, minus in rows)
    assert {0, 1, 2} <= {s for s, b, n, _ in rows if b + n == len(seqs[s]) and b > 0}
    assert all((s, 0, len(seqs[s]), m) in rows for s in range(len(seqs)) for m in (0, 1))
    assert len(rows) != len(set(rows)) and any(s == 7 for s, *_ in rows)
    assert rows != sorted(rows) and all(n >= 1 and b + n <= len(seqs[s]) for s, b, n, _ in rows)


@pytest.mark.gpu
def test_words_of_every_region(dcp):
    seqs, rows = sources(), region_list()
    sc = dcp.Scanner(0, lib=dcp.load_testhooks())
    sc.upload_seqs(seqs)
    sc.add_reverse_strand()
    strand2 = [sc.test_seq_words(len(seqs) + q) for q in range(len(seqs))]
    sc.upload_seqs(seqs)
    assert sc.regions == 0
    sc.cut_regions(*zip(*rows))
    assert sc.regions == sc.nseqs == len(rows) and sc.strands == 1 and sc.windows is None
    src, begin, minus = sc.region_map()
    assert (src.dtype, begin.dtype, minus.dtype) == (np.uint32, np.uint32, np.uint8)
    assert list(zip(src.tolist(), begin.tolist(), sc._seq_lens.tolist(), minus.tolist())) == rows
    for i, row in enumerate(rows):
        want = host_words(slice_of(seqs, row))
        got = sc.test_seq_words(i)
        assert np.array_equal(got, want), (i, row, [hex(x) for x in got[:4]], [hex(x) for x in want[:4]])
        s, b, n, m = row
        if m and b == 0 and n == len(seqs[s]):  # the whole source's minus strand: add_reverse_strand's words
            assert np.array_equal(got, strand2[s]), row
    for i in list(range(0, len(rows), 7)) + [rows.index((7, 1, (1 << 16) - 1, 1))]:
        assert np.array_equal(sc.fetch_seq(i), slice_of(seqs, rows[i])), rows[i]
    # a second list from a fresh upload: one region, the last base of the last source's neighbour
    sc.upload_seqs(seqs)
    assert sc.regions == 0
    sc.cut_regions([7], [(1 << 16) - 1], [1], [1])
    assert np.array_equal(sc.test_seq_words(0), host_words(3 - seqs[7][-1:]))
    sc.close()


# ---- the bits of a batch cut by hand -------------------------------------------------------------------------------

SAME_BITS_CASES = [(32, 1), (32, 2), (32, 3), (64, 1), (64, 4)]  # (precision, dcp_scan_params.kernel)


def scan_regions(seqs):
    """regions of the strands tests' queries: whole short ones, inner stretches at odd phases, both strands, the long
    query's ends, repeats -- 1 .. 700 nt"""
    rng = np.random.default_rng(77)
    rows = []
    for s, q in enumerate(seqs):
        L = len(q)
        rows.append((s, 0, L if L <= 100 else 100, s & 1))
        if L >= 5:
            b = int(rng.integers(1, L - 2))
            rows.append((s, b, int(rng.integers(1, min(L - b, 300) + 1)), (s + 1) & 1))
    long = max(range(len(seqs)), key=lambda s: len(seqs[s]))
    L = len(seqs[long])
    rows += [(long, L - 700, 700, 1), (long, L - 333, 333, 0), (long, 4001, 513, 1), (long, 4001, 513, 1)]
    return [rows[i] for i in rng.permutation(len(rows))]


@pytest.mark.gpu
@pytest.mark.parametrize("multi_hits", [False, True])
@pytest.mark.parametrize("precision,kernel", SAME_BITS_CASES)
def test_same_bits_as_the_slices_uploaded_by_hand(dcp, precision, kernel, multi_hits):
    profs, seqs = world(dcp, precision)
    rows = scan_regions(seqs)
    cut = [slice_of(seqs, row) for row in rows]
    a, b = dcp.Scanner(0), dcp.Scanner(0)
    a.upload_db(profs)
    b.upload_db(profs)
    a.upload_seqs(seqs)
    a.cut_regions(*zip(*rows))
    b.upload_seqs(cut)
    assert a.nseqs == b.nseqs == len(cut) and a.strands == 1
    assert a.cells == b.cells and a.algorithmic_bytes == b.algorithmic_bytes
    for h3 in (False, True):
        for thr in (10.0, 0.0):
            a.scan(multi_hits, h3, thr, kernel=kernel)
            b.scan(multi_hits, h3, thr, kernel=kernel)
            where = (precision, kernel, multi_hits, h3, thr)
            for x, y in zip(a.scores(), b.scores()):
                assert np.array_equal(bits(x), bits(y)), where
            assert hit_fields(a.hits()) == hit_fields(b.hits()), where
            assert a.last_scan_redo_pairs == b.last_scan_redo_pairs, where
            assert a.last_scan_kernel == b.last_scan_kernel == kernel, where
    a.close()
    b.close()


# ---- contract ------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_contract(dcp, precision):
    profs, seqs = world(dcp, precision)
    seqs = seqs[:12] + [seqs[18]]  # 1 .. 47 nt, and the 1 000-nt query
    n = len(seqs)
    rows = [(12, 100, 300, 1), (11, 0, 47, 0), (12, 700, 300, 0), (0, 0, 1, 1)]
    sc = dcp.Scanner(0)

    def state():
        return sc.nseqs, sc.strands, sc.windows, sc.regions

    def message(call, *words):
        with pytest.raises(dcp.DcpError) as e:
            call()
        assert e.value.rc == dcp.RC_EINVAL and all(w in str(e.value) for w in words), str(e.value)

    cut = lambda rr=rows: sc.cut_regions(*zip(*rr))
    # no batch resident (and no DB)
    message(cut, "no sequences resident")
    assert state() == (0, 0, None, 0)
    refused(dcp, sc, sc.region_map)
    sc.upload_seqs(seqs)
    cut()  # no DB resident: sequences only
    assert state() == (len(rows), 1, None, len(rows))
    sc.upload_db(profs)
    sc.upload_seqs(seqs)
    assert state() == (n, 1, None, 0)  # an upload clears the state
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    want = [bits(x).copy() for x in sc.scores()]

    def same_scan(k=None):
        sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
        for x, y in zip(sc.scores(), want):
            assert np.array_equal(bits(x)[:k], y[:k])

    # an empty list; bad regions, the first one named
    message(lambda: sc.cut_regions([], [], [], []), "empty list")
    message(lambda: cut(rows[:2] + [(n, 0, 1, 0)] + [(n + 1, 0, 1, 0)]), "region 2 ")
    message(lambda: cut([(12, 0, 0, 0)] + rows), "region 0 ")
    message(lambda: cut(rows + [(12, 701, 300, 0)]), "region 4 ")
    message(lambda: cut(rows + [(12, 2 ** 32 - 1, 2, 1)]), "region 4 ")  # begin + len in 64 bits
    with pytest.raises(dcp.DcpError):
        cut([(12, 0, 2 ** 32, 0)])
    with pytest.raises(dcp.DcpError):
        sc.cut_regions([0, 1], [0], [1], [0])
    assert state() == (n, 1, None, 0)
    same_scan()
    # explicit transitions in force, in the precision of the DB
    derived = (dcp.xtrans64 if precision == 64 else dcp.xtrans)
    sc.set_xtrans(np.stack([derived(len(s), True, False) for s in seqs]))
    message(cut, "explicit special transitions")
    assert state() == (n, 1, None, 0)
    sc.scan(False, True, 10.0, kernel=dcp.KERNEL_ROWSWEEP)  # the flags are ignored: the explicit rows still hold
    for x, y in zip(sc.scores(), want):
        assert np.array_equal(bits(x), y)
    # both strands resident; cut into windows
    sc.upload_seqs(seqs)
    sc.add_reverse_strand()
    message(cut, "both strands")
    assert state() == (2 * n, 2, None, 0)
    same_scan(n)
    sc.upload_seqs(seqs)
    sc.cut_windows(2000, 1000)  # every L <= window: the batch word for word
    message(cut, "windows")
    assert state() == (n, 1, (2000, 1000), 0)
    same_scan()
    # the regions' words would pass 2^32 - 1: 70 000 copies of a 2^20-nt source, refused before anything is allocated
    sc.upload_seqs([np.zeros(1 << 20, np.uint8), seqs[3]])
    many = 70000
    message(lambda: sc.cut_regions(np.zeros(many), np.zeros(many), np.full(many, 1 << 20), np.zeros(many)), "too large")
    assert state() == (2, 1, None, 0) and np.array_equal(sc.fetch_seq(1), seqs[3])
    # after the cut: no second cut, no reverse strand, no windows; the batch stays as it is
    sc.upload_seqs(seqs)
    cut()
    sc.scan(True, False, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    want = [bits(x).copy() for x in sc.scores()]
    message(cut, "already")
    message(sc.add_reverse_strand, "regions")
    message(lambda: sc.cut_windows(48, 31), "regions")
    assert state() == (len(rows), 1, None, len(rows))
    same_scan()
    short = np.zeros(len(rows), np.uint32)
    assert sc._lib.dcp_gpu_seqs_region_map(sc._c, short.ctypes.data, short.ctypes.data, short.ctypes.data, len(rows) - 1) == dcp.RC_ENOMEM
    assert not short.any()
    # explicit transitions after the cut take one row per region
    cutseqs = [slice_of(seqs, row) for row in rows]
    refused(dcp, sc, lambda: sc.set_xtrans(np.stack([derived(len(s), True, False) for s in seqs])))
    sc.set_xtrans(np.stack([derived(len(s), True, False) for s in cutseqs]))
    sc.scan(False, True, 10.0, kernel=dcp.KERNEL_ROWSWEEP)
    for x, y in zip(sc.scores(), want):
        assert np.array_equal(bits(x), y)
    # the next upload returns the context to normal
    sc.upload_seqs(cutseqs)
    assert state() == (len(rows), 1, None, 0)
    refused(dcp, sc, sc.region_map)
    same_scan()
    sc.add_reverse_strand()
    assert state() == (2 * len(rows), 2, None, 0)
    sc.close()
