"""What the context remembers of its last scan is that scan's alone.

dcp_gpu.hip keeps one record of the last scan (struct LastScan: range, kernel, launches, redo pairs, the pair list's
accounting, what has not been looked at yet).  Each of the four scan drivers -- dcp_gpu_scan_range, scan64,
dcp_gpu_scan_pairs, scan_pairs64 -- begins with a fresh record; a new DB or a new batch puts the empty one back; Forward
and the other list calls do not touch it.  So whatever ran before, the getters report after a call what a context that
ran that call alone reports.

One Scanner runs scans of every kind one after the other, on a float DB and then on a double DB of the same six
profiles; after each call a fresh Scanner runs that call alone and is the reference.  Nothing carries over.

The six core sizes are 40, 100, 300, 520, 700 and 1100: row-sweep classes of one wavefront, of 4 and of 8 wavefronts
per pair, and the f64 launch groups 0, 1 and 3 (no profile of 129 .. 256 nodes: group 2 stays empty)."""
import numpy as np
import pytest

from oracle_py import ENTRY_DIST_OCCUPANCY

CORE_SIZES = (40, 100, 300, 520, 700, 1100)
NEG_INF = float("-inf")  # every pair with finite scores is a hit: hits() has something to compare
# ten listed pairs: every profile, no pair twice (the order of two equal hit records is not defined)
PAIR_SEQ = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 3])
PAIR_PROF = np.array([0, 1, 2, 3, 4, 5, 5, 2, 3, 0])
FWD_SEQ, FWD_PROF = np.array([7, 1, 4, 2]), np.array([5, 0, 3, 1])


def snapshot(dcp, sc):
    """Every last-scan getter's answer; a refusal ("no scan yet") is an answer too."""
    def answer(get):
        try:
            return get()
        except dcp.DcpError as e:
            return ("refused", e.rc)

    infos = answer(lambda: [(li["R"], li["W"], li["nprofiles"], li["cells"], li["algorithmic_bytes"])
                            for li in sc.launch_infos()])
    return dict(cells=sc.cells, algorithmic_bytes=sc.algorithmic_bytes, kernel=sc.last_scan_kernel,
                launches=sc.last_scan_launches, redo_pairs=answer(lambda: sc.last_scan_redo_pairs),
                launch_infos=infos, hits=answer(lambda: sc.hits().tobytes()))


@pytest.mark.gpu
def test_getters_report_the_last_call_alone(dcp):
    cfg = dcp.ProteinCfg(ENTRY_DIST_OCCUPANCY, 0.01)
    profs = {precision: [dcp.ProteinProfile.sample(500 + i, M, cfg, f"LAST{i}", precision=precision)
                         for i, M in enumerate(CORE_SIZES)] for precision in (32, 64)}
    rng = np.random.default_rng(20261)
    seqs = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in rng.integers(30, 91, 8)]

    # (name, the DB's precision, the call; None: only the upload)
    steps = [
        ("float query-lane scan with redo lists", 32,
         lambda sc: sc.scan(True, False, NEG_INF, kernel=dcp.KERNEL_QLANE)),
        ("float pair list", 32, lambda sc: sc.scan_pairs(PAIR_SEQ, PAIR_PROF, lrt_threshold=NEG_INF)),
        ("float row sweep of [2, 6)", 32,
         lambda sc: sc.scan(True, False, NEG_INF, kernel=dcp.KERNEL_ROWSWEEP, q_range=(2, 6))),
        ("Forward scores of four pairs", 32, lambda sc: sc.forward_pairs(FWD_SEQ, FWD_PROF)),
        ("the double DB's upload", 64, None),
        ("double query-lane scan with redo lists", 64,
         lambda sc: sc.scan(True, False, NEG_INF, kernel=dcp.KERNEL_QLANE64)),
        ("double pair list", 64, lambda sc: sc.scan_pairs(PAIR_SEQ, PAIR_PROF, lrt_threshold=NEG_INF)),
        ("double row sweep", 64, lambda sc: sc.scan(True, False, NEG_INF, kernel=dcp.KERNEL_ROWSWEEP)),
    ]

    def alone(precision, call):
        fresh = dcp.Scanner(0)
        fresh.upload_db(profs[precision])
        fresh.upload_seqs(seqs)
        if call:
            call(fresh)
        snap = snapshot(dcp, fresh)
        fresh.close()
        return snap

    sc = dcp.Scanner(0)
    sc.upload_db(profs[32])
    sc.upload_seqs(seqs)
    resident, want = 32, None
    for name, precision, call in steps:
        if precision != resident:
            sc.upload_db(profs[precision])
            resident = precision
        if name.startswith("Forward"):
            call(sc)  # writes nothing of a scan's: the reference stays the scan before it
        else:
            if call:
                call(sc)
            want = alone(precision, call)
        got = snapshot(dcp, sc)
        for key in want:
            assert got[key] == want[key], f"after {name}: {key} is {got[key]!r}, a fresh context reports {want[key]!r}"
        if call and not name.startswith("Forward"):
            assert got["kernel"] != 0 and got["launches"] > 0 and len(got["hits"]) > 0, name
    sc.close()
    # the kinds differ in what they report: the comparison above is not one of equal constants
    assert alone(32, steps[1][2])["cells"] != alone(32, steps[2][2])["cells"]
