"""What the compiler made of viterbi64_qlane_kernel (dcp_f64_qlane.hip), checked on every build without a GPU: the
file is compiled for gfx950 with the Makefile's flags and the kernel's metadata and ISA are read.

  * two blocks of 256 threads per CU: LDS per block <= 81 920 B, at most 256 VGPRs; the scratch size is recorded
    (spills outside the row loops cost a tile's start, inside them they would cost every row);
  * inside the row loops -- the four tile variants' and the special states' -- no scratch operation and no
    `s_waitcnt vmcnt(0)`: the boundary planes are prefetched a turn of the ring ahead and waited for by count;
  * no s_sleep anywhere in the kernel (nothing polls), no cross-lane operation, and no inline assembly that touches
    memory: the only asm statements are empty ones and comment marks.

The row loops are found by the comment marks the source leaves at the top of each loop's body
(DCP_QL64_ROWS_BEGIN) and the loop membership the assembler's verbose output gives every basic block
("in Loop: Header=BB0_n")."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deciphon-old_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(CSRC, "dcp_f64_qlane.hip")
KERNEL = "viterbi64_qlane_kernel"
BLOCK = re.compile(r"^(?:\.LBB\d+_(\d+):|; %bb\.(\d+):)")


@pytest.fixture(scope="module")
def qlane64_asm(tmp_path_factory):
    if not shutil.which(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "f64_qlane.s"
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
             "-ffp-contract=off", "-fno-honor-nans", "-S", "--cuda-device-only"]  # the Makefile's HIPFLAGS
    subprocess.run([HIPCC] + flags + [SRC, "-o", str(out)], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    return out.read_text().splitlines()


def kernel_body(lines):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*%s\S*:" % KERNEL, l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def mnemonics(body):
    return [t.split()[0] for t in (l.strip() for l in body)
            if t and not t.startswith((";", ".")) and not t.endswith(":")]


def row_loops(body):
    """{loop header: lines of every basic block of that loop}, for the loops that carry a ROWS_BEGIN mark"""
    blocks = []
    for l in body:
        m = BLOCK.match(l)
        if m:
            blocks.append((m.group(1) or m.group(2), l, []))
        elif blocks:
            blocks[-1][2].append(l)
    loops = {}
    for num, head, text in blocks:
        if not any(t.strip() == "; DCP_QL64_ROWS_BEGIN" for t in text):
            continue
        m = re.search(r"in Loop: Header=BB\d+_(\d+)\b", head)
        hdr = m.group(1) if m else num
        loops[hdr] = [t for n, h, tx in blocks
                      if n == hdr or re.search(r"in Loop: Header=BB\d+_%s\b" % hdr, h) for t in tx]
    return loops


def metadata(lines, key):
    """`.key: value` of the kernel's entry in the AMDGPU metadata (entries of amdhsa.kernels start with `  - .`)"""
    first = next(i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")) + 1
    last = next(i for i in range(first, len(lines)) if lines[i].startswith("amdhsa.target"))
    starts = [i for i in range(first, last) if lines[i].startswith("  - .")] + [last]
    for lo, hi in zip(starts, starts[1:]):
        entry = lines[lo:hi]
        if any(re.match(r"\s*\.name:\s+\S*%s" % KERNEL, l) for l in entry):
            for l in entry:
                m = re.match(r"\s*(?:- )?\.%s:\s+(\d+)" % key, l)
                if m:
                    return int(m.group(1))
    raise KeyError(key)


@pytest.mark.timeout(600)
def test_resources_allow_two_blocks_per_cu(qlane64_asm, record_property):
    lds = metadata(qlane64_asm, "group_segment_fixed_size")
    vgpr = metadata(qlane64_asm, "vgpr_count")
    agpr = metadata(qlane64_asm, "agpr_count")
    scratch = metadata(qlane64_asm, "private_segment_fixed_size")
    for k, v in (("lds_bytes", lds), ("vgprs", vgpr), ("agprs", agpr), ("scratch_bytes_per_lane", scratch)):
        record_property(k, v)
    print(f"viterbi64_qlane_kernel: LDS {lds} B, {vgpr} VGPRs (+{agpr} AGPRs), scratch {scratch} B per lane")
    assert 3 * 1364 * 16 <= lds <= 81920  # the tile image, the insert / null table; two blocks in 160 KiB
    assert vgpr <= 256 and agpr == 0      # two wavefronts per SIMD (the count is of the unified file)
    assert metadata(qlane64_asm, "max_flat_workgroup_size") == 256


@pytest.mark.timeout(600)
def test_row_loops_have_no_scratch_and_no_full_wait(qlane64_asm):
    body = kernel_body(qlane64_asm)
    loops = row_loops(body)
    assert len(loops) == 5, sorted(loops)  # first / middle / last / only tile, and the special states' sweep
    ntile = 0
    for hdr, text in loops.items():
        ops = mnemonics(text)
        f64 = sum(o.startswith(("v_add_f64", "v_max_f64")) for o in ops)
        assert f64 >= 200, (hdr, f64)  # a turn of five rows, not a stub
        ntile += f64 >= 500
        assert not [o for o in ops if o.startswith("scratch_")], hdr
        assert not [t for t in text if "s_waitcnt" in t and re.search(r"vmcnt\(0\)", t)], hdr
        assert not [t for t in text if re.search(r"s_waitcnt\s+(0x[0-9a-f]+|\d+)\s*$", t.split(";")[0])], hdr  # raw encodings
        assert f64 < 500 or [o for o in ops if o.startswith("ds_read_b128")], hdr  # a tile's 32-byte image rows
    assert ntile == 4


@pytest.mark.timeout(600)
def test_nothing_polls_and_nothing_crosses_lanes(qlane64_asm):
    ops = mnemonics(kernel_body(qlane64_asm))
    assert len(ops) > 3000
    assert "s_sleep" not in ops
    assert not [o for o in ops if "dpp" in o or o.startswith(("ds_bpermute", "ds_permute", "ds_swizzle", "v_permlane"))]
    # (v_readlane / v_writelane may appear: the compiler keeps spilled scalar registers in a VGPR's lanes)
    # results leave through ordinary vector stores and global atomics
    assert [o for o in ops if o.startswith("global_store")] and [o for o in ops if o.startswith("global_atomic")]
    # the source's asm statements: empty ones (compiler barriers) and comment marks -- none touches memory
    src = open(SRC).read()
    asms = re.findall(r"asm\s+volatile\s*\(([^;]*)\)\s*;?", src) + re.findall(r"asm\s+volatile\((.*)\)$", src, flags=re.M)
    assert asms
    for a in asms:
        assert re.match(r'^\s*(""|"; "\s*name)\s*(:::?\s*("memory")?\s*)?$', a.strip()), a


def test_python_constant(dcp):
    assert dcp.KERNEL_QLANE64 == 4
    assert (dcp.KERNEL_AUTO, dcp.KERNEL_ROWSWEEP, dcp.KERNEL_QLANE, dcp.KERNEL_QLANE2) == (0, 1, 2, 3)
