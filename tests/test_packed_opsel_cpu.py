"""CPU guard of the packed-fp32 registry (tests/packed_opsel_registry.py): every kernel of the built library whose code
object holds a packed-fp32 form with a LOW result read from a HIGH half is covered by a named full-occupancy GPU test,
and every launch the registry records reaches the waves per SIMD it claims on that code object (the
failure needed two waves on a SIMD).  No GPU: the checks read the library's code objects (tools/scan_packed_opsel.py)."""
import ast
import os
import re
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import packed_opsel_registry as reg  # noqa: E402
import scan_packed_opsel as sp  # noqa: E402


def _tools():
    if not (os.path.exists(sp.OBJDUMP) and os.path.exists(sp.READELF)):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not found")


@pytest.fixture(scope="module")
def library():
    _tools()
    from geossl_amd import _lib
    return sp.scan(_lib.LIB_PATH), sp.resources(_lib.LIB_PATH)


def _res(vgpr, lds=0, agpr=0, max_threads=1024):
    return dict(vgpr_count=vgpr, agpr_count=agpr, sgpr_count=64, group_segment_fixed_size=lds,
                max_flat_workgroup_size=max_threads)


def test_waves_per_simd_on_hand_checked_launches():
    # registers: 214 VGPRs allocate 216 -> 512 // 216 = 2 waves; 64 -> 8; 65 -> 72 allocated -> 7; 257 -> 1
    assert sp.register_waves(_res(214)) == 2
    assert sp.register_waves(_res(64)) == 8 and sp.register_waves(_res(65)) == 7 and sp.register_waves(_res(257)) == 1
    assert sp.register_waves(_res(128)) == 4 and sp.register_waves(_res(129)) == 3
    # 512-thread blocks (8 waves, 2 per SIMD) at 214 VGPRs: one block per CU, 2 waves per SIMD
    assert sp.waves_per_simd(_res(214), 512, 0, 100000) == 2
    # 256-thread blocks at 2 waves/SIMD by registers: two blocks per CU -> 2; one block per CU (grid of 256) -> 1
    assert sp.waves_per_simd(_res(214), 256, 0, 100000) == 2
    assert sp.waves_per_simd(_res(214), 256, 0, 256) == 1
    # LDS: 96 KiB per block leaves one block of 256 threads per CU whatever the registers allow
    assert sp.waves_per_simd(_res(64), 256, 96 * 1024, 100000) == 1
    assert sp.waves_per_simd(_res(64, lds=16 * 1024), 256, 64 * 1024, 100000) == 2        # static + dynamic: 80 KiB
    # a grid smaller than the CU count: one block on the busiest CU
    assert sp.waves_per_simd(_res(40), 256, 0, 100) == 1
    assert sp.waves_per_simd(_res(40), 1024, 0, 200) == 4
    # the 8-waves-per-SIMD cap: 64-thread blocks at 40 VGPRs, a huge grid -> 32 blocks per CU, 8 waves per SIMD
    assert sp.waves_per_simd(_res(40), 64, 0, 1 << 20) == 8
    # the issue's example: filter_bwd_h<4,*> (512 threads, one block per CU) gets 2, the NW = 2 variant 1
    assert sp.waves_per_simd(_res(216, max_threads=512), 512, reg.filter_bwd_h_lds(128), reg.filter_bwd_grid()) == 2
    assert sp.waves_per_simd(_res(196, max_threads=256), 256, reg.filter_bwd_h_lds(64), reg.filter_bwd_grid()) == 1
    with pytest.raises(AssertionError):
        sp.waves_per_simd(_res(40, max_threads=256), 512, 0, 1)        # (beyond the kernel's launch bound)


def test_every_low_select_packed_kernel_is_registered(library):
    table, _ = library
    assert any("k_filter_bwd_h" in k for k in table), "the scan sees the library's kernels"
    missing = [k for k, c in table.items() if sp.lo_select_forms(c) and len(reg.entries_for(k)) != 1]
    assert not missing, "kernels with low-select packed fp32 forms and no (or an ambiguous) registry entry: %s" % missing


def test_every_registry_entry_names_one_kernel_of_the_library(library):
    _, res = library
    for e in reg.ENTRIES:
        hits = [k for k in res if re.search(e["symbol"], k)]
        assert len(hits) == 1, (e["symbol"], hits)


def test_registered_launches_reach_the_waves_per_simd_they_claim(library):
    _, res = library
    for e in reg.ENTRIES:
        (k,) = [k for k in res if re.search(e["symbol"], k)]
        assert e["launches"], e["symbol"]
        for label, block, lds, grid, waves, cap in e["launches"]:
            got = sp.waves_per_simd(res[k], block, lds, grid)
            assert got == waves, (e["symbol"], label, got, waves, res[k])
            if waves < 2:
                # one wave per SIMD only where the block and the kernel's resources (or the launcher's fixed grid) say so
                assert cap, (e["symbol"], label, "one wave per SIMD without a stated reason")
                fixed_grid = e["family"] in ("k_filter_bwd_h", "k_filter_bwd")
                limit = sp.waves_per_simd(res[k], block, lds, grid if fixed_grid else reg.HUGE_GRID)
                assert limit < 2, (e["symbol"], label, "a larger grid would reach %d waves per SIMD" % limit)


def _test_names(module_file):
    """Top-level test functions of a test module, read from its source (no import: the GPU modules need a GPU)."""
    tree = ast.parse(open(module_file).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_every_registered_test_exists():
    names = {}
    for e in reg.ENTRIES:
        for t in e["tests"]:
            mod, fn = t.split("::") if "::" in t else (reg.GPU_MODULE, t)
            if mod not in names:
                names[mod] = _test_names(os.path.join(REPO, "tests", mod + ".py"))
            assert fn in names[mod], (e["symbol"], t)


def test_scan_tool_prints_a_waves_per_simd_column(library):
    import subprocess
    from geossl_amd import _lib
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "scan_packed_opsel.py"), _lib.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    row = [ln for ln in out.splitlines() if "k_filter_bwd_hILi4ELb0E" in ln]
    assert len(row) == 1 and re.search(r"waves/SIMD\(regs\) 2 ", row[0]), row
