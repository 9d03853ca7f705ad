"""Packed-fp32 instructions of the built library, by kernel and op_sel form.

Why: on MI355X `v_pk_mul_f32 vD, vA, vB op_sel:[0,1]` (BOTH results read the HIGH half of src1) was seen to return a
low result of 0 in lanes 48-63, now and then, when a second wave shares the SIMD (round 6, DESIGN 7: the mu-zero form of
k_painn_fwd_mma; one block per CU, or the same kernel without packed ops: never).  painn_mma.hip is therefore compiled
without packed fp32 arithmetic; this tool lists what the other kernels contain and tests/test_round6_cpu.py holds the
matrix-pipe PaiNN kernels to zero.  The rest are covered by full-occupancy fp64 tests (tests/packed_opsel_registry.py):
resources() and waves_per_simd() give the occupancy a recorded launch reaches, from the code object itself.

    python tools/scan_packed_opsel.py [libgeossl_hip.so]          # table: kernel, register-limited waves/SIMD, packed ops
"""
import collections, os, re, struct, subprocess, sys, tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path):
    """The gfx950 ELF images inside a HIP fat binary (clang offload bundles: magic, u64 count, {offset, size, triple})."""
    data = open(path, "rb").read()
    out, pos = [], 0
    while True:
        b = data.find(MAGIC, pos)
        if b < 0:
            return out
        n = struct.unpack_from("<Q", data, b + len(MAGIC))[0]
        p = b + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "amdgcn" in triple and size:
                out.append(data[b + off:b + off + size])
        pos = b + len(MAGIC)


def disassemble(image):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(image)
        f.flush()
        return subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", f.name], capture_output=True, text=True, check=True).stdout


PK = re.compile(r"\b(v_pk_(?:mul|add|fma)_f32)\b(.*)")


def scan(path):
    """{kernel: Counter(form -> count)}; form = mnemonic + its op_sel / op_sel_hi modifiers ('plain' without op_sel)."""
    table = collections.defaultdict(collections.Counter)
    for image in code_objects(path):
        kernel = None
        for line in disassemble(image).splitlines():
            m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
            if m:
                kernel = m.group(1)
                continue
            m = PK.search(line)
            if m and kernel:
                mods = " ".join(re.findall(r"op_sel(?:_hi)?:\[[01,]+\]", m.group(2)))
                table[kernel][m.group(1) + (" " + mods if mods else "")] += 1
    return table


def lo_select_forms(counter):
    """The forms whose LOW result reads a source's high half (an op_sel bit set)."""
    return {f: c for f, c in counter.items() if re.search(r"op_sel:\[[01,]*1", f)}


RESOURCE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "max_flat_workgroup_size")


def resources(path):
    """{kernel: {vgpr_count, agpr_count, sgpr_count, group_segment_fixed_size, max_flat_workgroup_size}} from the AMDGPU
    metadata note of every code object (`llvm-readelf --notes`: one `- .key: value` entry per kernel, keys at indent 4)."""
    out = {}
    for image in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(image)
            f.flush()
            text = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        entries, cur = [], None
        for line in text.splitlines():
            m = re.match(r"^  - \.(\w+):\s*(.*)$", line)
            if m:
                cur = {}
                entries.append(cur)
            else:
                m = re.match(r"^    \.(\w+):\s*(.*)$", line)
            if m and cur is not None:
                cur[m.group(1)] = m.group(2).strip()
        for e in entries:
            if "name" in e:
                out[e["name"]] = {k: int(e.get(k, 0)) for k in RESOURCE_KEYS}
    return out


CUS, SIMDS_PER_CU, LDS_PER_CU, MAX_WAVES_PER_SIMD = 256, 4, 160 * 1024, 8


def register_waves(res):
    """Waves per SIMD the register file allows (MI355X: 512 VGPR+AGPR per lane and SIMD, allocated in granules of 8).
    On gfx950 the metadata's .vgpr_count is already the unified total (the VGPRs rounded up to 4, then the AGPRs)."""
    regs = max(res["vgpr_count"], res["agpr_count"])
    alloc = max(8, (regs + 7) // 8 * 8)
    return min(MAX_WAVES_PER_SIMD, 512 // alloc)


def waves_per_simd(res, block_threads, dynamic_lds, blocks_in_grid):
    """Waves per SIMD on the busiest CU of a launch: blocks of `block_threads` spread over the 256 CUs, as many on a CU
    as registers (register_waves), LDS (group_segment_fixed_size + dynamic_lds of 160 KiB), the 8-waves-per-SIMD cap and
    the grid (ceil(blocks / 256)) allow; a block's waves spread over the CU's four SIMDs."""
    assert 0 < block_threads <= res["max_flat_workgroup_size"], (block_threads, res["max_flat_workgroup_size"])
    wpb = (block_threads + 63) // 64
    per_cu = SIMDS_PER_CU * register_waves(res) // wpb
    lds = res["group_segment_fixed_size"] + dynamic_lds
    if lds > 0:
        per_cu = min(per_cu, LDS_PER_CU // lds)
    per_cu = min(per_cu, (blocks_in_grid + CUS - 1) // CUS)
    return (per_cu * wpb + SIMDS_PER_CU - 1) // SIMDS_PER_CU


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "geossl_amd", "lib", "libgeossl_hip.so")
    res = resources(lib)
    for k, c in sorted(scan(lib).items()):
        sel = lo_select_forms(c)
        w = register_waves(res[k]) if k in res else "?"
        print("%-90s waves/SIMD(regs) %s  packed %5d  op_sel %4d  %s" % (k[:90], w, sum(c.values()), sum(sel.values()),
                                                                        dict(sel) if sel else ""))
