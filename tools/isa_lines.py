#!/usr/bin/env python3
"""Static instruction mix of a stretch of one kernel BY SOURCE LINE (gfx950 assembly from -save-temps with line tables):
    python tools/isa_lines.py filter_bwd.hip k_filter_bwd_hILi4ELb0 .LBB3_114 .LBB3_145 [extra hipcc flags]
counts the instructions from the first label up to (not including) the second, per basic block and source line (the
innermost inlined line), so that the instructions of a loop can be sorted into work per row and work per tile.  The labels
are those of tools/isa_mix.py's listing: the block a backward branch returns to opens a loop."""
import collections, glob, os, re, subprocess, sys, tempfile
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src, pat, first, last = sys.argv[1:5]
tmp = tempfile.mkdtemp(prefix="isa_")
subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-gline-tables-only", "-I",
                here + "/include", "-I", here + "/geossl_amd/csrc", "-Wno-pass-failed", *sys.argv[5:], "-c",
                here + "/geossl_amd/csrc/" + src, "-o", "x.o", "-save-temps=obj"], cwd=tmp, stderr=subprocess.DEVNULL, check=True)
s = open(glob.glob(tmp + "/*gfx950*.s")[0]).read()
m = re.search(r"^(_ZN\S*" + re.escape(pat) + r"\S*):", s, re.M)
body = s[m.end():s.index("s_endpgm", m.end())]
files = {int(f.group(1)): os.path.basename(f.group(3) or f.group(2))
         for f in re.finditer(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', s)}


def kind(x):
    if x.startswith("v_mfma"): return "mfma"
    if x.startswith(("v_exp", "v_log", "v_rcp", "v_sqrt", "v_rsq")): return "trans"
    if x.startswith("v_"): return "valu"
    if x.startswith("ds_"): return "lds"
    if x.startswith(("global_", "buffer_", "scratch_")): return "vmem"
    if x.startswith("s_waitcnt"): return "wait"
    if x.startswith("s_barrier"): return "barrier"
    if x.startswith("s_"): return "salu"
    return "other"


on, loc, blk = False, (0, 0), None
per = collections.OrderedDict()
for l in body.split("\n"):
    l = l.strip()
    lab = re.match(r"^(\.?[A-Za-z_0-9$]+):", l)
    if lab:
        if lab.group(1).startswith(".LBB"):  # (the .Ltmp labels of the line tables do not end a block)
            blk = lab.group(1)
            on = (on or blk == first) and blk != last
        continue
    at = re.match(r"\.loc\s+(\d+)\s+(\d+)", l)
    if at:
        loc = (int(at.group(1)), int(at.group(2)))
    elif on and l and not l.startswith((".", ";")):
        per.setdefault((blk, files.get(loc[0], "?"), loc[1]), collections.Counter())[kind(l.split()[0])] += 1
for (b, f, ln), c in per.items():
    print("%-10s %-20s %5d  %s" % (b, f, ln, dict(c)))
