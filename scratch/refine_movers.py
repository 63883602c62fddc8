"""what refine_kernel's candidates do on the benchmark's synthetic frames: gathers per step, how the movers end, revisits, moves by axis.
   Needs the measurement build of the library (MI355_EXTRA_HIPCC_FLAGS=-DMI355_REFINE_STATS python -m imagemosaicing_amd.build --force,
   or MI355_LIB pointing at one): there refine_kernel runs every trajectory out instead of dropping a circling candidate early.
   python scratch/refine_movers.py [frames] [w] [h] [batch] [out.txt]"""
import sys, os, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import imagemosaicing_amd as im
from tests.synth_survey import render_frames
F = int(sys.argv[1]) if len(sys.argv) > 1 else 32
w = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
h = int(sys.argv[3]) if len(sys.argv) > 3 else 3000
B = int(sys.argv[4]) if len(sys.argv) > 4 else 32
out = sys.argv[5] if len(sys.argv) > 5 else None
L = im.load_library()
if not hasattr(L, "mi355_debug_refine_stats"):
    sys.exit("this library is not the measurement build (-DMI355_REFINE_STATS)")
L.mi355_debug_refine_stats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
ctx = im.Context(0)
ctx.set_option("sift_batch", B)
frames, A, gains, ws = render_frames(ctx, torch, F, w, h)
s = (C.c_ulonglong * 40)()
assert L.mi355_debug_refine_stats(s, 1) == 0
for k in range(F):
    ctx.SiftExtractDev(k, frames[k].data_ptr(), w, h, ws)
ctx.synchronize()
assert L.mi355_debug_refine_stats(s, 0) == 0
s = [int(x) / F for x in s]
PAT = ("row only", "layer only", "row and layer", "column involved, one pixel", "more than one pixel", "no move (offset of exactly 0.5)")
lines = ["refine_kernel's candidates, per frame: mean of %d synthetic survey frames %dx%d (the measurement build runs every trajectory out)" % (F, w, h), ""]
def row(name, v): lines.append("%-64s %10.1f" % (name, v))
row("candidates", s[4])
row("  converged at the start location (no gather after step 0)", s[6])
row("  diverged / NaN", s[9])
row("  moved at least once", s[5])
row("    then converged (accepted or rejected by the tests)", s[7])
row("    left the level (border, layer)", s[8])
row("    ran out of steps (dropped)", s[10])
for k in range(1, 5):
    row("      first back on a location of its own at step %d" % k, s[10 + k])
row("      (of these four, not seen by the kernel's three comparisons)", s[32])
row("      never before its steps ran out", s[15])
row("  revisit seen on a candidate that did NOT run out (must be 0)", s[30])
lines.append("")
row("gathers at step 0 (no saved cube)", s[31])
for k in range(1, 5):
    row("gathers at step %d" % k, s[k - 1])
g = sum(s[0:4])
row("gathers at steps 1-4", g)
row("  issued after the candidate's first revisit (part A removes them)", s[16])
lines.append("")
lines.append("the move before each gather of steps 1-4                      before a revisit   after one")
for p in range(6):
    lines.append("  %-58s %10.1f  %10.1f" % (PAT[p], s[17 + p], s[23 + p]))
useful = sum(s[17:23])
row("8-byte loads of the gathers before a revisit, twelve each", 12 * useful)
row("  if a row step loaded 4, a layer step 6, both 8 (part B)", s[29])
lines.append("")
lines.append("counters of the last frame: %s" % (ctx.last_sift_counters(),))
txt = "\n".join(lines)
print(txt)
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    open(out, "w").write(txt + "\n")
