"""Phase stamps (100 MHz wall clock) of one workgroup / one node of the chunk sweep (csrc/chunk.hip: k_chunk_sweep, two teams of
waves).  usage: sweep_stamps.py [workgroup] [node of the run]
node -1: the factorisation of the run's FIRST node (chain on wave 0, helper L on wave 1, helper U on strip wave 2), us from
the workgroup's start; every other node k: the iteration of node k, whose factorisation stamps are node k + 1's."""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from acinoset_amd import fte, synth
from acinoset_amd._lib import check, lib, ptr, stream_ptr
wg = int(sys.argv[1]) if len(sys.argv) > 1 else 100
kk = int(sys.argv[2]) if len(sys.argv) > 2 else 3
seq = synth.make_sequence(10000, "loop")
rig = (seq["K"], seq["D"], seq["R"], seq["t"])
det = torch.as_tensor(seq["det"], device="cuda")
x0 = fte.triangulation_init(det, *rig, 0.5)[:, fte.ACTIVE]
c = fte.FTEContext(det, *rig, seq["Ts"], ftol=0.0, xtol=0.0, gtol=0.0, clamp_lambda=True)
c.set_x(x0)
for _ in range(3):
    c.step()
dbg = torch.zeros(72, dtype=torch.int64, device="cuda")
dbg[64] = wg
dbg[65] = kk
check(lib().acino_fte_debug_stamps(c._h, ptr(dbg)))
c.step()
torch.cuda.synchronize()
d = dbg.cpu().numpy()
check(lib().acino_fte_debug_stamps(c._h, None))
c.close()
t0 = d[0] if d[0] else d[70]          # (node -1: no iteration is stamped)
names = {0: "D: iteration starts (loads of the next node requested)", 1: "D: U_k complete, strip waves through with Xg: queue of G_k opens",
         2: "D: G_k complete", 4: "D: next node built"}
for w in (0, 1, 5, 4):
    names[8 + w] = f"D wave {w}: node done"
    names[32 + w] = f"D wave {w}: its tiles of G_k done"
who = ["wave 2 (strip 1)", "wave 6 (strips 2, 0)", "wave 3 (strip 3)", "wave 7 (strip 4)"]
for r in range(4):
    names[16 + 4 * r] = f"S {who[r]}: G_k complete"; names[17 + 4 * r] = f"S {who[r]}: T = G F done"
    names[18 + 4 * r] = f"S {who[r]}: F^T T tiles done"; names[19 + 4 * r] = f"S {who[r]}: stencil done"
for kb in range(4):
    names[40 + 2 * kb] = f"chain: panel {kb} posted"; names[41 + 2 * kb] = f"chain: pivots {kb + 1} done"
    names[48 + kb] = f"helper L: trailing {kb}"; names[52 + kb] = f"helper U: trailing {kb}"; names[56 + kb] = f"helper L: starts trailing {kb}"
if d[63]:       # the last node of a run with a left separator: strips 3 and 0 are waves 0 and 1's (spike_node, roles 10 and 9; their
    #             stamps stand where the factorisation's would), wave 6 keeps strip 2 alone, wave 3 only computes its tiles of G_k
    for kb in range(4):
        for i in (40 + 2 * kb, 41 + 2 * kb, 48 + kb, 52 + kb, 56 + kb):
            del names[i]
    names[63] = "D waves 0, 1: take their strips (right separator built)"
    for base, w in ((20, "S wave 6 (strip 2 alone)"), (40, "D wave 1 (strip 0)"), (44, "D wave 0 (strip 3)")):
        names[base] = f"{w}: G_k complete, F_k complete, tiles of AL requested"; names[base + 1] = f"{w}: T = G F done"
        names[base + 2] = f"{w}: F^T T tiles done"; names[base + 3] = f"{w}: stencil done"
    names[20] = "S wave 6 (strip 2 alone): G_k complete"
    names[24] = "S wave 3 (no strip): G_k stored"
    names[62] = "node loop done (closing barrier passed)"
for i in sorted(names, key=lambda i: d[i]):
    if d[i]:
        print(f"{(d[i] - t0) / 100.0:8.2f} us  {names[i]}")
if d[70]:
    print(f"run-level (us from the workgroup's start): first node built {(d[60] - d[70]) / 100.0:.2f}, factored {(d[61] - d[70]) / 100.0:.2f}, "
          f"node loop done {(d[62] - d[70]) / 100.0:.2f}, workgroup done {(d[71] - d[70]) / 100.0:.2f}")
print("SIMD of waves 0..7:", [(int(d[67]) >> (4 * w)) & 3 for w in range(8)], " HW_ID of wave 0: %#x" % int(d[68]))
