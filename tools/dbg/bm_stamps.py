"""Per-phase s_memtime sums of bm_tile16_kernel: python tools/dbg/bm_stamps.py LIB [SIZE] [LABEL] [LAYOUT] > stamps.json
LIB is a library built with -DEXABM4D_BM_STAMPS (tools/dbg/build_variant.sh bmstamps -DEXABM4D_BM_STAMPS; the
stamp function itself is csrc/kernel_stamps.h.  The forms of before DESIGN.md 5.2o and 5.2r, whose stamps are
profiles/*/bm_stamps_parent.json, are in the history: docs/DESIGN_HISTORY.md, "Retired A/B switches").  One SIZE^3 uint16 launch after a warm-up launch.  "barriers_by_wave": the
exchange-barrier slot per wave index and per barrier of a (dz, pass) -- the wave that waits least arrived last.
LAYOUT = BARRIERSxWAVES of the library's barrier array: 6x12 (default: up to three exchange rounds, twelve waves,
DESIGN.md 5.2s) or 4x8 for a library built from a commit before that.  The launch runs in the geometry the plan
chooses; EXABM4D_BM_LAYERS=8 / 12 in the environment forces one (option bm_layers)."""
import os, sys, ctypes, json, numpy as np
os.environ["EXABM4D_LIB"] = os.path.abspath(sys.argv[1])
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "aind-exaspim-image-compression_amd"))
from aind_exaspim_image_compression import _native as nat
import bench
size = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
ctx = nat.context(0)
shape = (size,) * 3
d = ctx.to_device(bench.synth_u16(shape, 1000))
g = [len(nat.grid_positions(n)) for n in shape]
k = ctx.alloc(g[0] * g[1] * g[2] * 64)
L = ctypes.CDLL(os.environ["EXABM4D_LIB"])
out = (ctypes.c_ulonglong * 8)()
NB, NW = (int(t) for t in (sys.argv[4] if len(sys.argv) > 4 else "6x12").split("x"))
bar = (ctypes.c_ulonglong * (NB * NW))()
if os.environ.get("EXABM4D_BM_LAYERS"):
    ctx.set_option("bm_layers", int(os.environ["EXABM4D_BM_LAYERS"]))
for i in range(2):
    ctx.blockmatch_u16(d, shape, 24.0, 3.0, k); ctx.sync()
    L.exabm4d_debug_bm_stamps(out, 1)
    L.exabm4d_debug_bm_barrier_stamps(bar, 1)
# barriers and waves the launch used: the rest of the array stayed zero
used_b = max([b + 1 for b in range(NB) if any(bar[NW * b + w] for w in range(NW))] or [0])
used_w = max([w + 1 for w in range(NW) if any(bar[NW * b + w] for b in range(NB))] or [0])
bnames = [f"round {b // 2 + 1}, {('in front of', 'behind')[b & 1]} selection" for b in range(used_b)]
by_wave = {n: [round(bar[NW * b + w] / out[7], 5) for w in range(used_w)] for b, n in enumerate(bnames)}
by_wave["all"] = [round(sum(bar[NW * b + w] for b in range(used_b)) / out[7], 5) for w in range(used_w)]
names = ["top_wait", "cell_plane_wait", "window_wait", "accumulate", "exchange_barriers", "selection", "carry_waits"]
share = {n: round(out[i] / out[7], 4) for i, n in enumerate(names)}
share["other"] = round(1.0 - sum(share.values()), 4)
print(json.dumps({
    "what": "Diagnostic build (-DEXABM4D_BM_STAMPS: s_memtime sums over all waves of bm_tile16_kernel; slower than the "
            "plain build), one blockmatch_u16 launch after a warm-up launch.  share = fraction of the summed wave "
            "lifetimes.  top_wait: vmcnt(0) at the top of a step; cell_plane_wait: loading and awaiting the cell's "
            "own plane inside the step (nothing in the hand-waited form, which loads it a step ahead); window_wait: "
            "from the issue of the next plane to the arrival of the first window row; other: issuing the DMA, "
            "publishing sums, carry stores, prologue and table store.",
    "build": sys.argv[3] if len(sys.argv) > 3 else os.path.basename(sys.argv[1]),
    "volume": list(shape), "wave_cycles": int(out[7]), "share": share,
    "memory_waits": round(share["top_wait"] + share["cell_plane_wait"] + share["window_wait"], 4),
    "waves_per_workgroup": used_w, "barriers_per_pass": used_b,
    "barriers_by_wave": {"what": "share of the summed wave lifetimes (all waves) spent in each barrier, by wave "
                                 "index; a row sums to that barrier's part of exchange_barriers",
                         **by_wave}}, indent=1))
for n, row in by_wave.items():
    print(f"{n:32s}" + " ".join(f"{100 * v:6.2f}" for v in row) + f"   % of wave time, waves 0..{used_w - 1}", file=sys.stderr)
