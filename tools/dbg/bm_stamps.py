"""Per-phase s_memtime sums of bm_tile16_kernel: python tools/dbg/bm_stamps.py LIB [SIZE] [LABEL] > stamps.json
LIB is a library built with -DEXABM4D_BM_STAMPS (tools/dbg/build_variant.sh bmstamps -DEXABM4D_BM_STAMPS; add
-DEXABM4D_BM_HANDWAIT=0 for the form whose waits hipcc places).  One SIZE^3 uint16 launch after a warm-up launch."""
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
for i in range(2):
    ctx.blockmatch_u16(d, shape, 24.0, 3.0, k); ctx.sync()
    L.exabm4d_debug_bm_stamps(out, 1)
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
    "memory_waits": round(share["top_wait"] + share["cell_plane_wait"] + share["window_wait"], 4)}, indent=1))
