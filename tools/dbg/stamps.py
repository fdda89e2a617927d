"""Per-phase s_memtime sums of the stage kernels: python tools/dbg/stamps.py [LABEL] > stamps.json
Needs tools/dbg/libexabm4d_stamps.so, a library built with -DEXABM4D_STAMPS (tools/dbg/build_variant.sh; the
stamp function itself is csrc/kernel_stamps.h), or the library EXABM4D_STAMPS_LIB names.  SIZE (default 512) is the cube's edge.  Nine slots per kernel."""
import os, sys, ctypes, json
os.environ["EXABM4D_LIB"] = os.environ.get("EXABM4D_STAMPS_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "libexabm4d_stamps.so")
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "aind-exaspim-image-compression_amd"))
from aind_exaspim_image_compression import _native as nat
import bench
ctx = nat.context(0)
shape = (int(os.environ.get("SIZE", "512")),)*3
vol = bench.synth_u16(shape, 1000)
d_in = ctx.to_device(vol); d_out = ctx.alloc(vol.nbytes)
L = ctypes.CDLL(os.environ["EXABM4D_LIB"])
NSLOT = 9
out = (ctypes.c_ulonglong*(2*NSLOT))()
ctx.denoise_u16(d_in, d_out, shape, 24.0, 37.0); ctx.sync()
L.exabm4d_debug_stamps(out, 1)
ctx.denoise_u16(d_in, d_out, shape, 24.0, 37.0); ctx.sync()
L.exabm4d_debug_stamps(out, 1)
# slot 7 is the wave's lifetime; slot 4 runs from the end of the inverse transforms to the last ring add of a
# block pair and so contains slot 3 (and, in the hard-threshold kernel, the planes flushed from the gate)
names = ["forward", "shrink_exchange", "exchange_wait", "gate_wait", "inverse_ring_adds", "ack_wait",
         "handout_wait", None, "close_flush"]
res = {"label": sys.argv[1] if len(sys.argv) > 1 else "", "volume": list(shape)}
for base, lab in ((0, "stage_ht"), (NSLOT, "stage_wie")):
    tot = out[base + 7]
    res[lab] = {"wave_cycles": tot,
                "share": {n: round(out[base + i] / tot, 4) for i, n in enumerate(names) if n}}
print(json.dumps(res, indent=1))
