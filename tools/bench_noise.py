"""The noise table on a resident volume, against the uint16 histogram of the same volume in the same process.

usage: python tools/bench_noise.py [edge=1024] [runs=15] [out.json]
Both kernels read the volume once (2 bytes per voxel); the histogram makes eight updates per eight voxels where the
noise table makes one.  Times come from events on the context's stream around a single call (which ends in the
table's copy to the host and a synchronise), after warm-up, alternating the two; the median of `runs` is reported.
Prints one JSON line and, with a third argument, writes it to that file."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aind-exaspim-image-compression_amd"))
sys.path.insert(0, ROOT)

from aind_exaspim_image_compression import _native  # noqa: E402
from aind_exaspim_image_compression.utils import noise  # noqa: E402
from bench import synth_u16  # noqa: E402

HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E specification


def main():
    edge = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    runs = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 15
    shape = (edge,) * 3
    n = edge ** 3
    ctx = _native.context(0)
    vol = synth_u16(shape, 1)
    d_vol = ctx.to_device(vol)
    e0, e1 = ctx.event(), ctx.event()

    def once(fn):
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1)

    calls = {
        "noise_table": lambda: ctx.noise_table(d_vol, np.uint16, shape, 0),
        "u16_histogram": lambda: ctx.u16_histogram(d_vol, n),
    }
    for _ in range(3):
        for fn in calls.values():
            fn()
    ctx.sync()
    ms = {name: [] for name in calls}
    for _ in range(runs):
        for name, fn in calls.items():
            ms[name].append(once(fn))
    med = {name: statistics.median(v) for name, v in ms.items()}
    table = noise.noise_table(d_vol, shape=shape, dtype=np.uint16)
    levels = int(np.count_nonzero(table.counts))
    out = {
        "edge": edge,
        "runs": runs,
        "noise_table_ms": med["noise_table"],
        "noise_table_ms_min_max": [min(ms["noise_table"]), max(ms["noise_table"])],
        "u16_histogram_ms": med["u16_histogram"],
        "u16_histogram_ms_min_max": [min(ms["u16_histogram"]), max(ms["u16_histogram"])],
        "ratio_noise_over_histogram": med["noise_table"] / med["u16_histogram"],
        "algorithmic_bytes_per_voxel": 2,
        "noise_table_GBps": 2 * n / med["noise_table"] / 1e6,
        "u16_histogram_GBps": 2 * n / med["u16_histogram"] / 1e6,
        "noise_table_fraction_of_hbm_peak": 2 * n / med["noise_table"] / 1e6 / HBM_PEAK_GBPS,
        "hbm_peak_GBps": HBM_PEAK_GBPS,
        "timed": "one C-ABI call each, events on the context's stream: memset + kernel + copy of the table to the host",
        "levels_populated": levels,
        "levels_beyond_the_8_lds_slots": max(0, levels - 8),
        "sigma": table.pooled_sigma(),
        "shift": table.shift,
    }
    d_vol.free()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
        with open(sys.argv[3], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
