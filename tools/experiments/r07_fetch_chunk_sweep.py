"""Timing sweep: fetch chunk x full-launch gate_idle on a config's full frame (one process, one context)."""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import torch

from volume_path_tracer_amd.render import Integrator
from volume_path_tracer_amd.scenes import SynthGrid, workload

config = sys.argv[1]
chunks = [int(x) for x in sys.argv[2].split(",")]
idles = [int(x) for x in sys.argv[3].split(",")]
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
wl = workload(config)
dg = SynthGrid(wl.density_kind, wl.grid_n)
tg = SynthGrid(2, wl.grid_n) if wl.temperature else None
it = Integrator(wl.cfg, dg.grid(copy=False), tg.grid(copy=False) if tg else None)
it.render_waves(1, wl.spp)
torch.cuda.synchronize()
for rnd in range(2):
    for gi in idles:
        for ch in chunks:
            it.set_full_tuning(gate_idle=gi)
            it.set_fetch_chunk(ch)
            ms = []
            for _ in range(reps):
                it.film.zero_()
                torch.cuda.synchronize()
                t = time.perf_counter()
                it.render_waves(1, wl.spp)
                torch.cuda.synchronize()
                ms.append(round((time.perf_counter() - t) * 1e3, 2))
            print(json.dumps({"config": config, "round": rnd, "gate_idle": gi, "chunk": ch, "ran": it.launch_info()[2], "ms": ms}),
                  flush=True)
