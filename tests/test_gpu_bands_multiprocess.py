"""The multi-GPU `bands` mode with the HIP integrator in every rank: 2 processes on the box's one GPU,
torch.distributed over gloo, each rendering all spp waves of its cost-balanced band of tiles with one band launch
(distributed.render_rank, mode "bands") and summing the films with distributed.reduce_film.  Unlike the wave
shares (tests/test_gpu_multiprocess.py: rtol 1e-5), the reduced film is the oracle's BYTE FOR BYTE: each pixel is
one rank's wave-ordered sum plus +0.0 from the other."""
import json
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
from conftest import assert_hip_untouched
from volume_path_tracer_amd import distributed as D
from volume_path_tracer_amd.scenes import SynthGrid, workload

ROOT = Path(__file__).resolve().parents[1]
pytestmark = [pytest.mark.gpu, pytest.mark.spawns]

W, H, GRID = 64, 40, 64


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, spp, out_dir):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import torch
    import torch.distributed as dist

    from volume_path_tracer_amd import distributed as D
    from volume_path_tracer_amd.render import Integrator
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    wl = workload("c3", width=W, height=H, spp=spp, grid_n=GRID)
    it = Integrator(wl.cfg, SynthGrid(1, GRID).grid(), None, device=0)
    cost, _ = it.tile_costs()
    (band,) = D.render_rank(it, rank, world, spp, "bands")
    D.reduce_film(it.film)
    torch.cuda.synchronize()
    info = {"band": list(band), "own_cut": D.cost_bands(cost, world),
            "ordered_launches": it.film_order_info()["ordered_launches"]}
    (Path(out_dir) / f"rank{rank}.json").write_text(json.dumps(info))
    if rank == 0:
        np.save(Path(out_dir) / "reduced.npy", it.film.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_hip_integrator_world2_gloo_bands(tmp_path):
    import torch.multiprocessing as mp

    assert_hip_untouched()
    spp, world = 4, 2
    mp.start_processes(_worker, args=(world, _free_port(), spp, str(tmp_path)), nprocs=world, start_method="spawn")
    got = np.load(tmp_path / "reduced.npy")
    assert D.total_samples_per_pixel(world, spp, "bands") == spp
    wl = workload("c3", width=W, height=H, spp=spp, grid_n=GRID)
    T = wl.cfg.jobs_per_wave()
    ref, _, _ = O.render_jobs(wl.cfg, O.OracleGrid(SynthGrid(1, GRID).grid()), None, 0, T * spp)
    np.testing.assert_array_equal(got[..., 3], 4.0)
    assert got.tobytes() == ref.tobytes()
    r0, r1 = (json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(world))
    # rank 1 rendered rank 0's broadcast cut: the two bands meet and cover the frame
    cut0 = r0["own_cut"]
    assert r0["band"] == [cut0[0], cut0[1]] and r1["band"] == [cut0[1], cut0[2]] and cut0[0] == 0 and cut0[2] == T
    assert r0["ordered_launches"] == 1 and r1["ordered_launches"] == 1
