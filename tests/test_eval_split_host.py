"""The split density evaluation on the CPU (no GPU): tests/native/eval_split_host.cpp runs lane_iteration with one lane
in two environments that differ only in Env::kEvalSplit -- the evaluation whole at the end of an iteration, or
eval_issue at the top and eval_finish in front of the ray block.  A lane's own order of operations and draws must not
depend on it: per-sample records, every debug counter and the lane's final RNG state are identical between the two,
and equal to the oracle's.  Host grids have no direct-addressed pool, so this covers the state machine (gates at 1:
every parked collision is issued at once) and eval_finish's lookup path; the loads are the GPU tests'."""
import numpy as np
import pytest

import eval_split_lib as ES
import oracle_lib as O
from volume_path_tracer_amd.scenes import SynthGrid, workload

WAVES = 3
COUNTERS = ("samples", "dda_steps", "segments", "draws", "stencils", "density_evals", "temp_stencils", "scatters",
            "shadow_rays", "rng_draws")
M64 = (1 << 64) - 1


def job_seed(seed, k):
    """vpt_integrator.h job_seed: hash(seed, jid) | 3, pcg32_fast's seeding."""
    m = 0xc6a4a7935bd1e995
    h = (seed ^ (8 * m)) & M64
    k = (k * m) & M64
    k ^= k >> 47
    k = (k * m) & M64
    h ^= k
    h = (h * m) & M64
    h ^= h >> 47
    h = (h * m) & M64
    h ^= h >> 47
    return h | 3


# (workload, run skipping): the 64^3 cloud, the 64^3 constant cube on the run-skipping walk, the fire scene
SCENES = [("c3", 0), ("c2", 1), ("c4", 0)]


@pytest.mark.parametrize("name,runs", SCENES)
def test_split_and_whole_equal_the_oracle(name, runs):
    wl = workload(name, width=24, height=16, spp=WAVES, grid_n=64)
    jobs = wl.cfg.jobs_per_wave() * WAVES
    dens = SynthGrid(wl.density_kind, 64).grid()
    temp = SynthGrid(2, 64).grid() if wl.temperature else None
    od = O.OracleGrid(dens, fix_majorants=True)
    ot = O.OracleGrid(temp, fix_majorants=False) if temp is not None else None
    f_o, r_o, c_o = O.render_jobs(wl.cfg, od, ot, 0, jobs, records=True)
    # the oracle's final RNG state: the last job's stream advanced by that job's draws (pcg32_fast: state *= M per draw)
    _, _, c_last = O.render_jobs(wl.cfg, od, ot, jobs - 1, 1, records=True)
    rng_o = (job_seed(int(wl.cfg.seed), jobs - 1) * pow(6364136223846793005, c_last["rng_draws"], 1 << 64)) & M64
    out = {split: ES.render_jobs(wl.cfg, dens, temp, 0, jobs, split, runs) for split in (0, 1)}
    for split, (f, r, c, rng) in out.items():
        assert np.array_equal(r.view(np.uint32), r_o.view(np.uint32)), ("per-sample records differ", split)
        assert np.array_equal(f.view(np.uint32), f_o.view(np.uint32)), ("film differs", split)
        for k in COUNTERS:
            assert c[k] == c_o[k], (k, split, c[k], c_o[k])
        assert rng == rng_o, ("final RNG state", split, hex(rng), hex(rng_o))
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3]
    assert c_o["samples"] == 24 * 16 * WAVES and c_o["density_evals"] > 100
    if wl.temperature:
        assert c_o["temp_stencils"] > 0
