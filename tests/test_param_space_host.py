"""The scene-parameter space (tests/param_cases.py) on the CPU: the device state machine run through the host
simulator equals the oracle bit for bit on every case, and every case's conditions hold on the oracle's output --
so a GPU comparison on these inputs (tests/test_gpu_param_space.py) compares non-trivial work."""
import numpy as np
import pytest

import hostsim_lib as HS
import param_cases as P


@pytest.mark.parametrize("case_id", P.IDS)
def test_case_conditions_hold_on_the_oracle(case_id):
    P.check_case(case_id)


@pytest.mark.parametrize("case_id", P.IDS)
def test_host_simulator_equals_the_oracle(case_id):
    ref = P.reference(case_id)
    HS.walk_outside(reset=True)
    f_h, r_h, c_h = HS.render_jobs(ref.cfg, ref.dens, ref.temp, 0, ref.jobs, records=True)
    assert r_h.tobytes() == ref.rec.tobytes(), "per-sample radiance differs"
    assert f_h.tobytes() == ref.film.tobytes()
    for k in P.DEBUG_COUNTERS + (("temp_stencils",) if ref.temp is not None else ()):
        assert c_h[k] == ref.counters[k], (k, c_h[k], ref.counters[k])
    if P.BY_ID[case_id].group == "map":
        assert HS.walk_outside() == 0


def test_hot_case_on_the_host():
    """The `hot` case (part of the lookups at T >= 49 900 K, whose direct spectral integration is not bit-exact
    across builds): the case's conditions hold; the host simulator's counters are the oracle's; its samples
    without a hot lookup are the oracle's bytes -- which also checks the classification the GPU test relies on --
    and every word lies within 1e-6 (relative) of the oracle's."""
    ref = P.hot_reference()
    P.check_hot(ref)
    f_h, r_h, c_h = HS.render_jobs(ref.cfg, ref.dens, ref.temp, 0, ref.jobs, records=True)
    for k in P.DEBUG_COUNTERS + ("temp_stencils",):
        assert c_h[k] == ref.counters[k], k
    cold = ref.inside & ~ref.maybe_hot
    assert r_h[cold].tobytes() == ref.rec[cold].tobytes()
    np.testing.assert_allclose(r_h[ref.inside], ref.rec[ref.inside], rtol=1e-6, atol=0)
