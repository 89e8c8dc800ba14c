"""Light groups on the CPU: the device state machine with a groups Env (tests/native/light_groups_host.cpp) against the
oracle's isolated films (tests/light_groups_lib.py isolated_oracle).

Held byte for byte, modulo the sign of a zero: the three per-sample group records, the plain film pass in wave order
over them, and the band layout's pass -- each plane is the film the oracle renders with the other two sources off.  The
beauty samples and film stay the oracle's bit for bit.  scenes.light_gains and image.relight are checked here too: they
need no device.
"""
import numpy as np
import pytest

import light_groups_lib as LG
from volume_path_tracer_amd import image
from volume_path_tracer_amd.scenes import SynthGrid, light_gains, workload

# (workload, width, height, waves, band group): ragged tiles; a partly filled band group; more than one group of 64
CASES = [("c4", 16, 16, 4, 64), ("c3", 16, 16, 4, 64), ("c4", 20, 12, 3, 3), ("c3", 20, 12, 3, 64), ("c3", 16, 8, 70, 64),
         ("c4", 16, 8, 70, 64)]
_cache = {}


def _case(name, w, h, waves, G):
    key = (name, w, h, waves, G)
    if key not in _cache:
        wl = workload(name, width=w, height=h, spp=waves, grid_n=64)
        dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
        temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
        T = wl.cfg.jobs_per_wave()
        iso = LG.isolated_oracle(wl.cfg, dens, temp, 0, waves * T)
        host = LG.host_render_waves(wl.cfg, dens, temp, 0, waves, G)
        _cache[key] = (wl.cfg, iso, host)
    return _cache[key]


@pytest.mark.parametrize("name,w,h,waves,G", CASES)
def test_group_records_are_the_isolated_oracle_samples(name, w, h, waves, G):
    cfg, iso, (film, plain, band, cnt) = _case(name, w, h, waves, G)
    assert cnt == iso["counters"]
    # the beauty: untouched by the groups, the oracle's bit for bit
    assert np.array_equal(np.nan_to_num(plain[0], nan=-1.0).view(np.uint32),
                          np.nan_to_num(iso["rec"], nan=-1.0).view(np.uint32))
    assert np.array_equal(film.view(np.uint32), iso["film"].view(np.uint32))
    sampled = ~np.isnan(iso["rec"][:, 0])  # (a ragged tile's missing pixels hold no sample)
    assert sampled.any()
    for g, what in enumerate(LG.GROUPS):
        got, want = plain[1 + g], iso["group_recs"][g]
        assert np.array_equal(np.isnan(got[:, 0]), ~sampled), what
        assert LG.same_but_zero_sign(got[sampled], want[sampled]), f"{what}: per-sample records differ from the isolated oracle's"
    if name == "c4":
        assert (plain[1][sampled] != 0).any(), "the fire stand-in emits"
    assert (plain[2][sampled] != 0).any() and (plain[3][sampled] != 0).any()


@pytest.mark.parametrize("name,w,h,waves,G", CASES)
def test_film_passes_over_both_layouts_are_the_isolated_oracle_films(name, w, h, waves, G):
    cfg, iso, (film, plain, band, cnt) = _case(name, w, h, waves, G)
    assert np.array_equal(LG.film_pass_plain(cfg, plain[0], waves).view(np.uint32), iso["film"].view(np.uint32))
    assert np.array_equal(LG.film_pass_band(cfg, band[0], waves, G).view(np.uint32), iso["film"].view(np.uint32))
    for g, what in enumerate(LG.GROUPS):
        want = iso["group_films"][g]
        assert LG.same_but_zero_sign(LG.film_pass_plain(cfg, plain[1 + g], waves), want), f"{what}: plain pass"
        assert LG.same_but_zero_sign(LG.film_pass_band(cfg, band[1 + g], waves, G), want), f"{what}: band pass"
        assert (want[..., 3] == waves).all()


def test_sum_of_the_groups_is_the_beauty_to_rounding():
    """Not the parity check: fp32 addition does not associate, so the sum is the beauty only to a few ulp."""
    cfg, iso, (film, plain, band, cnt) = _case(*CASES[0])
    s = plain[1:].astype(np.float64).sum(axis=0)
    b = plain[0].astype(np.float64)
    ok = ~np.isnan(b)
    assert np.all(np.abs(s[ok] - b[ok]) <= 1e-3 * np.abs(b[ok]))


def test_relight_numpy_order_and_unit_gains():
    rng = np.random.default_rng(7)
    g = rng.standard_normal((3, 5, 7, 4)).astype(np.float32)
    g[:, 0, 0] = 0.0
    g[0, 1, 1, 3] = 0.0
    k = np.array([[0.3, 1.7, 2.9], [1.1, 0.7, 0.2], [5.0, 0.9, 1.3]], np.float32)
    out = image.relight(g, k)
    want = np.empty((5, 7, 4), np.float32)
    for c in range(3):
        want[..., c] = ((g[0, ..., c] * k[0, c]) + (g[1, ..., c] * k[1, c])) + (g[2, ..., c] * k[2, c])
    want[..., 3] = g[0, ..., 3]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        image.relight(g[:2], k)


def test_light_gains():
    cfg = workload("c4", width=16, height=16, spp=2, grid_n=64).cfg
    want = cfg.copy()
    want.worker_parameters.distant_light_multiplier = cfg.worker_parameters.distant_light_multiplier * 2
    want.worker_parameters.infinite_light_multiplier = cfg.worker_parameters.infinite_light_multiplier * 0.5
    want.volume_parameters.le_scale = cfg.volume_parameters.le_scale * 4
    k = light_gains(cfg, want)
    assert k.dtype == np.float32 and np.array_equal(k, np.array([[4, 4, 4], [2, 2, 2], [0.5, 0.5, 0.5]], np.float32))
    assert np.array_equal(light_gains(cfg, cfg), np.ones((3, 3), np.float32))
    tint = cfg.copy()
    tint.worker_parameters.infinite_light_xyz[1] = cfg.worker_parameters.infinite_light_xyz[1] * 3
    assert np.array_equal(light_gains(cfg, tint)[2], np.array([1, 3, 1], np.float32))
    off = cfg.copy()
    off.worker_parameters.distant_light_multiplier = 0.0
    assert np.array_equal(light_gains(cfg, off)[1], np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        light_gains(off, cfg)  # rendered at zero, wanted not
    assert np.array_equal(light_gains(off, off), np.ones((3, 3), np.float32))
    for change in ("seed", "g", "depth", "camera", "sun_dir", "temp", "size", "sigma"):
        other = cfg.copy()
        if change == "seed":
            other.seed = cfg.seed + 1
        elif change == "g":
            other.volume_parameters.henyey_greenstein_g = 0.123
        elif change == "depth":
            other.worker_parameters.max_depth = cfg.worker_parameters.max_depth + 1
        elif change == "camera":
            other.camera_parameters.position[0] = 3.0
        elif change == "sun_dir":
            other.worker_parameters.distant_light_inv_direction[0] = 0.77
        elif change == "temp":
            other.volume_parameters.temperature_scale = cfg.volume_parameters.temperature_scale * 2
        elif change == "size":
            other.output_size[0] = 32
        else:
            other.volume_parameters.sigma_a = cfg.volume_parameters.sigma_a + 1
        with pytest.raises(ValueError):
            light_gains(cfg, other)
