"""Tile-band launches (vpt_gpu_render_tiles / Integrator.render_tiles): `waves` waves of a band of consecutive
tiles in one launch, the band's pixels receiving their samples in wave order.

The expected film of a band is the oracle's film of the jobs [wave_begin * T, (wave_begin + n) * T) (tests/
oracle_lib.py render_jobs: the restated worker loop, jid order) with every pixel outside the band's tiles set to
+0.0, channel 3 included -- compared BIT FOR BIT: on every kernel variant and both kernels (latency / throughput),
ragged tiles, a second wave group (66 waves), a launch that fills its grid, capped (split) launches, the
single-pixel mode, other tile sizes, and a frame cut into cost-balanced bands whose films sum exactly.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from volume_path_tracer_amd import capi
from volume_path_tracer_amd import distributed as D
from volume_path_tracer_amd.scenes import SynthGrid, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VPT_E_INVALID, VPT_E_STATE = 1, 6


def _grids(wl):
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    return dens, temp


def _oracle(dens, temp):
    return O.OracleGrid(dens, fix_majorants=True), (O.OracleGrid(temp, fix_majorants=False) if temp is not None else None)


def _assert_bitwise(a, b, what=""):
    diff = (a.view(np.uint32) != b.view(np.uint32)).any(axis=-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ"


def _wl(name, w, h, n, waves, tile=None, single_pixel=None):
    wl = workload(name, width=w, height=h, spp=waves, grid_n=n)
    if tile is not None:
        wl.cfg.tile_size[0], wl.cfg.tile_size[1] = tile
    if single_pixel is not None:
        wl.cfg.worker_parameters.single_pixel_enabled = 1
        wl.cfg.worker_parameters.single_pixel_coord[0] = single_pixel[0]
        wl.cfg.worker_parameters.single_pixel_coord[1] = single_pixel[1]
    return wl


@functools.lru_cache(maxsize=None)
def _reference(name, w, h, n, wave_begin, waves, tile=None, single_pixel=None):
    """The oracle's film of waves [wave_begin, wave_begin + waves) (0-based), computed once per case and shared."""
    wl = _wl(name, w, h, n, waves, tile, single_pixel)
    T = wl.cfg.jobs_per_wave()
    f, _, _ = O.render_jobs(wl.cfg, *_oracle(*_grids(wl)), wave_begin * T, waves * T)
    f.setflags(write=False)
    return f


def _band_mask(cfg, lo, hi):
    tw, th = int(cfg.tile_size[0]), int(cfg.tile_size[1])
    ntx = -(-cfg.width // tw)
    m = np.zeros((cfg.height, cfg.width), bool)
    for t in range(lo, hi):
        x0, y0 = (t % ntx) * tw, (t // ntx) * th
        m[y0:y0 + th, x0:x0 + tw] = True
    return m


def _expected(ref, cfg, lo, hi):
    e = np.zeros_like(ref)  # (+0.0 everywhere outside the band)
    m = _band_mask(cfg, lo, hi)
    e[m] = ref[m]
    return e


def _band_film(it, lo, hi, first_wave, waves, film=None):
    film = torch.zeros_like(it.film) if film is None else film
    it.render_tiles(lo, hi, first_wave, waves, film=film)
    torch.cuda.synchronize()
    return film.cpu().numpy()


CASES = [
    # (workload, width, height, grid_n, run_skipping, waves, band)
    ("c3", 48, 40, 64, 0, 6, (7, 19)),
    ("c3", 37, 29, 128, 0, 5, (3, 20)),    # ragged last column and row
    ("c2", 64, 48, 128, 1, 5, (10, 40)),   # C2's cube, run skipping
    ("c4", 40, 32, 64, -1, 5, (0, 11)),    # temperature kernel
]


@pytest.mark.parametrize("lat", [0, 1])
@pytest.mark.parametrize("name,w,h,n,runs,waves,band", CASES)
def test_band_film_bit_identical(name, w, h, n, runs, waves, band, lat):
    from volume_path_tracer_amd.render import Integrator

    wl = _wl(name, w, h, n, waves)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    it.set_latency_kernel(lat)
    if runs >= 0:
        it.set_run_skipping(runs)
    lo, hi = band
    assert hi <= wl.cfg.jobs_per_wave()
    before = it.film_order_info()["ordered_launches"]
    f_g = _band_film(it, lo, hi, 1, waves)
    exp = _expected(_reference(name, w, h, n, 0, waves), wl.cfg, lo, hi)
    np.testing.assert_array_equal(f_g[..., 3], np.where(_band_mask(wl.cfg, lo, hi), float(waves), 0.0))
    _assert_bitwise(f_g, exp, f"{name} band {band} lat {lat}")
    info = it.film_order_info()
    assert info["ordered_launches"] == before + 1 and info["atomic_launches"] == 0
    assert info["buffer_bytes"] >= (hi - lo) * 64 * 64 * 12  # one padded group of 64 waves


@pytest.mark.parametrize("lat", [0, 1])
def test_band_from_a_later_wave(lat):
    """first_wave = 3: every job keeps its jid ((wave - 1) * T + tile) and its RNG stream."""
    from volume_path_tracer_amd.render import Integrator

    name, w, h, n, _, waves, (lo, hi) = CASES[0]
    wl = _wl(name, w, h, n, waves)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    it.set_latency_kernel(lat)
    f_g = _band_film(it, lo, hi, 3, waves)
    _assert_bitwise(f_g, _expected(_reference(name, w, h, n, 2, waves), wl.cfg, lo, hi), "first_wave 3")


@pytest.mark.parametrize("fill", [False, True])
def test_second_wave_group(fill):
    """66 waves: one full group of 64 and a last group of 2 (padded); `fill`: one block, so the launch fills its
    grid and runs the throughput kernel, a wavefront's lanes on one tile's consecutive waves."""
    from volume_path_tracer_amd.render import Integrator

    wl = _wl("c3", 48, 40, 64, 66)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    if fill:
        it.set_tuning(grid_blocks=1)
    f_g = _band_film(it, 5, 25, 1, 66)
    _assert_bitwise(f_g, _expected(_reference("c3", 48, 40, 64, 0, 66), wl.cfg, 5, 25), f"66 waves fill {fill}")
    assert it.film_order_info()["buffer_bytes"] >= 20 * 2 * 64 * 64 * 12


def test_capped_at_whole_groups():
    """130 waves of two tiles under a cap of 100 waves: blocks of 64, 64 and 2 waves (multiples of 64 where the
    cap allows), three film passes in wave order."""
    from volume_path_tracer_amd.render import Integrator

    wl = _wl("c3", 48, 40, 64, 130)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    it.set_film_order(capi.VPT_FILM_ORDERED, 100 * 2 * 64 * 12)
    f_g = _band_film(it, 28, 30, 1, 130)
    _assert_bitwise(f_g, _expected(_reference("c3", 48, 40, 64, 0, 130), wl.cfg, 28, 30), "130 waves, cap 100")
    info = it.film_order_info()
    assert info["ordered_launches"] == 3 and info["buffer_bytes"] == 64 * 2 * 64 * 12


def test_cost_balanced_bands_sum_to_the_frame():
    """Three cost-balanced bands, each into its own zero film and summed in fp32 on the host (what the multi-GPU
    all-reduce does), and the same bands one after another into one device film: both are the one-launch
    render_jobs film and the oracle's, byte for byte."""
    from volume_path_tracer_amd.render import Integrator

    waves = 6
    wl = _wl("c3", 48, 40, 64, waves)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    T = wl.cfg.jobs_per_wave()
    cost, _ = it.tile_costs()
    cut = D.cost_bands(cost, 3)
    assert cut[0] == 0 and cut[-1] == T and [D.rank_tile_band(r, 3, cost) for r in range(3)] == list(zip(cut, cut[1:]))
    ref = _reference("c3", 48, 40, 64, 0, waves)
    total = np.zeros_like(ref)
    for lo, hi in zip(cut, cut[1:]):
        total = total + _band_film(it, lo, hi, 1, waves)  # fp32 adds
    one = torch.zeros_like(it.film)
    for lo, hi in zip(cut, cut[1:]):
        it.render_tiles(lo, hi, 1, waves, film=one)
    whole = torch.zeros_like(it.film)
    it.render_jobs(0, waves * T, film=whole)
    torch.cuda.synchronize()
    whole = whole.cpu().numpy()
    assert whole.tobytes() == ref.tobytes()
    assert total.tobytes() == ref.tobytes()
    assert one.cpu().numpy().tobytes() == ref.tobytes()
    # the whole frame as one band launch, too
    assert _band_film(it, 0, T, 1, waves).tobytes() == ref.tobytes()


@pytest.mark.parametrize("cap_waves,launches", [(2, 3), (4, 2)])
def test_capped_band_launch_is_split_by_waves(cap_waves, launches):
    """max_bytes = two waves of the band: 5 waves run as blocks of 2, 2 and 1 waves, each with its own film pass in
    wave order -- the same film, three ordered launches (groups of 2 and 1 waves: staged with 4-B loads).  Four
    waves: blocks of 4 and 1 (a group of 4: 16-B loads)."""
    from volume_path_tracer_amd.render import Integrator

    name, w, h, n, _, _, (lo, hi) = CASES[0]
    waves = 5
    wl = _wl(name, w, h, n, waves)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    it.set_film_order(capi.VPT_FILM_ORDERED, cap_waves * (hi - lo) * 64 * 12)
    before = it.film_order_info()["ordered_launches"]
    f_g = _band_film(it, lo, hi, 1, waves)
    _assert_bitwise(f_g, _expected(_reference(name, w, h, n, 0, waves), wl.cfg, lo, hi), "capped")
    info = it.film_order_info()
    assert info["ordered_launches"] == before + launches and info["buffer_bytes"] <= cap_waves * (hi - lo) * 64 * 12
    # not one wave of the band fits: VPT_E_NOMEM
    it.set_film_order(capi.VPT_FILM_ORDERED, (hi - lo) * 64 * 12 - 1)
    with pytest.raises(RuntimeError, match=r"\(5\)"):
        it.render_tiles(lo, hi, 1, waves)


def test_compacting_kernel_band():
    """Live-path compaction moves paths between threads; a band job's sample address travels in the cold state."""
    from volume_path_tracer_amd.render import Integrator

    wl = _wl("c2", 96, 96, 128, 3)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    it.set_latency_kernel(1, 0)
    it.set_tuning(grid_blocks=4)
    it.set_compaction(4)
    it.counters(reset=True)
    f_g = _band_film(it, 20, 130, 1, 3)
    assert it.counters()["exchanged"] > 0
    _assert_bitwise(f_g, _expected(_reference("c2", 96, 96, 128, 0, 3), wl.cfg, 20, 130), "compaction")


def test_bands_on_three_streams_share_one_film():
    """Band launches of different bands and wave blocks enqueued round-robin on three streams: they run one at a
    time in enqueue order (the context's sample buffer and tile-rank buffer are theirs in turn), so the film is
    the oracle's 4-wave film byte for byte."""
    from volume_path_tracer_amd.render import Integrator

    wl = _wl("c3", 96, 64, 64, 4)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    T = wl.cfg.jobs_per_wave()
    streams = [torch.cuda.Stream(device=it.dev) for _ in range(3)]
    film = torch.zeros_like(it.film)
    torch.cuda.synchronize()  # (the fill runs on the current stream)
    cuts = [0, 5, 6, 40, T - 1, T]
    i = 0
    for first in (1, 3):  # waves 1-2, then 3-4, of every band
        for lo, hi in zip(cuts, cuts[1:]):
            it.render_tiles(lo, hi, first, 2, film=film, stream=streams[i % 3])
            i += 1
    torch.cuda.synchronize()
    assert film.cpu().numpy().tobytes() == _reference("c3", 96, 64, 64, 0, 4).tobytes()


def test_single_pixel_band():
    """single_pixel mode (worker.cpp:113-116): a band that holds the pixel gives it `waves` samples, the oracle's
    bit for bit; a band that does not leaves the film all zero."""
    from volume_path_tracer_amd.render import Integrator

    waves, sp = 4, (13, 21)  # tile (21 // 8) * 5 + 13 // 8 = 11
    wl = _wl("c4", 40, 32, 64, waves, single_pixel=sp)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    ref = _reference("c4", 40, 32, 64, 0, waves, None, sp)
    f_in = _band_film(it, 8, 14, 1, waves)
    _assert_bitwise(f_in, ref, "single pixel in the band")
    assert f_in[21, 13, 3] == float(waves) and f_in[..., 3].sum() == float(waves)
    f_out = _band_film(it, 0, 11, 1, waves)
    assert f_out.tobytes() == np.zeros_like(f_out).tobytes()


@pytest.mark.parametrize("tile", [(4, 4), (12, 8)])
def test_other_tile_sizes(tile):
    """4 x 4 tiles (16 pixels: a quarter of the order pass's wavefront) and 12 x 8 (96: a second, half-filled
    block per tile), with ragged edges."""
    from volume_path_tracer_amd.render import Integrator

    waves = 5
    wl = _wl("c3", 37, 29, 64, waves, tile=tile)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    T = wl.cfg.jobs_per_wave()
    lo, hi = T // 4, T - 1
    f_g = _band_film(it, lo, hi, 1, waves)
    _assert_bitwise(f_g, _expected(_reference("c3", 37, 29, 64, 0, waves, tile), wl.cfg, lo, hi), f"tile {tile}")
    f_all = _band_film(it, 0, T, 1, waves)
    assert f_all.tobytes() == _reference("c3", 37, 29, 64, 0, waves, tile).tobytes()


def test_no_growth_while_a_feed_is_open():
    """A band launch whose sample buffer would have to grow while a feed of the context is launched and not closed
    returns VPT_E_STATE at once (freeing or allocating device memory could wait for the feed's launch); after the
    close the band renders, and the feed's film holds every pushed job."""
    from volume_path_tracer_amd.render import Integrator

    wl = _wl("c3", 64, 48, 64, 16)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    it.set_tuning(grid_blocks=2)  # 512 lanes: the feed launches once 512 of the 768 jobs are pushed
    it.tile_costs()  # (the cost pass refuses while a feed is open, too: done before)
    L = capi.lib()
    T = wl.cfg.jobs_per_wave()
    feed_film, band_film = torch.zeros_like(it.film), torch.zeros_like(it.film)
    torch.cuda.synchronize()
    s, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(feed_film.data_ptr()), s, 1024, C.byref(f)), "open")
    jids = np.arange(16 * T, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(f, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    assert it.film_order_info()["buffer_bytes"] == 0
    rc = L.vpt_gpu_render_tiles(it.h, 3, 20, 0, 16, C.c_void_p(band_film.data_ptr()), C.c_void_p(it.stream_handle()))
    assert rc == VPT_E_STATE and b"grow" in L.vpt_last_error()
    capi.check(L.vpt_gpu_feed_close(f), "close")
    capi.check(L.vpt_gpu_feed_destroy(f), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    ref = _reference("c3", 64, 48, 64, 0, 16)
    np.testing.assert_array_equal(feed_film.cpu().numpy()[..., 3], 16.0)
    assert band_film.cpu().numpy().tobytes() == np.zeros_like(ref).tobytes()  # the refused call rendered nothing
    _assert_bitwise(_band_film(it, 3, 20, 1, 16, film=band_film), _expected(ref, wl.cfg, 3, 20), "after the feed")


def test_errors_leave_the_context_usable():
    from volume_path_tracer_amd.render import Integrator

    name, w, h, n, _, waves, (lo, hi) = CASES[0]
    wl = _wl(name, w, h, n, waves)
    it = Integrator(wl.cfg, *_grids(wl), device=0)
    T = wl.cfg.jobs_per_wave()
    L = capi.lib()
    exp = _expected(_reference(name, w, h, n, 0, waves), wl.cfg, lo, hi)
    film = torch.zeros_like(it.film)
    fptr, s = C.c_void_p(film.data_ptr()), C.c_void_p(it.stream_handle())

    def call(a, b, w0=0, nw=waves):
        return L.vpt_gpu_render_tiles(it.h, a, b, w0, nw, fptr, s)

    def still_renders(what):
        _assert_bitwise(_band_film(it, lo, hi, 1, waves), exp, what)

    for a, b in ((5, 5), (7, 3), (0, T + 1), (T, T + 1)):
        assert call(a, b) == VPT_E_INVALID, (a, b)
        assert b"tile range" in L.vpt_last_error()
    still_renders("after bad tile ranges")
    assert call(lo, hi, 0, 1 << 32) == VPT_E_INVALID  # 2^32 or more slots
    it.set_rng_mode(capi.VPT_RNG_PIXEL)
    assert call(lo, hi) == VPT_E_INVALID
    it.set_rng_mode(capi.VPT_RNG_REFERENCE)
    still_renders("after the pixel RNG mode")
    it.set_film_order(capi.VPT_FILM_ATOMIC)
    assert call(lo, hi) == VPT_E_STATE and b"ordered film" in L.vpt_last_error()
    it.set_film_order(capi.VPT_FILM_ORDERED)
    still_renders("after the atomic film mode")
    granted = C.c_uint64(2)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open")
    assert granted.value == 2
    assert call(lo, hi) == VPT_E_STATE and b"frame" in L.vpt_last_error()
    granted = C.c_uint64(0)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open (close)")
    still_renders("after an open frame")
    launches = it.film_order_info()["ordered_launches"]
    assert call(lo, hi, 0, 0) == capi.VPT_OK  # wave_count 0: nothing
    torch.cuda.synchronize()
    assert it.film_order_info()["ordered_launches"] == launches
    assert film.cpu().numpy().tobytes() == np.zeros_like(exp).tobytes()  # no call above touched the film
    with pytest.raises(ValueError):
        it.render_tiles(lo, hi, 0, waves)  # waves are 1-based
    still_renders("at the end")
