"""The grid space: one table of small frames shared by tests/test_grid_space_host.py (oracle vs the host simulator)
and tests/test_gpu_grid_space.py (oracle vs every HIP kernel), the counterpart of tests/param_cases.py.

param_cases.py moves one scene parameter per case over the plain 64^3 cloud; here the scene stays c3 (density) or
c4 (density + temperature) and the GRID moves to what a real .nvdb file looks like and the other test grids do not:
a non-zero background (positive and negative), an index box that cuts leaves or reaches far into empty root space
and onto root tiles, leaves that straddle lower / upper / root node boundaries and the origin, index coordinates
of 2^16 .. 2^22 (float index positions with sub-voxel spacing, large table origins), inactive voxels that hold
values, denormal voxel values and majorants (bit patterns inside and outside the walk table's zero-run codes 1..63),
plus the hand-built grids of tests/grids.py (every HDDA level, tiles only, negative values, non-identity maps,
temperature grids of another map or topology) at this table's frame size.

A case is (id, build, group, check): build() -> (workload, density grid, temperature grid or None).  Every frame
is 24x16, 2 waves.  `check` holds the case's conditions: assertions on the ORACLE's output alone that make the case
mean something (the background was read, rays cross empty root space, the rounding differs from the plain cloud's);
reference(id) computes a case's oracle outputs once per process; reference_compact(id) the same scene at 96x72,
for the compacting latency kernel.
"""
from __future__ import annotations

import numpy as np

import grids as G
import hostsim_lib as HS
import oracle_lib as O
from param_cases import (DEBUG_COUNTERS, PRODUCTION_COUNTERS, WAVES, Case, Reference, check_common,  # noqa: F401
                         inside_rows)
from volume_path_tracer_amd.scenes import SynthGrid, workload

W, H = 24, 16
COMPACT_W, COMPACT_H = 96, 72       # T = 108 > 96: a partly filled launch that is not latency-bound
DENORMAL_MIN_NORMAL = np.float32(2.0 ** -126)
MAPPED_NEARER = 0.5


def _cloud():
    return SynthGrid(1, 64).grid(copy=True)


def _wl(name, w, h, n=64):
    return workload(name, width=w, height=h, spp=WAVES, grid_n=n)


def _density(make, camera=None):
    """A c3 case on the density grid make(); camera(cfg) moves the camera."""
    def build(w=W, h=H):
        wl = _wl("c3", w, h)
        if camera is not None:
            camera(wl.cfg)
        return wl, make(), None
    return build


# Three geometries are not the ones the cases' existing tests use, because at 24x16 those fail the conditions below
# on the oracle alone (EXPERIMENTS.md, the grid-space section, has the figures):
#   sparse    the camera stands at z = -600, not -700 (972 density evaluations there; > 1000 is asked);
#   mapped:*  the camera stands MAPPED_NEARER x 2.6 = 1.3 world extents from the centre, not 2.6 (641 / 773 / 916
#             evaluations there).  0.7 x 2.6 meets the conditions too, but at 96x72 the compacting latency kernel
#             then has nothing to exchange on small_voxels (`exchanged` 0 at every meeting period, measured);
#   temp:*    the camera is the c4 workload's own, not the oblique one of the 48x40 production test (44 scatters
#             there; > 100 is asked).
def _sparse_camera(cfg):
    G.look_at(cfg, (-40.0, -90.0, -600.0), (-40.0, -90.0, 10.0))
    cfg.camera_parameters.vfov_deg = 50.0


def _tiles_only_camera(cfg):
    G.look_at(cfg, (-500.0, 30.0, -300.0), (500.0, 30.0, 60.0))


def _mapped(name):
    _, scale, ang = next(c for c in G.MAPPED_CASES if c[0] == name)

    def build(w=W, h=H):
        wl = _wl("c3", w, h)
        G.mapped_scene(wl.cfg, MAPPED_NEARER * 64 * max(scale), 1.0 / min(scale))
        return wl, G.mapped_grid(scale, ang), None
    return build


LOOSE = dict(pad_lo=(20, 9, 30), pad_hi=(17, 40, 5))   # [5, 58]^3 -> [-15, 75] x [-4, 98] x [-25, 63]
ROOT_TILES = dict(tile_origin=[[-4096, 0, 0], [0, 0, -4096]], tile_level=[3, 3], tile_value=[0.05, 0.02],
                  tile_active=[1, 1])


def _far(e):
    return (2 ** e, -2 ** e, 2 ** e + 8)


def _root_edge(background):
    """The part x < 40 of the cloud with its cut face on the root-node boundary x = 4096 and no root entry beyond it
    (the index box goes on to 4114): the trilinear corners at x = 4096 of the dense voxels on the cut are lookups
    in root space without an entry, which return the background."""
    def make():
        base = _cloud()
        return G.moved(G.leaves_where(base, base.leaf_origin[:, 0] < 40), (4056, 0, 0), background=background)
    return make


def _temperature(kind, change=None):
    """A c4 case on grids.temperature_pair(kind); change(dens, temp) -> (dens, temp) replaces the grids."""
    def build(w=W, h=H):
        dens, temp = G.temperature_pair(kind)
        wl = _wl("c4", w, h)
        if change is not None:
            dens, temp = change(dens, temp)
        return wl, dens, temp
    return build


def _temp_background(dens, temp):
    return dens, G.with_bbox(G.with_background(temp, 0.3), (2, 3, 4), (59, 60, 61))


def _temp_no_background(dens, temp):
    return dens, G.with_bbox(temp, (2, 3, 4), (59, 60, 61))


def _temp_far(dens, temp):
    return G.moved(dens, _far(20)), G.moved(temp, _far(20))


# ---- conditions (on the oracle's output alone) ---------------------------------------------------------------
def _work(ref, reference):
    c = ref.counters
    assert c["density_evals"] > 1000 and c["scatters"] > 100, c


def _tiles_only(ref, reference):
    assert ref.counters["draws"] > 0, ref.counters


def _differs_from(other_id):
    """The records differ from those of the same case with background 0: the background was read."""
    def fn(ref, reference):
        _work(ref, reference)
        assert ref.rec.tobytes() != reference(other_id).rec.tobytes()
    return fn


def _negative_background(ref, reference):
    """Negative densities never collide: the counters are the plain cloud's."""
    _work(ref, reference)
    assert ref.counters == reference("cloud").counters


def _bbox_cut(ref, reference):
    _work(ref, reference)
    assert ref.counters["dda_steps"] != reference("cloud").counters["dda_steps"]


def _loose(other_id):
    def fn(ref, reference):
        _work(ref, reference)
        assert ref.counters["dda_steps"] > 1.5 * reference("cloud").counters["dda_steps"], ref.counters
        if other_id is not None:
            assert ref.rec.tobytes() != reference(other_id).rec.tobytes()
    return fn


def _root_edge_read(ref, reference):
    """Not one of the cases first asked for: it is the one whose results depend on the value a lookup returns in
    root space without an entry (cell_at's last line), which no other case's do (EXPERIMENTS.md, the self-check)."""
    _work(ref, reference)
    g = ref.dens
    assert g.leaf_origin[:, 0].max() == 4088 and ref.od.get_dim(4096, 4 + 32, 4 + 32) == 4096
    assert ref.od.get_value(4096, 36, 36) == np.float32(g.desc.background) != 0.0
    edge = g.leaf_origin[:, 0] == 4088
    assert (g.leaf_values[edge].reshape(-1, 8, 64)[:, 7].max(axis=1) > 0.5).sum() > 10   # dense voxels at x = 4095
    assert ref.rec.tobytes() != reference("root_edge").rec.tobytes()


def _straddle_origin(ref, reference):
    _work(ref, reference)
    cloud = reference("cloud")
    assert ref.counters == cloud.counters
    assert ref.rec.tobytes() != cloud.rec.tobytes()
    assert len(np.unique(ref.dens.leaf_origin >> 12, axis=0)) == 8      # eight upper nodes
    assert len(np.unique(ref.dens.leaf_origin >> 7, axis=0)) == 8       # eight lower nodes


def _straddle_4096(ref, reference):
    _work(ref, reference)
    o = ref.dens.leaf_origin
    assert len(np.unique(o[:, 0] >> 12)) == 2 and len(np.unique(o[:, 1] >> 7)) == 2 and (o[:, 2] < 0).any() \
        and (o[:, 2] >= 0).any()


def _far_away(ref, reference):
    """Index positions round differently 2^16 .. 2^22 voxels from the origin."""
    _work(ref, reference)
    assert ref.rec.tobytes() != reference("cloud").rec.tobytes()


def _inactive(ref, reference):
    _work(ref, reference)
    assert (ref.dens.leaf_value_mask[:, 1::2] == 0).all() and (ref.dens.leaf_values[:, 64:128] != 0).any()
    assert ref.rec.tobytes() == reference("cloud").rec.tobytes()


def _denormal(bits):
    """The fixed majorant of a leaf covers its +1 apron, so the slab's last layer of leaves (origin.x = 24) reads
    the first normal layer (origin.x = 32) and its fixed majorant is a normal float: "every slab leaf's fixed
    majorant is a zero-run code" can hold only for the slab leaves whose +x neighbour lies in the slab too (88 of
    the 140).  For :40 those are all codes (bit patterns <= 63) or zero, and the last layer's are all normal: code
    majorants and normal ones meet inside the slab."""
    def fn(ref, reference):
        _work(ref, reference)
        g = ref.dens
        x = g.leaf_origin[:, 0]
        tiny = (g.leaf_max[x < 32] > 0) & (g.leaf_max[x < 32] < DENORMAL_MIN_NORMAL)
        assert tiny.any(), "no slab leaf has a denormal leaf_max"
        if bits == 40:
            fixed = HS.fixed_leaf_max(g)
            assert (x < 24).sum() > 50 and (fixed[x < 24].view(np.uint32) <= 63).all()
            assert (fixed[x < 24] > 0).any() and (fixed[x == 24] >= DENORMAL_MIN_NORMAL).all()
        assert ref.counters["draws"] != reference("cloud").counters["draws"]
    return fn


def _emission(other_id=None):
    def fn(ref, reference):
        _work(ref, reference)
        assert ref.counters["temp_stencils"] > 100, ref.counters
        assert (ref.rec[ref.inside][:, 1] > ref.env()[1]).any(), "no emission reached the film"
        if other_id is not None:
            assert ref.rec.tobytes() != reference(other_id).rec.tobytes()
    return fn


def _cases():
    out = [
        Case("sparse", _density(G.sparse_grid, _sparse_camera), "hand-built", check=_work),
        Case("tiles_only", _density(G.tiles_only_grid, _tiles_only_camera), "hand-built", check=_tiles_only),
        Case("signed", _density(G.signed_grid), "hand-built", check=_work),
    ]
    out += [Case(f"mapped:{name}", _mapped(name), "mapped", check=_work) for name, _, _ in G.MAPPED_CASES]
    out += [
        Case("background=+0.05", _density(lambda: G.with_background(_cloud(), 0.05)), "background",
             check=_differs_from("cloud")),
        Case("background=-0.05", _density(lambda: G.with_background(_cloud(), -0.05)), "background",
             check=_negative_background),
        Case("bbox_cut", _density(lambda: G.with_bbox(_cloud(), (13, 10, 21), (50, 53, 44))), "bbox", check=_bbox_cut),
        Case("bbox_loose+background", _density(lambda: G.moved(_cloud(), 0, background=0.04, **LOOSE)), "bbox",
             check=_loose("bbox_loose")),
        Case("bbox_loose+root_tiles", _density(lambda: G.moved(_cloud(), 0, tiles=ROOT_TILES, **LOOSE)), "bbox",
             check=_loose(None)),
        Case("root_edge+background", _density(_root_edge(0.05)), "bbox", check=_root_edge_read),
        Case("straddle_origin", _density(lambda: G.moved(_cloud(), (-32, -32, -32))), "straddle",
             check=_straddle_origin),
        Case("straddle_4096", _density(lambda: G.moved(_cloud(), (4072, 88, -8))), "straddle", check=_straddle_4096),
    ]
    out += [Case(f"far=2^{e}", _density(lambda e=e: G.moved(_cloud(), _far(e))), "far", check=_far_away)
            for e in (16, 20, 22)]
    out.append(Case("inactive_half", _density(lambda: G.inactive_half(_cloud())), "inactive", check=_inactive))
    out += [Case(f"denormal:{name}", _density(lambda b=b: G.denormal_slab(_cloud(), b)), "denormal", check=_denormal(b))
            for name, b in (("40", 40), ("5000", 5000), ("max", 0x7FFFFF))]
    out += [Case(f"temp:{kind}", _temperature(kind), "temperature", check=_emission())
            for kind in ("same", "shifted", "half_voxels", "sparse")]
    out.append(Case("temp:background", _temperature("shifted", _temp_background), "temperature",
                    check=_emission("temp:no_background")))
    out.append(Case("temp:far", _temperature("same", _temp_far), "temperature", check=_emission()))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
IDS = [c.id for c in CASES]
DENSITY_IDS = [c.id for c in CASES if c.group != "temperature"]

# What the conditions compare against; not cases of the table (the plain cloud is param_cases' base scene).
BASELINES = {
    "cloud": Case("cloud", _density(_cloud), "baseline"),
    "bbox_loose": Case("bbox_loose", _density(lambda: G.moved(_cloud(), 0, **LOOSE)), "baseline"),
    "root_edge": Case("root_edge", _density(_root_edge(0.0)), "baseline"),
    "temp:no_background": Case("temp:no_background", _temperature("shifted", _temp_no_background), "baseline"),
}

# The gang kernel, the pixel-RNG kernel, the band kernel, the compacting latency kernel and the feed kernel run these.
# (`sparse` was among them and left: with its 2.8 GB dense pool and 8 680 leaves its case took 0.53 - 0.68 s on an
# MI355X, more than twice the slowest case of test_gpu_param_space.py, 0.24 s; without these steps it takes 0.34 s.)
EXTRA_IDS = ["tiles_only", "signed", "mapped:small_voxels", "background=+0.05", "bbox_loose+root_tiles",
             "straddle_4096", "far=2^20", "denormal:40", "temp:shifted", "temp:background"]
assert all(i in BY_ID for i in EXTRA_IDS)

_REF: dict = {}
_REF_COMPACT: dict = {}


def reference(case_id: str) -> Reference:
    if case_id not in _REF:
        _REF[case_id] = Reference(BY_ID[case_id] if case_id in BY_ID else BASELINES[case_id])
    return _REF[case_id]


class CompactReference:
    """A case's scene at 96x72 and the oracle's film of each of its first WAVES waves alone, with the production
    counters summed over them (the compacting latency kernel's frame)."""

    def __init__(self, case: Case):
        self.wl, self.dens, self.temp = case.build(COMPACT_W, COMPACT_H)
        self.cfg = self.wl.cfg
        od = O.OracleGrid(self.dens, fix_majorants=True)
        ot = O.OracleGrid(self.temp, fix_majorants=False) if self.temp is not None else None
        self.T = self.cfg.jobs_per_wave()
        runs = [O.render_jobs(self.cfg, od, ot, w * self.T, self.T) for w in range(WAVES)]
        self.wave_films = [r[0] for r in runs]
        self.counters = {k: sum(r[2][k] for r in runs) for k in PRODUCTION_COUNTERS}


def reference_compact(case_id: str) -> CompactReference:
    """The second cached reference: the case at 96x72."""
    if case_id not in _REF_COMPACT:
        _REF_COMPACT[case_id] = CompactReference(BY_ID[case_id])
    return _REF_COMPACT[case_id]


def check_case(case_id: str) -> Reference:
    """Evaluates the case's conditions on the oracle's output; returns the reference."""
    ref = reference(case_id)
    check_common(ref)
    assert (ref.cfg.width, ref.cfg.height) == (W, H)
    BY_ID[case_id].check(ref, reference)
    return ref
