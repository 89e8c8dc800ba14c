// light_groups_host.cpp — TEST HARNESS: the device state machine (vpt_integrator.h lane_iteration) on the CPU, one lane,
// in an environment with light groups (Env::kGroups): hostsim.cpp's HostEnv plus the three per-source accumulators,
// stated the way include/vpt_gpu.h states them (E + sc * XYZ, D + pt * Li, D + 0.0f, le_inf iff ST_FINISH), and the
// two sample layouts a launch with groups writes -- four regions of the plain layout and four of the band layout
// (band_slot).  tests/test_light_groups_host.py holds the records and the film passes restated over them to the
// oracle's isolated films.  Not part of the product.
#include "hostsim.cpp"

namespace {
struct GroupsEnv : HostEnv {
  static constexpr bool kGroups = true;
  float E[3] = {0, 0, 0}, D[3] = {0, 0, 0};
  bool has_temp = false;
  // plain layout: region g (0 beauty, 1 emission, 2 sun, 3 sky) at plain + g * plain_stride
  float* plain = nullptr;
  uint64_t plain_stride = 0;
  // band layout over all T tiles: the same regions, band_stride floats apart
  float* band = nullptr;
  uint64_t band_stride = 0;
  uint32_t T = 0, groups = 0, G = 0;
  uint64_t wave0 = 0;
  void group_begin() {
    for (int c = 0; c < 3; ++c) E[c] = D[c] = 0.0f;
  }
  void group_emit(float sc, float X, float Y, float Z) {
    E[0] = E[0] + sc * X;
    E[1] = E[1] + sc * Y;
    E[2] = E[2] + sc * Z;
  }
  void group_sun(float pt, float l0, float l1, float l2) {
    D[0] = D[0] + pt * l0;
    D[1] = D[1] + pt * l1;
    D[2] = D[2] + pt * l2;
  }
  void group_sun_zero() {
    for (int c = 0; c < 3; ++c) D[c] = D[c] + 0.0f;
  }
  void film_add(const vpt::DevScene& S, const vpt::Lane& ln, int32_t px, int32_t py, int32_t rw) {
    HostEnv::film_add(S, ln, px, py, rw);
    const vpt::LaneCold& lc = cold_;
    const bool sky = ln.state == vpt::ST_FINISH;
    const uint32_t q = (uint32_t)((py - lc.y0) * rw + (px - lc.x0));
    const uint64_t jid = jid_begin + ln.jid_local;
    const uint32_t tile = (uint32_t)(jid % T), w = (uint32_t)(jid / T - wave0);
    float* at[2] = {plain + (ln.jid_local * (uint64_t)tile_area + q) * 3,
                    band + vpt::band_slot(tile, w, q, groups, (uint32_t)tile_area, G)};
    const uint64_t stride[2] = {plain_stride, band_stride};
    for (int l = 0; l < 2; ++l)
      for (int c = 0; c < 3; ++c) {
        at[l][c] = lc.L[c];
        at[l][stride[l] + c] = has_temp ? E[c] : 0.0f;  // (no temperature grid: the host zeroes the region)
        at[l][2 * stride[l] + c] = D[c];
        at[l][3 * stride[l] + c] = sky ? S.le_inf[c] : 0.0f;
      }
  }
};
static_assert(vpt::env_groups<GroupsEnv>::value && !vpt::env_groups<HostEnv>::value, "the trait");
}  // namespace

// `waves` whole waves from wave `wave_begin` of every tile, jid order, every gate at 1.  plain: float[4][jobs *
// tile_area * 3]; band: float[4][band_sample_floats(T, waves, tile_area, G)] (G = min(64, waves) as a capped launch's,
// or 64); film: the beauty film [H][W][4] (HostEnv's adds, jid order = wave order per pixel).
extern "C" int vptlg_render_waves(const vpt_configuration* cfg, const vpt_grid_desc* density, const vpt_grid_desc* temperature,
                                  uint64_t wave_begin, uint32_t waves, uint32_t G, float* film, float* plain, float* band,
                                  vpt_counters* counters) {
  vpt::DevScene S{};
  int rc = vpt::build_scene(*cfg, S);
  if (rc) return rc;
  vpt::HostGrid hd, ht;
  if ((rc = vpt::build_host_grid(*density, true, 0, hd))) return rc;
  vpt::compute_runs(hd, 0);
  const bool runs = !temperature && hd.run_fraction >= 0.25;
  S.density = hd.dev;
  vpt::scene_finalize(S);
  if (temperature) {
    if ((rc = vpt::build_host_grid(*temperature, false, 0, ht))) return rc;
    S.temperature = ht.dev;
    S.has_temperature = 1;
    S.bb_lds_ok = vpt::blackbody_rows_suffice(vpt::value_range(*temperature, 0), cfg->volume_parameters.temperature_scale,
                                              cfg->volume_parameters.temperature_offset, vpt::kBbLdsRows);
  }
  std::vector<float> bb(501 * 3, 0.0f);
  vpt::blackbody_table(bb.data());
  S.bb = bb.data();
  S.cie = vpt::cie_table();
  S.gate_min = S.gate_idle = S.gate_eval = S.gate_walk = 1;
  S.pixel_mode = 0;
  S.tile_area = (uint32_t)(S.tw * S.th);
  GroupsEnv env;
  env.jid_begin = wave_begin * S.T;
  env.jid_count = (uint64_t)waves * S.T;
  env.next = 0;
  env.film = film;
  env.records = nullptr;
  env.tile_area = S.tw * S.th;
  env.pixel_chunk = 1;
  env.has_temp = temperature != nullptr;
  env.plain = plain;
  env.plain_stride = env.jid_count * (uint64_t)env.tile_area * 3;
  env.band = band;
  env.T = (uint32_t)S.T;
  env.G = G;
  env.groups = vpt::band_groups(waves, G);
  env.band_stride = vpt::band_sample_floats(env.T, waves, S.tile_area, G);
  env.wave0 = wave_begin;
  vpt::Lane ln;
  std::memset(&ln, 0, sizeof ln);
  vpt::lane_init(ln);
  vpt::cold_init(env.cold());
  while (ln.state != vpt::ST_DONE) {
    if (temperature)
      vpt::lane_iteration<true, true, false>(&S, ln, env);
    else if (runs)
      vpt::lane_iteration<false, true, true>(&S, ln, env);
    else
      vpt::lane_iteration<false, true, false>(&S, ln, env);
  }
  env.cnt[vpt::CNT_DDA_STEPS] += ln.n_dda;
  uint64_t* o = reinterpret_cast<uint64_t*>(counters);
  for (int k = 0; counters && k < vpt::CNT_COUNT; ++k) o[k] += env.cnt[k];
  return 0;
}

extern "C" uint64_t vptlg_band_floats(uint32_t tiles, uint32_t waves, uint32_t tile_area, uint32_t G) {
  return vpt::band_sample_floats(tiles, waves, tile_area, G);
}
extern "C" uint64_t vptlg_band_slot(uint32_t tb, uint32_t w, uint32_t q, uint32_t groups, uint32_t tile_area, uint32_t G) {
  return vpt::band_slot(tb, w, q, groups, tile_area, G);
}
