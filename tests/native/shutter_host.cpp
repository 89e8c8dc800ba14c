// shutter_host.cpp — TEST HARNESS: the device state machine (vpt_integrator.h lane_iteration) on the CPU, one lane, in
// an environment with a shutter (Env::kShutter): hostsim.cpp's HostEnv plus the one dword the kernel keeps per lane
// (the job's offset in the shutter table, shutter_begin) and the table's rows (shutter_row), built by the product's
// own vpt::shutter_entry.  tests/test_shutter_host.py holds the film and the per-sample records to the ordered sum of
// the oracle's per-wave films, each rendered with that wave's camera.  Not part of the product.
#include "hostsim.cpp"

namespace {
struct ShutterEnv : HostEnv {
  static constexpr bool kShutter = true;
  const float* shutter = nullptr;  // [shutter_n][16]
  uint32_t shutter_n = 0;
  uint32_t at = 0;
  uint64_t begun = 0;
  const ShutterEnv* args() const { return this; }
  void shutter_begin(uint32_t entry) {
    at = entry * 16u;
    ++begun;
  }
  float4 shutter_row(int r) const {
    const float* p = shutter + at + 4 * r;
    float4 v;
    v.x = p[0];
    v.y = p[1];
    v.z = p[2];
    v.w = p[3];
    return v;
  }
};
static_assert(vpt::env_shutter<ShutterEnv>::value && !vpt::env_shutter<HostEnv>::value, "the trait");
}  // namespace

// Jobs [jid_begin, jid_begin + jid_count) in jid order, every gate at 1, job jid through camera (jid / T) % n of `cams`.
// film: [H][W][4] (HostEnv's adds: jid order = wave order per pixel); records: [jid_count * tile_area][3] or null.
extern "C" int vptsh_render_jobs(const vpt_configuration* cfg, const vpt_grid_desc* density, const vpt_grid_desc* temperature,
                                 const vpt_shutter_camera* cams, uint32_t n, uint64_t jid_begin, uint64_t jid_count,
                                 float* film, float* records, vpt_counters* counters) {
  if (!cams || !n) return VPT_E_INVALID;
  vpt::DevScene S{};
  int rc = vpt::build_scene(*cfg, S);
  if (rc) return rc;
  std::vector<float> table((size_t)n * 16);
  for (uint32_t i = 0; i < n; ++i) {
    if (vpt::camera_invalid(cams[i].position, cams[i].look, cams[i].up, cams[i].vfov_deg)) return VPT_E_INVALID;
    vpt::shutter_entry(cams[i], S.W, S.H, table.data() + (size_t)i * 16);
  }
  // (the scene's own camera must not be what the samples come from: poison it)
  for (int i = 0; i < 9; ++i) S.cam_L[i] = __builtin_nanf("");
  for (int i = 0; i < 3; ++i) S.cam_t[i] = S.cam_pos[i] = __builtin_nanf("");
  vpt::HostGrid hd, ht;
  if ((rc = vpt::build_host_grid(*density, true, 0, hd))) return rc;
  vpt::compute_runs(hd, 0);
  const bool runs = !temperature && (g_runs < 0 ? hd.run_fraction >= 0.25 : g_runs != 0);
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
  ShutterEnv env;
  env.jid_begin = jid_begin;
  env.jid_count = jid_count;
  env.next = 0;
  env.film = film;
  env.records = records;
  env.tile_area = S.tw * S.th;
  env.pixel_chunk = 1;
  env.shutter = table.data();
  env.shutter_n = n;
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
  if (env.begun != jid_count) return -100;  // (every job told the environment its entry)
  env.cnt[vpt::CNT_DDA_STEPS] += ln.n_dda;
  uint64_t* o = reinterpret_cast<uint64_t*>(counters);
  for (int k = 0; counters && k < vpt::CNT_COUNT; ++k) o[k] += env.cnt[k];
  return 0;
}
