// eval_split_host.cpp — TEST HARNESS: the device state machine (vpt_integrator.h lane_iteration) on the CPU, one lane,
// in two environments that differ only in the evaluation-split trait: HostEnv (hostsim.cpp's, the evaluation whole
// at the end of an iteration) and SplitEnv (kEvalSplit: eval_issue at the top, eval_finish in front of the ray
// block).  Host grids have no direct-addressed pool, so a split lane always takes eval_finish's lookup path
// (SM_FETCHED_LOOKUP); the loads' half is the GPU tests' (tests/test_gpu_eval_split.py).  Not part of the product.
#include "hostsim.cpp"

namespace {
struct SplitEnv : HostEnv {
  static constexpr bool kEvalSplit = true;
};
static_assert(!vpt::env_eval_split<HostEnv>::value && vpt::env_eval_split<SplitEnv>::value, "the trait is the only difference");

template <class Env>
int run(vpt::DevScene& S, bool temperature, bool runs, Env& env, uint64_t* rng_out) {
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
    // the fetched states never outlive the iteration that made them
    if (ln.sm == vpt::SM_FETCHED || ln.sm == vpt::SM_FETCHED_LOOKUP) return -100;
  }
  env.cnt[vpt::CNT_DDA_STEPS] += ln.n_dda;
  if (rng_out) *rng_out = ln.rng;
  return 0;
}
}  // namespace

// Jobs [jid_begin, jid_begin + jid_count) in jid order with every gate at 1, as vpths_render_jobs, in the split
// (split != 0) or the whole environment.  runs: -1 the GPU's rule, 0 / 1 forced.  *rng_out: the lane's RNG state
// after its last job.
extern "C" int vptes_render_jobs(const vpt_configuration* cfg, const vpt_grid_desc* density, const vpt_grid_desc* temperature,
                                 uint64_t jid_begin, uint64_t jid_count, float* film, float* records,
                                 vpt_counters* counters, int split, int runs_mode, uint64_t* rng_out) {
  vpt::DevScene S{};
  int rc = vpt::build_scene(*cfg, S);
  if (rc) return rc;
  vpt::HostGrid hd, ht;
  if ((rc = vpt::build_host_grid(*density, true, 0, hd))) return rc;
  vpt::compute_runs(hd, 0);
  const bool runs = !temperature && (runs_mode < 0 ? hd.run_fraction >= 0.25 : runs_mode != 0);
  S.density = hd.dev;
  if (S.density.dense) return -101;  // (host grids carry no dense pool: the lookup path is what this covers)
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
  auto fill = [&](HostEnv& e) {
    e.jid_begin = jid_begin;
    e.jid_count = jid_count;
    e.next = 0;
    e.film = film;
    e.records = records;
    e.tile_area = S.tw * S.th;
    e.pixel_chunk = 1;
  };
  uint64_t* o = reinterpret_cast<uint64_t*>(counters);
  if (split) {
    SplitEnv env;
    fill(env);
    if ((rc = run(S, temperature != nullptr, runs, env, rng_out))) return rc;
    for (int k = 0; counters && k < vpt::CNT_COUNT; ++k) o[k] += env.cnt[k];
  } else {
    HostEnv env;
    fill(env);
    if ((rc = run(S, temperature != nullptr, runs, env, rng_out))) return rc;
    for (int k = 0; counters && k < vpt::CNT_COUNT; ++k) o[k] += env.cnt[k];
  }
  return 0;
}
