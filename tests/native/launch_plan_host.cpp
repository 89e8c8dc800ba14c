// launch_plan_host.cpp -- the kernel-variant rule and the launch plan on the CPU (tests/test_launch_plan_host.py).
// Includes only the HIP-free header.  Checks: encode / decode round-trips over all 1 024 indices; variant_valid holds
// for exactly the 45 flag strings listed below (the integrate-kernel symbols of the library before the rule was
// written down once); and plan_launch / attachments_refuse reproduce every row of tests/golden/launch_plans.json, the
// decisions render() made before they moved into plan_launch.
//   launch_plan_host <launch_plans.json>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../volume_path_tracer_amd/csrc/vpt_variant.h"

namespace {

// HasTemp Debug Runs Lat Compact Feed Band Gang Groups Shutter
const char* const kVariants[] = {
    "0000000000", "0010000000", "1000000000", "0100000000", "0110000000", "1100000000", "0001000000", "0011000000",
    "1001000000", "0001100000", "0011100000", "1001100000", "0000010000", "0010010000", "1000010000", "0000001000",
    "0010001000", "1000001000", "0001001000", "0011001000", "1001001000", "0001101000", "0011101000", "1001101000",
    "0000000100", "0010000100", "1000000100", "0000000010", "0010000010", "1000000010", "0000001010", "0010001010",
    "1000001010", "0000000001", "0010000001", "1000000001", "0000001001", "0010001001", "1000001001", "0000000011",
    "0010000011", "1000000011", "0000001011", "0010001011", "1000001011"};

int g_fail = 0;
void fail(const std::string& what) {
  if (++g_fail <= 20) std::printf("FAIL %s\n", what.c_str());
}

std::string flag_string(const vpt::KernelVariant& v) {
  const bool f[10] = {v.temp, v.debug, v.runs, v.lat, v.compact, v.feed, v.band, v.gang, v.groups, v.shutter};
  std::string s;
  for (bool b : f) s += b ? '1' : '0';
  return s;
}

int check_variants() {
  std::set<std::string> want(std::begin(kVariants), std::end(kVariants)), have;
  for (uint32_t i = 0; i < vpt::kVariantCount; ++i) {
    const vpt::KernelVariant v = vpt::variant_decode(i);
    if (vpt::variant_index(v) != i) fail("round trip of index " + std::to_string(i));
    const std::string s = flag_string(v);
    if ((uint32_t)std::strtoul(s.c_str(), nullptr, 2) != i) fail("flag string of index " + std::to_string(i));
    if (vpt::variant_valid(v)) have.insert(s);
  }
  if (want.size() != 45) fail("the list holds 45 distinct variants");
  for (const std::string& s : have)
    if (!want.count(s)) fail("variant_valid accepts " + s);
  for (const std::string& s : want)
    if (!have.count(s)) fail("variant_valid rejects " + s);
  // the two functions of a variant at the values the kernels were built with
  for (const std::string& s : have) {
    const vpt::KernelVariant v = vpt::variant_decode((uint32_t)std::strtoul(s.c_str(), nullptr, 2));
    const int waves = v.compact ? 2 : v.lat ? VPT_WAVES_LAT : v.debug ? VPT_WAVES_SLOW : v.temp ? VPT_WAVES_TEMP : VPT_WAVES_FAST;
    if (vpt::variant_waves_per_simd(v) != waves) fail("waves per SIMD of " + s);
    if (vpt::variant_eval_split(v) != (!v.temp && !v.debug && !v.lat)) fail("evaluation split of " + s);
  }
  return (int)have.size();
}

// The golden file's tokens: strings and integers, punctuation dropped.
struct Token {
  bool is_name;
  std::string name;
  long long value;
};
std::vector<Token> tokens(const std::string& text) {
  std::vector<Token> out;
  for (size_t i = 0; i < text.size();) {
    const char c = text[i];
    if (c == '"') {
      const size_t e = text.find('"', i + 1);
      if (e == std::string::npos) break;
      out.push_back({true, text.substr(i + 1, e - i - 1), 0});
      i = e + 1;
    } else if (c == '-' || (c >= '0' && c <= '9')) {
      char* end = nullptr;
      const long long v = std::strtoll(text.c_str() + i, &end, 10);
      out.push_back({false, "", v});
      i = (size_t)(end - text.c_str());
    } else {
      ++i;
    }
  }
  return out;
}

int check_rows(const char* path) {
  std::ifstream f(path);
  if (!f) {
    fail(std::string("cannot read ") + path);
    return 0;
  }
  const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const std::vector<Token> tok = tokens(text);
  std::vector<std::string> in_names, plan_names;
  size_t i = 0;
  if (i >= tok.size() || tok[i].name != "in_fields") fail("in_fields first");
  for (++i; i < tok.size() && tok[i].is_name && tok[i].name != "plan_fields"; ++i) in_names.push_back(tok[i].name);
  for (++i; i < tok.size() && tok[i].is_name && tok[i].name != "rows"; ++i) plan_names.push_back(tok[i].name);
  ++i;
  const size_t per_row = in_names.size() + plan_names.size();
  if (per_row == 0 || (tok.size() - i) % per_row != 0) {
    fail("the rows are whole");
    return 0;
  }
  int rows = 0, refused = 0;
  std::set<uint32_t> seen;
  for (; i + per_row <= tok.size(); i += per_row, ++rows) {
    std::map<std::string, long long> a, want;
    for (size_t k = 0; k < in_names.size(); ++k) a[in_names[k]] = tok[i + k].value;
    for (size_t k = 0; k < plan_names.size(); ++k) want[plan_names[k]] = tok[i + in_names.size() + k].value;
    vpt::LaunchInputs in;
    in.jid_begin = (uint64_t)a.at("jid_begin");
    in.jid_count = (uint64_t)a.at("jid_count");
    in.T = (uint64_t)a.at("T");
    in.tile_area = (uint32_t)a.at("tile_area");
    in.grid_blocks = (int)a.at("grid_blocks");
    in.grid_user = (int)a.at("grid_user");
    in.cus = (int)a.at("cus");
    in.lat_per_cu = (int)a.at("lat_per_cu");
    in.lat_mode = (int)a.at("lat_mode");
    in.lat_ungated = (int)a.at("lat_ungated");
    in.compact_every = (int)a.at("compact_every");
    in.compact_per_cu = (int)a.at("compact_per_cu");
    in.has_temperature = a.at("has_temperature") != 0;
    in.use_runs = a.at("use_runs") != 0;
    in.pixel_mode = a.at("pixel_mode") != 0;
    in.pixel_chunk = (int)a.at("pixel_chunk");
    in.order_mode = (int)a.at("order_mode");
    in.order_tail_waves = (int)a.at("order_tail_waves");
    in.film_order = (int)a.at("film_order");
    in.frame_waves = (uint64_t)a.at("frame_waves");
    in.records = a.at("records") != 0;
    in.events = a.at("events") != 0;
    in.feed = a.at("feed") != 0;
    in.band = a.at("band") != 0;  // (band_list: a band's tile list reaches no decision, only the rank filter)
    in.groups = a.at("groups") != 0;
    in.shutter = a.at("shutter") != 0;
    in.moments = a.at("moments") != 0;
    const std::string row = "row " + std::to_string(rows);
    if (vpt::attachments_refuse(in) != (want.at("refused") != 0)) fail(row + ": refused");
    if (!vpt::variant_valid(vpt::variant_decode((uint32_t)want.at("variant")))) fail(row + ": the golden row names no instantiation");
    if (want.at("refused")) {  // render() returns before the plan
      ++refused;
      continue;
    }
    const vpt::LaunchPlan p = vpt::plan_launch(in);
    const std::map<std::string, long long> got = {
        {"refused", 0},
        {"variant", vpt::variant_index(p.variant)},
        {"blocks", p.blocks},
        {"lds_bytes", (long long)p.lds_bytes},
        {"gate_set", p.gate_set},
        {"latency", p.latency},
        {"pixel_chunk", p.pixel_chunk},
        {"items", (long long)p.items},
        {"ordered", p.ordered},
        {"cost_order", p.cost_order},
        {"order_group", p.order_group},
        {"order_tail_n", p.order_tail_n},
        {"order_tail_k0", p.order_tail_k0},
        {"compact_every", p.compact_every},
        {"zero_region1", p.zero_region1},
    };
    if (got.size() != want.size()) fail(row + ": the plan's fields");
    for (const auto& kv : want)
      if (!got.count(kv.first) || got.at(kv.first) != kv.second)
        fail(row + ": " + kv.first + " " + std::to_string(got.count(kv.first) ? got.at(kv.first) : -1) + ", golden " +
             std::to_string(kv.second));
    if (!vpt::variant_valid(p.variant)) fail(row + ": the plan names no instantiation");
    seen.insert(vpt::variant_index(p.variant));
  }
  std::printf("rows %d refused %d variants %zu\n", rows, refused, seen.size());
  return rows;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s launch_plans.json\n", argv[0]);
    return 2;
  }
  const int valid = check_variants();
  std::printf("variants %d of %u\n", valid, vpt::kVariantCount);
  if (valid != 45) fail("45 variants");
  check_rows(argv[1]);
  if (g_fail) {
    std::printf("launch_plan_host FAILED (%d)\n", g_fail);
    return 1;
  }
  std::printf("launch_plan_host ok\n");
  return 0;
}
