// band_host.cpp — a stand-alone host check of the band launch's shared arithmetic (vpt_gpu_render_tiles): the
// item -> (tile, wave) mapping and the lane-adjacent sample layout of vpt_integrator.h (band_job, band_slot,
// band_sample_floats: the functions the kernels call), and the drop-in's cost_bands cuts (include/vpt_run.hpp),
// which distributed.cost_bands restates in Python.  Built by tests/test_band_host.py like hostsim (hipcc, host
// only), once more with -fsanitize=address,undefined, and run directly.
//
//   band_host [costs.txt]     costs.txt: one line per case, "<bands> <cost 0> <cost 1> ..."; prints "cuts: ..."
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../../volume_path_tracer_amd/csrc/vpt_internal.h"
#include "vpt_run.hpp"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAIL %s: ", #cond);         \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++g_fail;                                \
    }                                          \
  } while (0)

// One band: T tiles per wave, the tiles [lo, hi), n waves, 8 x 8 tiles, groups of 64 waves.
void check_band(uint32_t T, uint32_t lo, uint32_t hi, uint32_t n) {
  const uint32_t B = hi - lo, area = 64, G = vpt::kBandGroup;
  // the tile ranks: a cost order with ties (stable: ties by tile index), filtered to the band
  std::vector<uint32_t> order(T);
  for (uint32_t i = 0; i < T; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [](uint32_t a, uint32_t b) { return (a * 7u) % 5u > (b * 7u) % 5u; });
  std::vector<uint32_t> rank;
  for (uint32_t t : order)
    if (t >= lo && t < hi) rank.push_back(t);
  CHECK(rank.size() == B, "T %u band [%u, %u)", T, lo, hi);

  // items <-> (tile, wave): a bijection onto the band's jobs, tile by tile in rank order, waves consecutive
  std::set<uint64_t> jobs;
  for (uint64_t k = 0; k < (uint64_t)B * n; ++k) {
    const uint64_t j = vpt::band_job(k, n, T, rank.data());
    const uint32_t w = (uint32_t)(j / T), t = (uint32_t)(j % T);
    CHECK(w < n && t >= lo && t < hi, "item %llu -> wave %u tile %u", (unsigned long long)k, w, t);
    CHECK(t == rank[k / n] && w == k % n, "item %llu: same-tile order", (unsigned long long)k);
    jobs.insert(j);
  }
  CHECK(jobs.size() == (uint64_t)B * n, "T %u band [%u, %u) n %u: %zu distinct jobs", T, lo, hi, n, jobs.size());

  // slots: unique, inside the buffer, and the G waves of one group at one pixel 3 floats apart
  const uint32_t groups = vpt::band_groups(n, G);
  const uint64_t size = vpt::band_sample_floats(B, n, area, G);
  CHECK(groups == (n + 63) / 64 && size == (uint64_t)B * groups * area * G * 3, "buffer size");
  std::vector<uint8_t> used(size / 3, 0);
  for (uint32_t tb = 0; tb < B; ++tb)
    for (uint32_t w = 0; w < n; ++w)
      for (uint32_t q = 0; q < area; ++q) {
        const uint64_t s = vpt::band_slot(tb, w, q, groups, area, G);
        CHECK(s % 3 == 0 && s + 3 <= size, "slot (%u, %u, %u) = %llu of %llu", tb, w, q, (unsigned long long)s,
              (unsigned long long)size);
        if (s + 3 > size) return;
        CHECK(!used[s / 3], "slot (%u, %u, %u) taken twice", tb, w, q);
        used[s / 3] = 1;
        if (w % G) CHECK(s == vpt::band_slot(tb, w - 1, q, groups, area, G) + 3, "lane-adjacent (%u, %u, %u)", tb, w, q);
        // a pixel's run of a group is G * 3 floats; the next pixel's follows it
        if (q) CHECK(s == vpt::band_slot(tb, w, q - 1, groups, area, G) + (uint64_t)G * 3, "pixel stride");
      }
}

// 64-bit arithmetic: a frame whose slots pass 2^32 floats keeps distinct, in-range offsets at its far corner.
void check_wide() {
  const uint32_t B = 32400, n = 1024, area = 64, G = vpt::kBandGroup, groups = vpt::band_groups(n, G);
  const uint64_t size = vpt::band_sample_floats(B, n, area, G);
  CHECK(size == 32400ull * 1024 * 64 * 3 && size > (1ull << 32), "wide size");
  const uint64_t last = vpt::band_slot(B - 1, n - 1, area - 1, groups, area, G);
  CHECK(last + 3 == size, "wide last slot %llu", (unsigned long long)last);
}

}  // namespace

int main(int argc, char** argv) {
  const uint32_t cases[4][4] = {{30, 7, 19, 6}, {20, 3, 20, 5}, {30, 0, 30, 66}, {30, 29, 30, 130}};
  for (const auto& c : cases) check_band(c[0], c[1], c[2], c[3]);
  check_wide();
  if (argc > 1) {
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      size_t n = 0;
      if (!(ls >> n)) continue;
      std::vector<float> cost;
      for (std::string v; ls >> v;) cost.push_back(std::strtof(v.c_str(), nullptr));
      const std::vector<uint32_t> cut = vpt_gpu::detail::cost_bands(cost, n);
      std::printf("cuts:");
      for (uint32_t c : cut) std::printf(" %u", c);
      std::printf("\n");
    }
  }
  if (g_fail) {
    std::printf("band_host: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("band_host ok\n");
  return 0;
}
