// dense_pool_host.cpp — TEST HARNESS: the direct-addressed stencil pool (DevGrid::dense, vpt_gpu_set_pool_layout) on
// the CPU.  Built by tests/test_dense_pool_host.py like band_host (hipcc, host only) as a stand-alone program, also
// under AddressSanitizer + UBSan:
//   dense_pool_host <grid file>...
// Each file is a vpt_grid_desc as tests/test_dense_pool_host.py writes it.  For every grid the program
//   1. expands every cell of the cells8 table with expand_cell -- the host restatement of vpt_dense_expand_kernel:
//      a leaf cell copies its sparse brick, any other cell takes dense_square per square -- and compares, for every
//      voxel of the cell, the eight floats the dense path of trilinear() reads (dense_index) with fetch_stencil's
//      through cell_at, as uint32; a leaf's copied brick must also equal its dense_square values;
//   2. evaluates trilinear() with and without the dense pool at points inside and outside the table, alone and
//      along short walks that share a StencilCell: same value bits, same refresh flag.
// Prints "<file>: cells C leaves L stencils S points P" and "dense_pool_host ok", or FAIL lines and exits 1.
// With --dump <cell_begin> <cell_count> <out> after one grid file it writes those cells' bricks (the GPU test's
// reference for vpt_gpu_debug_read_pool) instead.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vpt_gpu.h"
#include "../../volume_path_tracer_amd/csrc/vpt_integrator.h"
#include "../../volume_path_tracer_amd/csrc/vpt_internal.h"

namespace vpt {
static thread_local std::string g_err;
int set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace vpt

namespace {
using vpt::DevGrid;
using vpt::kBrickVox;

struct GridFile {
  vpt_grid_desc d{};
  std::vector<int32_t> leaf_origin, tile_origin, tile_level, lower_origin, upper_origin;
  std::vector<float> leaf_values, leaf_max, tile_value;
  std::vector<uint64_t> leaf_mask;
  std::vector<uint8_t> tile_active;
};

template <class T>
bool read_vec(std::FILE* f, std::vector<T>& v, uint64_t n) {
  v.resize((size_t)n);
  return n == 0 || std::fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

// The layout tests/test_dense_pool_host.py writes: uint64 leaf, tile, lower, upper counts; float mat[9], inv[9],
// vec[3], background; int32 bbox_min[3], bbox_max[3]; then the arrays in vpt_grid_desc's order.
bool read_grid(const char* path, GridFile& g) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint64_t n[4];
  float fl[22];
  int32_t bb[6];
  bool ok = std::fread(n, 8, 4, f) == 4 && std::fread(fl, 4, 22, f) == 22 && std::fread(bb, 4, 6, f) == 6;
  ok = ok && n[0] < (1u << 24) && n[1] < (1u << 24) && n[2] < (1u << 24) && n[3] < (1u << 24);
  ok = ok && read_vec(f, g.leaf_origin, 3 * n[0]) && read_vec(f, g.leaf_values, 512 * n[0]) &&
       read_vec(f, g.leaf_mask, 8 * n[0]) && read_vec(f, g.leaf_max, n[0]) && read_vec(f, g.tile_origin, 3 * n[1]) &&
       read_vec(f, g.tile_level, n[1]) && read_vec(f, g.tile_value, n[1]) && read_vec(f, g.tile_active, n[1]) &&
       read_vec(f, g.lower_origin, 3 * n[2]) && read_vec(f, g.upper_origin, 3 * n[3]);
  std::fclose(f);
  if (!ok) return false;
  vpt_grid_desc& d = g.d;
  std::memcpy(d.map_mat, fl, 36);
  std::memcpy(d.map_inv_mat, fl + 9, 36);
  std::memcpy(d.map_vec, fl + 18, 12);
  d.background = fl[21];
  std::memcpy(d.index_bbox_min, bb, 12);
  std::memcpy(d.index_bbox_max, bb + 3, 12);
  d.leaf_count = n[0];
  d.leaf_origin = g.leaf_origin.data();
  d.leaf_values = g.leaf_values.data();
  d.leaf_value_mask = g.leaf_mask.data();
  d.leaf_max = g.leaf_max.data();
  d.tile_count = n[1];
  d.tile_origin = n[1] ? g.tile_origin.data() : nullptr;
  d.tile_level = n[1] ? g.tile_level.data() : nullptr;
  d.tile_value = n[1] ? g.tile_value.data() : nullptr;
  d.tile_active = n[1] ? g.tile_active.data() : nullptr;
  d.lower_count = n[2];
  d.lower_origin = n[2] ? g.lower_origin.data() : nullptr;
  d.upper_count = n[3];
  d.upper_origin = n[3] ? g.upper_origin.data() : nullptr;
  return true;
}

uint32_t bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

// vpt_dense_expand_kernel's work for one table cell, on the host: out[kBrickVox].
void expand_cell(const DevGrid& g, uint64_t cell, float* out) {
  const uint64_t ny = (uint64_t)g.r8_n[1], nz = (uint64_t)g.r8_n[2];
  const int32_t code = vpt::cell8_code(g.cells8[cell].x);
  if (code >= 0) {
    std::memcpy(out, g.bricks + (int64_t)code * kBrickVox, kBrickVox * sizeof(float));
  } else {
    const int32_t c = (int32_t)(cell % nz), b = (int32_t)((cell / nz) % ny), a = (int32_t)(cell / (nz * ny));
    for (int32_t s = 0; s < kBrickVox / 4; ++s) vpt::dense_square(g, a, b, c, s, out + 4 * s);
  }
}

std::atomic<int> g_fail{0};
void fail(const std::string& msg) {
  if (g_fail.fetch_add(1) < 20) std::printf("FAIL %s\n", msg.c_str());
}

int threads() {
  const unsigned h = std::thread::hardware_concurrency();
  return (int)std::min(16u, std::max(1u, h));
}

// Check 1 over the cells [begin, end): returns the stencils compared.
uint64_t check_cells(const char* name, const DevGrid& g, uint64_t begin, uint64_t end) {
  const uint64_t ny = (uint64_t)g.r8_n[1], nz = (uint64_t)g.r8_n[2];
  std::vector<float> brick(kBrickVox), sq(4);
  uint64_t n = 0;
  for (uint64_t cell = begin; cell < end; ++cell) {
    expand_cell(g, cell, brick.data());
    const int32_t c = (int32_t)(cell % nz), b = (int32_t)((cell / nz) % ny), a = (int32_t)(cell / (nz * ny));
    if (vpt::cell8_code(g.cells8[cell].x) >= 0)  // the copied brick is what dense_square computes
      for (int32_t s = 0; s < kBrickVox / 4; ++s) {
        vpt::dense_square(g, a, b, c, s, sq.data());
        for (int q = 0; q < 4; ++q)
          if (bits(sq[q]) != bits(brick[4 * s + q]))
            fail(std::string(name) + ": leaf cell " + std::to_string(cell) + " square " + std::to_string(s));
      }
    for (int32_t x = 0; x < 8; ++x)
      for (int32_t y = 0; y < 8; ++y)
        for (int32_t z = 0; z < 8; ++z) {
          const int32_t i = g.r8_org[0] + a * 8 + x, j = g.r8_org[1] + b * 8 + y, k = g.r8_org[2] + c * 8 + z;
          // the table cell cell_at finds for this voxel is `cell`
          if (vpt::mad_index((i - g.r8_org[0]) >> 3, (j - g.r8_org[1]) >> 3, (k - g.r8_org[2]) >> 3, g.r8_n) != cell)
            fail(std::string(name) + ": table index of cell " + std::to_string(cell));
          const float* d = brick.data() + vpt::dense_index(0, i, j, k);
          float s[8];
          vpt::fetch_stencil(g, vpt::cell_at(g, i, j, k), i, j, k, s);
          for (int q = 0; q < 8; ++q)
            if (bits(d[q]) != bits(s[q]))
              fail(std::string(name) + ": cell " + std::to_string(cell) + " voxel (" + std::to_string(x) + ", " +
                   std::to_string(y) + ", " + std::to_string(z) + ") corner " + std::to_string(q));
          ++n;
        }
  }
  return n;
}

struct Pool {
  float* p = nullptr;
  std::vector<uint8_t> filled;  // per cell (empty: the whole pool is filled)
  ~Pool() { std::free(p); }
};

// The cell of the table that holds voxel (i, j, k), or false outside it.
bool table_cell(const DevGrid& g, int32_t i, int32_t j, int32_t k, uint64_t& cell) {
  const int32_t a = (i - g.r8_org[0]) >> 3, b = (j - g.r8_org[1]) >> 3, c = (k - g.r8_org[2]) >> 3;
  if (!((uint32_t)a < (uint32_t)g.r8_n[0] && (uint32_t)b < (uint32_t)g.r8_n[1] && (uint32_t)c < (uint32_t)g.r8_n[2]))
    return false;
  cell = vpt::mad_index(a, b, c, g.r8_n);
  return true;
}

// Check 2: walks of 1..6 points sharing a StencilCell per layout.  The pool is calloc'ed whole (the addresses the
// dense path computes are inside it for every table cell); tables above 64 MiB of bricks expand only the cells the
// points touch, the others stay zero pages.
uint64_t check_points(const char* name, const DevGrid& g, uint64_t cells, uint32_t seed) {
  Pool pool;
  pool.p = (float*)std::calloc((size_t)cells, kBrickVox * sizeof(float));
  if (!pool.p) {
    fail(std::string(name) + ": no memory for the pool");
    return 0;
  }
  const bool whole = cells * kBrickVox * sizeof(float) <= (64u << 20);
  if (whole) {
    std::vector<std::thread> th;
    const int nt = threads();
    for (int t = 0; t < nt; ++t)
      th.emplace_back([&, t] {
        for (uint64_t cell = (uint64_t)t; cell < cells; cell += (uint64_t)nt) expand_cell(g, cell, pool.p + cell * kBrickVox);
      });
    for (auto& t : th) t.join();
  } else {
    pool.filled.assign((size_t)cells, 0);
  }
  DevGrid gd = g;
  gd.dense = pool.p;
  std::mt19937 rng(seed);
  auto uni = [&](float lo, float hi) { return lo + (hi - lo) * (float)(rng() >> 8) * (1.0f / 16777216.0f); };
  const float lo[3] = {(float)g.r8_org[0], (float)g.r8_org[1], (float)g.r8_org[2]};
  const float hi[3] = {lo[0] + 8.0f * g.r8_n[0], lo[1] + 8.0f * g.r8_n[1], lo[2] + 8.0f * g.r8_n[2]};
  uint64_t n = 0;
  const int walks = 60000;
  for (int w = 0; w < walks; ++w) {
    float p[3], d[3];
    const int kind = w % 4;  // 0: inside, 1: a margin of 24 voxels around the table, 2: on a face, 3: far outside
    for (int a = 0; a < 3; ++a) {
      const float m = kind == 0 ? 0.0f : kind == 3 ? 6000.0f : 24.0f;
      p[a] = uni(lo[a] - m, hi[a] + m);
      d[a] = uni(-3.0f, 3.0f);
    }
    if (kind == 2) {
      const int a = (int)(rng() % 3);
      p[a] = (rng() & 1) ? hi[a] - uni(0.0f, 1.5f) : lo[a] + uni(-0.5f, 1.0f);
      if (rng() & 1) p[a] = floorf(p[a]);  // integer coordinates: weight 0 on the +1 corners
    }
    if ((w & 7) == 0) d[0] = d[1] = d[2] = 0.0f;  // the same voxel again: no refresh
    vpt::StencilCell sa{vpt::kNoCell, 0, 0, -1}, sb = sa;
    const int len = 1 + (int)(rng() % 6);
    for (int s = 0; s < len; ++s) {
      const float x = p[0] + d[0] * (float)s, y = p[1] + d[1] * (float)s, z = p[2] + d[2] * (float)s;
      uint64_t cell;
      if (!whole && table_cell(g, (int32_t)floorf(x), (int32_t)floorf(y), (int32_t)floorf(z), cell) && !pool.filled[cell]) {
        expand_cell(g, cell, pool.p + cell * kBrickVox);
        pool.filled[cell] = 1;
      }
      float va, vb;
      const bool ra = vpt::trilinear(g, sa, x, y, z, va), rb = vpt::trilinear(gd, sb, x, y, z, vb);
      if (bits(va) != bits(vb) || ra != rb || sa.i != sb.i || sa.j != sb.j || sa.k != sb.k)
        fail(std::string(name) + ": point (" + std::to_string(x) + ", " + std::to_string(y) + ", " + std::to_string(z) +
             ") sparse " + std::to_string(va) + " dense " + std::to_string(vb) + " refresh " + std::to_string(ra) + "/" +
             std::to_string(rb));
      ++n;
    }
  }
  return n;
}

int run_grid(const char* path) {
  GridFile gf;
  if (!read_grid(path, gf)) {
    std::printf("FAIL %s: cannot read\n", path);
    return 1;
  }
  vpt::HostGrid hg;
  if (vpt::build_host_grid(gf.d, true, 0, hg)) {
    std::printf("FAIL %s: build_host_grid: %s\n", path, vpt::g_err.c_str());
    return 1;
  }
  const DevGrid& g = hg.dev;
  const uint64_t cells = (uint64_t)hg.cells8.size();
  if (g.dense) fail(std::string(path) + ": host builds leave the dense pointer null");
  std::vector<std::thread> th;
  const int nt = threads();
  std::atomic<uint64_t> stencils{0};
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      stencils += check_cells(path, g, cells * (uint64_t)t / (uint64_t)nt, cells * (uint64_t)(t + 1) / (uint64_t)nt);
    });
  for (auto& t : th) t.join();
  const uint64_t points = check_points(path, g, cells, 12345u);
  std::printf("%s: cells %llu leaves %d stencils %llu points %llu\n", path, (unsigned long long)cells, g.leaf_count,
              (unsigned long long)stencils.load(), (unsigned long long)points);
  return 0;
}

int dump(const char* path, uint64_t begin, uint64_t count, const char* out) {
  GridFile gf;
  vpt::HostGrid hg;
  if (!read_grid(path, gf) || vpt::build_host_grid(gf.d, true, 0, hg)) return 1;
  if (begin > hg.cells8.size() || count > hg.cells8.size() - begin) return 1;
  std::vector<float> brick(kBrickVox);
  std::FILE* f = std::fopen(out, "wb");
  if (!f) return 1;
  bool ok = true;
  for (uint64_t c = begin; c < begin + count; ++c) {
    expand_cell(hg.dev, c, brick.data());
    ok = ok && std::fwrite(brick.data(), sizeof(float), kBrickVox, f) == (size_t)kBrickVox;
  }
  std::fclose(f);
  return ok ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 6 && !std::strcmp(argv[2], "--dump"))
    return dump(argv[1], std::strtoull(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10), argv[5]);
  if (argc < 2) {
    std::printf("usage: dense_pool_host <grid file>... | <grid file> --dump <cell_begin> <cell_count> <out>\n");
    return 2;
  }
  for (int i = 1; i < argc; ++i)
    if (run_grid(argv[i])) return 1;
  if (g_fail.load()) {
    std::printf("dense_pool_host: %d checks failed\n", g_fail.load());
    return 1;
  }
  std::printf("dense_pool_host ok\n");
  return 0;
}
