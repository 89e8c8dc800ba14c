/*
 * vpt_gpu.h — C ABI of the MI355X (gfx950) volumetric path-tracing integrator.
 *
 * This is the drop-in boundary for the reference's per-tile integration loop
 *
 *     void vpt::run(const WorkerParameters&, const Volume&, const Camera&, TileProvider&,
 *                   Image<float,4>& film, RandomNumberGenerator rng)
 *         — reference include/vpt/worker.hpp:11, src/worker.cpp:92-208
 *
 * The reference has no FFI or plugin registry: `run` is a plain C++ function called by
 * `num_workers` std::jthreads (src/main.cpp:63-68).  This header exposes the same work as
 * an opaque-context C API with plain pointers and sizes.  A (tile, wave) job is keyed by
 * its job id `jid` exactly as TileProvider::next() assigns it (src/tile_provider.cpp:27-31):
 *     tile = jid % T,  wave = 1 + jid / T,  T = ceil(W/tw) * ceil(H/th)
 * and its random stream is pcg32_fast seeded with hash(seed, jid) (include/vpt/random.hpp:93-95),
 * so any partition of the jid space (threads, launches, GPUs) renders the same samples.
 *
 * Every function returns VPT_OK (0) or an error code; vpt_last_error() gives the message
 * (thread-local).  The reference's fatal paths (`vptFATAL` = exit(1), include/vpt/logging.hpp:16)
 * become error returns here.
 *
 * INTEGRATION.md shows the reference-side binding (a `run_gpu` with run()'s signature).
 */
#ifndef VPT_GPU_H
#define VPT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPT_ABI_VERSION 1

enum {
  VPT_OK = 0,
  VPT_E_INVALID = 1,  /* bad argument / schema violation */
  VPT_E_HIP = 2,      /* HIP runtime failure or no HIP device */
  VPT_E_IO = 3,       /* file could not be read */
  VPT_E_PARSE = 4,    /* JSON syntax error, missing or unknown key */
  VPT_E_NOMEM = 5,
  VPT_E_STATE = 6     /* call not valid in the context's current state */
};

/* ---- scene configuration: include/vpt/configuration.hpp:14-65 ------------------------- */

/* CameraParameters, configuration.hpp:20-27 */
typedef struct vpt_camera_params {
  float position[3];
  float look[3];
  float up[3];
  float vfov_deg;
  float imaging_ratio;
} vpt_camera_params;

/* WorkerParameters, configuration.hpp:40-50 (image_point_t = Eigen::Index pair) */
typedef struct vpt_worker_params {
  int32_t single_pixel_enabled;
  int32_t use_jitter;
  int64_t single_pixel_coord[2]; /* (x, y) */
  float infinite_light_xyz[3];
  float infinite_light_multiplier;
  float distant_light_xyz[3];
  float distant_light_multiplier;
  float distant_light_inv_direction[3];
  uint32_t max_depth;
} vpt_worker_params;

/* VolumeParameters, configuration.hpp:52-59 */
typedef struct vpt_volume_params {
  float henyey_greenstein_g;
  float le_scale;
  float sigma_a;
  float sigma_s;
  float temperature_offset;
  float temperature_scale;
} vpt_volume_params;

/* Configuration, configuration.hpp:61-71 */
typedef struct vpt_configuration {
  uint32_t seed;
  uint32_t num_waves;
  uint32_t num_workers;
  uint32_t _pad0;
  int64_t output_size[2]; /* (w, h) */
  int64_t tile_size[2];   /* (w, h) */
  vpt_camera_params camera_parameters;
  vpt_worker_params worker_parameters;
  vpt_volume_params volume_parameters;
  char volume_path[4096]; /* as written in the JSON (relative to the config's directory) */
} vpt_configuration;

/* read_configuration (src/configuration.cpp:8-22): strict JSON reader for exactly this schema;
 * a missing key (glaze error_on_missing_keys) or an unknown key is VPT_E_PARSE. */
int vpt_config_read(const char* path, vpt_configuration* out);
int vpt_config_parse(const char* json_text, size_t len, vpt_configuration* out);

/* ---- grids: include/vpt/volume_grids.hpp:12-14 (nanovdb::NanoGrid<float>) -------------- */

/* A NanoVDB float grid flattened to plain arrays.  Node semantics are NanoVDB's:
 * leaves 8^3, lower nodes 16^3 leaves (128^3 voxels), upper nodes 32^3 lower nodes
 * (4096^3 voxels), root tiles keyed by 4096-aligned origin.  Node existence is implied:
 * a lower node exists if it holds a leaf or a level-1 tile (or is listed in lower_origin),
 * an upper node exists if it holds a lower node or a level-2 tile (or is listed).
 * Slots not covered by a child or a listed tile hold (background, inactive). */
typedef struct vpt_grid_desc {
  float map_mat[9];      /* nanovdb::Map::mMatF    (index->world, row-major) */
  float map_inv_mat[9];  /* nanovdb::Map::mInvMatF (world->index, row-major) */
  float map_vec[3];      /* nanovdb::Map::mVecF    (translation)             */
  float background;
  int32_t index_bbox_min[3]; /* Grid::indexBBox(), inclusive (volume.cpp:83) */
  int32_t index_bbox_max[3];
  uint64_t leaf_count;
  const int32_t* leaf_origin;      /* [leaf_count][3], multiples of 8                      */
  const float* leaf_values;        /* [leaf_count][512], n = (x&7)<<6 | (y&7)<<3 | (z&7)    */
  const uint64_t* leaf_value_mask; /* [leaf_count][8] active-voxel bits (NanoVDB Mask<3>)  */
  const float* leaf_max;           /* [leaf_count] LeafNode::getMax() as stored            */
  uint64_t tile_count;
  const int32_t* tile_origin; /* [tile_count][3]                                                    */
  const int32_t* tile_level;  /* 1: lower-node tile (8^3), 2: upper-node tile (128^3), 3: root tile */
  const float* tile_value;
  const uint8_t* tile_active;
  uint64_t lower_count;       /* optional extra internal nodes that hold no leaf (may be 0)  */
  const int32_t* lower_origin;
  uint64_t upper_count;
  const int32_t* upper_origin;
} vpt_grid_desc;

/* A nanovdb::NanoGrid<float> in memory -> vpt_grid_desc.  grid_buffer = the grid's own bytes, as the
 * reference holds them (&vol.grids().density(), grid.gridSize() bytes = GridHandle::data(); NanoVDB
 * 32.x layout restated, include/vpt/volume_grids.hpp:12-33): leaves with their values, value masks and
 * stored maxima, lower / upper node tiles (non-child slots that are active or differ from the
 * background), root tiles, and every internal node's origin.  Every offset in the buffer is
 * bounds-checked (VPT_E_INVALID on a malformed buffer).  *out owns its arrays: release it with
 * vpt_grid_free.  Replaces the NanoVDB tree walk a caller of vpt_gpu_create would otherwise write. */
int vpt_grid_from_nanovdb(const void* grid_buffer, size_t bytes, vpt_grid_desc** out);
/* nanovdb::io::readGrid(path, grid_name) for a float grid (src/volume_grids.cpp:38-67): .nvdb files
 * of NanoVDB 32.x, codec NONE or ZIP.  A file without a grid of that name returns VPT_OK with
 * *out = NULL (the reference's nanovdb_try_read_grid, volume_grids.cpp:38-46); an unreadable file is
 * VPT_E_IO, a malformed one VPT_E_INVALID.  Release *out with vpt_grid_free. */
int vpt_grid_read_nvdb(const char* path, const char* grid_name, vpt_grid_desc** out);
/* Releases a desc from vpt_grid_from_nanovdb / vpt_grid_read_nvdb / vpt_synth_grid. */
void vpt_grid_free(vpt_grid_desc* desc);

/* fix_majorants_for_interpolation(grid, order=1) (src/volume.cpp:104-160), host side:
 * out_leaf_max[i] = max(desc.leaf_max[i], getValue(c) for c in the 26 neighbour leaf boxes
 * intersected with leaf i's bbox expanded by 1).  Idempotent.  Uses up to num_threads threads. */
int vpt_fix_majorants(const vpt_grid_desc* grid, float* out_leaf_max, int num_threads);

/* ---- blackbody emission: src/precompute_blackbody.cpp:7-52, src/spectral.cpp:7-20 ------- */

#define VPT_BLACKBODY_ROWS 500
/* init_blackbody_radiation_xyz(): bb_xyz[i] = spectrum_to_xyz(planck(T = (i-1)*100 K)),
 * written as [500][3] floats, from the CIE 1931 table shipped with the package. */
int vpt_blackbody_table(float* out_500x3);
/* blackbody_radiation_xyz(T) on the host, for tests. */
int vpt_blackbody_xyz(const float* table_500x3, float temperature_k, float* out_xyz);

/* ---- output: film_to_image (src/main.cpp:12-24, include/vpt/color.hpp:8-30) --------------- */

/* XYZ/W -> linear sRGB (3x3 matrix) -> sRGB OETF -> clamp [0,1] -> *255 -> truncate to u8.
 * film: float[h][w][4]; out: uint8[h][w][3] (the 8-bit RGB image the reference saves as PNG). */
int vpt_film_to_srgb8(const float* film_hxwx4, int64_t w, int64_t h, uint8_t* out_hxwx3);

/* ---- the integrator ---------------------------------------------------------------------- */

typedef struct vpt_gpu_ctx vpt_gpu_ctx;

/* Event counters accumulated by every launch (for algorithmic bytes). */
typedef struct vpt_counters {
  uint64_t samples;        /* film samples written (pixels traced)                     */
  uint64_t dda_steps;      /* HDDA steps taken (volume.cpp:56)                          */
  uint64_t segments;       /* majorant segments returned by RayMajorantIterator::next   */
  uint64_t draws;          /* exponential free-flight draws (sampler.cpp:44)            */
  uint64_t stencils;       /* density trilinear stencil refreshes (cell changes)        */
  uint64_t density_evals;  /* density trilinear evaluations                             */
  uint64_t temp_stencils;  /* temperature trilinear stencil refreshes                   */
  uint64_t scatters;       /* scatter events                                            */
  uint64_t shadow_rays;    /* sample_Ld calls that traced a ray                         */
  uint64_t rng_draws;      /* uniform<float>() calls                                    */
  uint64_t exchanged;      /* paths moved by live-path compaction (vpt_gpu_set_compaction) */
} vpt_counters;

/* Create a context on HIP device `device`.  Copies everything it needs (the grids are
 * flattened into an HBM brick pool + leaf-slot/majorant tables; the caller's arrays may be
 * freed afterwards).  `density` is required (volume_grids.cpp:58-60); `temperature` may be
 * NULL (volume_grids.cpp:61-66).  `blackbody_500x3` may be NULL: the table is then computed
 * with vpt_blackbody_table().  The density grid's leaf maxima are fixed for interpolation
 * here (Volume::Volume, volume.cpp:162-170) — passing already-fixed maxima is harmless.
 * Device memory per grid: 9 KiB per leaf (the stencil pool: per voxel row the 2x2 squares of x = 0..8)
 * plus the cell tables (~12 B per 8^3 cell of the lower nodes' bounding box); the host holds the same
 * while building.  A grid that does not fit the device's free memory is VPT_E_NOMEM before any
 * allocation (e.g. 0.84 GB for the 512^3 cloud stand-in's 90 704 leaves). */
int vpt_gpu_create(const vpt_configuration* cfg, const vpt_grid_desc* density,
                   const vpt_grid_desc* temperature, const float* blackbody_500x3, int device,
                   vpt_gpu_ctx** out);
/* The same context on each of n devices (devices[i]; out[n]) with the grids flattened and majorant-fixed once on
 * the host and uploaded to every device in parallel (the multi-GPU drop-in's setup: one flatten instead of n
 * competing for the host's CPUs).  On failure no context is left (out[] NULL) and vpt_last_error() names the
 * device. */
int vpt_gpu_create_many(const vpt_configuration* cfg, const vpt_grid_desc* density,
                        const vpt_grid_desc* temperature, const float* blackbody_500x3, const int* devices, int n,
                        vpt_gpu_ctx** out);
/* The two halves of vpt_gpu_create_many, for a caller that flattens the grids while the HIP runtime starts
 * (vpt_gpu::run: the flatten is host work and needs no device).  vpt_grids_flatten: the host side of
 * Volume::Volume -- the grids flattened and the density's majorants fixed (no HIP call; the caller's arrays may be
 * freed afterwards).  vpt_gpu_create_from: a context per device from those grids, as vpt_gpu_create_many.  The
 * grids stay the caller's until vpt_grids_free. */
typedef struct vpt_host_grids vpt_host_grids;
int vpt_grids_flatten(const vpt_grid_desc* density, const vpt_grid_desc* temperature, vpt_host_grids** out);
int vpt_gpu_create_from(const vpt_configuration* cfg, const vpt_host_grids* grids, const float* blackbody_500x3,
                        const int* devices, int n, vpt_gpu_ctx** out);
void vpt_grids_free(vpt_host_grids* grids);
int vpt_gpu_destroy(vpt_gpu_ctx* ctx);

/* Jobs per wave T and total jobs num_waves*T of the context's configuration. */
int vpt_gpu_job_space(const vpt_gpu_ctx* ctx, uint64_t* jobs_per_wave, uint64_t* total_jobs);

/* ---- sequences: one context, many frames ---------------------------------------------------
 * A turntable, a fly-through, a look-dev sweep or a simulation sequence renders every frame on one context: the
 * two calls below replace the scene and the volume in place.  The contract of both: a frame rendered after an
 * update equals, byte for byte, the frame of a context created fresh with that configuration and those grids.
 *
 * Both calls are synchronous: they wait for the context's launches (as vpt_gpu_sync), update, and return with the
 * new state on the device.  They are NOT concurrent with any other call on the context (no launch, no setter, no
 * query from another thread while one runs).  Both return VPT_E_STATE while a feed of the context is open or a
 * drop-in frame is open (vpt_gpu_frame_open), leaving the context untouched.
 *
 * What an update keeps: the three gate sets as tuned (vpt_gpu_set_tuning, _set_latency_tuning, _set_full_tuning),
 * the RNG mode, the latency lanes and the pixel chunk, the stencil pool's policy and cap, the film order and its
 * sample buffer, the job order mode and tail, a grid set by vpt_gpu_set_tuning, the latency and compaction
 * settings, the attached moment plane, the denoiser's and the fused adaptive driver's scratch, the context's film
 * (not cleared), the counters and the uploaded tile list.
 * What an update drops, because it belongs to the scene that was replaced: the tile costs and ranks -- computed, or
 * set with vpt_gpu_set_tile_costs -- the band and list ranks filtered from them, and an explicit job permutation
 * (vpt_gpu_set_job_permutation).  The ranks are recomputed by the next call that needs them (one cost pass, counted
 * in vpt_gpu_setup_timings' tile-cost entry); their device buffers are reused, so a sequence allocates nothing per
 * frame.
 *
 * vpt_gpu_set_scene: replaces the configuration.  Everything in `cfg` may change -- seed, num_waves (the job space
 * of vpt_gpu_job_space follows), camera, worker_parameters, volume_parameters -- except output_size and tile_size:
 * a change of either is VPT_E_INVALID, naming the field.  volume_path and num_workers are ignored.  The new scene
 * is validated and derived aside first: on any error the context keeps the scene it had and renders it as before.
 *
 * vpt_gpu_set_grids: replaces the volume by flattened grids (vpt_grids_flatten; they stay the caller's).  The
 * configuration is unchanged: a frame that changes both calls vpt_gpu_set_grids, then vpt_gpu_set_scene.  The
 * temperature grid must be present after the swap exactly if it was before (VPT_E_INVALID otherwise, context
 * untouched): the kernel family hangs on it.  Re-derived as at creation: the upload, the run-skipping choice
 * (vpt_gpu_set_run_skipping's -1 follows the new grid, a forced 0 / 1 stays), the occupancy-sized grid (sized, as
 * at creation, for the kernel the grids choose; a grid set by vpt_gpu_set_tuning stays), the pool's layout under
 * the kept policy and cap, and the scene constants that read the grids.  The old tables and pools are freed before
 * the new ones are allocated, so the peak is one volume.  If the call fails after that free (VPT_E_NOMEM for a
 * volume that does not fit, VPT_POOL_DENSE without room, a HIP error) the context has NO volume: every call that
 * launches, computes tile costs or derives a scene returns VPT_E_STATE until a later vpt_gpu_set_grids succeeds;
 * settings, films and vpt_gpu_destroy keep working.
 *
 * vpt_gpu_set_grids frees device memory that launches may be reading, so beside the context's own launches it waits
 * for the whole device (hipDeviceSynchronize, as vpt_gpu_set_pool_layout does): work of OTHER contexts on the same
 * device is waited for too.  Only this context's feeds are checked -- an open feed of another context on the device
 * (several contexts of vpt_gpu_create_many on one GPU) blocks the swap until that feed is closed. */
int vpt_gpu_set_scene(vpt_gpu_ctx* ctx, const vpt_configuration* cfg);
int vpt_gpu_set_grids(vpt_gpu_ctx* ctx, const vpt_host_grids* grids);
/* Debug (tests of the contract above): the nth grid upload of vpt_gpu_set_grids from now on (1: the density's of the
 * next call, 2: the temperature's of a two-grid swap) returns VPT_E_NOMEM as a device without room returns it, after
 * the old volume was freed; 0 cancels.  One shot. */
int vpt_gpu_debug_fail_upload(vpt_gpu_ctx* ctx, int nth);

/* Render jobs [jid_begin, jid_begin + jid_count) asynchronously on `hip_stream`
 * (a hipStream_t; NULL = the null stream, as everywhere in HIP), accumulating into `film_device`:
 * a device float[H][W][4] (X, Y, Z, sample count; image.hpp:40-60) — NULL = the context's own
 * film.  With the ordered film (the default, vpt_gpu_set_film_order) each pixel's samples are
 * added in wave order, the reference's order, so a film rendered from zero equals the reference's
 * bit for bit; with VPT_FILM_ATOMIC they are fp32 atomics in completion order (≈1e-7 relative).
 *
 * Concurrency: launches of one context may be in flight on several streams at once.  Each launch
 * takes its own job counter from a ring of 64 per context; a ring slot is reused only after the
 * launch that last held it has completed (the new launch's stream waits on an event), so any number
 * of launches is safe.  Launches that share a film add into it atomically (ordered launches -- band launches,
 * vpt_gpu_render_tiles, among them -- run their film passes one after another instead).  The calls that change
 * context state read by running kernels (vpt_gpu_set_tuning, vpt_gpu_set_rng_mode) and
 * vpt_gpu_film_clear first wait for this context's launches.  One context is driven by one host
 * thread at a time (as the reference's `run` owns its RandomNumberGenerator): a state-changing call
 * made from a second thread while the first is inside vpt_gpu_render_jobs is not supported. */
int vpt_gpu_render_jobs(vpt_gpu_ctx* ctx, uint64_t jid_begin, uint64_t jid_count,
                        float* film_device, void* hip_stream);

/* How launches add into the film.  The reference's film receives each pixel's samples in wave order:
 * TileProvider::next() hands a tile's wave out only after its previous wave is released
 * (tile_provider.cpp:40-60), and a job adds each pixel's sample as it is traced (worker.cpp:203-204:
 * w += 1, xyz += imaging_ratio * L).
 *   VPT_FILM_ORDERED (default): a production launch stores every sample's L into a device buffer of
 *     jid_count * tile_w*tile_h * 12 bytes (plain stores, regrouped through the wavefront as the atomics
 *     were), then vpt_film_order_kernel adds them into the film pixel by pixel in wave order: a film
 *     rendered from zero by one launch -- or by launches of consecutive job ranges in jid order -- equals
 *     the reference's bit for bit, and every run gives the same film.  The buffer is the context's (kept
 *     between launches; C3: 6.4 GB, C5 on one GPU: 102 GB); ordered launches of a context run one at a time
 *     (each waits for the previous one's film pass on its stream).  max_bytes caps the buffer (0 = auto:
 *     3/4 of the device's free memory when it grows): a larger launch is split into consecutive launches,
 *     whole waves at a time where the range allows -- the same film.  Band launches (vpt_gpu_render_tiles) use
 *     the same buffer with a layout of their own, the same event and the same cap.
 *   VPT_FILM_ATOMIC: fp32 atomics as samples complete (the order varies run to run, ≈1e-7 relative).
 * Debug launches (records, events) and feeds always add atomically; so does a launch whose buffer would
 * have to grow while a feed of the context is open.  Growing the buffer frees and allocates device memory,
 * which may wait for the whole device (see the feeds below): with feeds of other contexts open on the same
 * device, size it beforehand (a first ordered launch of the largest range, or max_bytes).  Takes effect at
 * the next launch; VPT_FILM_ATOMIC frees the buffer. */
enum { VPT_FILM_ATOMIC = 0, VPT_FILM_ORDERED = 1 };
int vpt_gpu_set_film_order(vpt_gpu_ctx* ctx, int mode, uint64_t max_bytes);
/* The film mode, the sample buffer's size and the launches that ran ordered / atomic (feeds not counted). */
int vpt_gpu_film_order_info(const vpt_gpu_ctx* ctx, int* mode, uint64_t* buffer_bytes, uint64_t* ordered_launches,
                            uint64_t* atomic_launches);

/* The stencil pool's layout.  The sparse pool holds one 9-KiB brick of stencils per leaf, found through the cell
 * table: every trilinear evaluation loads its cell's table entry to learn the leaf's slot, then the stencil -- two
 * dependent memory waits.  The dense pool holds a brick of the same layout for every cell of the table (leaf bricks
 * copied; the bricks of cells without a leaf filled with the getValue of every voxel, neighbours included), so a
 * stencil's address follows from the position alone and the lookup goes.  Every value read is the same bits: films,
 * records and counters do not depend on the layout.  The dense pool is table cells x 9216 bytes per grid (the 512^3
 * stand-in: 2.4 GB beside the 0.84-GB sparse pool, which stays resident: the tree walk and points outside the table
 * read it).  It is expanded on the device from the uploaded tables; nothing more is uploaded.
 *   VPT_POOL_AUTO (a context's default): dense when the dense bytes of all its grids together are at most the cap --
 *     vpt_gpu_set_pool_cap's, else 1/8 of the device's memory -- and the allocation succeeds; else sparse, silently
 *     (vpt_gpu_pool_info tells).  VPT_POOL_DENSE: dense, or VPT_E_NOMEM.  VPT_POOL_SPARSE frees the dense pool.
 * The environment variable VPT_POOL_LAYOUT (sparse, dense or auto) replaces the default of contexts created while it
 * is set.  Callable while no feed or frame of the context is open (else VPT_E_STATE); waits for the context's
 * launches.  Allocating and freeing device memory may wait for the whole device (see the feeds below). */
enum { VPT_POOL_SPARSE = 0, VPT_POOL_DENSE = 1, VPT_POOL_AUTO = 2 };
int vpt_gpu_set_pool_layout(vpt_gpu_ctx* ctx, int layout);
/* The cap VPT_POOL_AUTO compares the dense bytes with (0 = 1/8 of the device's memory).  Read by the next
 * vpt_gpu_set_pool_layout; changes nothing by itself. */
int vpt_gpu_set_pool_cap(vpt_gpu_ctx* ctx, uint64_t max_bytes);
/* *layout: the layout in use (VPT_POOL_SPARSE or VPT_POOL_DENSE); *policy: the one asked for; sparse_bytes[2],
 * dense_bytes[2]: the pools' resident bytes of the density and the temperature grid (0 for a pool or a grid that is
 * not there); *expand_ms: what the last expansion's kernels took (HIP events).  Any pointer may be NULL. */
int vpt_gpu_pool_info(const vpt_gpu_ctx* ctx, int* layout, int* policy, uint64_t* sparse_bytes, uint64_t* dense_bytes,
                      double* expand_ms);
/* Debug (tests): copies the dense bricks of the table cells [cell_begin, cell_begin + cell_count) of the density
 * (grid 0) or temperature (grid 1) grid into out (cell_count x 2304 floats).  VPT_E_STATE without a dense pool. */
int vpt_gpu_debug_read_pool(vpt_gpu_ctx* ctx, int grid, uint64_t cell_begin, uint64_t cell_count, float* out);

/* A band launch: renders the jobs { (wave_begin + w) * T + t : t in [tile_lo, tile_hi), w in [0, wave_count) } --
 * wave_count waves (0-based) of a band of consecutive tiles -- asynchronously on `hip_stream`, adding into
 * `film_device` (NULL = the context's own film).  It is the partition a multi-GPU frame needs to stay bit-exact:
 * each pixel's samples are added in wave order (w += 1, xyz += imaging_ratio * L, vpt_film_order_kernel's
 * sequence), so a band rendered from a zero film equals the reference's film on the band's pixels bit for bit,
 * every other pixel is left untouched, and the films of disjoint bands sum exactly (x + (+0.0) == x).  Every job
 * keeps its jid and its RNG stream.
 *   Order and layout: the same-tile order restricted to the band -- the band's tiles by descending cost
 *     (vpt_gpu_tile_costs, ties as there), each tile's waves consecutively, whatever vpt_gpu_set_job_order says;
 *     grid size, latency kernel and gate set are chosen from the (tile_hi - tile_lo) * wave_count work items as
 *     vpt_gpu_render_jobs chooses them from jid_count.  The samples are stored in groups of 64 waves, a pixel's 64
 *     samples of a group adjacent (the 64 lanes of a wavefront store 768 contiguous bytes), in the context's sample
 *     buffer: (tile_hi - tile_lo) * ceil(wave_count / 64) * 64 * tile_w*tile_h * 12 bytes.
 *   Ordered film only: VPT_E_STATE with VPT_FILM_ATOMIC, while a frame is open (vpt_gpu_frame_open), and when the
 *     sample buffer would have to grow while a feed of the context is open (size it beforehand).  There are no
 *     records or events variants.
 *   VPT_E_INVALID: a null context, tile_lo >= tile_hi or tile_hi > T, the pixel RNG mode, 2^32 or more sample
 *     slots (wave_count rounded up to 64, times max(T, tile_hi - tile_lo)).  wave_count == 0 does nothing (VPT_OK).
 *   Band launches count as ordered launches (vpt_gpu_film_order_info) and run one at a time with the context's
 *     other ordered launches (each waits on its stream for the previous one's film pass).  Over max_bytes
 *     (vpt_gpu_set_film_order) a band launch is split into consecutive blocks of waves, multiples of 64 where the
 *     cap allows, each with its own film pass in wave order: the same film.  VPT_E_NOMEM when not one wave of the
 *     band fits.  Apart from the sample buffer nothing is allocated per launch (the band's tile ranks live in a
 *     buffer of T words allocated with the tile costs), so a launch never waits for a running feed. */
int vpt_gpu_render_tiles(vpt_gpu_ctx* ctx, uint32_t tile_lo, uint32_t tile_hi, uint64_t wave_begin,
                         uint64_t wave_count, float* film_device, void* hip_stream);

/* Adaptive sampling.  Four calls: a second-moment plane the ordered film passes keep beside the film, a launch
 * over an arbitrary list of tiles, a per-tile error estimate, and a driver that renders every tile until its
 * estimate is below a target.  A tile stopped after k waves holds exactly the reference's film of that tile after
 * k waves: every job keeps its jid and RNG stream, so adaptive sampling takes a per-tile prefix of the reference's
 * sample set and never leaves it.  Out of scope: the drop-in vpt_gpu::run (the reference's TileProvider dictates
 * its jobs), the multi-GPU modes, feeds, and the pixel RNG mode.
 *
 * The moment plane: `m2_device` is a device float[H][W] owned by the caller; NULL detaches.  While a plane is
 * attached every ordered production launch (vpt_gpu_render_jobs, vpt_gpu_render_tiles, vpt_gpu_render_tile_list,
 * the launches they are split into under max_bytes included) also does, for each sample it adds to a pixel, after
 * the four adds of the film and in the same wave order,
 *     y = imaging_ratio * L.y;   m2 = m2 + y * y          (fp32, not contracted)
 * reading and writing the plane once per pixel per pass.  Pixels that receive no sample (outside the band or list,
 * a ragged tile's padding, every other pixel in single-pixel mode) are not touched.  VPT_E_STATE with
 * VPT_FILM_ATOMIC and while a frame is open.  With a plane attached a launch that would add with film atomics --
 * a debug launch (records, events), the pixel RNG mode, VPT_FILM_ATOMIC, an open frame, a sample buffer that would
 * have to grow while a feed of the context is open -- fails with VPT_E_STATE instead of leaving the plane behind
 * the film.  Feeds are unaffected and never write the plane.  Takes effect at the next launch. */
int vpt_gpu_set_film_moments(vpt_gpu_ctx* ctx, float* m2_device);

/* Light groups.  The radiance is linear in the reference's three sources -- blackbody emission at collisions
 * (worker.cpp:156), the distant light through sample_Ld (:175), the infinite light on escape (:199) -- and no random
 * draw depends on their strength (apart from sample_Ld's test Li == 0), so one set of paths holds every relit
 * picture once the three sums are kept apart.
 *
 * `groups_device` is a device float[3][H][W][4] owned by the caller (16-byte aligned), in the order emission, sun,
 * sky; each plane is an ordinary XYZW film.  NULL detaches.  The contract is vpt_gpu_set_film_moments': while
 * attached every ordered production launch (vpt_gpu_render_jobs, vpt_gpu_render_tiles, vpt_gpu_render_tile_list,
 * the launches they are split into under max_bytes included) keeps, beside each sample's L, one fp32 accumulator per
 * group that receives only that group's adds, in path order and not contracted,
 *     emission:  E = E + (p_a * le_scale) * XYZ           at every collision (worker.cpp:156)
 *     sun:       D = D + (p * T_ray) * Li                  or D + 0.0f when sample_Ld returned zero (:175)
 *     sky:       le_inf if the path escaped, else +0.0     (:199)
 * and after the film's four adds, in the same wave order, does for each group g
 *     G[g].w = G[g].w + 1;   G[g].xyz = G[g].xyz + imaging_ratio * Lg.xyz       (fp32, not contracted).
 * A scene without a temperature grid adds +0.0 samples to the emission plane.  Each plane is therefore, bit for bit
 * (up to the sign of a zero), the film the reference renders with the other two sources switched off.  The beauty
 * film is unchanged; it is NOT the sum of the planes bit for bit (fp32 addition does not associate), only to a few
 * ulp.  Pixels that receive no sample are not touched.  The moment plane and the groups combine.
 * Memory: the sample buffer of a launch holds 48 bytes per sample instead of 12 (the sample, then its three group
 * terms, 12 bytes each, in four regions of the same layout); max_bytes splits launches accordingly and
 * vpt_gpu_film_order_info reports the buffer.  Launches with groups run the throughput kernels.
 * VPT_E_STATE with VPT_FILM_ATOMIC and while a frame is open.  With groups attached a launch that would add with
 * film atomics -- a debug launch (records, events), the pixel RNG mode, VPT_FILM_ATOMIC, an open frame, a sample
 * buffer that would have to grow while a feed of the context is open -- and vpt_gpu_render_adaptive_fused fail with
 * VPT_E_STATE instead of leaving the planes behind the film.  Feeds are unaffected and never write the planes.  The
 * attachment survives vpt_gpu_set_scene and vpt_gpu_set_grids.  Takes effect at the next launch. */
int vpt_gpu_set_light_groups(vpt_gpu_ctx* ctx, float* groups_device);

/* Relights group planes: for each pixel of the context's W x H frame
 *     out.c = ((G0.c * k0.c) + (G1.c * k1.c)) + (G2.c * k2.c)   for c = X, Y, Z;     out.w = G0.w
 * in fp32, in this order, not contracted.  `groups_device`: float[3][H][W][4] as above; `gains`: host, row-major
 * [group][XYZ]; `film_out_device`: float[H][W][4], which must not overlap the planes (VPT_E_INVALID).  Both 16-byte
 * aligned.  One small kernel on `hip_stream`; the call does not wait for it. */
int vpt_gpu_relight(vpt_gpu_ctx* ctx, const float* groups_device, const float gains[9], float* film_out_device,
                    void* hip_stream);

/* Camera motion blur: a camera per wave from a shutter table.  An entry holds the four camera fields a frame of a
 * sequence replaces; imaging_ratio stays the scene's. */
typedef struct vpt_shutter_camera {
  float position[3];
  float look[3];
  float up[3];
  float vfov_deg;
} vpt_shutter_camera;
#define VPT_SHUTTER_MAX 65536u

/* Attaches a shutter of `n` cameras (1 .. VPT_SHUTTER_MAX; the library copies them), or detaches it (cams == NULL and
 * n == 0; any other null / zero mix is VPT_E_INVALID).  A job is one tile in one wave, its wave is jid / T, and its
 * RNG stream depends on jid alone.  While a shutter is attached, job jid of vpt_gpu_render_jobs, vpt_gpu_render_tiles
 * and vpt_gpu_render_tile_list -- the launches they are split into under max_bytes included -- generates its primary
 * rays (Camera::generate_ray, camera.hpp:14-23) through entry (jid / T) % n instead of the scene's camera.  Nothing
 * else changes, no random draw included: the film is, bit for bit, the ordered fp32 sum of the films the reference
 * renders wave by wave, wave k with the scene whose camera is entry k % n.  An attached moment plane and attached
 * light-group planes keep their contracts on those samples.
 * Each entry is turned into the scene's 15 camera floats by the code that derives the scene's own camera (it reads
 * output_size besides the entry, which cannot change) and uploaded as a 64-byte row of the table.  An entry with a
 * non-finite field, look == position, an up vector that is zero or along the view direction, or vfov_deg outside
 * (0, 180) is VPT_E_INVALID naming its index, and the context keeps the shutter it had.
 * A sync point like vpt_gpu_set_scene (it waits for the context's launches); VPT_E_STATE while a feed of the context
 * or a drop-in frame is open.  The attachment survives vpt_gpu_set_scene and vpt_gpu_set_grids.
 * Launches with a shutter run the throughput kernels' Shutter instantiations (ordered launches: it needs
 * VPT_FILM_ORDERED).  Calls that cannot honour it fail with VPT_E_STATE while it is attached instead of rendering the
 * still camera: vpt_gpu_render_jobs_records, vpt_gpu_trace_jobs, the pixel RNG mode, VPT_FILM_ATOMIC, a feed's
 * launch, vpt_gpu_frame_open, vpt_gpu_render_adaptive_fused, vpt_gpu_render_alpha and vpt_gpu_render_depth (the
 * matte and the depth would be another camera's).  The tile-cost pass keeps using the scene's camera: only the schedule depends on it, never a sample. */
int vpt_gpu_set_shutter(vpt_gpu_ctx* ctx, const vpt_shutter_camera* cams, uint32_t n);
/* The attached shutter's entries, 0 if none. */
int vpt_gpu_shutter_info(const vpt_gpu_ctx* ctx, uint32_t* n);
/* One row of the shutter table as the library derives it for a width x height frame (host only, no device):
 * out16[4 i .. 4 i + 3] = cam_L[3 i], cam_L[3 i + 1], cam_L[3 i + 2], cam_t[i] for i = 0, 1, 2 (the rows of
 * Camera::raster_to_world_dir), out16[12 .. 14] = position, out16[15] = 0.  VPT_E_INVALID as vpt_gpu_set_shutter. */
int vpt_shutter_entry(const vpt_shutter_camera* cam, uint32_t width, uint32_t height, float* out16);

/* A tile-list launch: vpt_gpu_render_tiles for the tiles tiles[0..n) (a host array, strictly ascending, every entry
 * < T) instead of [tile_lo, tile_hi): renders the jobs (wave_begin + w) * T + tiles[i], w in [0, wave_count), adds
 * each pixel's samples in wave order and touches no pixel outside the listed tiles.  Order: the list's tiles by
 * descending cost (ties as in vpt_gpu_tile_costs' ranks), each tile's waves consecutively; the samples lie as a
 * band's, the tile's index in the list in place of its offset in the band (n * ceil(wave_count / 64) * 64 *
 * tile_w*tile_h * 12 bytes).  The same rules as band launches: ordered film only, no open frame (VPT_E_STATE), the
 * reference RNG mode (VPT_E_INVALID), split by waves under max_bytes, VPT_E_NOMEM when not one wave fits, counted
 * as ordered launches; wave_count == 0 or n == 0 does nothing (VPT_OK).  Also VPT_E_INVALID for an unsorted or
 * duplicated list or an entry >= T, and VPT_E_STATE while a feed of the context is launched and not closed: the
 * list is uploaded by the call (two buffers of T words allocated with the tile costs; the call first waits for the
 * context's previous ordered launch, which may still read them), and an upload must not wait for a launch that
 * holds the device.  A list equal to the previous call's is not uploaded again. */
int vpt_gpu_render_tile_list(vpt_gpu_ctx* ctx, const uint32_t* tiles, uint32_t n, uint64_t wave_begin,
                             uint64_t wave_count, float* film_device, void* hip_stream);

/* Per-tile error estimates of a film and its moment plane (film_device NULL = the context's own film), synchronous:
 * launched on `hip_stream`, err_T_host[t] is valid on return.  Everything is fp32, in exactly this order.  Pixel q
 * of tile t (q = y_local * rect_w + x_local) is counted if it lies in the image, is the single pixel when that
 * mode is on, and n = film.w >= 2; a counted pixel has
 *     mean = film.y / n;  ex2 = m2 / n;  v = ex2 - mean * mean, 0 unless v > 0;  se = sqrtf(v / (n - 1.0f))
 * and any other pixel se = mean = +0.0.  Both arrays, indexed by q and padded with +0.0 to P, the power of two >=
 * tile_w*tile_h, are reduced by the tree: for h = P/2, P/4, .., 1: a[i] = a[i] + a[i + h], i < h.  Then
 *     err_t = se[0] / (mean[0] + abs_floor * (float)cnt)      (cnt = counted pixels; err_t = 0 when cnt == 0)
 * -- the tile's mean standard error of Y relative to its mean Y, abs_floor keeping dark tiles finite.  Division and
 * square root are correctly rounded.  VPT_E_INVALID when abs_floor <= 0, when m2_device or err_T_host is null, and
 * for tiles of more than 8192 pixels (the tree is reduced in LDS); VPT_E_STATE while a feed of the context is
 * open. */
int vpt_gpu_tile_errors(vpt_gpu_ctx* ctx, const float* film_device, const float* m2_device, float abs_floor,
                        float* err_T_host, void* hip_stream);

/* The adaptive driver, synchronous.  film_device (NULL = the context's film) and m2_device start as zeros: the
 * caller zeroes them.  The call attaches m2_device and restores the previous attachment on return.
 *   Round 0 renders waves [0, min_waves) of every tile.  Every later round computes vpt_gpu_tile_errors, keeps the
 *   tiles of the previous round's list with err_t > target_error that are below max_waves, and renders the next
 *   min(step_waves, max_waves - done) waves of exactly those with one list launch; it stops when the list is empty.
 *   A tile that leaves the list never returns, so every listed tile has the same wave count and the result is a
 *   per-tile prefix of the uniform frame's samples.  target_error == 0 stops no tile -- not even a black one, whose
 *   estimate is exactly 0 -- so every tile gets max_waves and the film is the uniform frame's, byte for byte.
 * waves_T_host[t]: the waves tile t received.  err_T_host[t]: its error in the returned film (a last
 * vpt_gpu_tile_errors call follows the last round).  out (may be NULL): rounds (round 0 included), tiles_at_max,
 * jobs_rendered (the sum of waves_T_host), jobs_uniform = max_waves * T, max_error.
 * VPT_E_INVALID: a null argument, min_waves < 2, step_waves == 0, max_waves < min_waves, target_error < 0 or NaN,
 * abs_floor <= 0.  Otherwise the errors of the calls above.
 * Caveat, the usual one of adaptive sampling: a stopping rule fed by the samples it stops biases the estimate
 * slightly (tiles whose first samples happen to agree stop early).  min_waves is the guard against it. */
typedef struct vpt_adaptive_params {
  float target_error, abs_floor;
  uint32_t min_waves, step_waves, max_waves;
} vpt_adaptive_params;

typedef struct vpt_adaptive_result {
  uint32_t rounds, tiles_at_max;
  uint64_t jobs_rendered, jobs_uniform;
  float max_error;
} vpt_adaptive_result;

int vpt_gpu_render_adaptive(vpt_gpu_ctx* ctx, const vpt_adaptive_params* p, float* film_device, float* m2_device,
                            uint32_t* waves_T_host, float* err_T_host, vpt_adaptive_result* out, void* hip_stream);

/* The adaptive driver in one launch.  The same contract, arguments, outputs and parameter errors as
 * vpt_gpu_render_adaptive, and the same bytes: film, plane, waves_T_host, err_T_host and *out equal the rounds
 * driver's bit for bit (rounds = 1 + the later boundaries the longest-running tile crossed).  The stopping rule is per
 * tile, so no round needs the others: a wavefront of the throughput kernel owns a tile.  It claims tiles by
 * descending cost (vpt_gpu_tile_costs' ranks) from a counter; renders the tile's waves in groups of up to 64, one job
 * per lane, up to the next boundary (min_waves, then + step_waves each time, cut at max_waves); adds each group's
 * samples into the tile's film and plane pixels itself, in wave order, with the ordered film passes' sequence; at a
 * boundary evaluates the tile's estimate with vpt_gpu_tile_errors' arithmetic and tree and goes on iff
 * (target_error == 0 || err > target_error) and the tile is below max_waves; else stores the tile's waves and error
 * and claims again.  No host read-back, no drain between rounds, and no lane ever waits for another wavefront.
 *   Synchronous; the caller zeroes film_device (NULL = the context's film) and m2_device.  The plane is passed to
 *   the launch directly: the context's attachment (vpt_gpu_set_film_moments) is neither used, changed nor written.
 *   One ordered launch in vpt_gpu_film_order_info, on the throughput kernel's full resident grid (wavefronts beyond
 *   the T tiles end at their first claim) with the full-launch gates.
 *   Memory: the context's sample buffer is neither used nor resized and max_bytes does not apply.  The context keeps
 *   wavefronts x tile_w*tile_h x 64 x 12 bytes of scratch (8 x 8 tiles on a full grid: about 350 MB) and T words of
 *   wave counts, allocated by the first call and freed by vpt_gpu_destroy.  Two calls on one context must not
 *   overlap (they share that scratch).
 *   Limit: tiles of at most 256 pixels (tile_w*tile_h; the error tree is held in registers, four values per lane) --
 *   VPT_E_INVALID beyond; vpt_gpu_render_adaptive renders larger tiles.
 * VPT_E_INVALID also for the pixel RNG mode.  VPT_E_STATE with VPT_FILM_ATOMIC, while a frame is open, and while a
 * feed of the context is launched and not closed (the call allocates and waits for its launch).  Not covered, as for
 * the rounds driver: the drop-in vpt_gpu::run, the multi-GPU modes, feeds, the pixel RNG mode. */
int vpt_gpu_render_adaptive_fused(vpt_gpu_ctx* ctx, const vpt_adaptive_params* p, float* film_device, float* m2_device,
                                  uint32_t* waves_T_host, float* err_T_host, vpt_adaptive_result* out,
                                  void* hip_stream);

/* Alpha (coverage).  One deterministic pass that says how much of each pixel the medium covers: no random numbers,
 * no noise, a small fraction of a frame's cost.  Asynchronous on `hip_stream`; reads the scene and the density grid
 * only (never a film, a moment plane or the temperature grid) and writes the caller's planes.
 *
 * Definition.  Under delta tracking a primary ray has no real collision with probability exp(-tau),
 *     tau = sigma_t * integral of rho ds over the ray's positive-majorant segments
 * (RayMajorantIterator's segments inside Volume::intersect's clip; a segment whose majorant is <= 0 draws nothing
 * and counts nothing; rho is the trilinear density the integrator evaluates).  The pass walks the integrator's own
 * clip and segments, cuts every positive segment where the ray crosses an integer lattice plane of index space --
 * the field is a cubic of t between two crossings -- and adds Simpson's rule per piece,
 *     (tb - ta) * ((rho(ta) + 4 rho(tm)) + rho(tb)),  tm = ta + 0.5 (tb - ta),
 * pieces into their segment's sum, segment sums into the ray's, tau = (sigma_t * m_scale) * (sum / 6) clamped at
 * >= 0.  All fp32, not contracted, divisions and square roots correctly rounded, crossing times computed from
 * their integer plane as (k - e) * invDir (never accumulated): the tau plane is a function of the scene alone and
 * equals the host build of the same code (csrc/vpt_alpha.h) bit for bit.  A ray that misses the clip has tau = +0.
 *
 * Footprint.  `sub` in 1..8 sub-rays per axis.  The reference jitters a pixel's raster point over
 * [px + 0.5, px + 1) x [py + 0.5, py + 1) (jitter scale 0.5, worker.cpp:122); the matte averages that footprint.
 * Sub-ray (i, j), i, j in [0, sub), has the raster point
 *     ((float)px + 0.5f) + jitter_scale * (((float)i + 0.5f) / (float)sub),   likewise y with j,
 * and the camera ray Camera::generate_ray forms from it (the integrator's expressions and order).  With use_jitter
 * off all sub-rays coincide and one is evaluated (n = 1; otherwise n = sub * sub).
 *
 * Outputs, device float[H][W], caller-owned.  With the sub-rays taken in row-major order (j outer, i inner):
 *     alpha = 1 - (sum_k expf(-tau_k)) / n          tau = (sum_k tau_k) / n   (tau_device may be NULL)
 * both sums in that fixed order.  For n == 1 the tau plane is the ray's optical depth.  Every pixel of the frame is
 * written, so the caller need not clear; in single-pixel mode only that pixel is.  Rays that miss store +0.0.
 * The alpha plane depends on the platform's expf: within 2^-22 of 1 - exp(-tau) for n == 1.
 *
 * Launch: one wavefront per (tile, chunk of 64 pixels), tiles by descending cost (vpt_gpu_tile_costs' ranks, which
 * the context computes once, at the first call that needs them; nothing else is allocated).
 * VPT_E_INVALID: a null context or alpha plane, sub outside 1..8.  VPT_E_STATE while a feed of the context is
 * launched and not closed (the tile-list launch's rule: the pass must not queue behind a launch that holds the
 * device).  Out of scope: the drop-in vpt_gpu::run (the reference's film has no alpha), the multi-GPU modes,
 * per-band alpha and other AOVs.  Depth planes: the block "Depth" below. */
int vpt_gpu_render_alpha(vpt_gpu_ctx* ctx, uint32_t sub, float* alpha_device, float* tau_device, void* hip_stream);

/* Depth.  Noise-free opacity-threshold depths, a by-product of the matte's march: for each of up to four opacities
 * the distance from the camera before which that fraction of all primary paths has had its first real collision.
 * The rules of vpt_gpu_render_alpha: asynchronous on `hip_stream`, takes a launch slot (vpt_gpu_sync covers it),
 * reads the scene and the density grid only, allocates nothing beyond the tile ranks the context computes once.
 *
 * Levels.  `n_levels` in 1..VPT_DEPTH_MAX_LEVELS opacities 0 < a_0 < a_1 < ... < 1 (host array).  Each becomes an
 * optical depth once, on the host: tau_k = (float)(-log1p(-(double)a_k)).  a = 1/255 is the front surface of what
 * an 8-bit matte shows, a = 0.5 the median free-flight depth.
 *
 * Definition.  For one primary ray z_k is the world distance from the camera position along the unit camera
 * direction at which the accumulated optical depth first reaches tau_k.  The optical depth accumulates over the
 * ray's positive-majorant segments exactly as the Alpha block says: lattice pieces into their segment's sum,
 * segment sums into the ray's.  A ray that never reaches tau_k has no z_k.  World distance is the march's
 * index-space ray time -- measured from the camera position, not from the clip entry -- multiplied by m_scale, the
 * factor the optical depth is multiplied by.
 *   Piece test.  After each piece the accumulated tau is formed by the expression that forms the ray's final tau,
 *       (sigma_t * m_scale) * ((total + sum) / 6)      total: the finished segments, sum: the running segment,
 * the division correctly rounded, and compared with the next level: reached when tau >= tau_k.  Hence, bit for
 * bit at sub = 1: level k is reached if and only if tau_plane >= tau_k, tau_plane being what vpt_gpu_render_alpha
 * stores for the pixel (non-negative densities; the levels are tested in ascending order, so the reached levels
 * are a prefix).
 *   Bisection.  In the piece [ta, tb] where the test first passes: lo = ta, hi = tb, then 16 times
 *       tm = lo + 0.5 (hi - lo);  h = tm - ta;  part = h * ((rho(ta) + 4 rho(ta + 0.5 h)) + rho(tm))
 *       pass = (sigma_t * m_scale) * ((total + (sum_before_piece + part)) / 6) >= tau_k;  pass ? hi = tm : lo = tm
 * (Simpson's rule again: exact, because the field is one cubic on the whole piece).  The upper end always passes
 * the test under this arithmetic and is kept: z_k = hi * m_scale.  Several levels may fall into one piece; they
 * are handled in turn, each from [ta, tb].  fp32, not contracted, only +, *, comparisons and correctly rounded
 * division: the planes equal the host build of the same code (csrc/vpt_depth.h) bit for bit; no expf is involved.
 *   Early stop.  A ray stops marching as soon as its last level is reached.  Every loop keeps the matte's bounds
 * (HDDA steps per ray, pieces per segment counted before the loop, the NaN-time exit); a zero or non-finite
 * direction is no ray.
 *   Negative densities (a signed grid): "first reaches" is the first piece whose test passes and the bisection
 * returns one crossing within it; the result stays deterministic and equal on host and device, but the
 * equivalence with the tau plane need not hold.
 *
 * Footprint: the matte's -- `sub` in 1..8, the same raster points in row-major order, one ray with jitter off (n = 1;
 * otherwise n = sub * sub).
 *
 * Outputs, device float[n_levels][H][W], caller-owned, written for every pixel (in single-pixel mode only that one):
 *     depth[k][y][x] = (sum of z_k over the sub-rays that reached level k, in that order) / (their count),
 *                      +0.0 when none reached
 *     reach[k][y][x] = count / n     (reach_device may be NULL) the anti-aliased mask of "opacity at least a_k",
 *                      which makes the mean well defined for a consumer.
 *
 * VPT_E_INVALID: a null context, opacity array or depth plane, sub outside 1..8, n_levels outside 1..4, an opacity
 * not in (0, 1) (a NaN included), opacities not strictly ascending.  VPT_E_STATE while a feed of the context is
 * launched and not closed, and while a shutter is attached (the depth would be another camera's).  Out of scope:
 * depth under a shutter, the drop-in vpt_gpu::run and feeds, the multi-GPU modes, mean collision depth and deep
 * output, position planes (motion vectors: the block "Temporal" below). */
#define VPT_DEPTH_MAX_LEVELS 4
int vpt_gpu_render_depth(vpt_gpu_ctx* ctx, uint32_t sub, uint32_t n_levels, const float* opacity_host,
                         float* depth_device /* [n_levels][H][W] */, float* reach_device /* same shape, may be NULL */,
                         void* hip_stream);

/* Denoise.  A variance-guided a-trous filter over a film and its moment plane, optionally guided by up to four
 * feature planes (the matte's alpha and tau / (1 + tau) are the ones a volume has).  The film is not changed: the
 * denoised film is a second output, an ordinary film (XYZ sums and the count n) that every film consumer takes.
 * Asynchronous on `hip_stream`; takes a launch slot, so vpt_gpu_sync covers it; reads film, plane and guides only;
 * works on any film with a matching plane (uniform, band, tile-list, either adaptive driver: tiles may hold different
 * wave counts); independent of the scene and of the RNG mode.
 *
 * Arithmetic (fp32, not contracted, only + - * /, sqrtf, fabsf and comparisons, divisions and square roots
 * correctly rounded, in exactly this order: csrc/vpt_denoise.h is the code, tests/denoise_ref.py its numpy
 * restatement, and the device, the host build and numpy give the same bytes).
 *   Prepare, per pixel.  Valid iff n >= 1 (film.w; NaN is invalid).  c = xyz / n.  n >= 2:
 *     v = max(m2 / n - c.y c.y, 0) / (n - 1)   (the square of vpt_gpu_tile_errors' se, its expression order);
 *   otherwise v = c.y c.y.  An invalid pixel is never a tap (a select, so NaN or garbage in an unrendered pixel
 *   cannot leak) and its output is its input, copied.
 *   Iteration i = 0 .. iterations - 1, step s = 2^i, per valid pixel p:
 *     gv  = (sum b v_q) / (sum b) over the valid in-image neighbours q = p + (dx, dy), dy, dx in -1..1 (dy outer),
 *           b = b3[dy] * b3[dx], b3 = {1/4, 1/2, 1/4}, both sums sequential;
 *     den = (sigma_l * sqrtf(gv) + rel_floor * c_p.y) + 1e-20f;
 *     for q = p + s (dx, dy), dy, dx in -2..2 (dy outer), in the image and valid:
 *       d = fabsf(c_p.y - c_q.y) / den;   w = (h[dy] * h[dx]) / (1 + d d),   h = {1/16, 1/4, 3/8, 1/4, 1/16};
 *       for k = 0 .. n_guides - 1:  e = (g_k[p] - g_k[q]) / guide_sigma[k];  w = w / (1 + e e);
 *       acc += w c_q;   accv += (w w) v_q;   ws += w;        (sequential; the centre tap always counts: ws > 0)
 *     c_p' = acc / ws;   v_p' = accv / (ws ws).
 *   Iterations ping-pong between two packed planes; none reads what it writes.
 *   Finish.  out.xyz = c n, out.w = n.  var_out (may be NULL) receives the final v, the filtered variance of the
 *   mean of Y (a confidence map); +0 at an invalid pixel.
 *
 * Kernels: vpt_denoise_prepare_kernel packs (c, v) and the guides into float4 planes (an invalid pixel has v = -1),
 * vpt_denoise_atrous_kernel<G> runs once per iteration in blocks of 64 x 4 pixels -- a wavefront owns 64
 * consecutive pixels of a row, so every tap is one 16-byte load per lane -- and the last iteration stores the
 * finished film.  Scratch: 32 bytes per pixel, 48 with guides; it belongs to the context, is allocated by the
 * first call, grown when a later call needs more and freed by vpt_gpu_destroy.  Every call of a context uses the
 * same planes, so calls are serialised on the device: a call's kernels wait, on its own stream, for the previous
 * call's last iteration whatever stream that ran on (an event, as for the ordered film's sample buffer), and calls
 * from several threads take a lock around their launches.  Calls on different streams are therefore safe and run
 * one after the other; the caller's film, plane and guides must be ready on `hip_stream`.
 * Alignment: film_device and out_film_device are read and written 16 bytes at a time and must be 16-byte aligned
 * (any device allocation is); the planes and guides must be 4-byte aligned.
 *
 * VPT_E_INVALID: a null context, params, film, plane or output film; iterations outside 1..6; n_guides > 4 or a null
 * guide; sigma_l, rel_floor or a used guide_sigma that is not > 0 (NaN included); a film that is not 16-byte or a
 * plane that is not 4-byte aligned; an output that overlaps an input or the other output.  VPT_E_STATE while a feed of the context is launched and not closed (the tile-list launch's
 * rule: the call allocates and must not queue behind a launch that holds the device).  Out of scope: the drop-in
 * vpt_gpu::run and feeds (no moment plane there), the multi-GPU modes (temporal: the block below), colour-channel
 * variances (only Y has a moment), learned denoisers. */
typedef struct vpt_denoise_params {
  uint32_t iterations; /* 1..6; 4 is a good default */
  uint32_t n_guides;   /* 0..4 */
  float sigma_l;       /* Y distance scale in local standard deviations; default 4 */
  float rel_floor;     /* relative floor of that scale; default 1e-3 */
  float guide_sigma[4];
} vpt_denoise_params;
int vpt_gpu_denoise(vpt_gpu_ctx* ctx, const vpt_denoise_params* p, const float* film_device, const float* m2_device,
                    const float* const* guides_device /* n_guides device planes float[H][W]; may be NULL when 0 */,
                    float* out_film_device, float* var_out_device /* may be NULL */, void* hip_stream);

/* Temporal.  Accumulation across the frames of a sequence: the previous frame's accumulated film, reprojected through
 * the current frame's depth planes, is added to the current film.  A film is sums and a count, so history is added,
 * not blended; the result is an ordinary film with a matching moment plane, which vpt_gpu_denoise and every film
 * consumer take unchanged, and -- with this frame's depth planes and camera -- it is the next frame's history (the
 * caller swaps two buffer sets).  Asynchronous on `hip_stream`; takes a launch slot, so vpt_gpu_sync covers it; reads
 * its inputs only and allocates nothing.  The current camera is the context's scene camera (vpt_gpu_set_scene);
 * `prev_cam`, the camera the history was rendered with, becomes camera floats by the code that derives the scene's
 * camera and a shutter entry (vpt_shutter_entry), under vpt_gpu_set_shutter's validation.
 *
 * Arithmetic (fp32, not contracted, only + - * /, sqrtf, floorf, fabsf, comparisons and selects, divisions and square
 * roots correctly rounded, in exactly this order: csrc/vpt_temporal.h is the code, tests/temporal_ref.py its numpy
 * restatement, and the device, the host build and numpy give the same bytes).  dot(u, v) = u0 v0 + (u1 v1 + u2 v2);
 * cross(u, v) = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0).  L, t, pos: cam_L (row-major), cam_t and the position
 * of the current camera; L', t', pos': the previous camera's; L0', L1': the first two columns of L'.
 *   Previous camera, once, on the host (passed as kernel arguments):
 *     n = cross(L0', L1');  nn = dot(n, n);  a = cross(L1', n) / nn;  b = cross(n, L0') / nn   (per component);
 *     tn = dot(t', n);  ta = dot(t', a);  tb = dot(t', b).
 *   These solve t' + L0' rx + L1' ry = lambda q for a direction q:  lambda = tn / dot(q, n),
 *   rx = lambda dot(q, a) - ta,  ry = lambda dot(q, b) - tb.
 *   Per pixel p = (x, y):
 *   Depth.  z = depth[k][p] for the largest k < n_levels with depth[k][p] > 0 (the reached levels are a prefix);
 *     foreground iff there is one, else background.  The history's taps use the same rule on hist_depth.
 *   Position.  rx = (float)x + 0.5f, ry = (float)y + 0.5f;  dv_i = t_i + (L_i0 rx + (L_i1 ry + L_i2 0.0f));
 *     n2 = dv0 dv0 + (dv1 dv1 + dv2 dv2);  d = dv / sqrtf(n2) when n2 > 0  (Camera::generate_ray without jitter, the
 *     integrator's expressions: the direction the depth is measured along).
 *     Foreground: q = (pos + z d) - pos',  r = sqrtf(dot(q, q)).  Background: q = d (a point at infinity: rotation only).
 *   Projection.  lambda, px = rx', py = ry' as above.  There is a projection iff lambda > 0 and lambda, px and py are
 *     finite.  motion_out[p] = (px - rx, py - ry), else a NaN pair; written whether or not a history is given.
 *   Taps.  fx = px - 0.5f, fy = py - 0.5f, in range iff -1 < fx < W and -1 < fy < H (tested before any conversion to
 *     an integer);  x0 = floorf(fx), ax = fx - x0, likewise y.  The taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 *     (x0 + 1, y0 + 1), in this order, have w = (1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay.  A tap q is usable
 *     iff it lies in the image, its count n_q = hist_film[q].w >= 1 (NaN is not) and it agrees in depth -- foreground:
 *     z_q > 0 and fabsf(z_q - r) <= depth_tol r; background: z_q is background.  The exclusion is a select, so NaN
 *     or garbage in an unusable tap cannot leak.  Sequentially over the usable taps:
 *       ws += w;   s += w (xyz_q / n_q);   sm += w (m2_q / n_q);   sn += w n_q.
 *   History is used iff a history is given, n_c = film[p].w >= 1, there is a projection in range and ws >= 0.25f
 *     (VPT_TEMPORAL_MIN_WEIGHT: one far corner tap is not blown up by the renormalisation).  Then
 *       c_h = s / ws;   s_h = sm / ws;   n_0 = sn / ws;   c_c = xyz / n_c;
 *       v_c = n_c >= 2 ? max(m2 / n_c - c_c.y c_c.y, 0) / (n_c - 1) : c_c.y c_c.y      (the denoiser's prepare)
 *       v_h = max(s_h - c_h.y c_h.y, 0) / max(n_0 - 1, 1);
 *       e   = fabsf(c_c.y - c_h.y) / ((sigma_r sqrtf(v_c + v_h) + rel_floor c_c.y) + 1e-20f);
 *       n_h = min(n_0, max_history) / (1 + e e)                  (a rational rejection, as the denoiser's falloff)
 *     and, iff n_h > 0 (a NaN or a fully rejected history adds nothing):
 *       out.xyz = xyz + n_h c_h;   out.w = n_c + n_h;   out_m2 = m2 + n_h s_h;   hist_n_out = n_h.
 *   Every other pixel -- no current samples, no usable history, every pixel when the history pointers are NULL --
 *   passes through: out_film and out_m2 are the inputs' bytes, copied, and hist_n_out is +0.
 *
 * Kernel: vpt_temporal_kernel, blocks of 64 x 4 pixels, one lane per pixel, so a tap is one 16-byte film load plus
 * the plane's and the depth planes' dwords; no LDS, no atomics, no scratch, fixed trip counts; the level is picked
 * with selects.  Alignment: the three films 16 bytes, every plane 4 bytes.
 *
 * VPT_E_INVALID: a null context, params, film, plane, depth, previous camera, output film or output plane; a history
 * of which only some pointers are given; n_levels outside 1..4; max_history, depth_tol, sigma_r or rel_floor not > 0
 * (NaN included); a misaligned film or plane; a previous camera vpt_gpu_set_shutter would refuse; an output that
 * overlaps an input or another output.  The arguments are checked before the context is.  Out of scope: motion of
 * the medium (volume sequences), light groups, shutter frames, the drop-in vpt_gpu::run and feeds, the multi-GPU
 * modes, neighbourhood colour clamping, history length as a filter parameter of the a-trous pass, accumulated
 * variance as the adaptive stopping rule. */
#define VPT_TEMPORAL_MIN_WEIGHT 0.25f
typedef struct vpt_temporal_params {
  uint32_t n_levels; /* 1..VPT_DEPTH_MAX_LEVELS depth planes per frame, as vpt_gpu_render_depth writes them */
  float max_history; /* > 0: cap of the history's sample count per pixel */
  float depth_tol;   /* > 0: relative depth tolerance of a history tap; default 0.1 */
  float sigma_r;     /* > 0: Y rejection scale in standard deviations; default 4 */
  float rel_floor;   /* > 0: relative floor of that scale (the denoiser's meaning); default 1e-3 */
} vpt_temporal_params;
int vpt_gpu_temporal(vpt_gpu_ctx* ctx, const vpt_temporal_params* p, const float* film_device, const float* m2_device,
                     const float* depth_device /* current frame: [H][W][4], [H][W], [n_levels][H][W] */,
                     const vpt_shutter_camera* prev_cam /* the camera the history was rendered with */,
                     const float* hist_film_device, const float* hist_m2_device,
                     const float* hist_depth_device /* the same shapes; all three NULL: no history */,
                     float* out_film_device, float* out_m2_device /* an ordinary film and moment plane */,
                     float* motion_out_device /* [H][W][2], may be NULL */,
                     float* hist_n_out_device /* [H][W], may be NULL */, void* hip_stream);

/* The drop-in's ordered frame (vpt_run.hpp: vpt_gpu::run's film, bit-identical to the reference's).  A feed's jobs
 * arrive in the provider's order and its film is progressive, so its launch adds samples with fp32 atomics; with a
 * frame open, the context's feed launches also store the samples of the jobs of tiles [tile_lo, tile_hi) in waves
 * jid_lo / T .. + *waves - 1 (from job jid_lo on) in the context's sample buffer (*waves * (tile_hi - tile_lo) *
 * tile_area * 12 bytes, allocated here -- before any feed of the context is open: a running feed's launch holds the
 * device, which an allocation may wait for; VPT_E_STATE otherwise).  *waves: asked for in, granted out -- at most
 * what fits 3/4 of the device's free memory and 128 GiB (VPT_E_NOMEM when not one wave does).  After the feeds are collected,
 * vpt_gpu_frame_finish adds the stored samples of jobs [jid_lo, jid_end) pixel by pixel in wave order -- w += 1,
 * xyz += imaging_ratio * L (worker.cpp:203-204) -- onto `prior` (the host film before the frame, float[H][W][4];
 * NULL = zeros) and writes the frame's tiles' pixels into film_host, replacing what the feeds' collects added
 * there.  Every job of those tiles in [jid_lo, jid_end) must have been rendered by this context's feeds (one taker
 * hands out a contiguous range); jid_end beyond the frame's waves is VPT_E_INVALID (those jobs stored nothing).
 * waves = 0 closes the frame; finish closes it too.  While a frame is open the context's other ordered launches add
 * with atomics (the buffer is the frame's). */
int vpt_gpu_frame_open(vpt_gpu_ctx* ctx, uint64_t jid_lo, uint64_t* waves, uint32_t tile_lo, uint32_t tile_hi);
int vpt_gpu_frame_finish(vpt_gpu_ctx* ctx, uint64_t jid_end, const float* prior, float* film_host);

/* Like vpt_gpu_render_jobs but also writes every sample's radiance L (before the
 * imaging_ratio scale) to records_device[(jid - jid_begin) * tile_w*tile_h + y_local*rect_w + x_local][3]
 * — a debug path for bit-exact per-sample parity. */
int vpt_gpu_render_jobs_records(vpt_gpu_ctx* ctx, uint64_t jid_begin, uint64_t jid_count,
                                float* film_device, float* records_device, void* hip_stream);

/* ---- debug traces ------------------------------------------------------------ */

/* One line of the reference's event log (Logger<true>, src/worker.cpp:16-48 -> log.csv). */
enum {
  VPT_EV_NEW_RAY = 0,            /* v = camera ray origin xyz, direction xyz (worker.cpp:125)    */
  VPT_EV_SAMPLED_POINT = 1,      /* v = collision point xyz (world), density (worker.cpp:145)    */
  VPT_EV_NULL = 2,               /* (worker.cpp:164)                                             */
  VPT_EV_SCATTER_TERMINATED = 3, /* (worker.cpp:168)                                             */
  VPT_EV_SCATTER = 4,            /* v = new ray origin xyz, direction xyz (worker.cpp:180)       */
  VPT_EV_ABSORBED = 5            /* (worker.cpp:185)                                             */
};
typedef struct vpt_event {
  uint64_t jid;    /* job id                                                    */
  uint32_t pixel;  /* pixel within the job's clipped tile rect, y * width + x   */
  uint32_t seq;    /* order of the event within its job                         */
  uint32_t type;   /* VPT_EV_*                                                   */
  float v[7];
} vpt_event;     /* 48 bytes */

/* Render jobs like vpt_gpu_render_jobs and append every Logger event to events_device (capacity
 * entries, unordered across jobs: sort by (jid, seq)).  *count = events produced (may exceed
 * capacity; the excess is dropped).  Synchronous. */
int vpt_gpu_trace_jobs(vpt_gpu_ctx* ctx, uint64_t jid_begin, uint64_t jid_count, float* film_device,
                       vpt_event* events_device, uint64_t capacity, uint64_t* count, void* hip_stream);

/* Volume::log_dda_trace (src/volume.cpp:194-225) for one world ray, on the host: the voxels of
 * NanoVDB's unit DDA from 16 index units before to 16 after the ray's clip to the index bbox, with
 * getValue, getDim, getNodeInfo (dim, maximum) and isActive at each (row = one dda_trace.csv line).
 * *n_rows = voxels walked (rows beyond max_rows are not written), or -1 when the ray misses the
 * index bbox (the reference then writes no file). */
typedef struct vpt_dda_row {
  int32_t ijk[3];
  float t;
  float value;
  uint32_t dim_getdim;
  uint32_t dim_nodeinfo;
  int32_t active;
  float maximum;
} vpt_dda_row;
int vpt_dda_trace(const vpt_grid_desc* density, const float origin[3], const float direction[3], vpt_dda_row* rows,
                  int max_rows, int* n_rows);

/* Volume::log_majorant_trace (src/volume.cpp:176-192) for one world ray: per RayMajorantIterator
 * segment the row X0,Y0,Z0,X1,Y1,Z1,T0,T1,Majorant (index-space end points, world-space t).
 * rows_host: [max_rows][9]; *n_rows = segments (0 if the ray misses the volume).  Synchronous. */
int vpt_gpu_majorant_trace(vpt_gpu_ctx* ctx, const float origin[3], const float direction[3],
                           float* rows_host, int max_rows, int* n_rows);

/* Throughput mode.  VPT_RNG_REFERENCE (default): one pcg32_fast stream per job,
 * hash(seed, jid), a job's pixels traced in order -- the reference's samples.  VPT_RNG_PIXEL: every
 * pixel of a job is its own work item with stream hash(seed, jid * tile_area + pixel); it matches
 * the reference only in expectation and is never used for parity. */
enum { VPT_RNG_REFERENCE = 0, VPT_RNG_PIXEL = 1 };
int vpt_gpu_set_rng_mode(vpt_gpu_ctx* ctx, int mode);
/* Throughput mode's work granularity: pixels of one job per work item (a lane traces them in order, each
 * with its own stream, so the samples do not depend on it).  0 (default): the largest power of two
 * dividing the tile area that leaves >= 32 work items per resident lane; else a power of two dividing
 * the tile area (VPT_E_INVALID otherwise).  Applies from the next render call. */
int vpt_gpu_set_pixel_chunk(vpt_gpu_ctx* ctx, int chunk);

/* Kernel variant of density-only scenes.  The run-skipping variant takes, from an interior cell whose
 * majorant equals the segment's, the next r HDDA steps without loading their cells (r = the cell's
 * precomputed run radius); samples are identical.  mode -1 (default): chosen at creation (on when
 * >= 1/4 of the interior cells have r >= 2, e.g. C2's constant cube); 0: off; 1: on (VPT_E_INVALID
 * with a temperature grid).  Takes effect at the next launch. */
int vpt_gpu_set_run_skipping(vpt_gpu_ctx* ctx, int mode);
/* The production kernel the context launches: temperature grid present, run skipping on. */
int vpt_gpu_kernel_variant(const vpt_gpu_ctx* ctx, int* has_temperature, int* run_skipping);
/* The instantiation the context's last launch ran (host state only: no wait).  *eval_split: 1 when it evaluates
 * densities in two halves around the rare blocks (the density-only production launches of the throughput kernels:
 * plain, run-skipping, feed, band and gang), 0 when whole (temperature, records / events, latency, compacting), -1
 * before the first launch.  Samples never depend on it. */
int vpt_gpu_last_launch_variant(const vpt_gpu_ctx* ctx, int* eval_split);

/* Scheduling order of a whole-wave job range (jid_begin and jid_count multiples of T).  Results
 * never depend on it: every job keeps its jid and RNG stream, only the fp32 atomic film-add order
 * changes.  VPT_ORDER_JID: jid order, as TileProvider::next() hands jobs out.
 * VPT_ORDER_COST_WAVE_MAJOR: wave by wave, each wave's tiles costliest first.
 * VPT_ORDER_COST_TILE_MAJOR: the whole range as one costliest-first list -- tiles ranked by cost in
 * groups of 64, each group's waves consecutively (64 lanes = 64 tiles of one wave).
 * VPT_ORDER_COST_TAIL: wave-major, then the last ~6 x (resident lanes / T) waves
 * tile-major, so the launch drains on cheap (sky) jobs without concentrating the whole launch on
 * the densest tiles.
 * VPT_ORDER_COST_SAME_TILE (default): tile by tile, costliest first, each tile's waves consecutively --
 * the 64 lanes of a wavefront take one tile's jobs of 64 waves, so they trace the same pixels and their
 * rays walk the same cells until they scatter; the range drains on the cheapest tiles.  Launches that
 * add with film atomics (the ordered film off, feeds, debug launches) take VPT_ORDER_COST_TAIL instead
 * (64 lanes would add to one pixel at once), and so do partly filled launches (a few jobs per resident
 * lane: C2, a GPU's share of a frame), where it measured slower.  Costs: vpt_gpu_tile_costs.  Other
 * ranges run in jid order. */
enum {
  VPT_ORDER_JID = 0,
  VPT_ORDER_COST_WAVE_MAJOR = 1,
  VPT_ORDER_COST_TILE_MAJOR = 2,
  VPT_ORDER_COST_TAIL = 3,
  VPT_ORDER_COST_SAME_TILE = 4
};
int vpt_gpu_set_job_order(vpt_gpu_ctx* ctx, int mode);
/* VPT_ORDER_COST_TAIL's tile-major wave count (0 = auto: 6 x resident lanes / T, rounded up); also the
 * fallback of VPT_ORDER_COST_SAME_TILE. */
int vpt_gpu_set_job_order_tail(vpt_gpu_ctx* ctx, int waves);
/* The per-tile cost estimates (float[T], may be NULL) and the tile ranks by descending cost
 * (uint32[T], may be NULL): HDDA steps + 4 x majorant optical depth of 5 primary rays per tile. */
int vpt_gpu_tile_costs(vpt_gpu_ctx* ctx, float* cost_T, uint32_t* rank_T);
/* Replaces the cost estimates with caller-supplied per-tile costs (float[T], e.g. measured job times
 * of an earlier launch) and re-ranks the tiles; waits for all work on the device first. */
int vpt_gpu_set_tile_costs(vpt_gpu_ctx* ctx, const float* cost_T);
/* An explicit job order for launches of exactly n jobs (any jid_begin): work item k renders job
 * jid_begin + perm[k].  perm must be a permutation of 0..n-1; n = 0 clears it.  Samples never depend
 * on the order.  Not used in the pixel RNG mode. */
int vpt_gpu_set_job_permutation(vpt_gpu_ctx* ctx, const uint32_t* perm, uint64_t n);
/* *n: the length of the explicit job permutation in force (0: none -- never set, cleared, or dropped by a scene or
 * volume update). */
int vpt_gpu_job_permutation_info(const vpt_gpu_ctx* ctx, uint64_t* n);

int vpt_gpu_sync(vpt_gpu_ctx* ctx);

/* ---- pipelining and progressive films (the drop-in's drain, include/vpt_run.hpp) ------------ */

/* A HIP stream on the context's device (non-blocking w.r.t. the null stream), for launches that overlap:
 * a launch lasts as long as its longest job (a tile's pixels in one RNG stream), so back-to-back launches
 * on one stream would each pay that drain; launches on two streams fill it with the next one's jobs. */
int vpt_gpu_stream_create(vpt_gpu_ctx* ctx, void** hip_stream);
int vpt_gpu_stream_destroy(vpt_gpu_ctx* ctx, void* hip_stream);
/* Waits for the work enqueued on hip_stream so far. */
int vpt_gpu_stream_sync(vpt_gpu_ctx* ctx, void* hip_stream);
/* Binds the calling thread to the CPUs of the NUMA node the context's device is attached to (intersected
 * with the process's CPU set -- its main thread's, which taskset / numactl restrict -- rather than the
 * calling thread's own, which it inherited from whichever thread created it; *node = that node, or -1 when
 * it is unknown or the intersection is empty, and the thread is left as it was).  A feed's pusher reads and writes the pinned ring, which sits
 * in that node's memory, a slot per job: from the other socket of a 2-socket host every access crosses the
 * socket link (C4 through the drop-in: 174-205 ms per frame with the process on the far node, 119-148 on the
 * GPU's, profiles/archive/r05m_numa.txt).  `node` may be NULL. */
int vpt_gpu_bind_thread_near(vpt_gpu_ctx* ctx, int* node);
/* An extra device film (float[H][W][4], zeroed) of the context's size, e.g. the second buffer of a
 * progressive film; release it with vpt_gpu_film_free before vpt_gpu_destroy. */
int vpt_gpu_film_alloc(vpt_gpu_ctx* ctx, float** film_device);
int vpt_gpu_film_free(vpt_gpu_ctx* ctx, float* film_device);
/* film_host[i] += film_device[i], then film_device = 0 (film_device NULL = the context's own film).
 * Synchronous.  The caller must have waited for every launch that renders into film_device (this call
 * does not know their streams); launches into other films may keep running.  Uses a pinned staging
 * buffer owned by the context. */
int vpt_gpu_film_flush_to_host(vpt_gpu_ctx* ctx, float* film_device, float* film_host_hxwx4);

/* Feeds: one launch of the production kernel that renders job ids pushed by the host while it runs --
 * the drop-in's way of handing the GPU a TileProvider's tokens as they are taken, with a bounded queue and
 * no per-batch launch drain (a launch lasts as long as its longest job; a feed's lanes keep taking pushed
 * jobs instead).  vpt_gpu_feed_open prepares it on hip_stream (a stream of this context,
 * vpt_gpu_stream_create) into film_device (NULL = the context's own film); it is launched once as many jobs
 * are pushed as it has lanes (C3: 458 752), when the window fills, or at close.  `window` (rounded up to a
 * power of two, >= 1024 and >= twice the lanes) bounds the jobs pushed and not yet started:
 * vpt_gpu_feed_push blocks while the window is full (VPT_E_STATE if the launch stops taking jobs for 120 s).  Job ids are any jids (< 2^62), e.g.
 * token.jid(); their samples equal vpt_gpu_render_jobs's.  vpt_gpu_feed_close publishes the end: the
 * launch ends once every pushed job is rendered, then adds their sample counts to the film (asynchronous,
 * on the feed's stream).  vpt_gpu_feed_query: whether a closed feed's work is complete (non-blocking) and
 * the jobs pushed.  vpt_gpu_feed_destroy closes if needed, waits for the feed's work and frees it;
 * VPT_E_STATE if lanes gave up waiting for jobs (a lane waits at most 30 s, so a launch always ends: a
 * feed left open without pushes that long ends by itself).  A feed's launch holds the device's CUs until it
 * is closed -- a second feed opened meanwhile starts as the first one's lanes leave -- so push to a feed
 * only after the feeds opened before it have been closed; and a call that waits for the whole device
 * (hipDeviceSynchronize, and hipFree / hipHostMalloc / hipHostFree may) waits for an open feed's lanes to
 * give up: wait for streams instead.  The context's own calls that wait for its launches (vpt_gpu_sync,
 * vpt_gpu_film_clear, vpt_gpu_film_add_to_host, vpt_gpu_counters, vpt_gpu_profile, vpt_gpu_set_tuning,
 * vpt_gpu_set_full_tuning, vpt_gpu_set_latency_tuning, vpt_gpu_set_rng_mode, vpt_gpu_set_tile_costs,
 * vpt_gpu_set_job_permutation, and vpt_gpu_tile_costs before its first cost pass) return VPT_E_STATE while a
 * feed of the context is launched and not closed, instead of waiting 30 s for its lanes to give up.  A
 * destroyed feed's memory is kept by the context for the next vpt_gpu_feed_open (freed by vpt_gpu_destroy).
 * Feeds use a host-pinned ring (8 bytes per window slot) and run the reference RNG mode. */
typedef struct vpt_gpu_feed vpt_gpu_feed;
int vpt_gpu_feed_open(vpt_gpu_ctx* ctx, float* film_device, void* hip_stream, uint64_t window, vpt_gpu_feed** out);
int vpt_gpu_feed_push(vpt_gpu_feed* feed, const uint64_t* jids, uint64_t n);
int vpt_gpu_feed_close(vpt_gpu_feed* feed);
int vpt_gpu_feed_query(vpt_gpu_feed* feed, int* done, uint64_t* pushed);
int vpt_gpu_feed_destroy(vpt_gpu_feed* feed);
/* Jobs pushed and not yet taken by a lane -- an estimate: the lanes report every 1 024th job they take into
 * 4 words of the pinned block (their posted writes land in any order; the largest counts); before the launch
 * every pushed job counts.  It can read high, never for long while the lanes wait: a wavefront that finds
 * every published job taken stores the job count it saw (again every ~5 ms while it waits), and a count >= the
 * published one reads as 0; hints that have not moved for 10 ms read as 0 too.
 * Cheap: a read of one cache line. */
int vpt_gpu_feed_backlog(vpt_gpu_feed* feed, uint64_t* backlog);
/* Test hook for the backlog estimate's words (tests/test_gpu_integration.py): op 0 reads the "waiting" word into
 * *value, op 1 writes *value into it, op 2 writes *value into every reservation hint (and the host's view of
 * them) -- a stale value landing last, which waiting wavefronts overwrite within ~5 ms (they store the count they
 * see every 2^19 ticks of s_memrealtime) and the estimate ignores after 10 ms without a new hint. */
int vpt_gpu_feed_debug(vpt_gpu_feed* feed, int op, uint64_t* value);
/* A staged feed renders into film_device (NULL = the context's own film), which must be zero, on hip_stream
 * (NULL = a stream of the feed's own), and counts the jobs it completes per tile; its film reaches the host through the copy engines, which run beside a launch
 * that holds every CU (r05), so nothing in its life waits for CUs another feed's launch holds.
 *   vpt_gpu_feed_snapshot -- at any time, also while the launch runs: adds into film_host (film_count
 *     floats, the reference's [H][W][4] layout) what the launch has rendered since the previous snapshot --
 *     the completed jobs' sample counts and the film's radiance as copied (~2 ms for a 1080p film).  A
 *     progressive film (main.cpp:101-132's 5-FPS window): every snapshot's additions telescope to the final
 *     film (to fp32 rounding, see collect).  The caller serialises writers of film_host.
 *   vpt_gpu_feed_collect -- closes if needed, waits for the launch, adds the rest, clears film_device and
 *     frees the feed like destroy.  The sample counts then end exact (whole jobs per tile); the radiance ends
 *     equal to the launch's film within fp32 rounding (each snapshot adds a rounded difference, and several
 *     drivers may share film_host).  An intermediate snapshot's radiance includes samples of jobs still
 *     running while their counts arrive only when each job ends, so a progressive frame reads slightly bright
 *     until its jobs complete.
 * vpt_gpu_feed_prepare allocates a feed's memory (the ring, and with staged != 0 the copy buffers) into the
 * context's pool ahead of the first open, e.g. right after vpt_gpu_create, so that no allocation runs while a
 * launch holds the device. */
int vpt_gpu_feed_open_staged(vpt_gpu_ctx* ctx, float* film_device, void* hip_stream, uint64_t window,
                             vpt_gpu_feed** out);
int vpt_gpu_feed_snapshot(vpt_gpu_feed* feed, float* film_host);
int vpt_gpu_feed_collect(vpt_gpu_feed* feed, float* film_host);
int vpt_gpu_feed_prepare(vpt_gpu_ctx* ctx, uint64_t window, int staged);

/* Zero the context's own film. */
int vpt_gpu_film_clear(vpt_gpu_ctx* ctx);
/* Device pointer of the context's own film (for an RCCL reduce), and its element count H*W*4. */
int vpt_gpu_film_device_ptr(vpt_gpu_ctx* ctx, float** film_device, uint64_t* count);
/* film_host[i] += own film[i] (synchronous), the caller-owned reference-layout film. */
int vpt_gpu_film_add_to_host(vpt_gpu_ctx* ctx, float* film_host_hxwx4);
/* Counters summed over every launch since creation (or the last reset). */
int vpt_gpu_counters(vpt_gpu_ctx* ctx, vpt_counters* out, int reset);
/* Scheduling knobs (results never depend on them): a rare lane state (new job, new pixel, ray
 * setup, NEE completion, film write) runs when >= gate_min lanes of a wavefront wait for it or
 * fewer than gate_idle lanes are walking rays; a tentative collision's density evaluation waits
 * for gate_eval lanes likewise; grid_blocks overrides the persistent grid size; the ray walk
 * repeats in an inner loop while >= gate_walk lanes walk (0: one step per pass).
 * Pass <= 0 (gate_idle, gate_walk < 0) to keep a value; gate_idle 0 is rejected (VPT_E_INVALID): a
 * wavefront with no walking lane must run its waiting blocks.
 * A context keeps three gate sets: the context's (partly filled launches, feeds, debug launches), the
 * full-launch set (production launches of the throughput kernel: full frames such as C3 / C4) and the latency
 * set (vpt_gpu_set_latency_tuning).  vpt_gpu_set_tuning writes the first two. */
int vpt_gpu_set_tuning(vpt_gpu_ctx* ctx, int gate_min, int gate_idle, int grid_blocks, int gate_eval,
                       int gate_walk);
/* The full-launch gate set alone (meaning and "keep" conventions as in vpt_gpu_set_tuning; gate_idle 0 is
 * rejected): launches that run the throughput kernel outside feeds and debug launches read it.  Defaults: the
 * context's gates, with gate_idle 4 for the density kernel (its partly filled launches keep 8).  Results never
 * depend on it. */
int vpt_gpu_set_full_tuning(vpt_gpu_ctx* ctx, int gate_min, int gate_idle, int gate_eval, int gate_walk);
/* A gate set's values (gates[4]: gate_min, gate_idle, gate_eval, gate_walk; NULL to skip) and the set the
 * context's last launch read (*last_launch_set; -1 before the first launch; NULL to skip).  Host state only:
 * no wait. */
enum { VPT_GATES_CONTEXT = 0, VPT_GATES_LATENCY = 1, VPT_GATES_FULL = 2 };
int vpt_gpu_gate_info(const vpt_gpu_ctx* ctx, int set, int* gates, int* last_launch_set);
/* Latency-bound launches: a launch with fewer work items than its grid has lanes (e.g. C1, 4 096
 * jobs) lasts as long as its slowest job.  Such launches spread their items over the grid's
 * wavefronts -- the first wave_lanes lanes of each wavefront take jobs (0 = auto: 1 while items /
 * wavefronts < 3, each lane taking its jobs in sequence, else 1 + floor(items / wavefronts)) -- and run with their own gates (meaning as in vpt_gpu_set_tuning; defaults 1, 65, 1, 1:
 * every block runs as soon as one lane needs it).  Results never depend on them.  Pass < 0 (gate_min,
 * gate_eval: <= 0) to keep a value; gate_idle 0 is rejected. */
int vpt_gpu_set_latency_tuning(vpt_gpu_ctx* ctx, int wave_lanes, int gate_min, int gate_idle, int gate_eval,
                               int gate_walk);
/* The latency kernel: the same state machine with the lane's cold state in VGPRs instead of LDS and a
 * larger register budget (4-5 waves per SIMD instead of 7), for launches that occupy at most that many
 * anyway.  mode -1 (default): latency-bound launches (C1: 20.7-21.2 -> 19.2-19.7 ms) and partly filled ones
 * whose grid rule gives <= its resident blocks per CU (C2: 100-101 -> 95.7-96.6 ms; a GPU's small share of a
 * frame); 0: never; 1: always (tests, A/B).  ungated 0 (default): partly filled launches on it use the
 * context's gates; 1: the latency gates (every block runs for one waiting lane, vpt_gpu_set_latency_tuning;
 * measured slower there: C2 109 ms); -1: keep.  Latency-bound launches always use the latency gates.
 * Samples never depend on it.  Takes effect at the next launch. */
int vpt_gpu_set_latency_kernel(vpt_gpu_ctx* ctx, int mode, int ungated);
/* Live-path compaction (north_star's "ballot/prefix-sum to compact live rays") on the latency kernel's partly
 * filled launches (e.g. C2): every `every` outer iterations a block's four wavefronts meet and, when packing
 * helps, move their paths through LDS so that walking paths fill the first wavefronts (a kernel variant with a
 * 60 KiB LDS exchange: <= 2 blocks per CU; launches with more blocks per CU do not use it).  0 (default): off.
 * Samples never depend on it (counters: `exchanged`).  Takes effect at the next launch. */
int vpt_gpu_set_compaction(vpt_gpu_ctx* ctx, int every);
/* The mode and the latency kernel's resident blocks per CU. */
int vpt_gpu_latency_kernel_info(const vpt_gpu_ctx* ctx, int* mode, int* resident_blocks_per_cu);
/* SIMT-utilisation profile of profiling builds (-DVPT_PROFILE): for each block of the lane state
 * machine, [wave executions, active lanes] as 2*21 uint64 (the last 7: lanes per state at each walk-loop iteration), then the shader cycles the wavefronts
 * spent in each of 10 sections (fetch, pixel, ray, walk-loop control, eval, nee, finish, and the
 * walk's segment / step / draw parts); zeros in normal builds.  n must be >= 2 * 21 + 10. */
int vpt_gpu_profile(vpt_gpu_ctx* ctx, uint64_t* out, int n, int reset);
/* Launch geometry used by the integrator kernel (for reports). */
int vpt_gpu_launch_info(const vpt_gpu_ctx* ctx, int* grid_blocks, int* block_threads);
/* Number of HIP devices (0 without a GPU: VPT_OK, *count = 0). */
int vpt_gpu_device_count(int* count);
/* The drop-in's seed recovery on the GPU: the u32 seeds s (ascending, at most max_seeds written) whose job-0
 * stream -- pcg32_fast seeded with hash(s, 0) (hash.hpp:20-67, random.hpp:93-95) -- starts with the outputs
 * out0, out1; *n_found = how many exist (normally 1).  The reference's RandomNumberGenerator keeps its seed
 * private (random.hpp:86-115), so include/vpt_run.hpp finds it from two draws: all 2^32 candidates in one
 * launch on `device` (a few ms; the same scan took 1-3 s on 8-16 host threads).  Synchronous. */
int vpt_gpu_find_seeds(int device, uint32_t out0, uint32_t out1, uint32_t* seeds, int max_seeds, int* n_found);
/* What vpt_gpu_create and the first cost pass took (ms), n <= 5 of: [0] grid flatten + leaf-majorant fix (host),
 * [1] grid upload, [2] the rest of the context (tables, buffers, occupancy, scene constants), [3] the tile-cost
 * pass (vpt_gpu_tile_costs / the first cost-ordered launch), [4] binding the device (hipSetDevice: the HIP
 * runtime's start when it is the process's first HIP call). */
int vpt_gpu_setup_timings(const vpt_gpu_ctx* ctx, double* ms, int n);

/* ---- synthetic stand-in volumes (the reference's .nvdb files are not available) ---------- */

/* kind 0: constant density 1.0 over index [0,n)^3 (n = 128)
 * kind 1: procedural cloud density over [0,n)^3 (C3, n = 512):
 *         p = (ijk + 0.5)/(n/2) - 1, base = clamp((0.85 - |p|)/0.35, 0, 1),
 *         density = base * (0.5 + 0.5 sin(11px+2) sin(13py+1) sin(17pz+3))  (double, then float)
 * kind 2: temperature 40*base on the same lattice (C4)
 * world = index - n/2; leaves with no non-zero voxel are omitted; non-zero voxels are active;
 * indexBBox = bbox of active voxels; leaf_max = max over active voxels.  NULL on bad arguments.
 * The returned desc owns its arrays: release it with vpt_synth_free. */
vpt_grid_desc* vpt_synth_grid(int kind, int n);
void vpt_synth_free(vpt_grid_desc* desc);

/* Thread-local message for the last non-OK return. */
const char* vpt_last_error(void);
int vpt_abi_version(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* VPT_GPU_H */
