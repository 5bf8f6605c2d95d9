// er_tsdf.h -- what the translation units of path A (er_tsdf.hip, er_tsdf_pre.hip, er_tsdf_int.hip, er_tsdf_extract.hip, er_tsdf_band.hip) know about
// each other: the constants of the volume's tables and of the batch pipeline, the three kernels that live in files of their own, the handle, and
// the few host functions one file calls in another.  Internal: not part of the C ABI (include/er_hip.h).
#pragma once

#include "er_common.h"
#include "er_compact.h"
#include "er_mem.h"
#include "er_tsdf_math.h"

#include "../../include/er_hip.h"

#include <algorithm>
#include <cstdlib>
#include <functional>
#include <utility>
#include <vector>

// Path A's own namespace: er_grid.h (path B) has a kBlock too, in er::.  The kernels declared here are the ones with external linkage: the compiler
// flags that are best for the voxel pass are not the ones that are best for the pre-pass kernels (profiles/r04k_ab_compiler_flags.txt: without the
// SLP vectoriser's packed-math pairs -- which cost k_reproject_scatter 28 register moves per pixel -- and with the max-memory-clause scheduler the job
// gains 4.5 %; k_integrate alone is fastest with the max-ILP scheduler), and hipcc takes such flags per file.  So k_reproject_scatter and k_prepare
// are defined in er_tsdf_pre.hip, k_integrate in er_tsdf_int.hip, and er_tsdf.hip launches them.  Every other kernel sits in an anonymous namespace
// next to its host caller; device helpers have internal linkage and are compiled where they are used (er_tsdf_dev.h).
namespace er_tsdf_k {
using namespace er;

constexpr int kBlock = 256;
constexpr int kEmptyKey = -1;
constexpr uint32_t kZEmpty = 0xFFFFFFFFu;
// A z-buffer cell is (0xFFFF - epoch) << 16 | depth, epoch = the buffer's use counter (1 .. kZEpochMax; the handle advances it once per batch or
// single frame that scatters into the buffer).  A newer use's values compare below everything older uses left behind, so the scatter's atomicMin
// overwrites stale cells, and the consumer takes a cell as empty unless its upper half carries the current tag: nobody re-arms the buffer.  It is
// filled with 0xFF (= epoch 0, which no scatter uses) at create, at er_tsdf_reset and when the counter would wrap.
constexpr uint32_t kZEpochMax = 0xFFFFu;

// counters[] slots
enum { C_NUNITS = 0, C_NBATCH = 1 /* and 6, 7: one per pipeline slot */, C_POOL_OVERFLOW = 2, C_TABLE_FULL = 3, C_OUT_OF_RANGE = 4,
       C_NBATCH1 = 6, C_NBATCH2 = 7, C_ZERO_WRITE = 8 /* 8, 9: frames 0-31 / 32-63 of the batch; 10, 11 for the second pre-pass stream */,
       C_ZERO_WRITE1 = 10, C_COUNT = 12 };
constexpr int kDepth = 3;                // batches in flight: voxel pass of n, pre-passes of n+1 and n+2 (depth 2 with one pre-pass
constexpr int kAux = 2;                  // stream = the round-1 pipeline: profiles/r02n_ab_pipeline_depth_hw_queues.txt); pre-pass streams:
                                         // batch b runs on stream b mod kAux
constexpr int kZColor = kAux;            // index of the colour calls' z-buffer counter in er_tsdf_s::zepoch, behind the kAux pre-pass buffers'

// The unit hash map as a kernel that runs when nobody inserts reads it (the extraction kernels, the ray caster, the colour kernels): passed by
// value, built by er_tsdf_s::view.  slot (er_tsdf_dev.h): the unit's pool slot, -1 = no such unit.
struct UnitMap {
  const int* __restrict__ ht_key;
  const int* __restrict__ ht_slot;
  int cap_mask, shift;
  __device__ int slot(int key) const;
};
// ... and the sdf pool it indexes: what a reader of {sdf, weight} takes.  (The colour kernels index the accumulators, by the same slots: the map alone.)
struct VolumeView {
  const float2* __restrict__ pool;
  UnitMap map;
  __device__ const float2* unit(int slot) const { return pool + (size_t)slot * kUnitVox; }
};

// ------------------------------------------------------------------------------------------------
// Reproject, IntegrateApp.cpp:247-268: every source pixel is warped through its fragment's control
// grid and scattered into the frame's z-buffer.  The reference's sequential "write if empty or
// closer" is an order-independent min for dd != 0; a write of dd == 0 RESETS the cell (0 means
// empty), which is order dependent.  Such a write (a warped depth below 0.5 mm: practically never) records its source index
// in lastzero (max) and raises the FRAME's bit in the stream's flag word; k_reproject_fix then scatters the flagged frames a
// second time into a side buffer, zfix, under the replay rule -- only writes that come after the cell's last zero write
// count -- and the consumer of the z-buffer (k_prepare / k_zbuf_to_depth) takes cells with lastzero > 0 from zfix.
struct ReprojArgs {
  const uint16_t* depth;
  int n_frames, cols, rows;
  Camera cam;
  CameraInv cami;
  const double* seg12;
  const double* madj12;
  const int* grid_index;
  const float* ctr;
  int res;
  float grid_ul;
  int floats_per_grid;
  uint32_t* zbuf;
  uint32_t* lastzero;
  uint32_t* zfix;                        // the replay's z-buffer (all-empty outside a replay; re-armed by the consumer)
  int* zero_flag;                        // int[2], bit f: frame f of the batch saw a write of dd == 0 (one pair per pre-pass stream)
  uint32_t ztag;                         // (0xFFFF - epoch) << 16 of this use of zbuf (next_ztag)
};
__global__ void k_reproject_scatter(ReprojArgs A);

// k_reproject_fix's launch (er_tsdf.hip): kFixBlocks single-wave workgroups
constexpr int kFixThreads = 64;
constexpr int kFixBlocks = 256;

// Frames of the scaled-depth buffer are kScaledPad floats apart beyond their pixels; the pad stays 0.0f for ever (zero-filled at
// create, never written): a voxel whose projection misses the image gathers from it instead of taking a predicated load.
// tile_max / tile_lo / tile_lo_fine are laid out [tile][frame of the batch]: see k_integrate's culling.
constexpr int kScaledPad = 64;
constexpr int kTile = 32;
// Granularity of tile_lo_fine, the second-level per-tile MINIMUM of the scaled depth behind k_integrate's "full" verdict: 2^kLoShift pixels.
// 16-pixel tiles next to the 32-pixel tiles of tile_max / tile_lo: a pixel without usable depth (the warp's scatter leaves holes) spoils the
// minimum of its whole tile.  The fine tiles are the SECOND level of the verdict (er_tsdf_math.h: patch_may_update_box): the 32-pixel minimum
// decides first, the fine ones are read only when it fails for a patch that lies clearly in front of everything under it.
constexpr int kLoShift = 4;
constexpr int kLoSub = kTile >> kLoShift;               // tile_lo tiles per side of a 32 x 32 k_prepare tile: 2
constexpr int kTileKeys = 96;

constexpr int kPrepThreads = 256;                       // 8 column groups x 32 rows of threads, kPrepPix adjacent pixels of one row each
constexpr int kPrepPix = kTile * kTile / kPrepThreads;  // pixels per thread

// kWide: one 16-byte access per array and thread (8-byte for the 16-bit depth) behind one bounds test; needs cols % 4 == 0 and an 8-byte
// aligned depth pointer (run_batch chooses; er_tsdf_pre.hip)
template <bool kWide>
__global__ __launch_bounds__(kPrepThreads) void k_prepare(
    const uint16_t* __restrict__ depth, uint32_t* __restrict__ zbuf, int n_frames, int cols, int rows,
    Camera cam, CameraInv cami, const float* __restrict__ lambda, const double* __restrict__ T12, float* __restrict__ scaled,
    int* __restrict__ ht_key, int* __restrict__ ht_slot, unsigned long long* __restrict__ ht_mask, int cap_mask,
    int hash_shift, int* __restrict__ batch, int* __restrict__ nbatch,
    int* __restrict__ counters, float* __restrict__ tile_max, float* __restrict__ tile_lo, float* __restrict__ tile_lo_fine, int2 shard,
    uint32_t* __restrict__ lastzero, uint32_t* __restrict__ zfix, const int* __restrict__ zero_flag, uint32_t ztag);
extern template __global__ void k_prepare<true>(const uint16_t* __restrict__, uint32_t* __restrict__, int, int, int, Camera, CameraInv, const float* __restrict__, const double* __restrict__, float* __restrict__, int* __restrict__, int* __restrict__, unsigned long long* __restrict__, int, int, int* __restrict__, int* __restrict__, int* __restrict__, float* __restrict__, float* __restrict__, float* __restrict__, int2, uint32_t* __restrict__, uint32_t* __restrict__, const int* __restrict__, uint32_t);
extern template __global__ void k_prepare<false>(const uint16_t* __restrict__, uint32_t* __restrict__, int, int, int, Camera, CameraInv, const float* __restrict__, const double* __restrict__, float* __restrict__, int* __restrict__, int* __restrict__, unsigned long long* __restrict__, int, int, int* __restrict__, int* __restrict__, int* __restrict__, float* __restrict__, float* __restrict__, float* __restrict__, int2, uint32_t* __restrict__, uint32_t* __restrict__, const int* __restrict__, uint32_t);

// k_plan's records and k_integrate's work items
constexpr int kRows = 4;                  // register rows per lane of k_integrate: a wave owns an 8 x 4 x 8 box of voxels (2 x 4 x 8 lanes x 4 rows)
constexpr int kItemsPerUnit = 256;       // work items per unit: 8 x 8 x 16 voxels per 256-thread workgroup

struct Plan {
  int n_units;
  int next;      // work queue of k_integrate: index of the next unclaimed item (reset by k_plan)
};

// What k_integrate needs to know about one unit of the batch, in ONE 16-byte scalar load (round 3; it used to chase plan entry ->
// hash key -> pool slot -> frame mask through four dependent loads per item).
struct PlanRec {
  int key;                  // hash_key of the unit (TSDFVolume.h:62-64)
  int slot;                 // pool slot; < 0: the pool is exhausted (reported by the host), the unit is skipped
  unsigned long long mask;  // frames of the batch that touch the unit
};

constexpr int kIntMinBlocks = 5;                          // register budget handed to the compiler: 5 workgroups of 4 waves per CU = 102 VGPRs (the kernel uses 93 with 3, 4
                                          // or 5; with 6 it spills).  Same instructions, another register assignment: +1.0 % on the job against 4, five
                                          // interleaved runs out of five (profiles/r06v_ab_min_blocks.txt).  The grid launches kIntBlocksPerCu = 3
                                          // workgroups per CU -- the free registers go to the co-running pre-pass kernels

// kSure: the square-root-free "sure" path of the frame loop (er_tsdf_int.hip)
template <bool kSure>
__global__ __launch_bounds__(kBlock, kIntMinBlocks) void k_integrate(
    float2* __restrict__ pool, const PlanRec* __restrict__ plan_rec, Plan* __restrict__ plan,
    const FrameXform* __restrict__ frames, const float* __restrict__ scaled, const float* __restrict__ tile_max,
    const float* __restrict__ tile_lo, const float* __restrict__ tile_lo_fine, int tiles_x, int tiles_y, Camera cam, int cols, int rows);
extern template __global__ void k_integrate<true>(float2* __restrict__, const PlanRec* __restrict__, Plan* __restrict__, const FrameXform* __restrict__, const float* __restrict__, const float* __restrict__, const float* __restrict__, const float* __restrict__, int, int, Camera, int, int);
extern template __global__ void k_integrate<false>(float2* __restrict__, const PlanRec* __restrict__, Plan* __restrict__, const FrameXform* __restrict__, const float* __restrict__, const float* __restrict__, const float* __restrict__, const float* __restrict__, int, int, Camera, int, int);
}  // namespace er_tsdf_k

// The device memory of a handle.  A fresh er_tsdf_mem assigned over it frees all of it, at that point (er_tsdf_destroy: before own_stream goes).
struct er_tsdf_mem {
  er::DevScope fixed;                                   // what er_tsdf_create allocates: the arrays behind the handle's plain pointers
  // colour (er_tsdf_color.hip): per voxel two 64-bit words (r | g << 32), (b | n << 32) = uint32 r_sum, g_sum, b_sum, n; indexed like the pool, by the
  // unit's slot.  Empty until er_tsdf_color_enable: a volume that never enables colour allocates nothing.
  er::Buffer<unsigned long long> color;
  er::Buffer<int> key_scratch, slot_scratch;            // grow together (ensure_key_scratch)
  er::Buffer<float> ctr_dev[2];                         // the caller's lattices by call parity (upload_ctr)
  er::Buffer<char> band_scratch;                        // of the band kernels (owner merge)
  er::Buffer<char> color_scratch;                       // staging of the colour calls' inputs (frames, points), their own so that no pre-pass buffer is shared
};

// (the handle is a type of the C ABI, so it lives in the global namespace)
struct er_tsdf_s : er_tsdf_mem {
  int device = 0, cols = 0, rows = 0, pixels = 0, max_units = 0;
  er::Camera cam{};
  er::CameraInv cami{};
  hipStream_t own_stream = nullptr, stream = nullptr;   // `stream` (the caller's, or own_stream) carries every call but the voxel pass; k_integrate
                                                        // ALWAYS runs on own_stream, joined to `stream` in front of and behind er_tsdf_integrate_frames: the
                                                        // handle's three streams are created back to back and so get hardware queues of their own,
                                                        // a caller's stream may share one with a pre-pass stream (er_tsdf.hip: run_batch)
  hipEvent_t caller_ev = nullptr;                       // `stream` as it stood at the start of the call, for own_stream to wait for
  hipEvent_t voxel_done = nullptr;                      // the last voxel pass of the last call, for `stream` to wait for (join_voxel) ...
  bool voxel_ahead = false;                             // ... which it has not done yet
  hipStream_t aux_stream[er_tsdf_k::kAux] = {};                      // pre-passes (reproject, prepare) of the NEXT TWO batches run here, overlapped
  hipStream_t copy_stream = nullptr;                      // host depth -> depth_stage[slot], overlapped with all of the above; created on
                                                          // first use (HIP multiplexes streams over 4 hardware queues by default, see er_tsdf_create)
  hipEvent_t copy_done[er_tsdf_k::kDepth] = {};
  hipEvent_t consts_done[er_tsdf_k::kDepth] = {};                    // the per-batch constants of slot q have left the pinned block
  int n_cu = 256;
  int shard_rank = 0, shard_world = 1;                    // unit-shard mode (er_tsdf_set_unit_shard)
  // device memory
  float2* pool = nullptr;
  int *ht_key = nullptr, *ht_slot = nullptr, *unit_key = nullptr, *counters = nullptr;
  unsigned long long* stats = nullptr;
  // triple-buffered batch state (three batches in flight: pre-passes of n+1 and n+2 overlap k_integrate of n)
  long batch_no = 0;                                // batch b uses slot b mod kDepth and pre-pass stream b mod kAux
  bool used[er_tsdf_k::kDepth] = {};
  int* batch[er_tsdf_k::kDepth] = {};
  unsigned long long* ht_mask[er_tsdf_k::kDepth] = {};
  float *scaled[er_tsdf_k::kDepth] = {}, *tile_max[er_tsdf_k::kDepth] = {}, *tile_lo[er_tsdf_k::kDepth] = {}, *tile_lo_fine[er_tsdf_k::kDepth] = {};
  er::FrameXform* frames[er_tsdf_k::kDepth] = {};              // = &dstage[q]->fx
  void* dstage[er_tsdf_k::kDepth] = {};                        // device twin of the pinned per-batch constants (struct Staging)
  hipEvent_t pre_done[er_tsdf_k::kDepth] = {}, int_done[er_tsdf_k::kDepth] = {};
  er::PinnedBuffer<char> pinned[er_tsdf_k::kDepth];                  // host staging of the per-batch constants (struct Staging)
  int ht_cap = 0, ht_shift = 0;
  er_tsdf_k::VolumeView view() const { return {pool, {ht_key, ht_slot, ht_cap - 1, ht_shift}}; }   // for the kernels that only read the unit table
  float *lambda = nullptr, *ctr = nullptr;
  // The caller's lattices, double-buffered by call parity on the host (page-locked staging) AND on the device, so that the
  // upload of call c (copy stream) never waits for the pre-passes of call c-1 that still read the other buffer.
  er::PinnedBuffer<float> ctr_pinned[2];                    // (the device side is er_tsdf_mem::ctr_dev)
  hipEvent_t ctr_ev[2] = {nullptr, nullptr};                // upload of the buffer done
  hipEvent_t ctr_rd[2][er_tsdf_k::kAux] = {};                          // last pre-pass reader of the buffer, per pre-pass stream
  bool ctr_rd_set[2] = {false, false};
  int ctr_parity = 0, ctr_cur = 0;
  uint16_t* depth_stage[er_tsdf_k::kDepth] = {};              // host frames of the batch in flight, by pipeline slot
  uint32_t *zbuf[er_tsdf_k::kAux] = {}, *lastzero[er_tsdf_k::kAux] = {}, *zfix[er_tsdf_k::kAux] = {};  // Reproject's z-buffer and replay state, one per pre-pass stream
  uint32_t zepoch[er_tsdf_k::kAux + 1] = {};              // use counters of zbuf[0], zbuf[1] and of the colour calls' z-buffer (kZColor); next_ztag advances them
  double *T12 = nullptr, *seg12 = nullptr, *madj12 = nullptr, *dsum = nullptr;
  int* grid_index = nullptr;
  er_tsdf_k::PlanRec* plan_rec[er_tsdf_k::kDepth] = {};
  er_tsdf_k::Plan* plan[er_tsdf_k::kDepth] = {};
  // profiling
  int prof_stride = 0;                              // 0 = off, n = time every n-th k_integrate launch
  long prof_tick = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  double ms_total = 0.0;
  long launches = 0, frames_done = 0;
  // timeline of the batch pipeline (er_tsdf_set_timeline): while off, run_batch creates and records nothing
  struct TimelineRow {
    long batch;
    int slot, stream, frames;
    double host_ms[3];                              // against tl_host0
    hipEvent_t ev[7];                               // X: behind the int_done wait, the constants copy, k_reproject_fix, k_prepare, k_plan; V: round k_integrate
  };
  bool tl_on = false;
  hipEvent_t tl_base = nullptr;                     // recorded (and waited for) when the hook is switched on; tl_host0 is the host's clock just behind it
  double tl_host0 = 0.0;
  std::vector<TimelineRow> tl_rows;
  std::vector<hipEvent_t> tl_free;                  // timing events of rows already read, for the next rows
  // round 6 (owner merge): units this GPU handed to their owner -- zeroed, still in the table, hidden from every key / count / extraction query until
  // the next frame is integrated or the unit is imported again
  std::vector<int> dropped;                         // sorted
};

// ---- er_tsdf.hip: host functions the other files call (hidden: not part of the library's interface) ----
namespace er_tsdf_k {
// Waits for h->stream; fails if the unit pool or the hash table has overflowed.
__attribute__((visibility("hidden"))) int check_flags(er_tsdf_t h);
// keys (host) -> slots (device, h->slot_scratch) on h->stream, optionally allocating missing units.
__attribute__((visibility("hidden"))) int resolve_slots(er_tsdf_t h, const int* keys_host, int n, bool allocate);
// The units this GPU holds (without the ones handed to their owner), in ascending key order: keys and pool slots.  Calls check_flags.
__attribute__((visibility("hidden"))) int sorted_units(er_tsdf_t h, std::vector<int>& keys, std::vector<int>& slots);
// Advances the use counter `which` of the z-buffer zbuf (cells uint32) for one more scatter on stream X -- behind a fill with 0xFF on X when the
// counter would wrap -- and returns the tag of this use in *ztag (ReprojArgs::ztag, k_prepare, k_zbuf_to_depth).
__attribute__((visibility("hidden"))) int next_ztag(er_tsdf_t h, int which, uint32_t* zbuf, size_t cells, hipStream_t X, uint32_t* ztag);
// One frame (RA.n_frames == 1) reprojected on stream X into RA.zbuf and on into z_dev, 16-bit depth; lastzero, zfix and the flag words are
// left as they were found (all-empty / 0), zbuf holds stale cells of RA.ztag's epoch.
__attribute__((visibility("hidden"))) int reproject_single(er_tsdf_t h, const ReprojArgs& RA, uint16_t* z_dev, hipStream_t X);
// ---- er_tsdf_extract.hip, for er_mesh_cc.hip ----
// The indexed mesh of er_tsdf_extract_mesh_indexed in device memory: nv float4 vertices, nv float4 normals, ntri x 3 int32 indices (each NULL
// when it was not asked for or the mesh is empty).  `owned` is every device allocation of the call, the three arrays included; the kernels that
// fill them may still be in flight on the handle's stream when mesh_indexed_on_device returns, hipFree waits for them.
struct DeviceMesh {
  long nv = 0, ntri = 0;
  float4 *d_verts = nullptr, *d_nrm = nullptr;
  int* d_tri = nullptr;
  TwoPass lists;                           // the triangle and the vertex slabs between their passes (er_compact.h); outlives `owned`
  DevScope owned;
};
// Lists the units (*n_vertices = *n_triangles = 0 from then on), counts the mesh of the resident volume, sets the two counts, calls
// counted(nv, ntri) -- which refuses what the caller has to refuse, reporting it (non-zero ends the call with 1) -- and then enqueues on
// h->stream the kernels that write the arrays asked for (normals need want_v).  An empty volume returns 0 without calling counted.
// Failures are reported under `who`.
__attribute__((visibility("hidden"))) int mesh_indexed_on_device(er_tsdf_t h, const char* who, bool want_v, bool want_n, bool want_t,
                                                                 long* n_vertices, long* n_triangles, const std::function<int(long, long)>& counted,
                                                                 DeviceMesh* m);
// ---- er_tsdf_color.hip ----
// Zeroes the colour accumulators of the n units whose slots stand in h->slot_scratch (behind resolve_slots, on h->stream); nothing without colour.
__attribute__((visibility("hidden"))) int color_zero_slots(er_tsdf_t h, int n);
}  // namespace er_tsdf_k
