// er_tsdf_pre.hip -- path A's pre-pass kernels, k_reproject_scatter and k_prepare: a file of their own so that they can have compiler flags of
// their own (Makefile: FLAGS_er_tsdf_pre.hip; er_tsdf.h says why).  er_tsdf.hip launches them (run_batch, launch_reproject).
#include "er_tsdf_dev.h"

namespace er_tsdf_k {

// Reproject's scatter (the order-dependent case and its replay: see ReprojArgs in er_tsdf.h).
__global__ void k_reproject_scatter(ReprojArgs A) {
  // 64 x 4 pixel tiles per 256-thread workgroup, frame = blockIdx.z: no integer divisions for the indices.
  const int f = blockIdx.z;
  const int u = blockIdx.x * 64 + (threadIdx.x & 63);
  const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (u >= A.cols || v >= A.rows) return;
  reproject_scatter_px(A, f, u, v, 0);
}

namespace {

// Marks frame f in the unit's mask; the first toucher of the unit IN THIS BATCH (unique: its atomicOr
// returned 0) appends the unit to the batch list.  The pool slot of a unit that is new to the volume is handed out
// by k_plan (unit_slot_acquire in er_tsdf.hip), on the same pre-pass stream.
//
// Unit-shard mode (the bit-exact multi-GPU alternative): with shard.y > 1 GPUs every GPU runs the pre-pass of
// ALL frames but only owns -- allocates, integrates, reports -- the units with unit_owner(key) == shard.x.  Units are
// disjoint (TSDFVolume.cpp:45-63) and each one still sees every frame in order, so the union over the GPUs equals the
// single-GPU volume bit for bit; no collective touches the volume.
__device__ void touch_unit(int key, int f, int* __restrict__ ht_key, int* __restrict__ ht_slot,
                           unsigned long long* __restrict__ ht_mask, int cap_mask, int hash_shift,
                           int* __restrict__ batch, int* __restrict__ nbatch, int* __restrict__ counters, int2 shard) {
  if (shard.y > 1 && unit_owner(key, shard.y) != shard.x) return;
  const int e = ht_find_or_insert(ht_key, cap_mask, hash_shift, key);
  if (e < 0) {
    atomicOr(&counters[C_TABLE_FULL], 1);
    return;
  }
  const unsigned long long bit = 1ull << f;
  const unsigned long long seen = __hip_atomic_load(&ht_mask[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (seen & bit) return;                                               // touched_unit.find, TSDFVolume.cpp:53
  const unsigned long long old = atomicOr(&ht_mask[e], bit);
  if (old != 0ull) return;
  batch[atomicAdd(nbatch, 1)] = e;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Per pixel of every frame of the batch: ScaleDepth (TSDFVolume.cpp:19-36) and the unit-touch half
// of TSDFVolume::Integrate (TSDFVolume.cpp:45-58).
//
// One 1024-thread workgroup owns a 32x32 pixel TILE of one frame (a 64^3 unit projects to >100x100
// pixels at room scale, so a tile nearly always sees 1-3 units).  Lanes whose key differs from their
// left neighbour's append it to a small LDS list; after the barrier the list is de-duplicated and only
// the DISTINCT keys of the tile go to the global hash map.  Without this every wave hammered the same
// few hash entries with device-scope atomics at the same moment (measured: 90 % of wave time waiting).
__global__ __launch_bounds__(kPrepThreads) void k_prepare(
    const uint16_t* __restrict__ depth, uint32_t* __restrict__ zbuf, int n_frames, int cols, int rows,
    Camera cam, CameraInv cami, const float* __restrict__ lambda, const double* __restrict__ T12, float* __restrict__ scaled,
    int* __restrict__ ht_key, int* __restrict__ ht_slot, unsigned long long* __restrict__ ht_mask, int cap_mask,
    int hash_shift, int* __restrict__ batch, int* __restrict__ nbatch,
    int* __restrict__ counters, float* __restrict__ tile_max, float* __restrict__ tile_lo, float* __restrict__ tile_lo_fine, int2 shard,
    uint32_t* __restrict__ lastzero, uint32_t* __restrict__ zfix, const int* __restrict__ zero_flag) {
  __shared__ int s_keys[kTileKeys];
  __shared__ int s_n;
  __shared__ float s_wmax[kPrepThreads / 64], s_wlo[kLoSub][kLoSub][kPrepThreads / 64];
  const int pixels = cols * rows;
  const int f = blockIdx.z;
  const bool replayed = zbuf && ((zero_flag[f >> 5] >> (f & 31)) & 1);  // this frame saw a zero write (uniform; practically never)
  const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x >> 5;      // ty in [0, 8)
  const int x = blockIdx.x * kTile + tx;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  // Each thread owns 4 pixels of its column (rows ty, ty+8, ty+16, ty+24 of the tile): the four loads are
  // issued together, which is what hides the HBM/L2 latency here (the kernel is latency-, not VALU-bound).
  uint16_t d[kPrepPix];
  float lam[kPrepPix];
#pragma unroll
  for (int q = 0; q < kPrepPix; q++) {
    const int y = blockIdx.y * kTile + ty + q * (kTile / kPrepPix);
    d[q] = 0;
    lam[q] = 0.0f;
    if (x < cols && y < rows) {
      const int p = y * cols + x;
      const size_t o = (size_t)f * pixels + p;
      if (zbuf) {
        uint32_t z = zbuf[o];
        zbuf[o] = kZEmpty;                                              // re-arm the z-buffer for the next batch
        if (replayed) z = take_z(z, o, lastzero, zfix);
        d[q] = (z == kZEmpty) ? (uint16_t)0 : (uint16_t)z;
      } else {
        d[q] = depth[o];
      }
      lam[q] = lambda[p];
    }
  }
  float wmax = 0.0f, vlo[kPrepPix];
#pragma unroll
  for (int q = 0; q < kPrepPix; q++) vlo[q] = 3.0e38f;
#pragma unroll
  for (int q = 0; q < kPrepPix; q++) {
    const int y = blockIdx.y * kTile + ty + q * (kTile / kPrepPix);
    int key = -1;
    if (x < cols && y < rows) {
      const float sc = scale_depth_px(d[q], lam[q], cam.integration_trunc);
      scaled[(size_t)f * (pixels + kScaledPad) + y * cols + x] = sc;
      wmax = fmaxf(wmax, sc);
      vlo[q] = sc > 0.001f ? sc : 0.0f;                                 // (min over EVERY pixel of its tile below: 0 as soon as one carries no usable depth
                                                                        // (a NaN depth -- degenerate camera -- fails ":82 dp > 0.001" too: it counts as 0, fminf alone would skip it)
      if (d[q] > 0) {                                                   // TSDFVolume.cpp:47 (no range cut-off)
        key = touch_key(x, y, d[q], cam, cami, T12 + f * 12);
        if (key < 0) atomicAdd(&counters[C_OUT_OF_RANGE], 1);
      }
    }
    const int left = __shfl_up(key, 1);
    const bool leader = key >= 0 && (tx == 0 || left != key);
    if (leader) {
      const int slot = atomicAdd(&s_n, 1);
      if (slot < kTileKeys) {
        s_keys[slot] = key;
      } else {                                                          // list full (pathological tile): go direct
        touch_unit(key, f, ht_key, ht_slot, ht_mask, cap_mask, hash_shift, batch, nbatch, counters, shard);
      }
    }
  }
  // max of the scaled depth over the 32 x 32 tile and min over its kLoSub x kLoSub sub-tiles of 2^kLoShift pixels (consumed by
  // patch_may_update_box in k_integrate: culling / the full verdict).  A thread's pixel q lies in row 8 q + ty of the tile, column tx: the
  // sub-tile row is (8 q + ty) >> kLoShift, the column tx >> kLoShift; a wave holds rows ty = 2 w, 2 w + 1 (lane = 32 (ty & 1) + tx).
  for (int off = 32; off > 0; off >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, off));
  if ((threadIdx.x & 63) == 0) s_wmax[threadIdx.x >> 6] = wmax;
  {
    constexpr int qper = kPrepPix / kLoSub;             // pixel rows q of a thread per sub-tile row: 1, 2 or 4
#pragma unroll
    for (int sr = 0; sr < kLoSub; sr++) {
      float r = vlo[sr * qper];
#pragma unroll
      for (int e = 1; e < qper; e++) r = fminf(r, vlo[sr * qper + e]);
#pragma unroll
      for (int off = 1; off < (1 << kLoShift); off <<= 1) r = fminf(r, __shfl_xor(r, off));     // the columns of the sub-tile
      r = fminf(r, __shfl_xor(r, 32));                                                        // the wave's two rows
      if ((threadIdx.x & 32) == 0 && (tx & ((1 << kLoShift) - 1)) == 0) s_wlo[sr][tx >> kLoShift][threadIdx.x >> 6] = r;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = 0.0f, lo = 3.0e38f;
    for (int w = 0; w < kPrepThreads / 64; w++) m = fmaxf(m, s_wmax[w]);
    for (int e = 0; e < kLoSub * kLoSub * (kPrepThreads / 64); e++) lo = fminf(lo, (&s_wlo[0][0][0])[e]);
    const size_t t = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ER_MAX_BATCH + f;      // [tile][frame]: see k_integrate's culling
    tile_max[t] = m;
    tile_lo[t] = lo;                                      // the 32-pixel minimum: first level of the full verdict
  }
  if ((int)threadIdx.x < kLoSub * kLoSub) {
    const int sr = threadIdx.x / kLoSub, sg = threadIdx.x % kLoSub;
    float lo = 3.0e38f;
    for (int w = 0; w < kPrepThreads / 64; w++) lo = fminf(lo, s_wlo[sr][sg][w]);
    const int lx = blockIdx.x * kLoSub + sg, ly = blockIdx.y * kLoSub + sr;
    const int lo_tx = (cols + (1 << kLoShift) - 1) >> kLoShift, lo_ty = (rows + (1 << kLoShift) - 1) >> kLoShift;
    if (lx < lo_tx && ly < lo_ty) tile_lo_fine[((size_t)ly * lo_tx + lx) * ER_MAX_BATCH + f] = lo;
  }
  const int n = min(s_n, kTileKeys);
  if ((int)threadIdx.x < n) {
    const int k = s_keys[threadIdx.x];
    bool dup = false;
    for (int j = 0; j < (int)threadIdx.x; j++) dup = dup || (s_keys[j] == k);
    if (!dup) touch_unit(k, f, ht_key, ht_slot, ht_mask, cap_mask, hash_shift, batch, nbatch, counters, shard);
  }
}

}  // namespace er_tsdf_k
