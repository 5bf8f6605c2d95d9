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
// Cross-lane moves of k_prepare's reductions: DPP inside a 16-lane row, the half-exchanging permlane swaps between rows.  No LDS, no
// wait.  All of them are called with the whole wave active (outside every divergent branch): a DPP read of an inactive lane keeps `old`.
namespace {

template <int kCtrl>
__device__ __forceinline__ int dpp_mov(int v) {
  return __builtin_amdgcn_update_dpp(v, v, kCtrl, 0xF, 0xF, false);
}
constexpr int kDppQuadXor1 = 0xB1;       // quad_perm:[1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;       // quad_perm:[2,3,0,1]
constexpr int kDppRowShr1 = 0x111;       // row_shr:1: lane i takes lane i - 1 of its row (lane 0 of a row keeps its own value)
constexpr int kDppRowRor4 = 0x124;       // row_ror:4 / 8: lane i takes lane (i - n) mod 16 of its row
constexpr int kDppRowRor8 = 0x128;

template <int kCtrl>
__device__ __forceinline__ float dpp_movf(float v) {
  return __int_as_float(dpp_mov<kCtrl>(__float_as_int(v)));
}

struct FMin { __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); } };
struct FMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

// v_permlane16_swap a, b exchanges the odd rows of a with the even rows of b, v_permlane32_swap the upper half of a with the lower half of b:
// with a = b = v the two results hold, in every lane, this lane's value and the one 16 (32) lanes away.
template <class Op>
__device__ __forceinline__ float across_rows(float v, Op op) {
  const unsigned u = (unsigned)__float_as_int(v);
  const auto s16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = op(__int_as_float((int)s16[0]), __int_as_float((int)s16[1]));
  const unsigned w = (unsigned)__float_as_int(v);
  const auto s32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return op(__int_as_float((int)s32[0]), __int_as_float((int)s32[1]));
}

// Over the lanes that agree with this one in bit 2 (= the column half of the tile): the quad, then lanes + 8, + 16, + 32.
template <class Op>
__device__ __forceinline__ float reduce_half_columns(float v, Op op) {
  v = op(v, dpp_movf<kDppQuadXor1>(v));
  v = op(v, dpp_movf<kDppQuadXor2>(v));
  v = op(v, dpp_movf<kDppRowRor8>(v));
  return across_rows(v, op);
}

// Over the whole wave: the same ladder with the + 4 step (after the quad steps every lane of a quad holds the quad's value, so two rotations
// by 4 and 8 lanes cover the four quads of a row).
template <class Op>
__device__ __forceinline__ float reduce_wave(float v, Op op) {
  v = op(v, dpp_movf<kDppQuadXor1>(v));
  v = op(v, dpp_movf<kDppQuadXor2>(v));
  v = op(v, dpp_movf<kDppRowRor4>(v));
  v = op(v, dpp_movf<kDppRowRor8>(v));
  return across_rows(v, op);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Per pixel of every frame of the batch: ScaleDepth (TSDFVolume.cpp:19-36) and the unit-touch half
// of TSDFVolume::Integrate (TSDFVolume.cpp:45-58).
//
// One 256-thread workgroup owns a 32x32 pixel TILE of one frame (a 64^3 unit projects to >100x100
// pixels at room scale, so a tile nearly always sees 1-3 units).  Pixels whose key differs from their
// left neighbour's append it to a small LDS list; after the barrier the list is de-duplicated and only
// the DISTINCT keys of the tile go to the global hash map.  Without this every wave hammered the same
// few hash entries with device-scope atomics at the same moment (measured: 90 % of wave time waiting).
//
// Thread t owns the kPrepPix = 4 ADJACENT pixels x0 .. x0 + 3 of one row: column group c = t & 7 (x0 = 32 bx + 4 c), row r = t >> 3.  A wave
// is 8 rows x 32 columns, a 16-lane DPP row two pixel rows, a quad the four threads of one 16-pixel sub-tile column.  So three of a
// thread's four left neighbours are its own registers and the fourth is one DPP move away; the tile maximum and the sub-tile minima are
// short DPP / permlane-swap ladders (above); and in the kWide instantiation (the host picks it when cols % 4 == 0 and the depth pointer is
// 8-byte aligned: every frame base is then a multiple of four elements, and a thread's pixels are all inside the image or all outside) each
// array is reached by ONE 16-byte (depth: 8-byte) access behind ONE bounds test.  The narrow instantiation has the same layout with
// per-pixel accesses and tests.
static_assert(kTile == 32 && kPrepPix == 4 && kPrepThreads == 256, "k_prepare: 8 column groups x 32 rows of 4 pixels; a wave is 8 rows of the tile");
static_assert(kLoShift == 4 && kLoSub == 2, "k_prepare: a sub-tile is 4 threads (one quad) wide and 2 waves high; lane bit 2 is its column");
constexpr int kPrepCols = kTile / kPrepPix;                               // column groups of a tile: 8
constexpr int kPrepWaveRows = 64 / kPrepCols;                             // pixel rows of a wave: 8
constexpr int kPrepSubWaves = (1 << kLoShift) / kPrepWaveRows;            // waves per sub-tile row: 2

template <bool kWide>
__global__ __launch_bounds__(kPrepThreads) void k_prepare(
    const uint16_t* __restrict__ depth, uint32_t* __restrict__ zbuf, int n_frames, int cols, int rows,
    Camera cam, CameraInv cami, const float* __restrict__ lambda, const double* __restrict__ T12, float* __restrict__ scaled,
    int* __restrict__ ht_key, int* __restrict__ ht_slot, unsigned long long* __restrict__ ht_mask, int cap_mask,
    int hash_shift, int* __restrict__ batch, int* __restrict__ nbatch,
    int* __restrict__ counters, float* __restrict__ tile_max, float* __restrict__ tile_lo, float* __restrict__ tile_lo_fine, int2 shard,
    uint32_t* __restrict__ lastzero, uint32_t* __restrict__ zfix, const int* __restrict__ zero_flag, uint32_t ztag) {
  __shared__ int s_keys[kTileKeys];
  __shared__ int s_n;
  __shared__ float s_wmax[kPrepThreads / 64], s_wlo[kLoSub][kLoSub][kPrepSubWaves];
  const int pixels = cols * rows;
  const int f = blockIdx.z;
  const bool replayed = zbuf && ((zero_flag[f >> 5] >> (f & 31)) & 1);  // this frame saw a zero write (uniform; practically never)
  const int c = threadIdx.x & (kPrepCols - 1), r = threadIdx.x / kPrepCols;   // r in [0, 32)
  const int x0 = blockIdx.x * kTile + c * kPrepPix, y = blockIdx.y * kTile + r;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int p = y * cols + x0;
  const size_t o = (size_t)f * pixels + p;
  float* __restrict__ const sc_out = scaled + ((size_t)f * (pixels + kScaledPad) + p);
  // the loads of the four pixels are issued together, in front of the arithmetic: that is what hides the HBM / L2 latency here
  uint16_t d[kPrepPix];
  float lam[kPrepPix];
  bool in[kPrepPix];
#pragma unroll
  for (int j = 0; j < kPrepPix; j++) {
    d[j] = 0;
    lam[j] = 0.0f;
    in[j] = y < rows && x0 + (kWide ? 0 : j) < cols;
  }
  if constexpr (kWide) {
    if (in[0]) {
      if (zbuf) {
        const uint4 zv = *reinterpret_cast<const uint4*>(zbuf + o);      // (read only: the next batch's epoch makes these cells empty)
        uint32_t z[kPrepPix] = {z_of_epoch(zv.x, ztag), z_of_epoch(zv.y, ztag), z_of_epoch(zv.z, ztag), z_of_epoch(zv.w, ztag)};
        if (replayed) {
#pragma unroll
          for (int j = 0; j < kPrepPix; j++) z[j] = take_z(z[j], o + j, lastzero, zfix);
        }
#pragma unroll
        for (int j = 0; j < kPrepPix; j++) d[j] = (z[j] == kZEmpty) ? (uint16_t)0 : (uint16_t)z[j];
      } else {
        uint2 dv;
        __builtin_memcpy(&dv, __builtin_assume_aligned(depth + o, 8), 8);
        d[0] = (uint16_t)dv.x;
        d[1] = (uint16_t)(dv.x >> 16);
        d[2] = (uint16_t)dv.y;
        d[3] = (uint16_t)(dv.y >> 16);
      }
      const float4 lv = *reinterpret_cast<const float4*>(lambda + p);
      lam[0] = lv.x;
      lam[1] = lv.y;
      lam[2] = lv.z;
      lam[3] = lv.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPrepPix; j++) {
      if (in[j]) {
        if (zbuf) {
          uint32_t z = z_of_epoch(zbuf[o + j], ztag);
          if (replayed) z = take_z(z, o + j, lastzero, zfix);
          d[j] = (z == kZEmpty) ? (uint16_t)0 : (uint16_t)z;
        } else {
          d[j] = depth[o + j];
        }
        lam[j] = lambda[p + j];
      }
    }
  }
  float wmax = 0.0f, vlo = 3.0e38f, sc[kPrepPix];
  int key[kPrepPix];
#pragma unroll
  for (int j = 0; j < kPrepPix; j++) {
    key[j] = -1;
    sc[j] = 0.0f;
    if (in[j]) {
      sc[j] = scale_depth_px(d[j], lam[j], cam.integration_trunc);
      if constexpr (!kWide) sc_out[j] = sc[j];
      wmax = fmaxf(wmax, sc[j]);
      vlo = fminf(vlo, sc[j] > 0.001f ? sc[j] : 0.0f);                  // (min over EVERY pixel of its tile below: 0 as soon as one carries no usable depth
                                                                        // (a NaN depth -- degenerate camera -- fails ":82 dp > 0.001" too: it counts as 0, fminf alone would skip it)
      if (d[j] > 0) {                                                   // TSDFVolume.cpp:47 (no range cut-off)
        key[j] = touch_key(x0 + j, y, d[j], cam, cami, T12 + f * 12);
        if (key[j] < 0) atomicAdd(&counters[C_OUT_OF_RANGE], 1);
      }
    }
  }
  if constexpr (kWide) {
    if (in[0]) *reinterpret_cast<float4*>(sc_out) = make_float4(sc[0], sc[1], sc[2], sc[3]);
  }
  // key leaders: pixels 1..3 against the thread's own previous pixel, pixel 0 against the left thread's pixel 3 (column group 0 has none)
  const int left = dpp_mov<kDppRowShr1>(key[kPrepPix - 1]);
#pragma unroll
  for (int j = 0; j < kPrepPix; j++) {
    const bool leader = key[j] >= 0 && (j == 0 ? (c == 0 || left != key[0]) : key[j - 1] != key[j]);
    if (leader) {
      const int slot = atomicAdd(&s_n, 1);
      if (slot < kTileKeys) {
        s_keys[slot] = key[j];
      } else {                                                          // list full (pathological tile): go direct
        touch_unit(key[j], f, ht_key, ht_slot, ht_mask, cap_mask, hash_shift, batch, nbatch, counters, shard);
      }
    }
  }
  // max of the scaled depth over the 32 x 32 tile and min over its kLoSub x kLoSub sub-tiles of 2^kLoShift pixels (consumed by
  // patch_may_update_box in k_integrate: culling / the full verdict).  A wave's eight rows lie in ONE sub-tile row, r >> kLoShift; the
  // sub-tile column of a lane is bit 2 of its number (c >> 2).
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wmax = reduce_wave(wmax, FMax());
  vlo = reduce_half_columns(vlo, FMin());
  if (lane == 0) s_wmax[wave] = wmax;
  if ((lane & ~4) == 0) s_wlo[wave / kPrepSubWaves][lane >> 2][wave % kPrepSubWaves] = vlo;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = 0.0f, lo = 3.0e38f;
    for (int w = 0; w < kPrepThreads / 64; w++) m = fmaxf(m, s_wmax[w]);
    for (int e = 0; e < kLoSub * kLoSub * kPrepSubWaves; e++) lo = fminf(lo, (&s_wlo[0][0][0])[e]);
    const size_t t = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ER_MAX_BATCH + f;      // [tile][frame]: see k_integrate's culling
    tile_max[t] = m;
    tile_lo[t] = lo;                                      // the 32-pixel minimum: first level of the full verdict
  }
  if ((int)threadIdx.x < kLoSub * kLoSub) {
    const int sr = threadIdx.x / kLoSub, sg = threadIdx.x % kLoSub;
    float lo = 3.0e38f;
    for (int w = 0; w < kPrepSubWaves; w++) lo = fminf(lo, s_wlo[sr][sg][w]);
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

#define ER_PREPARE_INST(W) \
  template __global__ void k_prepare<W>(const uint16_t* __restrict__, uint32_t* __restrict__, int, int, int, Camera, CameraInv, const float* __restrict__, \
                                        const double* __restrict__, float* __restrict__, int* __restrict__, int* __restrict__,                             \
                                        unsigned long long* __restrict__, int, int, int* __restrict__, int* __restrict__, int* __restrict__,               \
                                        float* __restrict__, float* __restrict__, float* __restrict__, int2, uint32_t* __restrict__,                       \
                                        uint32_t* __restrict__, const int* __restrict__, uint32_t);
ER_PREPARE_INST(true)
ER_PREPARE_INST(false)
#undef ER_PREPARE_INST

}  // namespace er_tsdf_k
