// er_tsdf_dev.h -- the __device__ helpers of path A that kernels in more than one file use: the writers' side of the unit hash map (er_tsdf.hip,
// er_tsdf_pre.hip), the readers' side -- UnitMap::slot and the arithmetic of the voxel lattice (er_tsdf_extract.hip, er_tsdf_raycast.hip,
// er_tsdf_color.hip) -- and the two halves of Reproject's scatter with its replay (er_tsdf.hip, er_tsdf_pre.hip).  Internal
// linkage: each is compiled where it is used.  A helper with one user sits next to that user.
#pragma once

#include "er_tsdf.h"

namespace er_tsdf_k {

// The voxel lattice as a reader addresses it: 512 units of 64 voxels per axis, g = 0-based voxel index on the whole lattice (metres / kUnitLength
// + 256 * 64).  Host and device: er_tsdf_import_world packs keys too.
constexpr int kLatticeVox = 512 * 64;
__host__ __device__ __forceinline__ bool on_lattice(int gx, int gy, int gz) {
  return (unsigned)gx < (unsigned)kLatticeVox && (unsigned)gy < (unsigned)kLatticeVox && (unsigned)gz < (unsigned)kLatticeVox;
}
// the hash_key (TSDFVolume.h:62-64) of the unit that holds voxel g, and the voxel's offset inside that unit
__host__ __device__ __forceinline__ int unit_key_of(int gx, int gy, int gz) { return (gx >> 6) << 18 | (gy >> 6) << 9 | (gz >> 6); }
__host__ __device__ __forceinline__ size_t unit_offset_of(int gx, int gy, int gz) {
  return (size_t)(gx & 63) * 4096 + (size_t)(gy & 63) * 64 + (size_t)(gz & 63);
}
// float32 position of voxel a (0 .. 64: one past the end is voxel 0 of the next unit) of unit coordinate u along one axis
__host__ __device__ __forceinline__ float lattice_pos(int a, int u) { return (float)((double)(a + (u - 256) * 64) * kUnitLength); }

namespace {

__device__ __forceinline__ unsigned hash_unit_key(int key, int shift) { return ((unsigned)key * 2654435761u) >> shift; }

// Lock-free find-or-insert.  The entry index is stable, so callers never wait for anybody.
__device__ int ht_find_or_insert(int* __restrict__ ht_key, int cap_mask, int shift, int key) {
  unsigned h = hash_unit_key(key, shift);
  for (int probe = 0; probe <= cap_mask; ++probe) {
    int e = (int)((h + (unsigned)probe) & (unsigned)cap_mask);
    int k = __hip_atomic_load(&ht_key[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == key) return e;
    if (k == kEmptyKey) {
      int old = atomicCAS(&ht_key[e], kEmptyKey, key);
      if (old == kEmptyKey || old == key) return e;
    }
  }
  return -1;
}

}  // namespace

// Read-only lookup for kernels that run when nobody inserts (er_tsdf.h: UnitMap): the unit's pool slot, -1 = no such unit.  What "no unit" means
// beyond that is the caller's: the extraction kernels test slot < 0, the ray caster and the colour kernels (unsigned)slot >= (unsigned)max_units.
__device__ __forceinline__ int UnitMap::slot(int key) const {
  unsigned h = hash_unit_key(key, shift);
  for (int probe = 0; probe <= cap_mask; ++probe) {
    const int e = (int)((h + (unsigned)probe) & (unsigned)cap_mask);
    const int k = ht_key[e];
    if (k == key) return ht_slot[e];
    if (k == kEmptyKey) return -1;
  }
  return -1;
}

namespace {

// The write half of one source pixel p of frame f that landed on `cell` with depth dd (IntegrateApp.cpp:260-263).
__device__ __forceinline__ void scatter_px(const ReprojArgs& A, int f, int p, int cell, uint16_t dd, int replay) {
  const size_t o = (size_t)f * ((size_t)A.cols * A.rows) + cell;
  if (!replay) {
    if (dd != 0) {
      atomicMin(&A.zbuf[o], A.ztag | (uint32_t)dd);                    // below every cell of an older epoch (er_tsdf.h: kZEpochMax)
    } else {
      atomicMax(&A.lastzero[o], (uint32_t)p + 1u);
      atomicOr(&A.zero_flag[f >> 5], 1 << (f & 31));
    }
  } else {
    const uint32_t lz = A.lastzero[o];
    if (dd != 0 && lz > 0 && (uint32_t)p + 1u > lz) atomicMin(&A.zfix[o], (uint32_t)dd);
  }
}

// One source pixel (u, v) of frame f through the EXACT chain: warp, then scatter (replay = 0) or re-scatter under the
// replay rule (replay = 1).
__device__ __forceinline__ void reproject_scatter_px(const ReprojArgs& A, int f, int u, int v, int replay) {
  const int pixels = A.cols * A.rows;
  const int p = v * A.cols + u;
  const uint16_t d = A.depth[(size_t)f * pixels + p];
  if (d == 0) return;                                                   // UVD2XYZ false
  int cell;
  uint16_t dd;
  if (!reproject_px(u, v, d, A.cam, A.cami, A.cols, A.rows, A.seg12 + f * 16, A.madj12 + f * 12,
                    A.ctr + (size_t)A.grid_index[f] * A.floats_per_grid, A.res, A.grid_ul, cell, dd))
    return;
  scatter_px(A, f, p, cell, dd, replay);
}

// The consumer's reading of z-buffer cell z under the tag of the current epoch: the depth, or kZEmpty for a cell that this epoch's scatter did not
// write (whatever an older one left there).
__device__ __forceinline__ uint32_t z_of_epoch(uint32_t z, uint32_t ztag) {
  const uint32_t x = z ^ ztag;
  return x < 0x10000u ? x : kZEmpty;
}

// The consumer's half of the replay: the value of z-buffer cell o of a FLAGGED frame (z = what the plain scatter-min left there);
// cells that saw a zero write take the replay's value and re-arm both side buffers.
__device__ __forceinline__ uint32_t take_z(uint32_t z, size_t o, uint32_t* __restrict__ lastzero, uint32_t* __restrict__ zfix) {
  if (lastzero[o] == 0) return z;
  const uint32_t r = zfix[o];
  zfix[o] = kZEmpty;
  lastzero[o] = 0;
  return r;
}

}  // namespace
}  // namespace er_tsdf_k
