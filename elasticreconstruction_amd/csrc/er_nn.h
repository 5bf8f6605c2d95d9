// er_nn.h -- the device side of path B's exact nearest-neighbour search over a cloud's uniform grid (er_grid.h), for every translation unit that
// searches: the address-space pointer types, the block-cooperative search nn_block and the block reduction its callers end with.  Everything here is
// __device__ __forceinline__ or constexpr.
#pragma once

#include "er_grid.h"

namespace er {

// PairDev carries its pointers through memory, so the compiler emits FLAT loads for them (64-bit VALU address arithmetic, both wait counters).
// The hot accesses go through explicitly GLOBAL pointer types: global_load with a scalar base and a 32-bit offset, vmcnt only.
typedef float f4v __attribute__((ext_vector_type(4)));
#define ER_GLOBAL __attribute__((address_space(1)))
typedef const ER_GLOBAL f4v* gp_f4;
typedef const ER_GLOBAL float* gp_f;
typedef const ER_GLOBAL int* gp_i;
typedef ER_GLOBAL float* gp_fw;
typedef ER_GLOBAL int* gp_iw;
#define ER_GP(type, ptr) ((type)(ptr))

constexpr int kPadBatch = 4;   // rows whose four bounds are in flight at a time (4 registers per row; 8 = all rows: +11 VGPRs, within the noise)
typedef int i4v __attribute__((ext_vector_type(4), aligned(4)));   // (the four bounds of a row start at an arbitrary cell: 4-byte alignment only)

// Exact 1-NN of q among the target points of the 27 neighbouring cells: float32 squared distance ((dx*dx) + dy*dy) + dz*dz (FLANN L2_Simple), ties ->
// lower original index.  limit2 = squared search radius: callers discard anything farther, so cells lying entirely beyond it are skipped (margin: 1e-4
// relative plus an absolute part sized from the grid's extent, see grid_slack).
// Block-cooperative, two phases (one query per thread, kBlock queries per workgroup):
//   phase 0  the thread scans its query's own cell, then the left / right cell of the home row if its face is closer than the best so far; the eight
//            neighbour rows are trimmed by the same face tests and their NON-EMPTY ranges go to an LDS task list as (first candidate, count, query);
//   phase 1  the workgroup shares the list -- one range per thread and trip -- folding results into the query's packed (distance bits, index) key with a
//            64-bit LDS atomicMin, which IS the lexicographic (distance, index) minimum.
// Why: ~1.7 of the 8 neighbour rows survive for an average query, but a SIMT loop runs every row ANY lane needs; compacting the survivors across the
// workgroup removes that waste.  Candidates are scanned kUnroll at a time (the 16-byte loads are issued together).  What bounds it (counters,
// profiles/r04w_*, r05f_*): VALU issue in the straight-line part every query runs (~360 of ~735 instructions per slice of 64 queries) and LDS traffic per task.
constexpr int kUnroll = 4;
constexpr unsigned long long kNoHit = ((unsigned long long)0x7f7fffffu << 32) | 0xffffffffull;   // (FLT_MAX, -1)

constexpr int kTaskCap = kBlock * 4;   // (query, row) tasks of phase 1 held in LDS; a task beyond that is scanned by the thread that found it

struct NnShared {
  unsigned long long best[kBlock];
  float q[3][kBlock];
  int task_s0[kTaskCap];          // first candidate of the task's range in the cell-sorted target
  int task_nq[kTaskCap];          // candidates << 8 | query
  int ntask;
};

// Candidates [s0, s1) of the cell-sorted target against the query: the packed (distance bits, index) minimum -- every candidate against the key, exact by
// construction; ~54 VALU instructions per trip of four, 20 of them the selection.
// The kU loads of a trip are NOT clamped to the range: a trip that starts inside [s0, s1) may read up to kU - 1 entries past s1.  Those are points of the
// cells that follow in the cell-sorted array -- REAL points of the same cloud, so the minimum over the wider set is still the exact nearest neighbour --
// or, behind the cloud's last point, the kSentinel entries of +inf er_cloud_create appends (distance inf / NaN: a bit pattern that never wins).
template <int kU = kUnroll>
__device__ __forceinline__ unsigned long long scan_range(const Grid& g, int s0, int s1, float qx, float qy, float qz, unsigned long long key) {
  // candidates are addressed by UNSIGNED 32-bit byte offsets from the (wave-uniform) base: a scalar-base global load and one 32-bit
  // add per candidate instead of a sign extension and a 64-bit multiply-add each
  const ER_GLOBAL char* base = (const ER_GLOBAL char*)g.pts;
  const unsigned last = (unsigned)(s1 - 1) * 16u;
  for (unsigned o = (unsigned)s0 * 16u; o <= last && s0 < s1; o += 16u * kU) {
    f4v p[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) p[u] = *(const ER_GLOBAL f4v*)(base + o + 16u * (unsigned)u);
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const float dx = qx - p[u].x, dy = qy - p[u].y, dz = qz - p[u].z;
      const float d = ((dx * dx) + dy * dy) + dz * dz;
      // d >= 0, so its bit pattern orders like its value; NaN / inf patterns exceed FLT_MAX's and never win
      const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(p[u].w);
      key = k < key ? k : key;
    }
  }
  return key;
}

// Every thread of the workgroup must call this (it synchronises); `active` = this thread carries a query.
// Returns the index (or -1) and the squared distance of the nearest target point.  A cell is skipped only when every point in it is provably
// farther than the best so far: its nearest face already is, with the 1e-4 relative margin of grid_slack; ties cannot hide there.
// hit2 >= 0 (the Registration pre-check): the caller only needs to know whether ANY target point lies closer than sqrt(hit2) -- "count the points
// whose nearest neighbour is within reg_dist" is "count the points that have a neighbour within reg_dist" -- so a query stops as soon as it holds a
// candidate below hit2; the returned distance is then that candidate's, not the minimum.  Queries without one run the full exact search.
// kU = candidates per trip: 4 where the nearest neighbour is needed, 3 in the any-hit pre-check (profiles/r04t_ab_scan_unroll.txt).
template <int kU = kUnroll>
__device__ __forceinline__ int nn_block(NnShared& sh, const Grid& g, bool active, float qx, float qy, float qz, float limit2,
                                        float& best_d, float hit2 = -1.f) {
  const int tid = threadIdx.x;
  __syncthreads();                                            // the previous call's readers are done with `sh`
  if (tid == 0) sh.ntask = 0;
  // the query's cell (float32 expressions shared with the grid build)
  const float ux = (qx - g.org[0]) / g.cell, uy = (qy - g.org[1]) / g.cell, uz = (qz - g.org[2]) / g.cell;
  const float cx = floorf(ux), cy = floorf(uy), cz = floorf(uz);
  const bool inside = active && cx >= -1.f && cx <= (float)g.dim[0] && cy >= -1.f && cy <= (float)g.dim[1] && cz >= -1.f && cz <= (float)g.dim[2];
  const int ix = inside ? (int)cx : 0, iy = inside ? (int)cy : 0, iz = inside ? (int)cz : 0;
  __syncthreads();                                            // (sh.ntask is zero)
  unsigned long long key = kNoHit;
  // A query whose whole 27-neighbourhood is empty (55-63 % of the queries of a fragment pair: the part of the source that does not overlap the target)
  // has no neighbour within the radius; one byte per cell (k_chunk_occ) says so before the row tests.  Queries come in the source's cell order: whole
  // waves leave here (9-10 % of the ICP phase, profiles/r06c_*).
  const bool live = inside && ER_GP(const ER_GLOBAL unsigned char*, g.occ)[(unsigned)(((iz + 2) * g.pny + (iy + 2)) * g.pnx + (ix + 2))] != 0;
  if (live) {
    // distance from q to the lower / upper face of its own cell along x, y and z (metres), squared
    const float xlo = (ux - cx) * g.cell, xhi = g.cell - xlo, ylo = (uy - cy) * g.cell, yhi = g.cell - ylo, zlo = (uz - cz) * g.cell,
                zhi = g.cell - zlo;
    const float xl2 = xlo * xlo, xr2 = xhi * xhi;
    float bound = limit2 * 1.0001f + g.slack;
    const ER_GLOBAL char* csb = (const ER_GLOBAL char*)g.cell_start;
    const int pnx = g.pnx, pny = g.pny;
    int home = ((iz + 2) * pny + (iy + 2)) * pnx + (ix + 1);   // the cell LEFT of the query's own cell: where the four bounds of a row's three cells begin
    {
      const i4v h = *(const ER_GLOBAL i4v*)(csb + (unsigned)home * 4u);   // L, O, R, E of the home row
      key = scan_range<kU>(g, h.y, h.z, qx, qy, qz, key);                  // the query's own cell first
      bound = fminf(bound, __uint_as_float((unsigned)(key >> 32)) * 1.0001f + g.slack);   // the other cells must beat this one
      if (__uint_as_float((unsigned)(key >> 32)) < hit2) bound = -1.f;                   // (any-hit mode: done)
      if (xl2 <= bound) {
        key = scan_range<kU>(g, h.x, h.y, qx, qy, qz, key);
        bound = fminf(bound, __uint_as_float((unsigned)(key >> 32)) * 1.0001f + g.slack);
        if (__uint_as_float((unsigned)(key >> 32)) < hit2) bound = -1.f;
      }
      if (xr2 <= bound) {
        key = scan_range<kU>(g, h.z, h.w, qx, qy, qz, key);
        bound = fminf(bound, __uint_as_float((unsigned)(key >> 32)) * 1.0001f + g.slack);
        if (__uint_as_float((unsigned)(key >> 32)) < hit2) bound = -1.f;
      }
    }
    sh.q[0][tid] = qx;
    sh.q[1][tid] = qy;
    sh.q[2][tid] = qz;
    // the eight neighbour rows: wave-uniform steps away from the home row, every one of them inside the array -- all eight 16-byte loads are issued
    // up front behind one wait (a row that does not survive the test below is loaded anyway: no address select)
    asm volatile("" : "+v"(home));                            // (opaque, or the compiler folds the steps back into y and z)
    const float yl2 = ylo * ylo, yh2 = yhi * yhi, zl2 = zlo * zlo, zh2 = zhi * zhi;
    int r_s0[8], r_n[8];
#pragma unroll
    for (int j0 = 0; j0 < 8; j0 += kPadBatch) {                 // (kPadBatch rows' bounds in flight at a time: 4 registers per row)
      i4v rb[kPadBatch];
#pragma unroll
      for (int jj = 0; jj < kPadBatch; jj++) {
        const int j = j0 + jj, pass = j < 4 ? j : j + 1;
        const int dy = pass % 3 - 1, dz = pass / 3 - 1;
        rb[jj] = *(const ER_GLOBAL i4v*)(csb + (unsigned)(home + (dz * pny + dy) * pnx) * 4u);
      }
#pragma unroll
      for (int jj = 0; jj < kPadBatch; jj++) {
        const int j = j0 + jj, pass = j < 4 ? j : j + 1;
        const int dy = pass % 3 - 1, dz = pass / 3 - 1;
        const float e2 = (dy < 0 ? yl2 : (dy > 0 ? yh2 : 0.f)) + (dz < 0 ? zl2 : (dz > 0 ? zh2 : 0.f));
        const bool wl = xl2 + e2 <= bound, wr = xr2 + e2 <= bound;
        const int s0 = wl ? rb[jj].x : rb[jj].y, s1 = wr ? rb[jj].w : rb[jj].z;
        r_s0[j] = s0;
        r_n[j] = e2 <= bound ? s1 - s0 : 0;
        asm volatile("" : "+v"(r_s0[j]), "+v"(r_n[j]));         // materialised HERE: the four bounds die now (left alone, the compiler sinks the selects
      }                                                        // to each row's push and keeps all 32 bound registers alive across the fallback scans)
      __builtin_amdgcn_sched_barrier(0);                       // (... and the scheduler hoists all eight loads above the first batch's selects)
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int n = r_n[j];
      if (n > 0) {
        const int t = n < (1 << 23) ? atomicAdd(&sh.ntask, 1) : kTaskCap;
        if (t < kTaskCap) {
          sh.task_s0[t] = r_s0[j];
          sh.task_nq[t] = (n << 8) | tid;
        } else {                                              // the task list is full (or the range does not fit the packing): scan it here
          key = scan_range<kU>(g, r_s0[j], r_s0[j] + n, qx, qy, qz, key);
        }
      }
    }
  }
  sh.best[tid] = key;
  __syncthreads();
  const int nt = min(sh.ntask, kTaskCap);
  for (int t = tid; t < nt; t += kBlock) {
    const int s0 = sh.task_s0[t], nq = sh.task_nq[t], q = nq & 255;
    const unsigned long long k = scan_range<kU>(g, s0, s0 + (nq >> 8), sh.q[0][q], sh.q[1][q], sh.q[2][q], kNoHit);
    atomicMin(&sh.best[q], k);
  }
  __syncthreads();
  key = sh.best[tid];
  best_d = __uint_as_float((unsigned)(key >> 32));
  return (int)(unsigned)(key & 0xffffffffull);              // 0xffffffff -> -1
}

using NnSh = NnShared;

// Block reduction of NV float64 values per thread: wave shuffle (64 lanes) -> LDS -> lane 0 atomics.
template <int NV>
__device__ __forceinline__ void block_reduce_atomic(double (&v)[NV], double* __restrict__ out) {
  __shared__ double part[kBlock / 64][NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    double s = v[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (lane == 0) part[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) s += part[w][threadIdx.x];
    if (s != 0.0) atomicAdd(&out[threadIdx.x], s);
  }
}

}  // namespace er
