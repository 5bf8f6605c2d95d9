// er_tsdf_extract.hip -- what leaves the resident TSDF volume of path A (er_tsdf.hip): SaveWorld's voxel list, the zero crossings with and without
// normals, the oriented cloud handed to path B on the device, and the marching-cubes mesh, as a triangle soup and indexed -- and SaveWorld's
// inverse, the one way back in.  Every extraction kernel makes two passes over the slabs (64 per unit) of the units in ascending key order --
// count, then write at the slab's offset -- so the lists are reproducible element for element.
#include "er_tsdf_dev.h"
#include "er_mc_table.h"

#include <climits>
#include <cmath>

namespace {

using namespace er_tsdf_k;

// The frame of the five kernels that run one wave per (unit, i-slab) -- k_world, k_surface, k_mesh, k_mesh_index, k_mesh_verts: block 64 * rank + i,
// rank = the unit's place in ascending key order, lane = k; the wave walks the slab's 64 rows j.
struct Slab {
  int rank, i, lane, key, xi, yi, zi;
  __device__ __forceinline__ explicit Slab(const int* __restrict__ keys)
      : rank(blockIdx.x >> 6), i(blockIdx.x & 63), lane(threadIdx.x), key(keys[rank]), xi(key >> 18), yi((key >> 9) & 511), zi(key & 511) {}
  // float32 position of the lane's voxel (i, j, k); d = 1: of the voxel one step up that axis
  __device__ __forceinline__ float x(int d = 0) const { return lattice_pos(i + d, xi); }
  __device__ __forceinline__ float y(int j) const { return lattice_pos(j, yi); }
  __device__ __forceinline__ float z(int d = 0) const { return lattice_pos(lane + d, zi); }
};

// SaveWorld's filter (TSDFVolume.cpp:118).  One wave per (unit, i-slab); pass 0 counts, pass 1 writes
// the points in i,j,k order at the slab's offset (stable compaction by ballot prefix).
__device__ __forceinline__ bool world_keep(float2 v) { return v.y != 0.0f && v.x < 0.98f && v.x >= -0.98f; }

__global__ __launch_bounds__(64) void k_world(const float2* __restrict__ pool, const int* __restrict__ slots,
                                              const int* __restrict__ keys, long* __restrict__ slab_count,
                                              const long* __restrict__ slab_offset, float4* __restrict__ out, int pass) {
  const Slab S(keys);
  const int i = S.i, lane = S.lane;
  const float2* slab = pool + (size_t)slots[S.rank] * kUnitVox + (size_t)i * 4096;
  long base = pass ? slab_offset[blockIdx.x] : 0;
  long total = 0;
  for (int j = 0; j < 64; j++) {
    const float2 v = slab[j * 64 + lane];
    const bool keep = world_keep(v);
    const unsigned long long b = __ballot(keep);
    if (pass && keep) {
      const long o = base + total + wave_rank(b, lane);
      out[o] = make_float4((float)(i + (S.xi - 256) * 64), (float)(j + (S.yi - 256) * 64), (float)(lane + (S.zi - 256) * 64), v.x);
    }
    total += __popcll(b);
  }
  if (!pass && lane == 0) slab_count[blockIdx.x] = total;
}

// Zero-crossing extraction on the resident volume (what the out-of-repo kinfu "mesh_output" step does with
// world.pcd, done where the volume lives).  For every observed voxel (weight != 0) and each of its +x, +y, +z neighbours --
// inside the unit or in the adjacent unit, found through the hash map -- that is observed too: if the two sdf values have
// strictly opposite signs, the surface crosses that lattice edge at t = F / (F - Fn) and the point
//     p = voxel position + t * voxel size along the axis            (float32; position = (float)(global index * 3/512))
// is emitted (kinfu's extractCloud rule).  Order: units by ascending key, voxels in i,j,k order, axes x,y,z -- a stable
// ballot-prefix compaction in two passes like k_world, so the list is reproducible and a CPU restatement can match it
// element for element (tests/test_tsdf_gpu.py).
__device__ __forceinline__ bool crosses(float2 a, float2 b) {
  return a.y != 0.0f && b.y != 0.0f && ((a.x > 0.0f && b.x < 0.0f) || (a.x < 0.0f && b.x > 0.0f));
}

// A slab's voxels and their +x / +y / +z neighbours, inside the unit or in the adjacent one (wave-uniform look-ups): a voxel of a unit that does
// not exist or lies beyond the lattice reads as unobserved, {0, 0}.  k_surface's and k_mesh_verts' reading of the volume.
struct SlabVoxels {
  const float2 *slab, *slab_x, *unit_y, *unit_z;
  int lane;
  __device__ __forceinline__ SlabVoxels(const VolumeView& vol, const Slab& S, int slot) : lane(S.lane) {
    slab = vol.unit(slot) + (size_t)S.i * 4096;
    const int sx = (S.i == 63 && S.xi < 511) ? vol.map.slot(S.key + 512 * 512) : -1;
    const int sy = S.yi < 511 ? vol.map.slot(S.key + 512) : -1;
    const int sz = S.zi < 511 ? vol.map.slot(S.key + 1) : -1;
    slab_x = S.i < 63 ? slab + 4096 : (sx >= 0 ? vol.unit(sx) : nullptr);              // i + 1 (slab 0 of the next unit)
    unit_y = sy >= 0 ? vol.unit(sy) + (size_t)S.i * 4096 : nullptr;                     // j + 1 == 64: row 0 there
    unit_z = sz >= 0 ? vol.unit(sz) + (size_t)S.i * 4096 : nullptr;                     // k + 1 == 64: voxel 0 there
  }
  __device__ __forceinline__ float2 at(int j) const { return slab[j * 64 + lane]; }
  __device__ __forceinline__ float2 up_x(int j) const { return slab_x ? slab_x[j * 64 + lane] : make_float2(0.0f, 0.0f); }
  __device__ __forceinline__ float2 up_y(int j) const { return j < 63 ? slab[(j + 1) * 64 + lane] : (unit_y ? unit_y[lane] : make_float2(0.0f, 0.0f)); }
  // (every lane of the wave calls it: v = at(j), the neighbour is the next lane's)
  __device__ __forceinline__ float2 up_z(int j, float2 v) const {
    float2 nz;
    nz.x = __shfl_down(v.x, 1);
    nz.y = __shfl_down(v.y, 1);
    if (lane == 63) nz = unit_z ? unit_z[j * 64] : make_float2(0.0f, 0.0f);
    return nz;
  }
};

// Where the surface crosses the lattice edge that leaves the voxel at (px, py, pz) along `axis`: F / (F - Fn) of a voxel up that axis, F and Fn the
// sdf of the voxel and of its neighbour there; w = the axis.  The one statement of k_surface's point, the indexed mesh's vertex and k_mesh's corner.
__device__ __forceinline__ float4 edge_point(float px, float py, float pz, int axis, float F, float Fn) {
  const float d = (F / (F - Fn)) * (float)kUnitLength;
  return make_float4(axis == 0 ? px + d : px, axis == 1 ? py + d : py, axis == 2 ? pz + d : pz, (float)axis);
}

__global__ __launch_bounds__(64) void k_surface(VolumeView vol, const int* __restrict__ slots, const int* __restrict__ keys,
                                                long* __restrict__ slab_count, const long* __restrict__ slab_offset,
                                                float4* __restrict__ out, int pass) {
  const Slab S(keys);
  const SlabVoxels V(vol, S, slots[S.rank]);
  const float gx = S.x(), gz = S.z();
  const unsigned long long lt = (1ull << S.lane) - 1ull;
  long base = pass ? slab_offset[blockIdx.x] : 0;
  long total = 0;
  for (int j = 0; j < 64; j++) {
    const float2 v = V.at(j);
    const float2 nx = V.up_x(j), ny = V.up_y(j), nz = V.up_z(j, v);
    const bool cx = crosses(v, nx), cy = crosses(v, ny), cz = crosses(v, nz);
    const unsigned long long bx = __ballot(cx), by = __ballot(cy), bz = __ballot(cz);
    if (pass) {
      long o = base + total + __popcll(bx & lt) + __popcll(by & lt) + __popcll(bz & lt);
      const float gy = S.y(j);
      if (cx) out[o++] = edge_point(gx, gy, gz, 0, v.x, nx.x);
      if (cy) out[o++] = edge_point(gx, gy, gz, 1, v.x, ny.x);
      if (cz) out[o++] = edge_point(gx, gy, gz, 2, v.x, nz.x);
    }
    total += __popcll(bx) + __popcll(by) + __popcll(bz);
  }
  if (!pass && S.lane == 0) slab_count[blockIdx.x] = total;
}

// Oriented extraction (what the kinfu fragment step leaves in cloud_bin_<i>.pcd and CorresApp.cpp:82-99 reads back: the zero crossings WITH
// normals): a float4 {nx, ny, nz, 0} for every point of k_surface's list, at the same index.  The normal is the normalised central difference
// of the sdf at the point's NEAREST voxel v = rint((double)p / unit length) per component -- along the point's axis the crossed edge's lower
// voxel or the one above it, on the other two axes the lattice index itself -- and exists only if v and its six neighbours are all observed
// (weight != 0; a voxel of a unit that does not exist or lies outside the 512-unit lattice is unobserved) and the gradient is not zero;
// otherwise it is NaN in all three components.  g = S[v + e] - S[v - e], n2 = (gx gx + gy gy) + gz gz, n = g / sqrt(n2): float32, every
// operation rounded on its own (-ffp-contract=off, correctly rounded '/' and sqrtf), so a numpy restatement matches bit for bit
// (tests/test_oriented_gpu.py).
// One THREAD per point, behind k_surface's own write pass.  A first version did the seven fetches inside the slab loop of a copy of k_surface
// (one wave per slab, 64 serial rows): the rows with a crossing -- most rows of a slab the surface passes through -- each waited for three
// more dependent round trips to memory, 523 us against k_surface's 160 us on a 147-unit fragment (profiles/oriented_extraction.txt).  Here
// every point is independent: one hash-map lookup for the unit of v, direct addresses for the neighbours that stay in it, a lookup of their
// own for those across a unit border.  g = voxel index on the whole lattice, 0 .. 512 * 64 - 1 per axis.
__device__ __forceinline__ float2 fetch_voxel(const VolumeView& vol, const float2* __restrict__ unit, int key, int gx, int gy, int gz) {
  if (!on_lattice(gx, gy, gz)) return make_float2(0.0f, 0.0f);
  const int k = unit_key_of(gx, gy, gz);
  const size_t l = unit_offset_of(gx, gy, gz);
  if (k == key) return unit[l];
  const int s = vol.map.slot(k);
  return s >= 0 ? vol.unit(s)[l] : make_float2(0.0f, 0.0f);
}

// the nearest voxel's index: rint((double)p / unit length), round half to even, on the 0-based lattice
__device__ __forceinline__ int nearest_index(float p) { return (int)rint((double)p / kUnitLength) + 256 * 64; }

__global__ __launch_bounds__(256) void k_surface_normals(VolumeView vol, const float4* __restrict__ pts, long n, float4* __restrict__ out_n) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float4 p = pts[r];
  const int gx = nearest_index(p.x), gy = nearest_index(p.y), gz = nearest_index(p.z);
  // the unit of v: key -1 (matches no voxel) if v is outside the lattice or its unit does not exist -- the fetches then find that out themselves
  const bool in = on_lattice(gx, gy, gz);
  int key = in ? unit_key_of(gx, gy, gz) : -1;
  const int slot = in ? vol.map.slot(key) : -1;
  if (slot < 0) key = -1;
  const float2* unit = vol.unit(slot < 0 ? 0 : slot);
#define ER_F(dx, dy, dz) fetch_voxel(vol, unit, key, gx + (dx), gy + (dy), gz + (dz))
  const float2 c = ER_F(0, 0, 0);
  const float2 xl = ER_F(-1, 0, 0), xh = ER_F(1, 0, 0), yl = ER_F(0, -1, 0), yh = ER_F(0, 1, 0), zl = ER_F(0, 0, -1), zh = ER_F(0, 0, 1);
#undef ER_F
  const bool seen = c.y != 0.0f && xl.y != 0.0f && xh.y != 0.0f && yl.y != 0.0f && yh.y != 0.0f && zl.y != 0.0f && zh.y != 0.0f;
  const float ax = xh.x - xl.x, ay = yh.x - yl.x, az = zh.x - zl.x;
  const float nrm = sqrtf((ax * ax + ay * ay) + az * az);
  const float nan = __int_as_float(0x7fc00000);
  out_n[r] = seen && nrm > 0.0f ? make_float4(ax / nrm, ay / nrm, az / nrm, 0.0f) : make_float4(nan, nan, nan, 0.0f);
}

// The rows CCorresApp::LoadData keeps (CorresApp.cpp:93-98: normal_x is not NaN) that also lie in the fragment's cube 0 <= x, y, z < cube
// (PointCloud::GetCoordinate; cube <= 0: no cube test), compacted in order into packed xyz / normal rows -- er_cloud_create's input layout.
// One wave per 64 rows -- a block of one wave, so its ballot is the block's tally -- in the two passes of er_compact.h.
__global__ __launch_bounds__(64) void k_oriented_keep(const float4* __restrict__ pts, const float4* __restrict__ nrm, long n, float cube,
                                                      long* __restrict__ blk_count, const long* __restrict__ blk_offset,
                                                      float* __restrict__ xyz_out, float* __restrict__ nrm_out, int pass) {
  const int lane = threadIdx.x;
  const long r = (long)blockIdx.x * 64 + lane;
  bool keep = false;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f), q = p;
  if (r < n) {
    p = pts[r];
    q = nrm[r];
    keep = !(q.x != q.x) && (!(cube > 0.0f) || (p.x >= 0.0f && p.y >= 0.0f && p.z >= 0.0f && p.x < cube && p.y < cube && p.z < cube));
  }
  const unsigned long long b = __ballot(keep);
  if (!pass) {
    if (lane == 0) blk_count[blockIdx.x] = __popcll(b);
    return;
  }
  if (keep) {
    const size_t o = (size_t)(blk_offset[blockIdx.x] + wave_rank(b, lane)) * 3;
    xyz_out[o] = p.x;
    xyz_out[o + 1] = p.y;
    xyz_out[o + 2] = p.z;
    nrm_out[o] = q.x;
    nrm_out[o + 1] = q.y;
    nrm_out[o + 2] = q.z;
  }
}


// Marching cubes on the resident volume (the triangle connectivity the out-of-repo kinfu "mesh_output" step builds
// from world.pcd, done where the volume lives).  Cell (i, j, k) of a unit = the eight voxels (i..i+1, j..j+1, k..k+1) -- the last
// layer of cells reaches into the adjacent units (+x, +y, +z and their combinations, found through the hash map).  A cell
// yields triangles only if all eight voxels are observed (weight != 0, kinfu's rule); corner c is inside iff sdf < 0; the case
// table is generated on the host (er_mc_table.h) and staged in LDS.  A vertex on the lattice edge from the lower voxel L to the
// upper voxel H lies at  pos(L) + (F_L / (F_L - F_H)) * voxel size  along the edge's axis (float32; pos = (float)(global index *
// 3/512)) -- evaluated from the edge's LOWER end whichever cell asks, so the cells that share the edge produce the same bits and
// the triangle soup is watertight by vertex equality.  Order: units by ascending key, cells in i, j, k order, triangles in table
// order; two passes (count, then write at the slab's offset: a stable ballot-prefix compaction) like k_world / k_surface.

// element idx of a table of eight that lives in registers: a select chain over the VALUES (a run-time index, or a chain over references to
// the array's elements, which the compiler folds back into one, sends the table through scratch)
__device__ __forceinline__ int pick8v(int t0, int t1, int t2, int t3, int t4, int t5, int t6, int t7, int idx) {
  int r = t0;
  r = idx == 1 ? t1 : r;
  r = idx == 2 ? t2 : r;
  r = idx == 3 ? t3 : r;
  r = idx == 4 ? t4 : r;
  r = idx == 5 ? t5 : r;
  r = idx == 6 ? t6 : r;
  r = idx == 7 ? t7 : r;
  return r;
}
#define ER_PICK8(t, idx) pick8v(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], idx)

// Edge id e of the case table: its axis and the cell corner (a0, b0, c0) it STARTS at -- coordinate 0 along its axis; it ends one step up the axis.
struct CellEdge {
  int axis, a0, b0, c0;
  __device__ __forceinline__ explicit CellEdge(int e) {
    const int u = e & 1, v = (e >> 1) & 1;
    axis = e >> 2;
    a0 = axis == 0 ? 0 : u, b0 = axis == 1 ? 0 : (axis == 0 ? u : v), c0 = axis == 2 ? 0 : v;
  }
  __device__ __forceinline__ int corner() const { return a0 | b0 << 1 | c0 << 2; }
};

// The walk of k_mesh and k_mesh_index over a slab's cells, one row j of 64 cells at a time: what the two kernels know before they do their own
// thing with a cell's triangles (emit positions; mark the bitmap or emit indices).  The constructor holds the kernel's one __syncthreads().
// kRanks: also the units' ranks (position in key order; -1: none, or dropped), for the kernel that addresses per-unit arrays of its own.
template <bool kRanks>
struct CellWalk {
  const unsigned char* tab;                    // the case table, staged in LDS
  const float2* pool;
  int lane;
  // the (up to) eight units a slab of cells can touch: pool slots and ranks, [dx << 2 | dy << 1 | dz]; -1 = that unit does not exist (its voxels
  // count as unobserved).  Constant indices and ER_PICK8 only.
  int us[8], rk[8];
  int ia[2], ux[2];                            // slab index and unit offset dx of the two i layers

  __device__ __forceinline__ CellWalk(const VolumeView& vol, const Slab& S, int own_slot, const unsigned char* __restrict__ table,
                                      const int* __restrict__ slot_rank)
      : pool(vol.pool), lane(S.lane) {
    __shared__ unsigned char s_tab[256 * 16];
    for (int t = threadIdx.x; t < 256 * 16 / 4; t += 64) reinterpret_cast<unsigned*>(s_tab)[t] = reinterpret_cast<const unsigned*>(table)[t];
    __syncthreads();
    tab = s_tab;
#pragma unroll
    for (int dx = 0; dx < 2; dx++)
#pragma unroll
      for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dz = 0; dz < 2; dz++) {
          const bool need = (dx == 0 || S.i == 63);
          const bool ok = S.xi + dx < 512 && S.yi + dy < 512 && S.zi + dz < 512;
          const int s = (dx | dy | dz) == 0 ? own_slot : (need && ok ? vol.map.slot(S.key + dx * 512 * 512 + dy * 512 + dz) : -1);
          us[dx << 2 | dy << 1 | dz] = s;
          if (kRanks) rk[dx << 2 | dy << 1 | dz] = s >= 0 ? slot_rank[s] : -1;
        }
    ia[0] = S.i, ia[1] = S.i == 63 ? 0 : S.i + 1;
    ux[0] = 0, ux[1] = S.i == 63 ? 1 : 0;
  }

  // index into us / rk of the unit that holds row jj = j + b (0 .. 64) of i layer a, at dz = 0; | 1: its +z neighbour
  __device__ __forceinline__ int unit_at(int a, int jj) const { return ux[a] << 2 | (jj >> 6) << 1; }
  __device__ __forceinline__ int rank_at(int idx) const { return ER_PICK8(rk, idx); }

  // Row j: the eight corners of this lane's cell, f[a | b << 1 | c << 2] = voxel (i + a, j + b, k + c), and the cell's row of the case table;
  // -> its number of triangles, 0 unless all eight corners are observed.  Every lane of the wave calls it.
  __device__ __forceinline__ int cell(int j, float2 (&f)[8], const unsigned char*& row) const {
    // (the unobserved voxel is a VALUE in these conditionals: between two named objects the compiler selects an address, and one is in scratch)
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int jb = (j + b) & 63;
        const int s0 = ER_PICK8(us, unit_at(a, j + b)), s1 = ER_PICK8(us, unit_at(a, j + b) | 1);
        const size_t ro = (size_t)ia[a] * 4096 + (size_t)jb * 64;
        const float2 v = s0 >= 0 ? pool[(size_t)s0 * kUnitVox + ro + lane] : make_float2(0.0f, 0.0f);
        f[a | b << 1] = v;
        float2 w;
        w.x = __shfl_down(v.x, 1);
        w.y = __shfl_down(v.y, 1);
        if (lane == 63) w = s1 >= 0 ? pool[(size_t)s1 * kUnitVox + ro] : make_float2(0.0f, 0.0f);
        f[a | b << 1 | 4] = w;
      }
    bool valid = true;
    int cs = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      valid = valid && f[c].y != 0.0f;
      cs |= (f[c].x < 0.0f ? 1 : 0) << c;
    }
    row = tab + cs * 16;
    int nt = 0;
    if (valid)
      while (nt < 5 && row[3 * nt] != 255) nt++;
    return nt;
  }
};

__global__ __launch_bounds__(64) void k_mesh(VolumeView vol, const int* __restrict__ slots, const int* __restrict__ keys,
                                             const unsigned char* __restrict__ table, long* __restrict__ slab_count,
                                             const long* __restrict__ slab_offset, float* __restrict__ out, int pass) {
  const Slab S(keys);
  const CellWalk<false> W(vol, S, slots[S.rank], table, nullptr);
  const float gx = S.x(), gz = S.z();
  long base = pass ? slab_offset[blockIdx.x] : 0;
  long total = 0;
  for (int j = 0; j < 64; j++) {
    float2 f[8];
    const unsigned char* row;
    const int nt = W.cell(j, f, row);
    const int incl = wave_inclusive_sum(nt, S.lane);     // (k order)
    const int wave_total = __shfl(incl, 63);
    if (pass && nt > 0) {
      const float gy = S.y(j);
      float* __restrict__ o = out + (size_t)(base + total + (incl - nt)) * 9;
      for (int t = 0; t < 3 * nt; t++) {
        const CellEdge E(row[t]);
        // the edge's two ends; the eight corner values sit in registers, so they are picked with select chains, not with a runtime index
        const int cl = E.corner(), ch = cl | (1 << E.axis);
        float2 lo = f[0], hi = f[0];
#pragma unroll
        for (int c = 1; c < 8; c++) {
          lo = c == cl ? f[c] : lo;
          hi = c == ch ? f[c] : hi;
        }
        // from the lower end of the edge, voxel (i + a0, j + b0, k + c0)
        const float4 p = edge_point(E.a0 ? S.x(1) : gx, E.b0 ? S.y(j + 1) : gy, E.c0 ? S.z(1) : gz, E.axis, lo.x, hi.x);
        o[3 * t] = p.x;
        o[3 * t + 1] = p.y;
        o[3 * t + 2] = p.z;
      }
    }
    total += wave_total;
  }
  if (!pass && S.lane == 0) slab_count[blockIdx.x] = total;
}

// The INDEXED mesh (er_tsdf_extract_mesh_indexed): k_mesh's triangles as three int32 indices into a list of unique vertices.
// A vertex is a lattice EDGE -- its lower voxel L and an axis -- that at least one emitted triangle uses, never a position: two edges that
// meet in a voxel whose sdf is exactly 0 give the same coordinates and stay two vertices.  Vertex order: the unit of L by ascending key, L in
// i, j, k order, axes x, y, z (k_surface's order; not its set).  No sort and no float atomic; four passes over the slabs:
//   k_mesh_index, pass 0   k_mesh's cell loop; every edge a triangle uses sets one bit of a per-unit bitmap, 3 axes x 64^3 bits, at the edge's
//                          OWNER voxel L (which may lie in the +x / +y / +z neighbour unit: it exists, the cell is valid).  Row (unit, i, j) of
//                          the bitmap = three 64-bit masks over k.  The wave gathers the bits of a row of cells with one ballot per cell edge
//                          and lane 0 ORs the row masks in with 32-bit atomicOr: OR commutes, so the bitmap does not depend on who runs when.
//                          Counts the slab's triangles as k_mesh's pass 0 does.
//   k_mesh_rows            one wave per slab, lane = j: the popcount of the row's three masks and its exclusive prefix inside the slab.
//   k_mesh_verts           one wave per slab, lane = k: the vertex of bit (row, axis, k) goes to
//                              slab offset + row prefix + popc(the three masks below k) + (set bits of the lower axes at k)
//                          with k_mesh's own position expression, from the two sdf values the lane reads itself.
//   k_mesh_index, pass 1   the cell loop again, writing at k_mesh's slab offsets: a triangle corner's index is the same sum, read from the
//                          owner's row.  A row of cells touches four rows of the bitmap (i, i + 1) x (j, j + 1), the same for all 64 lanes --
//                          wave-uniform loads, once per row of cells -- and lane 63 alone four more in the +z unit.
// The bitmap is 96 KiB per unit, the row prefixes 16 KiB.

// ORs a row mask into bitmap row (unit of rank r, i, j), axis: two 32-bit words (little endian: word 0 = k 0 .. 31)
__device__ __forceinline__ void mark_row(unsigned long long* __restrict__ bm, int r, int i, int j, int axis, unsigned long long m) {
  if (r < 0) return;                           // (no such unit: cannot be the owner of an edge of a valid cell)
  unsigned* w = reinterpret_cast<unsigned*>(bm + ((size_t)r * 4096 + (size_t)i * 64 + j) * 3 + axis);
  const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
  if (lo) atomicOr(w, lo);
  if (hi) atomicOr(w + 1, hi);
}

__global__ __launch_bounds__(64) void k_mesh_index(VolumeView vol, const int* __restrict__ slots, const int* __restrict__ keys,
                                                   const unsigned char* __restrict__ table, const int* __restrict__ slot_rank,
                                                   unsigned long long* __restrict__ bm, const int* __restrict__ row_off,
                                                   const long* __restrict__ vslab_off, long* __restrict__ slab_count,
                                                   const long* __restrict__ slab_offset, int* __restrict__ out, int pass) {
  const Slab S(keys);
  const CellWalk<true> W(vol, S, slots[S.rank], table, slot_rank);
  const int lane = S.lane;
  const unsigned long long lt = (1ull << lane) - 1ull;
  long base = pass ? slab_offset[blockIdx.x] : 0;
  long total = 0;
  for (int j = 0; j < 64; j++) {
    float2 f[8];
    const unsigned char* row;
    const int nt = W.cell(j, f, row);
    const int incl = wave_inclusive_sum(nt, lane);       // (k order)
    const int wave_total = __shfl(incl, 63);
    total += wave_total;
    if (wave_total == 0) continue;             // (wave-uniform)
    if (!pass) {
      // the cell edges this lane's triangles use: bit e = edge id e of the table
      unsigned used = 0;
      for (int t = 0; t < 3 * nt; t++) used |= 1u << row[t];
#pragma unroll
      for (int e = 0; e < 12; e++) {
        const unsigned long long m = __ballot((used >> e) & 1u);
        if (m == 0 || lane != 0) continue;
        const CellEdge E(e);
        const int jb = (j + E.b0) & 63, u = W.unit_at(E.a0, j + E.b0);
        // owner voxel (i + a0, j + b0, k + c0): bit k + c0 of its row; k + c0 == 64 is voxel 0 of the row in the +z unit
        mark_row(bm, W.rank_at(u), W.ia[E.a0], jb, E.axis, E.c0 ? m << 1 : m);
        if (E.c0 && (m >> 63)) mark_row(bm, W.rank_at(u | 1), W.ia[E.a0], jb, E.axis, 1ull);
      }
      continue;
    }
    // pass 1.  Per corner cl = a | b << 1 | c << 2 of the cell, for the edges that START there: P = index of the first vertex of that
    // voxel, B = which of its x (bit 0) and y (bit 1) edges are vertices -- the index of (voxel, axis) is P + the set bits of the lower axes.
    int P[8], B[8];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int jb = (j + b) & 63, ia = W.ia[a];
        const int r0 = W.rank_at(W.unit_at(a, j + b)), r1 = W.rank_at(W.unit_at(a, j + b) | 1);
        unsigned long long mx = 0, my = 0, mz = 0;
        int rb = 0;
        if (r0 >= 0) {                         // (wave-uniform: one fetch of the row serves all 64 lanes)
          const size_t r = (size_t)r0 * 4096 + (size_t)ia * 64 + jb;
          mx = bm[r * 3];
          my = bm[r * 3 + 1];
          mz = bm[r * 3 + 2];
          rb = (int)vslab_off[r0 * 64 + ia] + row_off[r];
        }
        const int c = a | b << 1;
        P[c] = rb + __popcll(mx & lt) + __popcll(my & lt) + __popcll(mz & lt);
        B[c] = (int)((mx >> lane) & 1ull) | (int)((my >> lane) & 1ull) << 1;
        // k + 1: the same row one bit up; for lane 63 voxel 0 of the row in the +z unit
        const int k1 = (lane + 1) & 63;
        const unsigned long long lt1 = (lt << 1) | 1ull;
        int p1 = rb + __popcll(mx & lt1) + __popcll(my & lt1) + __popcll(mz & lt1);
        int q1 = (int)((mx >> k1) & 1ull) | (int)((my >> k1) & 1ull) << 1;
        if (lane == 63) {
          p1 = q1 = 0;
          if (r1 >= 0) {
            const size_t r = (size_t)r1 * 4096 + (size_t)ia * 64 + jb;
            p1 = (int)vslab_off[r1 * 64 + ia] + row_off[r];
            q1 = (int)(bm[r * 3] & 1ull) | (int)(bm[r * 3 + 1] & 1ull) << 1;
          }
        }
        P[c | 4] = p1;
        B[c | 4] = q1;
      }
    if (nt > 0) {
      int* __restrict__ o = out + (size_t)(base + (total - wave_total) + (incl - nt)) * 3;
      for (int t = 0; t < 3 * nt; t++) {
        const CellEdge E(row[t]);
        const int bits = ER_PICK8(B, E.corner());
        o[t] = ER_PICK8(P, E.corner()) + (E.axis > 0 ? bits & 1 : 0) + (E.axis > 1 ? bits >> 1 : 0);
      }
    }
  }
  if (!pass && lane == 0) slab_count[blockIdx.x] = total;
}

#undef ER_PICK8

// One wave per slab, lane = j: vertices of row (unit, i, j) and their exclusive prefix inside the slab (at most 64 * 192: an int).
__global__ __launch_bounds__(64) void k_mesh_rows(const unsigned long long* __restrict__ bm, int* __restrict__ row_off, long* __restrict__ vslab_count) {
  const int lane = threadIdx.x;
  const size_t r = (size_t)blockIdx.x * 64 + lane;
  const int c = __popcll(bm[r * 3]) + __popcll(bm[r * 3 + 1]) + __popcll(bm[r * 3 + 2]);
  const int incl = wave_inclusive_sum(c, lane);
  row_off[r] = incl - c;
  if (lane == 63) vslab_count[blockIdx.x] = incl;
}

// One wave per slab, lane = k: the vertices of the slab's marked edges, float4 = x y z axis like k_surface's points, the position by k_mesh's
// expression pos(L) + (F_L / (F_L - F_H)) * voxel size.  The upper voxel H exists wherever a bit is set (the cell that set it was valid).
__global__ __launch_bounds__(64) void k_mesh_verts(VolumeView vol, const int* __restrict__ slots, const int* __restrict__ keys,
                                                   const unsigned long long* __restrict__ bm, const int* __restrict__ row_off,
                                                   const long* __restrict__ vslab_off, float4* __restrict__ out) {
  const Slab S(keys);
  const SlabVoxels V(vol, S, slots[S.rank]);
  const int lane = S.lane;
  const float gx = S.x(), gz = S.z();
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long base = vslab_off[blockIdx.x];
  for (int j = 0; j < 64; j++) {
    const size_t r = (size_t)blockIdx.x * 64 + j;
    const unsigned long long mx = bm[r * 3], my = bm[r * 3 + 1], mz = bm[r * 3 + 2];
    if ((mx | my | mz) == 0) continue;         // (wave-uniform)
    const float2 v = V.at(j);
    const float nz = V.up_z(j, v).x;
    const bool cx = (mx >> lane) & 1ull, cy = (my >> lane) & 1ull, cz = (mz >> lane) & 1ull;
    long o = base + row_off[r] + __popcll(mx & lt) + __popcll(my & lt) + __popcll(mz & lt);
    const float gy = S.y(j);
    if (cx) out[o++] = edge_point(gx, gy, gz, 0, v.x, V.up_x(j).x);
    if (cy) out[o++] = edge_point(gx, gy, gz, 1, v.x, V.up_y(j).x);
    if (cz) out[o++] = edge_point(gx, gy, gz, 2, v.x, nz);
  }
}

// SaveWorld's inverse (er_tsdf_import_world): one thread per row x y z intensity of er_tsdf_extract_world's layout -- the host has checked that
// the coordinates are integers on the lattice and has created the row's unit -- stores (intensity, 1) in its voxel, one 8-byte vector store.
// The units were (+0, 0) everywhere, so afterwards the weights sum to the number of DISTINCT voxels listed: to the number of rows iff no
// voxel is listed twice.  (Adding 1 to the weight instead would not tell: that sum is the number of rows whatever they name.)
__global__ __launch_bounds__(256) void k_import_world(float2* __restrict__ pool, UnitMap map, const float4* __restrict__ rows, long n) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float4 p = rows[r];
  const int gx = (int)p.x + 256 * 64, gy = (int)p.y + 256 * 64, gz = (int)p.z + 256 * 64;
  if (!on_lattice(gx, gy, gz)) return;                                                                   // (refused by the host)
  const int slot = map.slot(unit_key_of(gx, gy, gz));
  if (slot < 0) return;                                                                                  // (the pool is exhausted: refused by the host)
  pool[(size_t)slot * kUnitVox + unit_offset_of(gx, gy, gz)] = make_float2(p.w, 1.0f);
}

// The first of the two passes of one extraction call over the device temporaries of that call: they live in `scope`, the call's own (freed when
// the call leaves, whichever way) or the one of the DeviceMesh that the call fills, and so does what the caller adds (its output, a table).
// keys / slots: the units in ascending key order, on the host and (d_keys / d_slots) on the device; cnt() / off(): per slab (64 per unit, one block
// each) what the count pass found and where the write pass starts -- a list of `lists` (er_compact.h), which lives with the scope.  A call with
// n_lists = 2 compacts a second list over the same slabs (the indexed mesh's vertices), counted and uploaded with the first.
struct SlabPass {
  DevScope& scope;
  TwoPass& lists;
  std::vector<int> keys, slots;                // (the host side of count()'s two copies; count() returns only behind a synchronise)
  int n = 0, nslab = 0;
  int *d_keys = nullptr, *d_slots = nullptr;

  SlabPass(DevScope& s, TwoPass& l) : scope(s), lists(l) {}
  long* cnt(int list = 0) const { return lists.blk(list); }
  const long* off(int list = 0) const { return lists.off(list); }

  // Lists the units (sorted_units: behind every queued batch): -> n and nslab, 0 for an empty volume.
  int units(er_tsdf_t h) {
    if (sorted_units(h, keys, slots)) return 1;
    n = (int)keys.size();
    nslab = n * 64;
    return 0;
  }

  int alloc(const char* who, int n_lists = 1) {
    for (int l = 0; l < n_lists; l++) lists.add(nslab, 1);
    return scope.alloc(&d_keys, (size_t)n, who) || scope.alloc(&d_slots, (size_t)n, who) || lists.alloc(scope, who);
  }

  // Uploads the unit list, runs the caller's count launch (-> 0, or non-zero after reporting its failure), reads the slab counts back and
  // sums them on the host: -> *total (and lists.total(1)).  Synchronises h->stream, on the ways out that fail too: nothing reads keys / slots
  // or the count launch's own host arrays afterwards.
  template <typename Launch>
  int count(er_tsdf_t h, const char* who, Launch count_launch, long* total) {
    auto enqueue = [&] {
      ER_W(who, hipMemcpyAsync(d_keys, keys.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
      ER_W(who, hipMemcpyAsync(d_slots, slots.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
      return count_launch() || lists.read_counts(who, h->stream) ? 1 : 0;
    };
    const int rc = enqueue();
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (rc) return 1;
    ER_W(who, e);
    lists.prefix();
    *total = lists.total(0);
    return 0;
  }

  // (only once the caller knows that there is something to write and room for it, behind the allocation of its output)
  int upload_offsets(er_tsdf_t h, const char* who) { return lists.upload_offsets(who, h->stream); }
};

// An extraction call that copies ONE list back to the host -- SaveWorld's voxels, the zero crossings, the triangle soup: the units, the count pass,
// the refusal of a capacity that is too small (nothing has been written then), the write pass at the slabs' offsets, the copy back.  An element
// is `per` Ts, called `what` in the refusal; launch(t, d_tab, out, pass) enqueues the list's kernel and returns 0, or non-zero after reporting;
// d_tab is the marching-cubes case table on the device where `mc` asks for it.  Synchronises h->stream.
template <typename T, typename Launch>
int extract_list(er_tsdf_t h, const char* who, const char* what, bool mc, int per, T* out_host, long capacity, long* count, Launch launch) {
  if (!h || !count) return er::fail("%s: NULL argument", who);
  ER_HIP_TRY(hipSetDevice(h->device));
  TwoPass lists;                               // (in this frame, outliving `own`: the call synchronises before it returns)
  DevScope own;
  SlabPass t(own, lists);
  if (t.units(h)) return 1;
  *count = 0;
  if (t.n == 0) return 0;
  unsigned char* d_tab = nullptr;
  T* d_out = nullptr;
  long total = 0;
  if (t.alloc(who)) return 1;
  if (mc && own.alloc(&d_tab, 256 * 16, who)) return 1;
  auto count_launch = [&] {
    if (mc) ER_W(who, hipMemcpyAsync(d_tab, er::mc_table().tri, 256 * 16, hipMemcpyHostToDevice, h->stream));
    return launch(t, d_tab, (T*)nullptr, 0);
  };
  if (t.count(h, who, count_launch, &total)) return 1;
  *count = total;
  if (out_host && total > 0) {
    if (capacity < total) return er::fail("%s: capacity %ld < %ld %s", who, capacity, total, what);
    if (own.alloc(&d_out, (size_t)total * per, who)) return 1;
    if (t.upload_offsets(h, who) || launch(t, d_tab, d_out, 1)) return 1;
    ER_W(who, hipMemcpyAsync(out_host, d_out, (size_t)total * per * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    ER_W(who, hipStreamSynchronize(h->stream));
  }
  return 0;
}

int extract_points(er_tsdf_t h, float* out_host, long capacity, long* count, int surface) {
  const char* who = "er_tsdf_extract_world";
  return extract_list(h, who, "points", false, 1, reinterpret_cast<float4*>(out_host), capacity, count,
                      [&](const SlabPass& t, const unsigned char*, float4* out, int pass) {
                        if (surface)
                          hipLaunchKernelGGL(k_surface, dim3(t.nslab), dim3(64), 0, h->stream, h->view(), t.d_slots, t.d_keys, t.cnt(), t.off(), out, pass);
                        else
                          hipLaunchKernelGGL(k_world, dim3(t.nslab), dim3(64), 0, h->stream, h->pool, t.d_slots, t.d_keys, t.cnt(), t.off(), out, pass);
                        ER_W(who, hipGetLastError());
                        return 0;
                      });
}

// The oriented list on the device: *d_pts / *d_nrm are arrays of *total float4 that belong to t (both NULL when the list is empty or
// want == false, which only counts).  k_surface's two passes, then k_surface_normals.  Synchronises h->stream.
int oriented_on_device(er_tsdf_t h, const char* who, bool want, SlabPass& t, float4** d_pts, float4** d_nrm, long* total_out) {
  *d_pts = *d_nrm = nullptr;
  *total_out = 0;
  if (t.units(h)) return 1;
  if (t.n == 0) return 0;
  long total = 0;
  auto launch = [&](float4* out, int pass) {
    hipLaunchKernelGGL(k_surface, dim3(t.nslab), dim3(64), 0, h->stream, h->view(), t.d_slots, t.d_keys, t.cnt(), t.off(), out, pass);
    ER_W(who, hipGetLastError());
    return 0;
  };
  if (t.alloc(who) || t.count(h, who, [&] { return launch(nullptr, 0); }, &total)) return 1;
  *total_out = total;
  if (want && total > 0) {
    if (t.scope.alloc(d_pts, (size_t)total, who)) return 1;
    if (t.scope.alloc(d_nrm, (size_t)total, who)) return 1;
    if (t.upload_offsets(h, who) || launch(*d_pts, 1)) return 1;
    hipLaunchKernelGGL(k_surface_normals, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->view(), *d_pts, total, *d_nrm);
    ER_W(who, hipGetLastError());
    ER_W(who, hipStreamSynchronize(h->stream));
  }
  return 0;
}

}  // namespace

extern "C" {

int er_tsdf_extract_world(er_tsdf_t h, float* out_host, long capacity, long* count) { return extract_points(h, out_host, capacity, count, 0); }
int er_tsdf_extract_surface(er_tsdf_t h, float* out_host, long capacity, long* count) { return extract_points(h, out_host, capacity, count, 1); }

int er_tsdf_extract_oriented(er_tsdf_t h, float* points_host, float* normals_host, long capacity, long* count) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_tsdf_extract_oriented: no HIP device available (liber_hip has no CPU fallback)");
  if (!h || !count) return er::fail("er_tsdf_extract_oriented: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  const bool want = points_host && normals_host;
  TwoPass lists;                               // (in this frame, outliving `own`: the call synchronises before it returns)
  DevScope own;
  SlabPass t(own, lists);
  float4 *d_pts = nullptr, *d_nrm = nullptr;
  *count = 0;
  if (oriented_on_device(h, "er_tsdf_extract_oriented", want, t, &d_pts, &d_nrm, count)) return 1;
  if (want && capacity < *count)
    return er::fail("er_tsdf_extract_oriented: capacity %ld < %ld points", capacity, *count);   // (nothing has been written to the host)
  if (want && *count > 0) {
    hipError_t e = hipMemcpyAsync(points_host, d_pts, (size_t)*count * sizeof(float4), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(normals_host, d_nrm, (size_t)*count * sizeof(float4), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return er::fail("er_tsdf_extract_oriented: copy back failed: %s", hipGetErrorString(e));
  }
  return 0;
}

int er_cloud_create_from_tsdf(er_tsdf_t h, float cube_length, float grid_cell, er_cloud_t* out, int* n_points) {
  const char* who = "er_cloud_create_from_tsdf";
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_cloud_create_from_tsdf: no HIP device available (liber_hip has no CPU fallback)");
  if (!h || !out) return er::fail("er_cloud_create_from_tsdf: NULL argument");
  *out = nullptr;
  if (n_points) *n_points = 0;
  if (!(grid_cell > 0.f)) return er::fail("er_cloud_create_from_tsdf: grid_cell must be positive");
  ER_HIP_TRY(hipSetDevice(h->device));
  TwoPass lists, rows;                         // the slabs of the oriented list, then its rows (in this frame, outliving `own`: as above)
  DevScope own;
  SlabPass t(own, lists);
  float4 *d_pts = nullptr, *d_nrm = nullptr;
  long total = 0, kept = 0;
  if (oriented_on_device(h, who, true, t, &d_pts, &d_nrm, &total)) return 1;
  float* d_rows = nullptr;        // [kept][3] coordinates, then [kept][3] normals
  const long nblk = (total + 63) / 64;
  if (total > 0) {
    const int lk = rows.add(nblk, 1);
    if (rows.alloc(t.scope, who)) return 1;
    auto keep = [&](int pass) {
      hipLaunchKernelGGL(k_oriented_keep, dim3((unsigned)nblk), dim3(64), 0, h->stream, d_pts, d_nrm, total, cube_length, rows.blk(lk), rows.off(lk),
                         d_rows, d_rows + (size_t)kept * 3, pass);
      ER_W(who, hipGetLastError());
      return 0;
    };
    if (keep(0) || rows.read_counts(who, h->stream)) return 1;
    ER_W(who, hipStreamSynchronize(h->stream));
    rows.prefix();
    kept = rows.total(lk);
    if (kept >= (1L << 27))
      return er::fail("er_cloud_create_from_tsdf: %ld points; the limit is 2^27 - 1 (32-bit byte offsets in the search kernels)", kept);
    if (kept > 0) {
      if (t.scope.alloc(&d_rows, (size_t)kept * 6, who)) return 1;
      if (rows.upload_offsets(who, h->stream) || keep(1)) return 1;
      ER_W(who, hipStreamSynchronize(h->stream));     // the cloud builder works on streams of its own: the rows are complete before it starts
    }
  }
  const int rc = er::cloud_create_device(d_rows, d_rows ? d_rows + (size_t)kept * 3 : nullptr, (int)kept, grid_cell, h->device, out);
  if (rc == 0 && n_points) *n_points = (int)kept;
  return rc;
}

int er_mc_table(unsigned char out[256 * 16]) {
  if (!out) return er::fail("er_mc_table: NULL argument");
  memcpy(out, er::mc_table().tri, 256 * 16);
  return 0;
}

int er_tsdf_extract_mesh(er_tsdf_t h, float* tri_host, long capacity_triangles, long* n_triangles) {
  const char* who = "er_tsdf_extract_mesh";
  return extract_list(h, who, "triangles", true, 9, tri_host, capacity_triangles, n_triangles,
                      [&](const SlabPass& t, const unsigned char* d_tab, float* out, int pass) {
                        hipLaunchKernelGGL(k_mesh, dim3(t.nslab), dim3(64), 0, h->stream, h->view(), t.d_slots, t.d_keys, d_tab, t.cnt(), t.off(), out, pass);
                        ER_W(who, hipGetLastError());
                        return 0;
                      });
}

int er_tsdf_extract_mesh_indexed(er_tsdf_t h, float* verts_host, float* normals_host, long capacity_vertices, int* tri_host,
                                 long capacity_triangles, long* n_vertices, long* n_triangles) {
  const char* who = "er_tsdf_extract_mesh_indexed";
  if (!h || !n_vertices || !n_triangles) return er::fail("er_tsdf_extract_mesh_indexed: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  const bool want_v = verts_host || normals_host;
  DeviceMesh m;
  auto counted = [&](long nv, long ntri) {
    if (nv > (long)INT_MAX) return er::fail("er_tsdf_extract_mesh_indexed: %ld vertices; the limit is 2^31 - 1 (int32 indices)", nv);
    if (want_v && capacity_vertices < nv) return er::fail("er_tsdf_extract_mesh_indexed: capacity %ld < %ld vertices", capacity_vertices, nv);
    if (tri_host && capacity_triangles < ntri) return er::fail("er_tsdf_extract_mesh_indexed: capacity %ld < %ld triangles", capacity_triangles, ntri);
    return 0;                                                // (nothing has been written to the host)
  };
  if (mesh_indexed_on_device(h, who, want_v, normals_host != nullptr, tri_host != nullptr, n_vertices, n_triangles, counted, &m)) return 1;
  if (m.d_verts && verts_host) ER_W(who, hipMemcpyAsync(verts_host, m.d_verts, (size_t)m.nv * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  if (m.d_nrm) ER_W(who, hipMemcpyAsync(normals_host, m.d_nrm, (size_t)m.nv * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  if (m.d_tri) ER_W(who, hipMemcpyAsync(tri_host, m.d_tri, (size_t)m.ntri * 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (m.d_verts || m.d_tri) ER_W(who, hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"

// The indexed mesh left ON THE DEVICE (er_tsdf.h): the body of er_tsdf_extract_mesh_indexed, which copies the three arrays back, and the
// first stage of er_tsdf_extract_mesh_cleaned (er_mesh_cc.hip), which goes on working on them in HBM.
int er_tsdf_k::mesh_indexed_on_device(er_tsdf_t h, const char* who, bool want_v, bool want_n, bool want_t,
                                      long* n_vertices, long* n_triangles, const std::function<int(long, long)>& counted, DeviceMesh* m) {
  SlabPass t(m->owned, m->lists);         // every temporary belongs to the caller's mesh: the kernels that read them are in flight on return
  if (t.units(h)) return 1;
  *n_vertices = *n_triangles = 0;
  if (t.n == 0) return 0;                                   // (an empty volume: 0 and 0)
  const int nslab = t.nslab;
  const size_t nrow = (size_t)nslab * 64;
  unsigned char* d_tab = nullptr;
  unsigned long long* d_bm = nullptr;     // [row][axis]: the edge bitmap
  int *d_rank = nullptr, *d_rowoff = nullptr;
  std::vector<int> rank((size_t)h->max_units, -1);           // pool slot -> position in the key order; -1: a dropped unit's slot
  for (int r = 0; r < t.n; r++) rank[(size_t)t.slots[(size_t)r]] = r;
  long ntri = 0, nv = 0;
  auto launch = [&](int* out, int pass) {
    hipLaunchKernelGGL(k_mesh_index, dim3(nslab), dim3(64), 0, h->stream, h->view(), t.d_slots, t.d_keys, d_tab, d_rank, d_bm, d_rowoff, t.off(1), t.cnt(),
                       t.off(), out, pass);
    ER_W(who, hipGetLastError());
    return 0;
  };
  if (t.alloc(who, 2)) return 1;                             // (the second list: the vertices of a slab)
  if (t.scope.alloc(&d_tab, 256 * 16, who)) return 1;
  if (t.scope.alloc(&d_bm, nrow * 3, who)) return 1;
  if (t.scope.alloc(&d_rank, rank.size(), who)) return 1;
  if (t.scope.alloc(&d_rowoff, nrow, who)) return 1;
  auto count_launch = [&] {
    ER_W(who, hipMemcpyAsync(d_tab, er::mc_table().tri, 256 * 16, hipMemcpyHostToDevice, h->stream));
    ER_W(who, hipMemcpyAsync(d_rank, rank.data(), rank.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    ER_W(who, hipMemsetAsync(d_bm, 0, nrow * 3 * sizeof(unsigned long long), h->stream));
    if (launch(nullptr, 0)) return 1;                        // marks the bitmap, counts the triangles
    hipLaunchKernelGGL(k_mesh_rows, dim3(nslab), dim3(64), 0, h->stream, d_bm, d_rowoff, t.cnt(1));
    ER_W(who, hipGetLastError());
    return 0;
  };
  if (t.count(h, who, count_launch, &ntri)) return 1;
  nv = t.lists.total(1);
  *n_vertices = m->nv = nv;
  *n_triangles = m->ntri = ntri;
  if (counted(nv, ntri)) return 1;
  if (nv == 0 || (!want_v && !want_t)) return 0;
  if (t.upload_offsets(h, who)) return 1;                    // (of both lists)
  if (want_v) {
    if (t.scope.alloc(&m->d_verts, (size_t)nv, who)) return 1;
    hipLaunchKernelGGL(k_mesh_verts, dim3(nslab), dim3(64), 0, h->stream, h->view(), t.d_slots, t.d_keys, d_bm, d_rowoff, t.off(1), m->d_verts);
    ER_W(who, hipGetLastError());
    if (want_n) {
      if (t.scope.alloc(&m->d_nrm, (size_t)nv, who)) return 1;
      hipLaunchKernelGGL(k_surface_normals, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, h->stream, h->view(), m->d_verts, nv, m->d_nrm);
      ER_W(who, hipGetLastError());
    }
  }
  if (want_t) {
    if (t.scope.alloc(&m->d_tri, (size_t)ntri * 3, who)) return 1;
    if (launch(m->d_tri, 1)) return 1;
  }
  return 0;                                                  // (the kernels are still in flight on h->stream: what they read or write is m's)
}

extern "C" {

int er_tsdf_import_world(er_tsdf_t h, const float* xyzi_host, long n, int* n_units) {
  const char* who = "er_tsdf_import_world";
  if (!h || (n > 0 && !xyzi_host)) return er::fail("er_tsdf_import_world: NULL argument");
  if (n_units) *n_units = 0;
  if (n < 0) return er::fail("er_tsdf_import_world: n = %ld", n);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (check_flags(h)) return 1;
  int held = 0;
  ER_W(who, hipMemcpy(&held, h->counters + C_NUNITS, sizeof(int), hipMemcpyDeviceToHost));
  if (held != 0) {
    (void)er_tsdf_reset(h);
    return er::fail("er_tsdf_import_world: the volume already holds %d units (er_tsdf_reset it first); it is empty now", held);
  }
  // the rows, in order: the first one that cannot be a voxel is named
  std::vector<int> ukeys;
  int last = -1;
  for (long r = 0; r < n; r++) {
    const float* p = xyzi_host + 4 * r;
    int g[3];
    for (int a = 0; a < 3; a++) {
      const float c = p[a];
      if (!(c >= -16384.0f && c <= 16383.0f) || c != std::floor(c))
        return er::fail("er_tsdf_import_world: row %ld: %c = %.9g is not a voxel index of the 512-unit lattice (an integer in -16384 .. 16383)", r,
                        "xyz"[a], (double)c);
      g[a] = (int)c + 256 * 64;
    }
    if (p[3] != p[3]) return er::fail("er_tsdf_import_world: row %ld: the intensity is NaN", r);
    const int key = unit_key_of(g[0], g[1], g[2]);
    if (key != last) ukeys.push_back(last = key);
  }
  std::sort(ukeys.begin(), ukeys.end());
  ukeys.erase(std::unique(ukeys.begin(), ukeys.end()), ukeys.end());
  if ((long)ukeys.size() > (long)h->max_units)
    return er::fail("er_tsdf_import_world: the list needs %ld units, max_units is %d", (long)ukeys.size(), h->max_units);
  if (n == 0) return 0;
  // From here on a failure leaves units behind: every exit but the last resets the volume.
  struct Undo {
    er_tsdf_t h;
    bool armed = true;
    ~Undo() { if (armed) (void)er_tsdf_reset(h); }
  } undo{h};
  DevScope own;
  const long chunk = std::min<long>(n, 1L << 22);            // 64 MiB of rows at a time
  float4* d_rows = nullptr;                                  // the staging buffer
  if (own.alloc(&d_rows, (size_t)chunk, who)) return 1;
  // the units: fresh ones of an empty volume are (+0, 0) everywhere (er_tsdf_create, er_tsdf_reset)
  if (resolve_slots(h, ukeys.data(), (int)ukeys.size(), true) || check_flags(h)) return 1;
  for (long r0 = 0; r0 < n; r0 += chunk) {
    const long m = std::min(chunk, n - r0);
    ER_W(who, hipMemcpyAsync(d_rows, xyzi_host + 4 * r0, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_import_world, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, h->pool, h->view().map, d_rows, m);
    ER_W(who, hipGetLastError());
    ER_W(who, hipStreamSynchronize(h->stream));             // (the host rows may be pageable, the staging buffer is reused)
  }
  double sum = 0.0;
  if (er_tsdf_sum_weight(h, &sum)) return 1;
  if (sum != (double)n) {
    // fewer distinct voxels than rows: one is listed twice.  The slow way to the FIRST row that repeats an earlier one:
    std::vector<std::pair<long long, long>> id((size_t)n);
    for (long r = 0; r < n; r++) {
      const float* p = xyzi_host + 4 * r;
      id[(size_t)r] = std::make_pair(((long long)((int)p[0] + 16384) << 30) | ((long long)((int)p[1] + 16384) << 15) | (long long)((int)p[2] + 16384), r);
    }
    std::sort(id.begin(), id.end());
    long first = -1, of = -1;
    for (long q = 1; q < n; q++)
      if (id[(size_t)q].first == id[(size_t)q - 1].first && (first < 0 || id[(size_t)q].second < first)) {
        first = id[(size_t)q].second;
        of = id[(size_t)q - 1].second;
      }
    if (first < 0) return er::fail("er_tsdf_import_world: the weights sum to %.17g, not to the %ld rows", sum, n);
    const float* p = xyzi_host + 4 * first;
    return er::fail("er_tsdf_import_world: row %ld lists voxel (%d, %d, %d) again (row %ld has it already)", first, (int)p[0], (int)p[1], (int)p[2], of);
  }
  undo.armed = false;
  if (n_units) *n_units = (int)ukeys.size();
  return 0;
}

}  // extern "C"
