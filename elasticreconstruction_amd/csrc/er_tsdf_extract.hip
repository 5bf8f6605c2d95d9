// er_tsdf_extract.hip -- what leaves the resident TSDF volume of path A (er_tsdf.hip): SaveWorld's voxel list, the zero crossings with and without
// normals, the oriented cloud handed to path B on the device, and the marching-cubes mesh.  Every kernel here makes two passes over the slabs
// (64 per unit) of the units in ascending key order -- count, then write at the slab's offset -- so the lists are reproducible element for element.
#include "er_tsdf_dev.h"
#include "er_mc_table.h"

namespace {

using namespace er_tsdf_k;

// SaveWorld's filter (TSDFVolume.cpp:118).  One wave per (unit, i-slab); pass 0 counts, pass 1 writes
// the points in i,j,k order at the slab's offset (stable compaction by ballot prefix).
__device__ __forceinline__ bool world_keep(float2 v) { return v.y != 0.0f && v.x < 0.98f && v.x >= -0.98f; }

__global__ __launch_bounds__(64) void k_world(const float2* __restrict__ pool, const int* __restrict__ slots,
                                              const int* __restrict__ keys, long* __restrict__ slab_count,
                                              const long* __restrict__ slab_offset, float4* __restrict__ out, int pass) {
  const int rank = blockIdx.x >> 6;          // unit in ascending key order
  const int i = blockIdx.x & 63;
  const int lane = threadIdx.x;
  const float2* slab = pool + (size_t)slots[rank] * kUnitVox + (size_t)i * 4096;
  const int key = keys[rank];
  const int xi = key >> 18, yi = (key >> 9) & 511, zi = key & 511;
  long base = pass ? slab_offset[blockIdx.x] : 0;
  long total = 0;
  for (int j = 0; j < 64; j++) {
    const float2 v = slab[j * 64 + lane];
    const bool keep = world_keep(v);
    const unsigned long long b = __ballot(keep);
    if (pass && keep) {
      const long o = base + total + __popcll(b & ((1ull << lane) - 1ull));
      out[o] = make_float4((float)(i + (xi - 256) * 64), (float)(j + (yi - 256) * 64), (float)(lane + (zi - 256) * 64), v.x);
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

__global__ __launch_bounds__(64) void k_surface(const float2* __restrict__ pool, const int* __restrict__ slots, const int* __restrict__ keys,
                                                const int* __restrict__ ht_key, const int* __restrict__ ht_slot, int cap_mask, int shift,
                                                long* __restrict__ slab_count, const long* __restrict__ slab_offset,
                                                float4* __restrict__ out, int pass) {
  const int rank = blockIdx.x >> 6;          // unit in ascending key order
  const int i = blockIdx.x & 63;
  const int lane = threadIdx.x;              // = k
  const int key = keys[rank];
  const int xi = key >> 18, yi = (key >> 9) & 511, zi = key & 511;
  const float2* unit = pool + (size_t)slots[rank] * kUnitVox;
  const float2* slab = unit + (size_t)i * 4096;
  // neighbours that live in adjacent units (wave-uniform lookups; -1 = that unit does not exist)
  const int sx = (i == 63 && xi < 511) ? ht_lookup_slot(ht_key, ht_slot, cap_mask, shift, key + 512 * 512) : -1;
  const int sy = yi < 511 ? ht_lookup_slot(ht_key, ht_slot, cap_mask, shift, key + 512) : -1;
  const int sz = zi < 511 ? ht_lookup_slot(ht_key, ht_slot, cap_mask, shift, key + 1) : -1;
  const float2 none = make_float2(0.0f, 0.0f);
  const float2* slab_x = i < 63 ? slab + 4096 : (sx >= 0 ? pool + (size_t)sx * kUnitVox : nullptr);              // i + 1 (slab 0 of the next unit)
  const float2* unit_y = sy >= 0 ? pool + (size_t)sy * kUnitVox + (size_t)i * 4096 : nullptr;                      // j + 1 == 64: row 0 there
  const float2* unit_z = sz >= 0 ? pool + (size_t)sz * kUnitVox + (size_t)i * 4096 : nullptr;                      // k + 1 == 64: voxel 0 there
  const float ulf = (float)kUnitLength;
  const float gx = (float)((double)(i + (xi - 256) * 64) * kUnitLength);
  const float gz = (float)((double)(lane + (zi - 256) * 64) * kUnitLength);
  const unsigned long long lt = (1ull << lane) - 1ull;
  long base = pass ? slab_offset[blockIdx.x] : 0;
  long total = 0;
  for (int j = 0; j < 64; j++) {
    const float2 v = slab[j * 64 + lane];
    const float2 nx = slab_x ? slab_x[j * 64 + lane] : none;
    const float2 ny = j < 63 ? slab[(j + 1) * 64 + lane] : (unit_y ? unit_y[lane] : none);
    float2 nz;
    nz.x = __shfl_down(v.x, 1);
    nz.y = __shfl_down(v.y, 1);
    if (lane == 63) nz = unit_z ? unit_z[j * 64] : none;
    const bool cx = crosses(v, nx), cy = crosses(v, ny), cz = crosses(v, nz);
    const unsigned long long bx = __ballot(cx), by = __ballot(cy), bz = __ballot(cz);
    if (pass) {
      long o = base + total + __popcll(bx & lt) + __popcll(by & lt) + __popcll(bz & lt);
      const float gy = (float)((double)(j + (yi - 256) * 64) * kUnitLength);
      if (cx) out[o++] = make_float4(gx + (v.x / (v.x - nx.x)) * ulf, gy, gz, 0.0f);
      if (cy) out[o++] = make_float4(gx, gy + (v.x / (v.x - ny.x)) * ulf, gz, 1.0f);
      if (cz) out[o++] = make_float4(gx, gy, gz + (v.x / (v.x - nz.x)) * ulf, 2.0f);
    }
    total += __popcll(bx) + __popcll(by) + __popcll(bz);
  }
  if (!pass && lane == 0) slab_count[blockIdx.x] = total;
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
__device__ __forceinline__ float2 fetch_voxel(const float2* __restrict__ pool, const float2* __restrict__ unit, int key, const int* __restrict__ ht_key,
                                              const int* __restrict__ ht_slot, int cap_mask, int shift, int gx, int gy, int gz) {
  if ((unsigned)gx >= 512u * 64u || (unsigned)gy >= 512u * 64u || (unsigned)gz >= 512u * 64u) return make_float2(0.0f, 0.0f);
  const int k = (gx >> 6) << 18 | (gy >> 6) << 9 | (gz >> 6);
  const size_t l = (size_t)(gx & 63) * 4096 + (size_t)(gy & 63) * 64 + (size_t)(gz & 63);
  if (k == key) return unit[l];
  const int s = ht_lookup_slot(ht_key, ht_slot, cap_mask, shift, k);
  return s >= 0 ? pool[(size_t)s * kUnitVox + l] : make_float2(0.0f, 0.0f);
}

// the nearest voxel's index: rint((double)p / unit length), round half to even, on the 0-based lattice
__device__ __forceinline__ int nearest_index(float p) { return (int)rint((double)p / kUnitLength) + 256 * 64; }

__global__ __launch_bounds__(256) void k_surface_normals(const float2* __restrict__ pool, const int* __restrict__ ht_key, const int* __restrict__ ht_slot,
                                                         int cap_mask, int shift, const float4* __restrict__ pts, long n, float4* __restrict__ out_n) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float4 p = pts[r];
  const int gx = nearest_index(p.x), gy = nearest_index(p.y), gz = nearest_index(p.z);
  // the unit of v: key -1 (matches no voxel) if v is outside the lattice or its unit does not exist -- the fetches then find that out themselves
  const bool in = (unsigned)gx < 512u * 64u && (unsigned)gy < 512u * 64u && (unsigned)gz < 512u * 64u;
  int key = in ? ((gx >> 6) << 18 | (gy >> 6) << 9 | (gz >> 6)) : -1;
  const int slot = in ? ht_lookup_slot(ht_key, ht_slot, cap_mask, shift, key) : -1;
  if (slot < 0) key = -1;
  const float2* unit = pool + (size_t)(slot < 0 ? 0 : slot) * kUnitVox;
#define ER_F(dx, dy, dz) fetch_voxel(pool, unit, key, ht_key, ht_slot, cap_mask, shift, gx + (dx), gy + (dy), gz + (dz))
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
// One wave per 64 rows, two passes (count, then write at the block's offset) like the extraction kernels.
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
    const size_t o = (size_t)(blk_offset[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull))) * 3;
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
__global__ __launch_bounds__(64) void k_mesh(const float2* __restrict__ pool, const int* __restrict__ slots, const int* __restrict__ keys,
                                             const int* __restrict__ ht_key, const int* __restrict__ ht_slot, int cap_mask, int shift,
                                             const unsigned char* __restrict__ table, long* __restrict__ slab_count,
                                             const long* __restrict__ slab_offset, float* __restrict__ out, int pass) {
  __shared__ unsigned char s_tab[256 * 16];
  for (int t = threadIdx.x; t < 256 * 16 / 4; t += 64) reinterpret_cast<unsigned*>(s_tab)[t] = reinterpret_cast<const unsigned*>(table)[t];
  __syncthreads();
  const int rank = blockIdx.x >> 6;          // unit in ascending key order
  const int i = blockIdx.x & 63;
  const int lane = threadIdx.x;              // = k
  const int key = keys[rank];
  const int xi = key >> 18, yi = (key >> 9) & 511, zi = key & 511;
  // the (up to) eight units a slab of cells can touch: [dx][dy][dz]; -1 = that unit does not exist (its voxels count as unobserved)
  int us[2][2][2];
  for (int dx = 0; dx < 2; dx++)
    for (int dy = 0; dy < 2; dy++)
      for (int dz = 0; dz < 2; dz++) {
        const bool need = (dx == 0 || i == 63);
        const bool ok = xi + dx < 512 && yi + dy < 512 && zi + dz < 512;
        us[dx][dy][dz] = (dx | dy | dz) == 0 ? slots[rank]
                         : (need && ok ? ht_lookup_slot(ht_key, ht_slot, cap_mask, shift, key + dx * 512 * 512 + dy * 512 + dz) : -1);
      }
  const int ia[2] = {i, i == 63 ? 0 : i + 1}, ux[2] = {0, i == 63 ? 1 : 0};      // slab index and unit offset of the two i layers
  const float2 none = make_float2(0.0f, 0.0f);
  const float ulf = (float)kUnitLength;
  const float gx = (float)((double)(i + (xi - 256) * 64) * kUnitLength);
  const float gz = (float)((double)(lane + (zi - 256) * 64) * kUnitLength);
  const unsigned long long lt = (1ull << lane) - 1ull;
  long base = pass ? slab_offset[blockIdx.x] : 0;
  long total = 0;
  for (int j = 0; j < 64; j++) {
    // the eight corners of this lane's cell: f[a][b][c] = voxel (i + a, j + b, k + c)
    float2 f[2][2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int jb = (j + b) & 63, uy = (j + b) >> 6;
        const int s0 = us[ux[a]][uy][0], s1 = us[ux[a]][uy][1];
        const size_t ro = (size_t)ia[a] * 4096 + (size_t)jb * 64;
        const float2 v = s0 >= 0 ? pool[(size_t)s0 * kUnitVox + ro + lane] : none;
        f[a][b][0] = v;
        float2 w;
        w.x = __shfl_down(v.x, 1);
        w.y = __shfl_down(v.y, 1);
        if (lane == 63) w = s1 >= 0 ? pool[(size_t)s1 * kUnitVox + ro] : none;
        f[a][b][1] = w;
      }
    bool valid = true;
    int cs = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const float2 v = f[c & 1][(c >> 1) & 1][c >> 2];
      valid = valid && v.y != 0.0f;
      cs |= (v.x < 0.0f ? 1 : 0) << c;
    }
    const unsigned char* __restrict__ row = s_tab + cs * 16;
    int nt = 0;
    if (valid)
      while (nt < 5 && row[3 * nt] != 255) nt++;
    // wave-level exclusive prefix of the triangle counts (k order)
    int incl = nt;
    for (int sft = 1; sft < 64; sft <<= 1) {
      const int t = __shfl_up(incl, sft);
      if (lane >= sft) incl += t;
    }
    const int wave_total = __shfl(incl, 63);
    if (pass && nt > 0) {
      const float gy = (float)((double)(j + (yi - 256) * 64) * kUnitLength);
      float* __restrict__ o = out + (size_t)(base + total + (incl - nt)) * 9;
      for (int t = 0; t < 3 * nt; t++) {
        const int e = row[t];
        const int axis = e >> 2, u = e & 1, v = (e >> 1) & 1;
        // lower corner of the edge (coordinate 0 along its axis) and the corner one step up the axis; the eight corner values sit
        // in registers, so they are picked with select chains, not with a runtime index (that would send them through scratch)
        const int a0 = axis == 0 ? 0 : u, b0 = axis == 1 ? 0 : (axis == 0 ? u : v), c0 = axis == 2 ? 0 : v;
        const int cl = a0 | b0 << 1 | c0 << 2, ch = cl | (1 << axis);
        float2 lo = none, hi = none;
#pragma unroll
        for (int c = 0; c < 8; c++) {
          const float2 fv = f[c & 1][(c >> 1) & 1][c >> 2];
          lo = c == cl ? fv : lo;
          hi = c == ch ? fv : hi;
        }
        const float tt = lo.x / (lo.x - hi.x);
        // lower end of the edge: lattice position of voxel (i + a0, j + b0, k + c0)
        float px = a0 ? (float)((double)(i + 1 + (xi - 256) * 64) * kUnitLength) : gx;
        float py = b0 ? (float)((double)(j + 1 + (yi - 256) * 64) * kUnitLength) : gy;
        float pz = c0 ? (float)((double)(lane + 1 + (zi - 256) * 64) * kUnitLength) : gz;
        if (axis == 0) px = px + tt * ulf;
        if (axis == 1) py = py + tt * ulf;
        if (axis == 2) pz = pz + tt * ulf;
        o[3 * t] = px;
        o[3 * t + 1] = py;
        o[3 * t + 2] = pz;
      }
    }
    total += wave_total;
  }
  (void)lt;
  if (!pass && lane == 0) slab_count[blockIdx.x] = total;
}

// One HIP call of an entry point: a failure is reported under the entry point's name and ends the function.
#define ER_W(who, expr)                                                                         \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return er::fail("%s: %s failed: %s", who, #expr, hipGetErrorString(e_)); \
  } while (0)
// hipMalloc of a device temporary that the call's SlabPass t frees: pp = the address of the caller's pointer.
#define ER_W_OWNED(who, t, pp, bytes)                 \
  do {                                                \
    ER_W(who, hipMalloc((void**)pp, bytes));          \
    (t).more.push_back(*(pp));                        \
  } while (0)

// The device temporaries of one extraction call, freed when the call leaves, whichever way, and the first of its two passes.
// d_keys / d_slots: the units in ascending key order; d_cnt / d_off: per slab (64 per unit) what the count pass found and where the write
// pass starts; more: what the caller adds with ER_W_OWNED (its output, a table).
struct SlabPass {
  int n = 0, nslab = 0;
  int *d_keys = nullptr, *d_slots = nullptr;
  long *d_cnt = nullptr, *d_off = nullptr;
  std::vector<long> off;                       // the offsets on the host (count)
  std::vector<void*> more;

  SlabPass() = default;
  SlabPass(const SlabPass&) = delete;
  SlabPass& operator=(const SlabPass&) = delete;
  ~SlabPass() {
    for (void* p : {(void*)d_keys, (void*)d_slots, (void*)d_cnt, (void*)d_off})
      if (p) (void)hipFree(p);
    for (void* p : more) (void)hipFree(p);
  }

  int alloc(const char* who, int n_units) {
    n = n_units;
    nslab = n * 64;
    ER_W(who, hipMalloc((void**)&d_keys, (size_t)n * sizeof(int)));
    ER_W(who, hipMalloc((void**)&d_slots, (size_t)n * sizeof(int)));
    ER_W(who, hipMalloc((void**)&d_cnt, (size_t)nslab * sizeof(long)));
    ER_W(who, hipMalloc((void**)&d_off, (size_t)nslab * sizeof(long)));
    return 0;
  }

  // Uploads the unit list, runs the caller's count launch (-> 0, or non-zero after reporting its failure), reads the slab counts back and
  // sums them on the host: -> *total, and `off` for upload_offsets.  Synchronises h->stream.
  template <typename Launch>
  int count(er_tsdf_t h, const char* who, const std::vector<int>& keys, const std::vector<int>& slots, Launch count_launch, long* total) {
    std::vector<long> cnt((size_t)nslab);
    ER_W(who, hipMemcpyAsync(d_keys, keys.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    ER_W(who, hipMemcpyAsync(d_slots, slots.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (count_launch()) return 1;
    ER_W(who, hipMemcpyAsync(cnt.data(), d_cnt, (size_t)nslab * sizeof(long), hipMemcpyDeviceToHost, h->stream));
    ER_W(who, hipStreamSynchronize(h->stream));
    off.resize((size_t)nslab);
    *total = 0;
    for (int s = 0; s < nslab; s++) {
      off[(size_t)s] = *total;
      *total += cnt[(size_t)s];
    }
    return 0;
  }

  // (only once the caller knows that there is something to write and room for it, behind the allocation of its output)
  int upload_offsets(er_tsdf_t h, const char* who) {
    ER_W(who, hipMemcpyAsync(d_off, off.data(), (size_t)nslab * sizeof(long), hipMemcpyHostToDevice, h->stream));
    return 0;
  }
};

int extract_points(er_tsdf_t h, float* out_host, long capacity, long* count, int surface) {
  const char* who = "er_tsdf_extract_world";
  if (!h || !count) return er::fail("er_tsdf_extract_world: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  std::vector<int> keys, slots;
  if (sorted_units(h, keys, slots)) return 1;
  const int n = (int)keys.size();
  *count = 0;
  if (n == 0) return 0;
  const int nslab = n * 64;
  SlabPass t;
  float4* d_out = nullptr;
  long total = 0;
  auto launch = [&](float4* out, int pass) {
    if (surface)
      hipLaunchKernelGGL(k_surface, dim3(nslab), dim3(64), 0, h->stream, h->pool, t.d_slots, t.d_keys, h->ht_key, h->ht_slot, h->ht_cap - 1, h->ht_shift,
                         t.d_cnt, t.d_off, out, pass);
    else
      hipLaunchKernelGGL(k_world, dim3(nslab), dim3(64), 0, h->stream, h->pool, t.d_slots, t.d_keys, t.d_cnt, t.d_off, out, pass);
    ER_W(who, hipGetLastError());
    return 0;
  };
  if (t.alloc(who, n) || t.count(h, who, keys, slots, [&] { return launch(nullptr, 0); }, &total)) return 1;
  *count = total;
  if (out_host && total > 0) {
    if (capacity < total) return er::fail("er_tsdf_extract_world: capacity %ld < %ld points", capacity, total);
    ER_W_OWNED(who, t, &d_out, (size_t)total * sizeof(float4));
    if (t.upload_offsets(h, who) || launch(d_out, 1)) return 1;
    ER_W(who, hipMemcpyAsync(out_host, d_out, (size_t)total * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    ER_W(who, hipStreamSynchronize(h->stream));
  }
  return 0;
}

// The oriented list on the device: *d_pts / *d_nrm are arrays of *total float4 that belong to t (both NULL when the list is empty or
// want == false, which only counts).  k_surface's two passes, then k_surface_normals.  Synchronises h->stream.
int oriented_on_device(er_tsdf_t h, const char* who, bool want, SlabPass& t, float4** d_pts, float4** d_nrm, long* total_out) {
  *d_pts = *d_nrm = nullptr;
  *total_out = 0;
  std::vector<int> keys, slots;
  if (sorted_units(h, keys, slots)) return 1;
  const int n = (int)keys.size();
  if (n == 0) return 0;
  const int nslab = n * 64;
  long total = 0;
  auto launch = [&](float4* out, int pass) {
    hipLaunchKernelGGL(k_surface, dim3(nslab), dim3(64), 0, h->stream, h->pool, t.d_slots, t.d_keys, h->ht_key, h->ht_slot, h->ht_cap - 1, h->ht_shift,
                       t.d_cnt, t.d_off, out, pass);
    ER_W(who, hipGetLastError());
    return 0;
  };
  if (t.alloc(who, n) || t.count(h, who, keys, slots, [&] { return launch(nullptr, 0); }, &total)) return 1;
  *total_out = total;
  if (want && total > 0) {
    ER_W_OWNED(who, t, d_pts, (size_t)total * sizeof(float4));
    ER_W_OWNED(who, t, d_nrm, (size_t)total * sizeof(float4));
    if (t.upload_offsets(h, who) || launch(*d_pts, 1)) return 1;
    hipLaunchKernelGGL(k_surface_normals, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->pool, h->ht_key, h->ht_slot, h->ht_cap - 1,
                       h->ht_shift, *d_pts, total, *d_nrm);
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
  SlabPass t;
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
  SlabPass t;
  float4 *d_pts = nullptr, *d_nrm = nullptr;
  long total = 0, kept = 0;
  if (oriented_on_device(h, who, true, t, &d_pts, &d_nrm, &total)) return 1;
  long* d_blk = nullptr;          // [2 nblk]: counts, then offsets
  float* d_rows = nullptr;        // [kept][3] coordinates, then [kept][3] normals
  const long nblk = (total + 63) / 64;
  std::vector<long> blk((size_t)nblk * 2);
  if (total > 0) {
    ER_W_OWNED(who, t, &d_blk, (size_t)nblk * 2 * sizeof(long));
    hipLaunchKernelGGL(k_oriented_keep, dim3((unsigned)nblk), dim3(64), 0, h->stream, d_pts, d_nrm, total, cube_length, d_blk, d_blk + nblk,
                       (float*)nullptr, (float*)nullptr, 0);
    ER_W(who, hipGetLastError());
    ER_W(who, hipMemcpyAsync(blk.data(), d_blk, (size_t)nblk * sizeof(long), hipMemcpyDeviceToHost, h->stream));
    ER_W(who, hipStreamSynchronize(h->stream));
    for (long b = 0; b < nblk; b++) {
      blk[(size_t)(nblk + b)] = kept;
      kept += blk[(size_t)b];
    }
    if (kept >= (1L << 27))
      return er::fail("er_cloud_create_from_tsdf: %ld points; the limit is 2^27 - 1 (32-bit byte offsets in the search kernels)", kept);
    if (kept > 0) {
      ER_W_OWNED(who, t, &d_rows, (size_t)kept * 6 * sizeof(float));
      ER_W(who, hipMemcpyAsync(d_blk + nblk, blk.data() + nblk, (size_t)nblk * sizeof(long), hipMemcpyHostToDevice, h->stream));
      hipLaunchKernelGGL(k_oriented_keep, dim3((unsigned)nblk), dim3(64), 0, h->stream, d_pts, d_nrm, total, cube_length, d_blk, d_blk + nblk,
                         d_rows, d_rows + (size_t)kept * 3, 1);
      ER_W(who, hipGetLastError());
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
  if (!h || !n_triangles) return er::fail("er_tsdf_extract_mesh: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  std::vector<int> keys, slots;
  if (sorted_units(h, keys, slots)) return 1;
  const int n = (int)keys.size();
  *n_triangles = 0;
  if (n == 0) return 0;
  const int nslab = n * 64;
  SlabPass t;
  unsigned char* d_tab = nullptr;
  float* d_out = nullptr;
  long total = 0;
  auto launch = [&](float* out, int pass) {
    hipLaunchKernelGGL(k_mesh, dim3(nslab), dim3(64), 0, h->stream, h->pool, t.d_slots, t.d_keys, h->ht_key, h->ht_slot, h->ht_cap - 1, h->ht_shift, d_tab,
                       t.d_cnt, t.d_off, out, pass);
    ER_W(who, hipGetLastError());
    return 0;
  };
  if (t.alloc(who, n)) return 1;
  ER_W_OWNED(who, t, &d_tab, 256 * 16);
  auto count_launch = [&] {
    ER_W(who, hipMemcpyAsync(d_tab, er::mc_table().tri, 256 * 16, hipMemcpyHostToDevice, h->stream));
    return launch(nullptr, 0);
  };
  if (t.count(h, who, keys, slots, count_launch, &total)) return 1;
  *n_triangles = total;
  if (tri_host && total > 0) {
    if (capacity_triangles < total) return er::fail("er_tsdf_extract_mesh: capacity %ld < %ld triangles", capacity_triangles, total);
    ER_W_OWNED(who, t, &d_out, (size_t)total * 9 * sizeof(float));
    if (t.upload_offsets(h, who) || launch(d_out, 1)) return 1;
    ER_W(who, hipMemcpyAsync(tri_host, d_out, (size_t)total * 9 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    ER_W(who, hipStreamSynchronize(h->stream));
  }
  return 0;
}

#undef ER_W_OWNED
#undef ER_W

}  // extern "C"
