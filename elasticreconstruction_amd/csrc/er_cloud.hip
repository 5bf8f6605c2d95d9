// er_cloud.hip -- the clouds of path B of liber_hip.so: one er_cloud_s per fragment, uploaded once and reused by every pair, with the uniform grid
// the nearest-neighbour search of er_nn.h walks, built on the device.
// Data layout in HBM:
//   xyz, nrm     float[3n] in file order (the cloud as SOURCE; NaN-normal points already dropped)
//   sorted       float4[n] = {x, y, z, bit_cast(original index)} ordered by grid cell
//   xn           float4[2n] file order, {xyz | normal} records of 32 bytes
//   cell_start   int[cells+1]   uniform grid, cell edge >= the largest search radius, so an exact
//                               nearest neighbour inside the radius lies in the 3x3x3 neighbourhood;
//                               cell id = (z*ny + y)*nx + x, so each (z,y) row is ONE contiguous range
// Clouds are immutable once built.  This is the one translation unit of path B that includes hipcub: what another one needs of it goes through
// er::sort_pairs_u32 and er::inclusive_sum_i32 (er_cloud.h).
#include "er_cloud.h"

#include <hipcub/hipcub.hpp>   // device radix sort / prefix sum of the grid build (library primitives; everything else is hand-written)

#include <atomic>
#include <climits>
#include <cmath>
#include <mutex>
#include <string>

namespace er {
// One device allocation shared by the clouds of a chunk (freed with the last of them).
struct CloudSlab {
  Buffer<char> p;
  std::atomic<int> refs{0};
};
}  // namespace er

using namespace er;

namespace {

// ---- uniform grids of a CHUNK of clouds, built on the device ---------------------------------------------------------------
// (the reference builds a kd-tree per pair and per function, CorresApp.cpp:129,238; here once per fragment)
// Up to kCloudChunk clouds go through ONE set of launches (round 4; before, every cloud had its own ~23 launches and a list of fragments was bound by
// the host's launch rate, not by PCIe: profiles/r04y_cloud_build_timeline.txt):
//   k_chunk_bounds  per cloud (blockIdx.y): min / max of the coordinates (float bits mapped to ordered ints, block reduce, 7 atomics per
//                   workgroup) + a non-finite flag;
//   k_chunk_cells   cell id of every point (the same float32 expression nn_block evaluates for a query) -> key = cloud << shift | cell, the
//                   histogram of every cloud's cells in one concatenated array [ncell_0 + 1 | ncell_1 + 1 | ...], and the interleaved
//                   {point, normal} records;
//   hipcub          ONE stable radix sort of (key, position in the chunk) and ONE prefix sum over the concatenated histograms: element 0 of
//                   cloud k's segment holds -n_(k-1), which cancels the running total at the segment's start, so every segment comes out as that
//                   cloud's own cell_start (0 ... n_k);
//   k_chunk_gather  sorted[s] = {x, y, z, original index within its cloud}; the clouds' sorted arrays are consecutive pieces of one array.
// A stable sort keeps the points of a cell in file order, like a counting sort on the host would: the layout -- and with it the
// order of every float64 reduction that walks the cloud -- is reproducible from run to run, and the same for a cloud built alone or in a list.
__device__ __forceinline__ int ordered_int(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float ordered_float(int i) {
  const int b = i >= 0 ? i : i ^ 0x7fffffff;
  float f;
  memcpy(&f, &b, sizeof f);
  return f;
}

constexpr int kCloudChunk = 8;          // clouds per chunk (3 key bits above the cell id)
struct ChunkDesc {                      // passed by value (kernel argument)
  int m;                                // clouds in the chunk
  int shift;                            // key = cloud << shift | cell
  int n[kCloudChunk];
  int pt_off[kCloudChunk + 1];          // prefix sum of n: a point's position in the chunk
  long cs_off[kCloudChunk + 1];         // prefix sum of (cells + 1): where a cloud's cell_start begins in the chunk's array
  const float* xyz[kCloudChunk];
  const float* nrm[kCloudChunk];
  float4* xn[kCloudChunk];
  GridDims G[kCloudChunk];
};

__global__ __launch_bounds__(kBlock) void k_chunk_bounds(ChunkDesc D, int* __restrict__ out8) {
  const int y = blockIdx.y, n = D.n[y];
  const float* __restrict__ xyz = D.xyz[y];
  int* out7 = out8 + 8 * y;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  int bad = 0, nmax = 0;                                        // nmax: bits of the largest finite |normal component| (both uploads are in: stage A)
  const float* __restrict__ nrm = D.nrm[y];
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float v = xyz[3 * (size_t)i + a];
      bad |= !isfinite(v);
      const int o = ordered_int(v);
      lo[a] = min(lo[a], o);
      hi[a] = max(hi[a], o);
      const float nv = fabsf(nrm[3 * (size_t)i + a]);
      if (isfinite(nv)) nmax = max(nmax, __float_as_int(nv));
    }
  }
  for (int off = 32; off > 0; off >>= 1) nmax = max(nmax, __shfl_down(nmax, off));
  if ((threadIdx.x & 63) == 0 && nmax > 0) atomicMax(&out8[8 * y + 7], nmax);
#pragma unroll
  for (int a = 0; a < 3; a++)
    for (int off = 32; off > 0; off >>= 1) {
      lo[a] = min(lo[a], __shfl_down(lo[a], off));
      hi[a] = max(hi[a], __shfl_down(hi[a], off));
    }
  bad = __any(bad) ? 1 : 0;
  __shared__ int part[kBlock / 64][7];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      part[wave][a] = lo[a];
      part[wave][3 + a] = hi[a];
    }
    part[wave][6] = bad;
  }
  __syncthreads();
  if (threadIdx.x < 7 && (int)blockIdx.x * kBlock < n) {       // 7 atomics per workgroup that saw points
    int v = part[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; w++)
      v = threadIdx.x < 3 ? min(v, part[w][threadIdx.x]) : (threadIdx.x < 6 ? max(v, part[w][threadIdx.x]) : (v | part[w][threadIdx.x]));
    if (threadIdx.x < 3) atomicMin(&out7[threadIdx.x], v);
    else if (threadIdx.x < 6) atomicMax(&out7[threadIdx.x], v);
    else if (v) atomicOr(&out7[6], 1);
  }
}

// xn[2 i] = {x, y, z, 0}, xn[2 i + 1] = {nx, ny, nz, 0} in file order: the matched target point of k_icp_iter is one aligned
// 32-byte record = one cache line instead of two 12-byte gathers from two arrays (those were ~30 % of an ICP iteration).
__global__ __launch_bounds__(kBlock) void k_chunk_cells(ChunkDesc D, unsigned* __restrict__ key, unsigned* __restrict__ idx, int* __restrict__ count) {
  const int y = blockIdx.y, n = D.n[y];
  int* __restrict__ cnt = count + D.cs_off[y];
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[0] = y > 0 ? -D.n[y - 1] : 0;   // (see the prefix sum above; nothing else touches element 0)
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ xyz = D.xyz[y];
  const float* __restrict__ nrm = D.nrm[y];
  const GridDims G = D.G[y];
  const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  int q[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    q[a] = (int)floorf((p[a] - G.org[a]) / G.cell);
    q[a] = min(max(q[a], 0), G.dim[a] - 1);
  }
  const int c = ((q[2] + 2) * (G.dim[1] + 4) + (q[1] + 2)) * (G.dim[0] + 4) + (q[0] + 2);   // two rings of empty cells around the box (struct Grid)
  const unsigned g = (unsigned)(D.pt_off[y] + i);
  key[g] = ((unsigned)y << D.shift) | (unsigned)c;
  idx[g] = g;
  atomicAdd(&cnt[c + 1], 1);                                 // integer histogram: the result does not depend on the order
  float4* __restrict__ xn = D.xn[y];
  xn[2 * (size_t)i] = make_float4(p[0], p[1], p[2], 0.f);
  xn[2 * (size_t)i + 1] = make_float4(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2], 0.f);
}

__global__ __launch_bounds__(kBlock) void k_chunk_gather(ChunkDesc D, const unsigned* __restrict__ key, const unsigned* __restrict__ idx, int total,
                                                         float4* __restrict__ sorted) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= total) return;
  const int y = (int)(key[s] >> D.shift);
  const int i = (int)idx[s] - D.pt_off[y];
  const float* __restrict__ xyz = D.xyz[y];
  float4* __restrict__ out = sorted + (size_t)s + (size_t)kSentinel * (size_t)y;       // kSentinel entries of +inf behind every cloud (scan_range)
  *out = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __int_as_float(i));
  if (s + 1 == D.pt_off[y + 1]) {                                // the cloud's last point in sorted order also writes the sentinels
    const float inf = __int_as_float(0x7f800000);
    for (int k = 1; k <= kSentinel; k++) out[k] = make_float4(inf, inf, inf, __int_as_float(-1));
  }
}

// occ[c] = 1 iff some cell of c's 3 x 3 x 3 neighbourhood holds a point (c over the padded array; cells of the outermost ring get 0: no query is searched
// from there).  One thread per cell, nine row sums of three cells each from the finished cell_start.
__global__ __launch_bounds__(kBlock) void k_chunk_occ(ChunkDesc D, const int* __restrict__ cell_start, unsigned char* __restrict__ occ) {
  const int y = blockIdx.y;
  const GridDims G = D.G[y];
  const int pnx = G.dim[0] + 4, pny = G.dim[1] + 4, pnz = G.dim[2] + 4;
  const long ncell = (long)pnx * pny * pnz;
  const long c = (long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= ncell) return;
  const int* __restrict__ cs = cell_start + D.cs_off[y];
  const int x = (int)(c % pnx), yy = (int)((c / pnx) % pny), z = (int)(c / ((long)pnx * pny));
  int any = 0;
  if (x >= 1 && x <= pnx - 2 && yy >= 1 && yy <= pny - 2 && z >= 1 && z <= pnz - 2) {
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
        const long row = ((long)(z + dz) * pny + (yy + dy)) * pnx + x;
        any |= cs[row + 2] - cs[row - 1];                       // points in cells x-1 .. x+1 of that row
      }
  }
  occ[D.cs_off[y] + c] = any ? 1 : 0;
}


// Grow-only scratch of the grid build, one per device, handed out under a mutex (er_cloud_create may be called from
// several host threads; builds on one device then take turns).
struct GridScratch {
  std::mutex mu;
  int device = -1;
  // Arrays that grow together have one capacity: a failed growth empties all of them.
  Buffer<unsigned> key[4], idx[4];                              // two sets: [2 lane], [2 lane + 1]
  Buffer<char> cub[2];
  Buffer<int> bounds;                                           // 8 ints per cloud of a batch ...
  PinnedBuffer<int> h_bounds;                                   // ... and its page-locked mirror: [cap][8] results, then [cap][8] initial pattern
  hipStream_t up[2] = {nullptr, nullptr};                       // uploads: coordinates on one, normals on the other (two DMA engines keep the link busy)
  hipStream_t cs2[2] = {nullptr, nullptr};                      // grid kernels: consecutive chunks alternate between two lanes
  hipStream_t bs = nullptr;                                     // the bounding boxes of EVERY chunk (stage A): waits for uploads never sit in front of a grid
  hipEvent_t lane_ev = nullptr;
  std::vector<hipEvent_t> ev;                                   // three per chunk of a batch: uploads done (two streams), bounds back
};
GridScratch& grid_scratch(int device) {
  static GridScratch* tab = new GridScratch[64];             // intentionally leaked (see WsPool)
  return tab[device & 63];
}

void slab_release(CloudSlab* sl) {
  if (sl && sl->refs.fetch_sub(1) == 1) delete sl;
}

}  // namespace

int er::no_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return er::fail("%s: no HIP device available (liber_hip has no CPU fallback)", who);
  return 0;
}

int er::check_pair(er_cloud_t src, er_cloud_t tgt, double radius, const char* who) {
  if (!src || !tgt) return er::fail("%s: NULL cloud", who);
  if (src->device != tgt->device) return er::fail("%s: source and target live on different devices", who);
  if (!(radius > 0.0) || radius > (double)tgt->radius_cap * (1.0 + 1e-6))
    return er::fail("%s: search radius %g exceeds the target's grid cell %g (er_cloud_create grid_cell)", who, radius, (double)tgt->radius_cap);
  return 0;
}

int er::cloud_bounds(const er_cloud_s* c, hipStream_t stream, float lo[3], float hi[3]) {
  const int n = c->n;
  DevScope B;
  int* d_box;
  if (B.alloc(&d_box, 8, "cloud_bounds")) return 1;
  int box[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
  ER_HIP_TRY(hipMemcpyAsync(d_box, box, sizeof box, hipMemcpyHostToDevice, stream));
  ChunkDesc D{};
  D.m = 1;
  D.n[0] = n;
  D.pt_off[1] = n;
  D.xyz[0] = c->xyz;
  D.nrm[0] = c->nrm;
  hipLaunchKernelGGL(k_chunk_bounds, dim3(std::min(nblocks_of(n), 128), 1), dim3(kBlock), 0, stream, D, d_box);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipMemcpyAsync(box, d_box, sizeof box, hipMemcpyDeviceToHost, stream));
  ER_HIP_TRY(hipStreamSynchronize(stream));
  for (int a = 0; a < 3; a++) {
    lo[a] = ordered_float(box[a]);
    hi[a] = ordered_float(box[3 + a]);
  }
  return 0;
}

hipError_t er::sort_pairs_u32(void* tmp, size_t& tmp_bytes, const unsigned* keys_in, unsigned* keys_out, const unsigned* values_in, unsigned* values_out,
                              int n, int begin_bit, int end_bit, hipStream_t stream) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys_in, keys_out, values_in, values_out, n, begin_bit, end_bit, stream);
}

hipError_t er::inclusive_sum_i32(void* tmp, size_t& tmp_bytes, int* in, int* out, int n, hipStream_t stream) {
  return hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, in, out, n, stream);
}

// Clouds of a LIST of fragments (BuildCorrespondence's LoadData loop, CorresApp.cpp:82-110, builds them one after the other), in chunks of up to
// kCloudChunk clouds that share two device allocations and ONE set of grid launches:
//   stage A, for every chunk up front: the chunk's allocation, its uploads -- coordinates and normals on two copy streams, truly asynchronous
//            when the caller's arrays are page-locked (er_host_alloc) -- and its bounding boxes on a compute lane as soon as the uploads are in;
//   stage B, chunk by chunk: ONE host wait for the boxes (the host sizes the grids from them), then cell ids + histogram + interleave, one
//            radix sort, one prefix sum, one gather for the whole chunk, while the later chunks are still uploading.
// The list is PCIe-bound; before round 4's last step it was bound by the host's launch rate (23 launches per cloud).
// `kind`: where the rows come from -- hipMemcpyHostToDevice (er_cloud_create / er_cloud_create_batch) or hipMemcpyDeviceToDevice (rows that a
// kernel on this device has left complete, er::cloud_create_device); everything behind the copy is the same.
static int cloud_create_impl(int n_clouds, const float* const* xyz_host, const float* const* normal_host, const int* counts, float grid_cell, int device,
                             er_cloud_t* out, hipMemcpyKind kind) {
  if (n_clouds < 0 || (n_clouds > 0 && (!xyz_host || !normal_host || !counts || !out))) return er::fail("er_cloud_create: bad arguments");
  for (int i = 0; i < n_clouds; i++) out[i] = nullptr;
  for (int i = 0; i < n_clouds; i++)
    if (counts[i] < 0 || (counts[i] > 0 && (!xyz_host[i] || !normal_host[i]))) return er::fail("er_cloud_create: bad arguments (cloud %d)", i);
  // the search kernels address candidates, matched-target records and the ICP loop's X by UNSIGNED 32-bit byte offsets (s * 16, i * 32, k * 12: struct
  // PairDev's hot accesses): a cloud must stay below 2^27 points, or those offsets wrap and the kernels read other memory
  for (int i = 0; i < n_clouds; i++)
    if (counts[i] >= (1 << 27)) return er::fail("er_cloud_create: cloud %d has %d points; the limit is 2^27 - 1 (32-bit byte offsets in the search kernels)", i, counts[i]);
  if (!(grid_cell > 0.f)) return er::fail("er_cloud_create: grid_cell must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_cloud_create: no HIP device available (liber_hip has no CPU fallback)");
  if (device < 0 || device >= ndev) return er::fail("er_cloud_create: device %d out of range [0,%d)", device, ndev);
  if (n_clouds == 0) return 0;
  ER_HIP_TRY(hipSetDevice(device));
  GridScratch& gs = grid_scratch(device);
  std::lock_guard<std::mutex> lock(gs.mu);
  auto sync_all = [&]() -> hipError_t {
    hipError_t e = hipSuccess;
    for (hipStream_t st : {gs.up[0], gs.up[1], gs.cs2[0], gs.cs2[1], gs.bs})
      if (st) {
        const hipError_t e1 = hipStreamSynchronize(st);
        if (e == hipSuccess) e = e1;
      }
    return e;
  };
  auto undo = [&]() {
    (void)sync_all();
    for (int i = 0; i < n_clouds; i++) {
      if (out[i]) er_cloud_destroy(out[i]);
      out[i] = nullptr;
    }
  };
#define ER_CTRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      er::fail("er_cloud_create: %s failed: %s", #expr, hipGetErrorString(e_));               \
      undo();                                                                                 \
      return 1;                                                                               \
    }                                                                                         \
  } while (0)
  for (int q = 0; q < 2; q++) {
    if (!gs.up[q]) ER_CTRY(hipStreamCreateWithFlags(&gs.up[q], hipStreamNonBlocking));
    if (!gs.cs2[q]) ER_CTRY(hipStreamCreateWithFlags(&gs.cs2[q], hipStreamNonBlocking));
    if (!gs.bs) ER_CTRY(hipStreamCreateWithFlags(&gs.bs, hipStreamNonBlocking));
  }
  if (!gs.lane_ev) ER_CTRY(hipEventCreateWithFlags(&gs.lane_ev, hipEventDisableTiming));
  // ---- the chunks: consecutive clouds, at most kCloudChunk of them and kChunkPoints points (the first cloud of a chunk always fits) ----
  constexpr long kChunkPoints = 16L << 20;
  struct Chunk {
    int i0 = 0, i1 = 0;
    long total = 0;                     // points
    CloudSlab *pts = nullptr, *cells = nullptr;
    float4* sorted = nullptr;           // the chunk's sorted array (the clouds' pieces are consecutive)
    ChunkDesc D{};
  };
  std::vector<Chunk> chunks;
  {
    // a chunk takes half of what is left (at most kCloudChunk): the list ends in small chunks, and what remains to be done after the
    // last upload -- the last chunk's grids -- is short (25 fragments: 8, 8, 5, 2, 1, 1)
    for (int i = 0; i < n_clouds;) {
      Chunk c;
      c.i0 = i;
      const int per = std::min(kCloudChunk, std::max(1, (n_clouds - i + 1) / 2));
      while (i < n_clouds && i - c.i0 < per && (i == c.i0 || c.total + counts[i] <= kChunkPoints)) c.total += counts[i++];
      c.i1 = i;
      chunks.push_back(c);
    }
  }
  const int n_chunks = (int)chunks.size();
  while ((int)gs.ev.size() < 3 * n_chunks) {
    hipEvent_t e = nullptr;
    ER_CTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    gs.ev.push_back(e);
  }
  const char* who = "er_cloud_create";
  if (gs.bounds.capacity() < (size_t)n_clouds * 8) {
    ER_CTRY(sync_all());
    const size_t cap = (size_t)n_clouds + 16;
    if (gs.bounds.reserve(cap * 8, who) || gs.h_bounds.reserve(cap * 16, who)) {
      gs.bounds.reset();
      undo();
      return 1;
    }
  }
  long t_max = 0;
  for (const Chunk& c : chunks) t_max = std::max(t_max, c.total);
  if (t_max >= (1L << 31) - kBlock) return er::fail("er_cloud_create: a cloud of %ld points is beyond the 32-bit point index", t_max);
  if (t_max > 0) {
    if (gs.key[0].capacity() < (size_t)t_max) {
      ER_CTRY(sync_all());
      const size_t cap = (size_t)t_max + (size_t)t_max / 8;
      bool ok = true;
      for (int q = 0; q < 4; q++) ok = ok && !gs.key[q].reserve(cap, who) && !gs.idx[q].reserve(cap, who);
      if (!ok) {
        for (int q = 0; q < 4; q++) gs.key[q].reset(), gs.idx[q].reset();
        undo();
        return 1;
      }
    }
    // temporary storage of the sort / scan for the largest chunk and the largest grids (2^25 cells and 3 cloud bits: 28 key bits) this call can meet
    size_t need_sort = 0, need_scan = 0;
    ER_CTRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, gs.key[0].get(), gs.key[1].get(), gs.idx[0].get(), gs.idx[1].get(), (int)t_max, 0, 28, gs.cs2[0]));
    ER_CTRY(hipcub::DeviceScan::InclusiveSum(nullptr, need_scan, (int*)nullptr, (int*)nullptr, kCloudChunk * ((1 << 25) + 1), gs.cs2[0]));
    const size_t need = std::max(need_sort, need_scan);
    if (gs.cub[0].capacity() < need) {
      ER_CTRY(sync_all());
      if (gs.cub[0].reserve(need + need / 4, who) || gs.cub[1].reserve(need + need / 4, who)) {
        gs.cub[0].reset();
        undo();
        return 1;
      }
    }
  }
  int* h_got = gs.h_bounds;
  int* h_init = gs.h_bounds + gs.bounds.capacity();
  for (int i = 0; i < n_clouds; i++) {
    const int init[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
    memcpy(h_init + (size_t)i * 8, init, sizeof init);
  }
  ER_CTRY(hipMemcpyAsync(gs.bounds, h_init, (size_t)n_clouds * 8 * sizeof(int), hipMemcpyHostToDevice, gs.cs2[0]));
  ER_CTRY(hipEventRecord(gs.lane_ev, gs.cs2[0]));
  ER_CTRY(hipStreamWaitEvent(gs.cs2[1], gs.lane_ev, 0));
  ER_CTRY(hipStreamWaitEvent(gs.bs, gs.lane_ev, 0));            // (the boxes' initial pattern is in place before the first bounds kernel)
  // ---- stage A of a chunk: allocation, uploads (two copy streams), bounding boxes (the chunk's compute lane) ----
  auto stage_a = [&](int ch) -> int {
    Chunk& C = chunks[(size_t)ch];
    const int m = C.i1 - C.i0;
    const size_t N = (size_t)C.total;
    // one allocation: [sorted N float4 + kSentinel entries of +inf behind every cloud (scan_range) | xn 2N float4 (32-byte aligned records) | per cloud: xyz 3n,
    // normals 3n floats]
    const size_t xn_base = (N + (size_t)kSentinel * (size_t)m + 1) & ~(size_t)1;
    const size_t f_base = (xn_base + 2 * N) * 4;
    const size_t bytes = std::max((f_base + 6 * N) * sizeof(float), (size_t)256);
    C.pts = new CloudSlab();
    if (C.pts->p.reserve(bytes, who)) {
      delete C.pts;
      C.pts = nullptr;
      return 1;
    }
    C.pts->refs = m;
    C.sorted = reinterpret_cast<float4*>(C.pts->p.get());
    float* fbase = reinterpret_cast<float*>(C.pts->p.get()) + f_base;
    C.D.m = m;
    long off = 0;
    for (int k = 0; k < m; k++) {                                 // the cloud objects first: from here on undo() releases the allocation through them
      const int i = C.i0 + k, n = counts[i];
      er_cloud_t c = new er_cloud_s();
      out[i] = c;
      c->device = device;
      c->n = n;
      c->radius_cap = grid_cell;
      c->pts_slab = C.pts;
      c->sorted = C.sorted + off + (long)kSentinel * k;
      c->xn = C.sorted + xn_base + 2 * off;
      c->xyz = fbase + 6 * off;
      c->nrm = c->xyz + 3 * (size_t)n;
      C.D.n[k] = n;
      C.D.pt_off[k] = (int)off;
      C.D.xyz[k] = c->xyz;
      C.D.nrm[k] = c->nrm;
      C.D.xn[k] = c->xn;
      off += n;
    }
    C.D.pt_off[m] = (int)off;
    for (int k = 0; k < m; k++) {
      const int i = C.i0 + k, n = counts[i];
      if (n > 0) {
        ER_HIP_TRY(hipMemcpyAsync(out[i]->xyz, xyz_host[i], (size_t)n * 3 * sizeof(float), kind, gs.up[0]));
        ER_HIP_TRY(hipMemcpyAsync(out[i]->nrm, normal_host[i], (size_t)n * 3 * sizeof(float), kind, gs.up[1]));
      }
    }
    // Stage A runs on a stream of its own (round 5): on the two grid lanes the upload waits of chunk 2, 4, ... were queued IN FRONT of
    // chunk 0's grid (in-order streams; every stage A is enqueued before the first stage B), so "built while the later chunks are still uploading" mostly
    // did not happen.  Stage B of a chunk starts after the HOST has seen the chunk's boxes (ev[3 ch + 2]), hence after its uploads.
    hipStream_t L = gs.bs;
    for (int q = 0; q < 2; q++) {
      ER_HIP_TRY(hipEventRecord(gs.ev[(size_t)(3 * ch + q)], gs.up[q]));
      ER_HIP_TRY(hipStreamWaitEvent(L, gs.ev[(size_t)(3 * ch + q)], 0));
    }
    int n_big = 0;
    for (int k = 0; k < m; k++) n_big = std::max(n_big, C.D.n[k]);
    if (n_big > 0)
      hipLaunchKernelGGL(k_chunk_bounds, dim3(std::min(nblocks_of(n_big), 128), m), dim3(kBlock), 0, L, C.D, gs.bounds + (size_t)C.i0 * 8);
    ER_HIP_TRY(hipGetLastError());
    ER_HIP_TRY(hipMemcpyAsync(h_got + (size_t)C.i0 * 8, gs.bounds + (size_t)C.i0 * 8, (size_t)m * 8 * sizeof(int), hipMemcpyDeviceToHost, L));
    ER_HIP_TRY(hipEventRecord(gs.ev[(size_t)(3 * ch + 2)], L));
    return 0;
  };
  // ---- stage B: the grids of the chunk (its boxes are back) ----
  auto stage_b = [&](int ch) -> int {
    Chunk& C = chunks[(size_t)ch];
    const int m = C.i1 - C.i0;
    ER_HIP_TRY(hipEventSynchronize(gs.ev[(size_t)(3 * ch + 2)]));
    long cs_total = 0;
    int max_cells = 1;
    for (int k = 0; k < m; k++) {
      er_cloud_t c = out[C.i0 + k];
      const int n = c->n;
      const int* got = h_got + (size_t)(C.i0 + k) * 8;
      float cell = grid_cell * 1.001f;                            // strictly larger than any admissible radius
      float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
      int dim[3] = {1, 1, 1};
      if (n > 0) {
        if (got[7] > 0) memcpy(&c->nmax, &got[7], sizeof(float));
        if (got[6]) return er::fail("er_cloud_create: non-finite coordinates");
        for (int a = 0; a < 3; a++) {
          lo[a] = ordered_float(got[a]);
          hi[a] = ordered_float(got[3 + a]);
        }
      }
      constexpr int kRing = 4;                                    // two rings of empty cells per axis (struct Grid)
      for (;;) {
        long total = 1;
        for (int a = 0; a < 3; a++) {
          dim[a] = (int)std::floor((hi[a] - lo[a]) / cell) + 1;
          total *= dim[a] + kRing;
        }
        if (total <= (1L << 25)) break;
        cell *= 2.f;
      }
      const int ncell = (dim[0] + kRing) * (dim[1] + kRing) * (dim[2] + kRing);
      max_cells = std::max(max_cells, ncell);
      C.D.cs_off[k] = cs_total;
      cs_total += (long)ncell + 1;
      c->grid.cell = cell;
      for (int a = 0; a < 3; a++) {
        c->grid.org[a] = C.D.G[k].org[a] = lo[a];
        c->grid.dim[a] = C.D.G[k].dim[a] = dim[a];
      }
      C.D.G[k].cell = cell;
      c->grid.slack = grid_slack(dim, cell);
      c->grid.pnx = dim[0] + 4;
      c->grid.pny = dim[1] + 4;
    }
    C.D.cs_off[m] = cs_total;
    C.cells = new CloudSlab();
    const size_t cells_bytes = (size_t)cs_total * sizeof(int) + (size_t)cs_total;   // cell_start of the chunk's clouds, then one occupancy byte per cell
    if (C.cells->p.reserve(cells_bytes, who)) {
      delete C.cells;
      C.cells = nullptr;
      return 1;
    }
    C.cells->refs = m;
    int* cs = reinterpret_cast<int*>(C.cells->p.get());
    unsigned char* occ = reinterpret_cast<unsigned char*>(cs + cs_total);
    for (int k = 0; k < m; k++) {
      er_cloud_t c = out[C.i0 + k];
      c->cell_slab = C.cells;
      c->cell_start = cs + C.D.cs_off[k];
      c->grid.pts = c->sorted;
      c->grid.cell_start = c->cell_start;
      c->grid.occ = occ + C.D.cs_off[k];
    }
    int bits = 1;
    while ((1L << bits) < (long)max_cells) bits++;
    C.D.shift = bits;
    const int q = ch & 1;
    hipStream_t L = gs.cs2[q];
    unsigned *k0 = gs.key[2 * q], *k1 = gs.key[2 * q + 1], *x0 = gs.idx[2 * q], *x1 = gs.idx[2 * q + 1];
    ER_HIP_TRY(hipMemsetAsync(cs, 0, (size_t)cs_total * sizeof(int), L));
    int n_big = 0;
    for (int k = 0; k < m; k++) n_big = std::max(n_big, C.D.n[k]);
    hipLaunchKernelGGL(k_chunk_cells, dim3(nblocks_of(n_big), m), dim3(kBlock), 0, L, C.D, k0, x0, cs);
    size_t tmp = gs.cub[q].capacity();
    if (C.total > 0) ER_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(gs.cub[q], tmp, k0, k1, x0, x1, (int)C.total, 0, bits + 3, L));
    tmp = gs.cub[q].capacity();
    ER_HIP_TRY(hipcub::DeviceScan::InclusiveSum(gs.cub[q], tmp, cs, cs, (int)cs_total, L));
    hipLaunchKernelGGL(k_chunk_occ, dim3((unsigned)((max_cells + kBlock - 1) / kBlock), m), dim3(kBlock), 0, L, C.D, cs, occ);
    if (C.total > 0) hipLaunchKernelGGL(k_chunk_gather, dim3(nblocks_of((int)C.total)), dim3(kBlock), 0, L, C.D, k1, x1, (int)C.total, C.sorted);
    ER_HIP_TRY(hipGetLastError());
    return 0;
  };
  int rc = 0;
  for (int ch = 0; ch < n_chunks && rc == 0; ch++) rc = stage_a(ch);   // every upload is queued before the first host wait
  for (int ch = 0; ch < n_chunks && rc == 0; ch++) rc = stage_b(ch);
  if (rc == 0 && sync_all() != hipSuccess)                              // the caller's arrays and the shared scratch are free again
    rc = er::fail("er_cloud_create: %s", hipGetErrorString(hipGetLastError()));
#undef ER_CTRY
  if (rc) {
    const std::string why = er_last_error();
    undo();
    return er::fail("%s", why.c_str());
  }
  return 0;
}

int er::cloud_create_device(const float* xyz_dev, const float* normal_dev, int n, float grid_cell, int device, er_cloud_s** out) {
  return cloud_create_impl(1, &xyz_dev, &normal_dev, &n, grid_cell, device, out, hipMemcpyDeviceToDevice);
}

extern "C" {

int er_cloud_create_batch(int n_clouds, const float* const* xyz_host, const float* const* normal_host, const int* counts, float grid_cell, int device,
                          er_cloud_t* out) {
  return cloud_create_impl(n_clouds, xyz_host, normal_host, counts, grid_cell, device, out, hipMemcpyHostToDevice);
}

int er_cloud_create(const float* xyz_host, const float* normal_host, int n, float grid_cell, int device, er_cloud_t* out) {
  if (!out) return er::fail("er_cloud_create: out is NULL");
  *out = nullptr;
  if (n < 0 || (n > 0 && (!xyz_host || !normal_host))) return er::fail("er_cloud_create: bad arguments");
  return er_cloud_create_batch(1, &xyz_host, &normal_host, &n, grid_cell, device, out);
}

int er_cloud_destroy(er_cloud_t c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  slab_release(c->pts_slab);                    // xyz, normals, sorted and xn live in the chunk's allocation, cell_start in its second one:
  slab_release(c->cell_slab);                   // both go with the last cloud of the chunk
  delete c;
  return 0;
}

int er_cloud_size(er_cloud_t c) { return c ? c->n : -1; }

}  // extern "C"
