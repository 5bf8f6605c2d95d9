// er_fpfh.hip -- the first half of GlobalRegistration's do_all on the device (it shares er_cloud_s, er_features_s and the chunk grid builder
// through er_cloud.h and, through er::StreamLease, the workspace pool of er_icp.hip): pcl::VoxelGrid at resample_leaf (GlobalRegistration.cpp:59-68),
// pcl::NormalEstimationOMP with the sign flip against the input normals (:81-117) and pcl::FPFHEstimationOMP (:121-128), once per
// fragment and from the cloud that is already in HBM.  The PCL calls are pinned to the restatement of tests/fpfh_restatement.py.
//   k_vox_keys / hipcub sort / k_vox_heads / hipcub scan / k_vox_starts / k_vox_mean      (hipcub through er::sort_pairs_u32 / er::inclusive_sum_i32)
//                     one key per point, a stable sort, the segment of every occupied cell, one float64 mean per cell and component
//   k_fp_normals      one wave per point: neighbour centroid, float64 covariance, smallest eigenvector, sign from the input normal
//   k_fp_spfh         one wave per point: the three pair features against every neighbour -> 3 x 11 INTEGER counts in LDS
//   k_fp_fpfh         one wave per point: the 1 / d^2 weighted sum of the neighbours' SPFH rows, lane b = bin b, then the block scaling
// Radius queries: a TEMPORARY grid per call, built by the cloud builder itself (er::cloud_create_device) with cell = radius, so that every
// neighbour lies in the 27 cells around a point's own -- nine contiguous ranges of the cell-sorted array.  The cloud's own grid (cell =
// max_corr_dist = 0.075) would need two or four rings (125 / 343 cells, mostly outside the sphere) and would make the candidate order, hence
// the float64 sums, depend on the grid_cell the caller happened to choose.  The neighbour lists are NOT stored: k_fp_fpfh searches again
// (the search is a few hundred 16-byte loads per point from L2; lists would need a count pass, a scan and a second walk anyway).
// Every result is a function of the cloud and the radius alone: a wave walks the nine ranges in a fixed order, candidate s of a range goes to
// lane (s - first) % 64, cross-lane sums are xor butterflies (the same bits in every lane), the histogram is integer, and k_fp_fpfh adds
// its neighbours one after the other in candidate order.  No float atomics.
#include "er_cloud.h"
#include "er_fpfh_math.h"

#include <algorithm>
#include <climits>
#include <cmath>

using namespace er;

namespace {

constexpr int kFpWaves = kBlock / 64;          // points per workgroup of the wave-per-point kernels

__device__ __forceinline__ double fp_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int fp_wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Every lane of the wave calls f(in_range, candidate) for the points of the 27 cells around q's own cell, 64 candidates per trip.  q must be a
// point of the cloud the grid was built for: its cell is inside the box, so all 27 cells exist (two rings of empty cells, struct Grid).
template <class F>
__device__ __forceinline__ void fp_for_candidates(const Grid& g, float qx, float qy, float qz, int lane, F&& f) {
  // the cell id as k_chunk_cells assigned it
  const int ix = min(max((int)floorf((qx - g.org[0]) / g.cell), 0), g.dim[0] - 1);
  const int iy = min(max((int)floorf((qy - g.org[1]) / g.cell), 0), g.dim[1] - 1);
  const int iz = min(max((int)floorf((qz - g.org[2]) / g.cell), 0), g.dim[2] - 1);
  const int own = ((iz + 2) * g.pny + (iy + 2)) * g.pnx + (ix + 2);
  for (int r = 0; r < 9; r++) {
    const int row = own + ((r / 3 - 1) * g.pny + (r % 3 - 1)) * g.pnx;
    const int s0 = g.cell_start[row - 1], s1 = g.cell_start[row + 2];           // cells x-1 .. x+1 of the row: one contiguous range
    for (int base = s0; base < s1; base += 64) {
      const int s = base + lane;
      const bool in = s < s1;
      const float4 p = in ? g.pts[s] : make_float4(0.f, 0.f, 0.f, 0.f);
      f(in, p);
    }
  }
}

// ---- voxel grid ------------------------------------------------------------------------------------------------------------
struct VoxDims {
  float inv;
  int min_b[3];
  int div[3];
};

__global__ __launch_bounds__(kBlock) void k_vox_keys(const float* __restrict__ xyz, int n, VoxDims V, unsigned* __restrict__ key,
                                                     unsigned* __restrict__ idx) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int a = er_fp::voxel_index(xyz[3 * (size_t)i], V.inv) - V.min_b[0];
  const int b = er_fp::voxel_index(xyz[3 * (size_t)i + 1], V.inv) - V.min_b[1];
  const int c = er_fp::voxel_index(xyz[3 * (size_t)i + 2], V.inv) - V.min_b[2];
  key[i] = (unsigned)a + (unsigned)b * (unsigned)V.div[0] + (unsigned)c * (unsigned)V.div[0] * (unsigned)V.div[1];
  idx[i] = (unsigned)i;
}

__global__ __launch_bounds__(kBlock) void k_vox_heads(const unsigned* __restrict__ key, int n, int* __restrict__ head) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  head[s] = (s == 0 || key[s] != key[s - 1]) ? 1 : 0;
}

// seg = inclusive sum of head: the sorted position s belongs to output point seg[s] - 1
__global__ __launch_bounds__(kBlock) void k_vox_starts(const unsigned* __restrict__ key, const int* __restrict__ seg, int n, int n_out,
                                                       int* __restrict__ start) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  if (s == 0 || key[s] != key[s - 1]) {
    const int o = seg[s] - 1;
    if (o >= 0 && o < n_out) start[o] = s;
  }
  if (s == n - 1) start[n_out] = n;
}

// One thread per occupied cell: the float64 sums of its members in file order (the sort is stable), divided by the count, rounded once.
__global__ __launch_bounds__(kBlock) void k_vox_mean(const float* __restrict__ xyz, const float* __restrict__ nrm, const unsigned* __restrict__ idx,
                                                     const int* __restrict__ start, int n_out, float* __restrict__ oxyz, float* __restrict__ onrm) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o >= n_out) return;
  const int s0 = start[o], s1 = start[o + 1];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int s = s0; s < s1; s++) {
    const size_t i = idx[s];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      acc[a] += (double)xyz[3 * i + a];
      acc[3 + a] += (double)nrm[3 * i + a];
    }
  }
  const double cnt = (double)(s1 - s0);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    oxyz[3 * (size_t)o + a] = (float)(acc[a] / cnt);
    onrm[3 * (size_t)o + a] = (float)(acc[3 + a] / cnt);
  }
}

// ---- normals ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_fp_normals(const float4* __restrict__ xn, int n, Grid g, float r2, float* __restrict__ out,
                                                       int* __restrict__ nn) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kFpWaves + (int)(threadIdx.x >> 6);
  if (i >= n) return;                                          // wave-uniform; the kernel has no barrier
  const float4 q = xn[2 * (size_t)i], nin = xn[2 * (size_t)i + 1];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int cnt = 0;
  fp_for_candidates(g, q.x, q.y, q.z, lane, [&](bool in, const float4& p) {
    if (in && er_fp::sqdist32(p.x, p.y, p.z, q.x, q.y, q.z) < r2) {
      sx += (double)p.x;
      sy += (double)p.y;
      sz += (double)p.z;
      cnt++;
    }
  });
  cnt = fp_wave_sum(cnt);
  const double cx = fp_wave_sum(sx) / (double)cnt, cy = fp_wave_sum(sy) / (double)cnt, cz = fp_wave_sum(sz) / (double)cnt;
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  fp_for_candidates(g, q.x, q.y, q.z, lane, [&](bool in, const float4& p) {
    if (in && er_fp::sqdist32(p.x, p.y, p.z, q.x, q.y, q.z) < r2) {
      const double dx = (double)p.x - cx, dy = (double)p.y - cy, dz = (double)p.z - cz;
      c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz;
      c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
    }
  });
#pragma unroll
  for (int k = 0; k < 6; k++) c[k] = fp_wave_sum(c[k]);
  float ox, oy, oz;
  if (cnt < 3) {
    ox = oy = oz = __int_as_float(0x7fc00000);
  } else {
    double v[3], lam[3];
    er_fp::smallest_eigvec(c, v, lam);
    if (er_fp::dot3(v[0], v[1], v[2], (double)nin.x, (double)nin.y, (double)nin.z) < 0.0) {
      v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2];
    }
    ox = (float)v[0]; oy = (float)v[1]; oz = (float)v[2];
  }
  if (lane == 0) {
    out[3 * (size_t)i] = ox;
    out[3 * (size_t)i + 1] = oy;
    out[3 * (size_t)i + 2] = oz;
    nn[i] = cnt;
  }
}

// ---- SPFH ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_fp_spfh(const float4* __restrict__ xn, int n, Grid g, float r2, int* __restrict__ counts,
                                                    int* __restrict__ nn) {
  __shared__ int hist[kFpWaves][er_fp::kDim];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kFpWaves + wave;
  if (lane < er_fp::kDim) hist[wave][lane] = 0;
  __syncthreads();
  int cnt = 0;
  if (i < n) {                                                 // wave-uniform
    const float4 q = xn[2 * (size_t)i], qn = xn[2 * (size_t)i + 1];
    const float p1[3] = {q.x, q.y, q.z}, n1[3] = {qn.x, qn.y, qn.z};
    fp_for_candidates(g, q.x, q.y, q.z, lane, [&](bool in, const float4& p) {
      if (in && er_fp::sqdist32(p.x, p.y, p.z, q.x, q.y, q.z) < r2) {
        cnt++;
        const int j = __float_as_int(p.w);
        if (j != i) {
          const float4 jn = xn[2 * (size_t)j + 1];
          const float p2[3] = {p.x, p.y, p.z}, n2[3] = {jn.x, jn.y, jn.z};
          int bin[3];
          if (er_fp::pair_bins(p1, n1, p2, n2, bin)) {
            atomicAdd(&hist[wave][bin[0]], 1);                 // integer: the order does not matter
            atomicAdd(&hist[wave][er_fp::kBins + bin[1]], 1);
            atomicAdd(&hist[wave][2 * er_fp::kBins + bin[2]], 1);
          }
        }
      }
    });
    cnt = fp_wave_sum(cnt);
  }
  __syncthreads();
  if (i < n) {
    if (lane < er_fp::kDim) counts[(size_t)i * er_fp::kDim + lane] = hist[wave][lane];
    if (lane == 0) nn[i] = cnt;
  }
}

// ---- FPFH ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_fp_fpfh(const float4* __restrict__ xn, int n, Grid g, float r2, const int* __restrict__ counts,
                                                    const int* __restrict__ nn, float* __restrict__ feat, int dp) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kFpWaves + (int)(threadIdx.x >> 6);
  if (i >= n) return;                                          // wave-uniform; no barrier
  const float4 q = xn[2 * (size_t)i], qn = xn[2 * (size_t)i + 1];
  const int b = lane < er_fp::kDim ? lane : 0;
  double acc = 0.0;
  fp_for_candidates(g, q.x, q.y, q.z, lane, [&](bool in, const float4& p) {
    const float d2 = er_fp::sqdist32(p.x, p.y, p.z, q.x, q.y, q.z);
    unsigned long long todo = __ballot(in && d2 < r2 && d2 != 0.f);
    while (todo) {                                             // the neighbours of this trip one after the other, in candidate order
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int j = __shfl(__float_as_int(p.w), src);
      const double w = 1.0 / (double)__shfl(d2, src);
      const int m = nn[j] - 1;
      if (m > 0) acc += ((double)counts[(size_t)j * er_fp::kDim + b] * 100.0 / (double)m) * w;
    }
  });
  // the three block sums, bin after bin, in every lane
  double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < er_fp::kDim; k++) sum[k / er_fp::kBins] += __shfl(acc, k);
  const double s = lane < er_fp::kBins ? sum[0] : (lane < 2 * er_fp::kBins ? sum[1] : sum[2]);
  float v = (float)(s != 0.0 ? acc * (100.0 / s) : acc);
  if (!(isfinite(qn.x) && isfinite(qn.y) && isfinite(qn.z))) v = 0.f;            // (er_features_s holds finite values only)
  if (lane < er_fp::kDim) feat[(size_t)i * dp + lane] = v;
}

struct CloudHolder {                               // a temporary cloud (the grid of one radius)
  er_cloud_t c = nullptr;
  ~CloudHolder() {
    if (c) er_cloud_destroy(c);
  }
};

bool fp_bad_length(float v) { return !(v > 0.f) || !std::isfinite(v); }

int fp_check_cloud(er_cloud_t c, const char* who) {
  if (!c) return er::fail("%s: NULL cloud", who);
  if (c->n <= 0) return er::fail("%s: the cloud is empty", who);
  return 0;
}

// The grid of one radius over the points of c (the cloud builder's own kernels; cell = 1.001 radius or, beyond 2^25 cells, a multiple).
// The 27-cell walk is exact as long as the float32 cell coordinate floorf((q - org) / cell) of a point and of its neighbour are each off by less
// than half of the 0.001 cell the grid adds to the radius: the coordinate carries 2 x 2^-24 of relative error, i.e. 1.2e-7 x (cells along the
// axis) cells, so the axis may span about 4 000 cells.  A cloud wider than that for this radius is refused (a fragment spans tens of cells).
constexpr int kFpMaxCellsPerAxis = 4000;
int fp_radius_grid(er_cloud_t c, float radius, CloudHolder* out, const char* who) {
  if (er::cloud_create_device(c->xyz, c->nrm, c->n, radius, c->device, &out->c)) return 1;
  const Grid& g = out->c->grid;
  if (std::max(g.dim[0], std::max(g.dim[1], g.dim[2])) > kFpMaxCellsPerAxis)
    return er::fail("%s: the cloud spans more than %d cells of radius %g along one axis; the radius search is not exact there", who, kFpMaxCellsPerAxis,
                    (double)radius);
  return 0;
}

int fp_blocks(int n) { return (n + kFpWaves - 1) / kFpWaves; }

}  // namespace

extern "C" {

int er_cloud_read(er_cloud_t c, float* xyz_host, float* normal_host) {
  if (no_device("er_cloud_read")) return 1;
  if (!c) return er::fail("er_cloud_read: NULL cloud");
  ER_HIP_TRY(hipSetDevice(c->device));
  if (c->n > 0 && xyz_host) ER_HIP_TRY(hipMemcpy(xyz_host, c->xyz, (size_t)c->n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (c->n > 0 && normal_host) ER_HIP_TRY(hipMemcpy(normal_host, c->nrm, (size_t)c->n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int er_features_dim(er_features_t f) { return f ? f->dim : -1; }

int er_features_read(er_features_t f, float* feat_host) {
  if (no_device("er_features_read")) return 1;
  if (!f || !feat_host) return er::fail("er_features_read: NULL argument");
  ER_HIP_TRY(hipSetDevice(f->device));
  if (f->n > 0)
    ER_HIP_TRY(hipMemcpy2D(feat_host, (size_t)f->dim * sizeof(float), f->d, (size_t)f->dp * sizeof(float), (size_t)f->dim * sizeof(float),
                           (size_t)f->n, hipMemcpyDeviceToHost));
  return 0;
}

int er_cloud_voxel_grid(er_cloud_t in, float leaf, float grid_cell, er_cloud_t* out, int* n_out) {
  if (!out) return er::fail("er_cloud_voxel_grid: out is NULL");
  *out = nullptr;
  if (n_out) *n_out = 0;
  if (no_device("er_cloud_voxel_grid")) return 1;
  if (fp_check_cloud(in, "er_cloud_voxel_grid")) return 1;
  if (fp_bad_length(leaf)) return er::fail("er_cloud_voxel_grid: leaf %g must be positive and finite", (double)leaf);
  if (fp_bad_length(grid_cell)) return er::fail("er_cloud_voxel_grid: grid_cell %g must be positive and finite", (double)grid_cell);
  const int n = in->n;
  StreamLease L;
  if (L.acquire(in->device)) return 1;
  hipStream_t st = L.stream;
  DevScope B;
  // the cloud's bounding box (k_chunk_bounds of the grid builder), then min_b / max_b = the cell of its corners: x -> floor(fl32(x * inv)) is monotonic
  float box_lo[3], box_hi[3];
  if (er::cloud_bounds(in, st, box_lo, box_hi)) return 1;
  VoxDims V;
  V.inv = 1.0f / leaf;
  double cells = 1.0;
  for (int a = 0; a < 3; a++) {
    const float lo = box_lo[a], hi = box_hi[a];
    if (!(std::fabs((double)(lo * V.inv)) < 2.0e9) || !(std::fabs((double)(hi * V.inv)) < 2.0e9))
      return er::fail("er_cloud_voxel_grid: leaf %g is too small for this cloud: the cell indices overflow an int (PCL returns the cloud unfiltered)", (double)leaf);
    V.min_b[a] = er_fp::voxel_index(lo, V.inv);
    const long d = (long)er_fp::voxel_index(hi, V.inv) - (long)V.min_b[a] + 1;
    V.div[a] = (int)std::min<long>(d, INT_MAX);
    cells *= (double)d;
  }
  if (cells > (double)INT_MAX)
    return er::fail("er_cloud_voxel_grid: leaf %g is too small for this cloud: %.0f cells exceed INT_MAX (PCL returns the cloud unfiltered)", (double)leaf, cells);
  int bits = 1;
  while (bits < 31 && (1L << bits) < (long)cells) bits++;
  unsigned *k0, *k1, *x0, *x1;
  int *head, *seg;
  if (B.alloc(&k0, (size_t)n, "er_cloud_voxel_grid")) return 1;
  if (B.alloc(&k1, (size_t)n, "er_cloud_voxel_grid")) return 1;
  if (B.alloc(&x0, (size_t)n, "er_cloud_voxel_grid")) return 1;
  if (B.alloc(&x1, (size_t)n, "er_cloud_voxel_grid")) return 1;
  if (B.alloc(&head, (size_t)n, "er_cloud_voxel_grid")) return 1;
  if (B.alloc(&seg, (size_t)n, "er_cloud_voxel_grid")) return 1;
  size_t need_sort = 0, need_scan = 0;
  ER_HIP_TRY(er::sort_pairs_u32(nullptr, need_sort, k0, k1, x0, x1, n, 0, bits, st));
  ER_HIP_TRY(er::inclusive_sum_i32(nullptr, need_scan, head, seg, n, st));
  size_t tmp_bytes = std::max(need_sort, need_scan);
  char* tmp;
  if (B.alloc(&tmp, tmp_bytes, "er_cloud_voxel_grid")) return 1;
  hipLaunchKernelGGL(k_vox_keys, dim3(nblocks_of(n)), dim3(kBlock), 0, st, in->xyz, n, V, k0, x0);
  size_t t = tmp_bytes;
  ER_HIP_TRY(er::sort_pairs_u32(tmp, t, k0, k1, x0, x1, n, 0, bits, st));       // stable: a cell's members stay in file order
  hipLaunchKernelGGL(k_vox_heads, dim3(nblocks_of(n)), dim3(kBlock), 0, st, k1, n, head);
  t = tmp_bytes;
  ER_HIP_TRY(er::inclusive_sum_i32(tmp, t, head, seg, n, st));
  ER_HIP_TRY(hipGetLastError());
  int m = 0;
  ER_HIP_TRY(hipMemcpyAsync(&m, seg + (n - 1), sizeof(int), hipMemcpyDeviceToHost, st));
  ER_HIP_TRY(hipStreamSynchronize(st));
  if (m < 1 || m > n) return er::fail("er_cloud_voxel_grid: internal error (%d cells of %d points)", m, n);
  int* start;
  float *oxyz, *onrm;
  if (B.alloc(&start, (size_t)m + 1, "er_cloud_voxel_grid")) return 1;
  if (B.alloc(&oxyz, (size_t)m * 3, "er_cloud_voxel_grid")) return 1;
  if (B.alloc(&onrm, (size_t)m * 3, "er_cloud_voxel_grid")) return 1;
  hipLaunchKernelGGL(k_vox_starts, dim3(nblocks_of(n)), dim3(kBlock), 0, st, k1, seg, n, m, start);
  hipLaunchKernelGGL(k_vox_mean, dim3(nblocks_of(m)), dim3(kBlock), 0, st, in->xyz, in->nrm, x1, start, m, oxyz, onrm);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipStreamSynchronize(st));
  if (er::cloud_create_device(oxyz, onrm, m, grid_cell, in->device, out)) return 1;
  if (n_out) *n_out = m;
  return 0;
}

int er_cloud_estimate_normals(er_cloud_t in, float radius, er_cloud_t* out, int* n_neighbours_host) {
  if (!out) return er::fail("er_cloud_estimate_normals: out is NULL");
  *out = nullptr;
  if (no_device("er_cloud_estimate_normals")) return 1;
  if (fp_check_cloud(in, "er_cloud_estimate_normals")) return 1;
  if (fp_bad_length(radius)) return er::fail("er_cloud_estimate_normals: radius %g must be positive and finite", (double)radius);
  const int n = in->n;
  CloudHolder T;
  if (fp_radius_grid(in, radius, &T, "er_cloud_estimate_normals")) return 1;
  StreamLease L;
  if (L.acquire(in->device)) return 1;
  hipStream_t st = L.stream;
  DevScope B;
  float* nrm;
  int* nn;
  if (B.alloc(&nrm, (size_t)n * 3, "er_cloud_estimate_normals")) return 1;
  if (B.alloc(&nn, (size_t)n, "er_cloud_estimate_normals")) return 1;
  hipLaunchKernelGGL(k_fp_normals, dim3(fp_blocks(n)), dim3(kBlock), 0, st, T.c->xn, n, T.c->grid, radius * radius, nrm, nn);
  ER_HIP_TRY(hipGetLastError());
  if (n_neighbours_host) ER_HIP_TRY(hipMemcpyAsync(n_neighbours_host, nn, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  ER_HIP_TRY(hipStreamSynchronize(st));
  return er::cloud_create_device(in->xyz, nrm, n, in->radius_cap, in->device, out);
}

int er_fpfh_estimate(er_cloud_t c, float radius, er_features_t* out, int* spfh_counts_host, int* n_neighbours_host) {
  if (!out) return er::fail("er_fpfh_estimate: out is NULL");
  *out = nullptr;
  if (no_device("er_fpfh_estimate")) return 1;
  if (fp_check_cloud(c, "er_fpfh_estimate")) return 1;
  if (fp_bad_length(radius)) return er::fail("er_fpfh_estimate: radius %g must be positive and finite", (double)radius);
  const int n = c->n;
  CloudHolder T;
  if (fp_radius_grid(c, radius, &T, "er_fpfh_estimate")) return 1;
  StreamLease L;
  if (L.acquire(c->device)) return 1;
  hipStream_t st = L.stream;
  DevScope B;
  int *counts, *nn;
  if (B.alloc(&counts, (size_t)n * er_fp::kDim, "er_fpfh_estimate")) return 1;
  if (B.alloc(&nn, (size_t)n, "er_fpfh_estimate")) return 1;
  er_features_s* f = new er_features_s();
  f->device = c->device; f->n = n; f->dim = er_fp::kDim; f->dp = (er_fp::kDim + 7) / 8 * 8;
  const size_t fbytes = (size_t)n * f->dp * sizeof(float);
  if (f->d.reserve((size_t)n * f->dp, "er_fpfh_estimate")) {
    delete f;
    return 1;
  }
  const float r2 = radius * radius;
  hipError_t e = hipMemsetAsync(f->d, 0, fbytes, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fp_spfh, dim3(fp_blocks(n)), dim3(kBlock), 0, st, T.c->xn, n, T.c->grid, r2, counts, nn);
    hipLaunchKernelGGL(k_fp_fpfh, dim3(fp_blocks(n)), dim3(kBlock), 0, st, T.c->xn, n, T.c->grid, r2, counts, nn, f->d, f->dp);
    e = hipGetLastError();
  }
  if (e == hipSuccess && spfh_counts_host)
    e = hipMemcpyAsync(spfh_counts_host, counts, (size_t)n * er_fp::kDim * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_neighbours_host) e = hipMemcpyAsync(n_neighbours_host, nn, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    delete f;
    return er::fail("er_fpfh_estimate: %s", hipGetErrorString(e));
  }
  *out = f;
  return 0;
}

}  // extern "C"
