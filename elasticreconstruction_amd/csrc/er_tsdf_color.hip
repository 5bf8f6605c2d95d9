// er_tsdf_color.hip -- colour on the resident TSDF volume of path A: per-voxel integer accumulators next to the unit pool, the
// forward splat of registered RGB frames into them, and the colour of a point (a mesh vertex) read back from them.
//
// The accumulators are sums of bytes and a count, added with integer atomics: exact, associative and order independent, so they hold the same
// bits whatever the batch split, the frame order, the stream or the run, and a numpy restatement (tests/color_restatement.py) matches them bit
// for bit.  A voxel is two 64-bit words, (r_sum | g_sum << 32) and (b_sum | n << 32) -- in memory uint32 r_sum, g_sum, b_sum, n -- and a sample
// adds (r | g << 32) and (b | 1 << 32) with one 64-bit atomic each.  A channel sum grows by at most 255 per sample: below 2^24 samples per voxel
// (2^24 * 255 < 2^32) no field carries into its neighbour.  Beyond that the sums are wrong; nothing checks it (a voxel is 6 mm wide: 2^24
// samples are 54 VGA frames that all land in it).
//
// Nothing here touches the sdf pool, the pre-pass buffers (zbuf, lastzero, zfix) or the batch pipeline: the calls run on the handle's stream behind
// the voxel passes (check_flags), read the unit table when nobody inserts, and stage their inputs in scratch of their own.
#include "er_tsdf_dev.h"
#include "er_mesh.h"

#include <cmath>

namespace {

using namespace er_tsdf_k;

constexpr int kColorBatch = 64;                      // frames per launch of k_color_splat (the frame is a grid axis) and per staging round
constexpr double kLatticeLo = -(256.0 * 64.0), kLatticeHi = 256.0 * 64.0;

// One thread per pixel, the frame on grid axis y.  Per pixel ("the splat"):
//   1. d = depth[p] != 0;
//   2. scale_depth_px(d, scale_lambda(u, v), integration_trunc) > 0.001f -- the pixels IntegrateVolumeUnit uses (TSDFVolume.cpp:29, 82);
//   3. the world point by touch_key_exact's float64 chain, the voxel g_a = floor(p_a / kUnitLength + 0.5); outside [-16384, 16384): out_of_range;
//   4. the unit of g through the hash map; none: no_unit;
//   5. (r, g, b, 1) added to voxel (g_a + 16384) & 63.
// The exact chain with its six float64 divisions: only the VOXEL index is observable, but nothing has asked for a faster form yet.
// stats: added, no_unit, out_of_range -- one atomic per wave and counter.
__global__ __launch_bounds__(kBlock) void k_color_splat(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ rgb, int pixels, int cols,
                                                        Camera cam, const double* __restrict__ T16, UnitMap map, int max_units,
                                                        unsigned long long* __restrict__ color, unsigned long long* __restrict__ stats) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  const int f = blockIdx.y;
  int verdict = 0;                                   // 1 added, 2 no unit, 3 out of range
  if (p < pixels) {
    const size_t o = (size_t)f * (size_t)pixels + (size_t)p;
    const uint16_t d = depth[o];
    const int v = p / cols, u = p - v * cols;
    if (d != 0 && scale_depth_px(d, scale_lambda(u, v, cam), cam.integration_trunc) > 0.001f) {
      const double* T = T16 + (size_t)f * 16;
      double x, y, z;
      uvd2xyz(u, v, d, cam, x, y, z);
      const double p0 = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
      const double p1 = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
      const double p2 = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
      const double g0 = floor(p0 / kUnitLength + 0.5), g1 = floor(p1 / kUnitLength + 0.5), g2 = floor(p2 / kUnitLength + 0.5);
      // (tested on the float64 values, before any integer conversion: NaN and overflow fail)
      if (!(g0 >= kLatticeLo && g0 < kLatticeHi && g1 >= kLatticeLo && g1 < kLatticeHi && g2 >= kLatticeLo && g2 < kLatticeHi)) {
        verdict = 3;
      } else {
        const int a0 = (int)g0 + 256 * 64, a1 = (int)g1 + 256 * 64, a2 = (int)g2 + 256 * 64;      // 0 .. 32767
        const int slot = map.slot(unit_key_of(a0, a1, a2));                                         // key_from_voxels
        if ((unsigned)slot >= (unsigned)max_units) {
          verdict = 2;
        } else {
          const size_t l = (size_t)slot * kUnitVox + unit_offset_of(a0, a1, a2);
          const uint8_t* c = rgb + o * 3;
          const unsigned long long rg = (unsigned long long)c[0] | (unsigned long long)c[1] << 32;
          const unsigned long long bn = (unsigned long long)c[2] | 1ull << 32;
          (void)__hip_atomic_fetch_add(&color[2 * l], rg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          (void)__hip_atomic_fetch_add(&color[2 * l + 1], bn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          verdict = 1;
        }
      }
    }
  }
  // every lane of the wave arrives here
  const unsigned long long b1 = __ballot(verdict == 1), b2 = __ballot(verdict == 2), b3 = __ballot(verdict == 3);
  if ((threadIdx.x & 63) == 0) {
    if (b1) atomicAdd(&stats[0], (unsigned long long)__popcll(b1));
    if (b2) atomicAdd(&stats[1], (unsigned long long)__popcll(b2));
    if (b3) atomicAdd(&stats[2], (unsigned long long)__popcll(b3));
  }
}

// The accumulators of voxel (gx, gy, gz) of the 0-based lattice added to s[4] (64-bit r, g, b, n); nothing for a voxel off the lattice or in a unit that does
// not exist.  *key / *slot cache the last unit looked up (a 3 x 3 x 3 neighbourhood spans at most eight).
__device__ __forceinline__ void color_gather(const unsigned long long* __restrict__ color, const UnitMap& map, int max_units, int gx, int gy, int gz,
                                             int* key, int* slot, unsigned long long s[4]) {
  if (!on_lattice(gx, gy, gz)) return;
  const int k = unit_key_of(gx, gy, gz);
  if (k != *key) {
    *key = k;
    *slot = map.slot(k);
  }
  if ((unsigned)*slot >= (unsigned)max_units) return;
  const size_t l = (size_t)*slot * kUnitVox + unit_offset_of(gx, gy, gz);
  const unsigned long long rg = color[2 * l], bn = color[2 * l + 1];
  s[0] += rg & 0xFFFFFFFFull;
  s[1] += rg >> 32;
  s[2] += bn & 0xFFFFFFFFull;
  s[3] += bn >> 32;
}

// One thread per point (x y z, 4th float ignored), as k_surface_normals.  v = rint((double)p / kUnitLength) per component, half to even --
// k_surface_normals' nearest voxel.  Level 0: v itself if it has samples; level 1: the 64-bit sums over the 27 voxels v + {-1, 0, 1}^3 that lie
// on the lattice in existing units, across unit borders.  Channel = (2 sum + n) / (2 n), integer division (round half up), a = 255.
// No sample, a non-finite coordinate or v off the lattice: 0 0 0 0.  counts: points coloured at level 0 and at level 1.
__global__ __launch_bounds__(kBlock) void k_color_sample(const unsigned long long* __restrict__ color, UnitMap map, int max_units,
                                                         const float4* __restrict__ pts, long n, uchar4* __restrict__ out,
                                                         unsigned long long* __restrict__ counts) {
  const long r = (long)blockIdx.x * kBlock + threadIdx.x;
  int level = -1;
  if (r < n) {
    const float4 p = pts[r];
    const double v0 = rint((double)p.x / kUnitLength), v1 = rint((double)p.y / kUnitLength), v2 = rint((double)p.z / kUnitLength);
    unsigned long long s[4] = {0, 0, 0, 0};
    // (a NaN or an infinite coordinate fails the comparisons)
    if (v0 >= kLatticeLo && v0 < kLatticeHi && v1 >= kLatticeLo && v1 < kLatticeHi && v2 >= kLatticeLo && v2 < kLatticeHi) {
      const int gx = (int)v0 + 256 * 64, gy = (int)v1 + 256 * 64, gz = (int)v2 + 256 * 64;
      int key = -2, slot = -1;
      color_gather(color, map, max_units, gx, gy, gz, &key, &slot, s);
      if (s[3] > 0) {
        level = 0;
      } else {
        for (int dx = -1; dx <= 1; dx++)
          for (int dy = -1; dy <= 1; dy++)
            for (int dz = -1; dz <= 1; dz++) color_gather(color, map, max_units, gx + dx, gy + dy, gz + dz, &key, &slot, s);
        if (s[3] > 0) level = 1;
      }
    }
    uchar4 c = make_uchar4(0, 0, 0, 0);
    if (level >= 0) {
      const unsigned long long d = 2 * s[3];
      c = make_uchar4((unsigned char)((2 * s[0] + s[3]) / d), (unsigned char)((2 * s[1] + s[3]) / d), (unsigned char)((2 * s[2] + s[3]) / d), 255);
    }
    out[r] = c;
  }
  const unsigned long long b0 = __ballot(level == 0), b1 = __ballot(level == 1);
  if ((threadIdx.x & 63) == 0) {
    if (b0) atomicAdd(&counts[0], (unsigned long long)__popcll(b0));
    if (b1) atomicAdd(&counts[1], (unsigned long long)__popcll(b1));
  }
}

// The warped colour image ("the warped colour image").  Z is the frame's reprojected depth image, exactly what er_tsdf_reproject
// returns.  winner(c) = the LOWEST source pixel p with depth[p] != 0 whose reproject_px succeeds with cell c and a depth dd == Z[c] != 0: one pass
// over the source pixels with an atomicMin of p into the cell's word (all ones = no winner), then the gather.  The rule is a definition: it does
// not depend on the order in which anything runs.  A is the frame's ReprojArgs (n_frames == 1).
__global__ __launch_bounds__(kBlock) void k_color_warp(ReprojArgs A, const uint16_t* __restrict__ Z, uint32_t* __restrict__ win) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= A.cols * A.rows) return;
  const uint16_t d = A.depth[p];
  if (d == 0) return;
  const int v = p / A.cols, u = p - v * A.cols;
  int cell;
  uint16_t dd;
  if (!reproject_px(u, v, d, A.cam, A.cami, A.cols, A.rows, A.seg12, A.madj12, A.ctr + (size_t)A.grid_index[0] * A.floats_per_grid, A.res, A.grid_ul,
                    cell, dd))
    return;
  if (dd != 0 && dd == Z[cell]) atomicMin(&win[cell], (uint32_t)p);
}

// C'[c] = C[winner(c)], 0 0 0 where there is none (then Z[c] == 0); re-arms the winner word.
__global__ __launch_bounds__(kBlock) void k_color_gather(const uint8_t* __restrict__ rgb, uint32_t* __restrict__ win, uint8_t* __restrict__ out, int pixels) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= pixels) return;
  const uint32_t w = win[c];
  win[c] = kZEmpty;
  const bool has = w < (uint32_t)pixels;
  const uint8_t* s = rgb + (size_t)(has ? w : 0u) * 3;
  out[(size_t)c * 3 + 0] = has ? s[0] : (uint8_t)0;
  out[(size_t)c * 3 + 1] = has ? s[1] : (uint8_t)0;
  out[(size_t)c * 3 + 2] = has ? s[2] : (uint8_t)0;
}

// The colour twin of k_zero_units: 4 MiB per unit, one uint4 (= one voxel) per thread.
__global__ __launch_bounds__(256) void k_zero_unit_colors(unsigned long long* __restrict__ color, const int* __restrict__ slots, int max_units) {
  const int slot = slots[blockIdx.y];
  if ((unsigned)slot >= (unsigned)max_units) return;
  uint4* __restrict__ u = reinterpret_cast<uint4*>(color + (size_t)slot * kUnitVox * 2);
  u[blockIdx.x * 256 + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

int ensure_color_scratch(er_tsdf_t h, size_t bytes) {
  if (h->color_scratch.reserve(bytes, "colour staging")) {
    (void)hipGetLastError();
    return er::fail("colour staging: cannot allocate %zu bytes of device memory", bytes);
  }
  return 0;
}

// What every colour call but er_tsdf_color_enable checks first.
int color_ready(er_tsdf_t h, const char* who) {
  if (!h->color) return er::fail("%s: colour is not enabled on this volume (er_tsdf_color_enable)", who);
  if (h->shard_world > 1) return er::fail("%s: colour is not carried across GPUs (er_tsdf_set_unit_shard has world = %d)", who, h->shard_world);
  return 0;
}

// The pool slot of an existing unit, for the two single-unit transfers.
int unit_slot(er_tsdf_t h, const char* who, int key, int* slot) {
  if (check_flags(h)) return 1;
  if (std::binary_search(h->dropped.begin(), h->dropped.end(), key)) return er::fail("%s: unit %d was handed to its owner by the last merge", who, key);
  if (resolve_slots(h, &key, 1, false)) return 1;
  *slot = -1;
  ER_HIP_TRY(hipMemcpyAsync(slot, h->slot_scratch, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  if (*slot < 0 || *slot >= h->max_units) return er::fail("%s: no unit with key %d", who, key);
  return 0;
}

// The frames of a colour call: staged (host frames, kColorBatch at a time), warped into the virtual camera if there is a warp, and splatted --
// or, for the single-frame hook er_tsdf_reproject_color (z_host, c_host != NULL; no T), the warped pair copied back instead.
// Everything the warp needs lives in the colour scratch: its own copy of the lattices and per-frame matrices, and its own z-buffer, replay
// buffers, flag words and winner words, armed here and re-armed by their consumers (the z-buffer: emptied by the next frame's epoch tag).  So a pre-pass stream that still works for a later batch
// shares nothing with it.
int color_run(er_tsdf_t h, const char* who, int n, const uint16_t* depth, const uint8_t* rgb, int on_device, const double* T, const er_warp* warp,
              uint16_t* z_host, uint8_t* c_host, long stats[3]) {
  if (warp && (!warp->ctr || !warp->grid_index || !warp->seg || !warp->madj || warp->num_grids <= 0 || warp->resolution <= 0))
    return er::fail("%s: incomplete er_warp", who);
  if (check_flags(h)) return 1;                      // behind the voxel passes, whose pre-passes created the units; nobody inserts from here on
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (n == 0) return 0;
  const size_t px = (size_t)h->pixels;
  const int nb_max = std::min(n, kColorBatch);
  const size_t verts = warp ? (size_t)(warp->resolution + 1) * (warp->resolution + 1) * (warp->resolution + 1) : 0;
  const size_t ctr_floats = warp ? verts * 3 * (size_t)warp->num_grids : 0;
  // scratch: counters | flag words | T | [depth | rgb of a batch, for host frames] | [seg | madj | grid index | lattices | zbuf | lastzero | zfix | winners | Z | C']
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t o = off; off += round256(bytes); return o; };
  const size_t o_stats = take(3 * sizeof(unsigned long long)), o_flag = take(2 * sizeof(int)), o_T = take((size_t)n * 16 * sizeof(double));
  const size_t o_d = take(on_device ? 0 : (size_t)nb_max * px * sizeof(uint16_t)), o_c = take(on_device ? 0 : (size_t)nb_max * px * 3);
  const size_t o_seg = take(warp ? (size_t)n * 16 * sizeof(double) : 0), o_madj = take(warp ? (size_t)n * 12 * sizeof(double) : 0);
  const size_t o_gi = take(warp ? (size_t)n * sizeof(int) : 0), o_ctr = take(ctr_floats * sizeof(float));
  const size_t o_zbuf = take(warp ? px * 4 : 0), o_lz = take(warp ? px * 4 : 0), o_zfix = take(warp ? px * 4 : 0), o_win = take(warp ? px * 4 : 0);
  const size_t o_Z = take(warp ? px * sizeof(uint16_t) : 0), o_C = take(warp ? px * 3 : 0);
  if (ensure_color_scratch(h, off)) return 1;
  char* S = h->color_scratch;
  hipStream_t X = h->stream;
  unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(S + o_stats);
  double* d_T = reinterpret_cast<double*>(S + o_T);
  ER_HIP_TRY(hipMemsetAsync(d_stats, 0, 3 * sizeof(unsigned long long), X));
  if (T) ER_HIP_TRY(hipMemcpyAsync(d_T, T, (size_t)n * 16 * sizeof(double), hipMemcpyHostToDevice, X));
  std::vector<double> seg16, madj12;                 // (alive until the stream has been synchronised below)
  if (warp) {
    seg16.assign((size_t)n * 16, 0.0);
    madj12.resize((size_t)n * 12);
    for (int f = 0; f < n; f++) {
      memcpy(&seg16[(size_t)f * 16], warp->seg + (size_t)f * 16, 12 * sizeof(double));
      memcpy(&madj12[(size_t)f * 12], warp->madj + (size_t)f * 16, 12 * sizeof(double));
      er::cube_coord_deltas(&seg16[(size_t)f * 16], h->cam, h->cols, h->rows, &seg16[(size_t)f * 16 + 12]);
      const int g = warp->grid_index[f];
      if (g < 0 || g >= warp->num_grids) return er::fail("%s: frame %d: control grid index %d out of [0,%d)", who, f, g, warp->num_grids);
    }
    ER_HIP_TRY(hipMemcpyAsync(S + o_seg, seg16.data(), seg16.size() * sizeof(double), hipMemcpyHostToDevice, X));
    ER_HIP_TRY(hipMemcpyAsync(S + o_madj, madj12.data(), madj12.size() * sizeof(double), hipMemcpyHostToDevice, X));
    ER_HIP_TRY(hipMemcpyAsync(S + o_gi, warp->grid_index, (size_t)n * sizeof(int), hipMemcpyHostToDevice, X));
    ER_HIP_TRY(hipMemcpyAsync(S + o_ctr, warp->ctr, ctr_floats * sizeof(float), hipMemcpyHostToDevice, X));
    ER_HIP_TRY(hipMemsetAsync(S + o_flag, 0, 2 * sizeof(int), X));
    ER_HIP_TRY(hipMemsetAsync(S + o_zbuf, 0xFF, px * 4, X));            // kZEmpty: above every epoch's tag (the scratch moves from call to call)
    ER_HIP_TRY(hipMemsetAsync(S + o_lz, 0, px * 4, X));
    ER_HIP_TRY(hipMemsetAsync(S + o_zfix, 0xFF, px * 4, X));
    ER_HIP_TRY(hipMemsetAsync(S + o_win, 0xFF, px * 4, X));
  }
  const unsigned blocks = (unsigned)((px + kBlock - 1) / kBlock);
  for (int start = 0; start < n; start += kColorBatch) {
    const int nb = std::min(kColorBatch, n - start);
    const uint16_t* dd = depth + (size_t)start * px;
    const uint8_t* dc = rgb + (size_t)start * px * 3;
    if (!on_device) {
      // (pageable copies have left the caller's memory when hipMemcpyAsync returns; the staging's reuse is ordered by the stream)
      ER_HIP_TRY(hipMemcpyAsync(S + o_d, dd, (size_t)nb * px * sizeof(uint16_t), hipMemcpyHostToDevice, X));
      ER_HIP_TRY(hipMemcpyAsync(S + o_c, dc, (size_t)nb * px * 3, hipMemcpyHostToDevice, X));
      dd = reinterpret_cast<const uint16_t*>(S + o_d);
      dc = reinterpret_cast<const uint8_t*>(S + o_c);
    }
    if (!warp) {
      hipLaunchKernelGGL(k_color_splat, dim3(blocks, (unsigned)nb), dim3(kBlock), 0, X, dd, dc, h->pixels, h->cols, h->cam, d_T + (size_t)start * 16,
                         h->view().map, h->max_units, h->color, d_stats);
      ER_HIP_TRY(hipGetLastError());
      continue;
    }
    uint16_t* Z = reinterpret_cast<uint16_t*>(S + o_Z);
    uint8_t* Cw = reinterpret_cast<uint8_t*>(S + o_C);
    uint32_t* win = reinterpret_cast<uint32_t*>(S + o_win);
    for (int f = 0; f < nb; f++) {                   // one frame at a time through the single-frame z-buffer
      const size_t F = (size_t)(start + f);
      uint32_t ztag = 0;                             // the frame's own epoch: the z-buffer is not re-armed between frames (er_tsdf.h: kZEpochMax)
      if (next_ztag(h, kZColor, reinterpret_cast<uint32_t*>(S + o_zbuf), px, X, &ztag)) return 1;
      const ReprojArgs RA{dd + (size_t)f * px, 1, h->cols, h->rows, h->cam, h->cami, reinterpret_cast<const double*>(S + o_seg) + F * 16,
                          reinterpret_cast<const double*>(S + o_madj) + F * 12, reinterpret_cast<const int*>(S + o_gi) + F,
                          reinterpret_cast<const float*>(S + o_ctr), warp->resolution, warp->length / (float)warp->resolution, (int)(verts * 3),
                          reinterpret_cast<uint32_t*>(S + o_zbuf), reinterpret_cast<uint32_t*>(S + o_lz), reinterpret_cast<uint32_t*>(S + o_zfix),
                          reinterpret_cast<int*>(S + o_flag), ztag};
      if (reproject_single(h, RA, Z, X)) return 1;
      hipLaunchKernelGGL(k_color_warp, dim3(blocks), dim3(kBlock), 0, X, RA, Z, win);
      hipLaunchKernelGGL(k_color_gather, dim3(blocks), dim3(kBlock), 0, X, dc + (size_t)f * px * 3, win, Cw, h->pixels);
      ER_HIP_TRY(hipGetLastError());
      if (z_host) {
        ER_HIP_TRY(hipMemcpyAsync(z_host, Z, px * sizeof(uint16_t), hipMemcpyDeviceToHost, X));
        ER_HIP_TRY(hipMemcpyAsync(c_host, Cw, px * 3, hipMemcpyDeviceToHost, X));
      } else {
        hipLaunchKernelGGL(k_color_splat, dim3(blocks, 1u), dim3(kBlock), 0, X, Z, Cw, h->pixels, h->cols, h->cam, d_T + F * 16, h->view().map, h->max_units,
                           h->color, d_stats);
        ER_HIP_TRY(hipGetLastError());
      }
    }
  }
  unsigned long long st[3] = {0, 0, 0};
  ER_HIP_TRY(hipMemcpyAsync(st, d_stats, sizeof st, hipMemcpyDeviceToHost, X));
  ER_HIP_TRY(hipStreamSynchronize(X));
  if (stats)
    for (int k = 0; k < 3; k++) stats[k] = (long)st[k];
  return 0;
}

}  // namespace

namespace er_tsdf_k {

int color_zero_slots(er_tsdf_t h, int n) {
  if (!h->color || n <= 0) return 0;
  hipLaunchKernelGGL(k_zero_unit_colors, dim3(kUnitVox / 256, n), dim3(256), 0, h->stream, h->color, h->slot_scratch, h->max_units);
  ER_HIP_TRY(hipGetLastError());
  return 0;
}

int color_sample_on_device(er_tsdf_t h, const char* who, const float4* d_points, long n, uchar4* d_rgba) {
  if (color_ready(h, who)) return 1;
  if (check_flags(h)) return 1;
  if (n == 0) return 0;
  if (n < 0 || n > 0x7FFFFFFFL) return er::fail("%s: %ld points are more than the 2^31 - 1 a colour call takes", who, n);
  if (ensure_color_scratch(h, 256)) return 1;                // (the level counts, which nobody reads here)
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(h->color_scratch.get());
  ER_HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(k_color_sample, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->color, h->view().map, h->max_units,
                     d_points, n, d_rgba, d_counts);
  ER_HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace er_tsdf_k

extern "C" {

int er_tsdf_color_enable(er_tsdf_t h) {
  if (!h) return er::fail("er_tsdf_color_enable: NULL handle");
  if (h->shard_world > 1) return er::fail("er_tsdf_color_enable: colour is not carried across GPUs (er_tsdf_set_unit_shard has world = %d)", h->shard_world);
  if (h->color) return 0;
  ER_HIP_TRY(hipSetDevice(h->device));
  const size_t bytes = (size_t)h->max_units * kUnitVox * 16;
  if (h->color.reserve(bytes / sizeof(unsigned long long), "er_tsdf_color_enable")) {
    (void)hipGetLastError();
    return er::fail("er_tsdf_color_enable: cannot allocate %zu bytes of device memory for the colour of %d units", bytes, h->max_units);
  }
  if (hipMemsetAsync(h->color, 0, bytes, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
    (void)hipGetLastError();
    h->color.reset();                                          // (enabled only once the block is zero)
    return er::fail("er_tsdf_color_enable: cannot zero %zu bytes of device memory", bytes);
  }
  return 0;
}

int er_tsdf_read_unit_color(er_tsdf_t h, int key, uint32_t* rgbn_host) {
  if (!h || !rgbn_host) return er::fail("er_tsdf_read_unit_color: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  int slot;
  if (color_ready(h, "er_tsdf_read_unit_color") || unit_slot(h, "er_tsdf_read_unit_color", key, &slot)) return 1;
  ER_HIP_TRY(hipMemcpyAsync(rgbn_host, h->color + (size_t)slot * kUnitVox * 2, (size_t)kUnitVox * 16, hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int er_tsdf_write_unit_color(er_tsdf_t h, int key, const uint32_t* rgbn_host) {
  if (!h || !rgbn_host) return er::fail("er_tsdf_write_unit_color: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  int slot;
  if (color_ready(h, "er_tsdf_write_unit_color") || unit_slot(h, "er_tsdf_write_unit_color", key, &slot)) return 1;
  ER_HIP_TRY(hipMemcpyAsync(h->color + (size_t)slot * kUnitVox * 2, rgbn_host, (size_t)kUnitVox * 16, hipMemcpyHostToDevice, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int er_tsdf_color_frames(er_tsdf_t h, int n, const uint16_t* depth, const uint8_t* rgb, int on_device, const double* T, const er_warp* warp,
                         long stats[3]) {
  if (!h) return er::fail("er_tsdf_color_frames: NULL handle");
  if (n < 0) return er::fail("er_tsdf_color_frames: negative frame count");
  if (n > 0 && (!depth || !rgb || !T)) return er::fail("er_tsdf_color_frames: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (color_ready(h, "er_tsdf_color_frames")) return 1;
  return color_run(h, "er_tsdf_color_frames", n, depth, rgb, on_device, T, warp, nullptr, nullptr, stats);
}

int er_tsdf_reproject_color(er_tsdf_t h, uint16_t* depth_inout_host, uint8_t* rgb_inout_host, const float* ctr_host, int resolution, float length,
                            const double seg[16], const double madj[16]) {
  if (!h || !depth_inout_host || !rgb_inout_host || !ctr_host || !seg || !madj) return er::fail("er_tsdf_reproject_color: NULL argument");
  if (resolution <= 0) return er::fail("er_tsdf_reproject_color: bad resolution");
  ER_HIP_TRY(hipSetDevice(h->device));
  int gi = 0;
  const er_warp w{ctr_host, 1, resolution, length, &gi, seg, madj};
  return color_run(h, "er_tsdf_reproject_color", 1, depth_inout_host, rgb_inout_host, 0, nullptr, &w, depth_inout_host, rgb_inout_host, nullptr);
}

int er_tsdf_sample_colors(er_tsdf_t h, const float* points_host, long n, uint8_t* rgba_host, long counts[2]) {
  if (!h) return er::fail("er_tsdf_sample_colors: NULL handle");
  if (n < 0) return er::fail("er_tsdf_sample_colors: negative point count");
  if (n > 0 && (!points_host || !rgba_host)) return er::fail("er_tsdf_sample_colors: NULL argument");
  if (n > 0x7FFFFFFFL) return er::fail("er_tsdf_sample_colors: %ld points are more than the 2^31 - 1 a call takes", n);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (color_ready(h, "er_tsdf_sample_colors")) return 1;
  if (check_flags(h)) return 1;
  if (counts) counts[0] = counts[1] = 0;
  if (n == 0) return 0;
  const size_t off_p = 256, off_o = off_p + round256((size_t)n * 16);
  if (ensure_color_scratch(h, off_o + round256((size_t)n * 4))) return 1;
  char* S = h->color_scratch;
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(S);
  ER_HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), h->stream));
  ER_HIP_TRY(hipMemcpyAsync(S + off_p, points_host, (size_t)n * 16, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_color_sample, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->color, h->view().map, h->max_units,
                     reinterpret_cast<const float4*>(S + off_p), n, reinterpret_cast<uchar4*>(S + off_o), d_counts);
  ER_HIP_TRY(hipGetLastError());
  unsigned long long ct[2] = {0, 0};
  ER_HIP_TRY(hipMemcpyAsync(rgba_host, S + off_o, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipMemcpyAsync(ct, d_counts, sizeof ct, hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  if (counts) {
    counts[0] = (long)ct[0];
    counts[1] = (long)ct[1];
  }
  return 0;
}

}  // extern "C"
