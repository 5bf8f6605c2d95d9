// er_odom.hip -- depth odometry of liber_hip.so on MI355X (gfx950): KinFu-style projective point-to-plane ICP between depth frames, batched over
// a pair list.  The reference tree has no KinFu (it lives in the author's PCL fork); what is restated here is
// tests/odometry_restatement.py, and nothing in this file is checked against PCL.  The per-pixel arithmetic is er_odom_math.h.
//
// Frames live in SLOTS of one slab (the "window"): per slot the raw frame, the filtered depth pyramid and, per level, a map of 32-byte records
// {vertex | normal} -- what one projective match gathers from the model is ONE record, as `xn` is for k_icp_iter.  The model side of a pair is
// nothing but "a record map with a pose": a ray-cast map takes a slot with no kernel change -- er_frame_to_model_align copies the record maps
// of er_tsdf_raycast (one per level) into a slot that is never preprocessed and aligns every frame of a list against it;
// er_frames_to_models_align does the same with n_models models, a slot each, and one of them per frame.
//   k_odom_bilateral  raw -> level 0 (13 x 13 bilateral filter, weights from two tables staged in LDS; depth limit)       blockIdx.y = frame
//   k_odom_pyr        level l -> l + 1 (5 x 5 integer mean of the taps near the centre)                                   blockIdx.y = frame
//   k_odom_maps       depth level -> records                                                                             blockIdx.y = frame
//   k_odom_iter       one iteration of every pair: projective match + 27 float64 sums of exact products + count           blockIdx.y = pair
//                     (kPix pixels per thread -> wave shuffle -> LDS -> ONE partial vector per workgroup; no float atomics)
//   k_odom_final      one workgroup per pair: fixed-order total, 6 x 6 float64 Cholesky, pose update, lost rule -- the loop stays on the device
// The partition of a level's pixels into workgroups depends on (cols, rows, level) only and every sum is added in a fixed order, so a pair's
// result is the same bits alone, in any list, in any order, for any window, on any run.  Fixed-order float64 partial sums are enough for that
// (the 128-bit integers of k_icp_iter buy independence from the PARTITION, which is fixed here).
// Reductions and gathers, not contractions: no MFMA.
#include "er_cloud.h"
#include "er_odom_math.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

using namespace er;

namespace {

constexpr int kMaxLevels = 4;
constexpr int kPix = 4;                    // pixels per thread of k_odom_iter: a workgroup takes kPix * kBlock consecutive pixels of the level
constexpr int kPartial = 28;               // doubles per partial vector (27 sums + padding)
constexpr size_t kSlabLimit = (size_t)2 << 30;
constexpr int kMaxWindow = 32768;          // pairs of a run sit on blockIdx.y (at most 65535)

struct Layout {                            // where things are in a slot; by value to every kernel
  char* base;
  size_t stride;                           // slot s starts at base + s * stride
  size_t off_raw, off_depth[kMaxLevels], off_rec[kMaxLevels];
  int cols[kMaxLevels], rows[kMaxLevels];
  er_od::Intr K[kMaxLevels];
};

__device__ __forceinline__ uint16_t* slot_depth(const Layout& L, int slot, int level) {
  return reinterpret_cast<uint16_t*>(L.base + (size_t)slot * L.stride + L.off_depth[level]);
}
__device__ __forceinline__ float4* slot_rec(const Layout& L, int slot, int level) {
  return reinterpret_cast<float4*>(L.base + (size_t)slot * L.stride + L.off_rec[level]);
}

struct Todo { int slot, frame; };          // a frame to preprocess into a slot
struct PairDesc { int mslot, cslot; };

struct OdomState {                         // the loop variables of one pair, on the device from the first to the last iteration
  double R[9], t[3];                       // m_T_c
  int lost, count, pad[2];
};

// raw frame -> level 0.  user_dev != NULL: the caller's frames are in device memory and are read where they are.
__global__ __launch_bounds__(kBlock) void k_odom_bilateral(Layout L, const Todo* __restrict__ todo, const uint16_t* __restrict__ user_dev,
                                                           const float* __restrict__ tables, int n_depth_w, int bilateral, int max_depth_mm) {
  __shared__ float space[er_od::kSpaceW];
  __shared__ float depth_w[er_od::kDepthWMax];
  for (int i = threadIdx.x; i < er_od::kSpaceW; i += kBlock) space[i] = tables[i];
  for (int i = threadIdx.x; i < er_od::kDepthWMax; i += kBlock) depth_w[i] = tables[er_od::kSpaceW + i];
  __syncthreads();
  const Todo td = todo[blockIdx.y];
  const int cols = L.cols[0], rows = L.rows[0], npix = cols * rows;
  const uint16_t* raw = user_dev ? user_dev + (size_t)td.frame * npix : reinterpret_cast<const uint16_t*>(L.base + (size_t)td.slot * L.stride + L.off_raw);
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) {
    int d = bilateral ? er_od::bilateral_pixel(raw, cols, rows, i % cols, i / cols, space, depth_w, n_depth_w) : raw[i];
    if (max_depth_mm > 0 && d > max_depth_mm) d = 0;
    slot_depth(L, td.slot, 0)[i] = (uint16_t)d;
  }
}

__global__ __launch_bounds__(kBlock) void k_odom_pyr(Layout L, const Todo* __restrict__ todo, int level) {   // level -> level + 1
  const Todo td = todo[blockIdx.y];
  const int cols = L.cols[level + 1], npix = cols * L.rows[level + 1];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < npix) slot_depth(L, td.slot, level + 1)[i] = er_od::pyr_down_pixel(slot_depth(L, td.slot, level), L.cols[level], L.rows[level], i % cols, i / cols);
}

__global__ __launch_bounds__(kBlock) void k_odom_maps(Layout L, const Todo* __restrict__ todo, int level) {
  const Todo td = todo[blockIdx.y];
  const int cols = L.cols[level], rows = L.rows[level], npix = cols * rows;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  const uint16_t* depth = slot_depth(L, td.slot, level);
  const er_od::Intr K = L.K[level];
  const int x = i % cols, y = i / cols;
  float4 v, n;
  v.w = n.w = 0.f;
  er_od::vertex(depth[i], x, y, K.fx, K.fy, K.cx, K.cy, v.x, v.y, v.z);
  er_od::normal(depth, cols, rows, x, y, K.fx, K.fy, K.cx, K.cy, n.x, n.y, n.z);
  float4* rec = slot_rec(L, td.slot, level);
  rec[2 * (size_t)i] = v;
  rec[2 * (size_t)i + 1] = n;
}

// One iteration of every pair of the run.  Workgroup b of a pair takes the pixels [b kPix kBlock, (b + 1) kPix kBlock) of the level, thread t the
// pixels b kPix kBlock + j kBlock + t in ascending j; thread sums -> shuffle tree -> the four waves in order.  A lost pair's workgroups leave at once.
__global__ __launch_bounds__(kBlock) void k_odom_iter(Layout L, int level, const PairDesc* __restrict__ pairs, const OdomState* __restrict__ S,
                                                      double* __restrict__ partial, int* __restrict__ pcount, int nblk, float dist_thresh,
                                                      float angle_thresh) {
  const OdomState& st = S[blockIdx.y];
  if (st.lost) return;                                       // wave-uniform, before any barrier
  const PairDesc pd = pairs[blockIdx.y];
  float R[9], t[3];                                          // the float64 state cast to float32 once
#pragma unroll
  for (int q = 0; q < 9; q++) R[q] = (float)st.R[q];
#pragma unroll
  for (int q = 0; q < 3; q++) t[q] = (float)st.t[q];
  const int cols = L.cols[level], rows = L.rows[level], npix = cols * rows;
  const er_od::Intr K = L.K[level];
  const float4* __restrict__ cur = slot_rec(L, pd.cslot, level);
  const float4* __restrict__ model = slot_rec(L, pd.mslot, level);
  double acc[er_od::kSums];
#pragma unroll
  for (int q = 0; q < er_od::kSums; q++) acc[q] = 0.0;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kPix; j++) {
    const int i = (blockIdx.x * kPix + j) * kBlock + (int)threadIdx.x;
    if (i < npix) {
      const float4 v = cur[2 * (size_t)i], n = cur[2 * (size_t)i + 1];
      float a[6], b;
      if (er_od::match_row(R, t, v.x, v.y, v.z, n.x, n.y, n.z, model, cols, rows, K, dist_thresh, angle_thresh, a, b)) {
        double w[er_od::kSums];
        er_od::row_products(a, b, w);
#pragma unroll
        for (int q = 0; q < er_od::kSums; q++) acc[q] += w[q];
        cnt++;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < er_od::kSums; q++)
    for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_down(acc[q], off);
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
  __shared__ double red[kBlock / 64][kPartial];
  __shared__ int redc[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < er_od::kSums; q++) red[wave][q] = acc[q];
    redc[wave] = cnt;
  }
  __syncthreads();
  const size_t slot = (size_t)blockIdx.y * nblk + blockIdx.x;
  if (threadIdx.x < er_od::kSums) partial[slot * kPartial + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  if (threadIdx.x == 32) pcount[slot] = ((redc[0] + redc[1]) + redc[2]) + redc[3];
}

// x = A^-1 b for the symmetric A whose upper triangle is tot[0..20] row by row and b = tot[21..26]: Cholesky A = L L^T with compile-time indices
// (everything stays in registers).  False as soon as a pivot is not positive or anything is not finite.
__device__ bool odom_solve(const double* tot, double x[6]) {
  double a[6][6];
  {
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = r; c < 6; c++) a[r][c] = a[c][r] = tot[k++];
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = a[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) d -= a[j][k] * a[j][k];
    ok = ok && d > 0.0 && isfinite(d);
    const double l = sqrt(d);
    a[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = a[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= a[i][k] * a[j][k];
      a[i][j] = s / l;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {                               // L y = b
    double s = tot[21 + i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= a[i][k] * y[k];
    y[i] = s / a[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {                              // L^T x = y
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) s -= a[k][i] * x[k];
    x[i] = s / a[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) ok = ok && isfinite(x[i]);
  return ok;
}

// The second half of the reduction and the step itself, one workgroup per pair: the partial vectors in a fixed order (8 strided slices per value, then
// the slices in order), then thread 0 decides.  solve = 0 (er_odom_linearize): totals only.  Every thread reaches every barrier, lost pair or not.
__global__ __launch_bounds__(kBlock) void k_odom_final(OdomState* __restrict__ S, const double* __restrict__ partial, const int* __restrict__ pcount, int nblk,
                                                       int min_valid, int solve, double* __restrict__ trace, int trace_len, int trace_at,
                                                       double* __restrict__ sums) {
  OdomState* st = S + blockIdx.x;
  const bool lost = st->lost != 0;
  const int val = threadIdx.x & 31, slice = threadIdx.x >> 5;
  const size_t first = (size_t)blockIdx.x * nblk;
  double q = 0.0;
  int c = 0;
  if (!lost && val < er_od::kSums)
    for (int b = slice; b < nblk; b += 8) q += partial[(first + b) * kPartial + val];
  if (!lost && val == 31)
    for (int b = slice; b < nblk; b += 8) c += pcount[first + b];
  __shared__ double fin[8][32];
  __shared__ int finc[8];
  __shared__ double tot[32];
  fin[slice][val] = q;
  if (val == 31) finc[slice] = c;
  __syncthreads();
  if (threadIdx.x < er_od::kSums) {
    double r = 0.0;
#pragma unroll
    for (int sl = 0; sl < 8; sl++) r += fin[sl][threadIdx.x];
    tot[threadIdx.x] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int count = 0;
    if (!lost) {
#pragma unroll
      for (int sl = 0; sl < 8; sl++) count += finc[sl];
      st->count = count;
      for (int k = 0; k < er_od::kSums; k++) sums[(size_t)blockIdx.x * er_od::kSums + k] = tot[k];
    }
    if (!lost && solve) {
      bool ok = count >= min_valid;
      for (int k = 0; k < er_od::kSums; k++) ok = ok && isfinite(tot[k]);
      double x[6];
      ok = odom_solve(tot, x) && ok;
      double Rn[9], tn[3];
      if (ok) {                                               // Rinc = Rz(gamma) Ry(beta) Rx(alpha); t <- Rinc t + tinc; R <- Rinc R
        double sa, ca, sb, cb, sg, cg;
        sincos(x[0], &sa, &ca);
        sincos(x[1], &sb, &cb);
        sincos(x[2], &sg, &cg);
        const double M[9] = {cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca,
                             sg * cb, cg * ca + sg * sb * sa,  -cg * sa + sg * sb * ca,
                             -sb,     cb * sa,                 cb * ca};
#pragma unroll
        for (int r = 0; r < 3; r++) {
          tn[r] = ((M[3 * r] * st->t[0] + M[3 * r + 1] * st->t[1]) + M[3 * r + 2] * st->t[2]) + x[3 + r];
#pragma unroll
          for (int cc = 0; cc < 3; cc++) Rn[3 * r + cc] = (M[3 * r] * st->R[cc] + M[3 * r + 1] * st->R[3 + cc]) + M[3 * r + 2] * st->R[6 + cc];
        }
        for (int k = 0; k < 9; k++) ok = ok && isfinite(Rn[k]);
        for (int k = 0; k < 3; k++) ok = ok && isfinite(tn[k]);
      }
      if (ok) {
        for (int k = 0; k < 9; k++) st->R[k] = Rn[k];
        for (int k = 0; k < 3; k++) st->t[k] = tn[k];
      } else {
        st->lost = 1;                                         // the pair keeps its last good pose; its remaining launches are empty loops
      }
    }
    if (trace) {
      double* tr = trace + ((size_t)blockIdx.x * trace_len + trace_at) * ER_ODOM_TRACE;
      for (int r = 0; r < 3; r++) {
        for (int cc = 0; cc < 3; cc++) tr[4 * r + cc] = st->R[3 * r + cc];
        tr[4 * r + 3] = st->t[r];
      }
      tr[12] = tr[13] = tr[14] = 0.0;
      tr[15] = 1.0;
      tr[16] = (double)count;
    }
  }
}

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

struct er_odom_s {
  int device = 0, cols = 0, rows = 0;
  er_odom_params P{};
  Layout lo{};
  int total_iters = 0;
  er::DevScope fixed;                      // d_tables
  float* d_tables = nullptr;
  int n_depth_w = 0;
  // the window: slots of the slab and the frame each holds (valid within one call: frames are named by their index into that call's depth array)
  int window = 0;
  std::vector<int> slot_frame;
  // the slab (lo.base) and the per-run workspace, sized for cap_pairs pairs: all in `win`, replaced together when the window grows
  er::DevScope win;
  int cap_pairs = 0;
  Todo* d_todo = nullptr;
  PairDesc* d_pairs = nullptr;
  OdomState* d_state = nullptr;
  double *d_partial = nullptr, *d_trace = nullptr, *d_sums = nullptr;
  int* d_pcount = nullptr;
};

namespace {

int nblk_of(const er_odom_s* h, int level) { return (h->lo.cols[level] * h->lo.rows[level] + kPix * kBlock - 1) / (kPix * kBlock); }

// The slab of `window` slots and a workspace for up to `window` pairs per run (grow-only).
int odom_ensure_window(er_odom_s* h, int window) {
  if (window <= h->window) return 0;
  const char* who = "the depth odometry window";
  const size_t w = (size_t)window, nblk = (size_t)nblk_of(h, 0);
  h->win.free_all();
  h->window = h->cap_pairs = 0;                    // (a failure below leaves no window: the next call starts over)
  if (h->win.alloc(&h->lo.base, h->lo.stride * w, who) || h->win.alloc(&h->d_todo, w, who) || h->win.alloc(&h->d_pairs, w, who) ||
      h->win.alloc(&h->d_state, w, who) || h->win.alloc(&h->d_partial, kPartial * nblk * w, who) || h->win.alloc(&h->d_pcount, nblk * w, who) ||
      h->win.alloc(&h->d_trace, ER_ODOM_TRACE * (size_t)h->total_iters * w, who) || h->win.alloc(&h->d_sums, er_od::kSums * w, who))
    return 1;
  h->window = h->cap_pairs = window;
  h->slot_frame.assign(window, -1);
  return 0;
}

int default_window(const er_odom_s* h) { return (int)std::max<size_t>(2, std::min<size_t>(kSlabLimit / h->lo.stride, kMaxWindow)); }

// The frames of `todo` -> their slots: upload (host frames), filter, pyramid, records.  Everything on `st`; todo must stay alive until st is synchronised.
int odom_preprocess(er_odom_s* h, hipStream_t st, const std::vector<Todo>& todo, const uint16_t* depth, int on_device) {
  const int m = (int)todo.size();
  if (m == 0) return 0;
  const Layout& L = h->lo;
  const size_t npix = (size_t)L.cols[0] * L.rows[0];
  if (!on_device)
    for (const Todo& t : todo)
      ER_HIP_TRY(hipMemcpyAsync(L.base + (size_t)t.slot * L.stride + L.off_raw, depth + (size_t)t.frame * npix, npix * sizeof(uint16_t), hipMemcpyHostToDevice, st));
  ER_HIP_TRY(hipMemcpyAsync(h->d_todo, todo.data(), sizeof(Todo) * m, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_odom_bilateral, dim3(nblocks_of((int)npix), m), dim3(kBlock), 0, st, L, h->d_todo, on_device ? depth : nullptr, h->d_tables,
                     h->n_depth_w, h->P.bilateral, h->P.max_depth_mm);
  for (int l = 0; l + 1 < h->P.levels; l++)
    hipLaunchKernelGGL(k_odom_pyr, dim3(nblocks_of(L.cols[l + 1] * L.rows[l + 1]), m), dim3(kBlock), 0, st, L, h->d_todo, l);
  for (int l = 0; l < h->P.levels; l++)
    hipLaunchKernelGGL(k_odom_maps, dim3(nblocks_of(L.cols[l] * L.rows[l]), m), dim3(kBlock), 0, st, L, h->d_todo, l);
  ER_HIP_TRY(hipGetLastError());
  return 0;
}

void state_from(const double* T, OdomState& s) {
  s = OdomState{};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) s.R[3 * r + c] = T ? T[4 * r + c] : (r == c ? 1.0 : 0.0);
    s.t[r] = T ? T[4 * r + 3] : 0.0;
  }
}

// One run: pairs [p0, p1) of the list, whose frames fit the window.  One stream lease per run.
// model_rec (nullable): the record maps of the MODELS, [model][level] device pointers; the list names model k as frame `n_frames + k`.  A model's
// slot is filled by device-to-device copies instead of the preprocessing, and stays resident from run to run like any frame that is needed again.
int odom_run(er_odom_s* h, const uint16_t* depth, int on_device, int p0, int p1, const int* model_idx, const int* frame_idx, const double* guess,
             double* T_out, int* status, double* trace, double* sums, const void* const* model_rec = nullptr, int n_frames = 0) {
  const int m = p1 - p0;
  std::vector<Todo> todo;                                    // (host buffers of asynchronous copies: declared before the lease, whose destructor drains the stream)
  std::vector<PairDesc> pairs(m);
  std::vector<OdomState> state(m);
  StreamLease lease;
  if (lease.acquire(h->device)) return 1;
  hipStream_t st = lease.stream;
  // slots: a frame that is resident and needed again stays; the others' slots are free
  std::vector<int> needed;
  for (int p = p0; p < p1; p++)
    for (int f : {model_idx[p], frame_idx[p]})
      if (std::find(needed.begin(), needed.end(), f) == needed.end()) needed.push_back(f);
  for (int& f : h->slot_frame)
    if (f >= 0 && std::find(needed.begin(), needed.end(), f) == needed.end()) f = -1;
  auto slot_of = [&](int f) { return (int)(std::find(h->slot_frame.begin(), h->slot_frame.end(), f) - h->slot_frame.begin()); };
  for (int f : needed)
    if (slot_of(f) == (int)h->slot_frame.size()) {
      const int s = slot_of(-1);
      if (s == (int)h->slot_frame.size()) return er::fail("er_odom_align_pairs: internal error, no free slot");
      h->slot_frame[s] = f;
      if (model_rec && f >= n_frames) {
        for (int l = 0; l < h->P.levels; l++)
          ER_HIP_TRY(hipMemcpyAsync(h->lo.base + (size_t)s * h->lo.stride + h->lo.off_rec[l], model_rec[(size_t)(f - n_frames) * h->P.levels + l],
                                    (size_t)h->lo.cols[l] * h->lo.rows[l] * 2 * sizeof(float4), hipMemcpyDeviceToDevice, st));
      } else {
        todo.push_back({s, f});
      }
    }
  if (odom_preprocess(h, st, todo, depth, on_device)) return 1;
  for (int q = 0; q < m; q++) {
    pairs[q] = {slot_of(model_idx[p0 + q]), slot_of(frame_idx[p0 + q])};
    state_from(guess ? guess + (size_t)(p0 + q) * 16 : nullptr, state[q]);
  }
  ER_HIP_TRY(hipMemcpyAsync(h->d_pairs, pairs.data(), sizeof(PairDesc) * m, hipMemcpyHostToDevice, st));
  ER_HIP_TRY(hipMemcpyAsync(h->d_state, state.data(), sizeof(OdomState) * m, hipMemcpyHostToDevice, st));
  ER_HIP_TRY(hipMemsetAsync(h->d_sums, 0, sizeof(double) * er_od::kSums * m, st));
  int at = 0;
  for (int l = h->P.levels - 1; l >= 0; l--) {
    const int nblk = nblk_of(h, l);
    for (int it = 0; it < h->P.iterations[l]; it++, at++) {
      hipLaunchKernelGGL(k_odom_iter, dim3(nblk, m), dim3(kBlock), 0, st, h->lo, l, h->d_pairs, h->d_state, h->d_partial, h->d_pcount, nblk,
                         h->P.dist_thresh, h->P.angle_thresh);
      hipLaunchKernelGGL(k_odom_final, dim3(m), dim3(kBlock), 0, st, h->d_state, h->d_partial, h->d_pcount, nblk, h->P.min_valid, 1,
                         trace ? h->d_trace : nullptr, h->total_iters, at, h->d_sums);
    }
  }
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipMemcpyAsync(state.data(), h->d_state, sizeof(OdomState) * m, hipMemcpyDeviceToHost, st));
  if (trace && h->total_iters > 0)
    ER_HIP_TRY(hipMemcpyAsync(trace + (size_t)p0 * h->total_iters * ER_ODOM_TRACE, h->d_trace, sizeof(double) * ER_ODOM_TRACE * h->total_iters * m,
                              hipMemcpyDeviceToHost, st));
  if (sums) ER_HIP_TRY(hipMemcpyAsync(sums + (size_t)p0 * er_od::kSums, h->d_sums, sizeof(double) * er_od::kSums * m, hipMemcpyDeviceToHost, st));
  ER_HIP_TRY(hipStreamSynchronize(st));
  for (int q = 0; q < m; q++) {
    double* T = T_out + (size_t)(p0 + q) * 16;
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) T[4 * r + c] = state[q].R[3 * r + c];
      T[4 * r + 3] = state[q].t[r];
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
    status[p0 + q] = state[q].lost ? ER_ODOM_LOST : ER_ODOM_OK;
  }
  return 0;
}

int odom_align(er_odom_s* h, const char* who, int n_frames, const uint16_t* depth, int on_device, int n_pairs, const int* model_idx,
               const int* frame_idx, const double* guess, double* T_out, int* status, double* trace, double* sums, int window,
               const void* const* model_rec = nullptr, int n_models = 0) {
  const int n_things = n_frames + (model_rec ? n_models : 0);      // a model is one more thing that needs a slot: model k is "frame" n_frames + k of the list
  if (window == 0) window = default_window(h);
  if (window < 2) return er::fail("%s: window = %d, must be at least 2 (or 0 for the default)", who, window);
  for (int p = 0; p < n_pairs; p++)
    if (model_idx[p] < 0 || model_idx[p] >= n_things || frame_idx[p] < 0 || frame_idx[p] >= n_frames)
      return er::fail("%s: pair %d names frames (%d, %d) outside the %d frames given", who, p, model_idx[p], frame_idx[p], n_frames);
  ER_HIP_TRY(hipSetDevice(h->device));
  window = std::min(std::min(window, kMaxWindow), std::max(n_things, 2));      // (a result does not depend on the window)
  // The slab holds exactly `window` slots for this call, whatever an earlier call left (the cut of the list depends on the window alone).
  if (odom_ensure_window(h, window)) return 1;
  h->slot_frame.assign(h->window, -1);
  for (int s = window; s < h->window; s++) h->slot_frame[s] = -2;      // slots beyond this call's window are not used
  int p0 = 0;
  while (p0 < n_pairs) {
    std::vector<int> frames;
    int p1 = p0;
    while (p1 < n_pairs && p1 - p0 < window) {
      int extra = 0;
      if (std::find(frames.begin(), frames.end(), model_idx[p1]) == frames.end()) extra++;
      if (frame_idx[p1] != model_idx[p1] && std::find(frames.begin(), frames.end(), frame_idx[p1]) == frames.end()) extra++;
      if ((int)frames.size() + extra > window) break;
      for (int f : {model_idx[p1], frame_idx[p1]})
        if (std::find(frames.begin(), frames.end(), f) == frames.end()) frames.push_back(f);
      p1++;
    }
    if (odom_run(h, depth, on_device, p0, p1, model_idx, frame_idx, guess, T_out, status, trace, sums, model_rec, n_frames)) return 1;
    p0 = p1;
  }
  return 0;
}

}  // namespace

// The general form behind er_frames_to_models_align, for the fragment builder (er_fragments.hip): any pair list whose model side names models.
int er::odom_align_models(er_odom_s* h, const char* who, int n_models, const void* const* model_rec_dev, int n_frames, const uint16_t* depth,
                          int on_device, int n_pairs, const int* model_idx, const int* frame_idx, const double* guess, double* T_out, int* status,
                          double* trace, double* sums, int window) {
  for (int k = 0; k < n_models; k++)
    for (int l = 0; l < h->P.levels; l++)
      if (!model_rec_dev[(size_t)k * h->P.levels + l]) return er::fail("%s: model %d has no record map for level %d of %d", who, k, l, h->P.levels);
  if (n_pairs > 0 && (!T_out || !status)) return er::fail("%s: T_out or status is NULL", who);
  if (window < 0) return er::fail("%s: window = %d, must be at least 2 (or 0 for the default)", who, window);
  return odom_align(h, who, n_frames, depth, on_device, n_pairs, model_idx, frame_idx, guess, T_out, status, trace, sums, window, model_rec_dev, n_models);
}
int er::odom_levels(er_odom_s* h) { return h->P.levels; }

extern "C" {

int er_odom_params_default(er_odom_params* p) {
  if (!p) return er::fail("er_odom_params_default: params is NULL");
  p->levels = 3;
  p->iterations[0] = 10;
  p->iterations[1] = 5;
  p->iterations[2] = 4;
  p->iterations[3] = 4;
  p->bilateral = 1;
  p->max_depth_mm = 0;
  p->min_valid = 50;
  p->dist_thresh = 0.10f;
  p->angle_thresh = 0.3420201433256687f;   // sin 20 deg
  return 0;
}

int er_odom_tables(float* space, float* depth_w, int* n_depth_w) {
  if (!space || !depth_w || !n_depth_w) return er::fail("er_odom_tables: NULL argument");
  float s[er_od::kSpaceW], d[er_od::kDepthWMax];
  *n_depth_w = er_od::build_tables(s, d);
  std::copy(s, s + er_od::kSpaceW, space);
  std::copy(d, d + *n_depth_w, depth_w);
  return 0;
}

int er_odom_create(int cols, int rows, const float* cam4, const er_odom_params* params, int device, er_odom_t* out) {
  if (!out) return er::fail("er_odom_create: out is NULL");
  *out = nullptr;
  if (no_device("er_odom_create")) return 1;
  if (!cam4) return er::fail("er_odom_create: cam4 is NULL");
  er_odom_params P;
  er_odom_params_default(&P);
  if (params) P = *params;
  if (P.levels < 1 || P.levels > kMaxLevels) return er::fail("er_odom_create: levels = %d, must be 1 .. 4", P.levels);
  const int div = 1 << (P.levels - 1);
  if (cols <= 0 || cols % div || cols > 16384) return er::fail("er_odom_create: cols = %d must be positive and divisible by %d (2^(levels-1))", cols, div);
  if (rows <= 0 || rows % div || rows > 16384) return er::fail("er_odom_create: rows = %d must be positive and divisible by %d (2^(levels-1))", rows, div);
  for (int l = 0; l < P.levels; l++)
    if (P.iterations[l] < 0 || P.iterations[l] > 1000) return er::fail("er_odom_create: iterations[%d] = %d, must be 0 .. 1000", l, P.iterations[l]);
  if (!(P.dist_thresh > 0.f) || !(P.angle_thresh > 0.f)) return er::fail("er_odom_create: dist_thresh and angle_thresh must be positive");
  if (P.max_depth_mm < 0 || P.min_valid < 0) return er::fail("er_odom_create: max_depth_mm and min_valid must not be negative");
  for (int q = 0; q < 4; q++)
    if (!std::isfinite(cam4[q])) return er::fail("er_odom_create: cam4[%d] is not finite", q);
  if (!(cam4[0] > 0.f) || !(cam4[1] > 0.f)) return er::fail("er_odom_create: cam4 focal lengths must be positive");
  int ndev = 0;
  ER_HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return er::fail("er_odom_create: device %d of %d", device, ndev);
  ER_HIP_TRY(hipSetDevice(device));
  er_odom_s* h = new er_odom_s;
  h->device = device;
  h->cols = cols;
  h->rows = rows;
  h->P = P;
  Layout& L = h->lo;
  size_t off = 0;
  L.off_raw = off;
  off = align_up(off + (size_t)cols * rows * sizeof(uint16_t));
  for (int l = 0; l < P.levels; l++) {
    L.cols[l] = cols >> l;
    L.rows[l] = rows >> l;
    const float s = (float)(1 << l);                                     // (a power of two: the divisions are exact)
    L.K[l] = {cam4[0] / s, cam4[1] / s, cam4[2] / s, cam4[3] / s};
    L.off_depth[l] = off;
    off = align_up(off + (size_t)L.cols[l] * L.rows[l] * sizeof(uint16_t));
    L.off_rec[l] = off;
    off = align_up(off + (size_t)L.cols[l] * L.rows[l] * 2 * sizeof(float4));
    h->total_iters += P.iterations[l];
  }
  L.stride = off;
  float tab[er_od::kSpaceW + er_od::kDepthWMax];
  h->n_depth_w = er_od::build_tables(tab, tab + er_od::kSpaceW);
  if (h->fixed.alloc(&h->d_tables, sizeof tab / sizeof tab[0], "er_odom_create")) {
    delete h;
    return 1;
  }
  const hipError_t e = hipMemcpy(h->d_tables, tab, sizeof tab, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete h;
    return er::fail("er_odom_create: %s", hipGetErrorString(e));
  }
  *out = h;
  return 0;
}

int er_odom_destroy(er_odom_t h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  h->win.free_all();
  h->fixed.free_all();
  delete h;
  return 0;
}

int er_odom_align_pairs(er_odom_t h, int n_frames, const uint16_t* depth, int depth_on_device, int n_pairs, const int* model_idx,
                        const int* frame_idx, const double* guess, double* T_out, int* status, double* trace, double* sums, int window) {
  const char* who = "er_odom_align_pairs";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  if (n_pairs < 0) return er::fail("%s: n_pairs = %d is negative", who, n_pairs);
  if (n_frames < 1 || !depth) return er::fail("%s: depth is NULL or n_frames = %d is not positive", who, n_frames);
  if (n_pairs > 0 && (!model_idx || !frame_idx)) return er::fail("%s: model_idx or frame_idx is NULL", who);
  if (n_pairs > 0 && !T_out) return er::fail("%s: T_out is NULL", who);
  if (n_pairs > 0 && !status) return er::fail("%s: status is NULL", who);
  if (window < 0) return er::fail("%s: window = %d, must be at least 2 (or 0 for the default)", who, window);
  return odom_align(h, who, n_frames, depth, depth_on_device, n_pairs, model_idx, frame_idx, guess, T_out, status, trace, sums, window);
}

int er_odom_track(er_odom_t h, int n_frames, const uint16_t* depth, int depth_on_device, double* T_rel, int* status, int window) {
  const char* who = "er_odom_track";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  if (n_frames < 2) return er::fail("%s: n_frames = %d, a track needs at least 2", who, n_frames);
  if (!depth) return er::fail("%s: depth is NULL", who);
  if (!T_rel) return er::fail("%s: T_rel is NULL", who);
  if (!status) return er::fail("%s: status is NULL", who);
  if (window < 0) return er::fail("%s: window = %d, must be at least 2 (or 0 for the default)", who, window);
  std::vector<int> a(n_frames - 1), b(n_frames - 1);
  for (int i = 0; i + 1 < n_frames; i++) a[i] = i, b[i] = i + 1;
  return odom_align(h, who, n_frames, depth, depth_on_device, n_frames - 1, a.data(), b.data(), nullptr, T_rel, status, nullptr, nullptr, window);
}

int er_frame_to_model_align(er_odom_t h, const void* const* model_rec_dev, int n_frames, const uint16_t* depth, int depth_on_device, const double* guess,
                            double* T_out, int* status, double* trace, double* sums, int window) {
  const char* who = "er_frame_to_model_align";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  if (n_frames < 1 || !depth) return er::fail("%s: depth is NULL or n_frames = %d is not positive", who, n_frames);
  if (!model_rec_dev) return er::fail("%s: model_rec_dev is NULL", who);
  for (int l = 0; l < h->P.levels; l++)
    if (!model_rec_dev[l]) return er::fail("%s: the model has no record map for level %d of %d", who, l, h->P.levels);
  if (!T_out) return er::fail("%s: T_out is NULL", who);
  if (!status) return er::fail("%s: status is NULL", who);
  if (window < 0) return er::fail("%s: window = %d, must be at least 2 (or 0 for the default)", who, window);
  std::vector<int> a(n_frames, n_frames), b(n_frames);                  // every frame against the model, which the list names as frame n_frames
  for (int i = 0; i < n_frames; i++) b[i] = i;
  return odom_align(h, who, n_frames, depth, depth_on_device, n_frames, a.data(), b.data(), guess, T_out, status, trace, sums, window, model_rec_dev, 1);
}

int er_frames_to_models_align(er_odom_t h, int n_models, const void* const* model_rec_dev, int n_frames, const uint16_t* depth, int depth_on_device,
                              const int* model_of_frame, const double* guess, double* T_out, int* status, double* trace, double* sums, int window) {
  const char* who = "er_frames_to_models_align";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  if (n_frames < 1 || !depth) return er::fail("%s: depth is NULL or n_frames = %d is not positive", who, n_frames);
  if (n_models < 1 || !model_rec_dev) return er::fail("%s: model_rec_dev is NULL or n_models = %d is not positive", who, n_models);
  if (!model_of_frame) return er::fail("%s: model_of_frame is NULL", who);
  std::vector<int> a(n_frames), b(n_frames);                            // frame i against its model, which the list names as frame n_frames + k
  for (int i = 0; i < n_frames; i++) {
    if (model_of_frame[i] < 0 || model_of_frame[i] >= n_models) return er::fail("%s: frame %d names model %d of %d", who, i, model_of_frame[i], n_models);
    a[i] = n_frames + model_of_frame[i];
    b[i] = i;
  }
  return er::odom_align_models(h, who, n_models, model_rec_dev, n_frames, depth, depth_on_device, n_frames, a.data(), b.data(), guess, T_out, status, trace,
                               sums, window);
}

int er_odom_linearize(er_odom_t h, const uint16_t* depth2, int on_device, int level, const double* T, double* sums, int* count) {
  const char* who = "er_odom_linearize";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  if (!depth2 || !T) return er::fail("%s: depth2 or T is NULL", who);
  if (!sums) return er::fail("%s: sums is NULL", who);
  if (!count) return er::fail("%s: count is NULL", who);
  if (level < 0 || level >= h->P.levels) return er::fail("%s: level = %d of %d", who, level, h->P.levels);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (odom_ensure_window(h, 2)) return 1;
  const std::vector<Todo> todo = {{0, 0}, {1, 1}};           // (host buffers of asynchronous copies: declared before the lease)
  const PairDesc pd = {0, 1};
  OdomState s;
  state_from(T, s);
  StreamLease lease;
  if (lease.acquire(h->device)) return 1;
  hipStream_t st = lease.stream;
  if (odom_preprocess(h, st, todo, depth2, on_device)) return 1;
  ER_HIP_TRY(hipMemcpyAsync(h->d_pairs, &pd, sizeof pd, hipMemcpyHostToDevice, st));
  ER_HIP_TRY(hipMemcpyAsync(h->d_state, &s, sizeof s, hipMemcpyHostToDevice, st));
  const int nblk = nblk_of(h, level);
  hipLaunchKernelGGL(k_odom_iter, dim3(nblk, 1), dim3(kBlock), 0, st, h->lo, level, h->d_pairs, h->d_state, h->d_partial, h->d_pcount, nblk, h->P.dist_thresh,
                     h->P.angle_thresh);
  hipLaunchKernelGGL(k_odom_final, dim3(1), dim3(kBlock), 0, st, h->d_state, h->d_partial, h->d_pcount, nblk, h->P.min_valid, 0, (double*)nullptr, 0, 0,
                     h->d_sums);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipMemcpyAsync(sums, h->d_sums, sizeof(double) * er_od::kSums, hipMemcpyDeviceToHost, st));
  ER_HIP_TRY(hipMemcpyAsync(&s, h->d_state, sizeof s, hipMemcpyDeviceToHost, st));
  ER_HIP_TRY(hipStreamSynchronize(st));
  *count = s.count;
  return 0;
}

int er_odom_read_maps(er_odom_t h, const uint16_t* depth1, int on_device, int level, uint16_t* depth_out, float* vmap_out, float* nmap_out) {
  const char* who = "er_odom_read_maps";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  if (!depth1) return er::fail("%s: depth1 is NULL", who);
  if (level < 0 || level >= h->P.levels) return er::fail("%s: level = %d of %d", who, level, h->P.levels);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (odom_ensure_window(h, 2)) return 1;
  const std::vector<Todo> todo = {{0, 0}};
  const size_t npix = (size_t)h->lo.cols[level] * h->lo.rows[level];
  std::vector<float> rec(npix * 8);
  StreamLease lease;
  if (lease.acquire(h->device)) return 1;
  hipStream_t st = lease.stream;
  if (odom_preprocess(h, st, todo, depth1, on_device)) return 1;
  if (depth_out) ER_HIP_TRY(hipMemcpyAsync(depth_out, h->lo.base + h->lo.off_depth[level], npix * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  ER_HIP_TRY(hipMemcpyAsync(rec.data(), h->lo.base + h->lo.off_rec[level], npix * 8 * sizeof(float), hipMemcpyDeviceToHost, st));
  ER_HIP_TRY(hipStreamSynchronize(st));
  for (size_t i = 0; i < npix; i++)
    for (int k = 0; k < 3; k++) {
      if (vmap_out) vmap_out[3 * i + k] = rec[8 * i + k];
      if (nmap_out) nmap_out[3 * i + k] = rec[8 * i + 4 + k];
    }
  return 0;
}

}  // extern "C"
