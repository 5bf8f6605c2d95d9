// er_ransac.hip -- GlobalRegistration's RANSAC pose search on the device (it shares the cloud types of er_cloud.h, the exact
// nearest-neighbour search nn_block of er_nn.h and, through er::StreamLease, the workspace pool of er_icp.hip).  RansacCurvature::computeTransformation
// (GlobalRegistration/RansacCurvature.h:411-657) with PolyRejector.h, the per-point features as an input.
//   k_feature_knn / k_feature_knn_merge   findSimilarFeatures' nearestKSearch for every source descriptor: brute force, the source
//                        descriptor of a lane in registers, target descriptors through LDS tiles read as broadcasts, top-k in registers
//   k_ransac_propose     one lane per iteration: counter-based draws, selectSamples, the pick among the k matches, the polygon test with
//                        an early exit per edge -> one ballot bit per iteration
//   k_ransac_list        the bits of a chunk -> the surviving iteration numbers in ascending order (one workgroup: count, scan, write)
//   k_ransac_estimate    the survivors: samples re-drawn from the iteration number, float64 rigid estimate, NaN / normal test
//   k_ransac_accept      stable compaction of the accepted ones
//   k_ransac_score       k_ransac_fitness's search over them, hypotheses read from device memory, 64-bit fixed-point distance sums
//   k_ransac_select      the reference's acceptance rule and the (error, iteration) minimum, carried across chunks; the aux rows
// Nothing comes back to the host between the chunks: every kernel reads the counts of its predecessor from device memory.
// Every kernel of the search takes its pair from a grid axis and a descriptor (RsPair) in device memory: er_ransac_align_batch runs a whole wave of
// pairs through each launch, er_ransac_align is the list of one.
#include "er_cloud.h"
#include "er_nn.h"
#include "er_ransac_math.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

using namespace er;

namespace {

constexpr int kKnnTile = 64;                   // target descriptors per LDS tile (64 x 64 floats = 16 KiB at most)

template <int K>
__device__ __forceinline__ void knn_insert(float (&kd)[K], int (&ki)[K], float d, int i) {
  if (d < kd[K - 1]) {                         // strict: an equal distance with a higher index never displaces an earlier one
    kd[K - 1] = d;
    ki[K - 1] = i;
#pragma unroll
    for (int m = K - 1; m > 0; m--)
      if (kd[m] < kd[m - 1]) {
        const float td = kd[m]; kd[m] = kd[m - 1]; kd[m - 1] = td;
        const int ti = ki[m]; ki[m] = ki[m - 1]; ki[m - 1] = ti;
      }
  }
}

// blockIdx.x = 256 source descriptors, blockIdx.y = a segment of seg_len target descriptors; partial top-K lists per segment.
template <int DP, int K>
__global__ __launch_bounds__(kBlock) void k_feature_knn(const float* __restrict__ src, int ns, const float* __restrict__ tgt, int nt, int seg_len,
                                                        float* __restrict__ pd, int* __restrict__ pi) {
  __shared__ float4 tile[kKnnTile * DP / 4];
  const int q = blockIdx.x * kBlock + (int)threadIdx.x;
  float a[DP];
#pragma unroll
  for (int j = 0; j < DP; j += 4) {
    const float4 v = q < ns ? *(const float4*)(src + (size_t)q * DP + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    a[j] = v.x; a[j + 1] = v.y; a[j + 2] = v.z; a[j + 3] = v.w;
  }
  float kd[K];
  int ki[K];
#pragma unroll
  for (int m = 0; m < K; m++) {
    kd[m] = INFINITY;
    ki[m] = -1;
  }
  const int t0 = blockIdx.y * seg_len, t1 = min(nt, t0 + seg_len);
  for (int tb = t0; tb < t1; tb += kKnnTile) {
    const int rows = min(kKnnTile, t1 - tb);
    __syncthreads();
    const float4* g4 = (const float4*)(tgt + (size_t)tb * DP);
    for (int e = threadIdx.x; e < rows * (DP / 4); e += kBlock) tile[e] = g4[e];
    __syncthreads();
    for (int r = 0; r < rows; r++) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < DP; j += 4) {
        const float4 b = tile[r * (DP / 4) + j / 4];
        const float e0 = a[j] - b.x, e1 = a[j + 1] - b.y, e2 = a[j + 2] - b.z, e3 = a[j + 3] - b.w;
        d = d + e0 * e0;
        d = d + e1 * e1;
        d = d + e2 * e2;
        d = d + e3 * e3;
      }
      knn_insert<K>(kd, ki, d, tb + r);
    }
  }
  if (q < ns) {
    const size_t o = ((size_t)blockIdx.y * (size_t)ns + (size_t)q) * K;
#pragma unroll
    for (int m = 0; m < K; m++) {
      pd[o + m] = kd[m];
      pi[o + m] = ki[m];
    }
  }
}

// The segments' lists in ascending segment order through the same insertion: ties still go to the lower index.
template <int K>
__global__ __launch_bounds__(kBlock) void k_feature_knn_merge(const float* __restrict__ pd, const int* __restrict__ pi, int ns, int segs, int k,
                                                              int* __restrict__ idx, float* __restrict__ dist) {
  const int q = blockIdx.x * kBlock + (int)threadIdx.x;
  if (q >= ns) return;
  float kd[K];
  int ki[K];
#pragma unroll
  for (int m = 0; m < K; m++) {
    kd[m] = INFINITY;
    ki[m] = -1;
  }
  for (int s = 0; s < segs; s++) {
    const size_t o = ((size_t)s * (size_t)ns + (size_t)q) * K;
#pragma unroll
    for (int m = 0; m < K; m++) {
      const int i = pi[o + m];
      if (i >= 0) knn_insert<K>(kd, ki, pd[o + m], i);
    }
  }
#pragma unroll
  for (int m = 0; m < K; m++)
    if (m < k) {
      idx[(size_t)q * k + m] = ki[m];
      dist[(size_t)q * k + m] = kd[m];
    }
}

template <int DP>
int knn_launch(int K, dim3 grid, hipStream_t st, const float* src, int ns, const float* tgt, int nt, int seg_len, float* pd, int* pi) {
  if (K == 2)
    hipLaunchKernelGGL((k_feature_knn<DP, 2>), grid, dim3(kBlock), 0, st, src, ns, tgt, nt, seg_len, pd, pi);
  else
    hipLaunchKernelGGL((k_feature_knn<DP, 8>), grid, dim3(kBlock), 0, st, src, ns, tgt, nt, seg_len, pd, pi);
  return 0;
}

// The segments of the target a source block's partial lists come from, and the floats / ints of scratch they need.
size_t knn_plan(int ns, int nt, int k, int* segs_out, int* seg_len_out) {
  const int K = k <= 2 ? 2 : 8;
  const int nbx = nblocks_of(ns);
  int segs = std::max(1, std::min(64, 1024 / nbx));
  const int seg_len = ((nt + segs - 1) / segs + kKnnTile - 1) / kKnnTile * kKnnTile;
  segs = (nt + seg_len - 1) / seg_len;
  if (segs_out) *segs_out = segs;
  if (seg_len_out) *seg_len_out = seg_len;
  return (size_t)segs * ns * K;
}

// idx / dist: device arrays [ns][k].  Enqueued on `st`; pd / pi: knn_plan() elements of scratch each, free again when the stream has passed this point.
int feature_knn_device(const er_features_s* s, const er_features_s* t, int k, hipStream_t st, int* d_idx, float* d_dist, float* pd, int* pi) {
  const int K = k <= 2 ? 2 : 8;
  const int nbx = nblocks_of(s->n);
  int segs, seg_len;
  knn_plan(s->n, t->n, k, &segs, &seg_len);
  const dim3 grid(nbx, segs);
  switch (s->dp) {
    case 8: knn_launch<8>(K, grid, st, s->d, s->n, t->d, t->n, seg_len, pd, pi); break;
    case 16: knn_launch<16>(K, grid, st, s->d, s->n, t->d, t->n, seg_len, pd, pi); break;
    case 24: knn_launch<24>(K, grid, st, s->d, s->n, t->d, t->n, seg_len, pd, pi); break;
    case 32: knn_launch<32>(K, grid, st, s->d, s->n, t->d, t->n, seg_len, pd, pi); break;
    case 40: knn_launch<40>(K, grid, st, s->d, s->n, t->d, t->n, seg_len, pd, pi); break;
    case 48: knn_launch<48>(K, grid, st, s->d, s->n, t->d, t->n, seg_len, pd, pi); break;
    case 56: knn_launch<56>(K, grid, st, s->d, s->n, t->d, t->n, seg_len, pd, pi); break;
    default: knn_launch<64>(K, grid, st, s->d, s->n, t->d, t->n, seg_len, pd, pi); break;
  }
  if (K == 2)
    hipLaunchKernelGGL((k_feature_knn_merge<2>), dim3(nbx), dim3(kBlock), 0, st, pd, pi, s->n, segs, k, d_idx, d_dist);
  else
    hipLaunchKernelGGL((k_feature_knn_merge<8>), dim3(nbx), dim3(kBlock), 0, st, pd, pi, s->n, segs, k, d_idx, d_dist);
  ER_HIP_TRY(hipGetLastError());
  return 0;
}

int check_features(er_features_t sf, er_features_t tf, int k, const char* who) {
  if (!sf || !tf) return er::fail("%s: NULL feature set", who);
  if (sf->device != tf->device) return er::fail("%s: the feature sets live on different devices", who);
  if (sf->dim != tf->dim) return er::fail("%s: source descriptors have %d dimensions, target descriptors %d", who, sf->dim, tf->dim);
  if (k < 1 || k > 8) return er::fail("%s: k = %d, must be 1 .. 8 (correspondence randomness must be > 0)", who, k);
  if (sf->n < 1 || tf->n < k) return er::fail("%s: %d source and %d target descriptors are too few for k = %d", who, sf->n, tf->n, k);
  return 0;
}

// ---- hypotheses -----------------------------------------------------------------------------------------------------------
// What the chunk's kernels hand to each other and carry across chunks.
struct RsState {
  int n_surv, n_acc;                     // of the current chunk
  long long tot_surv, tot_acc;
  int converged, best_it, best_count;
  double best_err;
  float best_M[16];
};

// What one pair of a list brings to the kernels of a chunk: its clouds, its k-NN table, its seed, its fixed-point scale and its slices of the call's
// workspace.  One descriptor per pair in flight, in device memory; state i belongs to descriptor i.  Everything else -- the iteration range, k, the
// thresholds -- is the same for every pair of a call and arrives as kernel arguments.
struct RsPair {
  const float4 *sxn, *txn, *src_sorted;  // source and target rows in file order, the cell-sorted source
  Grid g;                                // the target's grid
  const int* knn;                        // [n][k]
  int n;                                 // source points
  unsigned seed;
  double scale, inv_scale;               // of the 64-bit distance sums (k_ransac_score)
  unsigned long long* mask;
  int *list, *status, *acc, *count;
  long long* sum;
  float* M;
  er_ransac_aux* aux;
  long long aux_cap;
};

struct RsPoints {
  float x[er_rs::kMaxSamples][3], n[er_rs::kMaxSamples][3];
};

// Estimate + NaN check + thresholdNormal of one sample set whose points and normals are loaded: 0 accepted, 2 rejected.
template <int NS>
__device__ __forceinline__ int rs_estimate(const RsPoints& S, const RsPoints& T, double cos_angle, float* M) {
  double P[er_rs::kMaxSamples][3], Q[er_rs::kMaxSamples][3];
#pragma unroll
  for (int i = 0; i < er_rs::kMaxSamples; i++)
#pragma unroll
    for (int a = 0; a < 3; a++) {
      P[i][a] = i < NS ? (double)S.x[i][a] : 0.0;
      Q[i][a] = i < NS ? (double)T.x[i][a] : 0.0;
    }
  er_rs::rigid_estimate(P, Q, NS, M);
  bool ok = true;
#pragma unroll
  for (int e = 0; e < 12; e++) ok = ok && M[e] == M[e];
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const float d = er_rs::normal_dot(M, S.n[i][0], S.n[i][1], S.n[i][2], T.n[i][0], T.n[i][1], T.n[i][2]);
    if ((double)d < cos_angle) ok = false;          // (the reference's `nt.dot( nn ) < cos( angle_diff_ )`: a NaN dot product passes there too)
  }
  return ok ? 0 : 2;
}

template <int NS>
__device__ __forceinline__ void rs_load(const float4* __restrict__ xn, const int (&idx)[NS], RsPoints& out) {
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const float4 p = xn[2 * (size_t)idx[i]], n = xn[2 * (size_t)idx[i] + 1];
    out.x[i][0] = p.x; out.x[i][1] = p.y; out.x[i][2] = p.z;
    out.n[i][0] = n.x; out.n[i][1] = n.y; out.n[i][2] = n.z;
  }
}

// The matched target index of the i-th sample of an iteration.
__device__ __forceinline__ int rs_pick(const int* __restrict__ knn, int k, unsigned seed, unsigned it, int i, int s) {
  return k > 1 ? knn[(size_t)s * k + er_rs::index_of(er_rs::draw(seed, it, er_rs::kPickDraw + (unsigned)i), k)] : knn[s];
}

template <int NS>
__global__ __launch_bounds__(kBlock) void k_ransac_hypotheses(const float4* __restrict__ sxn, const float4* __restrict__ txn, int n_hyp,
                                                              const int* __restrict__ s_idx, const int* __restrict__ c_idx, float simsq,
                                                              double cos_angle, int* __restrict__ status, float* __restrict__ Mout) {
  const int h = blockIdx.x * kBlock + (int)threadIdx.x;
  if (h >= n_hyp) return;
  int s[NS], c[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) {
    s[i] = s_idx[(size_t)h * NS + i];
    c[i] = c_idx[(size_t)h * NS + i];
  }
  RsPoints S, T;
  rs_load<NS>(sxn, s, S);
  rs_load<NS>(txn, c, T);
  bool poly = true;
#pragma unroll
  for (int i = 0; i < NS; i++)
#pragma unroll
    for (int j = i + 1; j < NS; j++)
      poly = poly && er_rs::edge_ok(er_rs::sqdist(S.x[i][0], S.x[i][1], S.x[i][2], S.x[j][0], S.x[j][1], S.x[j][2]),
                                    er_rs::sqdist(T.x[i][0], T.x[i][1], T.x[i][2], T.x[j][0], T.x[j][1], T.x[j][2]), simsq);
  float M[16];
  int st = 1;
  if (poly) {
    st = rs_estimate<NS>(S, T, cos_angle, M);
  } else {
#pragma unroll
    for (int e = 0; e < 16; e++) M[e] = 0.f;
  }
  status[h] = st;
#pragma unroll
  for (int e = 0; e < 16; e++) Mout[(size_t)h * 16 + e] = M[e];
}

// One lane per iteration it0 + gid of pair blockIdx.y; bit gid of the pair's `mask` = the iteration passed the polygon test.  Every wave of the
// grid writes its word.
template <int NS>
__global__ __launch_bounds__(kBlock) void k_ransac_propose(const RsPair* __restrict__ P, int k, unsigned it0, int count, float simsq) {
  const RsPair& p = P[blockIdx.y];
  const float4* __restrict__ sxn = p.sxn;
  const float4* __restrict__ txn = p.txn;
  const int* __restrict__ knn = p.knn;
  const int n_src = p.n;
  const unsigned seed = p.seed;
  const int gid = blockIdx.x * kBlock + (int)threadIdx.x;
  bool ok = gid < count;
  if (ok) {
    const unsigned it = it0 + (unsigned)gid;
    int s[NS];
    er_rs::select_samples<NS>(seed, it, n_src, s);
    float4 ps[NS], pt[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) {
      if (ok) {                                     // a failed edge ends the iteration: the later points are never fetched
        const int c = rs_pick(knn, k, seed, it, i, s[i]);
        ps[i] = sxn[2 * (size_t)s[i]];
        pt[i] = txn[2 * (size_t)c];
#pragma unroll
        for (int j = 0; j < i; j++)
          ok = ok && er_rs::edge_ok(er_rs::sqdist(ps[j].x, ps[j].y, ps[j].z, ps[i].x, ps[i].y, ps[i].z),
                                    er_rs::sqdist(pt[j].x, pt[j].y, pt[j].z, pt[i].x, pt[i].y, pt[i].z), simsq);
      }
    }
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) p.mask[gid >> 6] = m;
}

// A value every lane of the wave holds alike (it was loaded through the pair's descriptor, whose address the compiler does not see to be uniform), moved
// to scalar registers: k_ransac_score then keeps the grid and its pointers where the by-value arguments of a single pair's launch used to be.
template <typename T>
__device__ __forceinline__ T wave_uniform(T v) {
  static_assert(sizeof(T) % 4 == 0, "whole dwords");
  union { T t; int w[sizeof(T) / 4]; } u;
  u.t = v;
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; i++) u.w[i] = __builtin_amdgcn_readfirstlane(u.w[i]);
  return u.t;
}

// Exclusive scan of one int per thread over a workgroup of 1024; returns the thread's offset, *total = the sum.
__device__ __forceinline__ int block_scan_1024(int v, int* sh /* [1024] */, int* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int add = t >= off ? sh[t - off] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  *total = sh[1023];
  const int incl = sh[t];
  __syncthreads();
  return incl - v;
}

// One workgroup per pair: the set bits of `words` mask words -> list[] = iteration numbers, ascending.  (The barriers are those of the scan: every
// thread of every workgroup reaches them, whatever its pair's counts are.)
__global__ __launch_bounds__(1024) void k_ransac_list(const RsPair* __restrict__ P, RsState* __restrict__ S, int words, unsigned it0) {
  __shared__ int sh[1024];
  const RsPair& p = P[blockIdx.x];
  const unsigned long long* __restrict__ mask = p.mask;
  int* __restrict__ list = p.list;
  RsState* st = S + blockIdx.x;
  const int per = (words + 1023) / 1024, w0 = min(words, (int)threadIdx.x * per), w1 = min(words, w0 + per);
  int c = 0;
  for (int w = w0; w < w1; w++) c += __popcll(mask[w]);
  int total;
  int pos = block_scan_1024(c, sh, &total);
  for (int w = w0; w < w1; w++) {
    unsigned long long m = mask[w];
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      list[pos++] = (int)(it0 + (unsigned)w * 64u + (unsigned)b);
      m &= m - 1;
    }
  }
  if (threadIdx.x == 0) {
    st->n_surv = total;
    st->tot_surv += total;
  }
}

// blockIdx.y = pair, blockIdx.x strides over the pair's survivors.
template <int NS>
__global__ __launch_bounds__(kBlock) void k_ransac_estimate(const RsPair* __restrict__ P, const RsState* __restrict__ S, int k, double cos_angle) {
  const RsPair& p = P[blockIdx.y];
  const float4* __restrict__ sxn = p.sxn;
  const float4* __restrict__ txn = p.txn;
  const int* __restrict__ knn = p.knn;
  const int* __restrict__ list = p.list;
  int* __restrict__ status = p.status;
  float* __restrict__ Mout = p.M;
  const int n_src = p.n;
  const unsigned seed = p.seed;
  const int n = S[blockIdx.y].n_surv;
  for (int j = blockIdx.x * kBlock + (int)threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const unsigned it = (unsigned)list[j];
    int s[NS], c[NS];
    er_rs::select_samples<NS>(seed, it, n_src, s);
#pragma unroll
    for (int i = 0; i < NS; i++) c[i] = rs_pick(knn, k, seed, it, i, s[i]);
    RsPoints Sp, Tp;
    rs_load<NS>(sxn, s, Sp);
    rs_load<NS>(txn, c, Tp);
    float M[16];
    status[j] = rs_estimate<NS>(Sp, Tp, cos_angle, M);
#pragma unroll
    for (int e = 0; e < 16; e++) Mout[(size_t)j * 16 + e] = M[e];
  }
}

// One workgroup per pair: acc[] = the positions j of the survivors with status 0, ascending; zeroes their score slots.  (A pair without a survivor
// still takes every barrier of the scan: its loops are empty, not skipped.)
__global__ __launch_bounds__(1024) void k_ransac_accept(const RsPair* __restrict__ P, RsState* __restrict__ S) {
  __shared__ int sh[1024];
  const RsPair& p = P[blockIdx.x];
  const int* __restrict__ status = p.status;
  int* __restrict__ acc = p.acc;
  int* __restrict__ count = p.count;
  long long* __restrict__ sum = p.sum;
  RsState* st = S + blockIdx.x;
  const int n = st->n_surv;
  const int per = (n + 1023) / 1024, j0 = min(n, (int)threadIdx.x * per), j1 = min(n, j0 + per);
  int c = 0;
  for (int j = j0; j < j1; j++) c += status[j] == 0;
  int total;
  int pos = block_scan_1024(c, sh, &total);
  for (int j = j0; j < j1; j++)
    if (status[j] == 0) {
      count[pos] = 0;
      sum[pos] = 0;
      acc[pos++] = j;
    }
  if (threadIdx.x == 0) {
    st->n_acc = total;
    st->tot_acc += total;
  }
}

// k_ransac_fitness for the accepted hypotheses of a chunk: blockIdx.z = pair, blockIdx.y strides over its hypotheses, blockIdx.x over its source
// points.  The inlier distances are added as 64-bit integers (d * scale truncated, scale a power of two with n * max_range * scale < 2^61): the sum
// does not depend on the order of the workgroups, nor on the grid, which is sized for the largest pair of the wave.
// nn_block synchronises, so whoever calls it must do so with the whole workgroup: a workgroup that has no source points of its pair (the pair is
// smaller than the one the grid was sized for) or whose pair has nothing to score leaves HERE, as a whole, before the first barrier; inside the
// loops every bound (nh, n, base) is the same for all threads of a workgroup.
__global__ __launch_bounds__(kBlock) void k_ransac_score(const RsPair* __restrict__ P, const RsState* __restrict__ S, float radius, float max_range) {
  __shared__ NnSh sh;
  __shared__ int pc[kBlock / 64];
  __shared__ long long ps[kBlock / 64];
  const RsPair& p = P[blockIdx.z];
  const int nh = wave_uniform(S[blockIdx.z].n_acc), n = wave_uniform(p.n);
  if (nh == 0 || (int)blockIdx.x * kBlock >= n) return;
  const Grid g = wave_uniform(p.g);
  const gp_f4 src_sorted = ER_GP(gp_f4, wave_uniform(p.src_sorted));
  const gp_f Mbuf = ER_GP(gp_f, wave_uniform(p.M));
  const gp_i acc = ER_GP(gp_i, wave_uniform(p.acc));
  int* __restrict__ count = wave_uniform(p.count);
  long long* __restrict__ sum = wave_uniform(p.sum);
  const double scale = wave_uniform(p.scale);
  for (int h = blockIdx.y; h < nh; h += gridDim.y) {
    const gp_f hyp = Mbuf + (size_t)wave_uniform<int>(acc[h]) * 16;
    float M[12];
#pragma unroll
    for (int q = 0; q < 12; q++) M[q] = wave_uniform<float>(hyp[q]);
    int local = 0;
    long long dsum = 0;
    for (int base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
      const int k = base + (int)threadIdx.x;
      float qx = 0.f, qy = 0.f, qz = 0.f, d;
      if (k < n) {
        const f4v s = src_sorted[k];
        qx = ((M[0] * s.x + M[1] * s.y) + M[2] * s.z) + M[3];
        qy = ((M[4] * s.x + M[5] * s.y) + M[6] * s.z) + M[7];
        qz = ((M[8] * s.x + M[9] * s.y) + M[10] * s.z) + M[11];
      }
      const int i = nn_block(sh, g, k < n, qx, qy, qz, radius * radius, d);
      if (k < n && i >= 0 && d < max_range) {
        local++;
        dsum += (long long)((double)d * scale);
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      local += __shfl_down(local, off);
      dsum += __shfl_down(dsum, off);
    }
    if ((threadIdx.x & 63) == 0) {
      pc[threadIdx.x >> 6] = local;
      ps[threadIdx.x >> 6] = dsum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int c = 0;
      long long s = 0;
      for (int w = 0; w < kBlock / 64; w++) {
        c += pc[w];
        s += ps[w];
      }
      if (c) {
        atomicAdd(&count[h], c);
        atomicAdd((unsigned long long*)&sum[h], (unsigned long long)s);
      }
    }
    __syncthreads();
  }
}

// One workgroup per pair: the aux rows of the chunk's scored hypotheses and the running (error, iteration) minimum over the acceptable ones.
// (One barrier, outside every loop: a pair with nothing scored takes it too.)
__global__ __launch_bounds__(kBlock) void k_ransac_select(const RsPair* __restrict__ P, RsState* __restrict__ S, float inlier_fraction, int inlier_number) {
  __shared__ double s_err[kBlock];
  __shared__ int s_it[kBlock], s_h[kBlock];
  const RsPair& p = P[blockIdx.x];
  const int* __restrict__ list = p.list;
  const int* __restrict__ acc = p.acc;
  const float* __restrict__ Mbuf = p.M;
  const int* __restrict__ count = p.count;
  const long long* __restrict__ sum = p.sum;
  er_ransac_aux* __restrict__ aux = p.aux;
  const long long aux_cap = p.aux_cap;
  const int n_src = p.n;
  const double inv_scale = p.inv_scale;
  RsState* st = S + blockIdx.x;
  const int nh = st->n_acc;
  const long long base = st->tot_acc - nh;                       // (k_ransac_accept has added this chunk already)
  double b_err = DBL_MAX;
  int b_it = 0x7fffffff, b_h = -1;
  for (int h = threadIdx.x; h < nh; h += kBlock) {
    const int j = acc[h], it = list[j], c = count[h];
    const double err = c > 0 ? ((double)sum[h] * inv_scale) / (double)c : (double)FLT_MAX;
    if (base + h < aux_cap) {
      er_ransac_aux& a = aux[base + h];
      a.iteration = it;
      a.count = c;
      a.error = err;
      for (int e = 0; e < 16; e++) a.M[e] = Mbuf[(size_t)j * 16 + e];
    }
    const bool acceptable = c > 0 && ((float)c / (float)n_src >= inlier_fraction || c > inlier_number);
    if (acceptable && (err < b_err || (err == b_err && it < b_it))) {
      b_err = err;
      b_it = it;
      b_h = h;
    }
  }
  s_err[threadIdx.x] = b_err;
  s_it[threadIdx.x] = b_it;
  s_h[threadIdx.x] = b_h;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < kBlock; t++)
      if (s_h[t] >= 0 && (b_h < 0 || s_err[t] < b_err || (s_err[t] == b_err && s_it[t] < b_it))) {
        b_err = s_err[t];
        b_it = s_it[t];
        b_h = s_h[t];
      }
    if (b_h >= 0 && (!st->converged || b_err < st->best_err || (b_err == st->best_err && b_it < st->best_it))) {
      st->converged = 1;
      st->best_err = b_err;
      st->best_it = b_it;
      st->best_count = count[b_h];
      for (int e = 0; e < 16; e++) st->best_M[e] = Mbuf[(size_t)acc[b_h] * 16 + e];
    }
  }
}

// ---- the search of a list of pairs ------------------------------------------------------------------------------------------------------------
// Everything er_ransac_align refuses about one pair; `who` names the entry point (and, for a list, the pair).
int ransac_check(er_cloud_t src, er_cloud_t tgt, er_features_t src_feat, er_features_t tgt_feat, const er_ransac_params* p, const char* who) {
  if (check_pair(src, tgt, (double)p->max_corr_dist, who)) return 1;
  if (p->nr_samples == 2)
    return er::fail("%s: nr_samples = 2 is refused: the reference's two-point branch builds the target's virtual points from the source's normal and "
                    "midpoint (RansacCurvature.h:575-580); matching it would mean copying a slip", who);
  if (p->nr_samples < 3 || p->nr_samples > er_rs::kMaxSamples) return er::fail("%s: nr_samples = %d, must be 3 .. 6", who, p->nr_samples);
  if (check_features(src_feat, tgt_feat, p->k_correspondences, who)) return 1;
  if (src_feat->device != src->device) return er::fail("%s: features and clouds live on different devices", who);
  if (src->n != src_feat->n)
    return er::fail("%s: the source points and source feature points need to be in a one-to-one relationship: %d vs %d", who, src->n, src_feat->n);
  if (tgt->n != tgt_feat->n)
    return er::fail("%s: the target points and target feature points need to be in a one-to-one relationship: %d vs %d", who, tgt->n, tgt_feat->n);
  if (!(p->inlier_fraction >= 0.f && p->inlier_fraction <= 1.f)) return er::fail("%s: illegal inlier fraction %g, must be in [0,1]", who, (double)p->inlier_fraction);
  if (!(p->similarity >= 0.f && p->similarity < 1.f))
    return er::fail("%s: illegal prerejection similarity threshold %g, must be in [0,1[", who, (double)p->similarity);
  if (p->max_iterations < 1 || p->max_iterations > (1 << 28)) return er::fail("%s: max_iterations = %d, must be 1 .. 2^28", who, p->max_iterations);
  if (p->chunk_iterations < 0) return er::fail("%s: chunk_iterations = %d is negative", who, p->chunk_iterations);
  if (src->n < p->nr_samples) return er::fail("%s: the number of samples (%d) must not be greater than the number of points (%d)", who, p->nr_samples, src->n);
  return 0;
}

constexpr size_t kWorkspaceDefault = (size_t)2 << 30;   // what the pairs in flight may take when the caller leaves max_concurrent to the library
constexpr int kConcurrentDefaultMax = 64;

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// The checked list in waves of at most max_concurrent pairs.  One allocation holds the descriptors, the states and, per pair in flight, the k-NN table
// and the chunk's arrays (88 bytes and one mask bit per chunk iteration); the feature k-NN of the wave's pairs is enqueued pair after pair through one
// scratch block, then every chunk runs the six kernels once for the whole wave, and the wave's states come back in one copy.  info_source36 /
// info_target36 (nullable): the information matrices of the wave's converged pairs through the lease's compaction chain.  aux: slot 0's rows (the
// single call).
int ransac_run(int n_pairs, const er_cloud_t* src, const er_cloud_t* tgt, const er_features_t* sf, const er_features_t* tf, const er_ransac_params* p,
               const unsigned* seeds, int max_concurrent, float* T_out, int* converged, int* n_inliers, double* error, er_ransac_stats* stats,
               double* info_s, double* info_t, er_ransac_aux* aux, int aux_capacity, int* aux_count) {
  const int chunk = std::min(p->max_iterations, p->chunk_iterations > 0 ? p->chunk_iterations : (1 << 20));
  const int k = p->k_correspondences, ns = p->nr_samples;
  const size_t words = ((size_t)chunk + kBlock - 1) / kBlock * (kBlock / 64);
  size_t max_nk = 0, max_part = 0;
  for (int i = 0; i < n_pairs; i++) {
    max_nk = std::max(max_nk, (size_t)src[i]->n * k);
    max_part = std::max(max_part, knn_plan(src[i]->n, tgt[i]->n, k, nullptr, nullptr));
  }
  // a slot = what one pair in flight owns
  const size_t o_knn = 0, o_mask = o_knn + up256(max_nk * sizeof(int)), o_list = o_mask + up256(words * sizeof(unsigned long long)),
               o_status = o_list + up256((size_t)chunk * sizeof(int)), o_acc = o_status + up256((size_t)chunk * sizeof(int)),
               o_count = o_acc + up256((size_t)chunk * sizeof(int)), o_sum = o_count + up256((size_t)chunk * sizeof(int)),
               o_M = o_sum + up256((size_t)chunk * sizeof(long long)), slot = o_M + up256((size_t)chunk * 16 * sizeof(float));
  int mc = max_concurrent > 0 ? max_concurrent : (int)std::min<size_t>(kConcurrentDefaultMax, std::max<size_t>(1, kWorkspaceDefault / slot));
  mc = std::min(mc, n_pairs);
  // shared by the slots
  const size_t o_desc = 0, o_state = o_desc + up256((size_t)mc * sizeof(RsPair)), o_kd = o_state + up256((size_t)mc * sizeof(RsState)),
               o_pd = o_kd + up256(max_nk * sizeof(float)), o_pi = o_pd + up256(max_part * sizeof(float)), o_aux = o_pi + up256(max_part * sizeof(int)),
               o_slots = o_aux + up256((size_t)aux_capacity * sizeof(er_ransac_aux)), total = o_slots + (size_t)mc * slot;
  StreamLease L;
  if (L.acquire(src[0]->device)) return 1;
  hipStream_t S = L.stream;
  DevScope B;
  char* ws;
  if (B.alloc(&ws, total, "the RANSAC search")) {
    (void)hipGetLastError();
    return er::fail("the RANSAC search: %zu MB of workspace for %d pairs in flight could not be allocated", total >> 20, mc);
  }
  RsPair* d_desc = (RsPair*)(ws + o_desc);
  RsState* d_st = (RsState*)(ws + o_state);
  er_ransac_aux* d_aux = (er_ransac_aux*)(ws + o_aux);
  std::vector<RsPair> hd((size_t)mc);
  std::vector<RsState> hs((size_t)mc);
  std::vector<er_cloud_t> c_src, c_tgt;
  std::vector<float> c_M;
  std::vector<double> c_is, c_it;
  const float simsq = p->similarity * p->similarity, radius = p->max_corr_dist, max_range = radius * radius;
  const double ca = std::cos((double)p->angle_diff);
  const int est_blocks = 256, score_by = 512;
  for (int w0 = 0; w0 < n_pairs; w0 += mc) {
    const int m = std::min(mc, n_pairs - w0);
    int n_max = 0;
    for (int q = 0; q < m; q++) {
      const er_cloud_s *s = src[w0 + q], *t = tgt[w0 + q];
      char* base = ws + o_slots + (size_t)q * slot;
      RsPair& d = hd[(size_t)q];
      d.sxn = s->xn; d.txn = t->xn; d.src_sorted = s->sorted;
      d.g = t->grid;
      d.knn = (int*)(base + o_knn);
      d.n = s->n;
      d.seed = seeds ? seeds[w0 + q] : p->seed;
      const double bound = (double)s->n * (double)max_range;
      const int sexp = 60 - (bound > 0.0 ? std::ilogb(bound) : 0);
      d.scale = std::ldexp(1.0, sexp); d.inv_scale = std::ldexp(1.0, -sexp);
      d.mask = (unsigned long long*)(base + o_mask);
      d.list = (int*)(base + o_list); d.status = (int*)(base + o_status); d.acc = (int*)(base + o_acc); d.count = (int*)(base + o_count);
      d.sum = (long long*)(base + o_sum);
      d.M = (float*)(base + o_M);
      d.aux = d_aux; d.aux_cap = (long long)aux_capacity;
      n_max = std::max(n_max, s->n);
      // (the k-NN kernels of consecutive pairs share pd / pi / kd: the stream orders them)
      if (feature_knn_device(sf[w0 + q], tf[w0 + q], k, S, (int*)(base + o_knn), (float*)(ws + o_kd), (float*)(ws + o_pd), (int*)(ws + o_pi))) return 1;
    }
    ER_HIP_TRY(hipMemcpyAsync(d_desc, hd.data(), (size_t)m * sizeof(RsPair), hipMemcpyHostToDevice, S));
    ER_HIP_TRY(hipMemsetAsync(d_st, 0, (size_t)m * sizeof(RsState), S));
    const int score_bx = std::max(1, std::min(nblocks_of(n_max), 8));
    for (int it0 = 0; it0 < p->max_iterations; it0 += chunk) {
      const int cnt = std::min(chunk, p->max_iterations - it0);
      const dim3 pg(nblocks_of(cnt), m), eg(est_blocks, m);
      const int w = (cnt + 63) / 64;
#define ER_RS_NS(NSV)                                                                                                          \
  hipLaunchKernelGGL((k_ransac_propose<NSV>), pg, dim3(kBlock), 0, S, d_desc, k, (unsigned)it0, cnt, simsq);                   \
  hipLaunchKernelGGL(k_ransac_list, dim3(m), dim3(1024), 0, S, d_desc, d_st, w, (unsigned)it0);                                \
  hipLaunchKernelGGL((k_ransac_estimate<NSV>), eg, dim3(kBlock), 0, S, d_desc, d_st, k, ca);
      switch (ns) {
        case 3: ER_RS_NS(3) break;
        case 4: ER_RS_NS(4) break;
        case 5: ER_RS_NS(5) break;
        default: ER_RS_NS(6) break;
      }
#undef ER_RS_NS
      hipLaunchKernelGGL(k_ransac_accept, dim3(m), dim3(1024), 0, S, d_desc, d_st);
      hipLaunchKernelGGL(k_ransac_score, dim3(score_bx, score_by, m), dim3(kBlock), 0, S, d_desc, d_st, radius, max_range);
      hipLaunchKernelGGL(k_ransac_select, dim3(m), dim3(kBlock), 0, S, d_desc, d_st, p->inlier_fraction, p->inlier_number);
      ER_HIP_TRY(hipGetLastError());
    }
    ER_HIP_TRY(hipMemcpyAsync(hs.data(), d_st, (size_t)m * sizeof(RsState), hipMemcpyDeviceToHost, S));
    ER_HIP_TRY(hipStreamSynchronize(S));
    c_src.clear(); c_tgt.clear(); c_M.clear();
    for (int q = 0; q < m; q++) {
      const RsState& h = hs[(size_t)q];
      const int i = w0 + q;
      converged[i] = h.converged;
      for (int e = 0; e < 16; e++) T_out[(size_t)i * 16 + e] = h.converged ? h.best_M[e] : (e % 5 == 0 ? 1.f : 0.f);
      if (n_inliers) n_inliers[i] = h.converged ? h.best_count : 0;
      if (error) error[i] = h.converged ? h.best_err : (double)FLT_MAX;
      if (stats) {
        stats[i].iterations = p->max_iterations;
        stats[i].polygon_rejections = (long long)p->max_iterations - h.tot_surv;
        stats[i].normal_rejections = h.tot_surv - h.tot_acc;
        stats[i].scored = h.tot_acc;
      }
      if (info_s) std::fill(info_s + (size_t)i * 36, info_s + (size_t)i * 36 + 36, 0.0);
      if (info_t) std::fill(info_t + (size_t)i * 36, info_t + (size_t)i * 36 + 36, 0.0);
      if (h.converged && (info_s || info_t)) {
        c_src.push_back(src[i]); c_tgt.push_back(tgt[i]);
        c_M.insert(c_M.end(), h.best_M, h.best_M + 16);
      }
    }
    if (!c_src.empty()) {
      const int nc = (int)c_src.size();
      c_is.assign((size_t)nc * 36, 0.0); c_it.assign((size_t)nc * 36, 0.0);
      if (L.ransac_information(nc, c_src.data(), c_tgt.data(), c_M.data(), radius, info_s ? c_is.data() : nullptr, info_t ? c_it.data() : nullptr)) return 1;
      for (int q = 0, c = 0; q < m; q++)
        if (hs[(size_t)q].converged) {
          if (info_s) std::copy(c_is.begin() + (size_t)c * 36, c_is.begin() + (size_t)c * 36 + 36, info_s + (size_t)(w0 + q) * 36);
          if (info_t) std::copy(c_it.begin() + (size_t)c * 36, c_it.begin() + (size_t)c * 36 + 36, info_t + (size_t)(w0 + q) * 36);
          c++;
        }
    }
  }
  if (aux || aux_count) {                                       // (the single call: one pair, one wave)
    const long long scored = hs[0].tot_acc;
    if (aux_capacity > 0 && scored > 0)
      ER_HIP_TRY(hipMemcpy(aux, d_aux, (size_t)std::min<long long>(scored, aux_capacity) * sizeof(er_ransac_aux), hipMemcpyDeviceToHost));
    if (aux_count) *aux_count = (int)std::min<long long>(scored, 0x7fffffff);
  }
  return 0;
}

}  // namespace

extern "C" {

int er_features_create(const float* feat_host, int n, int dim, int device, er_features_t* out) {
  if (!out) return er::fail("er_features_create: out is NULL");
  *out = nullptr;
  if (no_device("er_features_create")) return 1;
  if (n < 0 || (n > 0 && !feat_host)) return er::fail("er_features_create: bad arguments");
  if (dim < 1 || dim > 64) return er::fail("er_features_create: %d dimensions, must be 1 .. 64", dim);
  if (n >= (1 << 27)) return er::fail("er_features_create: %d descriptors are too many", n);
  const int dp = (dim + 7) / 8 * 8;
  std::vector<float> pad((size_t)std::max(n, 1) * dp, 0.f);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < dim; j++) {
      const float v = feat_host[(size_t)i * dim + j];
      if (!(std::fabs(v) <= 1e15f)) return er::fail("er_features_create: descriptor %d, dimension %d is not finite or larger than 1e15", i, j);
      pad[(size_t)i * dp + j] = v;
    }
  ER_HIP_TRY(hipSetDevice(device));
  er_features_s* f = new er_features_s();
  f->device = device; f->n = n; f->dim = dim; f->dp = dp;
  if (f->d.reserve(pad.size(), "er_features_create")) {
    delete f;
    return 1;
  }
  if (hipMemcpy(f->d, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    delete f;
    return er::fail("er_features_create: %s", hipGetErrorString(hipGetLastError()));
  }
  *out = f;
  return 0;
}

int er_features_destroy(er_features_t f) {
  if (!f) return 0;
  (void)hipSetDevice(f->device);
  delete f;
  return 0;
}

int er_features_size(er_features_t f) { return f ? f->n : -1; }

int er_feature_knn(er_features_t src, er_features_t tgt, int k, int* idx_host, float* sqdist_host) {
  if (no_device("er_feature_knn")) return 1;
  if (check_features(src, tgt, k, "er_feature_knn")) return 1;
  StreamLease L;
  if (L.acquire(src->device)) return 1;
  DevScope B;
  int *d_idx, *pi;
  float *d_dist, *pd;
  const size_t m = (size_t)src->n * k, part = knn_plan(src->n, tgt->n, k, nullptr, nullptr);
  if (B.alloc(&d_idx, m, "er_feature_knn")) return 1;
  if (B.alloc(&d_dist, m, "er_feature_knn")) return 1;
  if (B.alloc(&pd, part, "er_feature_knn")) return 1;
  if (B.alloc(&pi, part, "er_feature_knn")) return 1;
  if (feature_knn_device(src, tgt, k, L.stream, d_idx, d_dist, pd, pi)) return 1;
  if (idx_host) ER_HIP_TRY(hipMemcpyAsync(idx_host, d_idx, m * sizeof(int), hipMemcpyDeviceToHost, L.stream));
  if (sqdist_host) ER_HIP_TRY(hipMemcpyAsync(sqdist_host, d_dist, m * sizeof(float), hipMemcpyDeviceToHost, L.stream));
  ER_HIP_TRY(hipStreamSynchronize(L.stream));
  return 0;
}

int er_ransac_hypotheses(er_cloud_t src, er_cloud_t tgt, int n_hyp, int nr_samples, const int* sample_idx, const int* corr_idx, float similarity,
                         float angle_diff, int* status, float* M) {
  if (no_device("er_ransac_hypotheses")) return 1;
  if (!src || !tgt) return er::fail("er_ransac_hypotheses: NULL cloud");
  if (src->device != tgt->device) return er::fail("er_ransac_hypotheses: source and target live on different devices");
  if (n_hyp < 0 || (n_hyp > 0 && (!sample_idx || !corr_idx || !status || !M))) return er::fail("er_ransac_hypotheses: bad arguments");
  if (nr_samples < 3 || nr_samples > er_rs::kMaxSamples) return er::fail("er_ransac_hypotheses: nr_samples = %d, must be 3 .. 6", nr_samples);
  if (!(similarity >= 0.f && similarity < 1.f)) return er::fail("er_ransac_hypotheses: illegal prerejection similarity threshold %g, must be in [0,1[", (double)similarity);
  const size_t m = (size_t)n_hyp * nr_samples;
  for (size_t e = 0; e < m; e++)
    if (sample_idx[e] < 0 || sample_idx[e] >= src->n || corr_idx[e] < 0 || corr_idx[e] >= tgt->n)
      return er::fail("er_ransac_hypotheses: hypothesis %d names a point outside its cloud", (int)(e / nr_samples));
  if (n_hyp == 0) return 0;
  StreamLease L;
  if (L.acquire(src->device)) return 1;
  hipStream_t S = L.stream;
  DevScope B;
  int *d_s, *d_c, *d_st;
  float* d_M;
  if (B.alloc(&d_s, m, "er_ransac_hypotheses")) return 1;
  if (B.alloc(&d_c, m, "er_ransac_hypotheses")) return 1;
  if (B.alloc(&d_st, (size_t)n_hyp, "er_ransac_hypotheses")) return 1;
  if (B.alloc(&d_M, (size_t)n_hyp * 16, "er_ransac_hypotheses")) return 1;
  ER_HIP_TRY(hipMemcpyAsync(d_s, sample_idx, m * sizeof(int), hipMemcpyHostToDevice, S));
  ER_HIP_TRY(hipMemcpyAsync(d_c, corr_idx, m * sizeof(int), hipMemcpyHostToDevice, S));
  const float simsq = similarity * similarity;
  const double ca = std::cos((double)angle_diff);
  const dim3 grid(nblocks_of(n_hyp));
  switch (nr_samples) {
    case 3: hipLaunchKernelGGL((k_ransac_hypotheses<3>), grid, dim3(kBlock), 0, S, src->xn, tgt->xn, n_hyp, d_s, d_c, simsq, ca, d_st, d_M); break;
    case 4: hipLaunchKernelGGL((k_ransac_hypotheses<4>), grid, dim3(kBlock), 0, S, src->xn, tgt->xn, n_hyp, d_s, d_c, simsq, ca, d_st, d_M); break;
    case 5: hipLaunchKernelGGL((k_ransac_hypotheses<5>), grid, dim3(kBlock), 0, S, src->xn, tgt->xn, n_hyp, d_s, d_c, simsq, ca, d_st, d_M); break;
    default: hipLaunchKernelGGL((k_ransac_hypotheses<6>), grid, dim3(kBlock), 0, S, src->xn, tgt->xn, n_hyp, d_s, d_c, simsq, ca, d_st, d_M); break;
  }
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipMemcpyAsync(status, d_st, (size_t)n_hyp * sizeof(int), hipMemcpyDeviceToHost, S));
  ER_HIP_TRY(hipMemcpyAsync(M, d_M, (size_t)n_hyp * 16 * sizeof(float), hipMemcpyDeviceToHost, S));
  ER_HIP_TRY(hipStreamSynchronize(S));
  return 0;
}

int er_ransac_params_default(er_ransac_params* p) {
  if (!p) return er::fail("er_ransac_params_default: NULL argument");
  *p = er_ransac_params{4000000, 4, 2, 0.9f, 0.075f, 0.33f, 30000, 0.52359878f, 0u, 0};
  return 0;
}

int er_ransac_align(er_cloud_t src, er_cloud_t tgt, er_features_t src_feat, er_features_t tgt_feat, const er_ransac_params* p, float T_out[16],
                    int* converged, int* n_inliers, double* error, er_ransac_stats* stats, er_ransac_aux* aux, int aux_capacity, int* aux_count) {
  const char* who = "er_ransac_align";
  if (no_device(who)) return 1;
  if (!p || !T_out || !converged || aux_capacity < 0 || (aux_capacity > 0 && !aux)) return er::fail("%s: bad arguments", who);
  if (ransac_check(src, tgt, src_feat, tgt_feat, p, who)) return 1;
  return ransac_run(1, &src, &tgt, &src_feat, &tgt_feat, p, nullptr, 1, T_out, converged, n_inliers, error, stats, nullptr, nullptr, aux, aux_capacity,
                    aux_count);
}

int er_ransac_align_batch(int n_pairs, const er_cloud_t* src, const er_cloud_t* tgt, const er_features_t* src_feat, const er_features_t* tgt_feat,
                          const er_ransac_params* p, const unsigned int* seeds, int max_concurrent, float* T_out, int* converged, int* n_inliers,
                          double* error, er_ransac_stats* stats, double* info_source36, double* info_target36) {
  const char* who = "er_ransac_align_batch";
  if (n_pairs == 0) return 0;
  if (no_device(who)) return 1;
  if (n_pairs < 0) return er::fail("%s: n_pairs = %d is negative", who, n_pairs);
  if (max_concurrent < 0) return er::fail("%s: max_concurrent = %d is negative", who, max_concurrent);
  if (!src || !tgt || !src_feat || !tgt_feat) return er::fail("%s: a NULL array for %d pairs", who, n_pairs);
  if (!p || !T_out || !converged) return er::fail("%s: bad arguments", who);
  char name[64];
  for (int i = 0; i < n_pairs; i++) {
    snprintf(name, sizeof name, "%s: pair %d", who, i);
    if (ransac_check(src[i], tgt[i], src_feat[i], tgt_feat[i], p, name)) return 1;
    if (src[i]->device != src[0]->device) return er::fail("%s: all pairs of one list must live on one device", name);
  }
  return ransac_run(n_pairs, src, tgt, src_feat, tgt_feat, p, seeds, max_concurrent, T_out, converged, n_inliers, error, stats, info_source36,
                    info_target36, nullptr, 0, nullptr);
}

}  // extern "C"
