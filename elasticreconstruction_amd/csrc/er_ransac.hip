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

// idx / dist: device arrays [ns][k].  Enqueued on `st`; pd / pi are scratch the caller frees after the stream has drained.
int feature_knn_device(const er_features_s* s, const er_features_s* t, int k, hipStream_t st, int* d_idx, float* d_dist, float** pd_out, int** pi_out) {
  const int K = k <= 2 ? 2 : 8;
  const int nbx = nblocks_of(s->n);
  int segs = std::max(1, std::min(64, 1024 / nbx));
  int seg_len = ((t->n + segs - 1) / segs + kKnnTile - 1) / kKnnTile * kKnnTile;
  segs = (t->n + seg_len - 1) / seg_len;
  float* pd = nullptr;
  int* pi = nullptr;
  ER_HIP_TRY(hipMalloc((void**)&pd, (size_t)segs * s->n * K * sizeof(float)));
  *pd_out = pd;
  ER_HIP_TRY(hipMalloc((void**)&pi, (size_t)segs * s->n * K * sizeof(int)));
  *pi_out = pi;
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

// One lane per iteration it0 + gid; bit gid of `mask` = the iteration passed the polygon test.  Every wave of the grid writes its word.
template <int NS>
__global__ __launch_bounds__(kBlock) void k_ransac_propose(const float4* __restrict__ sxn, const float4* __restrict__ txn, int n_src,
                                                           const int* __restrict__ knn, int k, unsigned seed, unsigned it0, int count, float simsq,
                                                           unsigned long long* __restrict__ mask) {
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
  if ((threadIdx.x & 63) == 0) mask[gid >> 6] = m;
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

// One workgroup: the set bits of `words` mask words -> list[] = iteration numbers, ascending.
__global__ __launch_bounds__(1024) void k_ransac_list(const unsigned long long* __restrict__ mask, int words, unsigned it0, int* __restrict__ list,
                                                      RsState* __restrict__ st) {
  __shared__ int sh[1024];
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

template <int NS>
__global__ __launch_bounds__(kBlock) void k_ransac_estimate(const float4* __restrict__ sxn, const float4* __restrict__ txn, int n_src,
                                                            const int* __restrict__ knn, int k, unsigned seed, const int* __restrict__ list,
                                                            const RsState* __restrict__ st, double cos_angle, int* __restrict__ status,
                                                            float* __restrict__ Mout) {
  const int n = st->n_surv;
  for (int j = blockIdx.x * kBlock + (int)threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const unsigned it = (unsigned)list[j];
    int s[NS], c[NS];
    er_rs::select_samples<NS>(seed, it, n_src, s);
#pragma unroll
    for (int i = 0; i < NS; i++) c[i] = rs_pick(knn, k, seed, it, i, s[i]);
    RsPoints S, T;
    rs_load<NS>(sxn, s, S);
    rs_load<NS>(txn, c, T);
    float M[16];
    status[j] = rs_estimate<NS>(S, T, cos_angle, M);
#pragma unroll
    for (int e = 0; e < 16; e++) Mout[(size_t)j * 16 + e] = M[e];
  }
}

// One workgroup: acc[] = the positions j of the survivors with status 0, ascending; zeroes their score slots.
__global__ __launch_bounds__(1024) void k_ransac_accept(const int* __restrict__ status, int* __restrict__ acc, RsState* __restrict__ st,
                                                        int* __restrict__ count, long long* __restrict__ sum) {
  __shared__ int sh[1024];
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

// k_ransac_fitness for the accepted hypotheses of a chunk: blockIdx.y strides over them, blockIdx.x over the source points.  The inlier
// distances are added as 64-bit integers (d * scale truncated, scale a power of two with n * max_range * scale < 2^61): the sum does not
// depend on the order of the workgroups.
__global__ __launch_bounds__(kBlock) void k_ransac_score(const float4* __restrict__ src_sorted, int n, const float* __restrict__ Mbuf,
                                                         const int* __restrict__ acc, const RsState* __restrict__ st, Grid g, float radius,
                                                         float max_range, double scale, int* __restrict__ count, long long* __restrict__ sum) {
  __shared__ NnSh sh;
  __shared__ int pc[kBlock / 64];
  __shared__ long long ps[kBlock / 64];
  const int nh = st->n_acc;
  for (int h = blockIdx.y; h < nh; h += gridDim.y) {
    const float* hyp = Mbuf + (size_t)acc[h] * 16;
    float M[12];
#pragma unroll
    for (int q = 0; q < 12; q++) M[q] = hyp[q];
    int local = 0;
    long long dsum = 0;
    for (int base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
      const int k = base + (int)threadIdx.x;
      float qx = 0.f, qy = 0.f, qz = 0.f, d;
      if (k < n) {
        const float4 s = src_sorted[k];
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

// One workgroup: the aux rows of the chunk's scored hypotheses and the running (error, iteration) minimum over the acceptable ones.
__global__ __launch_bounds__(kBlock) void k_ransac_select(const int* __restrict__ list, const int* __restrict__ acc, const float* __restrict__ Mbuf,
                                                          const int* __restrict__ count, const long long* __restrict__ sum, RsState* __restrict__ st,
                                                          int n_src, float inlier_fraction, int inlier_number, double inv_scale,
                                                          er_ransac_aux* __restrict__ aux, long long aux_cap) {
  __shared__ double s_err[kBlock];
  __shared__ int s_it[kBlock], s_h[kBlock];
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
  if (hipMalloc((void**)&f->d, pad.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(f->d, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    if (f->d) (void)hipFree(f->d);
    delete f;
    return er::fail("er_features_create: %s", hipGetErrorString(hipGetLastError()));
  }
  *out = f;
  return 0;
}

int er_features_destroy(er_features_t f) {
  if (!f) return 0;
  (void)hipSetDevice(f->device);
  if (f->d) (void)hipFree(f->d);
  delete f;
  return 0;
}

int er_features_size(er_features_t f) { return f ? f->n : -1; }

int er_feature_knn(er_features_t src, er_features_t tgt, int k, int* idx_host, float* sqdist_host) {
  if (no_device("er_feature_knn")) return 1;
  if (check_features(src, tgt, k, "er_feature_knn")) return 1;
  StreamLease L;
  if (L.acquire(src->device)) return 1;
  DevBufs B;
  int* d_idx;
  float *d_dist, *pd = nullptr;
  int* pi = nullptr;
  const size_t m = (size_t)src->n * k;
  ER_HIP_TRY(B.alloc(&d_idx, m * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_dist, m * sizeof(float)));
  const int rc = feature_knn_device(src, tgt, k, L.stream, d_idx, d_dist, &pd, &pi);
  if (pd) B.p.push_back(pd);
  if (pi) B.p.push_back(pi);
  if (rc) return 1;
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
  DevBufs B;
  int *d_s, *d_c, *d_st;
  float* d_M;
  ER_HIP_TRY(B.alloc(&d_s, m * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_c, m * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_st, (size_t)n_hyp * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_M, (size_t)n_hyp * 16 * sizeof(float)));
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
  const int chunk = std::min(p->max_iterations, p->chunk_iterations > 0 ? p->chunk_iterations : (1 << 20));
  const int n = src->n, k = p->k_correspondences, ns = p->nr_samples;
  StreamLease L;
  if (L.acquire(src->device)) return 1;
  hipStream_t S = L.stream;
  DevBufs B;
  int *d_knn, *d_list, *d_status, *d_acc, *d_count;
  float *d_kd, *d_M, *pd = nullptr;
  int* pi = nullptr;
  unsigned long long* d_mask;
  long long* d_sum;
  RsState* d_st;
  er_ransac_aux* d_aux;
  const size_t words = ((size_t)chunk + kBlock - 1) / kBlock * (kBlock / 64);
  ER_HIP_TRY(B.alloc(&d_knn, (size_t)n * k * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_kd, (size_t)n * k * sizeof(float)));
  ER_HIP_TRY(B.alloc(&d_mask, words * sizeof(unsigned long long)));
  ER_HIP_TRY(B.alloc(&d_list, (size_t)chunk * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_status, (size_t)chunk * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_acc, (size_t)chunk * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_count, (size_t)chunk * sizeof(int)));
  ER_HIP_TRY(B.alloc(&d_sum, (size_t)chunk * sizeof(long long)));
  ER_HIP_TRY(B.alloc(&d_M, (size_t)chunk * 16 * sizeof(float)));
  ER_HIP_TRY(B.alloc(&d_st, sizeof(RsState)));
  ER_HIP_TRY(B.alloc(&d_aux, (size_t)aux_capacity * sizeof(er_ransac_aux)));
  const int krc = feature_knn_device(src_feat, tgt_feat, k, S, d_knn, d_kd, &pd, &pi);
  if (pd) B.p.push_back(pd);
  if (pi) B.p.push_back(pi);
  if (krc) return 1;
  ER_HIP_TRY(hipMemsetAsync(d_st, 0, sizeof(RsState), S));
  const float simsq = p->similarity * p->similarity, radius = p->max_corr_dist, max_range = radius * radius;
  const double ca = std::cos((double)p->angle_diff);
  const double bound = (double)n * (double)max_range;
  const int sexp = 60 - (bound > 0.0 ? std::ilogb(bound) : 0);
  const double scale = std::ldexp(1.0, sexp), inv_scale = std::ldexp(1.0, -sexp);
  const int est_blocks = 256, score_bx = std::max(1, std::min(nblocks_of(n), 8)), score_by = 512;
  for (int it0 = 0; it0 < p->max_iterations; it0 += chunk) {
    const int cnt = std::min(chunk, p->max_iterations - it0);
    const dim3 pg(nblocks_of(cnt));
    const int w = (cnt + 63) / 64;
#define ER_RS_NS(NSV)                                                                                                                              \
  hipLaunchKernelGGL((k_ransac_propose<NSV>), pg, dim3(kBlock), 0, S, src->xn, tgt->xn, n, d_knn, k, p->seed, (unsigned)it0, cnt, simsq, d_mask);   \
  hipLaunchKernelGGL(k_ransac_list, dim3(1), dim3(1024), 0, S, d_mask, w, (unsigned)it0, d_list, d_st);                                            \
  hipLaunchKernelGGL((k_ransac_estimate<NSV>), dim3(est_blocks), dim3(kBlock), 0, S, src->xn, tgt->xn, n, d_knn, k, p->seed, d_list, d_st, ca,      \
                     d_status, d_M);
    switch (ns) {
      case 3: ER_RS_NS(3) break;
      case 4: ER_RS_NS(4) break;
      case 5: ER_RS_NS(5) break;
      default: ER_RS_NS(6) break;
    }
#undef ER_RS_NS
    hipLaunchKernelGGL(k_ransac_accept, dim3(1), dim3(1024), 0, S, d_status, d_acc, d_st, d_count, d_sum);
    hipLaunchKernelGGL(k_ransac_score, dim3(score_bx, score_by), dim3(kBlock), 0, S, src->sorted, n, d_M, d_acc, d_st, tgt->grid, radius, max_range,
                       scale, d_count, d_sum);
    hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(kBlock), 0, S, d_list, d_acc, d_M, d_count, d_sum, d_st, n, p->inlier_fraction, p->inlier_number,
                       inv_scale, d_aux, (long long)aux_capacity);
    ER_HIP_TRY(hipGetLastError());
  }
  RsState hs;
  ER_HIP_TRY(hipMemcpyAsync(&hs, d_st, sizeof hs, hipMemcpyDeviceToHost, S));
  ER_HIP_TRY(hipStreamSynchronize(S));
  const long long scored = hs.tot_acc;
  if (aux_capacity > 0 && scored > 0)
    ER_HIP_TRY(hipMemcpy(aux, d_aux, (size_t)std::min<long long>(scored, aux_capacity) * sizeof(er_ransac_aux), hipMemcpyDeviceToHost));
  if (aux_count) *aux_count = (int)std::min<long long>(scored, 0x7fffffff);
  *converged = hs.converged;
  for (int e = 0; e < 16; e++) T_out[e] = hs.converged ? hs.best_M[e] : (e % 5 == 0 ? 1.f : 0.f);
  if (n_inliers) *n_inliers = hs.converged ? hs.best_count : 0;
  if (error) *error = hs.converged ? hs.best_err : (double)FLT_MAX;
  if (stats) {
    stats->iterations = p->max_iterations;
    stats->polygon_rejections = (long long)p->max_iterations - hs.tot_surv;
    stats->normal_rejections = hs.tot_surv - hs.tot_acc;
    stats->scored = hs.tot_acc;
  }
  return 0;
}

}  // extern "C"
