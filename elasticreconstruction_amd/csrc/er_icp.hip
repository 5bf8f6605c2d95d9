// er_icp.hip -- path B of liber_hip.so: pairwise ICP refinement + correspondence building on MI355X
// (gfx950).  Replaces the numeric core of CCorresApp::Registration / FindCorrespondence
// (BuildCorrespondence/CorresApp.cpp:112-319) including the PCL pieces it calls
// (pcl::IterativeClosestPoint + TransformationEstimationPointToPlaneLLS + KdTreeFLANN, :295-312).
// PCL semantics follow SURVEY.md Appendix B (PCL 1.7; the library itself is not vendored -- see
// oracle/icp_oracle.cpp's header for what is assumed and DESIGN.md "parity unpinned").
//
// The clouds (one er_cloud_s per fragment, uploaded once, reused by every pair: layout and grid build in er_cloud.hip) are immutable; what a list of
// pairs needs while it is processed are GROUP workspaces (streams, per-pair descriptors and ICP states, scratch slabs cut into one slice per pair) borrowed
// from a per-device pool, so any number of pair lists can be in flight.  er_ransac.hip and er_fpfh.hip borrow their stream from the same pool (er::StreamLease).
// Queries run in the SOURCE cloud's own cell-sorted order (thread t takes sorted[t]), so the lanes of a wave
// walk the same few target cells together (coalesced / broadcast candidate loads); results are written back
// by original index.  The NN search is block-cooperative (nn_block, er_nn.h); candidates stream from L2 as 16-byte loads.
// Every stage processes a whole GROUP of pairs per launch (blockIdx.y = pair; "pair groups" below):
//   k_count_inliers   transform (float64 -> float32) + NN + count           (Registration pre-check)
//   k_icp_iter        one ICP iteration: [apply guess / last increment] + NN + point-to-plane rows -> 27+2 float64 sums
//                     (4 points per thread -> wave shuffle -> LDS -> per-workgroup partial)
//   k_icp_final       one workgroup per pair: fixed-order total, 6x6 solve, increment, PCL's stop rule -- the loop stays on the device
//   k_find_corr       transform points+normals + NN + distance/normal tests -> match[orig index];
//                     k_count_blocks (+ information-matrix sums) + k_scan_blocks + k_compact = stable compaction in file order
// Reductions and scans, not contractions: no MFMA.
#include "er_cloud.h"
#include "er_nn.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace er;

namespace {

constexpr int kAcc = 32;   // 21 ATA + 6 ATb + sum d^2 + count (+ padding)

struct Mat12d { double m[12]; };
struct Mat12f { float m[12]; };

constexpr int kPrecheckUnroll = 3;   // candidates per trip of the any-hit pre-check (see nn_block)

// pcl::transformPointCloudWithNormals with a Matrix4d: float64 evaluation, float32 storage.
__device__ __forceinline__ void xform_d(const Mat12d& T, float x, float y, float z, float& ox, float& oy, float& oz) {
  const double dx = x, dy = y, dz = z;
  ox = (float)(((T.m[0] * dx + T.m[1] * dy) + T.m[2] * dz) + T.m[3]);
  oy = (float)(((T.m[4] * dx + T.m[5] * dy) + T.m[6] * dz) + T.m[7]);
  oz = (float)(((T.m[8] * dx + T.m[9] * dy) + T.m[10] * dz) + T.m[11]);
}

// RansacCurvature::getFitness (GlobalRegistration/RansacCurvature.h:661-704) for MANY pose hypotheses of one
// (source, target) pair: blockIdx.y = hypothesis, blockIdx.x strides over the source points.  Float32 transform
// ([PCL] transformPointCloud with a Matrix4f), exact NN, inlier iff d < threshold^2 (float compare, :670,:687);
// per hypothesis the inlier count (exact) and the float64 sum of the inlier distances.
__global__ __launch_bounds__(kBlock) void k_ransac_fitness(const float4* __restrict__ src_sorted, int n, const float* __restrict__ hyp,
                                                           int hyp0, Grid g, float radius, float max_range,
                                                           int* __restrict__ count, double* __restrict__ sum) {
  __shared__ NnSh sh;
  const int h = hyp0 + blockIdx.y;
  float M[12];
#pragma unroll
  for (int q = 0; q < 12; q++) M[q] = hyp[(size_t)h * 16 + q];
  int local = 0;
  double dsum = 0.0;
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
      dsum += (double)d;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    local += __shfl_down(local, off);
    dsum += __shfl_down(dsum, off);
  }
  __shared__ int pc[kBlock / 64];
  __shared__ double ps[kBlock / 64];
  if ((threadIdx.x & 63) == 0) {
    pc[threadIdx.x >> 6] = local;
    ps[threadIdx.x >> 6] = dsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    double s = 0.0;
    for (int w = 0; w < kBlock / 64; w++) {
      c += pc[w];
      s += ps[w];
    }
    if (c) {
      atomicAdd(&count[h], c);
      atomicAdd(&sum[h], s);
    }
  }
}

// ---- pair groups -------------------------------------------------------------------------------------------------------
// The reference's two loops run over a LIST of fragment pairs (CorresApp.cpp:121,220: #pragma omp parallel for).  Here a whole
// group of pairs goes through every stage in ONE launch: blockIdx.y = pair, blockIdx.x = a slice of that pair's source points.
// A 250 k-point pair alone is ~1000 workgroups of latency-bound exact-NN work -- half of what the 256 CUs hold -- and every
// launch, memset and small copy costs 5-20 us of an otherwise idle stream; 50 pairs per launch fill the chip and turn the
// host side into a handful of calls per stage (round 2: ~30 launches and ~7 copies PER PAIR over four streams).
// PairDev = what the kernels need to know about one pair of the group; read with scalar loads (blockIdx.y is wave-uniform).
struct PairDev {
  const float4* src_sorted;      // source, cell-sorted {x, y, z, original index}
  const float* src_xyz;          // source, file order (information matrix, CorresApp.cpp:192-196)
  const float* src_nrm;
  const float* tgt_xyz;
  const float* tgt_nrm;
  const float4* tgt_xn;          // target, file order, {xyz | normal} records of 32 bytes
  Grid g;                        // the target's uniform grid
  Mat12d T;                      // transform of the pre-check / FindCorrespondence (Matrix4d, rows 0..2)
  float* X;                      // [3 n]   ICP: the source as the loop transforms it (cell-sorted order)
  int* match;                    // [n]     FindCorrespondence: NN index or -1, file order
  int* block_count;              // [nb]
  int* block_offset;             // [nb]
  int* pairs;                    // [2 n]   compacted (target index, source index) list
  double* partial;               // [nbi][32] per-workgroup sums of one ICP iteration
  int n, nb, nbi, pts;           // source points, ceil(n / 256); nbi, pts: unused since round 4 (the points per thread of k_icp_iter are a launch argument)
  double fx_scale[32];           // round 6: power-of-two scale of each of the 29 ICP sums (see k_icp_iter: fixed-point partial sums) ...
  double fx_inv[32];             // ... and its reciprocal
};

// ---- the ICP loop's state lives on the device ------------------------------------------------------------------------
// pcl::IterativeClosestPoint::align's loop variables (final_transformation_, the last increment, the previous MSE, the
// iteration counter and the convergence flags), one per pair of the group.  k_icp_final updates them from the iteration's sums
// -- 6x6 solve, increment, PCL's stop rule -- and k_icp_iter reads the increment (and the `done` flag) from here, so a whole
// chunk of iterations is enqueued without a host round trip; workgroups that find `done` set return at once.
struct IcpDev {
  float fin[16];           // final_transformation_ (= the guess before the first iteration)
  float delta[16];         // last increment (identity before the first solve)
  float prev_delta[16];
  double prev_mse;
  int iter, done, conv, apply;   // apply: the next k_icp_iter multiplies X by delta first
  int init_apply, pad[3];        // iteration 0 reads the source itself and applies the guess unless it is the identity
};

struct IcpParams {
  double eps;
  int max_iter, stop_rule;
};

// Dense 6x6 solve by Gaussian elimination with partial pivoting (PCL: ATA.inverse() * ATb).
__device__ bool dev_solve6x6(double A[6][6], double b[6], double x[6]) {
  for (int c = 0; c < 6; c++) {
    int p = c;
    for (int r = c + 1; r < 6; r++)
      if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
    if (A[p][c] == 0.0 || !isfinite(A[p][c])) return false;
    if (p != c) {
      for (int k = 0; k < 6; k++) { const double t = A[p][k]; A[p][k] = A[c][k]; A[c][k] = t; }
      const double t = b[p]; b[p] = b[c]; b[c] = t;
    }
    for (int r = c + 1; r < 6; r++) {
      const double f = A[r][c] / A[c][c];
      for (int k = c; k < 6; k++) A[r][k] -= f * A[c][k];
      b[r] -= f * b[c];
    }
  }
  for (int r = 5; r >= 0; r--) {
    double s = b[r];
    for (int k = r + 1; k < 6; k++) s -= A[r][k] * x[k];
    x[r] = s / A[r][r];
  }
  return true;
}

// The same system by an LDL^T factorisation with compile-time indices (everything stays in registers; the pivoting
// elimination above indexes its rows dynamically, which puts the matrix into scratch memory: ~10 us for one thread).  A^T A is
// symmetric positive definite whenever the correspondences constrain all six degrees of freedom; returns false (caller
// falls back to the pivoting elimination) as soon as a pivot is not safely positive.
__device__ bool dev_solve6x6_spd(const double* acc, double x[6]) {
  double a[6][6];
  {
    int t = 0;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
      for (int c = r; c < 6; c++) a[r][c] = a[c][r] = acc[t++];
  }
  double d[6], y[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {                               // a[i][j] (i > j) becomes L_ij, d[j] the pivot
    double dj = a[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) dj -= a[j][k] * a[j][k] * d[k];
    if (!(dj > 1e-300) || !isfinite(dj)) return false;
    d[j] = dj;
    const double inv = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = a[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) s -= a[i][k] * a[j][k] * d[k];
      a[i][j] = s * inv;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {                               // L y = b
    double s = acc[21 + i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= a[i][k] * y[k];
    y[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {                              // L^T x = D^-1 y
    double s = y[i] / d[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) s -= a[k][i] * x[k];
    x[i] = s;
  }
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; i++) ok = ok && isfinite(x[i]);
  return ok;
}

// TransformationEstimationPointToPlaneLLS::constructTransformationMatrix: Rz(gamma) Ry(beta) Rx(alpha), float storage.
__device__ void dev_construct_increment(const double x[6], float M[16]) {
  double sa, ca, sb, cb, sg, cg;
  sincos(x[0], &sa, &ca);
  sincos(x[1], &sb, &cb);
  sincos(x[2], &sg, &cg);
  for (int i = 0; i < 16; i++) M[i] = 0.f;
  M[0] = (float)(cg * cb);
  M[1] = (float)(-sg * ca + cg * sb * sa);
  M[2] = (float)(sg * sa + cg * sb * ca);
  M[4] = (float)(sg * cb);
  M[5] = (float)(cg * ca + sg * sb * sa);
  M[6] = (float)(-cg * sa + sg * sb * ca);
  M[8] = (float)(-sb);
  M[9] = (float)(cb * sa);
  M[10] = (float)(cb * ca);
  M[3] = (float)x[3];
  M[7] = (float)x[4];
  M[11] = (float)x[5];
  M[15] = 1.f;
}

// One step of IterativeClosestPoint's loop after the correspondences of the iteration have been summed (acc[0..28]):
// min_number_correspondences_, estimateRigidTransformation, final = increment * final, ++iterations, the stop rule.
__device__ void dev_icp_decide(const double* acc, IcpDev* st, IcpParams P) {
  const double cnt = acc[28];
  double A[6][6], b[6], x[6];
  bool stop = false;
  st->apply = 0;
  if (cnt < 3.0) {                                           // min_number_correspondences_
    st->conv = 0;
    stop = true;
  } else {
    if (!dev_solve6x6_spd(acc, x)) {                         // (not positive definite: the general elimination decides)
      int t = 0;
      for (int r = 0; r < 6; r++)
        for (int c2 = r; c2 < 6; c2++) A[r][c2] = A[c2][r] = acc[t++];
      for (int r = 0; r < 6; r++) b[r] = acc[21 + r];
      if (!dev_solve6x6(A, b, x)) {
        st->conv = 0;
        stop = true;
      }
    }
  }
  if (!stop) {
    float D[16], F[16];
    for (int i = 0; i < 16; i++) st->prev_delta[i] = st->delta[i];
    dev_construct_increment(x, D);
    for (int r = 0; r < 4; r++)                              // final = increment * final
      for (int c = 0; c < 4; c++)
        F[r * 4 + c] = ((D[r * 4] * st->fin[c] + D[r * 4 + 1] * st->fin[4 + c]) + D[r * 4 + 2] * st->fin[8 + c]) + D[r * 4 + 3] * st->fin[12 + c];
    for (int i = 0; i < 16; i++) {
      st->fin[i] = F[i];
      st->delta[i] = D[i];
    }
    st->iter += 1;
    st->apply = 1;
    if (st->iter >= P.max_iter) {
      st->conv = 1;
      stop = true;
    } else if (P.stop_rule == 0) {                           // PCL 1.7 DefaultConvergenceCriteria
      const double cos_angle = 0.5 * (double)(D[0] + D[5] + D[10] - 1.f);
      const double tr2 = (double)(D[3] * D[3] + D[7] * D[7] + D[11] * D[11]);
      const double cur = acc[27] / cnt;
      if (cos_angle >= 1.0 - P.eps && tr2 <= P.eps) {
        st->conv = 1;
        stop = true;
      } else if (fabs(cur - st->prev_mse) < 1e-12) {
        st->conv = 1;
        stop = true;
      }
      st->prev_mse = cur;
    } else {                                                 // PCL <= 1.6
      float sum = 0.f;
      for (int i = 0; i < 16; i++) sum += D[i] - st->prev_delta[i];
      if (fabs((double)sum) < P.eps) {
        st->conv = 1;
        stop = true;
      }
    }
  }
  if (stop) st->done = 1;
}


constexpr int kIcpPtsMax = 2;              // slices of 256 source points per workgroup of k_icp_iter.  Round 6: two, not eight -- a workgroup of eight slices lasts
                                           // ~150 us of a ~700 us launch, and the launch ends with its last workgroup: ICP phase of the kinfu-like list 3.97 -> 3.48 ms,
                                           // hard list 5.17 -> 4.93, uniform 2.30 -> 2.21 (1: worse again; profiles/r06n_ab_icp_points_per_workgroup.txt).  Free to
                                           // choose since the sums are order-independent: every digest identical.

// Registration pre-check, CorresApp.cpp:257-264, for a group of pairs: counts[pair] = #{k : d2 < reg_dist^2}.  blockIdx.x
// strides over the pair's points; ONE atomic per workgroup.
__global__ __launch_bounds__(kBlock) void k_count_inliers(const PairDev* __restrict__ P, float radius, double maxd2, int* __restrict__ counts) {
  __shared__ NnSh sh;
  const PairDev& p = P[blockIdx.y];
  const int n = p.n;
  if ((int)blockIdx.x * kBlock >= n) return;                 // (wave-uniform: whole workgroups beyond a short pair's points)
  int local = 0;
  // any-hit threshold: a float strictly below both limits of the count test (d <= radius^2 as doubles, d < maxd2), so "d < hit2" implies the test
  const double lim = fmin((double)radius * (double)radius, maxd2);
  float hit2 = (float)lim;
  if ((double)hit2 >= lim) hit2 = __uint_as_float(__float_as_uint(hit2) - 1u);      // (lim > 0: the next float below)
  for (int base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
    const int k = base + (int)threadIdx.x;
    float qx = 0.f, qy = 0.f, qz = 0.f, d;
    if (k < n) {
      const float4 s = p.src_sorted[k];
      xform_d(p.T, s.x, s.y, s.z, qx, qy, qz);
    }
    const int i = nn_block<kPrecheckUnroll>(sh, p.g, k < n, qx, qy, qz, radius * radius, d, hit2);
    if (k < n && i >= 0 && (double)d <= (double)radius * (double)radius && (double)d < maxd2) local++;
  }
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off);
  __shared__ int part[kBlock / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kBlock / 64; w++) s += part[w];
    if (s) atomicAdd(&counts[blockIdx.y], s);
  }
}

// v (finite, |v| < 2^126) as a signed 128-bit integer, truncated towards zero below the units (hi: signed high word, lo: low word, two's complement).
__device__ __forceinline__ void to_fixed128(double v, long long& hi, unsigned long long& lo) {
  hi = 0;
  lo = 0;
  const double a = fabs(v);
  if (!(a > 0.0) || !(a < 8.0e37)) return;                       // 0, NaN, inf (cannot happen under the host's bound)
  int e;
  const double f = frexp(a, &e);                                 // a = f 2^e, 0.5 <= f < 1
  const unsigned long long m = (unsigned long long)ldexp(f, 53); // 2^52 <= m < 2^53, exact
  const int sh = e - 53;                                         // a = m 2^sh
  unsigned long long mh = 0, ml = 0;
  if (sh >= 64) mh = m << (sh - 64);
  else if (sh > 0) { mh = m >> (64 - sh); ml = m << sh; }
  else if (sh > -64) ml = m >> (-sh);
  if (v < 0.0) {                                                 // negate
    ml = ~ml + 1ull;
    mh = ~mh + (ml == 0ull ? 1ull : 0ull);
  }
  hi = (long long)mh;
  lo = ml;
}

// One ICP iteration of every ACTIVE pair of the group in one launch (blockIdx.y -> active[y] = the pair's slot):
//   iteration 0: X <- guess * source (IterativeClosestPoint::transformCloud, float32; a plain copy for an identity guess);
//   later:       X <- delta * X (the previous iteration's increment, float32);
//   correspondence estimation (exact NN, kept if d^2 <= max_dist^2); the sums of TransformationEstimationPointToPlaneLLS over
//   the kept correspondences: acc[0..20] upper triangle of AtA row by row, [21..26] Atb, [27] sum of d^2, [28] count.
// A thread takes `pts` points (slices of kBlock consecutive points: the NN search is a workgroup-cooperative step per slice)
// and adds their rows up privately; then thread rows -> wave shuffle tree -> LDS -> ONE partial vector per workgroup in
// `partial`; k_icp_final adds the partial vectors in a fixed order.  No float64 atomics: the sums are bit-reproducible from
// run to run (they still differ from a sequential CPU sum in the last bits).
__global__ __launch_bounds__(kBlock, 6) void k_icp_iter(const PairDev* __restrict__ P, const int* __restrict__ active, const IcpDev* __restrict__ S,
                                                     float radius, double maxd2, int pts) {
  __shared__ NnSh sh;
  const int slot = active[blockIdx.y];
  const PairDev& p = P[slot];
  const IcpDev& st = S[slot];
  if (st.done || (int)blockIdx.x >= (p.nb + pts - 1) / pts) return;   // the loop has ended / a shorter pair: wave-uniform exits
  const int n = p.n;
  const bool first = st.iter == 0;
  const int apply = first ? st.init_apply : st.apply;        // wave-uniform (scalar loads)
  const float* __restrict__ dm = first ? st.fin : st.delta;
  float* __restrict__ X = p.X;
  // Per slice of 256 points: NN, the point's 29 row values, a wave-level halving butterfly over the 32 value slots (29 used) -- at each
  // step the upper half of the lanes keeps the upper half of the remaining slots and hands the lower half over (and vice versa):
  // 16 + 8 + 4 + 2 + 1 exchanges and a final pair add instead of 29 x 6 shuffle-adds; lane l ends up with the wave total of slot
  // l >> 1 -- and the wave adds it to ITS row of the LDS accumulator.  The row values are live only between the NN search and the
  // butterfly, so the kernel keeps the register footprint of the plain NN kernels (occupancy is what the latency-bound search
  // needs: with thread-private float64 sums carried across the slices the kernel held 126 VGPRs = 4 waves per SIMD).
  // The sums ACROSS waves are exact.  A wave's 29 totals of one slice (float64, butterfly order: a function of the slice's 64 points alone) are converted
  // to 128-bit fixed point -- a power-of-two scale per sum, sized on the host from certain bounds (icp_fixed_point_scales: the total stays below 2^121);
  // with 120 bits the conversion is exact for anything but denormal dust -- and from there on everything is integer addition: associative, so a
  // pair's sums, its transform and its iteration count do not depend on `pts`, the chunking of the loop, the list the pair is part of or ER_ICP_SHARES.
  // (64 bits were not enough: a scale sized for the worst case leaves the point-to-plane residual sums A^T b -- terms of 1e-3 that cancel -- a
  // quantisation noise 300 x float64's, and on ill-posed pairs, where the solve divides noise by noise, 385 of configs[4]'s 2367 accepted pairs then
  // wandered for all 20 iterations instead of 12: profiles/r06g_allpairs_fixed_point_width.txt.)
  // The conversion waits until the slices are done: the wave totals of every slice are parked in LDS (8 KB) and converted after the loop, where the
  // registers of the search are free (inside the loop the 128-bit shifts pushed the kernel 12 bytes over its 80-VGPR budget).
  __shared__ double dslice[kIcpPtsMax][kBlock / 64][32];
  __shared__ unsigned long long part_lo[kBlock / 32][32];
  __shared__ long long part_hi[kBlock / 32][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < kIcpPtsMax * (kBlock / 64) * 32; t += kBlock) (&dslice[0][0][0])[t] = 0.0;   // (the first barrier of nn_block orders this)
  __shared__ double sfx[32];                                 // the scales wait in LDS: two registers less across the search (the kernel sits on its 80)
  if (threadIdx.x < 32) sfx[threadIdx.x] = p.fx_scale[threadIdx.x];
  for (int c = 0; c < pts; c++) {
    const int k = (blockIdx.x * pts + c) * kBlock + threadIdx.x;
    if ((blockIdx.x * pts + c) * kBlock >= n) break;         // wave-uniform
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (k < n) {
      if (first) {
        const float4 s = p.src_sorted[k];
        sx = s.x, sy = s.y, sz = s.z;
      } else {
        const ER_GLOBAL float* Xg = (const ER_GLOBAL float*)((const ER_GLOBAL char*)X + (unsigned)k * 12u);
        sx = Xg[0], sy = Xg[1], sz = Xg[2];
      }
      if (apply) {
        const float x = sx, y = sy, z = sz;
        sx = ((dm[0] * x + dm[1] * y) + dm[2] * z) + dm[3];
        sy = ((dm[4] * x + dm[5] * y) + dm[6] * z) + dm[7];
        sz = ((dm[8] * x + dm[9] * y) + dm[10] * z) + dm[11];
      }
      if (apply || first) {
        ER_GLOBAL float* Xw = (ER_GLOBAL float*)((ER_GLOBAL char*)X + (unsigned)k * 12u);
        Xw[0] = sx;
        Xw[1] = sy;
        Xw[2] = sz;
      }
    }
    float d;
    const int i = nn_block(sh, p.g, k < n, sx, sy, sz, radius * radius, d);
    double w[32];
#pragma unroll
    for (int t = 0; t < 32; t++) w[t] = 0.0;
    if (k < n && i >= 0 && (double)d <= (double)radius * (double)radius && !((double)d > maxd2)) {
      const ER_GLOBAL f4v* rec = (const ER_GLOBAL f4v*)((const ER_GLOBAL char*)p.tgt_xn + (unsigned)i * 32u);
      const f4v tp = rec[0], tn = rec[1];
      const float dx = tp.x, dy = tp.y, dz = tp.z, nx = tn.x, ny = tn.y, nz = tn.z;
      w[27] = (double)d;
      w[28] = 1.0;
      if (isfinite(sx) && isfinite(sy) && isfinite(sz) && isfinite(nx) && isfinite(ny) && isfinite(nz)) {
        const double a = (double)(nz * sy - ny * sz);      // float32 expressions widened to double (PCL)
        const double b = (double)(nx * sz - nz * sx);
        const double cc = (double)(ny * sx - nx * sy);
        const double dnx = nx, dny = ny, dnz = nz;
        w[0] = a * a;  w[1] = a * b;  w[2] = a * cc;  w[3] = a * dnx;  w[4] = a * dny;  w[5] = a * dnz;
        w[6] = b * b;  w[7] = b * cc;  w[8] = b * dnx; w[9] = b * dny; w[10] = b * dnz;
        w[11] = cc * cc; w[12] = cc * dnx; w[13] = cc * dny; w[14] = cc * dnz;
        w[15] = dnx * dnx; w[16] = dnx * dny; w[17] = dnx * dnz;
        w[18] = dny * dny; w[19] = dny * dnz;
        w[20] = dnz * dnz;
        const double e = (double)(nx * dx + ny * dy + nz * dz - nx * sx - ny * sy - nz * sz);
        w[21] = a * e; w[22] = b * e; w[23] = cc * e; w[24] = dnx * e; w[25] = dny * e; w[26] = dnz * e;
      }
    }
#pragma unroll
    for (int half = 16, mask = 32; half >= 1; half >>= 1, mask >>= 1) {
      const bool upper = (lane & mask) != 0;
#pragma unroll
      for (int t = 0; t < half; t++) {
        const double send = upper ? w[t] : w[t + half];
        const double keep = upper ? w[t + half] : w[t];
        w[t] = keep + __shfl_xor(send, mask);
      }
    }
    w[0] += __shfl_xor(w[0], 1);
    if ((lane & 1) == 0) dslice[c][wave][lane >> 1] = w[0];
  }
  __syncthreads();
  {
    const int slot = threadIdx.x & 31, g = threadIdx.x >> 5;     // 8 groups of 32 threads: group g converts slice g of this workgroup
    unsigned long long lo = 0;
    long long hi = 0;
    if (slot < 29 && g < pts) {
      const double fx = sfx[slot];
#pragma unroll
      for (int w2 = 0; w2 < kBlock / 64; w2++) {
        long long qh;
        unsigned long long ql;
        to_fixed128(dslice[g][w2][slot] * fx, qh, ql);           // (a power-of-two scale: the product is exact)
        const unsigned long long nlo = lo + ql;
        hi += qh + (long long)(nlo < lo);
        lo = nlo;
      }
    }
    part_lo[g][slot] = lo;
    part_hi[g][slot] = hi;
  }
  __syncthreads();
  if (threadIdx.x < 29) {
    unsigned long long lo = 0;
    long long hi = 0;
#pragma unroll
    for (int g = 0; g < kBlock / 32; g++) {
      const unsigned long long nlo = lo + part_lo[g][threadIdx.x];
      hi += part_hi[g][threadIdx.x] + (long long)(nlo < lo);
      lo = nlo;
    }
    unsigned long long* out = reinterpret_cast<unsigned long long*>(p.partial) + ((size_t)blockIdx.x * 32 + threadIdx.x) * 2;
    out[0] = lo;
    out[1] = (unsigned long long)hi;
  }
}

// Second half of the reduction, one workgroup PER ACTIVE PAIR: adds the pair's per-workgroup partial vectors in a fixed order
// (8 strided slices per value, then the slices in order) and decides -- 6x6 solve, increment, stop rule: the loop never leaves
// the device.  A separate launch on purpose: finishing inside k_icp_iter ("last workgroup done" ticket + __threadfence) costs
// an L2 write-back per workgroup on this multi-XCD part (measured in round 1: 100-600 us per launch instead of ~25).
// tot_out (NULL everywhere but er_icp_align_trace): the 29 totals as dev_icp_decide receives them, 32 doubles per active pair.
__global__ __launch_bounds__(kBlock) void k_icp_final(const PairDev* __restrict__ P, const int* __restrict__ active, IcpDev* __restrict__ S, IcpParams prm,
                                                      int pts, double* __restrict__ tot_out) {
  const int slot = active[blockIdx.x];
  IcpDev* st = S + slot;
  if (st->done) return;
  const unsigned long long* __restrict__ partial = reinterpret_cast<const unsigned long long*>(P[slot].partial);
  const int nparts = (P[slot].nb + pts - 1) / pts;
  const int val = threadIdx.x & 31, slice = threadIdx.x >> 5;   // 32 x 8
  unsigned long long lo = 0;                                    // (128-bit integer sums: any order gives the same total)
  long long hi = 0;
  if (val < 29) {
    for (int b = slice; b < nparts; b += 8) {
      const unsigned long long nlo = lo + partial[((size_t)b * 32 + val) * 2];
      hi += (long long)partial[((size_t)b * 32 + val) * 2 + 1] + (long long)(nlo < lo);
      lo = nlo;
    }
  }
  __shared__ unsigned long long fin_lo[8][32];
  __shared__ long long fin_hi[8][32];
  fin_lo[slice][val] = lo;
  fin_hi[slice][val] = hi;
  __syncthreads();
  __shared__ double tot[32];
  if (threadIdx.x < 29) {
    unsigned long long l = 0;
    long long h = 0;
#pragma unroll
    for (int sl = 0; sl < 8; sl++) {
      const unsigned long long nl = l + fin_lo[sl][threadIdx.x];
      h += fin_hi[sl][threadIdx.x] + (long long)(nl < l);
      l = nl;
    }
    // value = h 2^64 + l (two's complement): two roundings to float64, far below the wave sums' own
    tot[threadIdx.x] = (ldexp((double)h, 64) + (double)l) * P[slot].fx_inv[threadIdx.x];
    if (tot_out) tot_out[(size_t)blockIdx.x * kAcc + threadIdx.x] = tot[threadIdx.x];
  }
  __syncthreads();
  if (threadIdx.x == 0) dev_icp_decide(tot, st, prm);
}

// getFitnessScore-style diagnostic (logging only, CorresApp.cpp:307): per pair the sum and the number of the squared NN
// distances of final * source inside the search radius -> fit[2 pair], fit[2 pair + 1].
__global__ __launch_bounds__(kBlock) void k_fitness(const PairDev* __restrict__ P, const IcpDev* __restrict__ S, float radius, double* __restrict__ fit) {
  __shared__ NnSh sh;
  const PairDev& p = P[blockIdx.y];
  const int n = p.n;
  if ((int)blockIdx.x * kBlock >= n) return;
  const float* __restrict__ M = S[blockIdx.y].fin;
  double v[2] = {0.0, 0.0};
  for (int base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
    const int k = base + (int)threadIdx.x;
    float qx = 0.f, qy = 0.f, qz = 0.f, d;
    if (k < n) {
      const float4 s = p.src_sorted[k];
      qx = ((M[0] * s.x + M[1] * s.y) + M[2] * s.z) + M[3];
      qy = ((M[4] * s.x + M[5] * s.y) + M[6] * s.z) + M[7];
      qz = ((M[8] * s.x + M[9] * s.y) + M[10] * s.z) + M[11];
    }
    const int i = nn_block(sh, p.g, k < n, qx, qy, qz, radius * radius, d);
    if (k < n && i >= 0 && (double)d <= (double)radius * (double)radius) {
      v[0] += (double)d;
      v[1] += 1.0;
    }
  }
  __syncthreads();
  block_reduce_atomic<2>(v, fit + 2 * (size_t)blockIdx.y);
}

// FindCorrespondence, CorresApp.cpp:144-161: match[original index] = NN index passing the distance and normal tests, else -1.
__global__ __launch_bounds__(kBlock) void k_find_corr(const PairDev* __restrict__ P, float radius, double dist2, double normal_cos) {
  __shared__ NnSh sh;
  const PairDev& p = P[blockIdx.y];
  const int n = p.n;
  if ((int)blockIdx.x >= p.nb) return;
  const int q = blockIdx.x * kBlock + threadIdx.x;             // q = position in the source's cell-sorted order
  float qx = 0.f, qy = 0.f, qz = 0.f, d;
  int k = 0;
  if (q < n) {
    const float4 s = p.src_sorted[q];
    k = __float_as_int(s.w);                                   // original (file-order) index of this source point
    xform_d(p.T, s.x, s.y, s.z, qx, qy, qz);
  }
  const int i = nn_block(sh, p.g, q < n, qx, qy, qz, radius * radius, d);
  if (q >= n) return;
  int m = -1;
  if (i >= 0 && (double)d <= (double)radius * (double)radius && (double)d < dist2) {         // :154
    const double nx = p.src_nrm[3 * k], ny = p.src_nrm[3 * k + 1], nz = p.src_nrm[3 * k + 2];
    const float tnx = (float)((p.T.m[0] * nx + p.T.m[1] * ny) + p.T.m[2] * nz);              // n' = R n (double -> float)
    const float tny = (float)((p.T.m[4] * nx + p.T.m[5] * ny) + p.T.m[6] * nz);
    const float tnz = (float)((p.T.m[8] * nx + p.T.m[9] * ny) + p.T.m[10] * nz);
    // NormalDot, CorresApp.h:58-60: float32 products/sums, compared as double
    const float4 tn = p.tgt_xn[2 * (size_t)i + 1];                                              // the matched target normal: one aligned 16-byte load
    const float dot = (tn.x * tnx + tn.y * tny) + tn.z * tnz;
    if ((double)dot > normal_cos) m = i;                                                       // :155
  }
  p.match[k] = m;
}

// The accepted RANSAC hypothesis once more, this time keeping the lists (RansacCurvature.h:661-704: `inliers`, `inliers_target`):
// match[original source index] = NN index if d < threshold^2, else -1; acc[20] += d over the inliers.  (One pair: P[0].)
__global__ __launch_bounds__(kBlock) void k_ransac_match(const PairDev* __restrict__ P, Mat12f M, float radius, float max_range, double* __restrict__ acc) {
  __shared__ NnSh sh;
  const PairDev& p = P[0];
  const int n = p.n;
  const int q = blockIdx.x * kBlock + threadIdx.x;
  float qx = 0.f, qy = 0.f, qz = 0.f, d;
  int k = 0;
  if (q < n) {
    const float4 s = p.src_sorted[q];
    k = __float_as_int(s.w);
    qx = ((M.m[0] * s.x + M.m[1] * s.y) + M.m[2] * s.z) + M.m[3];
    qy = ((M.m[4] * s.x + M.m[5] * s.y) + M.m[6] * s.z) + M.m[7];
    qz = ((M.m[8] * s.x + M.m[9] * s.y) + M.m[10] * s.z) + M.m[11];
  }
  const int i = nn_block(sh, p.g, q < n, qx, qy, qz, radius * radius, d);
  const bool hit = q < n && i >= 0 && d < max_range;
  if (q < n) p.match[k] = hit ? i : -1;
  double v[1] = {hit ? (double)d : 0.0};
  __syncthreads();
  block_reduce_atomic<1>(v, acc + 20);
}

// Matches per block of 256 consecutive ORIGINAL indices (the order of the output list) and, optionally, the
// information matrix of CorresApp.cpp:186-208 over the matched, UNtransformed source points (target points: RansacCurvature.h
// :723-731 with which = 1):  info[0..2] = sum 2sx,2sy,2sz; [3..5] = sum (4sz^2+4sy^2),(4sz^2+4sx^2),(4sy^2+4sx^2);
// [6..8] = sum -4sysx, -4szsx, -4szsy; [9] = count   (the distinct terms of sum A^T A, A = [I | 2*skew-like(s)]); info is
// kAcc doubles per pair (source terms at 0, target terms at 10).
// A workgroup takes kCountSlices consecutive blocks, keeps the twenty sums thread-private across them and leaves ONE partial vector per workgroup in the
// pair's `partial` scratch (free here: the ICP loop that owns it has ended); k_scan_blocks adds the partial vectors in a fixed order: no float64
// atomics, a result that does not depend on arrival order.
constexpr int kCountSlices = 8;
__global__ __launch_bounds__(kBlock) void k_count_blocks(const PairDev* __restrict__ P, int want_source, int want_target) {
  const PairDev& p = P[blockIdx.y];
  const int n = p.n, nb = p.nb;
  const int b0 = blockIdx.x * kCountSlices;
  if (b0 >= nb) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int wcnt[kCountSlices][kBlock / 64];
  double v[20];
#pragma unroll
  for (int i = 0; i < 20; i++) v[i] = 0.0;
#pragma unroll
  for (int c = 0; c < kCountSlices; c++) {
    const int k = (b0 + c) * kBlock + (int)threadIdx.x;
    const int m = (b0 + c < nb && k < n) ? p.match[k] : -1;
    const bool hit = m >= 0;
    const unsigned long long b = __ballot(hit);
    if (lane == 0) wcnt[c][wave] = __popcll(b);
    if (hit) {                                                                                   // :192-204
#pragma unroll
      for (int which = 0; which < 2; which++) {
        if (!(which ? want_target : want_source)) continue;      // uniform
        const float* __restrict__ s = which ? p.tgt_xyz + 3 * (size_t)m : p.src_xyz + 3 * (size_t)k;
        const float sx = s[0], sy = s[1], sz = s[2];
        const double ax = (double)(2 * sx), ay = (double)(2 * sy), az = (double)(2 * sz);
        double* u = v + 10 * which;
        u[0] += ax; u[1] += ay; u[2] += az;
        u[3] += az * az + ay * ay;     // (0*0 + (-2sz)(-2sz)) + (2sy)(2sy)
        u[4] += az * az + ax * ax;     // ((2sz)(2sz) + 0*0) + (-2sx)(-2sx)
        u[5] += ay * ay + ax * ax;     // ((-2sy)(-2sy) + (2sx)(2sx)) + 0*0
        u[6] += ay * (-ax);            // (3,4): (2sy)(-2sx)
        u[7] += (-az) * ax;            // (3,5): (-2sz)(2sx)
        u[8] += az * (-ay);            // (4,5): (2sz)(-2sy)
        u[9] += 1.0;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kCountSlices && b0 + (int)threadIdx.x < nb)
    p.block_count[b0 + threadIdx.x] = ((wcnt[threadIdx.x][0] + wcnt[threadIdx.x][1]) + wcnt[threadIdx.x][2]) + wcnt[threadIdx.x][3];
  if (!(want_source | want_target)) return;                    // uniform
  __shared__ double red[kBlock / 64][20];
#pragma unroll
  for (int i = 0; i < 20; i++) {
    double t = v[i];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
    if (lane == 0) red[wave][i] = t;
  }
  __syncthreads();
  if (threadIdx.x < 20) p.partial[(size_t)blockIdx.x * 32 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// Exclusive scan of a pair's per-block match counts (a few thousand blocks at most) and, with want_info, the fixed-order total of the information
// partial vectors k_count_blocks left (info[0..19] of the pair are OVERWRITTEN; info[20], the fitness sum of k_ransac_match, is left alone): one workgroup per pair.
__global__ __launch_bounds__(1024) void k_scan_blocks(const PairDev* __restrict__ P, int* __restrict__ totals, double* __restrict__ info, int want_info) {
  __shared__ int buf[1024];
  __shared__ int carry;
  const PairDev& p = P[blockIdx.x];
  const int nb = p.nb;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + (int)threadIdx.x;
    const int v = i < nb ? p.block_count[i] : 0;
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int t = threadIdx.x >= (unsigned)off ? buf[threadIdx.x - off] : 0;
      __syncthreads();
      buf[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nb) p.block_offset[i] = carry + buf[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += buf[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
  if (want_info) {                                              // (uniform) 32 values x 32 strided slices of the partial vectors, then the slices in order
    __shared__ double fin[32][33];
    const int val = threadIdx.x & 31, slice = threadIdx.x >> 5;
    const int nparts = (nb + kCountSlices - 1) / kCountSlices;
    double q = 0.0;
    if (val < 20)
      for (int b = slice; b < nparts; b += 32) q += p.partial[(size_t)b * 32 + val];
    fin[slice][val] = q;
    __syncthreads();
    if (threadIdx.x < 20) {
      double r = 0.0;
#pragma unroll
      for (int sl = 0; sl < 32; sl++) r += fin[sl][threadIdx.x];
      info[(size_t)blockIdx.x * kAcc + threadIdx.x] = r;
    }
  }
}

// Stable compaction: pairs (match[k], k) in ascending k (CorresApp.cpp:157, file order of corres_*.txt).  p.pairs may be the caller's own buffer --
// device memory or page-locked host memory (er_find_correspondence_batch) -- in which case the list is complete where it is wanted when the kernel ends.
// (Staging the block's matches in LDS and storing them as aligned 16-byte bursts changed nothing for a host destination: profiles/r06l_fc_modes.txt.)
__global__ __launch_bounds__(kBlock) void k_compact(const PairDev* __restrict__ P) {
  const PairDev& p = P[blockIdx.y];
  const int n = p.n;
  if ((int)blockIdx.x >= p.nb) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = k < n ? p.match[k] : -1;
  const unsigned long long b = __ballot(m >= 0);
  __shared__ int wcnt[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wcnt[wave] = __popcll(b);
  __syncthreads();
  if (m >= 0) {
    int o = p.block_offset[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) o += wcnt[w];
    reinterpret_cast<int2*>(p.pairs)[o] = make_int2(m, k);       // (o < n: every match has its own k; the buffer is 8-byte aligned)
  }
}

// ---- group workspaces ----------------------------------------------------------------------------
// Everything a GROUP of pairs needs while it is being processed (clouds are immutable and shared): one compute stream and one
// copy stream, the per-pair descriptors and ICP states (device + pinned host mirrors), small per-pair result arrays, and slabs of
// per-source-point scratch cut into one slice per pair.  Groups live in a per-device pool: an API call borrows one (calls from
// several host threads -- the reference's "#pragma omp parallel for" -- borrow one each and overlap on the GPU) and returns it.
// The pool is never freed behind the HIP runtime's back (er_icp_release_workspaces does it).
// The memory of a group.  A fresh GroupMem assigned over it frees all of it, at that point (group_destroy: before the streams go).
struct GroupMem {
  // per pair, device and pinned host mirrors: they grow together (group_reserve), d_pairs first, so its capacity is the group's
  Buffer<PairDev> d_pairs;
  Buffer<IcpDev> d_state;
  Buffer<int> d_active, d_counts, d_totals;
  Buffer<double> d_info, d_fit;                    // kAcc per pair; 2 per pair
  PinnedBuffer<PairDev> h_pairs;
  PinnedBuffer<IcpDev> h_state;
  PinnedBuffer<int> h_active, h_counts, h_totals;
  PinnedBuffer<double> h_info, h_fit;
  // slabs of per-source-point scratch: [3 points], [points], [2 points], [blocks], [blocks], [64 parts]; they regrow together too
  Buffer<float> X;
  Buffer<int> match, pairs, block_count, block_offset;
  Buffer<double> partial;
  PinnedBuffer<int> stage;      // pair lists on their way to pageable caller memory (lazy)
};

struct Group : GroupMem {
  int device = 0;
  hipStream_t stream = nullptr, copy_stream = nullptr, copy_stream2 = nullptr;   // copy streams: list copies alternate between them
  hipEvent_t ev = nullptr, ev2 = nullptr;
  std::vector<hipEvent_t> sub_ev, sub_ev2;  // per sub-group of er_find_correspondence_batch (grown on demand): done / scanned
  int cap_pairs() const { return (int)d_pairs.capacity(); }
  size_t cap_points() const { return match.capacity(); }
  size_t cap_blocks() const { return block_count.capacity(); }
  size_t cap_parts() const { return partial.capacity() / 64; }
};

void group_destroy(Group* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  if (g->copy_stream) (void)hipStreamSynchronize(g->copy_stream);
  if (g->copy_stream2) (void)hipStreamSynchronize(g->copy_stream2);
  static_cast<GroupMem&>(*g) = GroupMem();
  if (g->ev) (void)hipEventDestroy(g->ev);
  if (g->ev2) (void)hipEventDestroy(g->ev2);
  for (hipEvent_t e : g->sub_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : g->sub_ev2)
    if (e) (void)hipEventDestroy(e);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  if (g->copy_stream) (void)hipStreamDestroy(g->copy_stream);
  if (g->copy_stream2) (void)hipStreamDestroy(g->copy_stream2);
  delete g;
}

constexpr int kPrecheckWgs = 16384;    // workgroups of one k_count_inliers launch (each strides over its pair's slices; 8192: +3 % time, 32768: the same)
// Slices of 256 points per workgroup of k_icp_iter when `blocks` slices are to be searched in one launch (the 29 cross-lane sums are paid
// once per workgroup, so more slices per workgroup are cheaper as long as the launch still fills the chip).
int icp_pts(long blocks) { return blocks >= 1024 ? kIcpPtsMax : 1; }
int nparts_of(int n, int pts) { return (std::max(n, 1) + kBlock * pts - 1) / (kBlock * pts); }

// Room for `pairs` descriptors and, when per-point scratch is needed, for `points` source points in `blocks` / `parts` blocks.
int group_reserve(Group* g, int pairs, size_t points, size_t blocks, size_t parts) {
  const char* who = "the ICP workspace";
  if (pairs > g->cap_pairs()) {
    ER_HIP_TRY(hipStreamSynchronize(g->stream));
    const size_t c = (size_t)std::max(pairs, 16);
    if (g->d_pairs.reserve(c, who) || g->d_state.reserve(c, who) || g->d_active.reserve(c, who) || g->d_counts.reserve(c, who) ||
        g->d_totals.reserve(c, who) || g->d_info.reserve(c * kAcc, who) || g->d_fit.reserve(c * 2, who) || g->h_pairs.reserve(c, who) ||
        g->h_state.reserve(c, who) || g->h_active.reserve(c, who) || g->h_counts.reserve(c, who) || g->h_totals.reserve(c, who) ||
        g->h_info.reserve(c * kAcc, who) || g->h_fit.reserve(c * 2, who)) {
      g->d_pairs.reset();                            // (capacity 0: the next call starts over)
      return 1;
    }
  }
  if (points > g->cap_points() || blocks > g->cap_blocks() || parts > g->cap_parts()) {
    ER_HIP_TRY(hipStreamSynchronize(g->stream));
    if (g->copy_stream) ER_HIP_TRY(hipStreamSynchronize(g->copy_stream));
    if (g->copy_stream2) ER_HIP_TRY(hipStreamSynchronize(g->copy_stream2));
    const size_t cp = std::max(points + points / 8, g->cap_points()), cb = std::max(blocks + blocks / 8, g->cap_blocks()),
                 cq = std::max(parts + parts / 8, g->cap_parts());
    auto drop = [g] {
      g->X.reset(), g->match.reset(), g->pairs.reset(), g->block_count.reset(), g->block_offset.reset(), g->partial.reset();
    };
    drop();                                          // all six go before the first comes back
    if (g->X.reserve(cp * 3, who) || g->match.reserve(cp, who) || g->pairs.reserve(cp * 2, who) || g->block_count.reserve(cb, who) ||
        g->block_offset.reserve(cb, who) || g->partial.reserve(cq * 64, who)) {   // partial: 32 x 16 bytes per part (k_icp_iter's 128-bit sums)
      drop();
      return 1;
    }
  }
  return 0;
}

struct GroupPool {
  std::mutex mu;
  std::vector<Group*> idle;
};
GroupPool& pool() {
  static GroupPool* p = new GroupPool();      // intentionally leaked: must outlive every static destructor
  return *p;
}

Group* group_acquire(int device) {
  Group* g = nullptr;
  {
    std::lock_guard<std::mutex> lock(pool().mu);
    // the idle workspace with the LARGEST scratch (ties: the one released last).  Until round 6 this took the first one: after a call that had used
    // several workspaces at once (er_registration_batch's shares, eight host threads with a pair each) a single-threaded caller rotated through all
    // of them, and every one sized for a share had to free and re-allocate its slabs for the full list -- 6.4 against 9.1 ms per 50-pair list,
    // alternating, in bench.py's kinfu-like leg (BENCH_r05: 5.5 k pairs/s where the kernels deliver 7.9 k).
    auto& v = pool().idle;
    long best = -1;
    for (size_t i = 0; i < v.size(); i++)
      if (v[i]->device == device && (best < 0 || v[i]->cap_points() >= v[(size_t)best]->cap_points())) best = (long)i;
    if (best >= 0) {
      g = v[(size_t)best];
      v.erase(v.begin() + best);
    }
  }
  if (hipSetDevice(device) != hipSuccess) {
    er::fail("hipSetDevice(%d) failed", device);
    return nullptr;
  }
  if (!g) {
    g = new Group();
    g->device = device;
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&g->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&g->copy_stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev2, hipEventDisableTiming) != hipSuccess) {
      er::fail("ICP workspace allocation failed: %s", hipGetErrorString(hipGetLastError()));
      group_destroy(g);
      return nullptr;
    }
  }
  return g;
}

void group_release(Group* g) {
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  if (g->copy_stream) (void)hipStreamSynchronize(g->copy_stream);
  if (g->copy_stream2) (void)hipStreamSynchronize(g->copy_stream2);
  std::lock_guard<std::mutex> lock(pool().mu);
  pool().idle.push_back(g);
}

struct GroupLease {             // RAII: the group of one API call
  Group* g = nullptr;
  ~GroupLease() {
    if (g) group_release(g);
  }
  int acquire(int device) {
    g = group_acquire(device);
    return g ? 0 : 1;
  }
};

// Pairs per group: bounded by the per-point scratch (32 bytes per source point and pair).  ER_ICP_GROUP overrides (tests use small groups).
static int group_cfg() { const char* e = getenv("ER_ICP_GROUP"); int v = e ? atoi(e) : 64; return v < 1 ? 1 : (v > 1024 ? 1024 : v); }

int batch_prologue(int n, const er_cloud_t* src, const er_cloud_t* tgt, double radius, const char* who, int* device) {
  if (n < 0 || (n > 0 && (!src || !tgt))) return er::fail("%s: bad arguments", who);
  *device = n > 0 && src[0] ? src[0]->device : 0;
  for (int i = 0; i < n; i++) {
    if (check_pair(src[i], tgt[i], radius, who)) return 1;
    if (src[i]->device != *device) return er::fail("%s: all pairs of one batch must live on one device", who);
  }
  return 0;
}

// Power-of-two scales of k_icp_iter's 128-bit fixed-point partial sums: scale_k = 2^(120 - ilogb(T_k)) with T_k a CERTAIN bound of |sum k| -- n_source terms,
// each bounded through  |s| <= M (a matched source point lies within the radius of a target point, i.e. within the target's box + radius),
// |normal component| <= nm (k_chunk_bounds), |d - s| <= r, |e| = |n . (d - s)| <= 3 nm (r + 1e-4 M) (the float32 expression cancels terms of size nm M) --
// so the 128-bit total cannot overflow (|sum| * scale < 2^121) whatever the points are.
void icp_fixed_point_scales(int n_src, const er_cloud_s* t, double* scale, double* inv) {
  double M = 0.0;
  const double r = 1.01 * (double)t->radius_cap;
  for (int a = 0; a < 3; a++)
    M = std::max(M, std::max(std::fabs((double)t->grid.org[a]), std::fabs((double)t->grid.org[a] + (double)(t->grid.dim[a] + 1) * (double)t->grid.cell)) + r);
  const double nm = std::max((double)t->nmax, 1e-30), n = 1.1 * (double)std::max(n_src, 1), e = 3.0 * nm * (r + 1e-4 * M);
  const double rot = 2.0 * nm * M;
  // classes: rot x rot, rot x normal, normal x normal, rot x e, normal x e, squared distance, count
  const double T[7] = {n * rot * rot, n * rot * nm, n * nm * nm, n * rot * e, n * nm * e, n * r * r, n};
  static const int cls[29] = {0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6};
  for (int k = 0; k < 32; k++) {
    double sc = 0.0;
    if (k < 29) {
      const double b = T[cls[k]];
      sc = (std::isfinite(b) && b > 0.0) ? std::ldexp(1.0, 120 - std::ilogb(b)) : 0.0;
    }
    scale[k] = sc;
    inv[k] = sc > 0.0 ? 1.0 / sc : 0.0;
  }
}

// Fills the descriptors of pairs [i0, i0 + m) of the caller's lists into slots 0..m-1 and cuts the scratch slabs (scratch = false:
// the pre-check needs none).  T16: one row-major float64 4x4 per pair, or NULL.
int group_describe(Group* g, int i0, int m, const er_cloud_t* src, const er_cloud_t* tgt, const double* T16, bool scratch, int* const* pairs_direct = nullptr) {
  size_t points = 0, blocks = 0, parts = 0;
  // (the per-workgroup partial sums of k_icp_iter: room for one slice of 256 points per workgroup, the finest split icp_pts below can pick)
  const int pts = 1;
  for (int q = 0; q < m; q++) {
    const int n = src[i0 + q]->n;
    points += (size_t)((n + 3) & ~3);                          // slices stay 16-byte aligned
    blocks += (size_t)nblocks_of(n);
    parts += (size_t)nparts_of(n, pts);
  }
  if (group_reserve(g, m, scratch ? points : 0, scratch ? blocks : 0, scratch ? parts : 0)) return 1;
  size_t op = 0, ob = 0, oq = 0;
  for (int q = 0; q < m; q++) {
    const er_cloud_s* s = src[i0 + q];
    const er_cloud_s* t = tgt[i0 + q];
    PairDev& P = g->h_pairs[q];
    memset(&P, 0, sizeof P);
    P.src_sorted = s->sorted; P.src_xyz = s->xyz; P.src_nrm = s->nrm;
    P.tgt_xyz = t->xyz; P.tgt_nrm = t->nrm; P.tgt_xn = t->xn;
    P.g = t->grid;
    if (T16)
      for (int c = 0; c < 12; c++) P.T.m[c] = T16[(size_t)(i0 + q) * 16 + c];
    P.n = s->n; P.nb = nblocks_of(s->n); P.nbi = nparts_of(s->n, pts); P.pts = pts;
    icp_fixed_point_scales(s->n, t, P.fx_scale, P.fx_inv);
    if (scratch) {
      P.X = g->X + 3 * op; P.match = g->match + op; P.pairs = g->pairs + 2 * op;
      P.block_count = g->block_count + ob; P.block_offset = g->block_offset + ob;
      P.partial = g->partial + 64 * oq;
      if (pairs_direct && pairs_direct[i0 + q]) P.pairs = pairs_direct[i0 + q];   // k_compact writes the list where the caller wants it (see er_find_correspondence_batch)
      op += (size_t)((s->n + 3) & ~3); ob += (size_t)P.nb; oq += (size_t)P.nbi;
    }
  }
  ER_HIP_TRY(hipMemcpyAsync(g->d_pairs, g->h_pairs, (size_t)m * sizeof(PairDev), hipMemcpyHostToDevice, g->stream));
  return 0;
}

int max_points(int i0, int m, const er_cloud_t* src) {
  int mx = 0;
  for (int q = 0; q < m; q++) mx = std::max(mx, src[i0 + q]->n);
  return mx;
}

// Lists are written in place by k_compact when the GPU can address the destination: device memory (no device-to-device copy) and page-locked host
// memory (no hipMemcpyAsync).  For a host destination that is 2.1-2.5 ms per 50-pair list whatever the state of the process: the copies it replaces
// took 1.6-1.9 ms when their two streams ran on separate SDMA engines and 4.3-4.7 ms when they shared one -- the runtime's choice, whole processes
// long (profiles/r06h_realistic_probe.txt, r06l_fc_modes.txt).
// Set by er_registration_batch's share workers: several shares are in flight, each on a thread and workspace of its own, so a share's list copies run
// behind the other shares' kernels -- and six shares' PCIe-bound compaction kernels at once are slower than their copies (fused list 6.05 against 4.28 ms,
// profiles/r06q_fused_modes.txt).  A single caller has nothing to hide a copy behind: its lists are written in place.
static thread_local bool tl_lists_by_copy = false;

// When lists ARE copied (pageable or too small destinations), the copies of one call are dealt to the group's two copy streams (four streams:
// 2.5-3.0 ms whatever the engines do, two: 1.6 or 4.4 ms; profiles/r06j_fc_modes.txt).

// Where a caller's list buffer lives: 0 = pageable host memory (staged through the group's page-locked block), 1 = page-locked host memory (the copy
// goes straight there), 2 = DEVICE memory of `device` (round 5: the list stays in HBM -- a device-to-device copy of exactly the list, no PCIe; what a
// consumer on the same GPU wants, er_fopt_set_correspondences_dev), -1 = device memory of another GPU (refused).
int buffer_kind(const void* p, int device, void** device_view = nullptr) {
  hipPointerAttribute_t at;
  if (device_view) *device_view = nullptr;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();                                 // plain malloc memory: "invalid value", not an error for us
    return 0;
  }
  if (at.type == hipMemoryTypeHost) {
    if (device_view) *device_view = at.devicePointer;       // page-locked host memory is mapped into the device's address space
    return 1;
  }
  if (at.type == hipMemoryTypeDevice) {
    if (device_view && at.device == device) *device_view = const_cast<void*>(p);
    return at.device == device ? 2 : -1;
  }
  return 0;
}
bool is_pinned_host(const void* p) { return buffer_kind(p, -1) == 1; }

// sum A^T A with A = [I | B], B = [[0, 2sz, -2sy], [-2sz, 0, 2sx], [2sy, -2sx, 0]]  (CorresApp.cpp:198-203,
// RansacCurvature.h:717-721) from its ten distinct terms (k_count_blocks).
void expand_information(const double* acc, double* I) {
  memset(I, 0, 36 * sizeof(double));
  const double N = acc[9];
  I[0 * 6 + 0] = I[1 * 6 + 1] = I[2 * 6 + 2] = N;
  I[0 * 6 + 4] = I[4 * 6 + 0] = acc[2];      //  sum 2sz
  I[0 * 6 + 5] = I[5 * 6 + 0] = -acc[1];     // -sum 2sy
  I[1 * 6 + 3] = I[3 * 6 + 1] = -acc[2];
  I[1 * 6 + 5] = I[5 * 6 + 1] = acc[0];      //  sum 2sx
  I[2 * 6 + 3] = I[3 * 6 + 2] = acc[1];
  I[2 * 6 + 4] = I[4 * 6 + 2] = -acc[0];
  I[3 * 6 + 3] = acc[3];
  I[4 * 6 + 4] = acc[4];
  I[5 * 6 + 5] = acc[5];
  I[3 * 6 + 4] = I[4 * 6 + 3] = acc[6];
  I[3 * 6 + 5] = I[5 * 6 + 3] = acc[7];
  I[4 * 6 + 5] = I[5 * 6 + 4] = acc[8];
}

// Iterations enqueued per host visit (the first visit; later ones twice as many).  PCL's loop runs 3 iterations on most fragment pairs of the
// pipeline (the third one meets the stop rule) and 4 on a few: one chunk usually ends the job; workgroups of a chunk that come after a pair's
// stop decision return at once.
constexpr int kIcpChunk = 4;

}  // namespace

// er::StreamLease (er_cloud.h): a group of the pool above, of which the borrower sees the compute stream only.
int er::StreamLease::acquire(int device) {
  Group* g = group_acquire(device);
  if (!g) return 1;
  group_ = g;
  stream = g->stream;
  return 0;
}
er::StreamLease::~StreamLease() {
  if (group_) group_release(static_cast<Group*>(group_));
}

extern "C" {

int er_icp_release_workspaces(void) {
  std::vector<Group*> v;
  {
    std::lock_guard<std::mutex> lock(pool().mu);
    v.swap(pool().idle);
  }
  for (Group* g : v) group_destroy(g);
  return 0;
}

// Registration pre-check of a pair list (CorresApp.cpp:249-264): one launch per group of pairs.
int er_icp_count_inliers_batch(int n, const er_cloud_t* src, const er_cloud_t* tgt, const double* T, double max_dist, int* counts) {
  int device;
  if (n > 0 && (!T || !counts)) return er::fail("er_icp_count_inliers_batch: NULL argument");
  if (batch_prologue(n, src, tgt, max_dist, "er_icp_count_inliers", &device)) return 1;
  if (n == 0) return 0;
  GroupLease L;
  if (L.acquire(device)) return 1;
  Group* g = L.g;
  const int G = group_cfg();
  for (int i0 = 0; i0 < n; i0 += G) {
    const int m = std::min(G, n - i0);
    if (group_describe(g, i0, m, src, tgt, T, false)) return 1;
    ER_HIP_TRY(hipMemsetAsync(g->d_counts, 0, (size_t)m * sizeof(int), g->stream));
    const int mx = max_points(i0, m, src);
    if (mx > 0) {
      // a few thousand workgroups in flight fill the chip; each strides over its pair's points (one atomic per workgroup)
      const int bx = std::max(1, std::min(nblocks_of(mx), std::max(64, kPrecheckWgs / m)));
      hipLaunchKernelGGL(k_count_inliers, dim3(bx, m), dim3(kBlock), 0, g->stream, g->d_pairs, (float)max_dist, max_dist * max_dist, g->d_counts);
      ER_HIP_TRY(hipGetLastError());
    }
    ER_HIP_TRY(hipMemcpyAsync(g->h_counts, g->d_counts, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, g->stream));
    ER_HIP_TRY(hipStreamSynchronize(g->stream));
    for (int q = 0; q < m; q++) counts[i0 + q] = (src[i0 + q]->n > 0 && tgt[i0 + q]->n > 0) ? g->h_counts[q] : 0;
  }
  return 0;
}

int er_icp_count_inliers(er_cloud_t src, er_cloud_t tgt, const double T[16], double max_dist, int* count) {
  if (!T || !count) return er::fail("er_icp_count_inliers: NULL argument");
  return er_icp_count_inliers_batch(1, &src, &tgt, T, max_dist, count);
}

// icp.align of a pair list (CorresApp.cpp:295-306).  Per group: the states go up once; chunks of kIcpChunk iterations are
// enqueued for the pairs that are still running -- two launches per iteration for the whole group -- and the states come back
// once per chunk; the host only compacts the list of running pairs.
int er_icp_align_batch(int n, const er_cloud_t* src, const er_cloud_t* tgt, const float* guess, double max_dist, int max_iter,
                       double transformation_epsilon, int stop_rule, float* out, int* iterations, int* converged, double* fitness) {
  int device;
  if (n > 0 && (!guess || !out)) return er::fail("er_icp_align: NULL argument");
  if (batch_prologue(n, src, tgt, max_dist, "er_icp_align", &device)) return 1;
  if (n == 0) return 0;
  GroupLease L;
  if (L.acquire(device)) return 1;
  Group* g = L.g;
  const IcpParams prm{transformation_epsilon, max_iter, stop_rule};
  const int G = group_cfg();
  for (int i0 = 0; i0 < n; i0 += G) {
    const int m = std::min(G, n - i0);
    if (group_describe(g, i0, m, src, tgt, nullptr, true)) return 1;
    int n_active = 0;
    for (int q = 0; q < m; q++) {
      IcpDev& st = g->h_state[q];
      memset(&st, 0, sizeof st);
      const float* gq = guess + (size_t)(i0 + q) * 16;
      memcpy(st.fin, gq, sizeof st.fin);                         // final_transformation_ = guess
      bool ident = true;
      for (int i = 0; i < 16; i++) {
        st.delta[i] = st.prev_delta[i] = (i % 5 == 0) ? 1.f : 0.f;
        ident = ident && gq[i] == ((i % 5 == 0) ? 1.f : 0.f);
      }
      st.prev_mse = DBL_MAX;
      st.init_apply = ident ? 0 : 1;
      if (src[i0 + q]->n == 0 || tgt[i0 + q]->n == 0) {
        st.done = 1;                                             // fewer than 3 correspondences by construction: not converged, the guess comes back
      } else {                                                   // (max_iter <= 0 still runs ONE iteration, like PCL's do { } while loop)
        g->h_active[n_active++] = q;
      }
    }
    ER_HIP_TRY(hipMemcpyAsync(g->d_state, g->h_state, (size_t)m * sizeof(IcpDev), hipMemcpyHostToDevice, g->stream));
    int chunk_no = 0;
    while (n_active > 0) {
      // the first chunk ends the job for most pairs; the stragglers then run twice as many iterations per host visit.  A launch pair whose pairs
      // are all done costs ~12 us (every workgroup leaves at once), a host visit ~60 us plus the ramp of the next launch: chunks err on the long side
      // (round 5: 4 then 8 iterations instead of 3 then 6 -- the one pair of the bench list that needs a fourth iteration no longer costs a second visit)
      const int chunk_len = chunk_no++ == 0 ? kIcpChunk : 2 * kIcpChunk;
      ER_HIP_TRY(hipMemcpyAsync(g->d_active, g->h_active, (size_t)n_active * sizeof(int), hipMemcpyHostToDevice, g->stream));
      // points per thread of k_icp_iter for THIS chunk: as many slices of 256 points per workgroup as still leave ~4 workgroups per CU in
      // flight -- 8 for a full list, 1 for the two or three stragglers of a hard list on their way to the iteration limit (round 4: the
      // split used to be fixed when the group was described, so three pairs in their 20th iteration ran as 369 workgroups of eight
      // sequential searches each on a chip that holds 2048)
      long act_blocks = 0;
      int mxb = 1;
      for (int a = 0; a < n_active; a++) {
        act_blocks += g->h_pairs[g->h_active[a]].nb;
        mxb = std::max(mxb, g->h_pairs[g->h_active[a]].nb);
      }
      const int pts = icp_pts(act_blocks);
      const int mxp = (mxb + pts - 1) / pts;
      for (int c = 0; c < chunk_len; c++) {
        hipLaunchKernelGGL(k_icp_iter, dim3(mxp, n_active), dim3(kBlock), 0, g->stream, g->d_pairs, g->d_active, g->d_state, (float)max_dist,
                           max_dist * max_dist, pts);
        hipLaunchKernelGGL(k_icp_final, dim3(n_active), dim3(kBlock), 0, g->stream, g->d_pairs, g->d_active, g->d_state, prm, pts, (double*)nullptr);
      }
      ER_HIP_TRY(hipGetLastError());
      ER_HIP_TRY(hipMemcpyAsync(g->h_state, g->d_state, (size_t)m * sizeof(IcpDev), hipMemcpyDeviceToHost, g->stream));
      ER_HIP_TRY(hipStreamSynchronize(g->stream));               // (d_active is free again: the chunk has run)
      int k = 0;
      for (int a = 0; a < n_active; a++)
        if (!g->h_state[g->h_active[a]].done) g->h_active[k++] = g->h_active[a];
      n_active = k;
    }
    if (fitness) {
      ER_HIP_TRY(hipMemsetAsync(g->d_fit, 0, (size_t)m * 2 * sizeof(double), g->stream));
      const int mx = max_points(i0, m, src);
      if (mx > 0) {
        const int bx = std::max(1, std::min(nblocks_of(mx), std::max(64, 8192 / m)));
        hipLaunchKernelGGL(k_fitness, dim3(bx, m), dim3(kBlock), 0, g->stream, g->d_pairs, g->d_state, (float)max_dist, g->d_fit);
        ER_HIP_TRY(hipGetLastError());
      }
      ER_HIP_TRY(hipMemcpyAsync(g->h_fit, g->d_fit, (size_t)m * 2 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
      ER_HIP_TRY(hipStreamSynchronize(g->stream));
    }
    for (int q = 0; q < m; q++) {
      const IcpDev& st = g->h_state[q];
      memcpy(out + (size_t)(i0 + q) * 16, st.fin, 16 * sizeof(float));
      if (iterations) iterations[i0 + q] = st.iter;
      if (converged) converged[i0 + q] = st.conv ? 1 : 0;
      if (fitness) fitness[i0 + q] = g->h_fit[2 * q + 1] > 0 ? g->h_fit[2 * q] / g->h_fit[2 * q + 1] : DBL_MAX;
    }
  }
  return 0;
}

int er_icp_align(er_cloud_t src, er_cloud_t tgt, const float guess[16], double max_dist, int max_iter,
                 double transformation_epsilon, int stop_rule, float out[16], int* iterations, int* converged, double* fitness) {
  if (!guess || !out) return er::fail("er_icp_align: NULL argument");
  return er_icp_align_batch(1, &src, &tgt, guess, max_dist, max_iter, transformation_epsilon, stop_rule, out, iterations, converged, fitness);
}

// Test hook: er_icp_align for ONE pair with one iteration per host visit -- the same k_icp_iter, k_icp_final and dev_icp_decide, `pts` slices per
// workgroup as the caller says -- and after every iteration the totals k_icp_final handed to dev_icp_decide and the state it left (include/er_hip.h).
int er_icp_align_trace(er_cloud_t src, er_cloud_t tgt, const float guess[16], double max_dist, int max_iter, double transformation_epsilon, int stop_rule,
                       int pts, int row_capacity, double* totals, float* fin, float* delta, int* state, double* prev_mse, double* fx_scale, int* n_rows,
                       float out[16], int* iterations, int* converged) {
  int device;
  if (!guess || !out || !n_rows || row_capacity < 0 || (row_capacity > 0 && (!totals || !fin || !delta || !state || !prev_mse)))
    return er::fail("er_icp_align_trace: NULL argument");
  if (pts < 1 || pts > kIcpPtsMax) return er::fail("er_icp_align_trace: pts = %d outside 1..%d", pts, kIcpPtsMax);
  if (batch_prologue(1, &src, &tgt, max_dist, "er_icp_align_trace", &device)) return 1;
  GroupLease L;
  if (L.acquire(device)) return 1;
  Group* g = L.g;
  const IcpParams prm{transformation_epsilon, max_iter, stop_rule};
  if (group_describe(g, 0, 1, &src, &tgt, nullptr, true)) return 1;
  if (fx_scale)
    for (int k = 0; k < 29; k++) fx_scale[k] = g->h_pairs[0].fx_scale[k];
  IcpDev& st = g->h_state[0];
  memset(&st, 0, sizeof st);
  memcpy(st.fin, guess, sizeof st.fin);
  bool ident = true;
  for (int i = 0; i < 16; i++) {
    st.delta[i] = st.prev_delta[i] = (i % 5 == 0) ? 1.f : 0.f;
    ident = ident && guess[i] == ((i % 5 == 0) ? 1.f : 0.f);
  }
  st.prev_mse = DBL_MAX;
  st.init_apply = ident ? 0 : 1;
  if (src->n == 0 || tgt->n == 0) st.done = 1;
  g->h_active[0] = 0;
  ER_HIP_TRY(hipMemcpyAsync(g->d_state, g->h_state, sizeof(IcpDev), hipMemcpyHostToDevice, g->stream));
  ER_HIP_TRY(hipMemcpyAsync(g->d_active, g->h_active, sizeof(int), hipMemcpyHostToDevice, g->stream));
  const int mxp = (g->h_pairs[0].nb + pts - 1) / pts;
  int rows = 0;
  while (!st.done) {
    hipLaunchKernelGGL(k_icp_iter, dim3(mxp, 1), dim3(kBlock), 0, g->stream, g->d_pairs, g->d_active, g->d_state, (float)max_dist, max_dist * max_dist, pts);
    hipLaunchKernelGGL(k_icp_final, dim3(1), dim3(kBlock), 0, g->stream, g->d_pairs, g->d_active, g->d_state, prm, pts, g->d_info);
    ER_HIP_TRY(hipGetLastError());
    ER_HIP_TRY(hipMemcpyAsync(g->h_state, g->d_state, sizeof(IcpDev), hipMemcpyDeviceToHost, g->stream));
    ER_HIP_TRY(hipMemcpyAsync(g->h_info, g->d_info, kAcc * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    ER_HIP_TRY(hipStreamSynchronize(g->stream));
    if (rows < row_capacity) {
      memcpy(totals + (size_t)rows * 29, g->h_info, 29 * sizeof(double));
      memcpy(fin + (size_t)rows * 16, st.fin, 16 * sizeof(float));
      memcpy(delta + (size_t)rows * 16, st.delta, 16 * sizeof(float));
      state[3 * rows] = st.iter;
      state[3 * rows + 1] = st.done;
      state[3 * rows + 2] = st.conv;
      prev_mse[rows] = st.prev_mse;
    }
    rows++;
  }
  *n_rows = rows;
  memcpy(out, st.fin, 16 * sizeof(float));
  if (iterations) *iterations = st.iter;
  if (converged) *converged = st.conv ? 1 : 0;
  return 0;
}

int er_ransac_fitness_batch(er_cloud_t src, er_cloud_t tgt, int n_hyp, const float* M, float corr_dist_threshold, int* inliers,
                            double* fitness) {
  if (n_hyp < 0 || (n_hyp > 0 && (!M || !inliers))) return er::fail("er_ransac_fitness_batch: bad arguments");
  if (check_pair(src, tgt, (double)corr_dist_threshold, "er_ransac_fitness_batch")) return 1;
  if (n_hyp == 0) return 0;
  GroupLease L;
  if (L.acquire(src->device)) return 1;
  Group* w = L.g;
  DevScope tmp;
  float* d_hyp = nullptr;
  int* d_cnt = nullptr;
  double* d_sum = nullptr;
  std::vector<double> sums((size_t)n_hyp, 0.0);
  int rc = 0;
  const size_t nh = (size_t)n_hyp;
  if (tmp.alloc(&d_hyp, nh * 16, "er_ransac_fitness_batch") || tmp.alloc(&d_cnt, nh, "er_ransac_fitness_batch") ||
      tmp.alloc(&d_sum, nh, "er_ransac_fitness_batch")) {
    rc = 1;
  } else if (hipMemcpyAsync(d_hyp, M, nh * 16 * sizeof(float), hipMemcpyHostToDevice, w->stream) != hipSuccess ||
             hipMemsetAsync(d_cnt, 0, nh * sizeof(int), w->stream) != hipSuccess ||
             hipMemsetAsync(d_sum, 0, nh * sizeof(double), w->stream) != hipSuccess) {
    rc = er::fail("er_ransac_fitness_batch: upload failed: %s", hipGetErrorString(hipGetLastError()));
  } else {
    if (src->n > 0 && tgt->n > 0) {
      // few workgroups per hypothesis when there are many hypotheses (the reference's clouds are down-sampled), all of them otherwise
      const int bx = std::max(1, std::min(nblocks_of(src->n), 4096 / std::min(n_hyp, 4096)));
      for (int h0 = 0; h0 < n_hyp && rc == 0; h0 += 32768) {
        const int hn = std::min(32768, n_hyp - h0);
        hipLaunchKernelGGL(k_ransac_fitness, dim3(bx, hn), dim3(kBlock), 0, w->stream, src->sorted, src->n, d_hyp, h0, tgt->grid,
                           corr_dist_threshold, corr_dist_threshold * corr_dist_threshold, d_cnt, d_sum);
        if (hipGetLastError() != hipSuccess) rc = er::fail("er_ransac_fitness_batch: launch failed");
      }
    }
    if (rc == 0 && (hipMemcpyAsync(inliers, d_cnt, nh * sizeof(int), hipMemcpyDeviceToHost, w->stream) != hipSuccess ||
                    hipMemcpyAsync(sums.data(), d_sum, nh * sizeof(double), hipMemcpyDeviceToHost, w->stream) != hipSuccess ||
                    hipStreamSynchronize(w->stream) != hipSuccess))
      rc = er::fail("er_ransac_fitness_batch: %s", hipGetErrorString(hipGetLastError()));
  }
  if (rc == 0 && fitness)
    for (int h = 0; h < n_hyp; h++) fitness[h] = inliers[h] > 0 ? sums[(size_t)h] / (double)inliers[h] : (double)FLT_MAX;   // :697-703
  return rc;
}

// Compaction chain of slots [s0, s0 + m) of the group (match already written): per-block counts (+ information terms), per-pair
// scan, stable compaction; the totals and the information terms come back to the pinned mirrors.  Records `done` on the stream.
static int corr_chain(Group* g, int s0, int m, int mxb, bool want_source, bool want_target, hipEvent_t done, hipStream_t S = nullptr,
                      hipStream_t compact_on = nullptr, hipEvent_t scanned = nullptr) {
  if (!S) S = g->stream;
  hipLaunchKernelGGL(k_count_blocks, dim3((mxb + kCountSlices - 1) / kCountSlices, m), dim3(kBlock), 0, S, g->d_pairs + s0, want_source ? 1 : 0,
                     want_target ? 1 : 0);
  hipLaunchKernelGGL(k_scan_blocks, dim3(m), dim3(1024), 0, S, g->d_pairs + s0, g->d_totals + s0, g->d_info + (size_t)s0 * kAcc,
                     (want_source || want_target) ? 1 : 0);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipMemcpyAsync(g->h_totals + s0, g->d_totals + s0, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, S));
  ER_HIP_TRY(hipMemcpyAsync(g->h_info + (size_t)s0 * kAcc, g->d_info + (size_t)s0 * kAcc, (size_t)m * kAcc * sizeof(double), hipMemcpyDeviceToHost, S));
  hipStream_t C = S;
  if (compact_on && compact_on != S && scanned) {               // the compaction (PCIe-bound when it writes into host memory) leaves the compute stream
    ER_HIP_TRY(hipEventRecord(scanned, S));
    ER_HIP_TRY(hipStreamWaitEvent(compact_on, scanned, 0));
    C = compact_on;
  }
  hipLaunchKernelGGL(k_compact, dim3(mxb, m), dim3(kBlock), 0, C, g->d_pairs + s0);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipEventRecord(done, C));
  return 0;
}

static int stage_reserve(Group* g, size_t ints) {
  if (ints <= g->stage.capacity()) return 0;
  ER_HIP_TRY(hipStreamSynchronize(g->copy_stream));
  ER_HIP_TRY(hipStreamSynchronize(g->copy_stream2));
  return g->stage.reserve(ints, "the ICP workspace");
}

int er_ransac_inliers(er_cloud_t src, er_cloud_t tgt, const float* M16, float corr_dist_threshold, int* pairs_host, int capacity,
                      int* n_inliers, double* fitness, double* info_source36, double* info_target36) {
  if (!M16 || !n_inliers || capacity < 0 || (capacity > 0 && !pairs_host)) return er::fail("er_ransac_inliers: bad arguments");
  if (check_pair(src, tgt, (double)corr_dist_threshold, "er_ransac_inliers")) return 1;
  *n_inliers = 0;
  if (fitness) *fitness = (double)FLT_MAX;
  if (info_source36) memset(info_source36, 0, 36 * sizeof(double));
  if (info_target36) memset(info_target36, 0, 36 * sizeof(double));
  if (src->n == 0 || tgt->n == 0) return 0;
  GroupLease L;
  if (L.acquire(src->device)) return 1;
  Group* g = L.g;
  if (group_describe(g, 0, 1, &src, &tgt, nullptr, true)) return 1;
  const int n = src->n, nb = nblocks_of(n);
  Mat12f M;
  for (int q = 0; q < 12; q++) M.m[q] = M16[q];
  ER_HIP_TRY(hipMemsetAsync(g->d_info, 0, kAcc * sizeof(double), g->stream));
  hipLaunchKernelGGL(k_ransac_match, dim3(nb), dim3(kBlock), 0, g->stream, g->d_pairs, M, corr_dist_threshold, corr_dist_threshold * corr_dist_threshold,
                     g->d_info);
  if (corr_chain(g, 0, 1, nb, info_source36 != nullptr, info_target36 != nullptr, g->ev)) return 1;
  ER_HIP_TRY(hipEventSynchronize(g->ev));
  const int total = g->h_totals[0];
  *n_inliers = total;
  if (info_source36) expand_information(g->h_info, info_source36);
  if (info_target36) expand_information(g->h_info + 10, info_target36);
  if (fitness && total > 0) *fitness = g->h_info[20] / (double)total;                               // :697-703
  const int ncopy = std::min(total, capacity);
  if (ncopy > 0) {
    const int kind = buffer_kind(pairs_host, src->device);
    if (kind < 0) return er::fail("er_ransac_inliers: the list buffer lives on another GPU than the clouds");
    const bool direct = kind >= 1;                              // page-locked host or device memory
    if (!direct && stage_reserve(g, (size_t)ncopy * 2)) return 1;
    ER_HIP_TRY(hipMemcpyAsync(direct ? pairs_host : g->stage, g->h_pairs[0].pairs, (size_t)ncopy * 2 * sizeof(int),
                              kind == 2 ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, g->stream));
    ER_HIP_TRY(hipStreamSynchronize(g->stream));
    if (!direct) memcpy(pairs_host, g->stage, (size_t)ncopy * 2 * sizeof(int));
  }
  return total > capacity ? er::fail("er_ransac_inliers: %d pairs exceed the capacity %d", total, capacity) : 0;
}

// FindCorrespondence of a pair list (CorresApp.cpp:112-210).  A group is described once; its pairs run in SUB-GROUPS of kCorrSub:
// search + compaction chain of sub-group s+1 are enqueued before the host waits for the totals of sub-group s, and the list copies
// of s (exactly total pairs each; PCIe-bound: 8 bytes per correspondence) run underneath on TWO copy streams in turn (one stream
// leaves ~12 us between consecutive copies: 38 instead of 53 GB/s, profiles/r03l_icp_timeline.txt).
constexpr int kCorrSub = 8;
int er_find_correspondence_batch(int n, const er_cloud_t* src, const er_cloud_t* tgt, const double* T, double dist, double normal_cos,
                                 int* const* pairs_host, const int* capacity, int* n_pairs, double* info36) {
  int device;
  if (n > 0 && (!T || !n_pairs || !pairs_host || !capacity)) return er::fail("er_find_correspondence: NULL argument");
  if (batch_prologue(n, src, tgt, dist, "er_find_correspondence", &device)) return 1;
  if (n == 0) return 0;
  size_t stage_need = 0;
  std::vector<char> direct((size_t)n, 0);                      // destination is page-locked: the list is copied straight into it
  // A list whose buffer the GPU can address and that has room for the largest possible list (one pair per source point) can be written THERE by k_compact:
  // no copy at all.  The copies of the other lists are dealt to two copy streams, and both could land on ONE SDMA engine --
  // 83 MB of lists in 4.4 instead of 1.6 ms (20 against 51 GB/s), whole processes long, flipping after unrelated calls created more streams
  // (profiles/r06h_realistic_probe.txt; BENCH_r05's kinfu-like figure sat in the slow mode).
  std::vector<int*> written((size_t)n, nullptr);
  for (int i = 0; i < n; i++) {
    if (capacity[i] > 0 && !pairs_host[i]) return er::fail("er_find_correspondence: NULL pair buffer for pair %d", i);
    if (capacity[i] > 0) {
      void* view = nullptr;
      const int kind = buffer_kind(pairs_host[i], device, &view);              // (asked once per pair, not again at copy time)
      if (kind < 0) return er::fail("er_find_correspondence: the list buffer of pair %d lives on another GPU than its clouds", i);
      direct[(size_t)i] = (char)kind;                                           // 1: page-locked host, 2: device memory -- both are copied to directly
      if (!direct[(size_t)i]) stage_need += (size_t)std::min(capacity[i], src[i]->n) * 2;
      if (kind > 0 && view && capacity[i] >= src[i]->n && ((uintptr_t)view & 7u) == 0 && !(kind == 1 && tl_lists_by_copy)) written[(size_t)i] = static_cast<int*>(view);
    }
  }
  GroupLease L;
  if (L.acquire(device)) return 1;
  Group* g = L.g;
  if (stage_need && stage_reserve(g, stage_need)) return 1;
  std::vector<long> staged((size_t)n, -1);
  size_t stage_used = 0;
  const int G = group_cfg();
  int rc = 0;
  hipStream_t cs[2] = {g->copy_stream, g->copy_stream2};
  for (int i0 = 0; i0 < n; i0 += G) {
    const int m = std::min(G, n - i0);
    for (int q = 0; q < 2; q++) ER_HIP_TRY(hipStreamSynchronize(cs[q]));          // the previous group's lists have left the slabs
    if (group_describe(g, i0, m, src, tgt, T, true, written.data())) return 1;
    ER_HIP_TRY(hipMemsetAsync(g->d_info, 0, (size_t)m * kAcc * sizeof(double), g->stream));
    // sub-groups exist to put the list copies of one behind the kernels of the next (PCIe); when every list of this group stays in HBM there is nothing
    // to hide and the whole group is ONE sub-group: 4 launches instead of 4 per 8 pairs, no partly filled last waves in between
    bool all_dev = true;
    for (int q = 0; q < m; q++) all_dev = all_dev && (capacity[i0 + q] <= 0 || direct[(size_t)(i0 + q)] == 2 || written[(size_t)(i0 + q)]);
    // Sub-groups put list COPIES behind the next kernels.  Lists that k_compact writes into HOST memory cross PCIe with its stores (1.5 ms for the 83 MB of
    // a 50-pair list: the link's rate, scripts/ubench/d2h_paths.hip) while the searches need 0.7 ms of the GPU: the group is cut into kFcSplit parts;
    // searches, counts and scans stay on the compute stream, the compactions go to two side streams behind an event each, so that one part's stores
    // leave while the next part searches.
    bool host_written = false;
    for (int q = 0; q < m; q++) host_written = host_written || (written[(size_t)(i0 + q)] && direct[(size_t)(i0 + q)] == 1);
    constexpr int kFcSplit = 4;
    const bool split = all_dev && host_written && m >= 2 * kFcSplit;
    const int sub = all_dev ? (split ? (m + kFcSplit - 1) / kFcSplit : std::max(m, 1)) : kCorrSub;
    const int nsub = (m + sub - 1) / sub;
    hipStream_t ks[2] = {g->stream, g->stream};
    while (split && (int)g->sub_ev2.size() < nsub) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return er::fail("er_find_correspondence: hipEventCreate failed");
      g->sub_ev2.push_back(e);
    }
    while ((int)g->sub_ev.size() < nsub) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return er::fail("er_find_correspondence: hipEventCreate failed");
      g->sub_ev.push_back(e);
    }
    std::vector<hipEvent_t>& evs = g->sub_ev;
    auto cleanup = [&]() {};
    auto enqueue = [&](int s) -> int {
      const int s0 = s * sub, ms = std::min(sub, m - s0);
      int mxb = 1;
      for (int q = 0; q < ms; q++) mxb = std::max(mxb, g->h_pairs[s0 + q].nb);
      hipLaunchKernelGGL(k_find_corr, dim3(mxb, ms), dim3(kBlock), 0, ks[s & 1], g->d_pairs + s0, (float)dist, dist * dist, normal_cos);
      return corr_chain(g, s0, ms, mxb, info36 != nullptr, false, evs[(size_t)s], ks[s & 1], split ? ((s & 1) ? g->copy_stream2 : g->copy_stream) : nullptr,
                        split ? g->sub_ev2[(size_t)s] : nullptr);
    };
    if (split) {
      for (int s = 0; s < nsub; s++)
        if (enqueue(s)) { cleanup(); return 1; }
    } else if (enqueue(0)) { cleanup(); return 1; }
    for (int s = 0; s < nsub; s++) {
      if (!split && s + 1 < nsub && enqueue(s + 1)) { cleanup(); return 1; }
      const int s0 = s * sub, ms = std::min(sub, m - s0);
      if (hipEventSynchronize(evs[(size_t)s]) != hipSuccess) { cleanup(); return er::fail("er_find_correspondence: %s", hipGetErrorString(hipGetLastError())); }
      for (int q = 0; q < ms; q++) {
        const int i = i0 + s0 + q;
        const bool empty = src[i]->n == 0 || tgt[i]->n == 0;
        n_pairs[i] = empty ? 0 : g->h_totals[s0 + q];
        if (empty) g->h_totals[s0 + q] = 0;
        if (info36) {
          if (empty) memset(info36 + (size_t)i * 36, 0, 36 * sizeof(double));
          else expand_information(g->h_info + (size_t)(s0 + q) * kAcc, info36 + (size_t)i * 36);
        }
        if (n_pairs[i] > capacity[i]) rc = er::fail("er_find_correspondence: %d pairs exceed the capacity %d", n_pairs[i], capacity[i]);
      }
      // copies of this sub-group's lists on the copy stream (its kernels are done: evs[s] has been waited for)
      for (int q = 0; q < 2; q++) ER_HIP_TRY(hipStreamWaitEvent(cs[q], evs[(size_t)s], 0));
      for (int q = 0; q < ms; q++) {
        const int i = i0 + s0 + q, ncopy = std::min(n_pairs[i], capacity[i]);
        if (ncopy <= 0 || written[(size_t)i]) continue;          // (written in place by k_compact)
        int* dst = pairs_host[i];
        if (!direct[(size_t)i]) {
          staged[(size_t)i] = (long)stage_used;
          dst = g->stage + stage_used;
          stage_used += (size_t)ncopy * 2;
        }
        if (hipMemcpyAsync(dst, g->h_pairs[s0 + q].pairs, (size_t)ncopy * 2 * sizeof(int), direct[(size_t)i] == 2 ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           cs[i % 2]) != hipSuccess) {
          cleanup();
          return er::fail("er_find_correspondence: %s", hipGetErrorString(hipGetLastError()));
        }
      }
    }
    cleanup();
  }
  for (int q = 0; q < 2; q++) ER_HIP_TRY(hipStreamSynchronize(cs[q]));
  for (int i = 0; i < n; i++)
    if (staged[(size_t)i] >= 0) memcpy(pairs_host[i], g->stage + staged[(size_t)i], (size_t)std::min(n_pairs[i], capacity[i]) * 2 * sizeof(int));
  return rc;
}

int er_find_correspondence(er_cloud_t src, er_cloud_t tgt, const double T[16], double dist, double normal_cos,
                           int* pairs_host, int capacity, int* n_pairs, double* info36) {
  if (!T || !n_pairs || (capacity > 0 && !pairs_host)) return er::fail("er_find_correspondence: NULL argument");
  int* const bufs[1] = {pairs_host};
  return er_find_correspondence_batch(1, &src, &tgt, T, dist, normal_cos, bufs, &capacity, n_pairs, info36);
}

// CCorresApp::Registration followed by CCorresApp::FindCorrespondence for a whole pair list in ONE call (CorresApp.cpp:212-319, then
// :112-210): per pair the pre-check count, the accept rule of :270 ("cnt >= reg_num_ || ( r1 > reg_ratio_ && r2 > reg_ratio_ )"), for
// the accepted pairs icp.align from the float32 cast of the guess (:295-312) and -- from the float64 cast of its result, as :312 stores
// it -- the correspondence list with the `Reduced too much` rule of :164-173 left to the caller (n_pairs and counts are both returned).
// The pairs are independent, so the list is cut into a few contiguous shares and every share runs the three stages on a host thread
// and a group workspace of its own: the host round trips of one share (accept rule, the states of an ICP chunk, list sizes) and its
// list copies over PCIe overlap the kernels of the others -- what the reference's "#pragma omp parallel for" does for its CPU loops.
// Results are those of the three *_batch calls in sequence (same kernels, same per-pair arithmetic; a share is a shorter list, so the slice count per
// workgroup of k_icp_iter -- and with it the grouping of the float64 sums -- can differ: last bits of a transform, see include/er_hip.h).
int er_registration_batch(int n, const er_cloud_t* src, const er_cloud_t* tgt, const double* T_guess, double reg_dist, int reg_num, double reg_ratio,
                          int max_iter, double transformation_epsilon, int stop_rule, double corr_dist, double normal_cos, int* counts,
                          int* accepted, float* T_final, int* iterations, int* converged, int* const* pairs_host, const int* capacity,
                          int* n_pairs, double* info36) {
  int device;
  if (n > 0 && (!T_guess || !counts || !accepted || !T_final || !pairs_host || !capacity || !n_pairs)) return er::fail("er_registration_batch: NULL argument");
  if (batch_prologue(n, src, tgt, reg_dist, "er_registration_batch", &device)) return 1;
  if (batch_prologue(n, src, tgt, corr_dist, "er_registration_batch", &device)) return 1;
  if (n == 0) return 0;
  const char* e = getenv("ER_ICP_SHARES");
  int shares = e ? atoi(e) : 6;                                              // (measured on the 50-pair list: 2 shares 10.5 k, 4: 10.4 k, 6: 10.9 k pairs/s)
  shares = std::max(1, std::min(shares, std::min(8, (n + 7) / 8)));          // at least ~8 pairs per share: every launch still fills the chip
  std::vector<int> rc((size_t)shares, 0);
  std::vector<std::string> why((size_t)shares);
  auto work = [&](int w) {
    const int lo = (int)((long)n * w / shares), hi = (int)((long)n * (w + 1) / shares), m = hi - lo;
    if (m <= 0) return;
    auto failed = [&]() { rc[(size_t)w] = 1; why[(size_t)w] = er_last_error(); };   // (the message lives in this thread's buffer)
    if (hipSetDevice(device) != hipSuccess) { er::fail("er_registration_batch: hipSetDevice(%d) failed", device); failed(); return; }
    if (er_icp_count_inliers_batch(m, src + lo, tgt + lo, T_guess + (size_t)lo * 16, reg_dist, counts + lo)) { failed(); return; }
    std::vector<int> idx;
    for (int i = lo; i < hi; i++) {
      const double r1 = (double)counts[i] / (double)tgt[i]->n, r2 = (double)counts[i] / (double)src[i]->n;   // :268-269 (0 / 0 = NaN: rejected)
      accepted[i] = (counts[i] >= reg_num || (r1 > reg_ratio && r2 > reg_ratio)) ? 1 : 0;
      n_pairs[i] = 0;
      if (iterations) iterations[i] = 0;
      if (converged) converged[i] = 0;
      for (int q = 0; q < 16; q++) T_final[(size_t)i * 16 + q] = (float)T_guess[(size_t)i * 16 + q];      // a rejected pair keeps its transform (:277-283)
      if (info36) memset(info36 + (size_t)i * 36, 0, 36 * sizeof(double));
      if (accepted[i]) idx.push_back(i);
    }
    const int a = (int)idx.size();
    if (a == 0) return;
    std::vector<er_cloud_t> s2((size_t)a), t2((size_t)a);
    std::vector<float> g2((size_t)a * 16), f2((size_t)a * 16);
    std::vector<double> T2((size_t)a * 16), I2(info36 ? (size_t)a * 36 : 0);
    std::vector<int> it2((size_t)a), cv2((size_t)a), cap2((size_t)a), np2((size_t)a);
    std::vector<int*> buf2((size_t)a);
    for (int k = 0; k < a; k++) {
      const int i = idx[(size_t)k];
      s2[(size_t)k] = src[i];
      t2[(size_t)k] = tgt[i];
      memcpy(&g2[(size_t)k * 16], &T_final[(size_t)i * 16], 16 * sizeof(float));                            // transformation_.cast<float>()
      cap2[(size_t)k] = capacity[i];
      buf2[(size_t)k] = pairs_host[i];
    }
    if (er_icp_align_batch(a, s2.data(), t2.data(), g2.data(), reg_dist, max_iter, transformation_epsilon, stop_rule, f2.data(), it2.data(), cv2.data(), nullptr)) {
      failed();
      return;
    }
    for (size_t q = 0; q < (size_t)a * 16; q++) T2[q] = (double)f2[q];                                        // getFinalTransformation().cast<double>()
    tl_lists_by_copy = shares > 1;
    const int frc = er_find_correspondence_batch(a, s2.data(), t2.data(), T2.data(), corr_dist, normal_cos, buf2.data(), cap2.data(), np2.data(),
                                                 info36 ? I2.data() : nullptr);
    tl_lists_by_copy = false;
    for (int k = 0; k < a; k++) {
      const int i = idx[(size_t)k];
      memcpy(&T_final[(size_t)i * 16], &f2[(size_t)k * 16], 16 * sizeof(float));
      if (iterations) iterations[i] = it2[(size_t)k];
      if (converged) converged[i] = cv2[(size_t)k];
      n_pairs[i] = np2[(size_t)k];
      if (info36) memcpy(info36 + (size_t)i * 36, &I2[(size_t)k * 36], 36 * sizeof(double));
    }
    if (frc) failed();
  };
  if (shares == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (int w = 0; w < shares; w++) th.emplace_back(work, w);
    for (std::thread& t : th) t.join();
  }
  for (int w = 0; w < shares; w++)
    if (rc[(size_t)w]) return er::fail("%s", why[(size_t)w].c_str());
  return 0;
}

}  // extern "C"

// What er_ransac_inliers does for its one pair, for m pairs in one chain: a search per pair (each has its own matrix), then one count / scan / compact
// over all of them and one wait.  Every sum of the chain belongs to one pair, so the matrices are those of m single calls.
int er::StreamLease::ransac_information(int m, const er_cloud_t* src, const er_cloud_t* tgt, const float* M16, float corr_dist_threshold,
                                        double* info_source36, double* info_target36) {
  Group* g = static_cast<Group*>(group_);
  if (m <= 0 || !g) return 0;
  if (group_describe(g, 0, m, src, tgt, nullptr, true)) return 1;
  ER_HIP_TRY(hipMemsetAsync(g->d_info, 0, (size_t)m * kAcc * sizeof(double), g->stream));
  int mxb = 1;
  for (int q = 0; q < m; q++) {
    const int nb = nblocks_of(src[q]->n);
    mxb = std::max(mxb, nb);
    Mat12f M;
    for (int e = 0; e < 12; e++) M.m[e] = M16[(size_t)q * 16 + e];
    hipLaunchKernelGGL(k_ransac_match, dim3(nb), dim3(kBlock), 0, g->stream, g->d_pairs + q, M, corr_dist_threshold,
                       corr_dist_threshold * corr_dist_threshold, g->d_info + (size_t)q * kAcc);
  }
  if (corr_chain(g, 0, m, mxb, info_source36 != nullptr, info_target36 != nullptr, g->ev)) return 1;
  ER_HIP_TRY(hipEventSynchronize(g->ev));
  for (int q = 0; q < m; q++) {
    if (info_source36) expand_information(g->h_info + (size_t)q * kAcc, info_source36 + (size_t)q * 36);
    if (info_target36) expand_information(g->h_info + (size_t)q * kAcc + 10, info_target36 + (size_t)q * 36);
  }
  return 0;
}
