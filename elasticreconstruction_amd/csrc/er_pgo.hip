// er_pgo.hip -- the pose graph optimiser of liber_hip.so on MI355X (gfx950): GraphOptimizer's switchable-constraint and EM modes
// (GraphOptimizer/OptApp.cpp, vertigo's switchable edge over g2o's VertexSE3 / EdgeSE3) as a dense Levenberg-Marquardt loop that stays
// on the device.  What is restated is tests/posegraph_restatement.py; nothing here is checked against g2o, and the LM
// schedule is this project's.  The per-edge arithmetic is er_pgo_math.h.
//   k_pgo_linearize   one edge per thread: residual, Jacobians (staged in LDS, interleaved by thread), the 12 x 12 contribution with the
//                     edge's switch eliminated, into an edge-ordered record
//   k_pgo_assemble    one workgroup per 6 x 6 block of the lower triangle: its records' sub-blocks added in ascending edge order (lists
//                     built at creation); the diagonal blocks do the right-hand side.  No floating-point atomics
//   k_pgo_shift_copy  M = H + lambda I (H is never factored in place: a trial may be rejected)
//   k_pgo_potrf / k_pgo_trsm / k_pgo_syrk   blocked right-looking Cholesky of M, 64-wide blocks, one launch of each per block column;
//                     the trailing update is plain FP64 VALU tiles (4 x 4 per thread)
//   k_pgo_fwd_* / k_pgo_bwd_*   blocked substitution
//   k_pgo_apply_*     the step into a candidate state;  k_pgo_cost + k_pgo_reduce: F of a state, summed in a fixed order
//   k_pgo_decide / k_pgo_commit   rho, lambda, nu, the counters and the accepted state, all in device memory
// Ordering is by launches on one stream; no kernel waits for another.  The matrix is padded to a multiple of 64 with an identity block, so
// every tile of the factorisation is a whole tile.  The host reads one PgoState per trial and does no arithmetic on poses, switches, H or b.
#include "er_cloud.h"
#include "er_pgo_math.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

using namespace er;

namespace {

constexpr int kNB = 64;                    // block size of the factorisation
constexpr int kMaxPoses = 1024;
constexpr int kTrialsPerIteration = 10;

struct PgoState {                          // the one record the host reads per trial
  double lambda, nu, F, F_new, rho, denom;
  double lambda_used, F_before;            // of the last trial, for the trace
  int accepted, status, last_status, trials;
};

// ---- linearisation ----------------------------------------------------------------------------------------------------------------------------
struct EdgeArgs {
  int n_edges, n_odo;
  const double* Z;       // [n_edges][16]
  const double* Om;      // [n_edges][36]
  const double* scale;   // [n_edges]: 1, or sqrt(l) of a loop edge in EM mode
  const int* ids;        // [n_edges][2]
};

__global__ __launch_bounds__(64) void k_pgo_linearize(EdgeArgs A, const double* __restrict__ poses, const double* __restrict__ sw, int switchable,
                                                      double weight, const double* __restrict__ lambda, double* __restrict__ rec) {
  __shared__ double sJ[72 * 64];           // thread t's Ji entry k at [k * 64 + t], Jj at [(36 + k) * 64 + t]
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= A.n_edges) return;              // (no barrier in this kernel)
  const int i = A.ids[2 * e], j = A.ids[2 * e + 1];
  double Z[16], Xi[16], Xj[16], r[6];
#pragma unroll
  for (int k = 0; k < 16; k++) { Z[k] = A.Z[16 * (size_t)e + k]; Xi[k] = poses[16 * i + k]; Xj[k] = poses[16 * j + k]; }
  double* Ji = sJ + threadIdx.x;
  double* Jj = sJ + 36 * 64 + threadIdx.x;
  er_pgo::residual_jacobians(Z, Xi, Xj, r, Ji, Jj, 64);
  const int is_sw = switchable && e >= A.n_odo;
  const double s = is_sw ? sw[e - A.n_odo] : 1.0;
  er_pgo::edge_record(A.Om + 36 * (size_t)e, A.scale[e], r, Ji, Jj, 64, is_sw, s, weight, *lambda, rec + (size_t)er_pgo::kEdgeRec * e);
}

// the cost of every edge at a state (and, if asked for, its r^T Omega r)
__global__ __launch_bounds__(64) void k_pgo_cost(EdgeArgs A, const double* __restrict__ poses, const double* __restrict__ sw, int switchable, double weight,
                                                 double* __restrict__ cost, double* __restrict__ chi2_out) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= A.n_edges) return;
  const int i = A.ids[2 * e], j = A.ids[2 * e + 1];
  double Z[16], Xi[16], Xj[16], r[6];
#pragma unroll
  for (int k = 0; k < 16; k++) { Z[k] = A.Z[16 * (size_t)e + k]; Xi[k] = poses[16 * i + k]; Xj[k] = poses[16 * j + k]; }
  er_pgo::residual(Z, Xi, Xj, r);
  const double chi2 = er_pgo::quad6(A.Om + 36 * (size_t)e, A.scale[e], r, r);
  const int is_sw = switchable && e >= A.n_odo;
  cost[e] = er_pgo::edge_cost(chi2, is_sw, is_sw ? sw[e - A.n_odo] : 1.0, weight);
  if (chi2_out) chi2_out[e] = chi2;
}

// E step of the EM mode: l = w^2 / (w^2 + r^T Omega r) with the edge's own information, scale = sqrt(l)
__global__ __launch_bounds__(64) void k_pgo_estep(EdgeArgs A, const double* __restrict__ poses, double weight, double* __restrict__ l_out, double* __restrict__ scale) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= A.n_edges - A.n_odo) return;
  const int e = A.n_odo + k;
  const int i = A.ids[2 * e], j = A.ids[2 * e + 1];
  double Z[16], Xi[16], Xj[16], r[6];
#pragma unroll
  for (int q = 0; q < 16; q++) { Z[q] = A.Z[16 * (size_t)e + q]; Xi[q] = poses[16 * i + q]; Xj[q] = poses[16 * j + q]; }
  er_pgo::residual(Z, Xi, Xj, r);
  const double chi2 = er_pgo::quad6(A.Om + 36 * (size_t)e, 1.0, r, r);
  const double l = (weight * weight) / (weight * weight + chi2);
  l_out[k] = l;
  scale[e] = std::sqrt(l);
}

// ---- assembly ---------------------------------------------------------------------------------------------------------------------------------
// list L: entries ent[ptr[L] .. ptr[L + 1]) = 4 * edge + 2 * (row half) + (column half), ascending; block (blk[2L], blk[2L + 1]), row >= column.
__global__ __launch_bounds__(64) void k_pgo_assemble(const int* __restrict__ ptr, const int* __restrict__ ent, const int* __restrict__ blk,
                                                     const double* __restrict__ rec, double* __restrict__ H, int ld, double* __restrict__ bvec) {
  const int L = blockIdx.x, t = threadIdx.x;
  const int a = blk[2 * L], b = blk[2 * L + 1];
  const int lo = ptr[L], hi = ptr[L + 1];
  if (t < 36) {
    const int r = t / 6, c = t % 6;
    double acc = 0.0;
    for (int q = lo; q < hi; q++) {
      const int v = ent[q];
      acc += rec[(size_t)er_pgo::kEdgeRec * (v >> 2) + er_pgo::kEdgeH + 12 * (6 * ((v >> 1) & 1) + r) + 6 * (v & 1) + c];
    }
    H[(size_t)(6 * a + r) * ld + 6 * b + c] = acc;
  } else if (t < 42 && a == b) {
    const int r = t - 36;
    double acc = 0.0;
    for (int q = lo; q < hi; q++) {
      const int v = ent[q];
      acc += rec[(size_t)er_pgo::kEdgeRec * (v >> 2) + er_pgo::kEdgeG + 6 * ((v >> 1) & 1) + r];
    }
    bvec[6 * a + r] = acc;
  }
}

// M = H + lambda I on the lower block triangle; the padding's diagonal is 1.  grid (nb, nb), 256 threads.  Also y = -b.
__global__ __launch_bounds__(256) void k_pgo_shift_copy(const double* __restrict__ H, double* __restrict__ M, int ld, int n, const double* __restrict__ lambda,
                                                        const double* __restrict__ bvec, double* __restrict__ y) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const double lam = *lambda;
  const int c = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < kNB; r += 4) {
    const int gr = kNB * bi + r, gc = kNB * bj + c;
    double v = H[(size_t)gr * ld + gc];
    if (gr == gc) v = gr < n ? v + lam : 1.0;
    M[(size_t)gr * ld + gc] = v;
  }
  if (bj == 0 && threadIdx.x < kNB) {
    const int g = kNB * bi + threadIdx.x;
    y[g] = g < n ? -bvec[g] : 0.0;
  }
}

// ---- Cholesky ---------------------------------------------------------------------------------------------------------------------------------
// the diagonal block k, unblocked in LDS; a pivot that is not positive and finite sets st->status and is replaced by 1 (the trial is rejected)
__global__ __launch_bounds__(64) void k_pgo_potrf(double* __restrict__ M, int ld, int k, PgoState* st) {
  __shared__ double T[kNB][kNB + 1];
  const int t = threadIdx.x;
  double* base = M + (size_t)kNB * k * ld + kNB * k;
  for (int r = 0; r < kNB; r++) T[r][t] = base[(size_t)r * ld + t];
  for (int j = 0; j < kNB; j++) {
    __syncthreads();
    double d = T[j][j];
    if (!(d > 0.0) || !(d < INFINITY)) {
      if (t == 0) st->status = 1;
      d = 1.0;
    }
    const double sq = std::sqrt(d);
    __syncthreads();
    if (t == j) T[j][j] = sq;
    if (t > j) T[t][j] = T[t][j] / sq;
    __syncthreads();
    if (t > j) {
      const double l = T[t][j];
      for (int c = j + 1; c <= t; c++) T[t][c] -= l * T[c][j];
    }
  }
  __syncthreads();
  for (int r = 0; r < kNB; r++) base[(size_t)r * ld + t] = T[r][t];
}

// the panel under block k: A_ik <- A_ik L_kk^-T, one workgroup per block row i = k + 1 + blockIdx.x, one row per thread
__global__ __launch_bounds__(64) void k_pgo_trsm(double* __restrict__ M, int ld, int k) {
  __shared__ double Lk[kNB * kNB];         // L_kk row-major (read as a broadcast)
  __shared__ double At[kNB * kNB - kNB];   // A^T: entry (row t, column c) at [c * 64 + t], columns 0 .. 62 (the last never feeds another)
  const int t = threadIdx.x, i = k + 1 + blockIdx.x;
  const double* Ld = M + (size_t)kNB * k * ld + kNB * k;
  double* Ad = M + (size_t)kNB * i * ld + kNB * k;
  for (int r = 0; r < kNB; r++) Lk[r * kNB + t] = Ld[(size_t)r * ld + t];
  __syncthreads();
  double* row = Ad + (size_t)t * ld;
  for (int j = 0; j < kNB; j++) {
    double x = row[j];
    for (int m = 0; m < j; m++) x = fma(-At[m * kNB + t], Lk[j * kNB + m], x);
    x = x / Lk[j * kNB + j];
    if (j < kNB - 1) At[j * kNB + t] = x;
    row[j] = x;
  }
}

// the trailing update: A_ij -= L_ik L_jk^T for k < j <= i.  grid (m, m), m = nb - k - 1; 256 threads, 4 x 4 entries each, K in two halves of 32
__global__ __launch_bounds__(256) void k_pgo_syrk(double* __restrict__ M, int ld, int k) {
  const int bi = k + 1 + blockIdx.y, bj = k + 1 + blockIdx.x;
  if (bj > bi) return;                     // (the whole workgroup)
  __shared__ double Li[32][kNB + 1], Lj[32][kNB + 1];      // transposed: [m][row]
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const double* Pi = M + (size_t)kNB * bi * ld + kNB * k;
  const double* Pj = M + (size_t)kNB * bj * ld + kNB * k;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = 0.0;
  for (int half = 0; half < 2; half++) {
    __syncthreads();
    {
      const int m = threadIdx.x & 31;
      for (int r = threadIdx.x >> 5; r < kNB; r += 8) {
        Li[m][r] = Pi[(size_t)r * ld + 32 * half + m];
        Lj[m][r] = Pj[(size_t)r * ld + 32 * half + m];
      }
    }
    __syncthreads();
    for (int m = 0; m < 32; m++) {
      double u[4], v[4];
#pragma unroll
      for (int a = 0; a < 4; a++) { u[a] = Li[m][4 * ty + a]; v[a] = Lj[m][4 * tx + a]; }
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = fma(u[a], v[b], acc[a][b]);
    }
  }
  double* C = M + (size_t)kNB * bi * ld + kNB * bj;
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) C[(size_t)(4 * ty + a) * ld + 4 * tx + b] -= acc[a][b];
}

// ---- substitution -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pgo_fwd_diag(const double* __restrict__ M, int ld, int k, double* __restrict__ y) {
  __shared__ double sh;
  const int t = threadIdx.x;
  const double* row = M + (size_t)(kNB * k + t) * ld + kNB * k;
  double v = y[kNB * k + t];
  for (int j = 0; j < kNB; j++) {
    if (t == j) { v = v / row[j]; sh = v; }
    __syncthreads();
    if (t > j) v -= row[j] * sh;
    __syncthreads();
  }
  y[kNB * k + t] = v;
}

// y_i -= L_ik y_k, i = k + 1 + blockIdx.x
__global__ __launch_bounds__(64) void k_pgo_fwd_update(const double* __restrict__ M, int ld, int k, double* __restrict__ y) {
  __shared__ double yk[kNB];
  const int t = threadIdx.x, i = k + 1 + blockIdx.x;
  yk[t] = y[kNB * k + t];
  __syncthreads();
  const double* row = M + (size_t)(kNB * i + t) * ld + kNB * k;
  double acc = 0.0;
  for (int c = 0; c < kNB; c++) acc += row[c] * yk[c];
  y[kNB * i + t] -= acc;
}

__global__ __launch_bounds__(64) void k_pgo_bwd_diag(const double* __restrict__ M, int ld, int k, double* __restrict__ y) {
  __shared__ double sh;
  const int t = threadIdx.x;
  const double* base = M + (size_t)kNB * k * ld + kNB * k;
  double v = y[kNB * k + t];
  for (int j = kNB - 1; j >= 0; j--) {
    if (t == j) { v = v / base[(size_t)j * ld + j]; sh = v; }
    __syncthreads();
    if (t < j) v -= base[(size_t)j * ld + t] * sh;
    __syncthreads();
  }
  y[kNB * k + t] = v;
}

// y_i -= L_ki^T x_k, i = blockIdx.x < k
__global__ __launch_bounds__(64) void k_pgo_bwd_update(const double* __restrict__ M, int ld, int k, double* __restrict__ y) {
  __shared__ double xk[kNB];
  const int t = threadIdx.x, i = blockIdx.x;
  xk[t] = y[kNB * k + t];
  __syncthreads();
  const double* base = M + (size_t)kNB * k * ld + kNB * i + t;
  double acc = 0.0;
  for (int r = 0; r < kNB; r++) acc += base[(size_t)r * ld] * xk[r];
  y[kNB * i + t] -= acc;
}

// ---- the step, F, the decision ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pgo_apply_poses(int n_poses, const double* __restrict__ cur, const double* __restrict__ x, double* __restrict__ cand) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n_poses) return;
  double X[16], D[16], Y[16], d[6];
#pragma unroll
  for (int k = 0; k < 16; k++) X[k] = cur[16 * v + k];
  if (v == 0) {
#pragma unroll
    for (int k = 0; k < 16; k++) cand[k] = X[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) d[k] = x[6 * (v - 1) + k];
  er_pgo::from_mqt(d, D);
  er_pgo::product(X, D, Y);
#pragma unroll
  for (int k = 0; k < 16; k++) cand[16 * v + k] = Y[k];
}

// delta_s of every loop edge, the clamped switch, and the edge's part of delta^T (lambda delta - b):
//   lambda ds^2 - bs ds - (Hps . dx) bs / Hss    (the last term is the edge's part of -b_pose . dx that the elimination moved out of b)
__global__ __launch_bounds__(64) void k_pgo_apply_switches(int n_loops, int n_odo, const int* __restrict__ ids, const double* __restrict__ rec,
                                                           const double* __restrict__ x, const double* __restrict__ s_cur, double* __restrict__ s_cand,
                                                           double* __restrict__ ds_out, double* __restrict__ den, const double* __restrict__ lambda) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n_loops) return;
  const int e = n_odo + k, i = ids[2 * e], j = ids[2 * e + 1];
  double dx[12];
#pragma unroll
  for (int q = 0; q < 6; q++) { dx[q] = i > 0 ? x[6 * (i - 1) + q] : 0.0; dx[6 + q] = j > 0 ? x[6 * (j - 1) + q] : 0.0; }
  const double* R = rec + (size_t)er_pgo::kEdgeRec * e;
  double hd;
  const double ds = er_pgo::delta_s(R, dx, &hd);
  const double s = s_cur[k] + ds;
  s_cand[k] = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
  ds_out[k] = ds;
  const double bs = R[er_pgo::kEdgeBs];
  den[k] = ((*lambda * ds) * ds - bs * ds) - hd * bs / R[er_pgo::kEdgeHss];
}

// One workgroup: thread t adds the entries t, t + 256, ... in order, then a fixed tree.  what = 0: st->F = sum cost.
// what = 1: st->F_new = sum cost, st->denom = sum den + sum x (lambda x - b).
__global__ __launch_bounds__(256) void k_pgo_reduce(int what, int n_edges, const double* __restrict__ cost, int n_loops, const double* __restrict__ den, int n,
                                                    const double* __restrict__ x, const double* __restrict__ bvec, const double* __restrict__ lambda, PgoState* st) {
  __shared__ double sa[256], sb[256];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int e = t; e < n_edges; e += 256) a += cost[e];
  if (what == 1) {
    const double lam = *lambda;
    for (int k = t; k < n_loops; k += 256) b += den[k];
    for (int q = t; q < n; q += 256) b += x[q] * (lam * x[q] - bvec[q]);
  }
  sa[t] = a;
  sb[t] = b;
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) { sa[t] += sa[t + w]; sb[t] += sb[t + w]; }
  }
  if (t == 0) {
    if (what == 0) st->F = sa[0];
    else { st->F_new = sa[0]; st->denom = sb[0]; }
  }
}

// lambda_0 = 1e-5 max diag(H), nu = 2
__global__ __launch_bounds__(256) void k_pgo_lambda0(const double* __restrict__ H, int ld, int n, PgoState* st) {
  __shared__ double sm[256];
  const int t = threadIdx.x;
  double m = 0.0;
  for (int q = t; q < n; q += 256) m = fmax(m, H[(size_t)q * ld + q]);
  sm[t] = m;
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) sm[t] = fmax(sm[t], sm[t + w]);
  }
  if (t == 0) { st->lambda = 1e-5 * sm[0]; st->nu = 2.0; }
}

__global__ void k_pgo_decide(PgoState* st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double rho = (st->F - st->F_new) / st->denom;
  const bool ok = st->status == 0 && st->F_new < INFINITY && st->F_new > -INFINITY && rho > 0.0;
  st->rho = rho;
  st->lambda_used = st->lambda;
  st->F_before = st->F;
  if (ok) {
    const double q = 2.0 * rho - 1.0;
    st->lambda *= fmax(1.0 / 3.0, fmin(1.0 - q * q * q, 2.0 / 3.0));
    st->nu = 2.0;
    st->F = st->F_new;
  } else {
    st->lambda *= st->nu;
    st->nu *= 2.0;
  }
  st->accepted = ok ? 1 : 0;
  st->last_status = st->status;
  st->status = 0;
  st->trials += 1;
}

__global__ __launch_bounds__(256) void k_pgo_commit(const PgoState* st, int n_pose_doubles, const double* __restrict__ pc, double* __restrict__ p, int n_loops,
                                                    const double* __restrict__ sc, double* __restrict__ s) {
  if (!st->accepted) return;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q < n_pose_doubles) p[q] = pc[q];
  if (q < n_loops) s[q] = sc[q];
}

}  // namespace

struct er_pgo_s {
  int device = 0, n_poses = 0, n_loops = 0, n_edges = 0, n = 0, np = 0, nb = 0, n_lists = 0;
  hipStream_t stream = nullptr;
  er::DevScope mem;                       // every device array below
  double *Z = nullptr, *Om = nullptr, *scale = nullptr, *poses = nullptr, *poses_c = nullptr, *sw = nullptr, *sw_c = nullptr, *lk = nullptr;
  double *rec = nullptr, *H = nullptr, *M = nullptr, *b = nullptr, *y = nullptr, *cost = nullptr, *chi2 = nullptr, *ds = nullptr, *den = nullptr;
  double* consts = nullptr;                // [0] = 0 (linearisation for lambda_0), [1] = the hooks' lambda
  int *ids = nullptr, *ptr = nullptr, *ent = nullptr, *blk = nullptr;
  PgoState* st = nullptr;
  std::vector<double> init_poses;
  bool profiling = false;                  // er_pgo_set_profiling: HIP events round the stages of every trial
  hipEvent_t ev[6] = {};
  double stage_ms[5] = {};                 // linearise, assemble, factor, solve, apply + evaluate, summed over the trials of the last optimize
};

namespace {


EdgeArgs edge_args(const er_pgo_s* h) { return EdgeArgs{h->n_edges, h->n_poses - 1, h->Z, h->Om, h->scale, h->ids}; }
int blocks64(int n) { return std::max(1, (n + 63) / 64); }

// linearise the current state with *lambda in the switches' H_ss, and assemble H and b
void pgo_mark(er_pgo_s* h, int k) {
  if (h->profiling) (void)hipEventRecord(h->ev[k], h->stream);
}

void pgo_linearize(er_pgo_s* h, int switchable, double weight, const double* lambda) {
  pgo_mark(h, 0);
  k_pgo_linearize<<<blocks64(h->n_edges), 64, 0, h->stream>>>(edge_args(h), h->poses, h->sw, switchable, weight, lambda, h->rec);
  pgo_mark(h, 1);
  k_pgo_assemble<<<h->n_lists, 64, 0, h->stream>>>(h->ptr, h->ent, h->blk, h->rec, h->H, h->np, h->b);
  pgo_mark(h, 2);
}

// factor H + *lambda I, solve for the step, apply it into the candidate state and evaluate F there (st->F_new, st->denom)
void pgo_step(er_pgo_s* h, int switchable, double weight, const double* lambda) {
  const int nb = h->nb, ld = h->np;
  k_pgo_shift_copy<<<dim3(nb, nb), 256, 0, h->stream>>>(h->H, h->M, ld, h->n, lambda, h->b, h->y);
  for (int k = 0; k < nb; k++) {
    k_pgo_potrf<<<1, 64, 0, h->stream>>>(h->M, ld, k, h->st);
    const int m = nb - k - 1;
    if (m > 0) {
      k_pgo_trsm<<<m, 64, 0, h->stream>>>(h->M, ld, k);
      k_pgo_syrk<<<dim3(m, m), 256, 0, h->stream>>>(h->M, ld, k);
    }
  }
  pgo_mark(h, 3);
  for (int k = 0; k < nb; k++) {
    k_pgo_fwd_diag<<<1, 64, 0, h->stream>>>(h->M, ld, k, h->y);
    if (nb - k - 1 > 0) k_pgo_fwd_update<<<nb - k - 1, 64, 0, h->stream>>>(h->M, ld, k, h->y);
  }
  for (int k = nb - 1; k >= 0; k--) {
    k_pgo_bwd_diag<<<1, 64, 0, h->stream>>>(h->M, ld, k, h->y);
    if (k > 0) k_pgo_bwd_update<<<k, 64, 0, h->stream>>>(h->M, ld, k, h->y);
  }
  pgo_mark(h, 4);
  k_pgo_apply_poses<<<blocks64(h->n_poses), 64, 0, h->stream>>>(h->n_poses, h->poses, h->y, h->poses_c);
  const int ks = switchable ? h->n_loops : 0;
  if (ks > 0)
    k_pgo_apply_switches<<<blocks64(ks), 64, 0, h->stream>>>(ks, h->n_poses - 1, h->ids, h->rec, h->y, h->sw, h->sw_c, h->ds, h->den, lambda);
  k_pgo_cost<<<blocks64(h->n_edges), 64, 0, h->stream>>>(edge_args(h), h->poses_c, h->sw_c, switchable, weight, h->cost, nullptr);
  k_pgo_reduce<<<1, 256, 0, h->stream>>>(1, h->n_edges, h->cost, ks, h->den, h->n, h->y, h->b, lambda, h->st);
  pgo_mark(h, 5);
}

// after the trial's stream has been synchronised: add the stage times of this trial
void pgo_collect(er_pgo_s* h) {
  if (!h->profiling) return;
  for (int k = 0; k < 5; k++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]) == hipSuccess) h->stage_ms[k] += ms;
  }
}

// F of the current state into st->F
void pgo_cost_now(er_pgo_s* h, int switchable, double weight) {
  k_pgo_cost<<<blocks64(h->n_edges), 64, 0, h->stream>>>(edge_args(h), h->poses, h->sw, switchable, weight, h->cost, nullptr);
  k_pgo_reduce<<<1, 256, 0, h->stream>>>(0, h->n_edges, h->cost, 0, h->den, 0, h->y, h->b, h->consts, h->st);
}

int pgo_set_scale_one(er_pgo_s* h) {
  std::vector<double> one((size_t)h->n_edges, 1.0);
  ER_HIP_TRY(hipMemcpyAsync(h->scale, one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int pgo_finish(er_pgo_s* h, const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return er::fail("%s: kernel launch failed: %s", who, hipGetErrorString(e));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

bool finite_all(const double* p, int n) {
  for (int k = 0; k < n; k++)
    if (!std::isfinite(p[k])) return false;
  return true;
}

}  // namespace

extern "C" {

int er_pgo_create(int n_poses, int n_loops, const double* odo_T, const double* odo_info, const int* loop_ids, const double* loop_T, const double* loop_info,
                  int device, er_pgo_t* out) {
  const char* who = "er_pgo_create";
  if (!out) return er::fail("%s: out is NULL", who);
  *out = nullptr;
  if (no_device(who)) return 1;
  if (n_poses < 2 || n_poses > kMaxPoses) return er::fail("%s: %d poses (2 .. %d; the odometry log has one entry fewer)", who, n_poses, kMaxPoses);
  if (n_loops < 0 || !odo_T || (n_loops > 0 && (!loop_ids || !loop_T))) return er::fail("%s: NULL argument", who);
  if ((long long)n_loops + n_poses > (1 << 29)) return er::fail("%s: %d loop edges are too many", who, n_loops);
  const int n_odo = n_poses - 1, E = n_odo + n_loops;
  for (int i = 0; i < n_odo; i++) {
    if (!finite_all(odo_T + 16 * (size_t)i, 16)) return er::fail("%s: odometry entry %d: the transform is not finite", who, i);
    if (odo_info && !finite_all(odo_info + 36 * (size_t)i, 36)) return er::fail("%s: odometry entry %d: the information matrix is not finite", who, i);
  }
  for (int k = 0; k < n_loops; k++) {
    const int a = loop_ids[2 * k], b = loop_ids[2 * k + 1];
    if (a < 0 || a >= n_poses || b < 0 || b >= n_poses) return er::fail("%s: loop entry %d: ids (%d, %d) are out of range for %d poses", who, k, a, b, n_poses);
    if (a == b) return er::fail("%s: loop entry %d: id1 == id2 == %d", who, k, a);
    if (!finite_all(loop_T + 16 * (size_t)k, 16)) return er::fail("%s: loop entry %d: the transform is not finite", who, k);
    if (loop_info && !finite_all(loop_info + 36 * (size_t)k, 36)) return er::fail("%s: loop entry %d: the information matrix is not finite", who, k);
  }
  int ndev = 0;
  ER_HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return er::fail("%s: device %d of %d", who, device, ndev);
  ER_HIP_TRY(hipSetDevice(device));

  // host copies: edges (odometry first), identity information where none is given, the chained initial poses
  std::vector<double> Z((size_t)E * 16), Om((size_t)E * 36);
  std::vector<int> ids((size_t)E * 2);
  for (int e = 0; e < E; e++) {
    const double* T = e < n_odo ? odo_T + 16 * (size_t)e : loop_T + 16 * (size_t)(e - n_odo);
    const double* I = e < n_odo ? (odo_info ? odo_info + 36 * (size_t)e : nullptr) : (loop_info ? loop_info + 36 * (size_t)(e - n_odo) : nullptr);
    std::copy(T, T + 16, &Z[16 * (size_t)e]);
    for (int q = 0; q < 36; q++) Om[36 * (size_t)e + q] = I ? I[q] : (q % 7 == 0 ? 1.0 : 0.0);
    ids[2 * e] = e < n_odo ? e : loop_ids[2 * (e - n_odo)];
    ids[2 * e + 1] = e < n_odo ? e + 1 : loop_ids[2 * (e - n_odo) + 1];
  }
  er_pgo_s* h = new er_pgo_s;
  h->device = device;
  h->n_poses = n_poses;
  h->n_loops = n_loops;
  h->n_edges = E;
  h->n = 6 * n_odo;
  h->nb = (h->n + kNB - 1) / kNB;
  h->np = h->nb * kNB;
  h->init_poses.assign((size_t)n_poses * 16, 0.0);
  for (int q = 0; q < 16; q++) h->init_poses[q] = q % 5 == 0 ? 1.0 : 0.0;
  for (int i = 0; i < n_odo; i++) {        // COptApp::Init: X_{i+1} = X_i odo_i (a general 4 x 4 product, as the file's rows are)
    const double *A = &h->init_poses[16 * (size_t)i], *B = odo_T + 16 * (size_t)i;
    double* C = &h->init_poses[16 * (size_t)(i + 1)];
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) C[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
  }
  // the assembly lists: (block row, block column, edge, halves), sorted; an edge meets a block at most once
  struct Item { int a, b, v; };
  std::vector<Item> items;
  items.reserve((size_t)E * 3);
  for (int e = 0; e < E; e++) {
    const int vi = ids[2 * e] - 1, vj = ids[2 * e + 1] - 1;
    if (vi >= 0) items.push_back({vi, vi, 4 * e + 0});
    if (vj >= 0) items.push_back({vj, vj, 4 * e + 3});
    if (vi >= 0 && vj >= 0) {
      if (vi > vj) items.push_back({vi, vj, 4 * e + 1});
      else items.push_back({vj, vi, 4 * e + 2});
    }
  }
  std::sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.a != y.a ? x.a < y.a : (x.b != y.b ? x.b < y.b : x.v < y.v); });
  std::vector<int> ptr, ent(items.size()), blk;
  for (size_t q = 0; q < items.size(); q++) {
    if (q == 0 || items[q].a != items[q - 1].a || items[q].b != items[q - 1].b) {
      ptr.push_back((int)q);
      blk.push_back(items[q].a);
      blk.push_back(items[q].b);
    }
    ent[q] = items[q].v;
  }
  ptr.push_back((int)items.size());
  h->n_lists = (int)ptr.size() - 1;

  int rc = 0;
  const size_t mat = (size_t)h->np * h->np;
  rc = rc || h->mem.alloc(&h->Z, Z.size(), who) || h->mem.alloc(&h->Om, Om.size(), who) || h->mem.alloc(&h->scale, (size_t)E, who) || h->mem.alloc(&h->ids, ids.size(), who);
  rc = rc || h->mem.alloc(&h->poses, (size_t)n_poses * 16, who) || h->mem.alloc(&h->poses_c, (size_t)n_poses * 16, who);
  rc = rc || h->mem.alloc(&h->sw, (size_t)n_loops, who) || h->mem.alloc(&h->sw_c, (size_t)n_loops, who) || h->mem.alloc(&h->lk, (size_t)n_loops, who);
  rc = rc || h->mem.alloc(&h->ds, (size_t)n_loops, who) || h->mem.alloc(&h->den, (size_t)n_loops, who);
  rc = rc || h->mem.alloc(&h->rec, (size_t)E * er_pgo::kEdgeRec, who) || h->mem.alloc(&h->cost, (size_t)E, who) || h->mem.alloc(&h->chi2, (size_t)E, who);
  rc = rc || h->mem.alloc(&h->H, mat, who) || h->mem.alloc(&h->M, mat, who) || h->mem.alloc(&h->b, (size_t)h->np, who) || h->mem.alloc(&h->y, (size_t)h->np, who);
  rc = rc || h->mem.alloc(&h->consts, 2, who) || h->mem.alloc(&h->st, 1, who);
  rc = rc || h->mem.alloc(&h->ptr, ptr.size(), who) || h->mem.alloc(&h->ent, ent.size(), who) || h->mem.alloc(&h->blk, blk.size(), who);
  hipError_t e = hipSuccess;
  if (!rc) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  auto up = [&](void* d, const void* s, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpy(d, s, bytes, hipMemcpyHostToDevice); };
  if (!rc) {
    up(h->Z, Z.data(), Z.size() * sizeof(double));
    up(h->Om, Om.data(), Om.size() * sizeof(double));
    up(h->ids, ids.data(), ids.size() * sizeof(int));
    up(h->ptr, ptr.data(), ptr.size() * sizeof(int));
    up(h->ent, ent.data(), ent.size() * sizeof(int));
    up(h->blk, blk.data(), blk.size() * sizeof(int));
    up(h->poses, h->init_poses.data(), h->init_poses.size() * sizeof(double));
    up(h->poses_c, h->init_poses.data(), h->init_poses.size() * sizeof(double));
    std::vector<double> one((size_t)std::max(E, n_loops), 1.0);
    up(h->scale, one.data(), (size_t)E * sizeof(double));
    up(h->sw, one.data(), (size_t)n_loops * sizeof(double));
    up(h->sw_c, one.data(), (size_t)n_loops * sizeof(double));
    if (e == hipSuccess) e = hipMemset(h->H, 0, mat * sizeof(double));
    if (e == hipSuccess) e = hipMemset(h->M, 0, mat * sizeof(double));
    if (e == hipSuccess) e = hipMemset(h->b, 0, (size_t)h->np * sizeof(double));
    if (e == hipSuccess) e = hipMemset(h->consts, 0, 2 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(h->st, 0, sizeof(PgoState));
    if (e == hipSuccess && n_loops > 0) e = hipMemset(h->lk, 0, (size_t)n_loops * sizeof(double));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);                // the uploads and memsets above, on the default stream
  }
  if (rc || e != hipSuccess) {
    if (!rc) er::fail("%s: %s", who, hipGetErrorString(e));
    er_pgo_destroy(h);
    return 1;
  }
  *out = h;
  return 0;
}

int er_pgo_destroy(er_pgo_t h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  h->mem.free_all();
  delete h;
  return 0;
}

int er_pgo_set_profiling(er_pgo_t h, int on) {
  const char* who = "er_pgo_set_profiling";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (on)
    for (hipEvent_t& e : h->ev)
      if (!e) ER_HIP_TRY(hipEventCreate(&e));
  h->profiling = on != 0;
  return 0;
}

int er_pgo_get_profile(er_pgo_t h, double* stage_ms) {
  if (no_device("er_pgo_get_profile")) return 1;
  if (!h || !stage_ms) return er::fail("er_pgo_get_profile: NULL argument");
  for (int k = 0; k < 5; k++) stage_ms[k] = h->stage_ms[k];
  return 0;
}

int er_pgo_set_state(er_pgo_t h, const double* poses, const double* switches) {
  const char* who = "er_pgo_set_state";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  ER_HIP_TRY(hipSetDevice(h->device));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  if (poses) ER_HIP_TRY(hipMemcpy(h->poses, poses, (size_t)h->n_poses * 16 * sizeof(double), hipMemcpyHostToDevice));
  if (switches && h->n_loops > 0) ER_HIP_TRY(hipMemcpy(h->sw, switches, (size_t)h->n_loops * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int er_pgo_get_state(er_pgo_t h, double* poses, double* switches) {
  const char* who = "er_pgo_get_state";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  ER_HIP_TRY(hipSetDevice(h->device));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  if (poses) ER_HIP_TRY(hipMemcpy(poses, h->poses, (size_t)h->n_poses * 16 * sizeof(double), hipMemcpyDeviceToHost));
  if (switches && h->n_loops > 0) ER_HIP_TRY(hipMemcpy(switches, h->sw, (size_t)h->n_loops * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int er_pgo_linearize(er_pgo_t h, double weight, double lambda, double* H_out, double* b_out, double* chi2_out) {
  const char* who = "er_pgo_linearize";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (pgo_set_scale_one(h)) return 1;
  ER_HIP_TRY(hipMemcpyAsync(h->consts + 1, &lambda, sizeof(double), hipMemcpyHostToDevice, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  pgo_linearize(h, 1, weight, h->consts + 1);
  if (pgo_finish(h, who)) return 1;
  const int n = h->n, ld = h->np;
  if (H_out) {
    std::vector<double> full((size_t)ld * ld);
    ER_HIP_TRY(hipMemcpy(full.data(), h->H, full.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int r = 0; r < n; r++)
      for (int c = 0; c < n; c++) H_out[(size_t)r * n + c] = r >= c ? full[(size_t)r * ld + c] : full[(size_t)c * ld + r];     // the lower triangle (what is factored), mirrored
  }
  if (b_out) ER_HIP_TRY(hipMemcpy(b_out, h->b, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (chi2_out) {
    std::vector<double> rec((size_t)h->n_edges * er_pgo::kEdgeRec);
    ER_HIP_TRY(hipMemcpy(rec.data(), h->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int e = 0; e < h->n_edges; e++) chi2_out[e] = rec[(size_t)e * er_pgo::kEdgeRec + er_pgo::kEdgeChi2];
  }
  return 0;
}

int er_pgo_trial(er_pgo_t h, double weight, double lambda, double* dx_out, double* ds_out, double* F_new_out, int* status_out) {
  const char* who = "er_pgo_trial";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (pgo_set_scale_one(h)) return 1;
  ER_HIP_TRY(hipMemsetAsync(h->st, 0, sizeof(PgoState), h->stream));
  ER_HIP_TRY(hipMemcpyAsync(h->consts + 1, &lambda, sizeof(double), hipMemcpyHostToDevice, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  pgo_linearize(h, 1, weight, h->consts + 1);
  pgo_step(h, 1, weight, h->consts + 1);
  if (pgo_finish(h, who)) return 1;
  PgoState st;
  ER_HIP_TRY(hipMemcpy(&st, h->st, sizeof(st), hipMemcpyDeviceToHost));
  if (dx_out) ER_HIP_TRY(hipMemcpy(dx_out, h->y, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost));
  if (ds_out && h->n_loops > 0) ER_HIP_TRY(hipMemcpy(ds_out, h->ds, (size_t)h->n_loops * sizeof(double), hipMemcpyDeviceToHost));
  if (F_new_out) *F_new_out = st.F_new;
  if (status_out) *status_out = st.status;
  return 0;
}

int er_pgo_optimize(er_pgo_t h, int method, double weight, int max_iteration, double* poses_out, double* switch_or_weight_out, int* iterations, int* trials,
                    double* chi2_trace) {
  const char* who = "er_pgo_optimize";
  if (no_device(who)) return 1;
  if (!h) return er::fail("%s: NULL handle", who);
  if (method != ER_PGO_SWITCHABLE && method != ER_PGO_EM) return er::fail("%s: method %d (ER_PGO_SWITCHABLE or ER_PGO_EM)", who, method);
  if (!(weight > 0.0) || !std::isfinite(weight)) return er::fail("%s: weight %g must be positive and finite", who, weight);
  ER_HIP_TRY(hipSetDevice(h->device));
  const int sw = method == ER_PGO_SWITCHABLE;
  // every run starts from the chained odometry with all switches at 1
  std::vector<double> one((size_t)std::max(h->n_loops, 1), 1.0);
  if (er_pgo_set_state(h, h->init_poses.data(), one.data())) return 1;
  if (pgo_set_scale_one(h)) return 1;
  ER_HIP_TRY(hipMemsetAsync(h->st, 0, sizeof(PgoState), h->stream));
  if (h->n_loops > 0) ER_HIP_TRY(hipMemsetAsync(h->lk, 0, (size_t)h->n_loops * sizeof(double), h->stream));
  int its = 0, total = 0;
  PgoState st{};
  for (double& ms : h->stage_ms) ms = 0.0;
  if (sw && max_iteration > 0) {
    pgo_cost_now(h, 1, weight);
    pgo_linearize(h, 1, weight, h->consts);
    k_pgo_lambda0<<<1, 256, 0, h->stream>>>(h->H, h->np, h->n, h->st);
  }
  for (int it = 0; it < max_iteration; it++) {
    if (!sw) {                             // E step, then one LM iteration with a fresh lambda_0
      if (h->n_loops > 0) k_pgo_estep<<<blocks64(h->n_loops), 64, 0, h->stream>>>(edge_args(h), h->poses, weight, h->lk, h->scale);
      pgo_cost_now(h, 0, weight);
      pgo_linearize(h, 0, weight, h->consts);
      k_pgo_lambda0<<<1, 256, 0, h->stream>>>(h->H, h->np, h->n, h->st);
    }
    bool accepted = false;
    for (int t = 0; t < kTrialsPerIteration && !accepted; t++) {
      const double* lam = &h->st->lambda;
      pgo_linearize(h, sw, weight, lam);
      pgo_step(h, sw, weight, lam);
      k_pgo_decide<<<1, 1, 0, h->stream>>>(h->st);
      k_pgo_commit<<<std::max(1, (std::max(16 * h->n_poses, h->n_loops) + 255) / 256), 256, 0, h->stream>>>(h->st, 16 * h->n_poses, h->poses_c, h->poses,
                                                                                                       sw ? h->n_loops : 0, h->sw_c, h->sw);
      ER_HIP_TRY(hipMemcpyAsync(&st, h->st, sizeof(st), hipMemcpyDeviceToHost, h->stream));
      if (pgo_finish(h, who)) return 1;
      pgo_collect(h);
      if (chi2_trace) {
        double* tr = chi2_trace + 4 * (size_t)total;
        tr[0] = st.lambda_used; tr[1] = st.F_before; tr[2] = st.F_new; tr[3] = (double)st.accepted;
      }
      total++;
      accepted = st.accepted != 0;
    }
    its++;
    if (!accepted && sw) break;
  }
  if (pgo_finish(h, who)) return 1;
  if (er_pgo_get_state(h, poses_out, sw ? switch_or_weight_out : nullptr)) return 1;
  if (!sw && switch_or_weight_out && h->n_loops > 0)
    ER_HIP_TRY(hipMemcpy(switch_or_weight_out, h->lk, (size_t)h->n_loops * sizeof(double), hipMemcpyDeviceToHost));
  if (iterations) *iterations = its;
  if (trials) *trials = total;
  return 0;
}

}  // extern "C"
