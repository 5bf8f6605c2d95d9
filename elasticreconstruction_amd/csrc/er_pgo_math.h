// er_pgo_math.h -- the per-edge arithmetic of the pose graph optimiser (er_pgo.hip), free of HIP types so that the same
// text compiles for the device and, for checking, for the host (tests/hostcheck/pgo_math_check.cpp).  float64 throughout, never fused
// (-ffp-contract=off).  Every function restates its namesake in tests/posegraph_restatement.py.  The model is g2o's VertexSE3 / EdgeSE3
// and vertigo's switchable edge as GraphOptimizer/OptApp.cpp uses them; the Jacobians are the closed forms of DESIGN.md 7.12, derived
// for this file, not g2o's generated derivative code.
//   pose       row-major 4x4 isometry X = (R, t)
//   minimal    (t, qx, qy, qz), qw = sqrt(1 - |q|^2) >= 0;  update X <- X fromMQT(delta)
//   residual   r = toMQT(Z^-1 Xi^-1 Xj)
// Pointers that a kernel passes may point into LDS: nothing here indexes a local array with a run-time index.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define ER_PGO_HD __host__ __device__ __forceinline__
#else
#define ER_PGO_HD inline
#endif

namespace er_pgo {

constexpr int kEdgeH = 0;       // the edge's 12 x 12 contribution, row-major: rows / columns 0..5 vertex id1, 6..11 vertex id2
constexpr int kEdgeG = 144;     // 12: its right-hand side
constexpr int kEdgeHps = 156;   // 12: H_ps = J^T Omega r (loop edges in switchable mode, else 0)
constexpr int kEdgeHss = 168;   // r^T Omega r + w + lambda
constexpr int kEdgeBs = 169;    // s r^T Omega r - w (1 - s)
constexpr int kEdgeChi2 = 170;  // r^T Omega r with the edge's information as it is used (EM: sqrt(l) Omega), without the switch
constexpr int kEdgeRec = 176;   // doubles per edge record

// Y = X^-1 of an isometry: (R^T, -R^T t)
ER_PGO_HD void inverse(const double* X, double* Y) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) Y[4 * r + c] = X[4 * c + r];
    Y[4 * r + 3] = -((X[r] * X[3] + X[4 + r] * X[7]) + X[8 + r] * X[11]);
  }
  Y[12] = 0.0; Y[13] = 0.0; Y[14] = 0.0; Y[15] = 1.0;
}

// C = A B of two isometries
ER_PGO_HD void product(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) C[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
    C[4 * r + 3] = ((A[4 * r] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3];
  }
  C[12] = 0.0; C[13] = 0.0; C[14] = 0.0; C[15] = 1.0;
}

// unit quaternion (x, y, z, w), w >= 0, of the rotation of E (the branch with the largest divisor), normalised
ER_PGO_HD void quaternion(const double* E, double* q) {
  const double m00 = E[0], m01 = E[1], m02 = E[2], m10 = E[4], m11 = E[5], m12 = E[6], m20 = E[8], m21 = E[9], m22 = E[10];
  const double tr = (m00 + m11) + m22;
  double x, y, z, w;
  if (tr > 0.0) {
    const double s = std::sqrt(tr + 1.0) * 2.0;
    w = 0.25 * s; x = (m21 - m12) / s; y = (m02 - m20) / s; z = (m10 - m01) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = std::sqrt(((1.0 + m00) - m11) - m22) * 2.0;
    w = (m21 - m12) / s; x = 0.25 * s; y = (m01 + m10) / s; z = (m02 + m20) / s;
  } else if (m11 > m22) {
    const double s = std::sqrt(((1.0 + m11) - m00) - m22) * 2.0;
    w = (m02 - m20) / s; x = (m01 + m10) / s; y = 0.25 * s; z = (m12 + m21) / s;
  } else {
    const double s = std::sqrt(((1.0 + m22) - m00) - m11) * 2.0;
    w = (m10 - m01) / s; x = (m02 + m20) / s; y = (m12 + m21) / s; z = 0.25 * s;
  }
  const double n = std::sqrt(((x * x + y * y) + z * z) + w * w);
  const double f = (w < 0.0) ? -1.0 / n : 1.0 / n;
  q[0] = x * f; q[1] = y * f; q[2] = z * f; q[3] = w * f;
}

// toMQT: (t, qx, qy, qz) of an isometry, the vector part negated when w < 0
ER_PGO_HD void to_mqt(const double* E, double* v6, double* w_out) {
  double q[4];
  quaternion(E, q);
  v6[0] = E[3]; v6[1] = E[7]; v6[2] = E[11];
  v6[3] = q[0]; v6[4] = q[1]; v6[5] = q[2];
  *w_out = q[3];
}

// fromMQT: the isometry of (t, qx, qy, qz); |q| > 1 is scaled back to the unit sphere (w = 0)
ER_PGO_HD void from_mqt(const double* v6, double* D) {
  double x = v6[3], y = v6[4], z = v6[5], w;
  const double n2 = (x * x + y * y) + z * z;
  if (n2 < 1.0) {
    w = std::sqrt(1.0 - n2);
  } else {
    const double n = std::sqrt(n2);
    x = x / n; y = y / n; z = z / n; w = 0.0;
  }
  D[0] = 1.0 - 2.0 * (y * y + z * z); D[1] = 2.0 * (x * y - z * w);       D[2] = 2.0 * (x * z + y * w);       D[3] = v6[0];
  D[4] = 2.0 * (x * y + z * w);       D[5] = 1.0 - 2.0 * (x * x + z * z); D[6] = 2.0 * (y * z - x * w);       D[7] = v6[1];
  D[8] = 2.0 * (x * z - y * w);       D[9] = 2.0 * (y * z + x * w);       D[10] = 1.0 - 2.0 * (x * x + y * y); D[11] = v6[2];
  D[12] = 0.0; D[13] = 0.0; D[14] = 0.0; D[15] = 1.0;
}

// r = toMQT(Z^-1 Xi^-1 Xj) alone
ER_PGO_HD void residual(const double* Z, const double* Xi, const double* Xj, double* r) {
  double A[16], T[16], B[16], E[16], w;
  inverse(Z, A);
  inverse(Xi, T);
  product(T, Xj, B);
  product(A, B, E);
  to_mqt(E, r, &w);
}

// r and the Jacobians Ji = dr / d(delta_i), Jj = dr / d(delta_j) (each 6 x 6 row-major, entry k at [k * ld]: a kernel interleaves the
// threads' matrices in LDS) at delta = 0.  With A = Z^-1, B = Xi^-1 Xj, E = A B:
//   dtE/dtj = R_E, dtE/dqj = 0, dqE/dqj = w_E I + [v_E]x;  dtE/dti = -R_A, dtE/dqi = R_A 2 [t_B]x,
//   dqE/dqi = -((w_A I + [v_A]x)(w_B I - [v_B]x) - v_A v_B^T) times the sign that makes q_A q_B the residual's quaternion.
ER_PGO_HD void residual_jacobians(const double* Z, const double* Xi, const double* Xj, double* r, double* Ji, double* Jj, int ld) {
  double A[16], T[16], B[16], E[16], wE;
  inverse(Z, A);
  inverse(Xi, T);
  product(T, Xj, B);
  product(A, B, E);
  to_mqt(E, r, &wE);
  double qa[4], qb[4];
  quaternion(A, qa);
  quaternion(B, qb);
#pragma unroll
  for (int k = 0; k < 36; k++) { Ji[k * ld] = 0.0; Jj[k * ld] = 0.0; }
  // vertex j
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) Jj[(6 * a + b) * ld] = E[4 * a + b];
  const double vx = r[3], vy = r[4], vz = r[5];
  Jj[21 * ld] = wE;  Jj[22 * ld] = -vz; Jj[23 * ld] = vy;
  Jj[27 * ld] = vz;  Jj[28 * ld] = wE;  Jj[29 * ld] = -vx;
  Jj[33 * ld] = -vy; Jj[34 * ld] = vx;  Jj[35 * ld] = wE;
  // vertex i: translation rows
  const double tx = B[3], ty = B[7], tz = B[11];
  const double S[9] = {0.0, -2.0 * tz, 2.0 * ty, 2.0 * tz, 0.0, -2.0 * tx, -2.0 * ty, 2.0 * tx, 0.0};     // 2 [t_B]x
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) {
      Ji[(6 * a + b) * ld] = -A[4 * a + b];
      Ji[(6 * a + 3 + b) * ld] = (A[4 * a] * S[b] + A[4 * a + 1] * S[3 + b]) + A[4 * a + 2] * S[6 + b];
    }
  // vertex i: quaternion rows
  const double ax = qa[0], ay = qa[1], az = qa[2], aw = qa[3], bx = qb[0], by = qb[1], bz = qb[2], bw = qb[3];
  const double P[9] = {aw, -az, ay, az, aw, -ax, -ay, ax, aw};          // w_A I + [v_A]x
  const double Q[9] = {bw, bz, -by, -bz, bw, bx, by, -bx, bw};          // w_B I - [v_B]x
  const double va[3] = {ax, ay, az}, vb[3] = {bx, by, bz};
  // the quaternion of E as the product q_A q_B, against the residual's
  const double px = (aw * bx + bw * ax) + (ay * bz - az * by);
  const double py = (aw * by + bw * ay) + (az * bx - ax * bz);
  const double pz = (aw * bz + bw * az) + (ax * by - ay * bx);
  const double pw = aw * bw - ((ax * bx + ay * by) + az * bz);
  const double sg = (((px * vx + py * vy) + pz * vz) + pw * wE >= 0.0) ? -1.0 : 1.0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++)
      Ji[(6 * (3 + a) + 3 + b) * ld] = sg * (((P[3 * a] * Q[b] + P[3 * a + 1] * Q[3 + b]) + P[3 * a + 2] * Q[6 + b]) - va[a] * vb[b]);
}

// x^T Omega y of 6-vectors, Omega row-major 6 x 6 times `scale`
ER_PGO_HD double quad6(const double* Om, double scale, const double* x, const double* y) {
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double row = 0.0;
#pragma unroll
    for (int b = 0; b < 6; b++) row += (scale * Om[6 * a + b]) * y[b];
    acc += x[a] * row;
  }
  return acc;
}

// The cost of one edge.  Odometry / EM edge (switchable = 0): r^T (scale Omega) r.  Switchable loop edge: s^2 r^T Omega r + w (1 - s)^2.
ER_PGO_HD double edge_cost(double chi2, int switchable, double s, double w) {
  return switchable ? (s * s) * chi2 + w * ((1.0 - s) * (1.0 - s)) : chi2;
}

// The edge's record (kEdgeRec doubles) from r, Ji, Jj (entry k at [k * ld]; scaled by s in place for a switchable edge).
//   H = J^T Om J - Hps Hps^T / Hss,  g = J^T Om (s r) - Hps bs / Hss,  J = s [Ji Jj],  Hps = J^T Om r,  Hss = r^T Om r + w + lambda,
//   bs = s r^T Om r - w (1 - s), Om = scale * Omega.  Without a switch the subtracted terms are absent and Hps = 0, Hss = 1, bs = 0.
ER_PGO_HD void edge_record(const double* Omega, double scale, const double* r, double* Ji, double* Jj, int ld, int switchable, double s, double w,
                           double lambda, double* rec) {
  if (switchable)
    for (int k = 0; k < 36; k++) { Ji[k * ld] = s * Ji[k * ld]; Jj[k * ld] = s * Jj[k * ld]; }
  double Or[6];                                             // Om r
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 6; b++) acc += (scale * Omega[6 * a + b]) * r[b];
    Or[a] = acc;
  }
  double chi2 = 0.0;
#pragma unroll
  for (int a = 0; a < 6; a++) chi2 += r[a] * Or[a];
  const double hss = switchable ? (chi2 + w) + lambda : 1.0;
  const double bs = switchable ? s * chi2 - w * (1.0 - s) : 0.0;
  for (int c = 0; c < 12; c++) {                            // Hps[c] = J[:, c] . (Om r);  g[c] = s Hps[c] - Hps[c] bs / Hss
    const double* J = c < 6 ? Ji + c * ld : Jj + (c - 6) * ld;
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 6; b++) acc += J[6 * b * ld] * Or[b];
    rec[kEdgeHps + c] = switchable ? acc : 0.0;
    rec[kEdgeG + c] = switchable ? s * acc - acc * bs / hss : acc;
  }
  for (int c = 0; c < 12; c++) {                            // column c of H
    const double* Jc = c < 6 ? Ji + c * ld : Jj + (c - 6) * ld;
    double OJ[6];                                           // Om J[:, c]
#pragma unroll
    for (int a = 0; a < 6; a++) {
      double acc = 0.0;
#pragma unroll
      for (int b = 0; b < 6; b++) acc += (scale * Omega[6 * a + b]) * Jc[6 * b * ld];
      OJ[a] = acc;
    }
    const double hc = rec[kEdgeHps + c];
    for (int a = 0; a < 12; a++) {
      const double* Ja = a < 6 ? Ji + a * ld : Jj + (a - 6) * ld;
      double acc = 0.0;
#pragma unroll
      for (int b = 0; b < 6; b++) acc += Ja[6 * b * ld] * OJ[b];
      if (switchable) acc -= rec[kEdgeHps + a] * hc / hss;
      rec[kEdgeH + 12 * a + c] = acc;
    }
  }
  rec[kEdgeHss] = hss;
  rec[kEdgeBs] = bs;
  rec[kEdgeChi2] = chi2;
  for (int k = kEdgeChi2 + 1; k < kEdgeRec; k++) rec[k] = 0.0;
}

// delta_s = (-bs - Hps . dx) / Hss, with dx the 12 entries of the edge's two poses (0 for the fixed one)
ER_PGO_HD double delta_s(const double* rec, const double* dx12, double* hps_dx_out) {
  double acc = 0.0;
  for (int c = 0; c < 12; c++) acc += rec[kEdgeHps + c] * dx12[c];
  *hps_dx_out = acc;
  return (-rec[kEdgeBs] - acc) / rec[kEdgeHss];
}

}  // namespace er_pgo
