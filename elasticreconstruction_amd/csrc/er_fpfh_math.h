// er_fpfh_math.h -- the per-point and per-pair arithmetic of the voxel grid, the normal estimation and the FPFH descriptor
// (er_fpfh.hip), free of HIP types so that the same text compiles for the device and, for checking, for the host:
//   voxel_index      pcl::VoxelGrid's cell coordinate of one axis (GlobalRegistration.cpp:63-68)
//   smallest_eigvec  pcl::NormalEstimation's plane fit: the eigenvector of the smallest eigenvalue of a symmetric 3x3 (:89-92)
//   pair_bins        pcl::computePairFeatures and the three histogram bins of FPFHEstimation (:121-128)
// Everything behind the float32 inputs is float64, so that two implementations agree on a bin except within ~1e-13 of an edge.
#pragma once

#include "er_ransac_math.h"

namespace er_fp {

constexpr int kBins = 11;              // bins per feature; a descriptor is 3 x 11
constexpr int kDim = 33;
constexpr double kPi = 3.14159265358979323846;

// floor(fl32(x * inv)) as an int, inv = fl32(1 / leaf)
ER_HD int voxel_index(float x, float inv) { return (int)floorf(x * inv); }

// The squared distance every radius query compares with fl32(r * r): float32, ((dx*dx) + dy*dy) + dz*dz.
ER_HD float sqdist32(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return ((dx * dx) + dy * dy) + dz * dz;
}

// c = {xx, xy, xz, yy, yz, zz} of a symmetric 3x3: its eigenvalues (ascending) and the unit eigenvector of the smallest one, by cyclic
// Jacobi sweeps (er_ransac_math.h's rotation on a 4x4 whose last row and column stay zero).
ER_HD void smallest_eigvec(const double (&c)[6], double (&v)[3], double (&lam)[3]) {
  double A[4][4], V[4][4];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      A[r][q] = 0.0;
      V[r][q] = r == q ? 1.0 : 0.0;
    }
  A[0][0] = c[0]; A[0][1] = A[1][0] = c[1]; A[0][2] = A[2][0] = c[2];
  A[1][1] = c[3]; A[1][2] = A[2][1] = c[4]; A[2][2] = c[5];
  for (int sweep = 0; sweep < 32; sweep++) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (!(off > 1e-40 * dia)) break;            // (also leaves on NaN)
    er_rs::jacobi_rotate<0, 1>(A, V);
    er_rs::jacobi_rotate<0, 2>(A, V);
    er_rs::jacobi_rotate<1, 2>(A, V);
  }
  // (selects on scalars: an indexed pick among V's columns would put them into scratch memory on the device)
  const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
  const bool p1 = d1 < d0;
  const double m01 = p1 ? d1 : d0, x01 = p1 ? d0 : d1;
  double e[3] = {p1 ? V[0][1] : V[0][0], p1 ? V[1][1] : V[1][0], p1 ? V[2][1] : V[2][0]};
  const bool p2 = d2 < m01;
  const double l0 = p2 ? d2 : m01, rest = p2 ? m01 : d2;
  e[0] = p2 ? V[0][2] : e[0];
  e[1] = p2 ? V[1][2] : e[1];
  e[2] = p2 ? V[2][2] : e[2];
  const double l1 = rest < x01 ? rest : x01, l2 = rest < x01 ? x01 : rest;
  const double nrm = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
  v[0] = e[0] / nrm; v[1] = e[1] / nrm; v[2] = e[2] / nrm;
  lam[0] = l0; lam[1] = l1; lam[2] = l2;
}

ER_HD double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

ER_HD int bin_of(double b) {
  const double f = floor(b);
  return !(f > 0.0) ? 0 : (f > (double)(kBins - 1) ? kBins - 1 : (int)f);      // (a NaN lands in bin 0: the index stays inside the histogram)
}

// computePairFeatures for p1, n1 = the point and p2, n2 = its neighbour, then the bin coordinates
//   b[0] = 11 (f1 + pi) / (2 pi), b[1] = 11 (f2 + 1) / 2, b[2] = 11 (f3 + 1) / 2.
// Returns false for a failed pair: coincident points, a non-finite normal, or d parallel to the normal that spans the frame.
ER_HD bool pair_features(const float* p1, const float* n1f, const float* p2, const float* n2f, double (&b)[3]) {
  double dx = (double)p2[0] - (double)p1[0], dy = (double)p2[1] - (double)p1[1], dz = (double)p2[2] - (double)p1[2];
  const double f4 = sqrt(dot3(dx, dy, dz, dx, dy, dz));
  if (f4 == 0.0) return false;
  double ax = n1f[0], ay = n1f[1], az = n1f[2], bx = n2f[0], by = n2f[1], bz = n2f[2];
  if (!(fabs(ax) <= 1.79e308 && fabs(ay) <= 1.79e308 && fabs(az) <= 1.79e308 && fabs(bx) <= 1.79e308 && fabs(by) <= 1.79e308 &&
        fabs(bz) <= 1.79e308))
    return false;
  const double a1 = dot3(ax, ay, az, dx, dy, dz) / f4, a2 = dot3(bx, by, bz, dx, dy, dz) / f4;
  double f3;
  if (fabs(a1) < fabs(a2)) {                    // PCL: acos(|a1|) > acos(|a2|) -- the frame is built on the other point
    double t;
    t = ax; ax = bx; bx = t;
    t = ay; ay = by; by = t;
    t = az; az = bz; bz = t;
    dx = -dx; dy = -dy; dz = -dz;
    f3 = -a2;
  } else {
    f3 = a1;
  }
  double vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;      // v = d x n1
  const double vn = sqrt(dot3(vx, vy, vz, vx, vy, vz));
  if (vn == 0.0) return false;
  vx /= vn; vy /= vn; vz /= vn;
  const double wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;  // w = n1 x v
  const double f2 = dot3(vx, vy, vz, bx, by, bz);
  const double f1 = atan2(dot3(wx, wy, wz, bx, by, bz), dot3(ax, ay, az, bx, by, bz));
  b[0] = (double)kBins * (f1 + kPi) / (2.0 * kPi);
  b[1] = (double)kBins * (f2 + 1.0) / 2.0;
  b[2] = (double)kBins * (f3 + 1.0) / 2.0;
  return true;
}

ER_HD bool pair_bins(const float* p1, const float* n1, const float* p2, const float* n2, int (&bin)[3]) {
  double b[3];
  if (!pair_features(p1, n1, p2, n2, b)) return false;
  bin[0] = bin_of(b[0]);
  bin[1] = bin_of(b[1]);
  bin[2] = bin_of(b[2]);
  return true;
}

}  // namespace er_fp
