// er_ransac_math.h -- the per-hypothesis arithmetic of the RANSAC pose search (er_ransac.hip), free of HIP types so that the
// same text compiles for the device and, for checking, for the host: the counter-based generator, selectSamples
// (GlobalRegistration/RansacCurvature.h:319-359), the polygon edge test (PolyRejector.h:262-295), the float64 rigid estimate and
// thresholdNormal (RansacCurvature.h:192-202).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define ER_HD __host__ __device__ __forceinline__
#else
#define ER_HD inline
#endif

namespace er_rs {

constexpr int kMaxSamples = 6;
constexpr unsigned kPickDraw = 8;   // draw numbers: 0 .. nr_samples-1 = the samples, 8 .. 8+nr_samples-1 = the pick among the k matches

// The random number of (seed, iteration, draw): the top 32 bits of splitmix64's output function applied to the counter
//   z = (seed << 32) + 16 * iteration + draw          (iteration < 2^28, draw < 16)
// (include/er_hip.h restates it).  No state: any lane can produce any iteration's numbers.
ER_HD unsigned draw(unsigned seed, unsigned iteration, unsigned d) {
  unsigned long long z = ((unsigned long long)seed << 32) + (unsigned long long)iteration * 16ull + (unsigned long long)d;
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (unsigned)(z >> 32);
}

// getRandomIndex (RansacCurvature.h:215-218): floor(m * u) with u = r / 2^32 in [0, 1)
ER_HD int index_of(unsigned r, int m) { return (int)(((unsigned long long)(unsigned)m * (unsigned long long)r) >> 32); }

// selectSamples: NS distinct indices of [0, n), ascending.  Every loop has compile-time bounds so that s[] stays in registers.
template <int NS>
ER_HD void select_samples(unsigned seed, unsigned iteration, int n, int (&s)[NS]) {
#pragma unroll
  for (int i = 0; i < NS; i++) {
    int v = index_of(draw(seed, iteration, (unsigned)i), n - i);
    bool placed = false;
#pragma unroll
    for (int j = 0; j < i; j++) {
      if (!placed) {
        if (v >= s[j]) {
          v++;
        } else {
#pragma unroll
          for (int k = i; k > j; k--) s[k] = s[k - 1];
          s[j] = v;
          placed = true;
        }
      }
    }
    if (!placed) s[i] = v;
  }
}

// computeSquaredDistance (PolyRejector.h:262-270): float32, p2 - p1, (dx*dx + dy*dy) + dz*dz
ER_HD float sqdist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = bx - ax, dy = by - ay, dz = bz - az;
  return (dx * dx + dy * dy) + dz * dz;
}

// thresholdEdgeLength (:280-295).  0 / 0 is NaN and fails the test, as in the reference.
ER_HD bool edge_ok(float dist_src, float dist_tgt, float simsq) {
  const float edge_sim = dist_src < dist_tgt ? dist_src / dist_tgt : dist_tgt / dist_src;
  return edge_sim >= simsq;
}

// One Jacobi rotation of the symmetric 4x4 A in the (P, Q) plane, accumulated into V (columns = eigenvectors).
template <int P, int Q>
ER_HD void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double akp = A[k][P], akq = A[k][Q];
    A[k][P] = c * akp - s * akq;
    A[k][Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double apk = A[P][k], aqk = A[Q][k];
    A[P][k] = c * apk - s * aqk;
    A[Q][k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

// Least-squares rigid transform of ns point pairs (source P -> target Q), float64: Horn's closed form.  The rotation is the
// eigenvector of the largest eigenvalue of the 4x4 matrix N built from the cross-covariance, found by cyclic Jacobi sweeps -- the
// same rotation Kabsch's SVD with its determinant correction gives.  M = row-major 4x4, rounded to float32 once.
ER_HD void rigid_estimate(const double (&P)[kMaxSamples][3], const double (&Q)[kMaxSamples][3], int ns, float* M) {
  double cp[3] = {0.0, 0.0, 0.0}, cq[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < kMaxSamples; i++)
    if (i < ns) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        cp[a] += P[i][a];
        cq[a] += Q[i][a];
      }
    }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    cp[a] /= (double)ns;
    cq[a] /= (double)ns;
  }
  double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int i = 0; i < kMaxSamples; i++)
    if (i < ns) {
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) S[a][b] += (P[i][a] - cp[a]) * (Q[i][b] - cq[b]);
    }
  double A[4][4], V[4][4];
  A[0][0] = S[0][0] + S[1][1] + S[2][2];
  A[1][1] = S[0][0] - S[1][1] - S[2][2];
  A[2][2] = -S[0][0] + S[1][1] - S[2][2];
  A[3][3] = -S[0][0] - S[1][1] + S[2][2];
  A[0][1] = A[1][0] = S[1][2] - S[2][1];
  A[0][2] = A[2][0] = S[2][0] - S[0][2];
  A[0][3] = A[3][0] = S[0][1] - S[1][0];
  A[1][2] = A[2][1] = S[0][1] + S[1][0];
  A[1][3] = A[3][1] = S[2][0] + S[0][2];
  A[2][3] = A[3][2] = S[1][2] + S[2][1];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; sweep++) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
    if (!(off > 1e-40 * dia)) break;            // (also leaves on NaN)
    jacobi_rotate<0, 1>(A, V);
    jacobi_rotate<0, 2>(A, V);
    jacobi_rotate<0, 3>(A, V);
    jacobi_rotate<1, 2>(A, V);
    jacobi_rotate<1, 3>(A, V);
    jacobi_rotate<2, 3>(A, V);
  }
  double best = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
  for (int c = 1; c < 4; c++)
    if (A[c][c] > best) {
      best = A[c][c];
#pragma unroll
      for (int r = 0; r < 4; r++) q[r] = V[r][c];
    }
  const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
  double R[3][3];
  R[0][0] = 1.0 - 2.0 * (y * y + z * z);
  R[0][1] = 2.0 * (x * y - w * z);
  R[0][2] = 2.0 * (x * z + w * y);
  R[1][0] = 2.0 * (x * y + w * z);
  R[1][1] = 1.0 - 2.0 * (x * x + z * z);
  R[1][2] = 2.0 * (y * z - w * x);
  R[2][0] = 2.0 * (x * z - w * y);
  R[2][1] = 2.0 * (y * z + w * x);
  R[2][2] = 1.0 - 2.0 * (x * x + y * y);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    M[4 * r + 0] = (float)R[r][0];
    M[4 * r + 1] = (float)R[r][1];
    M[4 * r + 2] = (float)R[r][2];
    M[4 * r + 3] = (float)(cq[r] - ((R[r][0] * cp[0] + R[r][1] * cp[1]) + R[r][2] * cp[2]));
  }
  M[12] = 0.f;
  M[13] = 0.f;
  M[14] = 0.f;
  M[15] = 1.f;
}

// One term of thresholdNormal: n_t . (R n_s) with the float32 matrix, float32 arithmetic.
ER_HD float normal_dot(const float* M, float sx, float sy, float sz, float tx, float ty, float tz) {
  const float nx = (M[0] * sx + M[1] * sy) + M[2] * sz;
  const float ny = (M[4] * sx + M[5] * sy) + M[6] * sz;
  const float nz = (M[8] * sx + M[9] * sy) + M[10] * sz;
  return (tx * nx + ty * ny) + tz * nz;
}

}  // namespace er_rs
