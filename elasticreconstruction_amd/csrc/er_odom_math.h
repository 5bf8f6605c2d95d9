// er_odom_math.h -- the per-pixel arithmetic of the depth odometry (er_odom.hip), free of HIP types so that the same
// text compiles for the device and, for checking, for the host (tests/hostcheck/odom_math_check.cpp): the bilateral filter, the pyramid
// step, the vertex and normal maps and the row of one projective match.  Every function restates its namesake in
// tests/odometry_restatement.py: float32, in the operation order written here, never fused (-ffp-contract=off), '/' and sqrtf correctly
// rounded.  Nothing here is PCL's text or is checked against PCL.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ER_HD __host__ __device__ __forceinline__
#else
#define ER_HD inline
#endif

namespace er_od {

constexpr int kBilateralRadius = 6;        // 13 x 13 window
constexpr int kSpaceW = 73;                // dx^2 + dy^2 = 0 .. 72
constexpr int kDepthWMax = 512;            // capacity of the depth-weight table (ER_ODOM_DEPTH_W)
constexpr double kSigmaSpace = 4.5;        // pixels
constexpr double kSigmaDepth = 30.0;       // millimetres
constexpr int kPyrSpan = 90;               // 3 sigma_depth: taps of the pyramid step farther than this from the centre do not count
constexpr int kSums = 27;                  // 21 entries of the upper triangle of J^T J row by row, then J^T r

// The tables, built ONCE on the host: float64 exp rounded to float32.  The depth table ends where its weight times the smallest space weight
// would no longer be a normal float32 ("underflows"): no subnormal number ever enters the filter, on any machine.  Returns the depth table's length.
inline int build_tables(float* space, float* depth_w) {
  for (int i = 0; i < kSpaceW; i++) space[i] = (float)std::exp(-(double)i / (2.0 * kSigmaSpace * kSigmaSpace));
  int n = 0;
  for (; n < kDepthWMax; n++) {
    const float w = (float)std::exp(-(double)n * (double)n / (2.0 * kSigmaDepth * kSigmaDepth));
    if ((double)w * (double)space[kSpaceW - 1] < 1.17549435082228750797e-38) break;
    depth_w[n] = w;
  }
  for (int i = n; i < kDepthWMax; i++) depth_w[i] = 0.f;
  return n;
}

ER_HD bool finite3(float x, float y, float z) { return std::isfinite(x) && std::isfinite(y) && std::isfinite(z); }

// bilateral_pixel: taps outside the image or with depth 0 are skipped, w and w d accumulated in row-major tap order; a centre of 0 stays 0.
ER_HD uint16_t bilateral_pixel(const uint16_t* img, int cols, int rows, int x, int y, const float* space, const float* depth_w, int n_depth_w) {
  const int c = img[(size_t)y * cols + x];
  if (c == 0) return 0;
  float wsum = 0.f, sum = 0.f;
  for (int dy = -kBilateralRadius; dy <= kBilateralRadius; dy++) {
    const int yy = y + dy;
    if (yy < 0 || yy >= rows) continue;
    for (int dx = -kBilateralRadius; dx <= kBilateralRadius; dx++) {
      const int xx = x + dx;
      if (xx < 0 || xx >= cols) continue;
      const int d = img[(size_t)yy * cols + xx];
      const int delta = d > c ? d - c : c - d;
      if (d == 0 || delta >= n_depth_w) continue;
      const float w = space[dx * dx + dy * dy] * depth_w[delta];
      wsum = wsum + w;
      sum = sum + w * (float)d;
    }
  }
  return (uint16_t)rintf(sum / wsum);      // (the centre itself has weight 1: wsum >= 1, and the mean lies between the taps: 1 .. 65535)
}

// pyr_down_pixel: level l + 1 at (x, y) from level l (scols x srows): integer mean of the 5 x 5 taps around (2x, 2y) that lie inside the image
// and within kPyrSpan of the centre; a centre of 0 gives 0.
ER_HD uint16_t pyr_down_pixel(const uint16_t* src, int scols, int srows, int x, int y) {
  const int cx = 2 * x, cy = 2 * y;
  const int c = src[(size_t)cy * scols + cx];
  if (c == 0) return 0;
  int sum = 0, count = 0;
  for (int dy = -2; dy <= 2; dy++) {
    const int yy = cy + dy;
    if (yy < 0 || yy >= srows) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int xx = cx + dx;
      if (xx < 0 || xx >= scols) continue;
      const int d = src[(size_t)yy * scols + xx];
      const int delta = d > c ? d - c : c - d;
      if (delta < kPyrSpan) {
        sum += d;
        count++;
      }
    }
  }
  return (uint16_t)(sum / count);
}

// vertex: back-projection of pixel (u, v) with depth d millimetres; NaN where d is 0.
ER_HD void vertex(int d, int u, int v, float fx, float fy, float cx, float cy, float& X, float& Y, float& Z) {
  if (d == 0) {
    X = Y = Z = NAN;
    return;
  }
  const float z = (float)d / 1000.0f;
  X = (z * ((float)u - cx)) / fx;
  Y = (z * ((float)v - cy)) / fy;
  Z = z;
}

// normal: normalize(cross(v(x+1, y) - v, v(x, y+1) - v)); NaN where one of the three pixels is invalid and on the last row and column.
ER_HD void normal(const uint16_t* depth, int cols, int rows, int x, int y, float fx, float fy, float cx, float cy, float& nx, float& ny, float& nz) {
  nx = ny = nz = NAN;
  if (x + 1 >= cols || y + 1 >= rows) return;
  const int d0 = depth[(size_t)y * cols + x], d1 = depth[(size_t)y * cols + x + 1], d2 = depth[(size_t)(y + 1) * cols + x];
  if (d0 == 0 || d1 == 0 || d2 == 0) return;
  float px, py, pz, qx, qy, qz, rx, ry, rz;
  vertex(d0, x, y, fx, fy, cx, cy, px, py, pz);
  vertex(d1, x + 1, y, fx, fy, cx, cy, qx, qy, qz);
  vertex(d2, x, y + 1, fx, fy, cx, cy, rx, ry, rz);
  const float ax = qx - px, ay = qy - py, az = qz - pz;
  const float bx = rx - px, by = ry - py, bz = rz - pz;
  const float cxx = ay * bz - az * by, cyy = az * bx - ax * bz, czz = ax * by - ay * bx;
  const float len = sqrtf((cxx * cxx + cyy * cyy) + czz * czz);
  nx = cxx / len;
  ny = cyy / len;
  nz = czz / len;
}

struct Intr { float fx, fy, cx, cy; };

// match_row: one pixel of the current frame (v, n) under the float32 pose (R row-major, t) against the model's records
// model[2 i] = {vm, .}, model[2 i + 1] = {nm, .} (F4: any type with x, y, z).  False: the pixel contributes nothing.  True: a[6], b of its row.
// The bounds of the projection are tested in float BEFORE the conversion to int (a NaN or a huge value converted to int is undefined).
template <typename F4>
ER_HD bool match_row(const float* R, const float* t, float vx, float vy, float vz, float nx, float ny, float nz, const F4* model, int cols,
                     int rows, Intr K, float dist_thresh, float angle_thresh, float* a, float& b) {
  if (!finite3(vx, vy, vz) || !finite3(nx, ny, nz)) return false;
  const float gx = ((R[0] * vx + R[1] * vy) + R[2] * vz) + t[0];
  const float gy = ((R[3] * vx + R[4] * vy) + R[5] * vz) + t[1];
  const float gz = ((R[6] * vx + R[7] * vy) + R[8] * vz) + t[2];
  const float hx = (R[0] * nx + R[1] * ny) + R[2] * nz;
  const float hy = (R[3] * nx + R[4] * ny) + R[5] * nz;
  const float hz = (R[6] * nx + R[7] * ny) + R[8] * nz;
  if (!finite3(gx, gy, gz) || !(gz > 0.f)) return false;
  const float pu = rintf((gx * K.fx) / gz + K.cx);
  const float pv = rintf((gy * K.fy) / gz + K.cy);
  if (!(pu >= 0.f && pu <= (float)(cols - 1) && pv >= 0.f && pv <= (float)(rows - 1))) return false;
  const int idx = (int)pv * cols + (int)pu;
  const F4 vm = model[2 * (size_t)idx], nm = model[2 * (size_t)idx + 1];
  if (!finite3(vm.x, vm.y, vm.z) || !finite3(nm.x, nm.y, nm.z)) return false;
  const float dx = vm.x - gx, dy = vm.y - gy, dz = vm.z - gz;
  const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
  if (!(dist <= dist_thresh)) return false;
  const float sx = hy * nm.z - hz * nm.y, sy = hz * nm.x - hx * nm.z, sz = hx * nm.y - hy * nm.x;
  const float sine = sqrtf((sx * sx + sy * sy) + sz * sz);
  if (!(sine < angle_thresh)) return false;
  a[0] = gy * nm.z - gz * nm.y;
  a[1] = gz * nm.x - gx * nm.z;
  a[2] = gx * nm.y - gy * nm.x;
  a[3] = nm.x;
  a[4] = nm.y;
  a[5] = nm.z;
  b = (nm.x * dx + nm.y * dy) + nm.z * dz;
  return true;
}

// The 27 products of a row, each of two float32 values taken in float64: exact.
ER_HD void row_products(const float* a, float b, double* w) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = i; j < 6; j++) w[k++] = (double)a[i] * (double)a[j];
#pragma unroll
  for (int i = 0; i < 6; i++) w[21 + i] = (double)a[i] * (double)b;
}

}  // namespace er_od
