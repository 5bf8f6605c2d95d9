// er_raycast_math.h -- the per-pixel rule of the ray caster (er_tsdf_raycast.hip), free of HIP types so that the same text
// compiles for the device and, for checking, for the host (tests/hostcheck/raycast_math_check.cpp).  Every function restates its namesake
// in tests/raycast_restatement.py: float32, in the operation order written here, never fused (-ffp-contract=off), '/' and sqrtf correctly
// rounded; only + - * / sqrtf floor rint and comparisons.  The march is KinFu's in outline (step along the ray, a front face is a change of
// sign from >= 0 to < 0, a back face ends the ray, the crossing is refined on interpolated values); nothing here is PCL's text or is checked
// against PCL.
//
// The volume is reached through a type Vol that the caller supplies:
//   bool fetch(int gx, int gy, int gz, float& F)   voxel (gx, gy, gz) of the 0-based lattice (any int: outside 0 .. 32767 is unobserved);
//                                                  true iff the voxel is OBSERVED (its unit exists and its weight is not 0), F = its sdf
//   int  advance(px, py, pz, step)                 after an unobserved nearest-voxel sample at p: how many steps the march may go on, >= 1.
//                                                  More than 1 only over samples that provably are unobserved too (skip_steps below); the
//                                                  plain march answers 1.
#pragma once

#include <cmath>
#include <cstdint>

#if !defined(ER_HD)
#if defined(__HIPCC__)
#define ER_HD __host__ __device__ __forceinline__
#else
#define ER_HD inline
#endif
#endif

namespace er_rc {

constexpr double kUnitLength = 3.0 / 512.0;      // voxel size in metres (er_tsdf_math.h: the same number)
constexpr int kHalf = 256 * 64;                  // voxel index of the origin on the 0-based lattice
constexpr int kLattice = 512 * 64;               // voxels per axis
constexpr int kMaxSteps = 65536;
constexpr int kBrackets = 4;                     // brackets the refinement tries: (t_{k-1}, t_k) and up to three moves of one step

// What the host derives ONCE per image from (cam4, world_T_camera, params) and every pixel reads.
struct Image {
  float fx, fy, cx, cy;
  float R[9], o[3];                              // float32 casts of the pose's rotation (row-major) and translation
  float t_min, step;
  int n_steps;
};

struct Pixel {
  float v[3], n[3];                              // camera frame; NaN where there is none
  uint16_t depth;                                // millimetres; 0 = none
};

ER_HD float quiet_nan() {
#if defined(__HIP_DEVICE_COMPILE__)
  return __int_as_float(0x7fc00000);
#else
  return std::nanf("");
#endif
}

// n_steps = ceil((t_max - t_min) / step) in double.  -> 0 ok, 1 not finite or step <= 0, 2 more than kMaxSteps steps.
inline int count_steps(float t_min, float t_max, float step, int* n_steps) {
  *n_steps = 0;
  if (!std::isfinite(t_min) || !std::isfinite(t_max) || !std::isfinite(step) || !(step > 0.f)) return 1;
  if (t_max <= t_min) return 0;
  const double n = std::ceil(((double)t_max - (double)t_min) / (double)step);
  if (!(n <= (double)kMaxSteps)) return 2;
  *n_steps = (int)n;
  return 0;
}

inline void make_image(const float cam4[4], const double T[16], float t_min, float step, int n_steps, Image& I) {
  I.fx = cam4[0], I.fy = cam4[1], I.cx = cam4[2], I.cy = cam4[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) I.R[3 * r + c] = (float)T[4 * r + c];
    I.o[r] = (float)T[4 * r + 3];
  }
  I.t_min = t_min, I.step = step, I.n_steps = n_steps;
}

// The nearest voxel's index on the 0-based lattice: er_tsdf_extract.hip's nearest_index, with the bounds tested on the double BEFORE it becomes
// an int (a NaN or a far-away coordinate is "off the lattice", never a conversion with an undefined result).
ER_HD bool nearest_index(float p, int& g) {
  const double q = rint((double)p / kUnitLength);
  if (!(q >= -(double)kHalf && q <= (double)(kHalf - 1))) return false;
  g = (int)q + kHalf;
  return true;
}

template <class Vol>
ER_HD bool sample_nearest(Vol& vol, float px, float py, float pz, float& F) {
  int gx, gy, gz;
  if (!(nearest_index(px, gx) & nearest_index(py, gy) & nearest_index(pz, gz))) return false;
  return vol.fetch(gx, gy, gz, F);
}

// floor and fraction of one coordinate in voxels; false off the lattice (the upper corner i + 1 may still be: fetch finds that out).
ER_HD bool cell_index(float p, int& i, float& f) {
  const double q = (double)p / kUnitLength;
  const double fl = floor(q);
  if (!(fl >= -(double)kHalf && fl <= (double)(kHalf - 1))) return false;
  i = (int)fl + kHalf;
  f = (float)(q - fl);
  return true;
}

// Trilinear sdf at p: eight fetches, z innermost, c = F0 + f (F1 - F0), then y, then x.  Valid iff all eight corners are observed.
template <class Vol>
ER_HD bool trilinear(Vol& vol, float px, float py, float pz, float& out) {
  int ix, iy, iz;
  float fx, fy, fz;
  if (!(cell_index(px, ix, fx) & cell_index(py, iy, fy) & cell_index(pz, iz, fz))) return false;
  float F000, F001, F010, F011, F100, F101, F110, F111;
  bool ok = vol.fetch(ix, iy, iz, F000);
  ok = vol.fetch(ix, iy, iz + 1, F001) && ok;
  ok = vol.fetch(ix, iy + 1, iz, F010) && ok;
  ok = vol.fetch(ix, iy + 1, iz + 1, F011) && ok;
  ok = vol.fetch(ix + 1, iy, iz, F100) && ok;
  ok = vol.fetch(ix + 1, iy, iz + 1, F101) && ok;
  ok = vol.fetch(ix + 1, iy + 1, iz, F110) && ok;
  ok = vol.fetch(ix + 1, iy + 1, iz + 1, F111) && ok;
  if (!ok) return false;
  const float c00 = F000 + fz * (F001 - F000);
  const float c01 = F010 + fz * (F011 - F010);
  const float c10 = F100 + fz * (F101 - F100);
  const float c11 = F110 + fz * (F111 - F110);
  const float c0 = c00 + fy * (c01 - c00);
  const float c1 = c10 + fy * (c11 - c10);
  out = c0 + fx * (c1 - c0);
  return true;
}

// The empty-space skip's bound, for a Vol whose nearest-voxel sample at p fell into unit (ux, uy, uz) that does not exist.  Every sample that
// rounds into that unit is unobserved, and p_k moves by at most step * max|dw_a| per step along each axis; so with rays of (nearly) unit
// length the march stays inside the unit's box for the distance d from p to the box's nearest face.  d less one voxel of safety -- two
// orders of magnitude above everything float32 rounding can do to t_k, p_k and d for the rays skip_allowed admits -- divided by step, rounded
// down, is a number of steps whose samples all lie in the box.  The bound is tested as a float before it becomes an int.
ER_HD int skip_steps(float px, float py, float pz, int ux, int uy, int uz, float step) {
  const float ul = (float)kUnitLength;
  const float lx = ((float)(64 * ux - kHalf) - 0.5f) * ul, ly = ((float)(64 * uy - kHalf) - 0.5f) * ul, lz = ((float)(64 * uz - kHalf) - 0.5f) * ul;
  const float w = 64.0f * ul;
  float d = px - lx;
  float e = (lx + w) - px;
  d = e < d ? e : d;
  e = py - ly;
  d = e < d ? e : d;
  e = (ly + w) - py;
  d = e < d ? e : d;
  e = pz - lz;
  d = e < d ? e : d;
  e = (lz + w) - pz;
  d = e < d ? e : d;
  const float r = floorf((d - ul) / step);
  if (!(r >= 1.0f)) return 1;
  return r >= (float)kMaxSteps ? kMaxSteps : (int)r;
}

// Rays the skip may be used on: direction components of at most unit size (the pose's rotation part is one) and an origin and a range small
// enough that float32 places every sample within a small fraction of a voxel.  Any other image is marched plainly.
ER_HD bool skip_allowed(const Image& I, float dwx, float dwy, float dwz) {
  const float lim = 1024.0f, one = 1.0001f;
  const float t_end = I.t_min + (float)I.n_steps * I.step;
  return fabsf(dwx) <= one && fabsf(dwy) <= one && fabsf(dwz) <= one && fabsf(I.o[0]) <= lim && fabsf(I.o[1]) <= lim && fabsf(I.o[2]) <= lim &&
         fabsf(I.t_min) <= lim && fabsf(t_end) <= lim;
}

// One pixel.  The brute-force march is the definition: t_k and p_k are computed from k afresh, so a Vol that advances by more than one step
// over unobserved samples changes no rounding of any other k.
template <class Vol>
ER_HD void cast_pixel(Vol& vol, const Image& I, int u, int v, Pixel& out) {
  const float nan = quiet_nan();
  out.v[0] = out.v[1] = out.v[2] = out.n[0] = out.n[1] = out.n[2] = nan;
  out.depth = 0;
  const float x = ((float)u - I.cx) / I.fx, y = ((float)v - I.cy) / I.fy;
  const float len = sqrtf((x * x + y * y) + 1.0f);
  const float dcx = x / len, dcy = y / len, dcz = 1.0f / len;
  const float dwx = (I.R[0] * dcx + I.R[1] * dcy) + I.R[2] * dcz;
  const float dwy = (I.R[3] * dcx + I.R[4] * dcy) + I.R[5] * dcz;
  const float dwz = (I.R[6] * dcx + I.R[7] * dcy) + I.R[8] * dcz;
  const bool may_skip = skip_allowed(I, dwx, dwy, dwz);
  bool prev_obs = false, hit = false;
  float Fp = 0.f, Fc = 0.f;
  int k = 0, advance = 1;
  for (; k < I.n_steps; k += advance) {
    const float t = I.t_min + (float)k * I.step;
    const float px = dwx * t + I.o[0], py = dwy * t + I.o[1], pz = dwz * t + I.o[2];
    const bool obs = sample_nearest(vol, px, py, pz, Fc);
    advance = 1;
    if (obs) {
      if (prev_obs && Fp >= 0.f && Fc < 0.f) {                 // front face between t_{k-1} and t_k
        hit = true;
        break;
      }
      if (prev_obs && Fp < 0.f && Fc >= 0.f) break;            // back face: the ray ends (kinfu's rule)
      prev_obs = true;
      Fp = Fc;
    } else {
      prev_obs = false;
      if (may_skip) advance = vol.advance(px, py, pz, I.step);
    }
  }
  if (!hit) return;
  // Refinement on trilinear values.  The nearest-voxel samples that found the crossing sit up to half a voxel's diagonal off the ray, so the
  // interpolated sdf may change sign a step or two earlier or later than they did: starting from (t_{k-1}, t_k) the bracket is moved one step
  // at a time, towards the surface, until the interpolated pair encloses it (A >= 0 > B) -- at most kBrackets brackets, always interpolation,
  // never extrapolation.  If a value is not valid (a corner unobserved) or no bracket is found, the nearest-voxel pair stands in
  // (Fp >= 0 > Fc: Fc - Fp is not 0).
  int j = k - 1;
  float A = 0.f, B = 0.f;
  {
    const float ta = I.t_min + (float)j * I.step, tb = I.t_min + (float)k * I.step;
    bool vA = trilinear(vol, dwx * ta + I.o[0], dwy * ta + I.o[1], dwz * ta + I.o[2], A);
    bool vB = trilinear(vol, dwx * tb + I.o[0], dwy * tb + I.o[1], dwz * tb + I.o[2], B);
    bool found = false;
    for (int s = 0; s < kBrackets; s++) {
      if (!(vA && vB)) break;
      if (A >= 0.f && B < 0.f) {
        found = true;
        break;
      }
      const bool fwd = B >= 0.f;                               // the surface lies farther along the ray; else nearer
      if (s == kBrackets - 1 || (fwd ? j + 2 >= I.n_steps : j < 1)) break;
      j += fwd ? 1 : -1;
      const float tq = I.t_min + (float)(fwd ? j + 1 : j) * I.step;
      float Cq = 0.f;
      const bool vC = trilinear(vol, dwx * tq + I.o[0], dwy * tq + I.o[1], dwz * tq + I.o[2], Cq);
      if (fwd) {
        A = B, vA = vB, B = Cq, vB = vC;
      } else {
        B = A, vB = vA, A = Cq, vA = vC;
      }
    }
    if (!found) {
      j = k - 1;
      A = Fp;
      B = Fc;
    }
  }
  const float t0 = I.t_min + (float)j * I.step, Ft = A, Ftdt = B;
  const float Ts = t0 - (I.step * Ft) / (Ftdt - Ft);
  out.v[0] = Ts * dcx, out.v[1] = Ts * dcy, out.v[2] = Ts * dcz;
  const float mm = rintf(out.v[2] * 1000.0f);
  out.depth = (mm >= 1.0f && mm <= 65535.0f) ? (uint16_t)mm : (uint16_t)0;
  // normal: central differences of the trilinear sdf one voxel to either side of the hit point, world frame, then R^T
  const float ul = (float)kUnitLength;
  const float hx = dwx * Ts + I.o[0], hy = dwy * Ts + I.o[1], hz = dwz * Ts + I.o[2];
  float a = 0.f, b = 0.f;
  bool ok = trilinear(vol, hx + ul, hy, hz, a);
  ok = trilinear(vol, hx - ul, hy, hz, b) && ok;
  const float gx = a - b;
  ok = trilinear(vol, hx, hy + ul, hz, a) && ok;
  ok = trilinear(vol, hx, hy - ul, hz, b) && ok;
  const float gy = a - b;
  ok = trilinear(vol, hx, hy, hz + ul, a) && ok;
  ok = trilinear(vol, hx, hy, hz - ul, b) && ok;
  const float gz = a - b;
  const float gl = sqrtf((gx * gx + gy * gy) + gz * gz);
  if (ok && gl > 0.f) {
    const float nx = -gx / gl, ny = -gy / gl, nz = -gz / gl;
    out.n[0] = (I.R[0] * nx + I.R[3] * ny) + I.R[6] * nz;
    out.n[1] = (I.R[1] * nx + I.R[4] * ny) + I.R[7] * nz;
    out.n[2] = (I.R[2] * nx + I.R[5] * ny) + I.R[8] * nz;
  }
}

}  // namespace er_rc
