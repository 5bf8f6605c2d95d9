// er_mesh_smooth_math.h -- the per-element arithmetic of Taubin smoothing and of vertex normals from triangles (er_mesh_smooth.hip, DESIGN.md
// 7.21; the definitions stand in include/er_hip.h above er_mesh_smooth), free of HIP types so that the same text compiles for the device and,
// for checking, for the host (tests/hostcheck/mesh_smooth_math_check.cpp).  Every function restates its namesake in
// tests/mesh_smooth_restatement.py.  float64 and int64 throughout, never fused (-ffp-contract=off), every operation rounded on its own.
// er_sc::quantise, er_sc::in_range, er_sc::finish_normal and er_sc::mix64 are er_mesh_simplify_math.h's.
#pragma once

#include "er_mesh_simplify_math.h"

namespace er_sm {

constexpr double kAreaQuant = 4294967296.0;    // 2^32 steps per m^2: |p| < 4096 gives |cross| < 2^27, |k| < 2^59
constexpr int kMaxIterations = 1024;

// lambda or mu: finite and at most 1 in magnitude (NaN fails the comparison)
ER_SC_HD bool factor_ok(float f) { return fabsf(f) <= 1.0f; }

// A vertex position that may stand: every coordinate finite and below 4096 m in magnitude.
ER_SC_HD bool position_ok(float x, float y, float z) { return er_sc::in_range(x) && er_sc::in_range(y) && er_sc::in_range(z); }

// The unordered pair {u, w}, u != w, as min << 32 | max.
ER_SC_HD uint64_t edge_key(int u, int w) {
  const uint32_t lo = (uint32_t)(u < w ? u : w), hi = (uint32_t)(u < w ? w : u);
  return (uint64_t)lo << 32 | (uint64_t)hi;
}

// x' = (float)((double)p + (double)f * (m - (double)p)), m = ((double)S / (double)deg) * 2^-20: S the int64 sum of the neighbours' quantised
// coordinates, deg > 0 their number.
ER_SC_HD float move(float p, long long S, int deg, float f) {
  const double m = ((double)S / (double)deg) * er_sc::kQuantInv;
  const double d = m - (double)p;
  const double step = (double)f * d;
  return (float)((double)p + step);
}

// k_a = llrint(cross_a * 2^32), cross = (b - a) x (c - a) in float64, each product rounded before the subtraction.
ER_SC_HD void area_normal(const float a[3], const float b[3], const float c[3], long long k[3]) {
  double d1[3], d2[3];
  for (int q = 0; q < 3; q++) {
    d1[q] = (double)b[q] - (double)a[q];
    d2[q] = (double)c[q] - (double)a[q];
  }
  for (int q = 0; q < 3; q++) {
    const int r = (q + 1) % 3, s = (q + 2) % 3;
    const double left = d1[r] * d2[s], right = d1[s] * d2[r];
    k[q] = llrint((left - right) * kAreaQuant);
  }
}

}  // namespace er_sm
