// er_mesh_simplify_math.h -- the per-element arithmetic of vertex clustering (er_mesh_simplify.hip; the definitions stand in
// include/er_hip.h above er_mesh_simplify), free of HIP types so that the same text compiles for the device and, for checking, for the host
// (tests/hostcheck/mesh_simplify_math_check.cpp).  Every function restates its namesake in tests/mesh_simplify_restatement.py.  float64 and
// int64 throughout, never fused (-ffp-contract=off), every operation rounded on its own.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ER_SC_HD __host__ __device__ __forceinline__
#else
#define ER_SC_HD inline
#endif

namespace er_sc {

constexpr long long kCellBias = 1ll << 20;     // a cell index lies in [-2^20, 2^20)
constexpr double kQuant = 1048576.0;           // 2^20 steps per metre: |p| < 4096 gives |q| < 2^32, and 2^31 members still fit an int64 sum
constexpr double kQuantInv = 1.0 / 1048576.0;
constexpr float kCoordLimit = 4096.0f;

// A coordinate, or a component of a normal, that takes part: finite and below 4096 in magnitude (NaN fails the comparison).
ER_SC_HD bool in_range(float x) { return fabsf(x) < kCoordLimit; }

// c = floor((double)p / (double)cell), as a double: the caller tests cell_ok before it converts.
ER_SC_HD double cell_of(float p, float cell) { return floor((double)p / (double)cell); }
ER_SC_HD bool cell_ok(double c) { return c >= -(double)kCellBias && c < (double)kCellBias; }

// 0: the vertex is fine.  1: a coordinate is not finite or is >= 4096 m in magnitude.  2: a cell index outside [-2^20, 2^20).
ER_SC_HD int vertex_offence(float x, float y, float z, float cell) {
  if (!(in_range(x) && in_range(y) && in_range(z))) return 1;
  if (!(cell_ok(cell_of(x, cell)) && cell_ok(cell_of(y, cell)) && cell_ok(cell_of(z, cell)))) return 2;
  return 0;
}

// (c_x + 2^20) << 42 | (c_y + 2^20) << 21 | (c_z + 2^20) of a vertex that vertex_offence passed
ER_SC_HD uint64_t cell_key(float x, float y, float z, float cell) {
  const uint64_t cx = (uint64_t)((long long)cell_of(x, cell) + kCellBias);
  const uint64_t cy = (uint64_t)((long long)cell_of(y, cell) + kCellBias);
  const uint64_t cz = (uint64_t)((long long)cell_of(z, cell) + kCellBias);
  return cx << 42 | cy << 21 | cz;
}

// q = llrint((double)p * 2^20): the product is exact, the rounding is half to even
ER_SC_HD long long quantise(float p) { return llrint((double)p * kQuant); }

ER_SC_HD bool normal_contributes(float x, float y, float z) { return in_range(x) && in_range(y) && in_range(z); }

// x_a = (float)(((double)S_a / (double)n) * 2^-20)
ER_SC_HD float finish_position(long long S, long long n) { return (float)(((double)S / (double)n) * kQuantInv); }

// (float)(g_a / len), len = sqrt((gx gx + gy gy) + gz gz) in float64; NaN NaN NaN when nobody contributed or len == 0
ER_SC_HD void finish_normal(long long Nx, long long Ny, long long Nz, long long contributors, float out[3]) {
  const double gx = (double)Nx, gy = (double)Ny, gz = (double)Nz;
  const double len = sqrt((gx * gx + gy * gy) + gz * gz);
  if (contributors == 0 || len == 0.0) {
    out[0] = out[1] = out[2] = NAN;
    return;
  }
  out[0] = (float)(gx / len);
  out[1] = (float)(gy / len);
  out[2] = (float)(gz / len);
}

// (2 sum + m) / (2 m) in integer division, over the m > 0 members with a != 0
ER_SC_HD unsigned finish_channel(long long sum, long long m) { return (unsigned)((2 * sum + m) / (2 * m)); }

// The rotation of (a, b, c) with its smallest entry first; the three are distinct (a degenerate triple is never keyed).
ER_SC_HD void canonical_rotation(int a, int b, int c, int out[3]) {
  if (a < b && a < c) {
    out[0] = a; out[1] = b; out[2] = c;
  } else if (b < c) {
    out[0] = b; out[1] = c; out[2] = a;
  } else {
    out[0] = c; out[1] = a; out[2] = b;
  }
}

// Where a key starts its probe sequence.  Not part of any result: which slot a key lands in shows only in the probe counts.
ER_SC_HD uint64_t mix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
ER_SC_HD uint64_t triple_hash(const int t[3]) {
  return mix64(((uint64_t)(uint32_t)t[0] << 32 | (uint64_t)(uint32_t)t[1]) ^ mix64((uint64_t)(uint32_t)t[2] + 0x9e3779b97f4a7c15ull));
}

}  // namespace er_sc
