// csrc/er_mesh_smooth_math.h compiled for the host (g++ -ffp-contract=off): the per-element arithmetic of mesh smoothing behind a C interface,
// for tests/test_mesh_smooth_cpu.py to compare with tests/mesh_smooth_restatement.py.
#include "er_mesh_smooth_math.h"

extern "C" {

// n rows: p [n][3], S [n][3], deg [n], one factor -> out [n][3]
void sm_moves(long n, const float* p, const long long* S, const int* deg, float f, float* out) {
  for (long i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) out[3 * i + a] = er_sm::move(p[3 * i + a], S[3 * i + a], deg[i], f);
}

// n triangles of three points each: abc [n][3][3] -> k [n][3]
void sm_area_normals(long n, const float* abc, long long* k) {
  for (long i = 0; i < n; i++) er_sm::area_normal(abc + 9 * i, abc + 9 * i + 3, abc + 9 * i + 6, k + 3 * i);
}

void sm_normals(long n, const long long* N, float* out) {
  for (long i = 0; i < n; i++) er_sc::finish_normal(N[3 * i], N[3 * i + 1], N[3 * i + 2], 1, out + 3 * i);
}

void sm_positions_ok(long n, const float* p, int* out) {
  for (long i = 0; i < n; i++) out[i] = er_sm::position_ok(p[3 * i], p[3 * i + 1], p[3 * i + 2]) ? 1 : 0;
}

void sm_factors_ok(long n, const float* f, int* out) {
  for (long i = 0; i < n; i++) out[i] = er_sm::factor_ok(f[i]) ? 1 : 0;
}

void sm_edge_keys(long n, const int* uw, uint64_t* out) {
  for (long i = 0; i < n; i++) out[i] = er_sm::edge_key(uw[2 * i], uw[2 * i + 1]);
}
}
