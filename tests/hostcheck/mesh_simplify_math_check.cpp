// csrc/er_mesh_simplify_math.h compiled for the host (g++ -ffp-contract=off): the per-element arithmetic of vertex clustering behind a C
// interface, for tests/test_mesh_simplify_cpu.py to compare with tests/mesh_simplify_restatement.py.
#include "er_mesh_simplify_math.h"

extern "C" {

// n rows x y z -> offence [n], and for the rows without one key [n] and q [n][3]
void sc_vertices(long n, const float* xyz, float cell, int* offence, uint64_t* key, long long* q) {
  for (long i = 0; i < n; i++) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    offence[i] = er_sc::vertex_offence(x, y, z, cell);
    if (offence[i]) continue;
    key[i] = er_sc::cell_key(x, y, z, cell);
    q[3 * i] = er_sc::quantise(x);
    q[3 * i + 1] = er_sc::quantise(y);
    q[3 * i + 2] = er_sc::quantise(z);
  }
}

void sc_positions(long n, const long long* S, const long long* members, float* out) {
  for (long i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) out[3 * i + a] = er_sc::finish_position(S[3 * i + a], members[i]);
}

void sc_contributes(long n, const float* nrm, int* out) {
  for (long i = 0; i < n; i++) out[i] = er_sc::normal_contributes(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]) ? 1 : 0;
}

void sc_normals(long n, const long long* N, const long long* contributors, float* out) {
  for (long i = 0; i < n; i++) er_sc::finish_normal(N[3 * i], N[3 * i + 1], N[3 * i + 2], contributors[i], out + 3 * i);
}

void sc_channels(long n, const long long* sum, const long long* m, unsigned* out) {
  for (long i = 0; i < n; i++) out[i] = er_sc::finish_channel(sum[i], m[i]);
}

void sc_rotations(long n, const int* tri, int* out) {
  for (long i = 0; i < n; i++) er_sc::canonical_rotation(tri[3 * i], tri[3 * i + 1], tri[3 * i + 2], out + 3 * i);
}
}
