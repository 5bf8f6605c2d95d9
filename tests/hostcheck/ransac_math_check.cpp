// Host build of csrc/er_ransac_math.h for tests/test_ransac_math_cpu.py: the same text the kernels of er_ransac.hip compile, behind
// a C interface over arrays.
#include "er_ransac_math.h"

namespace {

template <int NS>
void select_rows(unsigned seed, int m, const unsigned* it, int n, int* out) {
  for (int i = 0; i < m; i++) {
    int s[NS];
    er_rs::select_samples<NS>(seed, it[i], n, s);
    for (int k = 0; k < NS; k++) out[(long long)i * NS + k] = s[k];
  }
}

}  // namespace

extern "C" {

void rs_draw(int m, const unsigned* seed, const unsigned* it, const unsigned* d, unsigned* out) {
  for (int i = 0; i < m; i++) out[i] = er_rs::draw(seed[i], it[i], d[i]);
}

void rs_index_of(int m, const unsigned* r, const int* mm, int* out) {
  for (int i = 0; i < m; i++) out[i] = er_rs::index_of(r[i], mm[i]);
}

// out [m][ns]; returns 1 for an ns outside 3 .. 6
int rs_select_samples(int ns, unsigned seed, int m, const unsigned* it, int n, int* out) {
  switch (ns) {
    case 3: select_rows<3>(seed, m, it, n, out); return 0;
    case 4: select_rows<4>(seed, m, it, n, out); return 0;
    case 5: select_rows<5>(seed, m, it, n, out); return 0;
    case 6: select_rows<6>(seed, m, it, n, out); return 0;
  }
  return 1;
}

// a, b [m][3]
void rs_sqdist(int m, const float* a, const float* b, float* out) {
  for (int i = 0; i < m; i++) out[i] = er_rs::sqdist(a[3 * i], a[3 * i + 1], a[3 * i + 2], b[3 * i], b[3 * i + 1], b[3 * i + 2]);
}

void rs_edge_ok(int m, const float* ds, const float* dt, float simsq, unsigned char* out) {
  for (int i = 0; i < m; i++) out[i] = er_rs::edge_ok(ds[i], dt[i], simsq) ? 1 : 0;
}

// P, Q [m][ns][3] float64; M [m][16]
void rs_rigid_estimate(int m, int ns, const double* P, const double* Q, float* M) {
  for (int i = 0; i < m; i++) {
    double p[er_rs::kMaxSamples][3], q[er_rs::kMaxSamples][3];
    for (int k = 0; k < er_rs::kMaxSamples; k++)
      for (int a = 0; a < 3; a++) {
        p[k][a] = k < ns ? P[((long long)i * ns + k) * 3 + a] : 0.0;
        q[k][a] = k < ns ? Q[((long long)i * ns + k) * 3 + a] : 0.0;
      }
    er_rs::rigid_estimate(p, q, ns, M + (long long)i * 16);
  }
}

// M [m][16], sn, tn [m][3]
void rs_normal_dot(int m, const float* M, const float* sn, const float* tn, float* out) {
  for (int i = 0; i < m; i++)
    out[i] = er_rs::normal_dot(M + (long long)i * 16, sn[3 * i], sn[3 * i + 1], sn[3 * i + 2], tn[3 * i], tn[3 * i + 1], tn[3 * i + 2]);
}
}
