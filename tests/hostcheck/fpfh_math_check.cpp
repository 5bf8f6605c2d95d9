// Host build of csrc/er_fpfh_math.h for tests/test_fpfh_cpu.py: the same text the kernels of er_fpfh.hip compile, behind a C interface.
#include "er_fpfh_math.h"

extern "C" {

// bins [m][3], coords [m][3] (nullable), ok [m]
void fpfh_pair_bins(int m, const float* p1, const float* n1, const float* p2, const float* n2, int* bins, double* coords, unsigned char* ok) {
  for (int i = 0; i < m; i++) {
    double b[3] = {0.0, 0.0, 0.0};
    const bool good = er_fp::pair_features(p1 + 3 * i, n1 + 3 * i, p2 + 3 * i, n2 + 3 * i, b);
    ok[i] = good ? 1 : 0;
    for (int k = 0; k < 3; k++) {
      bins[3 * i + k] = good ? er_fp::bin_of(b[k]) : -1;
      if (coords) coords[3 * i + k] = b[k];
    }
  }
}

void fpfh_voxel_index(int m, const float* x, float inv, int* out) {
  for (int i = 0; i < m; i++) out[i] = er_fp::voxel_index(x[i], inv);
}

void fpfh_sqdist32(int m, const float* a, const float* b, float* out) {
  for (int i = 0; i < m; i++) out[i] = er_fp::sqdist32(a[3 * i], a[3 * i + 1], a[3 * i + 2], b[3 * i], b[3 * i + 1], b[3 * i + 2]);
}

// c [m][6] = {xx, xy, xz, yy, yz, zz}; v [m][3], lam [m][3]
void fpfh_smallest_eigvec(int m, const double* c, double* v, double* lam) {
  for (int i = 0; i < m; i++) {
    double cc[6], vv[3], ll[3];
    for (int k = 0; k < 6; k++) cc[k] = c[6 * i + k];
    er_fp::smallest_eigvec(cc, vv, ll);
    for (int k = 0; k < 3; k++) {
      v[3 * i + k] = vv[k];
      lam[3 * i + k] = ll[k];
    }
  }
}
}
