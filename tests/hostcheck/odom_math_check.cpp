// odom_math_check.cpp -- TEST-ONLY host build of csrc/er_odom_math.h (tests/test_odometry_cpu.py compiles it with g++ -ffp-contract=off):
// every per-pixel function of the depth odometry over whole images, for the bit-for-bit comparison with tests/odometry_restatement.py.
#include "er_odom_math.h"

#include <cstring>

namespace {
struct F4 { float x, y, z, w; };
}

extern "C" {

int od_tables(float* space, float* depth_w) { return er_od::build_tables(space, depth_w); }

void od_bilateral(const uint16_t* img, int cols, int rows, const float* space, const float* depth_w, int n_depth_w, uint16_t* out) {
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) out[(size_t)y * cols + x] = er_od::bilateral_pixel(img, cols, rows, x, y, space, depth_w, n_depth_w);
}

void od_pyr_down(const uint16_t* src, int scols, int srows, uint16_t* out) {
  for (int y = 0; y < srows / 2; y++)
    for (int x = 0; x < scols / 2; x++) out[(size_t)y * (scols / 2) + x] = er_od::pyr_down_pixel(src, scols, srows, x, y);
}

// rec[2 i] = {vertex, 0}, rec[2 i + 1] = {normal, 0}: the record layout of er_odom.hip
void od_maps(const uint16_t* depth, int cols, int rows, const float* cam4, float* rec) {
  F4* r = reinterpret_cast<F4*>(rec);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const size_t i = (size_t)y * cols + x;
      F4 v{0, 0, 0, 0}, n{0, 0, 0, 0};
      er_od::vertex(depth[i], x, y, cam4[0], cam4[1], cam4[2], cam4[3], v.x, v.y, v.z);
      er_od::normal(depth, cols, rows, x, y, cam4[0], cam4[1], cam4[2], cam4[3], n.x, n.y, n.z);
      r[2 * i] = v;
      r[2 * i + 1] = n;
    }
}

// Every pixel of cur against model at the float32 pose (R[9], t[3]): ok[i], a[i][6], b[i]; then the 27 products of every matched row.
int od_rows(const float* R, const float* t, const float* cur, const float* model, int cols, int rows, const float* cam4, float dist_thresh,
            float angle_thresh, unsigned char* ok, float* a, float* b, double* products) {
  const F4* c = reinterpret_cast<const F4*>(cur);
  const F4* m = reinterpret_cast<const F4*>(model);
  const er_od::Intr K = {cam4[0], cam4[1], cam4[2], cam4[3]};
  int count = 0;
  for (int i = 0; i < cols * rows; i++) {
    float ai[6] = {0, 0, 0, 0, 0, 0}, bi = 0.f;
    ok[i] = er_od::match_row(R, t, c[2 * i].x, c[2 * i].y, c[2 * i].z, c[2 * i + 1].x, c[2 * i + 1].y, c[2 * i + 1].z, m, cols, rows, K, dist_thresh,
                             angle_thresh, ai, bi);
    std::memcpy(a + 6 * (size_t)i, ai, sizeof ai);
    b[i] = bi;
    if (ok[i]) {
      er_od::row_products(ai, bi, products + (size_t)er_od::kSums * i);
      count++;
    } else {
      std::memset(products + (size_t)er_od::kSums * i, 0, sizeof(double) * er_od::kSums);
    }
  }
  return count;
}

}  // extern "C"
