// raycast_math_check.cpp -- TEST-ONLY host build of csrc/er_raycast_math.h (tests/test_raycast_cpu.py compiles it with g++ -ffp-contract=off):
// the ray caster's per-pixel rule over a whole image and a volume handed in from Python, for the bit-for-bit comparison with
// tests/raycast_restatement.py.  skip = 1 marches with the kernel's empty-space skip (er_rc::skip_steps over absent units), so that the
// skip can be held to the plain march without a GPU as well.
#include "er_raycast_math.h"

#include <algorithm>

namespace {

struct F4 { float x, y, z, w; };

// units in ascending key order: keys[n], sdf[n][64^3], weight[n][64^3]
struct HostVol {
  const int* keys;
  int n;
  const float* sdf;
  const float* weight;
  bool skip;
  int ckey = -1, cidx = -1, ux = 0, uy = 0, uz = 0;

  bool fetch(int gx, int gy, int gz, float& F) {
    if ((unsigned)gx >= (unsigned)er_rc::kLattice || (unsigned)gy >= (unsigned)er_rc::kLattice || (unsigned)gz >= (unsigned)er_rc::kLattice) return false;
    const int key = (gx >> 6) << 18 | (gy >> 6) << 9 | (gz >> 6);
    if (key != ckey) {
      const int* p = std::lower_bound(keys, keys + n, key);
      ckey = key;
      cidx = (p != keys + n && *p == key) ? (int)(p - keys) : -1;
      ux = gx >> 6, uy = gy >> 6, uz = gz >> 6;
    }
    if (cidx < 0) return false;
    const size_t l = (size_t)cidx * 262144 + ((size_t)(gx & 63) * 4096 + (size_t)(gy & 63) * 64 + (size_t)(gz & 63));
    F = sdf[l];
    return weight[l] != 0.0f;
  }

  int advance(float px, float py, float pz, float step) {
    if (!skip) return 1;
    int gx, gy, gz;
    if (!(er_rc::nearest_index(px, gx) & er_rc::nearest_index(py, gy) & er_rc::nearest_index(pz, gz))) return 1;
    if (cidx >= 0 || ckey != ((gx >> 6) << 18 | (gy >> 6) << 9 | (gz >> 6))) return 1;
    return er_rc::skip_steps(px, py, pz, ux, uy, uz, step);
  }
};

}  // namespace

extern "C" {

// -> 0, or count_steps' refusal (1: not finite or step <= 0, 2: too many steps).  rec: cols * rows * 2 float4 = {v, 0}, {n, 0}; depth: cols * rows.
int rc_raycast(const int* keys, int n_units, const float* sdf, const float* weight, int cols, int rows, const float* cam4, const double* T,
               float t_min, float t_max, float step, int skip, float* rec, uint16_t* depth) {
  int n_steps = 0;
  const int bad = er_rc::count_steps(t_min, t_max, step, &n_steps);
  if (bad) return bad;
  er_rc::Image I;
  er_rc::make_image(cam4, T, t_min, step, n_steps, I);
  F4* r = reinterpret_cast<F4*>(rec);
  for (int v = 0; v < rows; v++)
    for (int u = 0; u < cols; u++) {
      HostVol vol{keys, n_units, sdf, weight, skip != 0};
      er_rc::Pixel px;
      er_rc::cast_pixel(vol, I, u, v, px);
      const size_t i = (size_t)v * cols + u;
      r[2 * i] = F4{px.v[0], px.v[1], px.v[2], 0.f};
      r[2 * i + 1] = F4{px.n[0], px.n[1], px.n[2], 0.f};
      depth[i] = px.depth;
    }
  return 0;
}

int rc_count_steps(float t_min, float t_max, float step, int* n_steps) { return er_rc::count_steps(t_min, t_max, step, n_steps); }

int rc_skip_steps(float px, float py, float pz, int ux, int uy, int uz, float step) { return er_rc::skip_steps(px, py, pz, ux, uy, uz, step); }

}  // extern "C"
