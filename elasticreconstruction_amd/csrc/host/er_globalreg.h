// er_globalreg.h -- the host-only parts of bin/GlobalRegistration (plain C++17, no HIP): alignment.config (GlobalRegistration/helper.h:14-134),
// the three trajectories of the odometry mode (GlobalRegistration.cpp:197-225) in float64, the acceptance rule of align_redux
// (RansacCurvature.h:801-804) and the float 4x4 inverse smart swap needs.  tests/hostcheck/globalreg_check.cpp compiles it with g++.
#pragma once

#include "er_formats.h"

#include <cerrno>
#include <string>
#include <vector>

namespace ergr {

// alignment.config; the defaults are the values the reference ships.
struct Config {
  bool visualization = false, aux_data = false, estimate_normal = true, smart_swap = true;
  int max_iteration = 4000000, num_of_samples = 4, correspondence_randomness = 2, pcl_verbose = 3, inlier_number = 30000;
  float edge_similarity = 0.9f, resample_leaf = 0.05f, max_correspondence_distance = 0.075f, inlier_fraction = 0.33f,
        angle_difference = 0.52359878f, normal_radius = 0.1f, feature_radius = 0.25f;
};

inline std::string trimmed(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && isspace((unsigned char)s[a])) a++;
  while (b > a && isspace((unsigned char)s[b - 1])) b--;
  return s.substr(a, b - a);
}

// key=value lines.  A line without '=' and an unknown key are ignored; a boolean is true exactly when its value is "true" (the reference
// compares the string); a number that does not parse is an error (*why).  Returns 0 = read, 1 = no such file (the defaults stand), -1 = error.
// echo (nullable): "key = value" for every known key, as the reference prints them.
inline int load_config(const std::string& path, Config& c, std::string* why, FILE* echo = nullptr) {
  FILE* f = fopen(path.c_str(), "r");
  if (!f) return 1;
  char buf[1024];
  int rc = 0;
  while (rc == 0 && fgets(buf, sizeof buf, f)) {
    const std::string line(buf);
    const size_t eq = line.find('=');
    if (eq == std::string::npos) continue;
    const std::string key = trimmed(line.substr(0, eq)), val = trimmed(line.substr(eq + 1));
    bool* b = key == "visualization" ? &c.visualization : key == "aux_data" ? &c.aux_data : key == "estimate_normal" ? &c.estimate_normal
              : key == "smart_swap" ? &c.smart_swap : nullptr;
    int* i = key == "max_iteration" ? &c.max_iteration : key == "num_of_samples" ? &c.num_of_samples
             : key == "correspondence_randomness" ? &c.correspondence_randomness : key == "pcl_verbose" ? &c.pcl_verbose
             : key == "inlier_number" ? &c.inlier_number : nullptr;
    float* x = key == "edge_similarity" ? &c.edge_similarity : key == "resample_leaf" ? &c.resample_leaf
               : key == "max_correspondence_distance" ? &c.max_correspondence_distance : key == "inlier_fraction" ? &c.inlier_fraction
               : key == "angle_difference" ? &c.angle_difference : key == "normal_radius" ? &c.normal_radius
               : key == "feature_radius" ? &c.feature_radius : nullptr;
    char* end = nullptr;
    errno = 0;
    if (b) {
      *b = val == "true";
      if (echo) fprintf(echo, "%s = %d\n", key.c_str(), *b ? 1 : 0);
    } else if (i) {
      const long v = strtol(val.c_str(), &end, 10);
      if (val.empty() || *end || errno || v < -2147483647L || v > 2147483647L) rc = -1;
      else *i = (int)v;
      if (echo && rc == 0) fprintf(echo, "%s = %d\n", key.c_str(), *i);
    } else if (x) {
      const double v = strtod(val.c_str(), &end);
      if (val.empty() || *end || errno) rc = -1;
      else *x = (float)v;
      if (echo && rc == 0) fprintf(echo, "%s = %g\n", key.c_str(), (double)*x);
    }
    if (rc && why) *why = "alignment.config: `" + val + "` is not a value for " + key;
  }
  fclose(f);
  return rc;
}

// ---- 4x4, row-major ----
template <typename S>
inline void mul4(const S* a, const S* b, S* out) {
  S r[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) r[i * 4 + j] = ((a[i * 4] * b[j] + a[i * 4 + 1] * b[4 + j]) + a[i * 4 + 2] * b[8 + j]) + a[i * 4 + 3] * b[12 + j];
  for (int e = 0; e < 16; e++) out[e] = r[e];
}

// The inverse by 2x2 minors (cofactor expansion, as Eigen's fixed-size 4x4 inverse is one): every product and sum in S, in the order written.
// icp.inverse4f restates it for float32, operation for operation.  Returns false (out untouched) for a zero determinant.
template <typename S>
inline bool inverse4(const S* m, S* out) {
  const S s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3], s3 = m[1] * m[6] - m[5] * m[2],
          s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
  const S c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10],
          c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
  const S det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
  if (det == S(0)) return false;
  const S d = S(1) / det;
  S r[16];
  r[0] = ((m[5] * c5 - m[6] * c4) + m[7] * c3) * d;
  r[1] = ((-m[1] * c5 + m[2] * c4) - m[3] * c3) * d;
  r[2] = ((m[13] * s5 - m[14] * s4) + m[15] * s3) * d;
  r[3] = ((-m[9] * s5 + m[10] * s4) - m[11] * s3) * d;
  r[4] = ((-m[4] * c5 + m[6] * c2) - m[7] * c1) * d;
  r[5] = ((m[0] * c5 - m[2] * c2) + m[3] * c1) * d;
  r[6] = ((-m[12] * s5 + m[14] * s2) - m[15] * s1) * d;
  r[7] = ((m[8] * s5 - m[10] * s2) + m[11] * s1) * d;
  r[8] = ((m[4] * c4 - m[5] * c2) + m[7] * c0) * d;
  r[9] = ((-m[0] * c4 + m[1] * c2) - m[3] * c0) * d;
  r[10] = ((m[12] * s4 - m[13] * s2) + m[15] * s0) * d;
  r[11] = ((-m[8] * s4 + m[9] * s2) - m[11] * s0) * d;
  r[12] = ((-m[4] * c3 + m[5] * c1) - m[6] * c0) * d;
  r[13] = ((m[0] * c3 - m[1] * c1) + m[2] * c0) * d;
  r[14] = ((-m[12] * s3 + m[13] * s1) - m[14] * s0) * d;
  r[15] = ((m[8] * s3 - m[9] * s1) + m[10] * s0) * d;
  for (int e = 0; e < 16; e++) out[e] = r[e];
  return true;
}

inline erfmt::FramedTransformation framed(int id1, int id2, int frame, const double* T) {
  erfmt::FramedTransformation t;
  t.id1 = id1; t.id2 = id2; t.frame = frame;
  for (int e = 0; e < 16; e++) t.T[e] = T[e];
  return t;
}

// ---- the odometry mode's trajectories (float64) ----
// init.log: the segment's poses chained across fragments -- at the first pose of every fragment but the first, the base becomes
// init[i - 1] * segment[i]^-1; entry i = base * segment[i], with ids (i, i, i + 1).
inline std::vector<erfmt::FramedTransformation> init_trajectory(const std::vector<erfmt::FramedTransformation>& segment, int fragment) {
  std::vector<erfmt::FramedTransformation> init;
  double base[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, inv[16], T[16];
  for (size_t i = 0; i < segment.size(); i++) {
    if (fragment > 0 && i % (size_t)fragment == 0 && i > 0 && inverse4(segment[i].T, inv)) mul4(init[i - 1].T, inv, base);
    mul4(base, segment[i].T, T);
    init.push_back(framed((int)i, (int)i, (int)i + 1, T));
  }
  return init;
}

// pose.log: every fragment-th entry of init times segment[0]^-1, ids (f, f, f + 1).
inline std::vector<erfmt::FramedTransformation> pose_trajectory(const std::vector<erfmt::FramedTransformation>& init,
                                                                const std::vector<erfmt::FramedTransformation>& segment, int fragment) {
  std::vector<erfmt::FramedTransformation> pose;
  double inv[16], T[16];
  if (segment.empty() || fragment <= 0 || !inverse4(segment[0].T, inv)) return pose;
  for (size_t i = 0; i < init.size(); i += (size_t)fragment) {
    mul4(init[i].T, inv, T);
    const int f = (int)(i / (size_t)fragment);
    pose.push_back(framed(f, f, f + 1, T));
  }
  return pose;
}

// odometry.log: pose[i - 1]^-1 * pose[i] for the num - 1 consecutive pairs, ids (i - 1, i, num).  Needs num <= pose.size().
inline std::vector<erfmt::FramedTransformation> odometry_trajectory(const std::vector<erfmt::FramedTransformation>& pose, int num) {
  std::vector<erfmt::FramedTransformation> odo;
  double inv[16], T[16];
  for (int i = 1; i < num && (size_t)i < pose.size(); i++) {
    if (!inverse4(pose[(size_t)i - 1].T, inv)) break;
    mul4(inv, pose[(size_t)i].T, T);
    odo.push_back(framed(i - 1, i, num, T));
  }
  return odo;
}

// Poses the segment must hold for num fragments of `fragment` frames: pose.log needs init's entry (num - 1) * fragment.
inline long segment_entries_needed(int num, int fragment) { return (long)(num - 1) * (long)fragment + 1; }

// align_redux's acceptance of the guess (RansacCurvature.h:801-804): the inlier share as float32 against inlier_fraction, or more than
// inlier_number inliers; without an inlier the error is not below FLT_MAX and nothing is accepted.
inline bool redux_accepted(int count, int n, float inlier_fraction, int inlier_number) {
  return count > 0 && ((float)count / (float)n >= inlier_fraction || count > inlier_number);
}

}  // namespace ergr
