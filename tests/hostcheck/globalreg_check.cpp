// The host-only parts of bin/GlobalRegistration (csrc/host/er_globalreg.h) behind a C interface for tests/test_global_registration_cpu.py.
#include "er_globalreg.h"

extern "C" {

// bools: visualization, aux_data, estimate_normal, smart_swap; ints: max_iteration, num_of_samples, correspondence_randomness, pcl_verbose,
// inlier_number; floats: edge_similarity, resample_leaf, max_correspondence_distance, inlier_fraction, angle_difference, normal_radius,
// feature_radius.  Returns load_config's code.
int gr_load_config(const char* path, int* bools, int* ints, float* floats, char* why, int why_cap) {
  ergr::Config c;
  std::string w;
  const int rc = ergr::load_config(path, c, &w);
  bools[0] = c.visualization; bools[1] = c.aux_data; bools[2] = c.estimate_normal; bools[3] = c.smart_swap;
  ints[0] = c.max_iteration; ints[1] = c.num_of_samples; ints[2] = c.correspondence_randomness; ints[3] = c.pcl_verbose; ints[4] = c.inlier_number;
  floats[0] = c.edge_similarity; floats[1] = c.resample_leaf; floats[2] = c.max_correspondence_distance; floats[3] = c.inlier_fraction;
  floats[4] = c.angle_difference; floats[5] = c.normal_radius; floats[6] = c.feature_radius;
  if (why && why_cap > 0) snprintf(why, (size_t)why_cap, "%s", w.c_str());
  return rc;
}

static void put(const std::vector<erfmt::FramedTransformation>& v, int* ids, double* T) {
  for (size_t i = 0; i < v.size(); i++) {
    ids[i * 3] = v[i].id1; ids[i * 3 + 1] = v[i].id2; ids[i * 3 + 2] = v[i].frame;
    for (int e = 0; e < 16; e++) T[i * 16 + e] = v[i].T[e];
  }
}

// The three constructions from n_seg poses; every output holds room for n_seg entries.  counts: entries of init, pose, odometry.
void gr_trajectories(int n_seg, const double* seg, int fragment, int num, int* counts, int* init_ids, double* init_T, int* pose_ids, double* pose_T,
                     int* odo_ids, double* odo_T) {
  std::vector<erfmt::FramedTransformation> segment((size_t)n_seg);
  for (int i = 0; i < n_seg; i++) segment[(size_t)i] = ergr::framed(i, i, i + 1, seg + (size_t)i * 16);
  const auto init = ergr::init_trajectory(segment, fragment);
  const auto pose = ergr::pose_trajectory(init, segment, fragment);
  const auto odo = ergr::odometry_trajectory(pose, num);
  counts[0] = (int)init.size(); counts[1] = (int)pose.size(); counts[2] = (int)odo.size();
  put(init, init_ids, init_T);
  put(pose, pose_ids, pose_T);
  put(odo, odo_ids, odo_T);
}

long gr_segment_entries_needed(int num, int fragment) { return ergr::segment_entries_needed(num, fragment); }

int gr_redux_accepted(int count, int n, float inlier_fraction, int inlier_number) { return ergr::redux_accepted(count, n, inlier_fraction, inlier_number) ? 1 : 0; }

int gr_inverse4f(const float* m, float* out) { return ergr::inverse4<float>(m, out) ? 1 : 0; }

}  // extern "C"
