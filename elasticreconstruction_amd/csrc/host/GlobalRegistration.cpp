// GlobalRegistration -- drop-in for the reference's GlobalRegistration.exe (GlobalRegistration/GlobalRegistration.cpp) with the numeric core --
// voxel grid, normals, FPFH, feature k-NN, the RANSAC pose search, the information matrices -- on MI355X through liber_hip.so.
//   GlobalRegistration <dir>                                do_all: every pair i < j of <dir>cloud_bin_<i>.pcd -> ./result.txt, ./result.info
//   GlobalRegistration <dir> <segment.log> <segment_length> the odometry mode: ./init.log, ./pose.log, ./odometry.log, ./odometry.info, then do_all
//                                                           unless ./result.txt exists
// <dir> is prepended to the file names as it stands, so it ends with a '/'.  ./alignment.config as the reference reads it (er_globalreg.h);
// visualization and pcl_verbose are accepted and ignored, aux_data=true is refused: the hypotheses a seed draws here are not the reference's
// rand() sequence, so a test_<i>_<j>.txt could not be compared with anything.  Every fragment is preprocessed ONCE (the reference redoes it for
// both clouds of every pair); all pairs then go through ONE er_ransac_align_batch call.
// Additive: --seed S (default 0; the reference's rand() is unseeded).  ER_TIMING=1: the stages' wall times on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iostream>
#include <string>
#include <vector>

#include <unistd.h>

#include "er_formats.h"
#include "er_globalreg.h"
#include "er_hip.h"

namespace {

const char* kWho = "GlobalRegistration";

struct Fragment {
  er_cloud_t cloud = nullptr;      // downsampled, with the estimated normals
  er_features_t feat = nullptr;
  int n = 0;
};

int fail_lib() {
  fprintf(stderr, "%s: %s\n", kWho, er_last_error());
  return 1;
}

// <dir>cloud_bin_<i>.pcd -> voxel grid -> normals -> FPFH (GlobalRegistration.cpp:52-128), once per fragment.
int preprocess(const std::string& dir, int num, const ergr::Config& cfg, std::vector<Fragment>& frags) {
  std::vector<std::vector<float>> xyz((size_t)num), nrm((size_t)num);
  for (int i = 0; i < num; i++) {
    const std::string fn = dir + "cloud_bin_" + std::to_string(i) + ".pcd";
    std::vector<std::vector<float>> cols;
    size_t n = 0;
    if (!erfmt::load_pcd_fields(fn, {"x", "y", "z", "normal_x", "normal_y", "normal_z"}, cols, n)) {
      fprintf(stderr, "%s: cannot read %s\n", kWho, fn.c_str());
      return 1;
    }
    xyz[(size_t)i].resize(n * 3);
    nrm[(size_t)i].resize(n * 3);
    for (size_t p = 0; p < n; p++)
      for (int a = 0; a < 3; a++) {
        xyz[(size_t)i][p * 3 + a] = cols[(size_t)a][p];
        nrm[(size_t)i][p * 3 + a] = cols[(size_t)a + 3][p];
      }
  }
  erfmt::stage_done("LoadData (PCD files)");
  if (er_device_count() <= 0) {
    fprintf(stderr, "%s: no HIP device available (liber_hip has no CPU fallback)\n", kWho);
    return 1;
  }
  erfmt::stage_done("HIP runtime up");
  const float cell = cfg.max_correspondence_distance;
  frags.resize((size_t)num);
  for (int i = 0; i < num; i++) {
    er_cloud_t full = nullptr, down = nullptr;
    if (er_cloud_create(xyz[(size_t)i].data(), nrm[(size_t)i].data(), (int)(xyz[(size_t)i].size() / 3), cell, 0, &full)) return fail_lib();
    const int rc = er_cloud_voxel_grid(full, cfg.resample_leaf, cell, &down, &frags[(size_t)i].n);
    er_cloud_destroy(full);
    if (rc) return fail_lib();
    if (cfg.estimate_normal) {
      er_cloud_t est = nullptr;
      const int rn = er_cloud_estimate_normals(down, cfg.normal_radius, &est, nullptr);
      er_cloud_destroy(down);
      if (rn) return fail_lib();
      down = est;
    }
    frags[(size_t)i].cloud = down;
    if (er_fpfh_estimate(down, cfg.feature_radius, &frags[(size_t)i].feat, nullptr, nullptr)) return fail_lib();
    printf("Fragment %d: %d points, %d after downsampling.\n", i, (int)(xyz[(size_t)i].size() / 3), frags[(size_t)i].n);
  }
  erfmt::stage_done("Preprocess (voxel grid, normals, FPFH)");
  return 0;
}

er_ransac_params params_of(const ergr::Config& cfg, unsigned seed) {
  er_ransac_params p;
  er_ransac_params_default(&p);
  p.max_iterations = cfg.max_iteration;
  p.nr_samples = cfg.num_of_samples;
  p.k_correspondences = cfg.correspondence_randomness;
  p.similarity = cfg.edge_similarity;
  p.max_corr_dist = cfg.max_correspondence_distance;
  p.inlier_fraction = cfg.inlier_fraction;
  p.inlier_number = cfg.inlier_number;
  p.angle_diff = cfg.angle_difference;
  p.seed = seed;
  return p;
}

// do_all's loop (GlobalRegistration.cpp:38-188) as one call: scene = i, object = j, the smaller of the two downsampled clouds the source.
int do_all(const std::vector<Fragment>& frags, const ergr::Config& cfg, unsigned seed) {
  const int num = (int)frags.size();
  std::vector<er_cloud_t> src, tgt;
  std::vector<er_features_t> sf, tf;
  std::vector<int> id1, id2, swapped;
  for (int i = 0; i < num; i++)
    for (int j = i + 1; j < num; j++) {
      int scene = i, object = j, sw = 0;
      if (cfg.smart_swap && frags[(size_t)object].n > frags[(size_t)scene].n) {
        scene = j; object = i; sw = 1;
      }
      src.push_back(frags[(size_t)object].cloud); sf.push_back(frags[(size_t)object].feat);
      tgt.push_back(frags[(size_t)scene].cloud); tf.push_back(frags[(size_t)scene].feat);
      id1.push_back(i); id2.push_back(j); swapped.push_back(sw);
    }
  const int np = (int)src.size();
  const er_ransac_params p = params_of(cfg, seed);
  std::vector<float> T((size_t)np * 16);
  std::vector<int> conv((size_t)np), cnt((size_t)np);
  std::vector<double> err((size_t)np), info_s((size_t)np * 36), info_t((size_t)np * 36);
  if (er_ransac_align_batch(np, src.data(), tgt.data(), sf.data(), tf.data(), &p, nullptr, 0, T.data(), conv.data(), cnt.data(), err.data(), nullptr,
                            info_s.data(), info_t.data()))
    return fail_lib();
  erfmt::stage_done("RANSAC (er_ransac_align_batch)");
  std::vector<erfmt::FramedTransformation> traj;
  std::vector<erfmt::FramedInformation> info;
  for (int q = 0; q < np; q++) {
    printf("Between fragments %d and %d: ", id1[(size_t)q], id2[(size_t)q]);
    if (!conv[(size_t)q]) {
      printf("alignment failed.\n");
      continue;
    }
    float M[16];
    for (int e = 0; e < 16; e++) M[e] = T[(size_t)q * 16 + e];
    if (swapped[(size_t)q] && !ergr::inverse4<float>(M, M)) {
      fprintf(stderr, "%s: the transform of pair %d %d has no inverse\n", kWho, id1[(size_t)q], id2[(size_t)q]);
      return 1;
    }
    double Md[16];
    for (int e = 0; e < 16; e++) Md[e] = (double)M[e];
    traj.push_back(ergr::framed(id1[(size_t)q], id2[(size_t)q], num, Md));
    erfmt::FramedInformation fi;
    fi.id1 = id1[(size_t)q]; fi.id2 = id2[(size_t)q]; fi.frame = num;
    const double* I = (swapped[(size_t)q] ? info_t.data() : info_s.data()) + (size_t)q * 36;
    for (int e = 0; e < 36; e++) fi.info[e] = I[e];
    info.push_back(fi);
    printf("%d inliers of %d%s, t = < %0.3f, %0.3f, %0.3f >\n", cnt[(size_t)q], frags[(size_t)(swapped[(size_t)q] ? id1[(size_t)q] : id2[(size_t)q])].n,
           swapped[(size_t)q] ? " (swapped)" : "", Md[3], Md[7], Md[11]);
  }
  if (!erfmt::save_log("result.txt", traj) || !erfmt::save_info("result.info", info)) {
    fprintf(stderr, "%s: cannot write result.txt / result.info\n", kWho);
    return 1;
  }
  erfmt::stage_done("result.txt / result.info");
  return 0;
}

// create_odometry (GlobalRegistration.cpp:219-326): for every consecutive pair, scene = i - 1 and object = i without a swap, getFitness at the
// float cast of the odometry transform; information_source_ of its inliers where align_redux accepts the guess, zeros where it does not.
int odometry(const std::vector<Fragment>& frags, const ergr::Config& cfg, const std::vector<erfmt::FramedTransformation>& odo) {
  const int num = (int)frags.size();
  std::vector<erfmt::FramedInformation> info;
  for (int i = 1; i < num; i++) {
    const Fragment &object = frags[(size_t)i], &scene = frags[(size_t)i - 1];
    float M[16];
    for (int e = 0; e < 16; e++) M[e] = (float)odo[(size_t)i - 1].T[e];
    std::vector<int> pairs((size_t)std::max(object.n, 1) * 2);
    int count = 0;
    erfmt::FramedInformation fi;
    fi.id1 = i - 1; fi.id2 = i; fi.frame = num;
    if (er_ransac_inliers(object.cloud, scene.cloud, M, cfg.max_correspondence_distance, pairs.data(), object.n, &count, nullptr, fi.info, nullptr))
      return fail_lib();
    const bool ok = ergr::redux_accepted(count, object.n, cfg.inlier_fraction, cfg.inlier_number);
    if (!ok)
      for (int e = 0; e < 36; e++) fi.info[e] = 0.0;
    printf("Between fragments %d and %d: %d inliers of %d at the odometry guess, %s.\n", i - 1, i, count, object.n, ok ? "accepted" : "not accepted");
    info.push_back(fi);
  }
  if (!erfmt::save_log("odometry.log", odo) || !erfmt::save_info("odometry.info", info)) {
    fprintf(stderr, "%s: cannot write odometry.log / odometry.info\n", kWho);
    return 1;
  }
  erfmt::stage_done("Odometry (odometry.log, odometry.info)");
  return 0;
}

int run(int argc, char** argv) {
  erfmt::stage_done("process start");
  std::vector<std::string> pos;
  unsigned seed = 0;
  for (int a = 1; a < argc; a++) {
    if (strcmp(argv[a], "--seed") == 0 && a + 1 < argc)
      seed = (unsigned)strtoul(argv[++a], nullptr, 0);
    else
      pos.push_back(argv[a]);
  }
  if (pos.empty()) {
    std::cout << "Usage : " << std::endl;
    std::cout << "    GlobalRegistration <dir> [--seed S]" << std::endl;
    std::cout << "    GlobalRegistration <dir> <100-0.log> <segment_length> [--seed S]" << std::endl;
    return 0;
  }
  const std::string dir = pos[0];
  int num = 0;
  std::error_code ec;
  for (std::filesystem::directory_iterator it(dir, ec), end; !ec && it != end; it.increment(ec))
    if (it->path().extension() == ".pcd") num++;
  if (ec) {
    fprintf(stderr, "%s: cannot list %s: %s\n", kWho, dir.c_str(), ec.message().c_str());
    return 1;
  }
  std::cout << num << " detected." << std::endl << std::endl;
  if (pos.size() != 1 && pos.size() != 3) return 0;                // (the reference does nothing for other argument counts)

  ergr::Config cfg;
  std::string why;
  const int crc = ergr::load_config("alignment.config", cfg, &why, stdout);
  if (crc == 1) std::cout << "alignment.config not found! Use default parameters." << std::endl;
  if (crc < 0) {
    fprintf(stderr, "%s: %s\n", kWho, why.c_str());
    return 1;
  }
  if (cfg.aux_data) {
    fprintf(stderr, "%s: aux_data=true is refused: the hypothesis sequence is not the reference's, a test_<i>_<j>.txt could not be compared with anything\n", kWho);
    return 1;
  }

  std::vector<erfmt::FramedTransformation> segment, odo;
  int fragment = 0;
  if (pos.size() == 3) {
    erfmt::load_log(pos[1], segment);
    fragment = atoi(pos[2].c_str());
    if (fragment < 1) {
      fprintf(stderr, "%s: segment_length %s is not a positive number\n", kWho, pos[2].c_str());
      return 1;
    }
    if ((long)segment.size() < ergr::segment_entries_needed(num, fragment)) {
      fprintf(stderr, "%s: %s has %zu entries, %d fragments of %d frames need %ld\n", kWho, pos[1].c_str(), segment.size(), num, fragment,
              ergr::segment_entries_needed(num, fragment));
      return 1;
    }
    const std::vector<erfmt::FramedTransformation> init = ergr::init_trajectory(segment, fragment);
    const std::vector<erfmt::FramedTransformation> pose = ergr::pose_trajectory(init, segment, fragment);
    odo = ergr::odometry_trajectory(pose, num);
    if ((int)odo.size() != std::max(num - 1, 0)) {
      fprintf(stderr, "%s: %s holds a pose without an inverse\n", kWho, pos[1].c_str());
      return 1;
    }
    if (!erfmt::save_log("init.log", init) || !erfmt::save_log("pose.log", pose)) {
      fprintf(stderr, "%s: cannot write init.log / pose.log\n", kWho);
      return 1;
    }
    erfmt::stage_done("init.log, pose.log");
  }

  std::vector<Fragment> frags;
  if (preprocess(dir, num, cfg, frags)) return 1;
  if (pos.size() == 3) {
    if (odometry(frags, cfg, odo)) return 1;
    if (erfmt::file_exists("result.txt")) {
      std::cout << "result.txt detected. skip global registration." << std::endl;
      return 0;
    }
  }
  return do_all(frags, cfg, seed);
}

}  // namespace

int main(int argc, char* argv[]) {
  const int rc = run(argc, argv);
  // Every output file is closed: leave without the destructors (clouds, pooled workspaces, the HIP runtime's own teardown).
  fflush(nullptr);
  _exit(rc);
}
