// DepthOdometry.cpp -- a depth stream in, a trajectory out: the tracker half of the step that the real pipeline runs first (pcl_kinfu_largeScale
// writes the trajectory and the fragments; the reference tree does not contain it).  Thin over er_odom_align_pairs (include/er_hip.h):
// frame against frame, every pair of the stream in one batched call.
//   --depth_raw <file> | --depth_list <txt>   the depth readers of Integrate: raw little-endian uint16 frames, or one 16-bit PNG path per line
//   [--cols C --rows R] (640 x 480)  [--camera cam.param]  [--interval N]  [--window W]  [--device gpu]
//   --traj_log <out.log>                      entry i: "i i i+1" and world_T_camera(i) as %.8f rows (RGBDTrajectory's format), frame 0 at the identity.
// With --interval N the identity restarts every N frames: the segment log that Integrate --seg_traj consumes.
#include "er_formats.h"

#include "er_hip.h"

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

namespace {
const char* kWho = "DepthOdometry";

int print_help() {
  printf("Usage: DepthOdometry --depth_raw <raw_file> | --depth_list <txt>  --traj_log <out.log>\n"
         "       [--cols <C> (640)] [--rows <R> (480)] [--camera <cam.param>] [--interval <N>] [--window <W>] [--device <gpu> (0)]\n");
  return 0;
}

// C = A B, row-major 4x4, ((a0 b0 + a1 b1) + a2 b2) + a3 b3 (odometry.accumulate spells out the same order)
void mul4(const double* A, const double* B, double* C) {
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++)
      C[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}
}  // namespace

int main(int argc, char** argv) {
  using namespace erfmt;
  if (argc == 1 || find_switch(argc, argv, "--help") || find_switch(argc, argv, "-h")) return print_help();
  std::string raw_file, list_file, cam_file, out_file;
  int cols = 640, rows = 480, interval = 0, window = 0, device = 0;
  parse_argument(argc, argv, "--depth_raw", raw_file);
  parse_argument(argc, argv, "--depth_list", list_file);
  parse_argument(argc, argv, "--camera", cam_file);
  parse_argument(argc, argv, "--traj_log", out_file);
  parse_argument(argc, argv, "--cols", cols);
  parse_argument(argc, argv, "--rows", rows);
  parse_argument(argc, argv, "--interval", interval);
  parse_argument(argc, argv, "--window", window);
  parse_argument(argc, argv, "--device", device);
  if (raw_file.empty() == list_file.empty()) { fprintf(stderr, "%s: give one of --depth_raw and --depth_list\n", kWho); return 1; }
  if (out_file.empty()) { fprintf(stderr, "%s: --traj_log is required\n", kWho); return 1; }
  if (cols <= 0 || rows <= 0 || interval < 0) { fprintf(stderr, "%s: --cols, --rows must be positive and --interval not negative\n", kWho); return 1; }
  if (er_device_count() <= 0) {
    fprintf(stderr, "%s: no HIP device available (liber_hip has no CPU fallback)\n", kWho);
    return 1;
  }
  const size_t px = (size_t)cols * rows;
  std::vector<uint16_t> depth;
  if (!raw_file.empty()) {
    FILE* f = fopen(raw_file.c_str(), "rb");
    if (!f) { fprintf(stderr, "%s: cannot open %s\n", kWho, raw_file.c_str()); return 1; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    depth.resize((size_t)bytes / sizeof(uint16_t) / px * px);
    const size_t got = depth.empty() ? 0 : fread(depth.data(), sizeof(uint16_t), depth.size(), f);
    fclose(f);
    if (got != depth.size()) { fprintf(stderr, "%s: short read of %s\n", kWho, raw_file.c_str()); return 1; }
  } else {
    std::ifstream in(list_file);
    if (!in) { fprintf(stderr, "%s: cannot open %s\n", kWho, list_file.c_str()); return 1; }
    std::string line;
    std::vector<uint16_t> img;
    while (std::getline(in, line)) {
      if (line.empty()) continue;
      int w = 0, h = 0;
      if (!load_png16(line, w, h, img) || w != cols || h != rows) { fprintf(stderr, "%s: %s is not a %d x %d 16-bit PNG\n", kWho, line.c_str(), cols, rows); return 1; }
      depth.insert(depth.end(), img.begin(), img.end());
    }
  }
  const int n = (int)(depth.size() / px);
  if (n < 2) { fprintf(stderr, "%s: %d frames of %d x %d in the depth source, a trajectory needs at least 2\n", kWho, n, cols, rows); return 1; }
  stage_done("read depth");

  float cam[6];
  load_camera(cam_file, cam);
  er_odom_params P;
  er_odom_params_default(&P);
  er_odom_t h = nullptr;
  if (er_odom_create(cols, rows, cam, &P, device, &h)) { fprintf(stderr, "%s: %s\n", kWho, er_last_error()); return 1; }
  std::vector<int> mi, fi;
  for (int i = 1; i < n; i++)
    if (!(interval > 0 && i % interval == 0)) { mi.push_back(i - 1); fi.push_back(i); }
  std::vector<double> T(mi.size() * 16 + 16);
  std::vector<int> status(mi.size() + 1);
  if (er_odom_align_pairs(h, n, depth.data(), 0, (int)mi.size(), mi.data(), fi.data(), nullptr, T.data(), status.data(), nullptr, nullptr, window)) {
    fprintf(stderr, "%s: %s\n", kWho, er_last_error());
    er_odom_destroy(h);
    return 1;
  }
  er_odom_destroy(h);
  stage_done("odometry");

  std::vector<FramedTransformation> traj(n);
  int lost = 0;
  size_t p = 0;
  for (int i = 0; i < n; i++) {
    traj[i].id1 = traj[i].id2 = i;
    traj[i].frame = i + 1;
    if (i == 0 || (interval > 0 && i % interval == 0)) {
      for (int k = 0; k < 16; k++) traj[i].T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    } else {
      mul4(traj[i - 1].T, &T[p * 16], traj[i].T);
      if (status[p] != ER_ODOM_OK) {
        lost++;
        fprintf(stderr, "%s: lost between frames %d and %d (the last good pose is kept)\n", kWho, i - 1, i);
      }
      p++;
    }
  }
  if (!save_log(out_file, traj)) { fprintf(stderr, "%s: cannot write %s\n", kWho, out_file.c_str()); return 1; }
  printf("%s: %d frames, %d pairs, %d lost -> %s\n", kWho, n, (int)mi.size(), lost, out_file.c_str());
  return 0;
}
