// MakeFragments.cpp -- a depth stream in, fragments out: what pcl_kinfu_largeScale writes for the rest of the pipeline (README.txt:41-60; the
// reference tree does not contain it).  Thin over er_frag_build (include/er_hip.h): every `interval` frames are a fragment,
// tracked frame-to-model against a TSDF volume of their own in the fragment's cube frame, first camera at the kinfu base pose.
//   --depth_raw <file> | --depth_list <txt>   the depth readers of Integrate: raw little-endian uint16 frames, or one 16-bit PNG path per line
//   --dir <out>                               receives cloud_bin_<k>.pcd (x y z normal_x normal_y normal_z, NaN-normal rows kept)
//   [--seg_log <file>] (<dir>/100-0.log)      entry i: "i i i+1" and the pose of frame i in its fragment's frame as %.8f rows -- what
//                                             Integrate --seg_traj and GlobalRegistration <dir> <100-0.log> <interval> read
//   [--interval N] (50)  [--lanes L] (8)  [--max_units U] (512)  [--length m] (3.0)  [--cols C --rows R] (640 x 480)  [--camera cam.param]  [--device gpu]
#include "er_formats.h"

#include "er_hip.h"

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

namespace {
const char* kWho = "MakeFragments";

int print_help() {
  printf("Usage: MakeFragments --depth_raw <raw_file> | --depth_list <txt>  --dir <out_dir>\n"
         "       [--seg_log <file> (<out_dir>/100-0.log)] [--interval <N> (50)] [--lanes <L> (8)] [--max_units <U> (512)] [--length <m> (3.0)]\n"
         "       [--cols <C> (640)] [--rows <R> (480)] [--camera <cam.param>] [--device <gpu> (0)]\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  using namespace erfmt;
  if (argc == 1 || find_switch(argc, argv, "--help") || find_switch(argc, argv, "-h")) return print_help();
  er_frag_params P;
  er_frag_params_default(&P);
  std::string raw_file, list_file, cam_file, dir, seg_file;
  int cols = 640, rows = 480, device = 0;
  double length = P.length;
  parse_argument(argc, argv, "--depth_raw", raw_file);
  parse_argument(argc, argv, "--depth_list", list_file);
  parse_argument(argc, argv, "--camera", cam_file);
  parse_argument(argc, argv, "--dir", dir);
  parse_argument(argc, argv, "--seg_log", seg_file);
  parse_argument(argc, argv, "--cols", cols);
  parse_argument(argc, argv, "--rows", rows);
  parse_argument(argc, argv, "--interval", P.interval);
  parse_argument(argc, argv, "--lanes", P.lanes);
  parse_argument(argc, argv, "--max_units", P.max_units);
  parse_argument(argc, argv, "--length", length);
  parse_argument(argc, argv, "--device", device);
  P.length = (float)length;
  if (raw_file.empty() == list_file.empty()) { fprintf(stderr, "%s: give one of --depth_raw and --depth_list\n", kWho); return 1; }
  if (dir.empty()) { fprintf(stderr, "%s: --dir is required\n", kWho); return 1; }
  if (cols <= 0 || rows <= 0) { fprintf(stderr, "%s: --cols and --rows must be positive\n", kWho); return 1; }
  if (seg_file.empty()) seg_file = dir + "/100-0.log";
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
  if (n < 1) { fprintf(stderr, "%s: no frame of %d x %d in the depth source\n", kWho, cols, rows); return 1; }
  stage_done("read depth");

  float cam[6];
  load_camera(cam_file, cam);
  er_frag_t h = nullptr;
  if (er_frag_create(cols, rows, cam, nullptr, &P, device, &h)) { fprintf(stderr, "%s: %s\n", kWho, er_last_error()); return 1; }
  std::vector<double> W((size_t)n * 16);
  std::vector<int> status((size_t)n);
  if (er_frag_build(h, n, depth.data(), 0, nullptr, 1, W.data(), status.data())) {
    fprintf(stderr, "%s: %s\n", kWho, er_last_error());
    er_frag_destroy(h);
    return 1;
  }
  stage_done("fragments");

  std::vector<FramedTransformation> traj((size_t)n);
  int lost = 0;
  for (int i = 0; i < n; i++) {
    traj[(size_t)i].id1 = traj[(size_t)i].id2 = i;
    traj[(size_t)i].frame = i + 1;
    for (int k = 0; k < 16; k++) traj[(size_t)i].T[k] = W[(size_t)i * 16 + k];
    if (status[(size_t)i] != ER_ODOM_OK) {
      lost++;
      fprintf(stderr, "%s: lost at frame %d of fragment %d (the last good pose is kept, the frame is not integrated)\n", kWho, i, i / P.interval);
    }
  }
  if (!save_log(seg_file, traj)) { fprintf(stderr, "%s: cannot write %s\n", kWho, seg_file.c_str()); er_frag_destroy(h); return 1; }
  int n_frag = 0;
  er_frag_count(h, &n_frag);
  long total = 0;
  for (int k = 0; k < n_frag; k++) {
    long m = 0;
    er_frag_read(h, k, nullptr, nullptr, 0, &m);
    std::vector<float> xyz((size_t)m * 3), nrm((size_t)m * 3), rows6((size_t)m * 6);
    if (er_frag_read(h, k, xyz.data(), nrm.data(), m, &m)) { fprintf(stderr, "%s: %s\n", kWho, er_last_error()); er_frag_destroy(h); return 1; }
    for (long i = 0; i < m; i++)
      for (int c = 0; c < 3; c++) {
        rows6[(size_t)i * 6 + c] = xyz[(size_t)i * 3 + c];
        rows6[(size_t)i * 6 + 3 + c] = nrm[(size_t)i * 3 + c];
      }
    const std::string name = dir + "/cloud_bin_" + std::to_string(k) + ".pcd";
    if (!save_pcd_xyzn(name, rows6.data(), (size_t)m)) { fprintf(stderr, "%s: cannot write %s\n", kWho, name.c_str()); er_frag_destroy(h); return 1; }
    total += m;
  }
  er_frag_destroy(h);
  stage_done("write");
  printf("%s: %d frames, %d fragments of %d, %ld points, %d lost -> %s, %s\n", kWho, n, n_frag, P.interval, total, lost, dir.c_str(), seg_file.c_str());
  return 0;
}
