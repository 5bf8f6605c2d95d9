// GraphOptimizer.cpp -- drop-in for the reference's GraphOptimizer (GraphOptimizer/GraphOptimizer.cpp, OptApp.cpp): the candidate loop closures of
// GlobalRegistration in, pruned closures and fragment poses out.  Thin over er_pgo_optimize (include/er_hip.h); the model is the
// reference's, the solver is the library's own (g2o cannot be built from the reference tree).
//   --function/-f switchable|em (switchable)   --weight/-w <w> (1.0)   --iteration/-i <n> (100)
//   --odometry <odometry.log>  --odometryinfo <odometry.info>  --loop <loop.log>  --loopinfo <loop.info>
//   --pose <opt_output.log>    --keep <loop_remain.log>        --refine <refine.log>
// Every option as "--name value", "--name=value" or, where it has one, the short form "-x value".  No argument or --help/-h: the options, exit code 1.
// A missing odometry log: no work, exit code 0.  Missing .info files: identity information.
#include "er_formats.h"

#include "er_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace {
const char* kWho = "GraphOptimizer";

int print_help() {
  printf("Generic Options:\n"
         "  -h [ --help ]                         print this message\n"
         "  -f [ --function ] arg (=switchable)   possible choices: switchable/em\n"
         "  -w [ --weight ] arg (=1)              weight for switchable constraint penalty\n"
         "  -i [ --iteration ] arg (=100)         maximum optimization iteration\n\n"
         "Input/Output Options (configured automatically if not otherwise specified):\n"
         "  --odometry arg (=odometry.log)        odometry transformations\n"
         "  --odometryinfo arg (=odometry.info)   odometry information matrices, optional\n"
         "  --loop arg (=loop.log)                loop closure transformations\n"
         "  --loopinfo arg (=loop.info)           loop closure information matrices, optional\n"
         "  --pose arg (=opt_output.log)          output poses of fragments\n"
         "  --keep arg (=loop_remain.log)         output pruned loop closure transformations\n"
         "  --refine arg (=refine.log)            loop closure and odometry edges that need to be refined\n\n");
  return 1;
}

// "--name value", "--name=value", "-x value" (short may be NULL); the last occurrence wins
bool option(int argc, char** argv, const char* name, const char* short_name, std::string& v) {
  const std::string eq = std::string(name) + "=";
  bool found = false;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if ((a == name || (short_name && a == short_name)) && i + 1 < argc) { v = argv[++i]; found = true; }
    else if (a.compare(0, eq.size(), eq) == 0) { v = a.substr(eq.size()); found = true; }
  }
  return found;
}
}  // namespace

int main(int argc, char** argv) {
  using namespace erfmt;
  if (argc == 1 || find_switch(argc, argv, "--help") || find_switch(argc, argv, "-h")) return print_help();
  std::string method = "switchable", weight_s = "1.0", iter_s = "100";
  std::string odo_file = "odometry.log", odo_info_file = "odometry.info", loop_file = "loop.log", loop_info_file = "loop.info";
  std::string pose_file = "opt_output.log", keep_file = "loop_remain.log", refine_file = "refine.log";
  option(argc, argv, "--function", "-f", method);
  option(argc, argv, "--weight", "-w", weight_s);
  option(argc, argv, "--iteration", "-i", iter_s);
  option(argc, argv, "--odometry", nullptr, odo_file);
  option(argc, argv, "--odometryinfo", nullptr, odo_info_file);
  option(argc, argv, "--loop", nullptr, loop_file);
  option(argc, argv, "--loopinfo", nullptr, loop_info_file);
  option(argc, argv, "--pose", nullptr, pose_file);
  option(argc, argv, "--keep", nullptr, keep_file);
  option(argc, argv, "--refine", nullptr, refine_file);
  const double weight = atof(weight_s.c_str());
  const int iteration = atoi(iter_s.c_str());
  if (method != "switchable" && method != "em") return 0;                     // (GraphOptimizer.cpp:58-66: neither branch runs)

  // COptApp::Init
  std::vector<FramedTransformation> odo, loops;
  std::vector<FramedInformation> odo_info, loop_info;
  if (file_exists(odo_file)) {
    load_log(odo_file, odo);
    if (file_exists(odo_info_file)) load_info(odo_info_file, odo_info);
  }
  if (file_exists(loop_file)) {
    load_log(loop_file, loops);
    if (file_exists(loop_info_file)) load_info(loop_info_file, loop_info);
  }
  if (odo.empty()) return 0;
  stage_done("read logs");
  if (!odo_info.empty() && odo_info.size() != odo.size()) {
    fprintf(stderr, "%s: %s has %d entries, %s has %d\n", kWho, odo_info_file.c_str(), (int)odo_info.size(), odo_file.c_str(), (int)odo.size());
    return 1;
  }
  if (!loop_info.empty() && loop_info.size() != loops.size()) {
    fprintf(stderr, "%s: %s has %d entries, %s has %d\n", kWho, loop_info_file.c_str(), (int)loop_info.size(), loop_file.c_str(), (int)loops.size());
    return 1;
  }
  if (er_device_count() <= 0) {
    fprintf(stderr, "%s: no HIP device available (liber_hip has no CPU fallback)\n", kWho);
    return 1;
  }
  const int n_poses = (int)odo.size() + 1, n_loops = (int)loops.size();
  std::vector<double> oT((size_t)odo.size() * 16), oI((size_t)odo_info.size() * 36), lT((size_t)n_loops * 16), lI((size_t)loop_info.size() * 36);
  std::vector<int> ids((size_t)n_loops * 2);
  for (size_t i = 0; i < odo.size(); i++) std::copy(odo[i].T, odo[i].T + 16, &oT[16 * i]);
  for (size_t i = 0; i < odo_info.size(); i++) std::copy(odo_info[i].info, odo_info[i].info + 36, &oI[36 * i]);
  for (int k = 0; k < n_loops; k++) {
    std::copy(loops[k].T, loops[k].T + 16, &lT[16 * (size_t)k]);
    ids[2 * k] = loops[k].id1;
    ids[2 * k + 1] = loops[k].id2;
  }
  for (size_t k = 0; k < loop_info.size(); k++) std::copy(loop_info[k].info, loop_info[k].info + 36, &lI[36 * k]);

  er_pgo_t h = nullptr;
  if (er_pgo_create(n_poses, n_loops, oT.data(), oI.empty() ? nullptr : oI.data(), ids.data(), lT.data(), lI.empty() ? nullptr : lI.data(), 0, &h)) {
    fprintf(stderr, "%s: %s\n", kWho, er_last_error());
    return 1;
  }
  stage_done("build graph");
  const bool sw = method == "switchable";
  std::vector<double> poses((size_t)n_poses * 16), values((size_t)n_loops + 1);
  int its = 0, trials = 0;
  if (er_pgo_optimize(h, sw ? ER_PGO_SWITCHABLE : ER_PGO_EM, weight, iteration, poses.data(), values.data(), &its, &trials, nullptr)) {
    fprintf(stderr, "%s: %s\n", kWho, er_last_error());
    er_pgo_destroy(h);
    return 1;
  }
  er_pgo_destroy(h);
  stage_done("optimize (er_pgo_optimize)");

  std::vector<FramedTransformation> pose_traj(n_poses), remain, refine;
  for (int i = 0; i < n_poses; i++) {
    pose_traj[i].id1 = pose_traj[i].id2 = i;
    pose_traj[i].frame = i + 1;
    std::copy(&poses[16 * (size_t)i], &poses[16 * (size_t)i] + 16, pose_traj[i].T);
  }
  const double keep_above = sw ? 0.5 : 0.25;                                  // OptApp.cpp:142, 260
  for (int k = 0; k < n_loops; k++)
    if (values[k] > keep_above) remain.push_back(loops[k]);
  bool ok = save_log(pose_file, pose_traj) && save_log(keep_file, remain);
  if (sw) {
    refine = odo;
    for (const auto& t : remain)
      if (t.id1 + 1 < t.id2) refine.push_back(t);
    ok = ok && save_log(refine_file, refine);
  }
  if (!ok) { fprintf(stderr, "%s: cannot write the output logs\n", kWho); return 1; }
  stage_done("write logs");
  printf("%s: %d poses, %d loop closures, %d kept; %d iterations, %d trials (%s)\n", kWho, n_poses, n_loops, (int)remain.size(), its, trials, method.c_str());
  return 0;
}
