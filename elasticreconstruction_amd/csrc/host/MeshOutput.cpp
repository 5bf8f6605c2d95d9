// MeshOutput -- the last box of the reference workflow (README.txt:100-103: "pcl_kinfu_largeScale_mesh_output world.pcd", a tool of the
// author's PCL fork, outside the reference tree): world.pcd in, a triangle mesh out, with the numeric core on MI355X through liber_hip.so.
//
//   MeshOutput <world.pcd> [--save_to mesh.ply] [--ascii] [--no_normals] [--min_triangles N] [--largest_only] [--cell C]
//              [--smooth N [--smooth_lambda L] [--smooth_mu M] [--smooth_fix_boundary]] [--device D]
//
// world.pcd is TSDFVolume::SaveWorld's voxel list (FIELDS x y z intensity; ascii, binary or binary_compressed): integer voxel indices and
// the sdf.  The list goes back into a volume sized from its own unit keys (er_tsdf_import_world: every listed voxel observed with weight 1),
// the volume's marching-cubes mesh comes out indexed with a normal per vertex (er_tsdf_extract_mesh_indexed), and the mesh is written as
// PLY (binary little endian unless --ascii; nx ny nz unless --no_normals; a vertex without a normal gets 0 0 0).  The mesh is the one of the
// voxels the file holds: SaveWorld drops |sdf| >= 0.98 and unobserved voxels, so cells next to those are missing here and present in
// `Integrate --save_mesh`, which reads the resident volume.  --min_triangles N drops the connected components of the mesh that have fewer than
// N triangles, --largest_only all but the one with the most (er_tsdf_extract_mesh_cleaned: the unfiltered mesh never leaves the device);
// without the two the file is the unfiltered mesh.  --cell C simplifies what is left by vertex clustering, one vertex per occupied cell of C
// metres (er_tsdf_extract_mesh_simplified, in device memory too).  --smooth N runs N Taubin iterations (a pass with --smooth_lambda, 0.5, then
// a pass with --smooth_mu, -0.53; --smooth_fix_boundary holds the boundary vertices) after the cleaning and before the clustering, and the
// normals become those of the smoothed triangles (er_tsdf_extract_mesh_smoothed).  ER_TIMING=1 prints the stages.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "er_formats.h"
#include "er_hip.h"

namespace {

const char* kWho = "MeshOutput";

int print_help() {
  printf("Usage: MeshOutput <world.pcd> [options]\n"
         "  world.pcd                 the voxel list Integrate writes (FIELDS x y z intensity)\n"
         "  --save_to <file> (=mesh.ply)  the mesh: indexed triangles, PLY\n"
         "  --ascii                   write an ascii PLY (default: binary_little_endian)\n"
         "  --no_normals              leave out the per-vertex normals nx ny nz\n"
         "  --min_triangles <n> (=0)  drop the connected components of the mesh that have fewer than n triangles\n"
         "  --largest_only            keep only the connected component with the most triangles\n"
         "  --cell <metres>           simplify the mesh by vertex clustering: one vertex per occupied cell of that size\n"
         "  --smooth <n>              smooth the mesh with n Taubin iterations (after the cleaning, before the clustering)\n"
         "  --smooth_lambda <l> (=0.5)   the factor of an iteration's first pass, at most 1 in magnitude\n"
         "  --smooth_mu <m> (=-0.53)     the factor of its second pass; 0 gives plain Laplacian smoothing\n"
         "  --smooth_fix_boundary     boundary vertices stay where they are\n"
         "  --device <gpu> (=0)\n"
         "  -h [ --help ]             print this message\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  erfmt::stage_done("process start");
  using namespace erfmt;
  if (argc == 1 || find_switch(argc, argv, "--help") || find_switch(argc, argv, "-h")) return print_help();
  std::string in_file = argv[1], out_file = "mesh.ply";
  int device = 0;
  parse_argument(argc, argv, "--save_to", out_file);
  parse_argument(argc, argv, "--device", device);
  const bool ascii = find_switch(argc, argv, "--ascii"), no_normals = find_switch(argc, argv, "--no_normals");
  int min_triangles = 0;
  parse_argument(argc, argv, "--min_triangles", min_triangles);
  const bool largest_only = find_switch(argc, argv, "--largest_only"), clean = min_triangles > 1 || largest_only;
  if (min_triangles < 0) {
    fprintf(stderr, "%s: --min_triangles must not be negative\n", kWho);
    return 1;
  }
  std::string cell_text;
  const bool simplify = find_switch(argc, argv, "--cell");
  parse_argument(argc, argv, "--cell", cell_text);
  float cell = 0.0f;
  if (simplify && !parse_cell(cell_text, &cell)) {
    fprintf(stderr, "%s: --cell needs a finite size above 0, in metres\n", kWho);
    return 1;
  }
  SmoothOptions sm;
  if (!parse_smooth(argc, argv, kWho, "--smooth", &sm)) return 1;
  const bool smooth = sm.given && sm.iterations > 0;

  std::vector<std::vector<float>> cols;
  size_t n = 0;
  if (!file_exists(in_file)) {
    fprintf(stderr, "%s: cannot open %s\n", kWho, in_file.c_str());
    return 1;
  }
  if (!load_pcd_fields(in_file, {"x", "y", "z", "intensity"}, cols, n)) {
    fprintf(stderr, "%s: %s is not a PCD file this program can read\n", kWho, in_file.c_str());
    return 1;
  }
  // rows x y z intensity, and the units they name: the volume is sized from the file (a row that is no voxel index is left to
  // er_tsdf_import_world, which names it)
  std::vector<float> rows(n * 4);
  std::vector<int> keys;
  int last = -1;
  for (size_t i = 0; i < n; i++) {
    int g[3];
    bool ok = true;
    for (int a = 0; a < 3; a++) {
      const float c = cols[(size_t)a][i];
      rows[i * 4 + (size_t)a] = c;
      ok = ok && c >= -16384.0f && c <= 16383.0f;
      g[a] = ok ? (int)std::floor(c) + 256 * 64 : 0;
    }
    rows[i * 4 + 3] = cols[3][i];
    const int key = (g[0] >> 6) << 18 | (g[1] >> 6) << 9 | (g[2] >> 6);
    if (ok && key != last) keys.push_back(last = key);
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  stage_done("read world.pcd");

  if (er_device_count() <= 0) {
    fprintf(stderr, "%s: no HIP device available (liber_hip has no CPU fallback)\n", kWho);
    return 1;
  }
  er_tsdf_t vol = nullptr;
  float cam[6];
  load_camera("", cam);                                      // (the volume's image plays no part here: the default camera)
  if (er_tsdf_create(640, 480, cam, (int)std::max<size_t>(keys.size(), 1), device, &vol) != 0) {
    fprintf(stderr, "%s: %s\n", kWho, er_last_error());
    return 1;
  }
  stage_done("HIP runtime up, volume created");
  int rc = 0, n_units = 0;
  long nv = 0, nt = 0, stats[4] = {0, 0, 0, 0}, before[2] = {0, 0}, smooth_stats[4] = {0, 0, 0, 0};
  std::vector<float> verts, nrm;
  std::vector<int> tris;
  if (er_tsdf_import_world(vol, rows.data(), (long)n, &n_units) != 0) rc = 1;
  stage_done("import (er_tsdf_import_world)");
  auto extract = [&](float* v, float* q, int* t) {
    if (smooth)
      return er_tsdf_extract_mesh_smoothed(vol, sm.iterations, sm.lambda, sm.mu, sm.fix_boundary ? 1 : 0, cell, min_triangles, largest_only ? 1 : 0, 0, v, q, nullptr,
                                           nv, t, nt, &nv, &nt, smooth_stats, stats, before);
    if (simplify)
      return er_tsdf_extract_mesh_simplified(vol, cell, min_triangles, largest_only ? 1 : 0, 0, v, q, nullptr, nullptr, nv, t, nt, &nv, &nt, stats, before, nullptr);
    return clean ? er_tsdf_extract_mesh_cleaned(vol, min_triangles, largest_only ? 1 : 0, v, q, nullptr, nv, t, nt, &nv, &nt, stats)
                 : er_tsdf_extract_mesh_indexed(vol, v, q, nv, t, nt, &nv, &nt);
  };
  if (rc == 0 && extract(nullptr, nullptr, nullptr) != 0) rc = 1;
  if (rc == 0 && nv > 0) {
    verts.resize((size_t)nv * 4);
    if (!no_normals) nrm.resize((size_t)nv * 4);
    tris.resize((size_t)nt * 3);
    if (extract(verts.data(), no_normals ? nullptr : nrm.data(), tris.data()) != 0) rc = 1;
  }
  stage_done(smooth ? "mesh and smoothing (er_tsdf_extract_mesh_smoothed)" : simplify ? "mesh and simplification (er_tsdf_extract_mesh_simplified)" : clean ? "mesh and cleaning (er_tsdf_extract_mesh_cleaned)" : "mesh (er_tsdf_extract_mesh_indexed)");
  if (rc != 0) {
    fprintf(stderr, "%s: %s\n", kWho, er_last_error());
    er_tsdf_destroy(vol);
    return 1;
  }
  static const float none[4] = {0.f, 0.f, 0.f, 0.f};         // (an empty mesh with normals still declares nx ny nz)
  if (!save_ply(out_file, verts.data(), 4, no_normals ? nullptr : (nv > 0 ? nrm.data() : none), 4, (size_t)nv, tris.data(), (size_t)nt, !ascii)) {
    fprintf(stderr, "%s: cannot write %s\n", kWho, out_file.c_str());
    er_tsdf_destroy(vol);
    return 1;
  }
  stage_done("write PLY");
  if (smooth)
    printf("%s: %d iterations of lambda %g, mu %g%s: %ld vertices and %ld triangles, %ld edges (%ld boundary, %ld non-manifold), %ld vertices held\n", kWho,
           sm.iterations, (double)sm.lambda, (double)sm.mu, sm.fix_boundary ? ", boundary fixed" : "", before[0], before[1], smooth_stats[0], smooth_stats[1],
           smooth_stats[2], smooth_stats[3]);
  if (simplify)
    printf("%s: cells of %g m: %ld vertices and %ld triangles in %ld cells -> %ld vertices and %ld triangles (%ld degenerate and %ld duplicate triangles, %ld cells dropped)\n",
           kWho, (double)cell, before[0], before[1], stats[0], nv, nt, stats[1], stats[2], stats[3]);
  else if (clean && !smooth) printf("%s: %ld of %ld components kept, %ld vertices and %ld triangles dropped\n", kWho, stats[1], stats[0], stats[2], stats[3]);
  printf("%s: %zu voxels in %d units -> %ld vertices, %ld triangles -> %s\n", kWho, n, n_units, nv, nt, out_file.c_str());
  er_tsdf_destroy(vol);
  return 0;
}
