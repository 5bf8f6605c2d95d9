// ply_check -- writes a mesh through erfmt::save_ply (csrc/host/er_formats.h) so that tests/test_mesh_cpu.py can compare the file byte for
// byte with formats.save_ply's.  Usage: ply_check <arrays.bin> <out.ply> <binary 0|1> <normals 0|1>
// arrays.bin: int64 nv, nt; float32 verts[nv][4]; float32 normals[nv][4]; int32 tris[nt][3]  (the layouts of er_tsdf_extract_mesh_indexed).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../elasticreconstruction_amd/csrc/host/er_formats.h"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n[2] = {0, 0};
  if (fread(n, sizeof(int64_t), 2, f) != 2) return 4;
  std::vector<float> verts((size_t)n[0] * 4), nrm((size_t)n[0] * 4);
  std::vector<int32_t> tris((size_t)n[1] * 3);
  if (fread(verts.data(), 4, verts.size(), f) != verts.size() || fread(nrm.data(), 4, nrm.size(), f) != nrm.size() ||
      fread(tris.data(), 4, tris.size(), f) != tris.size())
    return 5;
  fclose(f);
  static const float none[4] = {0.f, 0.f, 0.f, 0.f};
  const float* np = atoi(argv[4]) ? (n[0] > 0 ? nrm.data() : none) : nullptr;
  return erfmt::save_ply(argv[2], verts.data(), 4, np, 4, (size_t)n[0], tris.data(), (size_t)n[1], atoi(argv[3]) != 0) ? 0 : 1;
}
