// color_check -- the host-side fronts of the colour tests (tests/test_color_cpu.py, tests/color_restatement.py):
//   color_check ply <arrays.bin> <out.ply> <binary 0|1> <normals 0|1>
//       writes a coloured mesh through erfmt::save_ply (csrc/host/er_formats.h); arrays.bin: int64 nv, nt; float32 verts[nv][4]; float32
//       normals[nv][4]; int32 tris[nt][3]; uint8 colors[nv][4]
//   color_check png <in.png> <out.bin>
//       erfmt::load_png_rgb8; out.bin: int32 w, h; uint8 rgb[h][w][3].  Exit status 1 and no file if the PNG is refused.
//   color_check cells <in.bin> <out.bin>
//       er::reproject_px (csrc/er_tsdf_math.h) compiled for the host, for every pixel of one frame.  in.bin: int32 cols, rows, res; float32 cam6[6],
//       length; float64 seg[16], madj[16]; float32 ctr[(res + 1)^3][3]; uint16 depth[rows][cols].  out.bin: int32 cell[rows * cols] (-1: depth 0
//       or no cell), int32 dd[rows * cols].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../elasticreconstruction_amd/csrc/er_tsdf_math.h"
#include "../../elasticreconstruction_amd/csrc/host/er_formats.h"

template <typename V>
static bool rd(FILE* f, std::vector<V>& v) { return fread(v.data(), sizeof(V), v.size(), f) == v.size(); }

static int do_ply(char** a) {
  FILE* f = fopen(a[0], "rb");
  if (!f) return 3;
  int64_t n[2] = {0, 0};
  if (fread(n, sizeof(int64_t), 2, f) != 2) return 4;
  std::vector<float> verts((size_t)n[0] * 4), nrm((size_t)n[0] * 4);
  std::vector<int32_t> tris((size_t)n[1] * 3);
  std::vector<uint8_t> col((size_t)n[0] * 4);
  if (!rd(f, verts) || !rd(f, nrm) || !rd(f, tris) || !rd(f, col)) return 5;
  fclose(f);
  return erfmt::save_ply(a[1], verts.data(), 4, atoi(a[3]) ? nrm.data() : nullptr, 4, (size_t)n[0], tris.data(), (size_t)n[1], atoi(a[2]) != 0, col.data())
             ? 0 : 1;
}

static int do_png(char** a) {
  int w = 0, h = 0;
  std::vector<uint8_t> px;
  if (!erfmt::load_png_rgb8(a[0], w, h, px)) return 1;
  FILE* f = fopen(a[1], "wb");
  if (!f) return 3;
  const int32_t wh[2] = {w, h};
  fwrite(wh, 4, 2, f);
  fwrite(px.data(), 1, px.size(), f);
  return fclose(f) == 0 ? 0 : 3;
}

static int do_cells(char** a) {
  FILE* f = fopen(a[0], "rb");
  if (!f) return 3;
  int32_t hd[3];
  float cam6[6], length;
  double seg[16], madj[16];
  if (fread(hd, 4, 3, f) != 3 || fread(cam6, 4, 6, f) != 6 || fread(&length, 4, 1, f) != 1 || fread(seg, 8, 16, f) != 16 || fread(madj, 8, 16, f) != 16) return 4;
  const int cols = hd[0], rows = hd[1], res = hd[2];
  std::vector<float> ctr((size_t)(res + 1) * (res + 1) * (res + 1) * 3);
  std::vector<uint16_t> depth((size_t)cols * rows);
  if (!rd(f, ctr) || !rd(f, depth)) return 5;
  fclose(f);
  er::Camera cam{cam6[0], cam6[1], cam6[2], cam6[3], cam6[4], cam6[5]};
  er::CameraInv ci;
  ci.inv_fx = 1.0 / (double)cam.fx;
  ci.inv_fy = 1.0 / (double)cam.fy;
  ci.pp_small = (std::fabs((double)cam.cx) < 1e6 && std::fabs((double)cam.cy) < 1e6) ? 1 : 0;
  ci.pad = 0;
  double seg16[16] = {0};
  memcpy(seg16, seg, 12 * sizeof(double));
  er::cube_coord_deltas(seg16, cam, cols, rows, seg16 + 12);
  const float grid_ul = length / (float)res;
  std::vector<int32_t> cell((size_t)cols * rows, -1), dd((size_t)cols * rows, 0);
  for (int p = 0; p < cols * rows; p++) {
    if (depth[p] == 0) continue;
    int c;
    uint16_t d;
    if (!er::reproject_px(p % cols, p / cols, depth[p], cam, ci, cols, rows, seg16, madj, ctr.data(), res, grid_ul, c, d)) continue;
    cell[p] = c;
    dd[p] = d;
  }
  f = fopen(a[1], "wb");
  if (!f) return 3;
  fwrite(cell.data(), 4, cell.size(), f);
  fwrite(dd.data(), 4, dd.size(), f);
  return fclose(f) == 0 ? 0 : 3;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "ply" && argc == 6) return do_ply(argv + 2);
  if (cmd == "png" && argc == 4) return do_png(argv + 2);
  if (cmd == "cells" && argc == 4) return do_cells(argv + 2);
  return 2;
}
