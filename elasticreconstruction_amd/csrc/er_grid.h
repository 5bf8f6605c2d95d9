// er_grid.h -- what host and device code of path B share about a cloud's uniform grid: the block size, the grid descriptor the search kernels take by
// value, and the pruning margin the host sizes from the grid's extent.  Plain C++ (no HIP header): tests/hostcheck/grid_slack_check.cpp compiles it with g++.
#pragma once

#include <algorithm>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
struct float4;   // (a host-only build never touches a point: an opaque type keeps Grid's layout)
#endif

namespace er {

constexpr int kBlock = 256;
constexpr int kSentinel = 8;            // float4 entries of +inf behind every cloud's sorted array (>= the largest kU - 1 of scan_range, er_nn.h)

// The grid carries TWO RINGS OF EMPTY CELLS around the cloud's bounding box (cell (x, y, z) of the box is cell (x + 2, y + 2, z + 2) of the array).  A query is
// searched only if its home cell lies within one cell of the box, so every cell of its 27-neighbourhood EXISTS -- no flags, range tests or clamps -- and
// the four bounds L, O, R, E of a row's three cells x-1, x, x+1 are four consecutive ints of cell_start: one 16-byte load per row.
// (What was tried on this search and dropped, with numbers: profiles/HISTORY.md "Path B: the search, rounds 3-6".)
struct Grid {
  const float4* pts;
  const int* cell_start;
  float org[3];
  float cell;
  int dim[3];      // cells of the bounding box per axis (the array has dim + 4 per axis: two rings of empty cells)
  float slack;     // absolute part of nn_block's pruning margin (square metres), from the grid's extent: grid_slack()
  int pnx, pny;    // dim[0] + 4, dim[1] + 4: strides of the padded array
  const unsigned char* occ;   // [cells] 1 = some cell of this cell's 27-neighbourhood holds a point (round 6; see nn_block)
};

// The grid of one cloud of a chunk as the cloud builder's kernels see it (er_cloud.hip: ChunkDesc).
struct GridDims {
  float org[3];
  float cell;
  int dim[3];
};

// The pruning margin of nn_block.  A cell (or row of cells) is skipped when the squared distance f'^2 from the query to its nearest face, as the
// kernel computes it, exceeds  B * (1 + 1e-4) + slack,  B = the best float32 squared distance so far (or the squared search radius).  For that to
// be exact -- no point p of a skipped cell may have a float32 distance below B -- the margin has to cover what the float32 cell arithmetic can be
// off by:  u = fl(fl(q - org) / cell) carries a relative error of 2 x 2^-24, i.e. up to 1.2e-7 x |q - org| metres in the face distance, and the
// target points were assigned to their cells by the same expression, so the face itself is that fuzzy once more:  f' <= f + D  per axis with
// D = 2.5e-7 x (largest extent + 2 cells) + 4e-9, and sqrt(3) D for the rows and corners that combine two or three axes.  With S^2 = B (1 + r) + A,
// a skipped point has a true distance >= S - sqrt(3) D, its float32 squared distance is >= (S - sqrt(3) D)^2 (1 - 3e-7), and
// 2 S sqrt(3) D <= (r / 4) S^2 + 12 D^2 / r  gives  (S - sqrt(3) D)^2 (1 - 3e-7) >= B  as soon as  A >= 1.2001e5 D^2  (r = 1e-4); the code takes 1.3e5.
// (A constant absolute part would cover D only for best distances below a micrometre or above several millimetres; tests/test_icp_gpu.py builds the
// queries in between on purpose.)
inline float grid_slack(const int dim[3], float cell) {
  const int big = std::max(dim[0], std::max(dim[1], dim[2]));
  const double D = 2.5e-7 * (double)(big + 2) * (double)cell + 4e-9;
  return (float)(1.3e5 * D * D);
}

}  // namespace er
