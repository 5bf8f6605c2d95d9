// Host build of csrc/er_grid.h for tests/test_nn_margin.py: grid_slack as the cloud builder calls it, behind a C interface.
#include "er_grid.h"

extern "C" float gs_grid_slack(int dx, int dy, int dz, float cell) {
  const int dim[3] = {dx, dy, dz};
  return er::grid_slack(dim, cell);
}
