// csrc/er_pgo_math.h compiled for the host (g++ -ffp-contract=off): the per-edge arithmetic of the pose graph optimiser behind a C interface, for
// tests/test_posegraph_cpu.py to compare with tests/posegraph_restatement.py.
#include "er_pgo_math.h"

extern "C" {

// n edges: Z, Xi, Xj [n][16], Om [n][36], scale, s [n], switchable [n] -> r [n][6], Ji, Jj [n][36] (unscaled), rec [n][176]
void pgo_edges(int n, const double* Z, const double* Xi, const double* Xj, const double* Om, const double* scale, const int* switchable, const double* s,
               double w, double lambda, double* r, double* Ji, double* Jj, double* rec) {
  for (int e = 0; e < n; e++) {
    double a[36], b[36];
    er_pgo::residual_jacobians(Z + 16 * e, Xi + 16 * e, Xj + 16 * e, r + 6 * e, Ji + 36 * e, Jj + 36 * e, 1);
    for (int k = 0; k < 36; k++) { a[k] = Ji[36 * e + k]; b[k] = Jj[36 * e + k]; }
    er_pgo::edge_record(Om + 36 * e, scale[e], r + 6 * e, a, b, 1, switchable[e], s[e], w, lambda, rec + er_pgo::kEdgeRec * e);
  }
}

void pgo_residuals(int n, const double* Z, const double* Xi, const double* Xj, double* r) {
  for (int e = 0; e < n; e++) er_pgo::residual(Z + 16 * e, Xi + 16 * e, Xj + 16 * e, r + 6 * e);
}

// ds [n] and Hps . dx [n] from rec [n][176], dx [n][12]
void pgo_delta_s(int n, const double* rec, const double* dx, double* ds, double* hd) {
  for (int e = 0; e < n; e++) ds[e] = er_pgo::delta_s(rec + er_pgo::kEdgeRec * e, dx + 12 * e, hd + e);
}

void pgo_from_mqt(int n, const double* d, double* D) {
  for (int e = 0; e < n; e++) er_pgo::from_mqt(d + 6 * e, D + 16 * e);
}

double pgo_edge_cost(double chi2, int switchable, double s, double w) { return er_pgo::edge_cost(chi2, switchable, s, w); }

int pgo_record_size() { return er_pgo::kEdgeRec; }
}
