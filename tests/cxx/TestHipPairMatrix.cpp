// The set-pair interaction matrix through the C++ mirror (cpp/AGBNPForce.h: HipCalcAGBNPForceKernel::setAtomSets, pairMatrix):
// with the sets of the table's last column the matrix must be symmetric, sum to the energy it returns and to the energy of
// energy(), and its rows must sum to the sets' shares of decompose()'s planes; a partition that the mirror must refuse is
// refused before the library sees it, and the one before it stays in force.
// Built and run by tests/test_gpu_pair_matrix.py (on the GPU box), compiled for syntax by tests/test_pair_matrix_api.py.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../cpp/AGBNPForce.h"

using namespace AGBNPPlugin;

int main(int argc, char** argv) {
  // whitespace table: radius gamma alpha charge ishydrogen x y z set per line (written by the driving test)
  AGBNPForce force;
  force.setVersion(1);
  std::vector<double> pos;
  std::vector<int> sets;
  std::ifstream in(argc > 1 ? argv[1] : "");
  double r, g, a, q, h, x, y, z, set;
  while (in >> r >> g >> a >> q >> h >> x >> y >> z >> set) {
    force.addParticle(r, g, a, q, h != 0.0);
    pos.push_back(x), pos.push_back(y), pos.push_back(z);
    sets.push_back((int)set);
  }
  if (sets.empty()) {
    std::fprintf(stderr, "usage: TestHipPairMatrix SYSTEM.txt\n");
    return 2;
  }
  try {
    HipCalcAGBNPForceKernel kernel;
    kernel.initialize(force);
    bool ok = kernel.numAtomSets() == 0;
    kernel.setAtomSets(sets);
    const size_t n = sets.size(), S = (size_t)kernel.numAtomSets();
    std::vector<int> bad(sets);
    bad[0] = (int)S;
    int refused = 0;
    try {
      kernel.setAtomSets(bad, (int)S);
    } catch (const OpenMMException&) {
      refused++;
    }
    try {
      kernel.setAtomSets(sets, AGBNP_HIP_MAX_SETS + 1);
    } catch (const OpenMMException&) {
      refused++;
    }
    ok = ok && refused == 2 && (size_t)kernel.numAtomSets() == S;

    std::vector<double> m, terms;
    const double e = kernel.pairMatrix(pos, m), e_planes = kernel.decompose(pos, terms), e_only = kernel.energy(pos);
    ok = ok && m.size() == S * S;
    double total = 0.0, worst_symmetry = 0.0, worst_row = 0.0;
    std::vector<double> share(S, 0.0);
    for (int t = 0; t < AGBNP_HIP_DECOMPOSITION_TERMS; t++)
      for (size_t i = 0; i < n; i++) share[sets[i]] += terms[t * n + i];
    for (size_t p = 0; p < S && ok; p++) {
      double row = 0.0;
      for (size_t c = 0; c < S; c++) {
        row += m[p * S + c];
        worst_symmetry = std::fmax(worst_symmetry, std::fabs(m[p * S + c] - m[c * S + p]));
      }
      total += row;
      worst_row = std::fmax(worst_row, std::fabs(row - share[p]));
    }
    std::printf("sets %zu  E %.9f  sum M %.9f  E(decompose) %.9f  E(energy) %.9f\n", S, e, total, e_planes, e_only);
    std::printf("worst: M - M^T %.3e, rows - planes %.3e\n", worst_symmetry, worst_row);
    const double tol = 1e-7 * std::fmax(1.0, 1e-3 * std::fabs(e));
    ok = ok && worst_symmetry < 1e-9 && worst_row < 1e-7 && std::fabs(total - e) < tol;
    ok = ok && std::fabs(e - e_planes) < 1e-9 * std::fmax(1.0, std::fabs(e)) && std::fabs(e - e_only) < tol;
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
  } catch (const OpenMMException& ex) {
    std::fprintf(stderr, "OpenMMException: %s\n", ex.what());
    return 1;
  }
}
