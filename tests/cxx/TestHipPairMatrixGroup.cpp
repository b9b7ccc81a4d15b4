// Pair-matrix groups and the set-pair matrix of a binding energy through the C++ mirror (cpp/AGBNPForce.h:
// HipCalcAGBNPForceKernel::pairMatrixGroup, Binding::setAtomSets / numAtomSets / pairMatrix): the first `nligand` atoms of a system
// as the ligand, the sets of the table's last column as the partition of the complex.  pairMatrixGroup over {complex, ligand,
// receptor}, each with the partition restricted to its atoms, must give every member the matrix and the energy of its own
// pairMatrix(); Binding::pairMatrix must give D = M_RL - M_R - M_L formed from those matrices, symmetric, summing to the u it
// returns and to the u of Binding::energy, its rows summing to the sets' shares of Binding::decompose; a partition the mirror
// must refuse is refused and the one before it stays in force.
// Built and run by tests/test_gpu_pair_matrix_group.py (on the GPU box), compiled for syntax by tests/test_pair_matrix_group_api.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../../cpp/AGBNPForce.h"

using namespace AGBNPPlugin;

namespace {
struct System {
  std::vector<double> r, g, a, q, pos;
  std::vector<int> h, set;
};

// whitespace table: radius gamma alpha charge ishydrogen x y z set per line (written by the driving test)
bool read_system(const char* path, System& s) {
  std::ifstream in(path);
  if (!in) return false;
  double r, g, a, q, x, y, z, h, set;
  while (in >> r >> g >> a >> q >> h >> x >> y >> z >> set) {
    s.r.push_back(r), s.g.push_back(g), s.a.push_back(a), s.q.push_back(q), s.h.push_back(h != 0.0), s.set.push_back((int)set);
    s.pos.push_back(x), s.pos.push_back(y), s.pos.push_back(z);
  }
  return !s.r.empty();
}

// the atoms [first, last) of the system as a force of their own, their positions and their sets
AGBNPForce make_force(const System& s, size_t first, size_t last, std::vector<double>& pos, std::vector<int>& sets) {
  AGBNPForce f;
  f.setVersion(1);
  pos.clear();
  sets.assign(s.set.begin() + first, s.set.begin() + last);
  for (size_t i = first; i < last; i++) {
    f.addParticle(s.r[i], s.g[i], s.a[i], s.q[i], s.h[i] != 0);
    pos.insert(pos.end(), s.pos.begin() + 3 * i, s.pos.begin() + 3 * i + 3);
  }
  return f;
}

double worst_difference(const std::vector<double>& a, const std::vector<double>& b) {
  if (a.size() != b.size()) return INFINITY;
  double worst = 0.0;
  for (size_t k = 0; k < a.size(); k++) worst = std::fmax(worst, std::fabs(a[k] - b[k]));
  return worst;
}
}  // namespace

int main(int argc, char** argv) {
  System s;
  if (argc < 3 || !read_system(argv[1], s)) {
    std::fprintf(stderr, "usage: TestHipPairMatrixGroup SYSTEM.txt NLIGAND\n");
    return 2;
  }
  const size_t n = s.r.size(), nl = (size_t)std::atoi(argv[2]);
  int highest = 0;
  for (int a : s.set) highest = a > highest ? a : highest;
  const size_t S = (size_t)highest + 1;
  try {
    std::vector<std::vector<double>> pos(3);
    std::vector<int> sets[3];
    const AGBNPForce complex_force = make_force(s, 0, n, pos[0], sets[0]);
    const AGBNPForce ligand_force = make_force(s, 0, nl, pos[1], sets[1]), receptor_force = make_force(s, nl, n, pos[2], sets[2]);
    HipCalcAGBNPForceKernel group[3], alone[3];
    const AGBNPForce* forces[3] = {&complex_force, &ligand_force, &receptor_force};
    for (int m = 0; m < 3; m++) {
      group[m].initialize(*forces[m]), alone[m].initialize(*forces[m]);
      group[m].setAtomSets(sets[m], (int)S), alone[m].setAtomSets(sets[m], (int)S);
    }

    // the group form against every member's own pairMatrix() on a twin
    std::vector<std::vector<double>> matrices;
    const std::vector<double> energies = HipCalcAGBNPForceKernel::pairMatrixGroup({&group[0], &group[1], &group[2]}, pos, matrices);
    double worst_twin = 0.0, worst_sum = 0.0;
    for (int m = 0; m < 3; m++) {
      std::vector<double> own;
      const double e = alone[m].pairMatrix(pos[m], own);
      double sum = 0.0;
      for (double c : matrices[m]) sum += c;
      worst_twin = std::fmax(worst_twin, std::fmax(worst_difference(matrices[m], own), std::fabs(energies[m] - e)));
      worst_sum = std::fmax(worst_sum, std::fabs(sum - energies[m]));
    }
    // a member without a partition is refused by the mirror
    HipCalcAGBNPForceKernel bare;
    bare.initialize(ligand_force);
    int refused = 0;
    try {
      std::vector<std::vector<double>> none;
      HipCalcAGBNPForceKernel::pairMatrixGroup({&group[0], &bare}, {pos[0], pos[1]}, none);
    } catch (const OpenMMException&) {
      refused++;
    }

    // the binding's matrix against the difference of the members' matrices
    std::vector<int> ligand(nl);
    for (size_t i = 0; i < nl; i++) ligand[i] = (int)(nl - 1 - i);  // (descending: the order of the argument does not matter)
    Binding b(complex_force, ligand);
    bool ok = b.numAtomSets() == 0;
    b.setAtomSets(s.set, (int)S);
    std::vector<int> bad(s.set);
    bad[0] = (int)S;
    try {
      b.setAtomSets(bad, (int)S);
    } catch (const OpenMMException&) {
      refused++;
    }
    ok = ok && refused == 2 && (size_t)b.numAtomSets() == S;
    std::vector<double> d, terms;
    const double u = b.pairMatrix(pos[0], d), u_terms = b.decompose(pos[0], terms);
    double u_energy = 0.0;
    b.energy(pos[0], 0.35, u_energy);
    ok = ok && d.size() == S * S;
    double worst_d = 0.0, worst_symmetry = 0.0, worst_row = 0.0, total = 0.0;
    std::vector<double> share(S, 0.0);
    for (int t = 0; t < AGBNP_HIP_DECOMPOSITION_TERMS; t++)
      for (size_t i = 0; i < n; i++) share[s.set[i]] += terms[t * n + i];
    for (size_t p = 0; p < S && ok; p++) {
      double row = 0.0;
      for (size_t c = 0; c < S; c++) {
        const size_t at = p * S + c;
        row += d[at];
        worst_d = std::fmax(worst_d, std::fabs(d[at] - (matrices[0][at] - matrices[1][at] - matrices[2][at])));
        worst_symmetry = std::fmax(worst_symmetry, std::fabs(d[at] - d[c * S + p]));
      }
      total += row;
      worst_row = std::fmax(worst_row, std::fabs(row - share[p]));
    }
    std::printf("sets %zu  E_RL %.9f  E_L %.9f  E_R %.9f  u %.9f  sum D %.9f\n", S, energies[0], energies[1], energies[2], u, total);
    std::printf("worst: group - alone %.3e, cells - energy %.3e, D - (M_RL - M_R - M_L) %.3e, D - D^T %.3e, rows - planes %.3e\n",
                worst_twin, worst_sum, worst_d, worst_symmetry, worst_row);
    const double tol = 1e-7 * std::fmax(1.0, 1e-3 * std::fabs(energies[0]));
    ok = ok && worst_twin < 1e-9 && worst_sum < tol && worst_d < 1e-9 && worst_symmetry < 1e-9 && worst_row < 5e-7;
    ok = ok && std::fabs(u - (energies[0] - energies[1] - energies[2])) < 1e-9 * std::fmax(1.0, std::fabs(energies[0]));
    ok = ok && std::fabs(total - u) < 3 * tol && std::fabs(u_energy - u) < 1e-9 * std::fmax(1.0, std::fabs(u));
    ok = ok && std::fabs(u_terms - u) < 1e-9 * std::fmax(1.0, std::fabs(u));
    ok = ok && b.finish() == 0 && b.withheld().empty();
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
  } catch (const OpenMMException& ex) {
    std::fprintf(stderr, "OpenMMException: %s\n", ex.what());
    return 1;
  }
}
