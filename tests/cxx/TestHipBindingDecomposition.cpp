// Decomposition groups and the per-atom decomposition of a binding energy through the C++ mirror (cpp/AGBNPForce.h:
// HipCalcAGBNPForceKernel::decomposeGroup, Binding::decompose): the first `nligand` atoms of a system as the ligand.
// decomposeGroup over {complex, ligand, receptor} must give every member the planes and the energy of its own decompose();
// Binding::decompose must give D[t][i] = T_RL[t][i] - T_own[t][own(i)] formed from those planes, terms that sum to the u it
// returns, and the u of Binding::energy.
// Built and run by tests/test_gpu_binding_decomposition.py (on the GPU box), compiled for syntax by
// tests/test_decompose_group_api.py.
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
  std::vector<int> h;
};

// whitespace table: radius gamma alpha charge ishydrogen x y z per line (written by the driving test)
bool read_system(const char* path, System& s) {
  std::ifstream in(path);
  if (!in) return false;
  double r, g, a, q, x, y, z, h;
  while (in >> r >> g >> a >> q >> h >> x >> y >> z) {
    s.r.push_back(r), s.g.push_back(g), s.a.push_back(a), s.q.push_back(q), s.h.push_back(h != 0.0);
    s.pos.push_back(x), s.pos.push_back(y), s.pos.push_back(z);
  }
  return !s.r.empty();
}

// the atoms [first, last) of the system as a force of their own, and their positions
AGBNPForce make_force(const System& s, size_t first, size_t last, std::vector<double>& pos) {
  AGBNPForce f;
  f.setVersion(1);
  pos.clear();
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
    std::fprintf(stderr, "usage: TestHipBindingDecomposition SYSTEM.txt NLIGAND\n");
    return 2;
  }
  const size_t n = s.r.size(), nl = (size_t)std::atoi(argv[2]), nr = n - nl;
  const int T = AGBNP_HIP_DECOMPOSITION_TERMS;
  try {
    std::vector<std::vector<double>> pos(3);
    const AGBNPForce complex_force = make_force(s, 0, n, pos[0]);
    const AGBNPForce ligand_force = make_force(s, 0, nl, pos[1]), receptor_force = make_force(s, nl, n, pos[2]);
    HipCalcAGBNPForceKernel group[3], alone[3];
    const AGBNPForce* forces[3] = {&complex_force, &ligand_force, &receptor_force};
    for (int m = 0; m < 3; m++) group[m].initialize(*forces[m]), alone[m].initialize(*forces[m]);

    // the group form against every member's own decompose() on a twin
    std::vector<std::vector<double>> terms;
    const std::vector<double> energies = HipCalcAGBNPForceKernel::decomposeGroup({&group[0], &group[1], &group[2]}, pos, terms);
    double worst_twin = 0.0, worst_sum = 0.0;
    for (int m = 0; m < 3; m++) {
      std::vector<double> own;
      const double e = alone[m].decompose(pos[m], own);
      double sum = 0.0;
      for (double t : terms[m]) sum += t;
      worst_twin = std::fmax(worst_twin, std::fmax(worst_difference(terms[m], own), std::fabs(energies[m] - e)));
      worst_sum = std::fmax(worst_sum, std::fabs(sum - energies[m]));
    }

    // the binding's decomposition against the difference of the members' planes
    std::vector<int> ligand(nl);
    for (size_t i = 0; i < nl; i++) ligand[i] = (int)(nl - 1 - i);  // (descending: the order of the argument does not matter)
    Binding b(complex_force, ligand);
    std::vector<double> d;
    const double u = b.decompose(pos[0], d);
    double u_energy = 0.0;
    b.energy(pos[0], 0.35, u_energy);
    double worst_d = d.size() == (size_t)T * n ? 0.0 : INFINITY, total = 0.0;
    for (int t = 0; t < T && d.size() == (size_t)T * n; t++)
      for (size_t i = 0; i < n; i++) {
        const double own = i < nl ? terms[1][t * nl + i] : terms[2][t * nr + (i - nl)];
        worst_d = std::fmax(worst_d, std::fabs(d[t * n + i] - (terms[0][t * n + i] - own)));
        total += d[t * n + i];
      }
    std::printf("E_RL %.9f  E_L %.9f  E_R %.9f  u %.9f  sum D %.9f\n", energies[0], energies[1], energies[2], u, total);
    std::printf("worst: group - alone %.3e, planes - energy %.3e, D - (T_RL - T_own) %.3e\n", worst_twin, worst_sum, worst_d);
    const double tol = 1e-7 * std::fmax(1.0, 1e-3 * std::fabs(energies[0]));
    bool ok = worst_twin < 1e-9 && worst_sum < 1e-7 && worst_d < 1e-9;
    ok = ok && std::fabs(u - (energies[0] - energies[1] - energies[2])) < 1e-9 * std::fmax(1.0, std::fabs(energies[0]));
    ok = ok && std::fabs(total - u) < 3 * tol && std::fabs(u_energy - u) < 1e-9 * std::fmax(1.0, std::fabs(u));
    ok = ok && b.finish() == 0 && b.withheld().empty();
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
  } catch (const OpenMMException& ex) {
    std::fprintf(stderr, "OpenMMException: %s\n", ex.what());
    return 1;
  }
}
