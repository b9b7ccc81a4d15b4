// Binding-energy evaluations through the C++ mirror (cpp/AGBNPForce.h, AGBNPPlugin::Binding): the first `nligand` atoms of a
// system as the ligand.  execute() at lambda = 0.35 and energy() must agree with each other, lambda = 1 with a context of the
// complex alone, and u with E_RL - E_R - E_L formed from three contexts of its own making.
// Built and run by tests/test_gpu_binding.py (on the GPU box), compiled for syntax by tests/test_binding_api.py.
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

double energy_of(const AGBNPForce& f, const std::vector<double>& pos, std::vector<double>& forces) {
  HipCalcAGBNPForceKernel k;
  k.initialize(f);
  forces.assign(pos.size(), 0.0);
  return k.execute(pos, forces);
}
}  // namespace

int main(int argc, char** argv) {
  System s;
  if (argc < 3 || !read_system(argv[1], s)) {
    std::fprintf(stderr, "usage: TestHipBinding SYSTEM.txt NLIGAND\n");
    return 2;
  }
  const size_t n = s.r.size(), nl = (size_t)std::atoi(argv[2]);
  try {
    std::vector<double> pos, pos_l, pos_r, f_rl, f_l, f_r;
    const AGBNPForce complex_force = make_force(s, 0, n, pos);
    const double e_rl = energy_of(complex_force, pos, f_rl);
    const double e_l = energy_of(make_force(s, 0, nl, pos_l), pos_l, f_l);
    const double e_r = energy_of(make_force(s, nl, n, pos_r), pos_r, f_r);

    std::vector<int> ligand(nl);
    for (size_t i = 0; i < nl; i++) ligand[i] = (int)(nl - 1 - i);  // (descending: the order of the argument does not matter)
    Binding b(complex_force, ligand);
    const double lambda = 0.35;
    std::vector<double> f(3 * n, 0.0);
    double u = 0.0, u_only = 0.0;
    const double e = b.execute(pos, lambda, f, u);
    const double e_only = b.energy(pos, lambda, u_only);
    double worst = 0.0;
    for (size_t i = 0; i < n; i++)
      for (int d = 0; d < 3; d++) {
        const double own = i < nl ? f_l[3 * i + d] : f_r[3 * (i - nl) + d];
        worst = std::fmax(worst, std::fabs(f[3 * i + d] - (lambda * f_rl[3 * i + d] + (1.0 - lambda) * own)));
      }
    std::printf("E_RL %.9f  E_R %.9f  E_L %.9f  u %.9f  E_lambda %.9f  worst force difference %.3e\n", e_rl, e_r, e_l, u, e, worst);
    const double tol = 1e-7 * std::fmax(1.0, 1e-3 * std::fabs(e_rl));
    bool ok = std::fabs(u - (e_rl - e_r - e_l)) < 3 * tol && std::fabs(e - (e_r + e_l + lambda * u)) < 3 * tol && worst < 1e-7;
    ok = ok && std::fabs(e_only - e) < 1e-9 * std::fmax(1.0, std::fabs(e)) && std::fabs(u_only - u) < 1e-9 * std::fmax(1.0, std::fabs(u));
    ok = ok && b.finish() == 0 && b.withheld().empty() && agbnp_hip_num_particles(b.member(Binding::Ligand)) == (int)nl;
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
  } catch (const OpenMMException& ex) {
    std::fprintf(stderr, "OpenMMException: %s\n", ex.what());
    return 1;
  }
}
