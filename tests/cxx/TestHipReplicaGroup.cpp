// Replica groups through the C++ mirror (cpp/AGBNPForce.h, HipCalcAGBNPForceKernel::executeGroup): three contexts -- two of one
// system, one of another -- evaluated in one call; each must agree with the same context's own execute() at the same positions.
// Built and run by tests/test_gpu_replica_group.py (on the GPU box), compiled for syntax by tests/test_replica_group_api.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
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
  double r, g, a, q, x, y, z;
  int h;
  while (in >> r >> g >> a >> q >> h >> x >> y >> z) {
    s.r.push_back(r), s.g.push_back(g), s.a.push_back(a), s.q.push_back(q), s.h.push_back(h);
    s.pos.push_back(x), s.pos.push_back(y), s.pos.push_back(z);
  }
  return !s.r.empty();
}

AGBNPForce make_force(const System& s) {
  AGBNPForce f;
  f.setVersion(1);
  for (size_t i = 0; i < s.r.size(); i++) f.addParticle(s.r[i], s.g[i], s.a[i], s.q[i], s.h[i] != 0);
  return f;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s system_a.txt system_b.txt\n", argv[0]);
    return 2;
  }
  System sa, sb;
  if (!read_system(argv[1], sa) || !read_system(argv[2], sb)) {
    std::fprintf(stderr, "cannot read the systems\n");
    return 2;
  }
  const System* sys[3] = {&sa, &sa, &sb};
  std::vector<std::unique_ptr<HipCalcAGBNPForceKernel>> group, alone;
  for (int i = 0; i < 3; i++) {
    group.emplace_back(new HipCalcAGBNPForceKernel(0)), alone.emplace_back(new HipCalcAGBNPForceKernel(0));
    group.back()->initialize(make_force(*sys[i]));
    alone.back()->initialize(make_force(*sys[i]));
  }
  double worst = 0.0;
  for (int step = 0; step < 3; step++) {
    std::vector<std::vector<double>> pos(3), frc(3);
    for (int i = 0; i < 3; i++) {
      pos[i] = sys[i]->pos;
      for (size_t k = 0; k < pos[i].size(); k++) pos[i][k] += 1e-3 * std::sin(0.37 * k + 1.3 * step + i);  // small moves
      frc[i].assign(pos[i].size(), 0.0);
    }
    std::vector<HipCalcAGBNPForceKernel*> members = {group[0].get(), group[1].get(), group[2].get()};
    const std::vector<double> e = HipCalcAGBNPForceKernel::executeGroup(members, pos, frc);
    for (int i = 0; i < 3; i++) {
      std::vector<double> f(pos[i].size(), 0.0);
      const double e1 = alone[i]->execute(pos[i], f);
      worst = std::max(worst, std::fabs(e[i] - e1));
      for (size_t k = 0; k < f.size(); k++) worst = std::max(worst, std::fabs(frc[i][k] - f[k]));
    }
  }
  std::printf("replica group vs alone: max difference %.3e\n", worst);
  return worst < 1e-9 ? 0 : 1;
}
