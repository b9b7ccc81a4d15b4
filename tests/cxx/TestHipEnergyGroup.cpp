// Energy-only replica groups and the jump hint through the C++ mirror (cpp/AGBNPForce.h, HipCalcAGBNPForceKernel::energyGroup /
// expectJump): three contexts -- two of one system, one of another -- evaluated in one call; each must agree with the same
// context's own energy() at the same positions.  Then a far geometry behind expectJump(): the first evaluation is complete.
// Built and run by tests/test_gpu_energy_group.py (on the GPU box), compiled for syntax by tests/test_energy_group_api.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

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
  std::vector<HipCalcAGBNPForceKernel*> members = {group[0].get(), group[1].get(), group[2].get()};
  for (int step = 0; step < 3; step++) {
    std::vector<std::vector<double>> pos(3);
    for (int i = 0; i < 3; i++) {
      pos[i] = sys[i]->pos;
      for (size_t k = 0; k < pos[i].size(); k++) pos[i][k] += 1e-3 * std::sin(0.37 * k + 1.3 * step + i);  // small moves
    }
    const std::vector<double> e = HipCalcAGBNPForceKernel::energyGroup(members, pos);
    for (int i = 0; i < 3; i++) worst = std::max(worst, std::fabs(e[i] - alone[i]->energy(pos[i])));
  }
  std::printf("energy group vs alone: max difference %.3e\n", worst);
  if (!(worst < 1e-9)) return 1;

  // a far geometry (every atom 0.1 nm away) behind the hint: the first evaluation on the device is complete
  std::vector<double> far = sa.pos;
  for (size_t k = 0; k < far.size(); k += 3) far[k] += 0.1;
  const double reference = alone[0]->energy(far);  // (repeats a withheld evaluation inside)
  agbnp_hip_context* ctx = group[0]->handle();
  double *d_pos = nullptr, *d_energy = nullptr, e_far = 0.0;
  int withheld = -1;
  if (hipMalloc(reinterpret_cast<void**>(&d_pos), sizeof(double) * far.size()) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&d_energy), sizeof(double)) != hipSuccess)
    return 2;
  if (hipMemcpy(d_pos, far.data(), sizeof(double) * far.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_energy, 0, sizeof(double)) != hipSuccess)
    return 2;
  group[0]->expectJump();
  if (agbnp_hip_energy_device(ctx, d_pos, d_energy, nullptr) != AGBNP_HIP_OK || agbnp_hip_finish(ctx, nullptr, &withheld) != AGBNP_HIP_OK)
    return 2;
  if (hipMemcpy(&e_far, d_energy, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 2;
  (void)hipFree(d_pos);
  (void)hipFree(d_energy);
  std::printf("expectJump: withheld %d, difference %.3e\n", withheld, std::fabs(e_far - reference));
  return withheld == 0 && std::fabs(e_far - reference) < 1e-9 ? 0 : 1;
}
