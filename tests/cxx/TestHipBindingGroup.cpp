// Binding groups through the C++ mirror (cpp/AGBNPForce.h, AGBNPPlugin::executeBindingGroup / energyBindingGroup): four bindings
// of one complex (the first `nligand` atoms the ligand) at lambda = 0, 0.35, 1, 1.5 in one call must give what each binding gives
// alone through Binding::execute(), the energy form the same scalars, and a count of 0 or 17 an OpenMMException.
// Built and run by tests/test_gpu_binding_group.py (on the GPU box), compiled for syntax by tests/test_lambda_exchange_api.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <vector>

#include "../../cpp/AGBNPForce.h"

using namespace AGBNPPlugin;

namespace {
// whitespace table: radius gamma alpha charge ishydrogen x y z per line (written by the driving test)
bool read_system(const char* path, AGBNPForce& f, std::vector<double>& pos) {
  std::ifstream in(path);
  if (!in) return false;
  double r, g, a, q, x, y, z, h;
  f.setVersion(1);
  while (in >> r >> g >> a >> q >> h >> x >> y >> z) {
    f.addParticle(r, g, a, q, h != 0.0);
    pos.push_back(x), pos.push_back(y), pos.push_back(z);
  }
  return !pos.empty();
}

template <typename F>
bool throws(F call) {
  try {
    call();
  } catch (const OpenMMException&) {
    return true;
  }
  return false;
}
}  // namespace

int main(int argc, char** argv) {
  AGBNPForce force;
  std::vector<double> pos;
  if (argc < 3 || !read_system(argv[1], force, pos)) {
    std::fprintf(stderr, "usage: TestHipBindingGroup SYSTEM.txt NLIGAND\n");
    return 2;
  }
  const size_t n3 = pos.size();
  const int nl = std::atoi(argv[2]);
  try {
    std::vector<int> ligand(nl);
    for (int i = 0; i < nl; i++) ligand[i] = i;
    const std::vector<double> lambdas = {0.0, 0.35, 1.0, 1.5};
    const size_t K = lambdas.size();
    std::vector<std::unique_ptr<Binding>> own;
    std::vector<Binding*> bindings;
    for (size_t k = 0; k < K; k++) {
      own.emplace_back(new Binding(force, ligand));
      bindings.push_back(own.back().get());
    }
    // every binding alone
    std::vector<std::vector<double>> f_alone(K, std::vector<double>(n3, 0.0));
    std::vector<double> e_alone(K), u_alone(K);
    for (size_t k = 0; k < K; k++) e_alone[k] = bindings[k]->execute(pos, lambdas[k], f_alone[k], u_alone[k]);
    // all of them in one call, into forces that hold 1.0 already
    std::vector<std::vector<double>> positions(K, pos), f(K, std::vector<double>(n3, 1.0));
    std::vector<double> u, u_only;
    const std::vector<double> e = executeBindingGroup(bindings, positions, lambdas, f, u);
    const std::vector<double> e_only = energyBindingGroup(bindings, positions, lambdas, u_only);
    bool ok = e.size() == K && u.size() == K && e_only.size() == K && u_only.size() == K;
    for (size_t k = 0; k < K && ok; k++) {
      double worst = 0.0;
      for (size_t i = 0; i < n3; i++) worst = std::fmax(worst, std::fabs(f[k][i] - 1.0 - f_alone[k][i]));
      const double scale = std::fmax(1.0, 1e-3 * std::fabs(e_alone[k]));
      std::printf("lambda %.2f  E_lambda %.9f (alone %.9f, energy form %.9f)  u %.9f (alone %.9f)  worst force difference %.3e\n", lambdas[k],
                  e[k], e_alone[k], e_only[k], u[k], u_alone[k], worst);
      ok = ok && worst < 1e-9 && std::fabs(e[k] - e_alone[k]) < 1e-9 * scale && std::fabs(u[k] - u_alone[k]) < 1e-9 * scale;
      ok = ok && std::fabs(e_only[k] - e[k]) < 1e-9 * scale && std::fabs(u_only[k] - u[k]) < 1e-9 * scale;
      ok = ok && bindings[k]->finish() == 0 && bindings[k]->withheld().empty();
    }
    ok = ok && std::fabs(u[0] - u[3]) < 1e-9 * std::fmax(1.0, std::fabs(u[0]));  // (u does not depend on lambda)
    // the counts outside 1 .. 16, and lists that do not match
    std::vector<Binding*> none, many(17, bindings[0]);
    std::vector<std::vector<double>> p17(17, pos), f17(17, std::vector<double>(n3, 0.0)), p0, f0;
    std::vector<double> l17(17, 0.5), l0, scratch;
    ok = ok && throws([&] { executeBindingGroup(none, p0, l0, f0, scratch); }) && throws([&] { executeBindingGroup(many, p17, l17, f17, scratch); });
    ok = ok && throws([&] { energyBindingGroup(none, p0, l0, scratch); }) && throws([&] { energyBindingGroup(many, p17, l17, scratch); });
    ok = ok && throws([&] { energyBindingGroup(bindings, positions, l17, scratch); });
    std::vector<Binding*> twice = {bindings[0], bindings[0]};
    std::vector<std::vector<double>> p2(2, pos);
    const std::vector<double> l2 = {0.0, 1.0};
    ok = ok && throws([&] { energyBindingGroup(twice, p2, l2, scratch); });  // (the library's refusal)
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
  } catch (const OpenMMException& ex) {
    std::fprintf(stderr, "OpenMMException: %s\n", ex.what());
    return 1;
  }
}
