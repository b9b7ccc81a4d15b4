// Energy-only evaluations through the plugin path: calcForcesAndEnergy(false, true) -- what OpenMM does for
// getState(getEnergy=True) without forces -- reaches HipCalcAGBNPForceKernel::execute with includeForces = false, which
// runs agbnp_hip_energy_openmm.  On a "HIP" context with shuffled, padded atoms: the energy equals the one of
// calcForcesAndEnergy(true, true) at the same positions (1e-9 relative) and the force buffer stays zero.  Reads the reference
// test's structure format on stdin; usage:  TestHipPlatformEnergyOnly <version> <double|mixed|single>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <random>
#include <vector>

#include "AGBNPForce.h"
#include "HipAGBNPKernels.h"
#include "openmm/Context.h"
#include "openmm/System.h"
#include "openmm/Vec3.h"
#include "openmm/hip/HipPlatform.h"

using namespace AGBNPPlugin;
using namespace OpenMM;

struct Double4 { double x, y, z, w; };
struct Float4 { float x, y, z, w; };

static void uploadPositions(HipContext& cu, const std::vector<Vec3>& pos, const std::vector<double>& charge) {
  const int padded = cu.getPaddedNumAtoms();
  const std::vector<int>& index = cu.getAtomIndex();
  if (cu.getUseDoublePrecision()) {
    std::vector<Double4> posq(padded, Double4{0, 0, 0, 0});
    for (int s = 0; s < cu.getNumAtoms(); s++) posq[s] = Double4{pos[index[s]][0], pos[index[s]][1], pos[index[s]][2], charge[index[s]]};
    cu.getPosq().upload(posq);
    return;
  }
  std::vector<Float4> posq(padded, Float4{0, 0, 0, 0}), corr(padded, Float4{0, 0, 0, 0});
  for (int s = 0; s < cu.getNumAtoms(); s++) {
    const Vec3& p = pos[index[s]];
    posq[s] = Float4{(float)p[0], (float)p[1], (float)p[2], (float)charge[index[s]]};
    corr[s] = Float4{(float)(p[0] - (double)posq[s].x), (float)(p[1] - (double)posq[s].y), (float)(p[2] - (double)posq[s].z), 0.f};
  }
  cu.getPosq().upload(posq);
  if (cu.getUseMixedPrecision()) cu.getPosqCorrection().upload(corr);
}

// energy and forces (particle order) of one evaluation, read the way OpenMM reads them from a GPU context (the force
// buffer is cleared first: after an energy-only evaluation it must still be zero)
static double evaluate(Context& context, HipContext& cu, std::vector<Vec3>& forces, bool includeForces) {
  std::vector<long long> zeros(3 * (size_t)cu.getPaddedNumAtoms(), 0);
  cu.getLongForceBuffer().upload(zeros);
  double energy = 0.0;
  if (cu.getUseDoublePrecision() || cu.getUseMixedPrecision()) {
    std::vector<double> e(cu.getEnergyBuffer().getSize(), 0.0);
    cu.getEnergyBuffer().upload(e);
    energy += context.getImpl().calcForcesAndEnergy(includeForces, true);
    (void)hipStreamSynchronize(cu.getCurrentStream());
    cu.getEnergyBuffer().download(e);
    for (double v : e) energy += v;
  } else {
    std::vector<float> e(cu.getEnergyBuffer().getSize(), 0.f);
    cu.getEnergyBuffer().upload(e);
    energy += context.getImpl().calcForcesAndEnergy(includeForces, true);
    (void)hipStreamSynchronize(cu.getCurrentStream());
    cu.getEnergyBuffer().download(e);
    for (float v : e) energy += v;
  }
  std::vector<long long> fixed;
  cu.getLongForceBuffer().download(fixed);
  const int padded = cu.getPaddedNumAtoms();
  const double scale = 1.0 / (double)0x100000000LL;
  forces.assign(cu.getNumAtoms(), Vec3());
  for (int s = 0; s < cu.getNumAtoms(); s++)
    forces[cu.getAtomIndex()[s]] = Vec3(scale * fixed[s], scale * fixed[s + padded], scale * fixed[s + 2 * padded]);
  return energy;
}

int main(int argc, char** argv) {
  try {
    const int version = argc > 1 ? atoi(argv[1]) : 1;
    const std::string precision = argc > 2 ? argv[2] : "double";
    int numParticles = 0;
    std::cin >> numParticles;
    System system;
    AGBNPForce* force = new AGBNPForce();
    force->setNonbondedMethod(AGBNPForce::NoCutoff);
    force->setCutoffDistance(1.0);
    force->setVersion(version);
    system.addForce(force);
    const double ang2nm = 0.1, kcalmol2kjmol = 4.184;
    const double sigmaw = 3.15365 * ang2nm, epsilonw = 0.155 * kcalmol2kjmol, rho = 0.033428 / pow(ang2nm, 3);
    const double epsilon_LJ = 0.155 * kcalmol2kjmol;
    std::vector<Vec3> positions;
    std::vector<double> charges;
    for (int i = 0; i < numParticles; i++) {
      double id, x, y, z, radius, charge, gamma;
      int ih;
      std::cin >> id >> x >> y >> z >> radius >> charge >> gamma >> ih;
      system.addParticle(1.0);
      positions.push_back(Vec3(x * ang2nm, y * ang2nm, z * ang2nm));
      charges.push_back(charge);
      radius *= ang2nm;
      gamma *= kcalmol2kjmol / (ang2nm * ang2nm);
      const double sij = sqrt(sigmaw * 2. * radius), eij = sqrt(epsilonw * epsilon_LJ);
      force->addParticle(radius, gamma, -16.0 * M_PI * rho * eij * pow(sij, 6) / 3.0, charge, ih > 0);
    }

    // the platform side: a "HIP" platform with one device context whose atoms are shuffled
    HipPlatform* platform = new HipPlatform();
    Platform::registerPlatform(platform);
    registerAGBNPHipKernelFactories();
    if (!platform->supportsKernels({CalcAGBNPForceKernel::Name()})) {
      std::cout << "FAIL: the HIP platform has no CalcAGBNPForce factory" << std::endl;
      return 1;
    }
    HipPlatform::PlatformData data;
    data.contexts.push_back(new HipContext(numParticles, 0, precision == "double", precision == "mixed"));
    HipContext& cu = *data.contexts[0];
    std::vector<int> order(cu.getPaddedNumAtoms());
    for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
    std::mt19937 rng(20261004);
    std::shuffle(order.begin(), order.begin() + numParticles, rng);
    cu.setAtomIndex(order);

    Context context(system, *platform, &data);
    uploadPositions(cu, positions, charges);
    std::vector<Vec3> forces;
    const double e_full = evaluate(context, cu, forces, true);
    std::vector<Vec3> none;
    const double e_only = evaluate(context, cu, none, false);
    positions[0][0] += 1e-3;  // a second geometry, energy-only first this time
    uploadPositions(cu, positions, charges);
    const double e_only2 = evaluate(context, cu, none, false);
    const double e_full2 = evaluate(context, cu, forces, true);
    double fmax = 0.0;
    for (const Vec3& f : none) fmax = std::max(fmax, std::max(fabs(f[0]), std::max(fabs(f[1]), fabs(f[2]))));
    std::cout.precision(12);
    std::cout << "Energy (forces and energy): " << e_full << " " << e_full2 << std::endl;
    std::cout << "Energy (energy only): " << e_only << " " << e_only2 << std::endl;
    std::cout << "Largest force after energy-only evaluations: " << fmax << std::endl;
    const double tol = precision == "single" ? 1e-6 : 1e-9;  // (single: the energy buffer is float)
    const bool ok = fabs(e_only - e_full) <= tol * fabs(e_full) && fabs(e_only2 - e_full2) <= tol * fabs(e_full2) && fmax == 0.0 &&
                    e_full != 0.0;
    std::cout << (ok ? "PASS" : "FAIL") << std::endl;
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << std::endl;
    return 2;
  }
}
