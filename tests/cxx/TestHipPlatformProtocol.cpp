// The glue's repeat protocol end to end (openmm_glue/HipAGBNPKernels.cpp, execute(): finish, and an evaluation that the engine
// withheld is enqueued again -- the reference invalidates the forces and retries the step, OpenCLAGBNPKernels.cpp:3613-3634):
// Context -> calcForcesAndEnergy on a sequence that MAKES it repeat.  Evaluation k runs on the positions of evaluation k - 1
// plus the lines of stage k of the steps file (tests/golden/protocol_steps.dat): the file's geometry; one heavy atom by 0.1 nm
// (a jump: the engine withholds that evaluation once); a small step; HipContext::setAtomIndex with another order, everything
// uploaded again, and a small step.  Reads the reference test's structure format on stdin; usage:
//   TestHipPlatformProtocol <double|mixed> <steps file>
// Prints, per evaluation, "evaluation k energy E", then "pos i x y z" (the positions the context holds: posq + correction) and
// "force i fx fy fz" in particle order, all %.17g: tests/test_openmm_glue.py compares every one of them with the oracle.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
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

// posq (+ correction) in the context's order; `seen`: what the context then holds, in particle order
static void uploadPositions(HipContext& cu, const std::vector<Vec3>& pos, const std::vector<double>& charge, std::vector<Vec3>& seen) {
  const int padded = cu.getPaddedNumAtoms();
  const std::vector<int>& index = cu.getAtomIndex();
  seen = pos;
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
    seen[index[s]] = Vec3((double)posq[s].x + (double)corr[s].x, (double)posq[s].y + (double)corr[s].y, (double)posq[s].z + (double)corr[s].z);
  }
  cu.getPosq().upload(posq);
  cu.getPosqCorrection().upload(corr);
}

// energy and forces (particle order) of one evaluation, read the way OpenMM reads them from a GPU context
static double evaluate(Context& context, HipContext& cu, std::vector<Vec3>& forces) {
  std::vector<long long> zeros(3 * (size_t)cu.getPaddedNumAtoms(), 0);
  cu.getLongForceBuffer().upload(zeros);
  std::vector<double> e(cu.getEnergyBuffer().getSize(), 0.0);
  cu.getEnergyBuffer().upload(e);
  double energy = context.getImpl().calcForcesAndEnergy(true, true);
  (void)hipStreamSynchronize(cu.getCurrentStream());
  cu.getEnergyBuffer().download(e);
  for (double v : e) energy += v;
  std::vector<long long> fixed;
  cu.getLongForceBuffer().download(fixed);
  const int padded = cu.getPaddedNumAtoms();
  const double scale = 1.0 / (double)0x100000000LL;
  forces.assign(cu.getNumAtoms(), Vec3());
  for (int s = 0; s < cu.getNumAtoms(); s++)
    forces[cu.getAtomIndex()[s]] = Vec3(scale * fixed[s], scale * fixed[s + padded], scale * fixed[s + 2 * padded]);
  return energy;
}

// a context's atom order without a random number: slot s holds particle (a s + b) mod n, a prime to n
static std::vector<int> affineOrder(int n, int padded, int a, int b) {
  std::vector<int> order(padded);
  for (int s = 0; s < padded; s++) order[s] = s < n ? (int)(((long long)a * s + b) % n) : s;
  return order;
}

static int coprimeFrom(int a, int n) {
  auto gcd = [](int x, int y) {
    while (y) {
      const int t = x % y;
      x = y, y = t;
    }
    return x;
  };
  while (gcd(a, n) != 1) a++;
  return a;
}

int main(int argc, char** argv) {
  try {
    const std::string precision = argc > 1 ? argv[1] : "double";
    if (argc < 3 || (precision != "double" && precision != "mixed")) {
      std::cout << "usage: TestHipPlatformProtocol <double|mixed> <steps file>" << std::endl;
      return 1;
    }
    struct Move { int stage, atom; double d[3]; };
    std::vector<Move> moves;
    {
      std::ifstream in(argv[2]);
      if (!in) throw OpenMMException("cannot read the steps file");
      std::string line;
      while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        Move m;
        if (ss >> m.stage >> m.atom >> m.d[0] >> m.d[1] >> m.d[2]) moves.push_back(m);
      }
    }
    int numParticles = 0;
    std::cin >> numParticles;
    System system;
    AGBNPForce* force = new AGBNPForce();
    force->setNonbondedMethod(AGBNPForce::NoCutoff);
    force->setCutoffDistance(1.0);
    force->setVersion(1);
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
    for (const Move& m : moves)
      if (m.atom < 0 || m.atom >= numParticles || m.stage < 1 || m.stage > 3) throw OpenMMException("the steps file names an atom or a stage that does not exist");

    HipPlatform* platform = new HipPlatform();
    Platform::registerPlatform(platform);
    registerAGBNPHipKernelFactories();
    HipPlatform::PlatformData data;
    data.contexts.push_back(new HipContext(numParticles, 0, precision == "double", precision == "mixed"));
    HipContext& cu = *data.contexts[0];
    cu.setAtomIndex(affineOrder(numParticles, cu.getPaddedNumAtoms(), coprimeFrom(41, numParticles), 7));
    Context context(system, *platform, &data);

    std::vector<Vec3> forces, seen;
    for (int k = 0; k <= 3; k++) {
      for (const Move& m : moves)
        if (m.stage == k)
          for (int d = 0; d < 3; d++) positions[m.atom][d] += m.d[d];
      if (k == 3)  // the real context does this in reorderAtoms(): same arrays, new contents
        cu.setAtomIndex(affineOrder(numParticles, cu.getPaddedNumAtoms(), coprimeFrom(101, numParticles), 19));
      uploadPositions(cu, positions, charges, seen);
      const double energy = evaluate(context, cu, forces);
      printf("evaluation %d energy %.17g\n", k, energy);
      for (int i = 0; i < numParticles; i++) printf("pos %d %.17g %.17g %.17g\n", i, seen[i][0], seen[i][1], seen[i][2]);
      for (int i = 0; i < numParticles; i++) printf("force %d %.17g %.17g %.17g\n", i, forces[i][0], forces[i][1], forces[i][2]);
    }
    return 0;
  } catch (const std::exception& e) {
    std::cout << "exception: " << e.what() << std::endl;
    return 2;
  }
}
