// C++ host-side mirror of the reference's API class and kernel interface, on top of the C ABI
// (include/agbnp_hip.h).  Header-only; link against openmm_agbnp_plugin_amd/libagbnp_hip.so.
//
//   AGBNPPlugin::AGBNPForce            <-> openmmapi/include/AGBNPForce.h:39-155, openmmapi/src/AGBNPForce.cpp:15-78
//   AGBNPPlugin::HipCalcAGBNPForceKernel <-> CalcAGBNPForceKernel, openmmapi/include/AGBNPKernels.h:19-47
//
// Same method names, argument order and meaning, defaults and error behaviour (exceptions with the
// reference's messages).  OpenMM types are replaced by plain containers because OpenMM is not part of this
// path: positions / forces are std::vector<double> of 3N values (x0,y0,z0,x1,...), nm and kJ/mol/nm.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/agbnp_hip.h"

namespace AGBNPPlugin {

// stands in for OpenMM::OpenMMException
class OpenMMException : public std::runtime_error {
 public:
  explicit OpenMMException(const std::string& msg) : std::runtime_error(msg) {}
};

class AGBNPForce {
 public:
  enum NonbondedMethod { NoCutoff = 0, CutoffNonPeriodic = 1, CutoffPeriodic = 2 };

  // defaults of the reference constructor (AGBNPForce.cpp:15)
  AGBNPForce() : nonbondedMethod(NoCutoff), cutoffDistance(1.0), version(1), solvent_radius(1.0 * (0.1f)) {}

  int addParticle(double radius, double gamma, double vdw_alpha, double charge, bool ishydrogen) {
    particles.push_back(ParticleInfo{radius, gamma, vdw_alpha, charge, ishydrogen});
    return (int)particles.size() - 1;
  }
  void setParticleParameters(int index, double radius, double gamma, double vdw_alpha, double charge, bool ishydrogen) {
    checkIndex(index);
    particles[index] = ParticleInfo{radius, gamma, vdw_alpha, charge, ishydrogen};
  }
  void getParticleParameters(int index, double& radius, double& gamma, double& vdw_alpha, double& charge, bool& ishydrogen) const {
    checkIndex(index);
    const ParticleInfo& p = particles[index];
    radius = p.radius;
    gamma = p.gamma;
    vdw_alpha = p.vdw_alpha;
    charge = p.charge;
    ishydrogen = p.ishydrogen;
  }
  int getNumParticles() const { return (int)particles.size(); }
  NonbondedMethod getNonbondedMethod() const { return nonbondedMethod; }
  void setNonbondedMethod(NonbondedMethod method) { nonbondedMethod = method; }
  double getCutoffDistance() const { return cutoffDistance; }
  void setCutoffDistance(double distance) { cutoffDistance = distance; }
  double getSolventRadius() const { return solvent_radius; }
  void setVersion(int agbnp_version) {  // 0 = GVolSA, 1 = AGBNP1, 2 = AGBNP2 (AGBNPForce.cpp:52-59)
    if (agbnp_version >= 0 && agbnp_version <= 2)
      version = (unsigned)agbnp_version;
    else
      throw OpenMMException("AGBNPForce::setVersion(): illegal version number");
  }
  unsigned int getVersion() const { return version; }

 private:
  struct ParticleInfo {
    double radius, gamma, vdw_alpha, charge;
    bool ishydrogen;
  };
  void checkIndex(int index) const {
    if (index < 0 || index >= (int)particles.size()) throw OpenMMException("Assertion failure: Index out of range");
  }
  std::vector<ParticleInfo> particles;
  NonbondedMethod nonbondedMethod;
  double cutoffDistance;
  unsigned int version;
  double solvent_radius;
};

class Binding;

// The "HIP platform" implementation of the plugin's kernel interface.
class HipCalcAGBNPForceKernel {
 public:
  static std::string Name() { return "CalcAGBNPForce"; }
  explicit HipCalcAGBNPForceKernel(int device = 0) : ctx(nullptr), device(device), numParticles(0) {}
  ~HipCalcAGBNPForceKernel() { agbnp_hip_destroy(ctx); }
  HipCalcAGBNPForceKernel(const HipCalcAGBNPForceKernel&) = delete;
  HipCalcAGBNPForceKernel& operator=(const HipCalcAGBNPForceKernel&) = delete;

  void initialize(const AGBNPForce& force) {
    agbnp_hip_destroy(ctx);
    ctx = nullptr;
    std::vector<double> r, g, a, q;
    std::vector<int> h;
    gather(force, r, g, a, q, h);
    numParticles = (int)r.size();
    if (agbnp_hip_create(&ctx, numParticles, r.data(), g.data(), a.data(), q.data(), h.data(), (int)force.getVersion(),
                         (int)force.getNonbondedMethod(), force.getCutoffDistance(), device) != AGBNP_HIP_OK)
      throw OpenMMException(agbnp_hip_last_error(nullptr));
  }

  // CPU-platform data convention of the reference (ReferenceAGBNPKernels.cpp:27-35,197,794): forces are
  // accumulated into `forces`, the energy is returned; the two flags are accepted and ignored.
  double execute(const std::vector<double>& positions, std::vector<double>& forces, bool includeForces = true,
                 bool includeEnergy = true) {
    (void)includeForces;
    (void)includeEnergy;
    if (!ctx) throw OpenMMException("HipCalcAGBNPForceKernel: initialize() has not been called");
    if ((int)positions.size() != 3 * numParticles || (int)forces.size() != 3 * numParticles)
      throw OpenMMException("execute(): positions and forces must hold 3N values");
    double energy = 0.0;
    if (agbnp_hip_execute_host(ctx, positions.data(), forces.data(), &energy) != AGBNP_HIP_OK)
      throw OpenMMException(agbnp_hip_last_error(ctx));
    return energy;
  }

  // Energy-only evaluation (what OpenMM asks for with includeForces = false): the energy execute() would return at these
  // positions, without the force passes where the context allows it; no forces are written (include/agbnp_hip.h).
  double energy(const std::vector<double>& positions) {
    if (!ctx) throw OpenMMException("HipCalcAGBNPForceKernel: initialize() has not been called");
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("energy(): positions must hold 3N values");
    double e = 0.0;
    if (agbnp_hip_energy_host(ctx, positions.data(), &e) != AGBNP_HIP_OK) throw OpenMMException(agbnp_hip_last_error(ctx));
    return e;
  }

  // Per-atom decomposition of the energy at these positions (agbnp_hip_decompose_host): returns the energy; `terms` receives
  // AGBNP_HIP_DECOMPOSITION_TERMS planes of N doubles -- cavity, vdW, GB self, GB pair (each pair shared half and half) -- whose
  // sum over everything is the energy.  Version 0 has the cavity plane only.  No forces are written.
  double decompose(const std::vector<double>& positions, std::vector<double>& terms) {
    if (!ctx) throw OpenMMException("HipCalcAGBNPForceKernel: initialize() has not been called");
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("decompose(): positions must hold 3N values");
    terms.assign((size_t)AGBNP_HIP_DECOMPOSITION_TERMS * numParticles, 0.0);
    double e = 0.0;
    if (agbnp_hip_decompose_host(ctx, positions.data(), terms.data(), &e) != AGBNP_HIP_OK)
      throw OpenMMException(agbnp_hip_last_error(ctx));
    return e;
  }

  // Replica groups (agbnp_hip_execute_group_host): one evaluation of every kernel in `kernels`, the launches of the members
  // that can share them made once for all; positions[i] (3N_i) read, forces[i] accumulated, the members' energies returned.
  static std::vector<double> executeGroup(const std::vector<HipCalcAGBNPForceKernel*>& kernels,
                                          const std::vector<std::vector<double>>& positions, std::vector<std::vector<double>>& forces) {
    const size_t n = kernels.size();
    if (n < 1 || n > AGBNP_HIP_MAX_GROUP) throw OpenMMException("executeGroup(): a group has 1 to 16 members");
    if (positions.size() != n || forces.size() != n) throw OpenMMException("executeGroup(): one position and one force array per member");
    std::vector<agbnp_hip_context*> ctxs(n);
    std::vector<const double*> pos(n);
    std::vector<double*> frc(n);
    for (size_t i = 0; i < n; i++) {
      if (!kernels[i] || !kernels[i]->ctx) throw OpenMMException("HipCalcAGBNPForceKernel: initialize() has not been called");
      const size_t n3 = 3 * (size_t)kernels[i]->numParticles;
      if (positions[i].size() != n3 || forces[i].size() != n3) throw OpenMMException("executeGroup(): arrays must hold 3N values");
      ctxs[i] = kernels[i]->ctx, pos[i] = positions[i].data(), frc[i] = forces[i].data();
    }
    std::vector<double> energies(n, 0.0);
    if (agbnp_hip_execute_group_host(ctxs.data(), (int)n, pos.data(), frc.data(), energies.data()) != AGBNP_HIP_OK)
      throw OpenMMException(agbnp_hip_last_error(ctxs[0]));
    return energies;
  }

  // Energy-only replica groups (agbnp_hip_energy_group_host): the energy of every kernel in `kernels` at positions[i] (3N_i),
  // on shared energy-only launches where the members allow it; no force is written anywhere.
  static std::vector<double> energyGroup(const std::vector<HipCalcAGBNPForceKernel*>& kernels,
                                         const std::vector<std::vector<double>>& positions) {
    const size_t n = kernels.size();
    if (n < 1 || n > AGBNP_HIP_MAX_GROUP) throw OpenMMException("energyGroup(): a group has 1 to 16 members");
    if (positions.size() != n) throw OpenMMException("energyGroup(): one position array per member");
    std::vector<agbnp_hip_context*> ctxs(n);
    std::vector<const double*> pos(n);
    for (size_t i = 0; i < n; i++) {
      if (!kernels[i] || !kernels[i]->ctx) throw OpenMMException("HipCalcAGBNPForceKernel: initialize() has not been called");
      if (positions[i].size() != 3 * (size_t)kernels[i]->numParticles) throw OpenMMException("energyGroup(): arrays must hold 3N values");
      ctxs[i] = kernels[i]->ctx, pos[i] = positions[i].data();
    }
    std::vector<double> energies(n, 0.0);
    if (agbnp_hip_energy_group_host(ctxs.data(), (int)n, pos.data(), energies.data()) != AGBNP_HIP_OK)
      throw OpenMMException(agbnp_hip_last_error(ctxs[0]));
    return energies;
  }

  // The positions of the next evaluation are unrelated to the last ones (agbnp_hip_expect_jump): it lays the neighbour masks
  // down at its own positions first and is not withheld for the jump.
  void expectJump() {
    if (!ctx) throw OpenMMException("HipCalcAGBNPForceKernel: initialize() has not been called");
    if (agbnp_hip_expect_jump(ctx) != AGBNP_HIP_OK) throw OpenMMException(agbnp_hip_last_error(ctx));
  }

  void copyParametersToContext(const AGBNPForce& force) {
    if (!ctx) throw OpenMMException("HipCalcAGBNPForceKernel: initialize() has not been called");
    std::vector<double> r, g, a, q;
    std::vector<int> h;
    gather(force, r, g, a, q, h);
    if (agbnp_hip_update_parameters(ctx, (int)r.size(), r.data(), g.data(), a.data(), q.data(), h.data()) != AGBNP_HIP_OK)
      throw OpenMMException(agbnp_hip_last_error(ctx));
  }

  agbnp_hip_context* handle() const { return ctx; }

 private:
  friend class Binding;
  static void gather(const AGBNPForce& force, std::vector<double>& r, std::vector<double>& g, std::vector<double>& a,
                     std::vector<double>& q, std::vector<int>& h) {
    const int n = force.getNumParticles();
    r.resize(n), g.resize(n), a.resize(n), q.resize(n), h.resize(n);
    for (int i = 0; i < n; i++) {
      bool ish;
      force.getParticleParameters(i, r[i], g[i], a[i], q[i], ish);
      h[i] = ish ? 1 : 0;
    }
  }
  agbnp_hip_context* ctx;
  int device;
  int numParticles;
};

// Binding-energy evaluations (agbnp_hip_binding_*): the complex, its receptor and its ligand in one call.  `force` holds the
// particles of the complex, `ligandAtoms` 1 to N - 1 distinct atom indices in any order; the rest is the receptor.  With E_RL,
// E_R, E_L the three systems' energies at the complex's positions: u = E_RL - E_R - E_L, E_lambda = E_R + E_L + lambda u,
// F_lambda = lambda F^RL + (1 - lambda) F^{R|L}.  A binding evaluation reaches the caller's buffers only if all three members'
// evaluations completed.  Do not evaluate or finish a member() directly between two finish() calls.
class Binding {
 public:
  enum Member { Complex = 0, Receptor = 1, Ligand = 2 };
  Binding(const AGBNPForce& force, const std::vector<int>& ligandAtoms, int device = 0, int mode = AGBNP_HIP_MODE_REFERENCE)
      : b(nullptr), numParticles(force.getNumParticles()) {
    std::vector<double> r, g, a, q;
    std::vector<int> h;
    HipCalcAGBNPForceKernel::gather(force, r, g, a, q, h);
    if (agbnp_hip_binding_create(&b, numParticles, r.data(), g.data(), a.data(), q.data(), h.data(), ligandAtoms.data(),
                                 (int)ligandAtoms.size(), (int)force.getVersion(), (int)force.getNonbondedMethod(),
                                 force.getCutoffDistance(), device) != AGBNP_HIP_OK)
      throw OpenMMException(agbnp_hip_last_error(nullptr));
    if (mode != AGBNP_HIP_MODE_REFERENCE) setMode(mode);
  }
  ~Binding() { agbnp_hip_binding_destroy(b); }
  Binding(const Binding&) = delete;
  Binding& operator=(const Binding&) = delete;

  // forces (3N) are accumulated, E_lambda is returned, u goes to `bindingEnergy`; withheld evaluations are repeated inside
  double execute(const std::vector<double>& positions, double lambda, std::vector<double>& forces, double& bindingEnergy) {
    if ((int)positions.size() != 3 * numParticles || (int)forces.size() != 3 * numParticles)
      throw OpenMMException("Binding::execute(): positions and forces must hold 3N values");
    double e = 0.0;
    check(agbnp_hip_binding_execute_host(b, positions.data(), lambda, forces.data(), &e, &bindingEnergy));
    return e;
  }
  // the same without forces: three energy-only evaluations
  double energy(const std::vector<double>& positions, double lambda, double& bindingEnergy) {
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("Binding::energy(): positions must hold 3N values");
    double e = 0.0;
    check(agbnp_hip_binding_energy_host(b, positions.data(), lambda, &e, &bindingEnergy));
    return e;
  }
  // device pointers: F_lambda, E_lambda and u are ADDED -- all of them or, if a member is withheld, nothing; asynchronous
  void executeDevice(const double* dPositions, double lambda, double* dForces, double* dEnergy, double* dBindingEnergy,
                     void* stream = nullptr) {
    check(agbnp_hip_binding_execute_device(b, dPositions, lambda, dForces, dEnergy, dBindingEnergy, stream));
  }
  void energyDevice(const double* dPositions, double lambda, double* dEnergy, double* dBindingEnergy, void* stream = nullptr) {
    check(agbnp_hip_binding_energy_device(b, dPositions, lambda, dEnergy, dBindingEnergy, stream));
  }
  // binding evaluations since the previous finish() with at least one withheld member: run those again
  int finish(void* stream = nullptr) {
    int repeat = 0;
    check(agbnp_hip_binding_finish(b, stream, &repeat));
    return repeat;
  }
  std::vector<int> withheld() const {
    const int n = agbnp_hip_binding_withheld_evaluations(b, nullptr, 0);
    std::vector<int> idx(n > 0 ? n : 0, -1);
    agbnp_hip_binding_withheld_evaluations(b, idx.data(), (int)idx.size());
    while (!idx.empty() && idx.back() < 0) idx.pop_back();  // (beyond the log's bitmap evaluations are only counted)
    return idx;
  }
  void expectJump() { check(agbnp_hip_binding_expect_jump(b)); }
  void setMode(int mode) { check(agbnp_hip_binding_set_mode(b, mode)); }
  // `force` holds the parameters of the COMPLEX; every member gets its subset
  void copyParametersToContext(const AGBNPForce& force) {
    std::vector<double> r, g, a, q;
    std::vector<int> h;
    HipCalcAGBNPForceKernel::gather(force, r, g, a, q, h);
    check(agbnp_hip_binding_update_parameters(b, (int)r.size(), r.data(), g.data(), a.data(), q.data(), h.data()));
  }
  // a member's context, for scalars, vectors, poll and wait_verdict; the binding owns it
  agbnp_hip_context* member(Member which) const { return agbnp_hip_binding_member(b, (int)which); }
  agbnp_hip_binding* handle() const { return b; }
  int getNumParticles() const { return numParticles; }

 private:
  static void check(int rc) {
    if (rc != AGBNP_HIP_OK) throw OpenMMException(agbnp_hip_last_error(nullptr));
  }
  agbnp_hip_binding* b;
  int numParticles;
};

// Binding groups (agbnp_hip_binding_execute_group_host): one evaluation of every binding in `bindings` at its own lambda -- one
// gather launch, the members' evaluations as replica groups, one combine launch.  positions[k] (3N_k) read, forces[k]
// accumulated, E_lambda of every binding returned, u in `bindingEnergies`.  A binding whose evaluation was withheld is repeated
// inside.
inline std::vector<double> executeBindingGroup(const std::vector<Binding*>& bindings, const std::vector<std::vector<double>>& positions,
                                               const std::vector<double>& lambdas, std::vector<std::vector<double>>& forces,
                                               std::vector<double>& bindingEnergies) {
  const size_t n = bindings.size();
  if (n < 1 || n > AGBNP_HIP_MAX_BINDING_GROUP) throw OpenMMException("executeBindingGroup(): a binding group has 1 to 16 bindings");
  if (positions.size() != n || forces.size() != n || lambdas.size() != n)
    throw OpenMMException("executeBindingGroup(): one position array, one force array and one lambda per binding");
  std::vector<agbnp_hip_binding*> bs(n);
  std::vector<const double*> pos(n);
  std::vector<double*> frc(n);
  for (size_t i = 0; i < n; i++) {
    if (!bindings[i]) throw OpenMMException("executeBindingGroup(): null binding");
    const size_t n3 = 3 * (size_t)bindings[i]->getNumParticles();
    if (positions[i].size() != n3 || forces[i].size() != n3) throw OpenMMException("executeBindingGroup(): arrays must hold 3N values");
    bs[i] = bindings[i]->handle(), pos[i] = positions[i].data(), frc[i] = forces[i].data();
  }
  std::vector<double> energies(n, 0.0);
  bindingEnergies.assign(n, 0.0);
  if (agbnp_hip_binding_execute_group_host(bs.data(), (int)n, pos.data(), lambdas.data(), frc.data(), energies.data(),
                                           bindingEnergies.data()) != AGBNP_HIP_OK)
    throw OpenMMException(agbnp_hip_last_error(nullptr));
  return energies;
}

// The same without forces (agbnp_hip_binding_energy_group_host): no force is written anywhere.
inline std::vector<double> energyBindingGroup(const std::vector<Binding*>& bindings, const std::vector<std::vector<double>>& positions,
                                              const std::vector<double>& lambdas, std::vector<double>& bindingEnergies) {
  const size_t n = bindings.size();
  if (n < 1 || n > AGBNP_HIP_MAX_BINDING_GROUP) throw OpenMMException("energyBindingGroup(): a binding group has 1 to 16 bindings");
  if (positions.size() != n || lambdas.size() != n) throw OpenMMException("energyBindingGroup(): one position array and one lambda per binding");
  std::vector<agbnp_hip_binding*> bs(n);
  std::vector<const double*> pos(n);
  for (size_t i = 0; i < n; i++) {
    if (!bindings[i]) throw OpenMMException("energyBindingGroup(): null binding");
    if (positions[i].size() != 3 * (size_t)bindings[i]->getNumParticles()) throw OpenMMException("energyBindingGroup(): arrays must hold 3N values");
    bs[i] = bindings[i]->handle(), pos[i] = positions[i].data();
  }
  std::vector<double> energies(n, 0.0);
  bindingEnergies.assign(n, 0.0);
  if (agbnp_hip_binding_energy_group_host(bs.data(), (int)n, pos.data(), lambdas.data(), energies.data(), bindingEnergies.data()) != AGBNP_HIP_OK)
    throw OpenMMException(agbnp_hip_last_error(nullptr));
  return energies;
}

}  // namespace AGBNPPlugin
