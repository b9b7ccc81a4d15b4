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

// What the classes below share (not part of the mirrored interface).
namespace detail {

// a return code of the library: a failure throws with the message the library keeps for `ctx` (null: the message of the calls
// that are not made on a context)
inline void check(int rc, agbnp_hip_context* ctx = nullptr) {
  if (rc != AGBNP_HIP_OK) throw OpenMMException(agbnp_hip_last_error(ctx));
}

// the particle parameters of a force as they cross the C ABI
struct Parameters {
  std::vector<double> r, g, a, q;
  std::vector<int> h;
  int n() const { return (int)r.size(); }
};
inline Parameters gather(const AGBNPForce& force) {
  Parameters p;
  const int n = force.getNumParticles();
  p.r.resize(n), p.g.resize(n), p.a.resize(n), p.q.resize(n), p.h.resize(n);
  for (int i = 0; i < n; i++) {
    bool ish;
    force.getParticleParameters(i, p.r[i], p.g[i], p.a[i], p.q[i], ish);
    p.h[i] = ish ? 1 : 0;
  }
  return p;
}

// A partition as both setAtomSets() check it before the library is touched (`who`: the method's name, for the messages): one
// index per atom, 0 .. numSets - 1; returns numSets, a negative one resolved to the largest index + 1
inline int checkAtomSets(const std::string& who, const std::vector<int>& sets, int numParticles, int numSets) {
  if ((int)sets.size() != numParticles) throw OpenMMException(who + "(): one set index per atom is needed");
  int lowest = 0, highest = -1;
  for (int s : sets) lowest = s < lowest ? s : lowest, highest = s > highest ? s : highest;
  if (numSets < 0) numSets = highest + 1;
  if (numSets < 1 || numSets > AGBNP_HIP_MAX_SETS) throw OpenMMException(who + "(): numSets must be 1 .. AGBNP_HIP_MAX_SETS");
  if (lowest < 0 || highest >= numSets) throw OpenMMException(who + "(): every set index must be 0 .. numSets - 1");
  return numSets;
}

// The arrays of a group call: the members' handles, their positions and, where `forces` is given, their forces.  `bound` and
// `each` are the refusals of a wrong member count and of per-member arguments that are not one per member (`counted`: what the
// caller has counted itself).  A member class names its handle type, its bound and its particle count, and hands out a member's
// handle or throws (groupHandle).
struct Group {
  template <class Member>
  struct Arrays {
    std::vector<typename Member::Handle*> handles;
    std::vector<const double*> pos;
    std::vector<double*> frc;
  };
  template <class Member>
  static Arrays<Member> collect(const std::string& who, const std::vector<Member*>& members, const char* bound, const char* each,
                                bool counted, const std::vector<std::vector<double>>& positions,
                                std::vector<std::vector<double>>* forces = nullptr) {
    const size_t n = members.size();
    if (n < 1 || n > Member::maxGroup) throw OpenMMException(who + "(): " + bound);
    if (positions.size() != n || (forces && forces->size() != n) || !counted) throw OpenMMException(who + "(): " + each);
    Arrays<Member> g;
    g.handles.resize(n), g.pos.resize(n), g.frc.resize(forces ? n : 0);
    for (size_t i = 0; i < n; i++) {
      g.handles[i] = Member::groupHandle(members[i], who);
      const size_t n3 = 3 * (size_t)members[i]->numParticles;
      if (positions[i].size() != n3 || (forces && (*forces)[i].size() != n3)) throw OpenMMException(who + "(): arrays must hold 3N values");
      g.pos[i] = positions[i].data();
      if (forces) g.frc[i] = (*forces)[i].data();
    }
    return g;
  }
};

}  // namespace detail

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
    const detail::Parameters p = detail::gather(force);
    numParticles = p.n();
    detail::check(agbnp_hip_create(&ctx, p.n(), p.r.data(), p.g.data(), p.a.data(), p.q.data(), p.h.data(), (int)force.getVersion(),
                                   (int)force.getNonbondedMethod(), force.getCutoffDistance(), device));
  }

  // CPU-platform data convention of the reference (ReferenceAGBNPKernels.cpp:27-35,197,794): forces are
  // accumulated into `forces`, the energy is returned; the two flags are accepted and ignored.
  double execute(const std::vector<double>& positions, std::vector<double>& forces, bool includeForces = true,
                 bool includeEnergy = true) {
    (void)includeForces;
    (void)includeEnergy;
    need();
    if ((int)positions.size() != 3 * numParticles || (int)forces.size() != 3 * numParticles)
      throw OpenMMException("execute(): positions and forces must hold 3N values");
    double energy = 0.0;
    check(agbnp_hip_execute_host(ctx, positions.data(), forces.data(), &energy));
    return energy;
  }

  // Energy-only evaluation (what OpenMM asks for with includeForces = false): the energy execute() would return at these
  // positions, without the force passes where the context allows it; no forces are written (include/agbnp_hip.h).
  double energy(const std::vector<double>& positions) {
    need();
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("energy(): positions must hold 3N values");
    double e = 0.0;
    check(agbnp_hip_energy_host(ctx, positions.data(), &e));
    return e;
  }

  // Per-atom decomposition of the energy at these positions (agbnp_hip_decompose_host): returns the energy; `terms` receives
  // AGBNP_HIP_DECOMPOSITION_TERMS planes of N doubles -- cavity, vdW, GB self, GB pair (each pair shared half and half) -- whose
  // sum over everything is the energy.  Version 0 has the cavity plane only.  No forces are written.
  double decompose(const std::vector<double>& positions, std::vector<double>& terms) {
    need();
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("decompose(): positions must hold 3N values");
    terms.assign((size_t)AGBNP_HIP_DECOMPOSITION_TERMS * numParticles, 0.0);
    double e = 0.0;
    check(agbnp_hip_decompose_host(ctx, positions.data(), terms.data(), &e));
    return e;
  }

  // The partition that pairMatrix() tabulates (agbnp_hip_set_atom_sets): sets[i] in 0 .. numSets - 1 is the set of atom i (its
  // residue, its chain, receptor or ligand); numSets < 0: the largest index + 1.  Checked before the library is touched; replaces
  // an earlier partition and survives copyParametersToContext().
  void setAtomSets(const std::vector<int>& sets, int numSets = -1) {
    need();
    numSets = detail::checkAtomSets("setAtomSets", sets, numParticles, numSets);
    check(agbnp_hip_set_atom_sets(ctx, numParticles, sets.data(), numSets));
  }
  int numAtomSets() const { return ctx ? agbnp_hip_num_atom_sets(ctx) : 0; }

  // Set-pair interaction matrix of the energy at these positions (agbnp_hip_pair_matrix_host): returns the energy; `matrix`
  // receives M[S][S], row-major, over the sets of setAtomSets() -- M[a][b] = M[b][a] half the GB pair energy between sets a and b,
  // M[a][a] what set a holds in itself -- whose sum over everything is the energy.  No forces are written.
  double pairMatrix(const std::vector<double>& positions, std::vector<double>& matrix) {
    need();
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("pairMatrix(): positions must hold 3N values");
    const size_t s = (size_t)numAtomSets();
    matrix.assign(s * s + (s == 0), 0.0);  // (no partition: the library refuses, with its message)
    double e = 0.0;
    check(agbnp_hip_pair_matrix_host(ctx, positions.data(), matrix.data(), &e));
    return e;
  }

  // Replica groups (agbnp_hip_execute_group_host): one evaluation of every kernel in `kernels`, the launches of the members
  // that can share them made once for all; positions[i] (3N_i) read, forces[i] accumulated, the members' energies returned.
  static std::vector<double> executeGroup(const std::vector<HipCalcAGBNPForceKernel*>& kernels,
                                          const std::vector<std::vector<double>>& positions, std::vector<std::vector<double>>& forces) {
    auto g = detail::Group::collect("executeGroup", kernels, "a group has 1 to 16 members", "one position and one force array per member",
                                    true, positions, &forces);
    std::vector<double> energies(kernels.size(), 0.0);
    detail::check(agbnp_hip_execute_group_host(g.handles.data(), (int)kernels.size(), g.pos.data(), g.frc.data(), energies.data()),
                  g.handles[0]);
    return energies;
  }

  // Energy-only replica groups (agbnp_hip_energy_group_host): the energy of every kernel in `kernels` at positions[i] (3N_i),
  // on shared energy-only launches where the members allow it; no force is written anywhere.
  static std::vector<double> energyGroup(const std::vector<HipCalcAGBNPForceKernel*>& kernels,
                                         const std::vector<std::vector<double>>& positions) {
    auto g = detail::Group::collect("energyGroup", kernels, "a group has 1 to 16 members", "one position array per member", true, positions);
    std::vector<double> energies(kernels.size(), 0.0);
    detail::check(agbnp_hip_energy_group_host(g.handles.data(), (int)kernels.size(), g.pos.data(), energies.data()), g.handles[0]);
    return energies;
  }

  // Decomposition groups (agbnp_hip_decompose_group_host): the per-atom decomposition of every kernel in `kernels` at
  // positions[i] (3N_i), the members that can share on the energy-only group's launches plus one plane launch per launch set.
  // terms[i] receives AGBNP_HIP_DECOMPOSITION_TERMS planes of N_i doubles (as decompose()); the members' energies are returned.
  static std::vector<double> decomposeGroup(const std::vector<HipCalcAGBNPForceKernel*>& kernels,
                                            const std::vector<std::vector<double>>& positions, std::vector<std::vector<double>>& terms) {
    auto g = detail::Group::collect("decomposeGroup", kernels, "a group has 1 to 16 members", "one position array per member", true, positions);
    terms.resize(kernels.size());
    std::vector<double*> planes(kernels.size());
    for (size_t i = 0; i < kernels.size(); i++) {
      terms[i].assign((size_t)AGBNP_HIP_DECOMPOSITION_TERMS * kernels[i]->numParticles, 0.0);
      planes[i] = terms[i].data();
    }
    std::vector<double> energies(kernels.size(), 0.0);
    detail::check(agbnp_hip_decompose_group_host(g.handles.data(), (int)kernels.size(), g.pos.data(), planes.data(), energies.data()),
                  g.handles[0]);
    return energies;
  }

  // Pair-matrix groups (agbnp_hip_pair_matrix_group_host): the set-pair matrix of every kernel in `kernels` at positions[i]
  // (3N_i), each over its own partition (setAtomSets(); checked here), the members that can share on the energy-only group's
  // launches plus one matrix launch per launch set.  matrices[i] receives M[S_i][S_i], row-major (as pairMatrix()); the members'
  // energies are returned.
  static std::vector<double> pairMatrixGroup(const std::vector<HipCalcAGBNPForceKernel*>& kernels,
                                             const std::vector<std::vector<double>>& positions, std::vector<std::vector<double>>& matrices) {
    auto g = detail::Group::collect("pairMatrixGroup", kernels, "a group has 1 to 16 members", "one position array per member", true, positions);
    matrices.resize(kernels.size());
    std::vector<double*> targets(kernels.size());
    for (size_t i = 0; i < kernels.size(); i++) {
      const size_t s = (size_t)kernels[i]->numAtomSets();
      if (s == 0) throw OpenMMException("pairMatrixGroup(): a member has no partition (setAtomSets())");
      matrices[i].assign(s * s, 0.0);
      targets[i] = matrices[i].data();
    }
    std::vector<double> energies(kernels.size(), 0.0);
    detail::check(agbnp_hip_pair_matrix_group_host(g.handles.data(), (int)kernels.size(), g.pos.data(), targets.data(), energies.data()),
                  g.handles[0]);
    return energies;
  }

  // The parameter sets that perturbedEnergies() scores (agbnp_hip_set_parameter_sets): gamma, vdwAlpha and charge hold M sets of N
  // values each, set-major, M 1 .. AGBNP_HIP_MAX_PARAMETER_SETS; radii and hydrogen flags are the kernel's own.  Checked before the
  // library is touched; replaces earlier sets and survives copyParametersToContext().
  void setParameterSets(const std::vector<double>& gamma, const std::vector<double>& vdwAlpha, const std::vector<double>& charge) {
    need();
    const size_t n = (size_t)numParticles, m = n ? gamma.size() / n : 0;
    if (m < 1 || m > AGBNP_HIP_MAX_PARAMETER_SETS || gamma.size() != m * n || vdwAlpha.size() != m * n || charge.size() != m * n)
      throw OpenMMException("setParameterSets(): gamma, vdwAlpha and charge must each hold M x N values, M 1 .. 16");
    check(agbnp_hip_set_parameter_sets(ctx, numParticles, (int)m, gamma.data(), vdwAlpha.data(), charge.data()));
  }
  int numParameterSets() const { return ctx ? agbnp_hip_num_parameter_sets(ctx) : 0; }

  // The energy of these positions under every set of setParameterSets(), from one evaluation (agbnp_hip_perturbed_energies_host):
  // returns the kernel's own energy; energies[m] receives what a kernel initialised with set m would return.  No forces are written.
  double perturbedEnergies(const std::vector<double>& positions, std::vector<double>& energies) {
    need();
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("perturbedEnergies(): positions must hold 3N values");
    const size_t m = (size_t)numParameterSets();
    energies.assign(m + (m == 0), 0.0);  // (no sets: the library refuses, with its message)
    double e = 0.0;
    check(agbnp_hip_perturbed_energies_host(ctx, positions.data(), energies.data(), &e));
    return e;
  }

  // Perturbation groups (agbnp_hip_perturbed_energies_group_host): the perturbation energies of every kernel in `kernels` at
  // positions[i] (3N_i), each over its own sets (setParameterSets(); checked here), the members that can share on the energy-only
  // group's launches plus one perturbation launch per launch set.  energies[i] receives [M_i]; the members' own energies are returned.
  static std::vector<double> perturbedEnergiesGroup(const std::vector<HipCalcAGBNPForceKernel*>& kernels,
                                                    const std::vector<std::vector<double>>& positions, std::vector<std::vector<double>>& energies) {
    auto g = detail::Group::collect("perturbedEnergiesGroup", kernels, "a group has 1 to 16 members", "one position array per member", true, positions);
    energies.resize(kernels.size());
    std::vector<double*> targets(kernels.size());
    for (size_t i = 0; i < kernels.size(); i++) {
      const size_t m = (size_t)kernels[i]->numParameterSets();
      if (m == 0) throw OpenMMException("perturbedEnergiesGroup(): a member has no parameter sets (setParameterSets())");
      energies[i].assign(m, 0.0);
      targets[i] = energies[i].data();
    }
    std::vector<double> own(kernels.size(), 0.0);
    detail::check(agbnp_hip_perturbed_energies_group_host(g.handles.data(), (int)kernels.size(), g.pos.data(), targets.data(), own.data()),
                  g.handles[0]);
    return own;
  }

  // The positions of the next evaluation are unrelated to the last ones (agbnp_hip_expect_jump): it lays the neighbour masks
  // down at its own positions first and is not withheld for the jump.
  void expectJump() {
    need();
    check(agbnp_hip_expect_jump(ctx));
  }

  void copyParametersToContext(const AGBNPForce& force) {
    need();
    const detail::Parameters p = detail::gather(force);
    check(agbnp_hip_update_parameters(ctx, p.n(), p.r.data(), p.g.data(), p.a.data(), p.q.data(), p.h.data()));
  }

  agbnp_hip_context* handle() const { return ctx; }

 private:
  friend struct detail::Group;
  typedef agbnp_hip_context Handle;
  static constexpr size_t maxGroup = AGBNP_HIP_MAX_GROUP;
  static agbnp_hip_context* groupHandle(const HipCalcAGBNPForceKernel* k, const std::string&) {
    if (!k || !k->ctx) throw OpenMMException("HipCalcAGBNPForceKernel: initialize() has not been called");
    return k->ctx;
  }
  void need() const { groupHandle(this, ""); }
  void check(int rc) const { detail::check(rc, ctx); }
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
    const detail::Parameters p = detail::gather(force);
    check(agbnp_hip_binding_create(&b, numParticles, p.r.data(), p.g.data(), p.a.data(), p.q.data(), p.h.data(), ligandAtoms.data(),
                                   (int)ligandAtoms.size(), (int)force.getVersion(), (int)force.getNonbondedMethod(),
                                   force.getCutoffDistance(), device));
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
  // Per-atom decomposition of the binding energy (agbnp_hip_binding_decompose_host): returns u; `terms` receives
  // AGBNP_HIP_DECOMPOSITION_TERMS planes of N doubles in the complex's atom order, D[t][i] = T_RL[t][i] - T_own[t][own(i)] -- the
  // complex's term of atom i minus the term of the same atom in its own sub-system alone -- which sum to u.  Withheld evaluations
  // are repeated inside.
  double decompose(const std::vector<double>& positions, std::vector<double>& terms) {
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("Binding::decompose(): positions must hold 3N values");
    terms.assign((size_t)AGBNP_HIP_DECOMPOSITION_TERMS * numParticles, 0.0);
    double u = 0.0;
    check(agbnp_hip_binding_decompose_host(b, positions.data(), terms.data(), &u));
    return u;
  }
  // device pointers: the 4N terms and u are ADDED -- all of them or, if a member is withheld, nothing; asynchronous
  void decomposeDevice(const double* dPositions, double* dPerAtom, double* dBindingEnergy, void* stream = nullptr) {
    check(agbnp_hip_binding_decompose_device(b, dPositions, dPerAtom, dBindingEnergy, stream));
  }
  // The partition that pairMatrix() tabulates (agbnp_hip_binding_set_atom_sets): sets[i] in 0 .. numSets - 1 is the set of atom i
  // of the COMPLEX (a set may mix receptor and ligand atoms); numSets < 0: the largest index + 1.  Checked before the library is
  // touched, as HipCalcAGBNPForceKernel::setAtomSets() checks; a refused partition leaves the earlier one in force.
  void setAtomSets(const std::vector<int>& sets, int numSets = -1) {
    numSets = detail::checkAtomSets("Binding::setAtomSets", sets, numParticles, numSets);
    check(agbnp_hip_binding_set_atom_sets(b, numParticles, sets.data(), numSets));
  }
  int numAtomSets() const { return agbnp_hip_binding_num_atom_sets(b); }
  // Set-pair matrix of the binding energy (agbnp_hip_binding_pair_matrix_host): returns u; `matrix` receives D[S][S], row-major,
  // D = M_RL - M_R - M_L of the members' pairMatrix() tables over the sets of setAtomSets(), which sums to u.  Withheld
  // evaluations are repeated inside.
  double pairMatrix(const std::vector<double>& positions, std::vector<double>& matrix) {
    if ((int)positions.size() != 3 * numParticles) throw OpenMMException("Binding::pairMatrix(): positions must hold 3N values");
    const size_t s = (size_t)numAtomSets();
    matrix.assign(s * s + (s == 0), 0.0);  // (no partition: the library refuses, with its message)
    double u = 0.0;
    check(agbnp_hip_binding_pair_matrix_host(b, positions.data(), matrix.data(), &u));
    return u;
  }
  // device pointers: the S S entries of D and u are ADDED -- all of them or, if a member is withheld, nothing; asynchronous
  void pairMatrixDevice(const double* dPositions, double* dMatrix, double* dBindingEnergy, void* stream = nullptr) {
    check(agbnp_hip_binding_pair_matrix_device(b, dPositions, dMatrix, dBindingEnergy, stream));
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
    const detail::Parameters p = detail::gather(force);
    check(agbnp_hip_binding_update_parameters(b, p.n(), p.r.data(), p.g.data(), p.a.data(), p.q.data(), p.h.data()));
  }
  // a member's context, for scalars, vectors, poll and wait_verdict; the binding owns it
  agbnp_hip_context* member(Member which) const { return agbnp_hip_binding_member(b, (int)which); }
  agbnp_hip_binding* handle() const { return b; }
  int getNumParticles() const { return numParticles; }

 private:
  friend struct detail::Group;
  typedef agbnp_hip_binding Handle;
  static constexpr size_t maxGroup = AGBNP_HIP_MAX_BINDING_GROUP;
  static agbnp_hip_binding* groupHandle(const Binding* binding, const std::string& who) {
    if (!binding) throw OpenMMException(who + "(): null binding");
    return binding->b;
  }
  static void check(int rc) { detail::check(rc); }  // (a binding's messages are kept with those of no context)
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
  auto g = detail::Group::collect("executeBindingGroup", bindings, "a binding group has 1 to 16 bindings",
                                  "one position array, one force array and one lambda per binding", lambdas.size() == n, positions, &forces);
  std::vector<double> energies(n, 0.0);
  bindingEnergies.assign(n, 0.0);
  detail::check(agbnp_hip_binding_execute_group_host(g.handles.data(), (int)n, g.pos.data(), lambdas.data(), g.frc.data(), energies.data(),
                                                     bindingEnergies.data()));
  return energies;
}

// The same without forces (agbnp_hip_binding_energy_group_host): no force is written anywhere.
inline std::vector<double> energyBindingGroup(const std::vector<Binding*>& bindings, const std::vector<std::vector<double>>& positions,
                                              const std::vector<double>& lambdas, std::vector<double>& bindingEnergies) {
  const size_t n = bindings.size();
  auto g = detail::Group::collect("energyBindingGroup", bindings, "a binding group has 1 to 16 bindings",
                                  "one position array and one lambda per binding", lambdas.size() == n, positions);
  std::vector<double> energies(n, 0.0);
  bindingEnergies.assign(n, 0.0);
  detail::check(agbnp_hip_binding_energy_group_host(g.handles.data(), (int)n, g.pos.data(), lambdas.data(), energies.data(),
                                                    bindingEnergies.data()));
  return energies;
}

}  // namespace AGBNPPlugin
