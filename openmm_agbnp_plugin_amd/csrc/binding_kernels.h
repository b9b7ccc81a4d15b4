// Launchers of the two launches a binding evaluation puts round its group call (binding_kernels.hip; engine_binding.hip;
// agbnp_hip_binding_*, include/agbnp_hip.h): the single-binding forms, with their short argument lists and lambda by value, and
// the group forms.  Both are wrappers round the same device bodies; binding_enqueue picks the form by where its lambdas are.
#pragma once
#include <hip/hip_runtime.h>

namespace agbnp {

constexpr int kBindingMembers = 3;  // complex, receptor, ligand -- the `which` of agbnp_hip_binding_member

// Where the combine launch finds the three members' verdicts on the evaluation that has just been enqueued: each member's
// per-evaluation status words as its own argument block names them (PairArgs::estatus, five, epoch) behind its launches.
struct BindingVerdicts {
  const int* estatus[kBindingMembers];
  const int* epoch[kBindingMembers];  // read only where five == 2: the device names the set (rebase_for_parity, after_role = 1)
  int five[kBindingMembers];
};

// One thread per atom of the receptor and the ligand: sub_pos[3 t] = pos[3 sub2complex[t]].  sub2complex: the receptor's atoms
// in ascending complex order, then the ligand's -- sub_pos is the receptor's position array followed by the ligand's.
hipError_t launch_binding_gather(int n, const double* pos, const int* sub2complex, double* sub_pos, hipStream_t st);

// The full form: one thread per atom of the complex, thread 0 the scalars.  f_complex[3n] and f_sub[3n] (receptor then ligand)
// and e[3] are the binding's own buffers, which the members ADDED to: read, and CLEARED whatever the verdict.
// d_energy / d_binding may be null.
hipError_t launch_binding_combine(int n, const BindingVerdicts& v, double lambda, const int* complex2sub, double* f_complex,
                                  double* f_sub, double* e, double* d_forces, double* d_energy, double* d_binding, hipStream_t st);

// The energy-only form: one small workgroup, the scalars alone.
hipError_t launch_binding_combine_energy(const BindingVerdicts& v, double lambda, double* e, double* d_energy, double* d_binding,
                                         hipStream_t st);

// The per-atom decomposition of a binding (agbnp_hip_binding_decompose_*): one thread per atom of the complex, thread 0 the
// scalars.  t_complex[4n] and t_sub[4 nr + 4 (n - nr)] (the receptor's planes, then the ligand's) and e[3] are the binding's own
// staging words, which the members of one agbnp_hip_decompose_group ADDED to: read, and CLEARED whatever the verdict.
// D[t][i] = t_complex[t][i] - t_own[t][own(i)] is ADDED to d_per_atom[4n], u to *d_binding (may be null).
hipError_t launch_binding_decompose_combine(int n, int nr, const BindingVerdicts& v, const int* complex2sub, double* t_complex,
                                            double* t_sub, double* e, double* d_per_atom, double* d_binding, hipStream_t st);

// The set-pair matrix of a binding (agbnp_hip_binding_pair_matrix_*): one thread per cell of the S x S matrix, thread 0 the
// scalars.  m[3][S S] (the complex's, the receptor's and the ligand's matrix, one set numbering) and e[3] are the binding's own
// staging words, which the members of one agbnp_hip_pair_matrix_group ADDED to: read, and CLEARED whatever the verdict.
// D[a][b] = m[0][a][b] - m[1][a][b] - m[2][a][b] is ADDED to d_matrix[S S], u to *d_binding (may be null).
hipError_t launch_binding_matrix_combine(int num_sets, const BindingVerdicts& v, double* m, double* e, double* d_matrix, double* d_binding,
                                         hipStream_t st);

// ---- Binding groups (agbnp_hip_binding_execute_group / _energy_group): the same two launches, made once for up to
// kMaxBindingGroup bindings.  Every binding keeps the grid it would launch alone; the grids lie side by side and a workgroup finds
// its binding by its number (first[]), as the workgroups of a replica group's launches do (group_args.h: GroupLaunch::first).
constexpr int kMaxBindingGroup = 16;  // AGBNP_HIP_MAX_BINDING_GROUP (include/agbnp_hip.h)

// One binding's words of a group launch: 120 bytes.
struct BindingGroupMember {
  BindingVerdicts v;   // [64 bytes] the three members' verdicts on the evaluation that has just been enqueued
  const int* maps;     // [2n] sub2complex, complex2sub
  double* work;        // [9n + 3] the binding's own: sub-system positions | F^RL | F^{R|L} | the three energies
  const double* pos;   // the caller's positions [3n]
  double* forces;      // the caller's F_lambda [3n] (null: the energy-only form), E_lambda and u (either may be null)
  double* energy;
  double* binding;
  int n;               // atoms of the complex
};

// The kernel argument of a group launch, by value: 72 + 16 * 120 + 8 = 2000 bytes (static_assert in binding_kernels.hip), inside
// the 4096 bytes that a kernel's arguments may take.  Every word a workgroup reads of it is uniform: scalar loads.
struct BindingGroupArgs {
  int count;                        // bindings of the call
  int first[kMaxBindingGroup + 1];  // first workgroup of every binding (256 atoms each); first[count] = the grid
  BindingGroupMember m[kMaxBindingGroup];
  const double* lambdas;            // [count] DEVICE words, read by the combine launch when it runs
};

// One launch for all bindings: m[k].work[3 t] = m[k].pos[3 sub2complex[t]] for t < m[k].n.
hipError_t launch_binding_gather_group(const BindingGroupArgs& G, hipStream_t st);
// One launch for all bindings: per binding what launch_binding_combine does, with lambda = lambdas[k].
hipError_t launch_binding_combine_group(const BindingGroupArgs& G, hipStream_t st);
// The energy-only form: one small workgroup per binding, the scalars alone.
hipError_t launch_binding_combine_energy_group(const BindingGroupArgs& G, hipStream_t st);

}  // namespace agbnp
