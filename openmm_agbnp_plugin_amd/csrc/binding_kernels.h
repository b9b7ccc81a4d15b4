// Launchers of the two launches a binding evaluation puts round its group call (binding_kernels.hip; engine_binding.hip;
// agbnp_hip_binding_*, include/agbnp_hip.h).
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

}  // namespace agbnp
