// Binding-energy evaluations (agbnp_hip_binding_*, include/agbnp_hip.h; host side: engine_binding.hip): the two launches round
// the group call that evaluates the complex, the receptor and the ligand.
//   k_binding_gather   in front: the receptor's and the ligand's positions out of the complex's array, through the index map
//   k_binding_combine  behind: F_lambda = lambda F^RL + (1 - lambda) F^{R|L}, E_lambda = (1 - lambda)(E_R + E_L) + lambda E_RL and
//                      u = E_RL - E_R - E_L ADDED to the caller's buffers -- if and only if ALL THREE members' evaluations are
//                      complete.  The members are gated one by one (each adds nothing when it is withheld itself); what ties the
//                      three verdicts together is this launch, which reads every member's verdict words behind the group's
//                      launches, the way k_decompose reads its context's.
// The members ADD into buffers of the binding's own.  The combine launch CLEARS them whatever the verdict: a withheld binding
// evaluation whose receptor was complete would otherwise leave the receptor's forces behind for the next one.
// Both are streaming kernels, one thread per atom, elementwise: no order-dependent sum, so the deterministic mode's outputs are
// bit-identical from run to run as the members' are.  The gather's indexed read is the only uncoalesced access.
// Binding groups (agbnp_hip_binding_execute_group) make the same two launches ONCE for up to 16 bindings, every
// binding's grid side by side, its words by value in the kernel argument (BindingGroupArgs) and its lambda read from device
// memory when the launch runs.
// The per-atom work stands ONCE, in the device bodies below (binding_gather_atom, binding_combine_atom, binding_complete,
// binding_scalars).  The six kernels are wrappers, as the single and group kernels round pair_bodies.h are: each finds its
// binding, its lambda and its pointers -- the single forms in their own short argument lists, lambda by value; the group forms in
// BindingGroupArgs -- and calls the body.
//
// The verdict test is the engine's own (evaluation_overflowed), read as a device function as the decomposition's unit reads it:
// this unit launches none of the kernels of pair_bodies.h.
#define AGBNP_GROUP_TU
#include "pair_bodies.h"

#include "binding_kernels.h"

namespace agbnp {

// ---- the bodies ----
// atom t of the receptor-then-ligand order: its position out of the complex's array
__device__ __forceinline__ void binding_gather_atom(int t, const double* __restrict__ pos, const int* __restrict__ sub2complex,
                                                    double* __restrict__ sub_pos) {
  const size_t src = 3 * (size_t)sub2complex[t], dst = 3 * (size_t)t;
  const double x = pos[src], y = pos[src + 1], z = pos[src + 2];
  sub_pos[dst] = x;
  sub_pos[dst + 1] = y;
  sub_pos[dst + 2] = z;
}

// all three members complete?  (the same for every thread of the launch: scalar loads)
__device__ __forceinline__ bool binding_complete(const BindingVerdicts& v) {
  bool ok = true;
#pragma unroll
  for (int m = 0; m < kBindingMembers; m++) {
    // (five == 2, a member that was once captured into a graph: its block names set 0 and the device's counter, which its GB
    // launch has advanced, names the set -- rebase_for_parity with after_role = 1)
    const int par = v.five[m] == 2 ? (v.epoch[m][0] + 1) & 1 : 0;
    ok = ok && !evaluation_overflowed(v.estatus[m] + kStatBlockStride * par);
  }
  return ok;
}

// the role lane: the three energies read and cleared, E_lambda and u added
__device__ __forceinline__ void binding_scalars(bool ok, double lambda, double* __restrict__ e, double* __restrict__ d_energy,
                                                double* __restrict__ d_binding) {
  // (atomic loads, so that they are VECTOR loads: the address is uniform, and as plain loads they become scalar loads, which the
  // clears below -- vector stores with no data dependence on them -- are issued past: an energy word then reads as the zero
  // that was about to be written.  Loads and stores of one wave through the vector pipe stay in order.)
  const double e_rl = __hip_atomic_load(&e[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double e_r = __hip_atomic_load(&e[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double e_l = __hip_atomic_load(&e[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  e[0] = e[1] = e[2] = 0.0;
  if (!ok) return;
  if (d_energy) d_energy[0] += (1.0 - lambda) * (e_r + e_l) + lambda * e_rl;
  if (d_binding) d_binding[0] += e_rl - e_r - e_l;
}

// atom i of the complex, t = complex2sub[i] its place in the receptor-then-ligand order: its two force terms read and cleared,
// F_lambda added.  (Plain pointers: that the buffers do not alias is the wrappers' promise, made where each names them.)
__device__ __forceinline__ void binding_combine_atom(int i, int t, bool ok, double lambda, double* f_complex, double* f_sub,
                                                     double* d_forces) {
  const size_t a = 3 * (size_t)i, s = 3 * (size_t)t;
  const double w = 1.0 - lambda;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const double f_rl = f_complex[a + d], f_own = f_sub[s + d];
    f_complex[a + d] = 0.0;
    f_sub[s + d] = 0.0;
    if (ok) d_forces[a + d] += lambda * f_rl + w * f_own;
  }
}

// ---- one binding ----
__global__ __launch_bounds__(256) void k_binding_gather(int n, const double* __restrict__ pos, const int* __restrict__ sub2complex,
                                                        double* __restrict__ sub_pos) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < n) binding_gather_atom(t, pos, sub2complex, sub_pos);
}

__global__ __launch_bounds__(256) void k_binding_combine(int n, BindingVerdicts v, double lambda, const int* __restrict__ complex2sub,
                                                         double* __restrict__ f_complex, double* __restrict__ f_sub,
                                                         double* __restrict__ e, double* __restrict__ d_forces,
                                                         double* __restrict__ d_energy, double* __restrict__ d_binding) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool ok = binding_complete(v);
  if (i == 0) binding_scalars(ok, lambda, e, d_energy, d_binding);  // the role lane
  binding_combine_atom(i, complex2sub[i], ok, lambda, f_complex, f_sub, d_forces);
}

__global__ __launch_bounds__(64) void k_binding_combine_energy(BindingVerdicts v, double lambda, double* __restrict__ e,
                                                               double* __restrict__ d_energy, double* __restrict__ d_binding) {
  if (threadIdx.x == 0) binding_scalars(binding_complete(v), lambda, e, d_energy, d_binding);
}

// ---- per-atom decomposition of a binding (agbnp_hip_binding_decompose_*): D[t][i] = T_RL[t][i] - T_own[t][own(i)] ----
// Behind ONE agbnp_hip_decompose_group over {complex, receptor, ligand}, whose members ADDED their planes and energies to the
// binding's staging buffer: one thread per atom i of the complex reads its four terms of the complex's planes [4][n] and of its
// own sub-system's -- the receptor's [4][nr] at complex2sub[i], or the ligand's [4][n - nr] at complex2sub[i] - nr --, CLEARS the
// eight words whatever the verdict, and adds the differences to the caller's planes if all three members are complete.  Thread 0
// is also the role lane: binding_scalars with lambda = 1 and no E_lambda target reads and clears the three energies and adds u.
// The per-atom words are read by the thread that clears them, through vector loads in front of its own vector stores; the
// uniform words -- the verdicts (never cleared here) and the energies (atomic loads: vector loads, see binding_scalars) -- are
// what the compiler hazard of DESIGN.md s.4n is about.  Elementwise: bit-identical from run to run where the members are.
__global__ __launch_bounds__(256) void k_binding_decompose_combine(int n, int nr, BindingVerdicts v, const int* __restrict__ complex2sub,
                                                                   double* t_complex, double* t_sub, double* __restrict__ e,
                                                                   double* d_per_atom, double* __restrict__ d_binding) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool ok = binding_complete(v);
  if (i == 0) binding_scalars(ok, 1.0, e, nullptr, d_binding);  // the role lane: u = E_RL - E_R - E_L
  const int t = complex2sub[i];
  const bool in_receptor = t < nr;
  const size_t n_own = in_receptor ? (size_t)nr : (size_t)(n - nr);
  double* own = in_receptor ? t_sub + t : t_sub + 4 * (size_t)nr + (t - nr);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const size_t a = (size_t)k * n + i, s = (size_t)k * n_own;
    const double t_rl = t_complex[a], t_own = own[s];
    t_complex[a] = 0.0;
    own[s] = 0.0;
    if (ok) d_per_atom[a] += t_rl - t_own;
  }
}

// ---- set-pair matrix of a binding (agbnp_hip_binding_pair_matrix_*): D[a][b] = M_RL[a][b] - M_R[a][b] - M_L[a][b] ----
// Behind ONE agbnp_hip_pair_matrix_group over {complex, receptor, ligand}, whose members ADDED their matrices -- all three [S][S],
// one set numbering -- and energies to the binding's staging buffer m[3][cells] | e[3]: one thread per cell reads its three words,
// CLEARS them whatever the verdict, and adds the difference to the caller's matrix if all three members are complete.  Thread 0
// is also the role lane, as in k_binding_decompose_combine.  Every cell is read by the thread that clears it, through vector loads
// in front of its own vector stores.  Elementwise: bit-identical from run to run where the members are.
__global__ __launch_bounds__(256) void k_binding_matrix_combine(size_t cells, BindingVerdicts v, double* m, double* __restrict__ e,
                                                                double* d_matrix, double* __restrict__ d_binding) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const bool ok = binding_complete(v);
  if (c == 0) binding_scalars(ok, 1.0, e, nullptr, d_binding);  // the role lane: u = E_RL - E_R - E_L
  const double m_rl = m[c], m_r = m[cells + c], m_l = m[2 * cells + c];
  m[c] = 0.0;
  m[cells + c] = 0.0;
  m[2 * cells + c] = 0.0;
  if (ok) d_matrix[c] += m_rl - m_r - m_l;
}

// ---- binding groups: the same launches once for all bindings of a call (binding_kernels.h: BindingGroupArgs) ----
static_assert(sizeof(BindingGroupMember) == 120 && sizeof(BindingGroupArgs) == 2000, "BindingGroupArgs: the size binding_kernels.h states");
static_assert(sizeof(BindingGroupArgs) <= 4096, "a kernel's arguments take 4096 bytes at most");

// the binding of the workgroup and the workgroup's number inside that binding's grid (both uniform; group_args.h: group_index)
__device__ __forceinline__ int binding_group_index(const BindingGroupArgs& G, int& blk) {
  const int b = (int)blockIdx.x;
  int k = 0;
#pragma unroll
  for (int j = 1; j < kMaxBindingGroup; j++)
    if (j < G.count && b >= G.first[j]) k = j;
  blk = b - G.first[k];
  return k;
}

// lambda of binding k: a device word that a kernel earlier on the stream may have written.  (An atomic load, so that it is a
// VECTOR load like the role lane's reads of the energy words: see binding_scalars.)
__device__ __forceinline__ double binding_group_lambda(const BindingGroupArgs& G, int k) {
  return __hip_atomic_load(&G.lambdas[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_binding_gather_group(const BindingGroupArgs G) {
  int blk;
  const BindingGroupMember& B = G.m[binding_group_index(G, blk)];
  const int t = blk * 256 + threadIdx.x;
  if (t < B.n) binding_gather_atom(t, B.pos, B.maps, B.work);
}

__global__ __launch_bounds__(256) void k_binding_combine_group(const BindingGroupArgs G) {
  int blk;
  const int k = binding_group_index(G, blk);
  const BindingGroupMember& B = G.m[k];
  const int i = blk * 256 + threadIdx.x, n = B.n;
  if (i >= n) return;
  const bool ok = binding_complete(B.v);
  const double lambda = binding_group_lambda(G, k);
  double* __restrict__ f_complex = B.work + 3 * (size_t)n;
  double* __restrict__ f_sub = B.work + 6 * (size_t)n;
  double* __restrict__ d_forces = B.forces;
  if (i == 0) binding_scalars(ok, lambda, B.work + 9 * (size_t)n, B.energy, B.binding);  // the binding's role lane
  binding_combine_atom(i, B.maps[n + i], ok, lambda, f_complex, f_sub, d_forces);
}

__global__ __launch_bounds__(64) void k_binding_combine_energy_group(const BindingGroupArgs G) {
  const int k = blockIdx.x;  // (one workgroup per binding)
  const BindingGroupMember& B = G.m[k];
  if (threadIdx.x == 0) binding_scalars(binding_complete(B.v), binding_group_lambda(G, k), B.work + 9 * (size_t)B.n, B.energy, B.binding);
}

// ---- launchers ----
hipError_t launch_binding_gather(int n, const double* pos, const int* sub2complex, double* sub_pos, hipStream_t st) {
  hipLaunchKernelGGL(k_binding_gather, dim3((n + 255) / 256), dim3(256), 0, st, n, pos, sub2complex, sub_pos);
  return hipGetLastError();
}

hipError_t launch_binding_combine(int n, const BindingVerdicts& v, double lambda, const int* complex2sub, double* f_complex,
                                  double* f_sub, double* e, double* d_forces, double* d_energy, double* d_binding, hipStream_t st) {
  hipLaunchKernelGGL(k_binding_combine, dim3((n + 255) / 256), dim3(256), 0, st, n, v, lambda, complex2sub, f_complex, f_sub, e,
                     d_forces, d_energy, d_binding);
  return hipGetLastError();
}

hipError_t launch_binding_combine_energy(const BindingVerdicts& v, double lambda, double* e, double* d_energy, double* d_binding,
                                         hipStream_t st) {
  hipLaunchKernelGGL(k_binding_combine_energy, dim3(1), dim3(64), 0, st, v, lambda, e, d_energy, d_binding);
  return hipGetLastError();
}

hipError_t launch_binding_decompose_combine(int n, int nr, const BindingVerdicts& v, const int* complex2sub, double* t_complex,
                                            double* t_sub, double* e, double* d_per_atom, double* d_binding, hipStream_t st) {
  hipLaunchKernelGGL(k_binding_decompose_combine, dim3((n + 255) / 256), dim3(256), 0, st, n, nr, v, complex2sub, t_complex, t_sub, e,
                     d_per_atom, d_binding);
  return hipGetLastError();
}

hipError_t launch_binding_matrix_combine(int num_sets, const BindingVerdicts& v, double* m, double* e, double* d_matrix, double* d_binding,
                                         hipStream_t st) {
  const size_t cells = (size_t)num_sets * (size_t)num_sets;  // (at most 2048^2: 16384 workgroups)
  hipLaunchKernelGGL(k_binding_matrix_combine, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, cells, v, m, e, d_matrix, d_binding);
  return hipGetLastError();
}

hipError_t launch_binding_gather_group(const BindingGroupArgs& G, hipStream_t st) {
  hipLaunchKernelGGL(k_binding_gather_group, dim3(G.first[G.count]), dim3(256), 0, st, G);
  return hipGetLastError();
}

hipError_t launch_binding_combine_group(const BindingGroupArgs& G, hipStream_t st) {
  hipLaunchKernelGGL(k_binding_combine_group, dim3(G.first[G.count]), dim3(256), 0, st, G);
  return hipGetLastError();
}

hipError_t launch_binding_combine_energy_group(const BindingGroupArgs& G, hipStream_t st) {
  hipLaunchKernelGGL(k_binding_combine_energy_group, dim3(G.count), dim3(64), 0, st, G);
  return hipGetLastError();
}

}  // namespace agbnp
