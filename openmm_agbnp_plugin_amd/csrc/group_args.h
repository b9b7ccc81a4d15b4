// Replica groups (agbnp_hip_execute_group, engine_group.hip): the launches that several contexts share.
//
// Every context of a launch set keeps exactly the grid it would launch alone; the grids are laid side by side, and a
// workgroup finds its member by its number (GroupLaunch::first) and runs the member's kernel body with its number inside
// that member's grid.  No workgroup of these kernels waits for another one, so concatenating grids changes nothing but
// where a workgroup sits in the launch.
//
// What the bodies read of a member -- but for the caller's output buffers, which travel in the launch's argument -- lives on the device, in the context's own argument block (one per parity of the
// five-launch mode's sets), and arrives through scalar loads like a kernel argument: the block is addressed through the
// constant address space.  The engine rewrites a block, stream-ordered, only when the host-built one differs from what it
// last wrote (a new capacity variant, grown rows, the other entry point, another position buffer): a steady run of group evaluations writes nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "pair_kernels.h"
#include "tree_kernels.h"

// The kernels that members share are written once, in pair_bodies.h and tree_bodies.h, and name themselves through these.
// pair_kernels.hip and tree_kernels.hip read the headers as they are: the bodies are __global__ kernels.  group_kernels.hip
// sets AGBNP_GROUP_TU before it reads them: the bodies are device functions that take the workgroup's number (and the grid's
// size) inside the member's grid, and that unit's own kernels call them.
#ifdef AGBNP_GROUP_TU
#define AGBNP_KERNEL __device__ __forceinline__
#define AGBNP_BOUNDS(...)
#define AGBNP_WG agbnp_wg
#define AGBNP_NWG agbnp_nwg
#define AGBNP_WG_PARAM , const unsigned agbnp_wg, const unsigned agbnp_nwg
#define AGBNP_WG_ARG , agbnp_wg, agbnp_nwg
#else
#define AGBNP_KERNEL __global__
#define AGBNP_BOUNDS(...) __launch_bounds__(__VA_ARGS__)
#define AGBNP_WG blockIdx.x
#define AGBNP_NWG gridDim.x
#define AGBNP_WG_PARAM
#define AGBNP_WG_ARG
#endif

namespace agbnp {

constexpr int kMaxGroup = 16;  // AGBNP_HIP_MAX_GROUP (include/agbnp_hip.h)

// One member's arguments of the shared launches, as its single-context launches would carry them
struct GroupMemberArgs {
  PairArgs P;
  TreeArgs T;             // T.out: the outputs of the pseudo-volume launch (forest_blocks set)
  double* components;
  int tree_blocks;        // forest workgroups of the cavity launch (its prep workgroups follow)
  int born_role;          // Born rows: the first mask tile (role_arg of k_rows<kBornRows, false, true>)
  int chain_role;         // chain-rule rows: the roles' LDS bytes
  int pseudo_blocks;      // workgroups of the member's pseudo-volume launch
  int out_role_bytes;     // version 0 output launch: the roles' LDS bytes
  int out_mask_from;      // ... and its first mask tile
};

// The kernel argument of a group launch (by value: a few hundred bytes)
struct GroupLaunch {
  int count;                             // members of the launch set
  int first[kMaxGroup + 1];              // first workgroup of every member; first[count] = the grid
  unsigned long long args[kMaxGroup];    // device address of every member's GroupMemberArgs (its parity's copy)
};
// The caller's output buffers of a call, which are not part of the blocks (TreeOutputs::force is null there): a caller may pass
// other output buffers in every call without a block being rewritten.  A second kernel argument of the launches that write them.
// (The positions are read through the block's PairArgs::pos / TreeArgs::pos: a caller that keeps its position buffers writes no
// block.)
struct GroupOutputs {
  unsigned long long force[kMaxGroup], energy[kMaxGroup];
};

// The members' plane buffers of a decomposition group (agbnp_hip_decompose_group): [4][N_m] each, a kernel argument of the plane
// launch alone -- like GroupOutputs, so that the members' argument blocks stay what a full or an energy-only group writes.
struct GroupPlanes {
  unsigned long long per_atom[kMaxGroup];
};

// The members' matrices and partitions of a pair-matrix group (agbnp_hip_pair_matrix_group): [S_m][S_m] each and the AtomSets
// its own matrix launch would take, a kernel argument of the matrix launch alone -- again so that the blocks stay what the other
// three kinds write.  16 x (32 + 8) bytes beside GroupLaunch's 200: far inside the 4096 bytes a kernel's arguments may take.
struct GroupMatrices {
  AtomSets sets[kMaxGroup];
  unsigned long long matrix[kMaxGroup];
};

// The members' parameter sets and output words of a perturbation group (agbnp_hip_perturbed_energies_group): the ParamSets its own
// perturbation launch would take and its [M_m] words, a kernel argument of that launch alone -- once more so that the blocks stay
// what the other kinds write.  16 x (32 + 8) bytes.
struct GroupPerturb {
  ParamSets sets[kMaxGroup];
  unsigned long long energies[kMaxGroup];
};

// (sv_large: the instantiations that also collect the enlarged-radius self volumes -- a decomposition group's cavity launch;
// single_gather: the forests' single-gather form, as the members' TreeArgs::single_gather says -- never both)
hipError_t launch_group_cavity_five(int variant, const GroupLaunch& G, size_t lds, hipStream_t st, bool sv_large = false, bool single_gather = false);
hipError_t launch_group_pseudo(int variant, const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st);
hipError_t launch_group_born_rows(const GroupLaunch& G, size_t lds, hipStream_t st);
hipError_t launch_group_gb(int gb_far, const GroupLaunch& G, hipStream_t st);
hipError_t launch_group_chain_rows(const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st);
hipError_t launch_group_outputs(const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st);
// energy-only groups (agbnp_hip_energy_group): the launches behind the cavity and Born-rows launches, which are the full group's
hipError_t launch_group_gb_energy(int gb_far, const GroupLaunch& G, hipStream_t st);
hipError_t launch_group_energy_roles(const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st);
hipError_t launch_group_outputs_energy(const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st);
hipError_t launch_group_put(const GroupMemberArgs& a, GroupMemberArgs* dst, hipStream_t st);
// decomposition groups (agbnp_hip_decompose_group; decompose_kernels.hip): the ONE plane launch behind an energy-only launch set,
// every member's grid of decompose_blocks(n, version) workgroups side by side
int decompose_blocks(int n, int version);
hipError_t launch_group_decompose(const GroupLaunch& G, const GroupPlanes& O, int version, hipStream_t st);
// pair-matrix groups (agbnp_hip_pair_matrix_group; pair_matrix_kernels.hip): the ONE matrix launch behind an energy-only launch
// set, on the same grids; lds: the largest depth^2 x 8 bytes over the members
hipError_t launch_group_pair_matrix(const GroupLaunch& G, const GroupMatrices& O, int version, size_t lds, hipStream_t st);
// perturbation groups (agbnp_hip_perturbed_energies_group; perturb_kernels.hip): the ONE perturbation launch behind an energy-only
// launch set, on the same grids, in the tier of the member with the most sets
hipError_t launch_group_perturb(const GroupLaunch& G, const GroupPerturb& O, int version, hipStream_t st);

#ifdef __HIP_DEVICE_COMPILE__
typedef const __attribute__((address_space(4))) GroupMemberArgs* GroupArgsPtr;
#endif

// the member of the workgroup and the workgroup's number inside that member's grid (both uniform)
__device__ __forceinline__ int group_index(const GroupLaunch& G, int& blk) {
  const int b = (int)blockIdx.x;
  int m = 0;
#pragma unroll
  for (int k = 1; k < kMaxGroup; k++)
    if (k < G.count && b >= G.first[k]) m = k;
  blk = b - G.first[m];
  return m;
}
// ... and that member's argument block
__device__ __forceinline__ const GroupMemberArgs& group_args(const GroupLaunch& G, int m) {
#ifdef __HIP_DEVICE_COMPILE__
  return *(const GroupMemberArgs*)(GroupArgsPtr)G.args[m];  // (constant address space: scalar loads, as for a kernel argument)
#else
  return *(const GroupMemberArgs*)G.args[m];
#endif
}
__device__ __forceinline__ const GroupMemberArgs& group_member(const GroupLaunch& G, int& blk) { return group_args(G, group_index(G, blk)); }

}  // namespace agbnp
