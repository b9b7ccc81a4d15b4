// Replica groups (group_args.h, engine_group.hip agbnp_hip_execute_group): the kernels and launchers of the launches that several
// contexts share.  The kernel bodies are those of pair_bodies.h and tree_bodies.h, which this translation unit reads with
// the switch below set (group_args.h): k_gb_tiles, k_rows, k_outputs, k_tree_cavity_five and k_tree_pseudo are then device functions that take the
// workgroup's number inside a member's grid, and the kernels below call them.  A translation unit of its own, so that the
// kernels of pair_kernels.hip and tree_kernels.hip -- and the compiler's inlining decisions for them -- stay what they are.
#define AGBNP_GROUP_TU
#include "pair_bodies.h"
#include "tree_bodies.h"

namespace agbnp {

// ---- replica groups (group_args.h): the pair-stage launches of several contexts in one grid ---------------------------------
// The instantiations a sharing member launches alone: the five-launch mode's Born rows with their mask tiles, the Reference GB
// tiles, the chain-rule rows; version 0's output launch with its role workgroups and mask tiles.
__global__ __launch_bounds__(64 * kRowWaves, 6) void k_group_born_rows(GroupLaunch G) {
  int blk;
  const GroupMemberArgs& g = group_member(G, blk);
  k_rows<kBornRows, false, true, false>(g.P, nullptr, nullptr, g.born_role, (unsigned)blk, 0u);
}
template <bool kFar>
__global__ __launch_bounds__(256) void k_group_gb_tiles(GroupLaunch G) {
  int blk;
  const GroupMemberArgs& g = group_member(G, blk);
  const PairArgs& P = g.P;
  k_gb_tiles<false, false, kFar, false, false>(P.n, P.gb_items, (const double4*)P.aposq, (const double*)P.born_part, P.inv_rvdw, P.alpha, P.born,
                                               P.born_fp, P.brw, P.e_atom, P.gb_fx, P.egb_part, P, (unsigned)blk, 0u);
}
__global__ __launch_bounds__(64 * kRowWaves, 6) void k_group_chain_rows(GroupLaunch G, GroupOutputs O) {
  int blk;
  const int m = group_index(G, blk);
  const GroupMemberArgs& g = group_args(G, m);
  k_rows<kChainRows, false, false, false>(g.P, reinterpret_cast<double*>(O.energy[m]), g.components, g.chain_role, (unsigned)blk, 0u);
}
__global__ __launch_bounds__(256) void k_group_outputs(GroupLaunch G, GroupOutputs O) {
  int blk;
  const int m = group_index(G, blk);
  const GroupMemberArgs& g = group_args(G, m);
  k_outputs(g.P, 0, reinterpret_cast<double*>(O.force[m]), reinterpret_cast<double*>(O.energy[m]), g.components, g.out_role_bytes,
            g.out_mask_from, (unsigned)blk, 0u);
}
// ---- energy-only replica groups (agbnp_hip_energy_group): the launches behind the shared cavity and Born-rows launches ------
// They read the members' argument blocks as the full group's launches do and nothing a full group call does not put there: the
// roles' LDS bytes are those of the chain-rule launch (GroupMemberArgs::chain_role, as k_energy_roles takes them), the force-less
// output launch of version 0 has its first mask tile behind its two role workgroups, and TreeOutputs is not read.
// The GB stage's energy-only instantiation (the body launch_energy_only_stages launches for one context)
template <bool kFar>
__global__ __launch_bounds__(256) void k_group_gb_tiles_energy(GroupLaunch G) {
  int blk;
  const GroupMemberArgs& g = group_member(G, blk);
  const PairArgs& P = g.P;
  k_gb_tiles<false, false, kFar, false, true>(P.n, P.gb_items, (const double4*)P.aposq, (const double*)P.born_part, P.inv_rvdw, P.alpha, P.born,
                                              P.born_fp, P.brw, P.e_atom, P.gb_fx, P.egb_part, P, (unsigned)blk, 0u);
}
// The close of a version-1 member's energy-only evaluation, three workgroups per member exactly as in k_energy_roles
__global__ __launch_bounds__(256) void k_group_energy_roles(GroupLaunch G, GroupOutputs O) {
  extern __shared__ double2 s_dyn[];
  int blk;
  const int m = group_index(G, blk);
  const GroupMemberArgs& g = group_args(G, m);
  const PairArgs& P = g.P;
  if (blk == 0) return energy_role(P, 1, reinterpret_cast<double*>(O.energy[m]), g.components, reinterpret_cast<char*>(s_dyn));
  if (blk == 1) return dealing_role(P, reinterpret_cast<char*>(s_dyn), g.chain_role);
  if (threadIdx.x == 0 && P.rows_on) rows_close_evaluation(P.nl_flag, P.nl_nitems, P.row_target, P.gb_rows != 0);
}
// Version 0: the output launch in its force-less shape (two role workgroups, then the mask tiles)
__global__ __launch_bounds__(256) void k_group_outputs_energy(GroupLaunch G, GroupOutputs O) {
  int blk;
  const int m = group_index(G, blk);
  const GroupMemberArgs& g = group_args(G, m);
  k_outputs(g.P, 0, nullptr, reinterpret_cast<double*>(O.energy[m]), g.components, g.out_role_bytes, 2, (unsigned)blk, 0u);
}
// a member's argument block, rewritten in stream order (the new block travels as this launch's argument)
static_assert(sizeof(GroupMemberArgs) % 8 == 0 && sizeof(GroupMemberArgs) + 8 <= 4096, "the block travels as a kernel argument");
__global__ __launch_bounds__(256) void k_group_put(GroupMemberArgs a, GroupMemberArgs* __restrict__ dst) {
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&a);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(dst);
  for (int w = threadIdx.x; w < (int)(sizeof(GroupMemberArgs) / 8); w += 256) out[w] = src[w];
}

// ---- ... and their launchers: one launch per stage for every member of a launch set ---------------------------------------------
hipError_t launch_group_born_rows(const GroupLaunch& G, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(k_group_born_rows, dim3(G.first[G.count]), dim3(64 * kRowWaves), lds, st, G);
  return hipGetLastError();
}

hipError_t launch_group_gb(int gb_far, const GroupLaunch& G, hipStream_t st) {
  if (gb_far)
    hipLaunchKernelGGL(k_group_gb_tiles<true>, dim3(G.first[G.count]), dim3(256), 0, st, G);
  else
    hipLaunchKernelGGL(k_group_gb_tiles<false>, dim3(G.first[G.count]), dim3(256), 0, st, G);
  return hipGetLastError();
}

hipError_t launch_group_chain_rows(const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(k_group_chain_rows, dim3(G.first[G.count]), dim3(64 * kRowWaves), lds, st, G, O);
  return hipGetLastError();
}

hipError_t launch_group_outputs(const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(k_group_outputs, dim3(G.first[G.count]), dim3(256), lds, st, G, O);
  return hipGetLastError();
}

hipError_t launch_group_gb_energy(int gb_far, const GroupLaunch& G, hipStream_t st) {
  if (gb_far)
    hipLaunchKernelGGL(k_group_gb_tiles_energy<true>, dim3(G.first[G.count]), dim3(256), 0, st, G);
  else
    hipLaunchKernelGGL(k_group_gb_tiles_energy<false>, dim3(G.first[G.count]), dim3(256), 0, st, G);
  return hipGetLastError();
}

hipError_t launch_group_energy_roles(const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(k_group_energy_roles, dim3(G.first[G.count]), dim3(256), lds, st, G, O);
  return hipGetLastError();
}

hipError_t launch_group_outputs_energy(const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(k_group_outputs_energy, dim3(G.first[G.count]), dim3(256), lds, st, G, O);
  return hipGetLastError();
}

hipError_t launch_group_put(const GroupMemberArgs& a, GroupMemberArgs* dst, hipStream_t st) {
  hipLaunchKernelGGL(k_group_put, dim3(1), dim3(256), 0, st, a, dst);
  return hipGetLastError();
}

// ---- replica groups (group_args.h): the cavity and pseudo-volume launches of several contexts in one grid --------------------
// The instantiations of the five-launch mode with the host-named set (eager launches) and, for the pseudo-volume launch, the
// forces leaving with it: what a sharing member would launch alone.
// SV1: the instantiations of a decomposition group (agbnp_hip_decompose_group), which also collect the enlarged-radius self
// volumes, as k_tree_cavity_five's own SV1 instantiations do for one context
// At four waves per SIMD (128 VGPRs) the SV1 forms of the two smallest stores park two registers in scratch, as
// k_tree_cavity_five's do; these are asked for three (168 VGPRs) and keep everything in registers.  The 512-node store's four
// workgroups per CU are three waves per SIMD as it is; the 432-node store then holds four workgroups per CU where the other
// launches hold five -- a decomposition of a system with more than 1024 forests runs its cavity launch in more rounds.
constexpr int group_cavity_waves(int ncap, bool sv1) { return sv1 && ncap <= 512 ? 3 : tree_waves_per_simd(ncap); }
// SINGLE: the forests' single-gather form (tree_bodies.h), what a version-1 member would launch alone
template <int NCAP, int ACAP, int BS, bool SV1, bool SINGLE = false>
__global__ __launch_bounds__(BS, group_cavity_waves(NCAP, SV1)) void k_group_cavity_five(GroupLaunch G) {
  int blk;
  const GroupMemberArgs& g = group_member(G, blk);
  k_tree_cavity_five<NCAP, ACAP, BS, false, false, SV1, SINGLE>(g.T, g.P, g.tree_blocks, (unsigned)blk, 0u);
}
template <int NCAP, int ACAP, int BS, bool PIPE>
__global__ __launch_bounds__(BS, tree_waves_per_simd(NCAP)) void k_group_pseudo(GroupLaunch G, GroupOutputs O) {
  int blk;
  const int m = group_index(G, blk);
  const GroupMemberArgs& g = group_args(G, m);
  TreeArgs A = g.T;
  A.out.force = reinterpret_cast<double*>(O.force[m]);  // (the caller's outputs travel with the launch)
  k_tree_pseudo<NCAP, ACAP, BS, false, PIPE, false>(A, (unsigned)blk, (unsigned)g.pseudo_blocks);
}

// replica groups: one launch per stage for every member of a launch set (engine_group.hip, agbnp_hip_execute_group)
template <class K, class... Args>
static hipError_t launch_group(K kernel, const GroupLaunch& G, size_t lds, hipStream_t st, const Args&... args) {
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(G.first[G.count]), dim3(kBS), lds, st, G, args...);
  return hipGetLastError();
}

hipError_t launch_group_cavity_five(int variant, const GroupLaunch& G, size_t lds, hipStream_t st, bool sv_large, bool single_gather) {
  return with_tree_variant(variant, [&](auto v) {
    using V = decltype(v);
    if constexpr (V::kGlobal) {
      return hipErrorInvalidValue;
    } else if (single_gather) {
      if constexpr (TreeStore<V::kNodeCap, V::kAtomCap>::kPairGather) {
        if (!sv_large) return launch_group(k_group_cavity_five<V::kNodeCap, V::kAtomCap, kBS, false, true>, G, lds, st);
      }
      return hipErrorInvalidValue;
    } else if (sv_large)
      return launch_group(k_group_cavity_five<V::kNodeCap, V::kAtomCap, kBS, true>, G, lds, st);
    else
      return launch_group(k_group_cavity_five<V::kNodeCap, V::kAtomCap, kBS, false>, G, lds, st);
  });
}

// (a member's forces always leave with the launch)
hipError_t launch_group_pseudo(int variant, const GroupLaunch& G, const GroupOutputs& O, size_t lds, hipStream_t st) {
  return with_tree_variant(variant, [&](auto v) {
    using V = decltype(v);
    if constexpr (V::kGlobal)
      return hipErrorInvalidValue;
    else
      return launch_group(k_group_pseudo<V::kNodeCap, V::kAtomCap, kBS, !pseudo_forces_lean(V::kNodeCap)>, G, lds, st, O);
  });
}

}  // namespace agbnp
