// Overlap-tree stage, one context at a time (see tree_kernels.h for the algorithm; the kernel bodies are in tree_bodies.h):
// the six-launch cavity kernel, the capacity variants' numbers, the grids and every single-context launcher.
#include "tree_bodies.h"

namespace agbnp {

// the cavity launch of the six-launch mode (behind k_prep): every workgroup is a forest workgroup
// (SINGLE: the forests' single-gather form, tree_bodies.h)
template <int NCAP, int ACAP, int BS, bool GLOBAL, bool SV1, bool SINGLE = false>
__global__ __launch_bounds__(BS, tree_waves_per_simd(NCAP)) void k_tree_cavity(TreeArgs A) {
  cavity_forests<NCAP, ACAP, BS, GLOBAL, SV1, false, false, SINGLE>(A, (int)gridDim.x);
}

// ---- host-side launchers (the capacity variants: tree_bodies.h) -----------------------------------
size_t tree_variant_lds_bytes(int variant) {
  return with_tree_variant(variant, [](auto v) { return decltype(v)::kLdsBytes; });
}
size_t tree_variant_replay_bytes(int variant) {
  return with_tree_variant(variant, [](auto v) { return decltype(v)::kReplayBytes; });
}
size_t tree_variant_scratch_bytes(int variant) {
  return with_tree_variant(variant, [](auto v) { return decltype(v)::kScratchBytes; });
}
int tree_variant_node_cap(int variant) {
  return with_tree_variant(variant, [](auto v) { return decltype(v)::kNodeCap; });
}
int tree_variant_atom_cap(int variant) {
  return with_tree_variant(variant, [](auto v) { return decltype(v)::kAtomCap; });
}
// Which evaluations take the cavity launch in its single-gather form (cavity_forests, SINGLE) and so the replay with the combined
// weights: those that end in a replay (version 1) on a store that gathers over the membership list.  (A launch that is to collect
// the self volumes of pass 1 -- an analysis' request, the diagnostics -- needs that pass's own gather: the engine asks for both
// gathers there, TreeArgs::single_gather = 0.)
bool tree_single_gather(int variant, int version) {
  return version == 1 && with_tree_variant(variant, [](auto v) { return TreeStore<decltype(v)::kNodeCap, decltype(v)::kAtomCap>::kPairGather; });
}
// workgroups of the build kernel that a CU holds: LDS granules of 1280 B (128 per CU), 32 waves, the register budget
int tree_variant_wgs_per_cu(int variant) {
  const size_t bytes = tree_variant_lds_bytes(variant) + 16 + sizeof(int) * kPendCap;  // (+ the kernels' static LDS)
  if (tree_variant_lds_bytes(variant) == 0) return 1;
  const int by_lds = (int)(128 / ((bytes + 1279) / 1280));
  const int waves = kBS / 64;
  const int by_regs = 4 * tree_waves_per_simd(tree_variant_node_cap(variant)) / waves;
  return std::max(1, std::min(std::min(by_lds, by_regs), 32 / waves));
}

// workgroups of the five-launch mode's cavity launch: the forest workgroups, then the prep workgroups (replica groups lay the
// grids of several contexts side by side, engine_group.hip)
int tree_five_grid(int slots, const PairArgs& P) {
  const int work = std::max(std::max(P.n, P.nslots), (int)kStatEvalWords);
  return slots + (work + kBS - 1) / kBS;
}
// ... of the six-launch cavity launch and of the pseudo-volume launch's forest part.  slots: min(work slots that may be
// planned, workgroups the device keeps resident)
static int tree_forest_blocks(int variant, int global_grid, int slots, const TreeArgs& A) {
  return variant <= 3 ? slots : (global_grid < A.nh ? global_grid : A.nh);
}
// ... of the pseudo-volume launch: where the forces leave with it (TreeOutputs), one lane per atom follows the forest workgroups
int tree_pseudo_grid(int variant, int global_grid, int slots, const TreeArgs& A) {
  return tree_forest_blocks(variant, global_grid, slots, A) + (A.out.enabled ? (A.out.n + kBS - 1) / kBS : 0);
}

template <class K, class... Args>
static hipError_t launch_tree(K kernel, int grid, size_t lds, hipStream_t st, const Args&... args) {
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBS), lds, st, args...);
  return hipGetLastError();
}

hipError_t launch_tree_cavity(int variant, int global_grid, int slots, const TreeArgs& A, hipStream_t st, bool sv_large) {
  if (A.nh <= 0) return hipSuccess;
  const int grid = tree_forest_blocks(variant, global_grid, slots, A);
  return with_tree_variant(variant, [&](auto v) {
    using V = decltype(v);
    constexpr bool kPairs = TreeStore<V::kNodeCap, V::kAtomCap>::kPairGather;
    const bool sv1 = A.want_sv_large || sv_large;
    if (A.single_gather) {  // (the replay behind this launch takes the vdW-radius gradient along: the form that leaves it out)
      if constexpr (kPairs) {
        if (!sv1) return launch_tree(k_tree_cavity<V::kNodeCap, V::kAtomCap, kBS, false, false, true>, grid, V::kLdsBytes, st, A);
      }
      return hipErrorInvalidValue;
    }
    if (sv1)  // (the self volumes of pass 1, a diagnostic or a decomposition's request: a kernel of their own)
      return launch_tree(k_tree_cavity<V::kNodeCap, V::kAtomCap, kBS, V::kGlobal, true>, grid, V::kLdsBytes, st, A);
    return launch_tree(k_tree_cavity<V::kNodeCap, V::kAtomCap, kBS, V::kGlobal, false>, grid, V::kLdsBytes, st, A);
  });
}

// (round 6: every LDS variant -- rounds 5 left the mode for good at the first store beyond (512, 64))
// sv_large: the instantiations that also collect the enlarged-radius self volumes (a decomposition's request, engine_eval.hip;
// the caller's FP64 positions only: there is no OpenMM-buffer form of that call)
hipError_t launch_tree_cavity_five(int variant, int slots, const TreeArgs& A, const PairArgs& P, hipStream_t st, bool sv_large) {
  if (A.nh <= 0 || variant > 3) return hipErrorInvalidValue;  // (the engine leaves the mode before it gets here)
  const bool dev = A.five == 2, posq = A.posq != nullptr;
  if (sv_large && posq) return hipErrorInvalidValue;
  const int grid = tree_five_grid(slots, P);
  return with_tree_variant(variant, [&](auto v) {
    using V = decltype(v);
    if constexpr (V::kGlobal) {
      return hipErrorInvalidValue;
    } else {
      constexpr int N = V::kNodeCap, AC = V::kAtomCap;
      if (A.single_gather) {  // (as in launch_tree_cavity)
        if constexpr (TreeStore<N, AC>::kPairGather) {
          if (sv_large) return hipErrorInvalidValue;
          if (dev && posq) return launch_tree(k_tree_cavity_five<N, AC, kBS, true, true, false, true>, grid, V::kLdsBytes, st, A, P, slots);
          if (dev) return launch_tree(k_tree_cavity_five<N, AC, kBS, true, false, false, true>, grid, V::kLdsBytes, st, A, P, slots);
          if (posq) return launch_tree(k_tree_cavity_five<N, AC, kBS, false, true, false, true>, grid, V::kLdsBytes, st, A, P, slots);
          return launch_tree(k_tree_cavity_five<N, AC, kBS, false, false, false, true>, grid, V::kLdsBytes, st, A, P, slots);
        }
        return hipErrorInvalidValue;
      }
      if (sv_large && dev) return launch_tree(k_tree_cavity_five<N, AC, kBS, true, false, true>, grid, V::kLdsBytes, st, A, P, slots);
      if (sv_large) return launch_tree(k_tree_cavity_five<N, AC, kBS, false, false, true>, grid, V::kLdsBytes, st, A, P, slots);
      if (dev && posq) return launch_tree(k_tree_cavity_five<N, AC, kBS, true, true>, grid, V::kLdsBytes, st, A, P, slots);
      if (dev) return launch_tree(k_tree_cavity_five<N, AC, kBS, true, false>, grid, V::kLdsBytes, st, A, P, slots);
      if (posq) return launch_tree(k_tree_cavity_five<N, AC, kBS, false, true>, grid, V::kLdsBytes, st, A, P, slots);
      return launch_tree(k_tree_cavity_five<N, AC, kBS, false, false>, grid, V::kLdsBytes, st, A, P, slots);
    }
  });
}

hipError_t launch_tree_pseudo(int variant, int global_grid, int slots, const TreeArgs& A0, hipStream_t st) {
  if (A0.nh <= 0) return hipSuccess;
  TreeArgs A = A0;
  A.out.forest_blocks = tree_forest_blocks(variant, global_grid, slots, A);
  const int grid = tree_pseudo_grid(variant, global_grid, slots, A);
  return with_tree_variant(variant, [&](auto v) {
    using V = decltype(v);
    constexpr int N = V::kNodeCap, AC = V::kAtomCap;
    if constexpr (V::kGlobal) {
      return launch_tree(k_tree_pseudo<N, AC, kBS, true>, grid, 0, st, A);
    } else {
      auto launch = [&](auto pipe) {
        constexpr bool PIPE = decltype(pipe)::value;
        if (A.five == 2) return launch_tree(k_tree_pseudo<N, AC, kBS, false, PIPE, true>, grid, V::kReplayBytes, st, A);
        return launch_tree(k_tree_pseudo<N, AC, kBS, false, PIPE>, grid, V::kReplayBytes, st, A);
      };
      if constexpr (pseudo_forces_lean(N))
        if (A.out.enabled) return launch(std::false_type());
      return launch(std::true_type());
    }
  });
}

// Diagnostic build only (-DAGBNP_STAMPS): the stamps of this unit's kernels, read back (and cleared)
#ifdef AGBNP_STAMPS
extern "C" void agbnp_debug_stamps(unsigned long long* out, int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 16);
  if (reset) {
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z));
  }
}
extern "C" void agbnp_debug_wg_log(unsigned long long* out, int slots) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_log), sizeof(unsigned long long) * 24 * (size_t)(slots < kWgLogSlots ? slots : kWgLogSlots));
}
extern "C" void agbnp_debug_stamps_slowest(unsigned long long* out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_slowest), sizeof(unsigned long long) * 24);
}
extern "C" void agbnp_debug_stamps_max(unsigned long long* out, int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_max), sizeof(unsigned long long) * 16);
  if (reset) {
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_max), z, sizeof(z));
  }
}
#endif

}  // namespace agbnp
