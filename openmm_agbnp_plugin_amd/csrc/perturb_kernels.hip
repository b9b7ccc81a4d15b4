// Perturbation energies of an evaluation (agbnp_hip_perturbed_energies_*, include/agbnp_hip.h): ONE launch behind the evaluation
// that a per-atom decomposition runs (engine_eval.hip, enqueue_launch), on the same stream.  The overlap trees, both sets of self
// volumes and the Born radii depend on the geometry and the radii alone, so the energy under another set m of
// (gamma, vdw_alpha, charge) is an explicit function of that set over what the evaluation left (the terms of k_decompose):
//   E_m = sum_i nu_i^m (sv_large_i - sv_vdw_i)                       nu = gamma / roffset, 0 for a hydrogen
//       + sum_i alpha_i^m / (B_i + 0.14 nm)^3  +  k sum_i (q_i^m)^2 / B_i
//       + 2k sum_{i<j} q_i^m q_j^m f_ij                               f_ij = 1 / sqrt(d^2 + B_i B_j exp(-d^2 / (4 B_i B_j)))
// With M sets (ParamSets: three [M][n] tables owned by the context) it ADDS E_0 .. E_{M-1} to the caller's [M] words.  Version 0
// has the first line only.  Every workgroup is gated on the evaluation's verdict words: a withheld evaluation adds nothing.
//
// The grid is k_decompose's: role workgroups (one thread per atom: the three per-atom terms of every set) and one workgroup per
// 64 x 64 tile, on the tile walk of pair_tile.h with the charge product replaced by the pair's 0/1 weight (kUnit), so that a met
// pair's value is w f_ij -- the FP64 exp and rsqrt -- formed ONCE and multiplied by M charge products: block J's charges of every
// set sit in LDS, doubled like the walk's own copy of the block, the lane's own in registers, and acc[m] += q_j^m w f_ij.  M is a
// compile-time tier (4, 8, 16; the sets beyond M carry zero charges and add nothing) so that the accumulators stay in registers.
// A workgroup sums its M totals in a fixed order and leaves with M atomics.  Deterministic mode: every total is rounded to the
// energies' quantum before its add, so that the order of the atomics does not matter.
#define AGBNP_GROUP_TU
#include "pair_tile.h"

namespace agbnp {

// ---- a workgroup's M sums ----------------------------------------------------------------------------------------------------
// e[m] of every thread of the workgroup of 256, summed in a fixed order (halves of a wave, then 16 threads per set over the 128
// partials, then their tree) and ADDED to out[m], m < sets.  s_part: [kM][128], free to be overwritten (the caller has put a
// barrier behind its last reader).
template <int kM>
__device__ __forceinline__ void perturb_leave(const double (&e)[kM], double (*s_part)[128], int sets, bool det, double* __restrict__ out) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int m = 0; m < kM; m++) {
    const double x = e[m] + __shfl_xor(e[m], 32, 64);
    if (lane < 32) s_part[m][32 * wave + lane] = x;
  }
  __syncthreads();
  if (t >= 16 * kM) return;  // (whole waves: kM is a multiple of 4)
  const int m = t >> 4, sub = t & 15;
  double x = 0.0;
#pragma unroll
  for (int k = 0; k < 8; k++) x += s_part[m][16 * k + sub];
  for (int off = 8; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  if (sub == 0 && m < sets && x != 0.0) hbm_add(&out[m], quantize(x, kQEnergy, det));
}

// ---- role workgroups: one thread per atom, the per-atom terms of every set ---------------------------------------------------------
template <int kM>
__device__ __forceinline__ void perturb_atoms(const PairArgs& P, const ParamSets& S, int version, int i, double (*s_part)[128],
                                              double* __restrict__ out) {
  const size_t n = (size_t)P.n;
  double e[kM];
#pragma unroll
  for (int m = 0; m < kM; m++) e[m] = 0.0;
  if (i < P.n) {
    const int h = P.a2h[i];
    const double area = h >= 0 ? P.sv_large[h] - P.sv_vdw[h] : 0.0;  // (times nu: the cavity term)
    double inv_bh3 = 0.0, self = 0.0;  // (version 0: the cavity term alone)
    if (version == 1) {
      const double b = P.born[i], bh = b + kHBRadius;
      inv_bh3 = 1.0 / (bh * bh * bh), self = kDielFactor / b;
    }
#pragma unroll
    for (int m = 0; m < kM; m++)
      if (m < S.num_sets) {
        const double q = S.charge[m * n + i];
        e[m] = S.nu[m * n + i] * area + S.alpha[m * n + i] * inv_bh3 + self * q * q;
      }
  }
  perturb_leave<kM>(e, s_part, S.num_sets, P.det != 0, out);
}

// ---- tile workgroups: the pair terms of every set --------------------------------------------------------------------------------
// s_q [kM][128]: block J's charges of every set, twice over -- entry j and j + 64 are atom 64 J + j (at 16 sets 16 KB, beside the
// walk's own 9 KB); the workgroup's partial sums afterwards, as in a role workgroup
template <bool kCut, int kM>
__device__ __forceinline__ void perturb_tile(const PairArgs& P, const ParamSets& S, int tile, double (*s_q)[128], double* __restrict__ out) {
  PairTile W;
  if (!pair_tile_of(P.n, tile, W)) return;
  const size_t n = (size_t)P.n;
  const int t = threadIdx.x, lane = W.lane;
  {
    const int a = 64 * W.J + lane;
    for (int m = t >> 6; m < kM; m += 4) {
      const double q = m < S.num_sets && a < P.n ? S.charge[m * n + a] : 0.0;
      s_q[m][lane] = s_q[m][lane + 64] = q;
    }
  }
  // (the walk's barrier stands between these writes and their readers)
  double qi[kM], acc[kM];
  {
    const int a = 64 * W.I + lane;
#pragma unroll
    for (int m = 0; m < kM; m++) {
      qi[m] = m < S.num_sets && a < P.n ? S.charge[m * n + a] : 0.0;
      acc[m] = 0.0;
    }
  }
  const int base = (lane + W.start) & 63;
  if (!walk_pair_tile<kCut, true>(P, W, [&](int k, double s1) {
#pragma unroll
        for (int m = 0; m < kM; m++) acc[m] = fma(s_q[m][base + k], s1, acc[m]);
      }))
    return;
  // a pair is met once and stands for both of its ends: 2k q_i q_j f_ij
#pragma unroll
  for (int m = 0; m < kM; m++) acc[m] *= (2.0 * kDielFactor) * qi[m];
  __syncthreads();  // every wave is done with s_q
  perturb_leave<kM>(acc, s_q, S.num_sets, P.det != 0, out);
}

template <bool kCut, int kM>
__global__ __launch_bounds__(256) void k_perturb(PairArgs P, ParamSets S, int version, int role_blocks, double* __restrict__ out) {
  rebase_for_parity(P, 1);  // (five-launch mode, the device names the set: behind the GB launch)
  if (evaluation_overflowed(P.estatus)) return;  // a withheld evaluation adds nothing (see energy_role)
  __shared__ double s_sets[kM][128];
  if ((int)blockIdx.x < role_blocks) return perturb_atoms<kM>(P, S, version, blockIdx.x * 256 + threadIdx.x, s_sets, out);
  perturb_tile<kCut, kM>(P, S, (int)blockIdx.x - role_blocks, s_sets, out);
}

// Perturbation groups (agbnp_hip_perturbed_energies_group; group_args.h, engine_group.hip): the perturbation launch of every
// member of a launch set in one grid, as k_group_decompose is the plane launch of every member.  A workgroup finds its member
// and its number inside that member's grid (group_index) and does there what k_perturb's workgroup of that number does, on the
// member's PairArgs out of its argument block and on the member's own tables and output words out of the launch's argument
// (GroupPerturb: the blocks are not touched).  Gated on that member's own verdict words.  Sharing members run the Reference
// semantics with the host-named set: no cutoff instantiation, no parity rebase.  The tier is that of the member with the most
// sets.
template <int kM>
__global__ __launch_bounds__(256) void k_group_perturb(GroupLaunch G, GroupPerturb O, int version) {
  int blk;
  const int m = group_index(G, blk);
  const PairArgs& P = group_args(G, m).P;
  if (evaluation_overflowed(P.estatus)) return;  // this member's evaluation was withheld: it adds nothing
  const ParamSets& S = O.sets[m];
  double* __restrict__ out = reinterpret_cast<double*>(O.energies[m]);
  const int role_blocks = (P.n + 255) / 256;
  __shared__ double s_sets[kM][128];
  if (blk < role_blocks) return perturb_atoms<kM>(P, S, version, blk * 256 + (int)threadIdx.x, s_sets, out);
  perturb_tile<false, kM>(P, S, blk - role_blocks, s_sets, out);
}

static_assert(sizeof(GroupLaunch) + sizeof(GroupPerturb) + sizeof(int) <= 4096, "a kernel's arguments take 4096 bytes at most");

// the compile-time tier of a number of sets
template <class F>
static void with_perturb_tier(int sets, F&& f) {
  if (sets <= 4) return f(std::integral_constant<int, 4>());
  if (sets <= 8) return f(std::integral_constant<int, 8>());
  f(std::integral_constant<int, kMaxParamSets>());
}

hipError_t launch_group_perturb(const GroupLaunch& G, const GroupPerturb& O, int version, hipStream_t st) {
  int most = 0;
  for (int k = 0; k < G.count; k++) most = std::max(most, O.sets[k].num_sets);
  with_perturb_tier(most, [&](auto tier) {
    hipLaunchKernelGGL(k_group_perturb<decltype(tier)::value>, dim3(G.first[G.count]), dim3(256), 0, st, G, O, version);
  });
  return hipGetLastError();
}

hipError_t launch_perturb(const PairArgs& P, const ParamSets& S, int version, double* out, hipStream_t st) {
  // k_decompose's grid: the role workgroups, then (version 1) the tiles
  const int role_blocks = (P.n + 255) / 256, blocks = decompose_blocks(P.n, version);
  with_perturb_tier(S.num_sets, [&](auto tier) {
    constexpr int kM = decltype(tier)::value;
    if (P.fast)
      hipLaunchKernelGGL((k_perturb<true, kM>), dim3(blocks), dim3(256), 0, st, P, S, version, role_blocks, out);
    else
      hipLaunchKernelGGL((k_perturb<false, kM>), dim3(blocks), dim3(256), 0, st, P, S, version, role_blocks, out);
  });
  return hipGetLastError();
}

}  // namespace agbnp
