// Per-atom decomposition of an evaluation (agbnp_hip_decompose_*, include/agbnp_hip.h): ONE launch behind an energy-only-style
// evaluation of the context (engine_eval.hip, enqueue_decomposition), on the same stream.  It reads what the evaluation left --
// the Born radii, the self volumes with both sets of radii, the records {x, y, z, q} by atom -- and ADDS four planes of N
// doubles, term-major, atom order:
//   plane 0  cavity    nu_i (sv_large_i - sv_vdw_i), nu_i = gamma_i / roffset (0 for a hydrogen); the planes' sum is E_vol1 + E_vol2
//   plane 1  vdW       alpha_i / (B_i + 0.14 nm)^3
//   plane 2  GB self   k q_i^2 / B_i
//   plane 3  GB pair   k q_i sum_{j != i} q_j f_ij,  f_ij = 1 / sqrt(d^2 + B_i B_j exp(-d^2 / (4 B_i B_j))): every pair shared half and
//                      half between its ends, so that the plane sums to the GB pair energy 2k sum_{i<j} q_i q_j f_ij
// Version 0 has plane 0 only.  Every workgroup is gated on the evaluation's verdict words, as every other output is: a withheld
// evaluation adds nothing.
//
// The shared device code (rot1, gb_pair_terms, the status words' test, the parity rebase; the tile walk of pair_tile.h) is read as
// device functions, as the replica groups' unit reads it (group_args.h): this unit launches none of the kernels of pair_bodies.h.
#define AGBNP_GROUP_TU
#include "pair_tile.h"

namespace agbnp {

// ---- role workgroups: one thread per atom, planes 0-2 ---------------------------------------------------------------------
__device__ __forceinline__ void decompose_atoms(const PairArgs& P, int version, int i, double* __restrict__ per_atom) {
  if (i >= P.n) return;
  const size_t n = (size_t)P.n;
  const int h = P.a2h[i];
  if (h >= 0) hbm_add(&per_atom[i], P.gam_cav[h] * (P.sv_large[h] - P.sv_vdw[h]));
  if (version != 1) return;
  const double b = P.born[i], q = P.charge[i], bh = b + kHBRadius;
  hbm_add(&per_atom[n + i], P.alpha[i] / (bh * bh * bh));
  hbm_add(&per_atom[2 * n + i], kDielFactor * q * q / b);
}

// ---- tile workgroups: plane 3 ------------------------------------------------------------------------------------------------
// The tile walk of pair_tile.h: a pair is evaluated once and credited to both ends -- to the lane's own atom, and to the j atom,
// whose running sum travels round the wave by DPP rotation.  Two sums per lane where k_gb_tiles carries nine.
template <bool kCut>
__device__ __forceinline__ void decompose_tile(const PairArgs& P, int tile, double* __restrict__ plane) {
  __shared__ double s_red[4][2][64];
  PairTile W;
  if (!pair_tile_of(P.n, tile, W)) return;
  double ei = 0.0, ej = 0.0;  // sum q_i q_j f_ij of the lane's own atom / of the j atom in hand
  if (!walk_pair_tile<kCut>(P, W, [&](int, double s1) {
        ei += s1;
        ej = rot1(ej + s1);
      }))
    return;
  const int lane = W.lane, wave = W.wave;
  s_red[wave][0][lane] = ei;
  s_red[wave][1][(lane + W.start + W.nsteps) & 63] = ej;  // whose sum the lane holds after the rotations
  __syncthreads();
  if (wave >= 2) return;
  // wave 0 adds the sums of block I, wave 1 those of block J (the deterministic mode: a tile's totals are rounded to the
  // energies' quantum, so that the order of the atomics does not matter)
  const int a = 64 * (wave == 0 ? W.I : W.J) + lane;
  const double sum = (s_red[0][wave][lane] + s_red[1][wave][lane]) + (s_red[2][wave][lane] + s_red[3][wave][lane]);
  if (a < P.n) hbm_add(&plane[a], quantize(kDielFactor * sum, kQEnergy, P.det != 0));
}

template <bool kCut>
__global__ __launch_bounds__(256) void k_decompose(PairArgs P, int version, int role_blocks, double* __restrict__ per_atom) {
  rebase_for_parity(P, 1);  // (five-launch mode, the device names the set: behind the GB launch)
  if (evaluation_overflowed(P.estatus)) return;  // a withheld evaluation adds nothing (see energy_role)
  if ((int)blockIdx.x < role_blocks) return decompose_atoms(P, version, blockIdx.x * 256 + threadIdx.x, per_atom);
  decompose_tile<kCut>(P, (int)blockIdx.x - role_blocks, per_atom + 3 * (size_t)P.n);
}

// Decomposition groups (agbnp_hip_decompose_group; group_args.h, engine_group.hip): the plane launch of every member of a launch
// set in one grid.  A workgroup finds its member and its number inside that member's grid (group_index) and does there what
// k_decompose's workgroup of that number does, on the member's PairArgs out of its argument block: the member's first
// ceil(n / 256) workgroups are role workgroups, the rest are tiles.  Gated on that member's own verdict words.  Sharing members
// run the Reference semantics with the host-named set: no cutoff instantiation, no parity rebase.  The plane pointers travel in
// the launch's argument (GroupPlanes): the blocks are not touched.
__global__ __launch_bounds__(256) void k_group_decompose(GroupLaunch G, GroupPlanes O, int version) {
  int blk;
  const int m = group_index(G, blk);
  const PairArgs& P = group_args(G, m).P;
  if (evaluation_overflowed(P.estatus)) return;  // this member's evaluation was withheld: it adds nothing
  double* __restrict__ per_atom = reinterpret_cast<double*>(O.per_atom[m]);
  const int role_blocks = (P.n + 255) / 256;
  if (blk < role_blocks) return decompose_atoms(P, version, blk * 256 + (int)threadIdx.x, per_atom);
  decompose_tile<false>(P, blk - role_blocks, per_atom + 3 * (size_t)P.n);
}

// workgroups of a context's plane launch: the role workgroups, then (version 1) the tiles
int decompose_blocks(int n, int version) {
  const int nb = (n + 63) / 64;
  return (n + 255) / 256 + (version == 1 ? nb * (nb + 1) / 2 : 0);
}

hipError_t launch_group_decompose(const GroupLaunch& G, const GroupPlanes& O, int version, hipStream_t st) {
  hipLaunchKernelGGL(k_group_decompose, dim3(G.first[G.count]), dim3(256), 0, st, G, O, version);
  return hipGetLastError();
}

hipError_t launch_decompose(const PairArgs& P, int version, double* per_atom, hipStream_t st, Timeline* tl) {
  if (tl) {
    hipError_t m = tl->mark(kKDecompose, st);
    if (m != hipSuccess) return m;
  }
  const int role_blocks = (P.n + 255) / 256, tiles = decompose_blocks(P.n, version) - role_blocks;
  if (P.fast)
    hipLaunchKernelGGL(k_decompose<true>, dim3(role_blocks + tiles), dim3(256), 0, st, P, version, role_blocks, per_atom);
  else
    hipLaunchKernelGGL(k_decompose<false>, dim3(role_blocks + tiles), dim3(256), 0, st, P, version, role_blocks, per_atom);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return tl ? tl->mark(-1, st) : hipSuccess;
}

}  // namespace agbnp
