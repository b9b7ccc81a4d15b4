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
// The shared device code (rot1, gb_pair_terms, the status words' test, the parity rebase) is read as device functions, as the
// replica groups' unit reads it (group_args.h): this unit launches none of the kernels of pair_bodies.h.
#define AGBNP_GROUP_TU
#include "pair_bodies.h"

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
// All 64 x 64 block pairs (I <= J) of the atoms in atom order, numbered by arithmetic from the workgroup's number (rows of the
// upper triangle laid end to end, as neighbor_tile does): no item list -- neither the row form nor the fast mode keeps one of
// the GB stage.  The pair step is k_gb_tiles': lane l of every wave keeps atom 64 I + l, meets a quarter of block J in cyclic
// order from a doubled copy of the block in LDS, and the j atom's running sum travels round the wave by DPP rotation, so that a
// pair is evaluated once and credited to both ends.  Two sums per lane where k_gb_tiles carries nine.
// kCut (fast mode): a pair beyond the cutoff carries a zero charge product, as in k_gb_tiles<kCut>; a tile whose blocks' boxes
// are further apart than the cutoff leaves before its walk (the boxes are formed here: the fast mode's row form keeps none).
template <bool kCut>
__device__ __forceinline__ void decompose_tile(const PairArgs& P, int tile, double* __restrict__ plane) {
  __shared__ double2 s_xy[128], s_zq[128], s_bb[128];  // block J twice over: entry m and m + 64 are atom 64 J + m
  __shared__ double2 s_ixy[64], s_izq[64], s_ibc[64];  // block I: {x, y}, {z, q}, {B, -log2(e)/(4 B)}
  __shared__ double s_red[4][2][64];
  __shared__ double s_box[2][6];
  const int n = P.n, nb = (n + 63) >> 6;
  if (tile >= nb * (nb + 1) / 2) return;
  int I = (int)(0.5 * ((double)(2 * nb + 1) - sqrt((double)(2 * nb + 1) * (double)(2 * nb + 1) - 8.0 * (double)tile)));
  I = max(0, min(I, nb - 1));
  while (I > 0 && I * nb - I * (I - 1) / 2 > tile) I--;  // (guards against rounding)
  while (I + 1 < nb && (I + 1) * nb - (I + 1) * I / 2 <= tile) I++;
  const int J = I + (tile - (I * nb - I * (I - 1) / 2));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool diag = I == J;
  if (wave < 2) {  // wave 0 prepares block J, wave 1 block I
    const int a = 64 * (wave == 0 ? J : I) + lane;
    const bool va = a < n;
    const int ac = va ? a : n - 1;
    const double4 pa = P.aposq[ac];
    const double br = P.born[ac], inv_br = 1.0 / br;
    const double qa = va ? pa.w : 0.0;  // zero charge switches a padded atom off
    if (wave == 0) {
      s_xy[lane] = s_xy[lane + 64] = make_double2(pa.x, pa.y);
      s_zq[lane] = s_zq[lane + 64] = make_double2(pa.z, qa);
      s_bb[lane] = s_bb[lane + 64] = make_double2(br, inv_br);
    } else {
      s_ixy[lane] = make_double2(pa.x, pa.y);
      s_izq[lane] = make_double2(pa.z, qa);
      s_ibc[lane] = make_double2(br, (-0.25 * 1.4426950408889634074) * inv_br);
    }
    if (kCut && !diag) {  // the block's bounding box (a padded lane repeats atom n - 1: inside the box)
      double lo[3] = {pa.x, pa.y, pa.z}, hi[3] = {pa.x, pa.y, pa.z};
      for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; d++) {
          lo[d] = fmin(lo[d], __shfl_xor(lo[d], off, 64));
          hi[d] = fmax(hi[d], __shfl_xor(hi[d], off, 64));
        }
      if (lane == 0)
        for (int d = 0; d < 3; d++) s_box[wave][d] = lo[d], s_box[wave][3 + d] = hi[d];
    }
  }
  __syncthreads();
  if (kCut && !diag) {
    if (box_gap2(&s_box[0][0], 0, 1) >= P.gb_cut2) return;  // (the same for every lane of the workgroup)
  }
  // the four waves take a quarter of the cyclic distances each (diagonal tile: distances 1..32, 8 per wave)
  const int nsteps = diag ? 8 : 16;
  const int start = (diag ? 1 : 0) + nsteps * wave;  // cyclic offset of the first j met by lane l
  const double2 ixy = s_ixy[lane], izq = s_izq[lane], ibc = s_ibc[lane];
  const double xi = ixy.x, yi = ixy.y, zi = izq.x, qi = izq.y, bi = ibc.x, ci = ibc.y;
  // diagonal tile, cyclic distance 32 (the last step of the last wave): the pair (l, l + 32) is met from the lower lane only,
  // and that one meeting credits both of its ends
  const int masked_step = diag ? 32 - start : -1;
  const double qlast = lane >= 32 ? 0.0 : qi;
  const int base = (lane + start) & 63;
  const double2* __restrict__ jxy = s_xy + base;
  const double2* __restrict__ jzq = s_zq + base;
  const double2* __restrict__ jbb = s_bb + base;
  double ei = 0.0, ej = 0.0;  // sum q_i q_j f_ij of the lane's own atom / of the j atom in hand
#pragma unroll 8
  for (int k = 0; k < nsteps; k++) {
    const double2 xy = jxy[k], zq = jzq[k], bj = jbb[k];
    const double dx = xy.x - xi, dy = xy.y - yi, dz = zq.x - zi;
    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
    double qq = (k == masked_step ? qlast : qi) * zq.y;
    if (kCut) qq = d2 < P.gb_cut2 ? qq : 0.0;
    const GbPairTerms<double> t = gb_pair_terms(d2, bi * bj.x, ci * bj.y, qq);  // (only s1 is used: the rest is dropped)
    ei += t.s1;
    ej = rot1(ej + t.s1);
  }
  s_red[wave][0][lane] = ei;
  s_red[wave][1][(lane + start + nsteps) & 63] = ej;  // whose sum the lane holds after the rotations
  __syncthreads();
  if (wave >= 2) return;
  // wave 0 adds the sums of block I, wave 1 those of block J (the deterministic mode: a tile's totals are rounded to the
  // energies' quantum, so that the order of the atomics does not matter)
  const int a = 64 * (wave == 0 ? I : J) + lane;
  const double sum = (s_red[0][wave][lane] + s_red[1][wave][lane]) + (s_red[2][wave][lane] + s_red[3][wave][lane]);
  if (a < n) hbm_add(&plane[a], quantize(kDielFactor * sum, kQEnergy, P.det != 0));
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
