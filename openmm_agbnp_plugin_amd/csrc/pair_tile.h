// The all-pairs 64 x 64 tile walk of the analysis launches (k_decompose, decompose_kernels.hip; k_pair_matrix,
// pair_matrix_kernels.hip; k_perturb, perturb_kernels.hip): which pair of blocks a workgroup has, and the GB pair step over it.  What a launch does with a met
// pair's value is its own (the `met` argument): the walk is said once.
//
// All 64 x 64 block pairs (I <= J) of the atoms in atom order, numbered by arithmetic from the workgroup's number (rows of the
// upper triangle laid end to end, as neighbor_tile does): no item list -- neither the row form nor the fast mode keeps one of
// the GB stage.  The pair step is k_gb_tiles': lane l of every wave keeps atom 64 I + l and meets a quarter of block J in cyclic
// order from a doubled copy of the block in LDS, so that a pair is evaluated once.
// kCut (fast mode): a pair beyond the cutoff carries a zero charge product, as in k_gb_tiles<kCut>; a tile whose blocks' boxes
// are further apart than the cutoff leaves before its walk (the boxes are formed here: the fast mode's row form keeps none).
#pragma once
#include "pair_bodies.h"

namespace agbnp {

struct PairTile {
  int I, J;     // the blocks, I <= J
  bool diag;    // I == J: cyclic distances 1..32, the pair (l, l + 32) met from the lower lane only
  int lane, wave;
  int nsteps;   // steps of a wave's walk
  int start;    // cyclic offset of the first j met by lane l: step k meets atom 64 J + ((lane + start + k) & 63)
};

// the tile of a workgroup; false: the launch has no such tile
__device__ __forceinline__ bool pair_tile_of(int n, int tile, PairTile& W) {
  const int nb = (n + 63) >> 6;
  if (tile >= nb * (nb + 1) / 2) return false;
  int I = (int)(0.5 * ((double)(2 * nb + 1) - sqrt((double)(2 * nb + 1) * (double)(2 * nb + 1) - 8.0 * (double)tile)));
  I = max(0, min(I, nb - 1));
  while (I > 0 && I * nb - I * (I - 1) / 2 > tile) I--;  // (guards against rounding)
  while (I + 1 < nb && (I + 1) * nb - (I + 1) * I / 2 <= tile) I++;
  W.I = I;
  W.J = I + (tile - (I * nb - I * (I - 1) / 2));
  W.diag = W.I == W.J;
  W.lane = threadIdx.x & 63;
  W.wave = threadIdx.x >> 6;
  // the four waves take a quarter of the cyclic distances each (diagonal tile: distances 1..32, 8 per wave)
  W.nsteps = W.diag ? 8 : 16;
  W.start = (W.diag ? 1 : 0) + W.nsteps * W.wave;
  return true;
}

// The walk of a workgroup of 256 over its tile: met(k, s1) at step k of the lane's walk, s1 = q_i q_j f_ij of the pair met there
// (0 for a padded atom, for a pair beyond the cutoff, and for the pair that the other lane credits).  Holds one barrier, which
// every thread of the workgroup reaches; false (for the whole workgroup): the tile lies beyond the cutoff, nothing was met.
// kUnit (k_perturb, perturb_kernels.hip: many charge tables over one walk): every real atom carries the charge 1, so that the
// product is the pair's 0/1 weight -- 0 in exactly the three cases above -- and s1 = w f_ij.
template <bool kCut, bool kUnit = false, class Met>
__device__ __forceinline__ bool walk_pair_tile(const PairArgs& P, const PairTile& W, Met&& met) {
  __shared__ double2 s_xy[128], s_zq[128], s_bb[128];  // block J twice over: entry m and m + 64 are atom 64 J + m
  __shared__ double2 s_ixy[64], s_izq[64], s_ibc[64];  // block I: {x, y}, {z, q}, {B, -log2(e)/(4 B)}
  __shared__ double s_box[2][6];
  const int n = P.n, lane = W.lane, wave = W.wave;
  if (wave < 2) {  // wave 0 prepares block J, wave 1 block I
    const int a = 64 * (wave == 0 ? W.J : W.I) + lane;
    const bool va = a < n;
    const int ac = va ? a : n - 1;
    const double4 pa = P.aposq[ac];
    const double br = P.born[ac], inv_br = 1.0 / br;
    const double qa = va ? (kUnit ? 1.0 : pa.w) : 0.0;  // zero charge switches a padded atom off
    if (wave == 0) {
      s_xy[lane] = s_xy[lane + 64] = make_double2(pa.x, pa.y);
      s_zq[lane] = s_zq[lane + 64] = make_double2(pa.z, qa);
      s_bb[lane] = s_bb[lane + 64] = make_double2(br, inv_br);
    } else {
      s_ixy[lane] = make_double2(pa.x, pa.y);
      s_izq[lane] = make_double2(pa.z, qa);
      s_ibc[lane] = make_double2(br, (-0.25 * 1.4426950408889634074) * inv_br);
    }
    if (kCut && !W.diag) {  // the block's bounding box (a padded lane repeats atom n - 1: inside the box)
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
  if (kCut && !W.diag) {
    if (box_gap2(&s_box[0][0], 0, 1) >= P.gb_cut2) return false;  // (the same for every lane of the workgroup)
  }
  const double2 ixy = s_ixy[lane], izq = s_izq[lane], ibc = s_ibc[lane];
  const double xi = ixy.x, yi = ixy.y, zi = izq.x, qi = izq.y, bi = ibc.x, ci = ibc.y;
  // diagonal tile, cyclic distance 32 (the last step of the last wave): the pair (l, l + 32) is met from the lower lane only,
  // and that one meeting credits both of its ends
  const int masked_step = W.diag ? 32 - W.start : -1;
  const double qlast = lane >= 32 ? 0.0 : qi;
  const int base = (lane + W.start) & 63;
  const double2* __restrict__ jxy = s_xy + base;
  const double2* __restrict__ jzq = s_zq + base;
  const double2* __restrict__ jbb = s_bb + base;
#pragma unroll 8
  for (int k = 0; k < W.nsteps; k++) {
    const double2 xy = jxy[k], zq = jzq[k], bj = jbb[k];
    const double dx = xy.x - xi, dy = xy.y - yi, dz = zq.x - zi;
    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
    double qq = (k == masked_step ? qlast : qi) * zq.y;
    if (kCut) qq = d2 < P.gb_cut2 ? qq : 0.0;
    const GbPairTerms<double> t = gb_pair_terms(d2, bi * bj.x, ci * bj.y, qq);  // (only s1 is used: the rest is dropped)
    met(k, t.s1);
  }
  return true;
}

}  // namespace agbnp
