// Set-pair interaction matrix of an evaluation (agbnp_hip_pair_matrix_*, include/agbnp_hip.h): ONE launch behind the evaluation
// that a per-atom decomposition runs (engine_eval.hip, enqueue_decomposition), on the same stream.  With the atoms partitioned
// into S sets (agbnp_hip_set_atom_sets) and T the per-atom terms of k_decompose, it ADDS to M[S][S], row-major:
//   M[a][a]  sum_{i in a} (T0 + T1 + T2)_i  +  k sum_{i != j, both in a} q_i q_j f_ij        (ordered pairs)
//   M[a][b]  k sum_{i in a, j in b} q_i q_j f_ij  =  M[b][a]
// so that row a sums to the set's share of the four planes and the whole matrix to the energy.  Version 0 has the cavity term
// on the diagonal only.  Every workgroup is gated on the evaluation's verdict words: a withheld evaluation adds nothing.
//
// The grid is k_decompose's: role workgroups (one thread per atom) and one workgroup per 64 x 64 tile, on the tile walk of
// pair_tile.h.  What differs is where a pair's value goes: every met pair (i, j) adds k s1 to M[s_i][s_j] and to M[s_j][s_i],
// which covers diagonal tiles, off-diagonal tiles and sets that span both blocks alike.  No pair goes to HBM by itself.  A block
// of 64 atoms names few sets (AtomSets: a residue partition about 9, never more than 64), so a tile owns an accumulator
// acc[nI][nJ] in LDS -- by the places of the sets in the two blocks' lists -- and leaves with 2 nI nJ HBM atomics; and atoms of
// a set mostly lie in runs, so a lane sums while the j atom's place stays what it was and sends a run, not a pair, to LDS.
// Deterministic mode: atomics arrive in any order, so every value that enters one, in LDS or HBM, is a multiple of the
// energies' quantum (sums of which are exact): the matrix is bit-identical from run to run.
#define AGBNP_GROUP_TU
#include "pair_tile.h"

namespace agbnp {

// ---- role workgroups: one thread per atom, T0 + T1 + T2 to the diagonal -------------------------------------------------------
// A workgroup holds four blocks: the terms meet in LDS by (block, place), and every set of a block leaves once.
__device__ __forceinline__ void matrix_atoms(const PairArgs& P, const AtomSets& A, int version, int first_block,
                                             double* __restrict__ matrix) {
  __shared__ double s_diag[4][kSetBlock];
  const int t = threadIdx.x, i = kSetBlock * first_block + t, b = first_block + (t >> 6), place = t & 63;
  const int nb = (P.n + kSetBlock - 1) / kSetBlock;
  s_diag[t >> 6][place] = 0.0;
  __syncthreads();
  if (i < P.n) {
    const int h = P.a2h[i];
    double term = h >= 0 ? P.gam_cav[h] * (P.sv_large[h] - P.sv_vdw[h]) : 0.0;
    if (version == 1) {
      const double br = P.born[i], q = P.charge[i], bh = br + kHBRadius;
      term += P.alpha[i] / (bh * bh * bh) + kDielFactor * q * q / br;
    }
    if (term != 0.0) lds_add(&s_diag[t >> 6][A.rank[i]], quantize(term, kQEnergy, P.det != 0));
  }
  __syncthreads();
  if (b < nb && place < A.block_count[b]) {
    const double v = s_diag[t >> 6][place];
    const size_t a = (size_t)A.block_sets[b * kSetBlock + place];
    if (v != 0.0) hbm_add(&matrix[a * (size_t)A.num_sets + a], v);
  }
}

// ---- tile workgroups: the pair terms -----------------------------------------------------------------------------------------
template <bool kCut>
__device__ __forceinline__ void matrix_tile(const PairArgs& P, const AtomSets& A, int tile, double* __restrict__ matrix) {
  extern __shared__ double s_acc[];                 // [nI][nJ], by the sets' places in the two blocks' lists
  __shared__ unsigned char s_jplace[2 * kSetBlock];  // block J twice over, as the walk's copy of the block
  __shared__ int s_sets[2][kSetBlock];               // the lists of block I and block J
  PairTile W;
  if (!pair_tile_of(P.n, tile, W)) return;
  const int t = threadIdx.x, nI = A.block_count[W.I], nJ = A.block_count[W.J];
  for (int c = t; c < nI * nJ; c += 256) s_acc[c] = 0.0;
  if (t < 2 * kSetBlock) s_jplace[t] = A.rank[kSetBlock * W.J + (t & 63)];
  else s_sets[(t >> 6) - 2][t & 63] = A.block_sets[(t < 3 * kSetBlock ? W.I : W.J) * kSetBlock + (t & 63)];
  // (the walk's barrier stands between these writes and their readers)
  const bool det = P.det != 0;
  double* __restrict__ row = s_acc + (int)A.rank[kSetBlock * W.I + W.lane] * nJ;
  const unsigned char* __restrict__ jplace = s_jplace + ((W.lane + W.start) & 63);
  int place = -1;    // of the j atoms of the run in hand
  double run = 0.0;  // sum q_i q_j f_ij over the run
  auto flush = [&]() {
    if (run != 0.0) lds_add(&row[place], quantize(kDielFactor * run, kQEnergy, det));
  };
  if (!walk_pair_tile<kCut>(P, W, [&](int k, double s1) {
        const int pj = jplace[k];
        if (pj != place) {
          flush();
          place = pj;
          run = 0.0;
        }
        run += s1;
      }))
    return;
  flush();
  __syncthreads();
  // cell (p, q) leaves for M[sI_p][sJ_q] and M[sJ_q][sI_p] (one set on both sides: both are the same word)
  const size_t S = (size_t)A.num_sets;
  for (int c = t; c < nI * nJ; c += 256) {
    const double v = s_acc[c];
    if (v == 0.0) continue;
    const size_t a = (size_t)s_sets[0][c / nJ], b = (size_t)s_sets[1][c % nJ];
    if (a == b) {
      hbm_add(&matrix[a * S + a], 2.0 * v);
    } else {
      hbm_add(&matrix[a * S + b], v);
      hbm_add(&matrix[b * S + a], v);
    }
  }
}

template <bool kCut>
__global__ __launch_bounds__(256) void k_pair_matrix(PairArgs P, AtomSets A, int version, int role_blocks, double* __restrict__ matrix) {
  rebase_for_parity(P, 1);  // (five-launch mode, the device names the set: behind the GB launch)
  if (evaluation_overflowed(P.estatus)) return;  // a withheld evaluation adds nothing (see energy_role)
  if ((int)blockIdx.x < role_blocks) return matrix_atoms(P, A, version, 4 * (int)blockIdx.x, matrix);
  matrix_tile<kCut>(P, A, (int)blockIdx.x - role_blocks, matrix);
}

// Pair-matrix groups (agbnp_hip_pair_matrix_group; group_args.h, engine_group.hip): the matrix launch of every member of a launch
// set in one grid, as k_group_decompose is the plane launch of every member.  A workgroup finds its member and its number inside
// that member's grid (group_index) and does there what k_pair_matrix's workgroup of that number does, on the member's PairArgs
// out of its argument block and on the member's own partition and matrix out of the launch's argument (GroupMatrices: the blocks
// are not touched).  Gated on that member's own verdict words.  Sharing members run the Reference semantics with the host-named
// set: no cutoff instantiation, no parity rebase.  The dynamic LDS is sized for the deepest partition of the set; a tile uses
// the first nI nJ words of it, by its own member's counts.
__global__ __launch_bounds__(256) void k_group_pair_matrix(GroupLaunch G, GroupMatrices O, int version) {
  int blk;
  const int m = group_index(G, blk);
  const PairArgs& P = group_args(G, m).P;
  if (evaluation_overflowed(P.estatus)) return;  // this member's evaluation was withheld: it adds nothing
  const AtomSets& A = O.sets[m];
  double* __restrict__ matrix = reinterpret_cast<double*>(O.matrix[m]);
  const int role_blocks = (P.n + 255) / 256;
  if (blk < role_blocks) return matrix_atoms(P, A, version, 4 * blk, matrix);
  matrix_tile<false>(P, A, blk - role_blocks, matrix);
}

static_assert(sizeof(GroupLaunch) + sizeof(GroupMatrices) + sizeof(int) <= 4096, "a kernel's arguments take 4096 bytes at most");

hipError_t launch_group_pair_matrix(const GroupLaunch& G, const GroupMatrices& O, int version, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(k_group_pair_matrix, dim3(G.first[G.count]), dim3(256), lds, st, G, O, version);
  return hipGetLastError();
}

int atom_set_tables(int n, const int* set_of_atom, std::vector<unsigned char>& rank, std::vector<int>& block_sets,
                    std::vector<int>& block_count) {
  const int nb = (n + kSetBlock - 1) / kSetBlock;
  rank.assign((size_t)nb * kSetBlock, 0);
  block_sets.assign((size_t)nb * kSetBlock, 0);
  block_count.assign(nb, 0);
  int depth = 0;
  for (int b = 0; b < nb; b++) {
    int* list = &block_sets[(size_t)b * kSetBlock];
    int& count = block_count[b];
    for (int i = b * kSetBlock; i < std::min(n, (b + 1) * kSetBlock); i++) {
      int place = 0;
      while (place < count && list[place] != set_of_atom[i]) place++;
      if (place == count) list[count++] = set_of_atom[i];
      rank[i] = (unsigned char)place;
    }
    depth = std::max(depth, count);
  }
  return depth;
}

hipError_t launch_pair_matrix(const PairArgs& P, const AtomSets& A, int version, double* matrix, hipStream_t st, Timeline* tl) {
  if (tl) {
    hipError_t m = tl->mark(kKPairMatrix, st);
    if (m != hipSuccess) return m;
  }
  // k_decompose's grid: the role workgroups, then (version 1) the tiles
  const int nb = (P.n + kSetBlock - 1) / kSetBlock;
  const int role_blocks = (P.n + 255) / 256, tiles = version == 1 ? nb * (nb + 1) / 2 : 0;
  const size_t lds = sizeof(double) * (size_t)A.depth * (size_t)A.depth;  // at most 32 KB beside the tile's own 10 KB
  if (P.fast)
    hipLaunchKernelGGL(k_pair_matrix<true>, dim3(role_blocks + tiles), dim3(256), lds, st, P, A, version, role_blocks, matrix);
  else
    hipLaunchKernelGGL(k_pair_matrix<false>, dim3(role_blocks + tiles), dim3(256), lds, st, P, A, version, role_blocks, matrix);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return tl ? tl->mark(-1, st) : hipSuccess;
}

}  // namespace agbnp
