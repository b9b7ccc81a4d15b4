// Pair stages of AGBNP1 on gfx950, one context at a time: inverse Born radii, GB pair energy/forces, Born-radius chain-rule
// forces, plus the per-atom glue between them.  The device code these kernels share with the replica groups' (k_gb_tiles,
// k_rows, k_outputs and everything below them; the reference semantics and the machine mapping) is in pair_bodies.h; here
// are the kernels only a single context launches, every single-context launcher and the launch shapes.
#include "pair_bodies.h"

namespace agbnp {

// ---- geometry in, accumulators cleared (neighbor_tile: pair_bodies.h) ---------------------------------------------------
__global__ __launch_bounds__(256) void k_prep(PairArgs P, int prep_blocks) {
  if ((int)blockIdx.x >= prep_blocks) return neighbor_tile(P, blockIdx.x - prep_blocks);
  prep_atoms(P, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.x == 0, false);
}

// five-launch mode: the neighbour masks alone (a launch of its own, only when the masks in hand have gone stale), and where
// the heavy atoms are while they are laid down
__global__ __launch_bounds__(256) void k_masks(PairArgs P, int ref_blocks) {
  if ((int)blockIdx.x >= ref_blocks) return neighbor_tile(P, blockIdx.x - ref_blocks);
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= P.nh) return;
  const Pos3 r = heavy_position(P, h);
  P.mask_ref[3 * h] = r.x;
  P.mask_ref[3 * h + 1] = r.y;
  P.mask_ref[3 * h + 2] = r.z;
}

// ---- descreening sums of the inverse Born radii, 64x64 tiles in "pair order" with range culling -------------
// Reference loop (ReferenceAGBNPKernels.cpp:435-449): sum_i over all atoms, heavy j != i, d < 2 nm:
//   born_part_i += s_j Q(d; type_i, type_j)       s_j = selfvol_j / (4 pi R_j^3 / 3)   (:420-433)
// Only heavy atoms descreen, so the atoms are walked in pair order (pslot): all heavy atoms first, then all
// hydrogens, each group padded to whole blocks of 64 (slot h of a heavy block IS heavy atom h).  Two kinds of tiles:
//   heavy x heavy  symmetric tiles (I <= J), every unordered pair met once, both directions (two look-ups)
//   heavy x H      full tiles, one direction (the heavy atom descreens the hydrogen, one look-up)
// One workgroup = one tile, four waves of a quarter of the cyclic distances each; block I in registers, the
// static record of block J from a doubled LDS copy, the running sum of the j atom travels by DPP rotation.  A
// tile whose two bounding boxes are more than the table's 2 nm reach apart exits at once.
template <bool kBoth>
__device__ __forceinline__ void born_walk(double& sum_i, double& sum_j, const double2* __restrict__ s_lut,
                                          const double2* __restrict__ jxy, const double2* __restrict__ jzs,
                                          const double* __restrict__ jty, double xi, double yi, double zi, double si, int row,
                                          int tsr, int nsteps, int masked_step, bool vi, bool lower, int ntj, double range2) {
#pragma unroll 4
  for (int k = 0; k < nsteps; k++) {
    const double2 xy = jxy[k], zs = jzs[k];
    const double ty = jty[k];
    const double dx = xy.x - xi, dy = xy.y - yi, dz = zs.x - zi;
    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
    const int tj = __double2loint(ty);  // screened type | screener type << 16
    if (d2 < range2 && vi && __double2hiint(ty) >= 0 && (k != masked_step || lower)) {
      const double d = d2 * rsqrt_pos(d2);
      sum_j = fma(si, spline_value(s_lut, ((tj & 0xffff) * ntj + tsr) * kLutStride, d), sum_j);   // i descreens j
      if (kBoth) sum_i = fma(zs.y, spline_value(s_lut, (row + (tj >> 16)) * kLutStride, d), sum_i);  // j descreens i
    }
    sum_j = rot1(sum_j);
  }
}

__global__ __launch_bounds__(256) void k_born_tiles(int nh, int nhb, int ntj, int lut_entries, const int* __restrict__ items,
                                                   const int* __restrict__ pslot, const double* __restrict__ pbox,
                                                   const double4* __restrict__ prec, const double* __restrict__ sv_vdw,
                                                   const double* __restrict__ inv_vol_h, const double2* __restrict__ lut,
                                                   double* __restrict__ born_part, double range2, int det, int cull_first) {
  extern __shared__ double2 s_lut[];
  __shared__ double2 s_xy[128], s_zs[128];  // block J twice over: {x, y}, {z, s}
  __shared__ double s_ty[128];               // low word: types, high word: >= 0 for a real atom
  __shared__ double2 s_ixy[64], s_izs[64];   // block I, on its way from memory to the lanes' registers
  __shared__ double s_ity[64];
  __shared__ double s_red[4][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  PAIR_STAMP(0, 0);
  const int item = items[blockIdx.x];
  PAIR_STAMP_WAIT(0, 7, "lgkmcnt(0)");  // kernel arguments and the item are here
  const int I = tile_I(item), J = tile_J(item);
  const bool diag = I == J;
  const bool both = J < nhb;  // heavy x heavy
  // Everything the tile reads from memory is asked for here, before anything is waited for, so the workgroup's start
  // is ONE round trip deep (records by slot: no slot -> atom indirection; a slot of a heavy block is the heavy atom
  // itself, so its self volume comes straight from the tree's row).
  auto out_of_range = [&]() {  // workgroup-uniform range test on the two bounding boxes
    return !diag && box_gap2(pbox, I, J) >= range2;
  };
  // (a large system culls most of its tiles: there the test comes first and a culled tile costs two scalar loads; a
  // small one culls next to none: there the test waits until the tile's loads are on their way)
  if (cull_first && out_of_range()) return;
  // Every slot of the tile is fetched ONCE (the start of a launch is a burst of every workgroup's loads at the same
  // time: it is their volume that the first microseconds wait for): lanes 0..15 of wave w take slots 16w.. of block I,
  // lanes 16..31 those of block J (the upper half of the wave repeats the same addresses), and block I reaches the
  // lanes' registers through LDS.
  const int islot = 64 * I + lane, jslot = 64 * J + lane;
  const int fpart = (lane >> 4) & 1, fidx = 16 * wave + (lane & 15);
  const int fslot = 64 * (fpart ? J : I) + fidx, fh = min(fslot, nh - 1);  // (clamped: the loads are unconditional, the choice comes after)
  const double4 fr = prec[fslot];
  const double fsv = sv_vdw[fh], fiv = inv_vol_h[fh];
  const int a_out = pslot[wave == 0 ? islot : jslot];  // wave 0 adds the sums of block I, wave 1 those of block J: by atom
  const LutBatch lut0 = lut_fetch(lut, lut_entries, 0);
  PAIR_STAMP_WAIT(0, 8, "vmcnt(0)");  // everything has arrived
  const double fs = fslot < nh ? fsv * fiv : 0.0;
  lut_store(s_lut, lut0, lut_entries, 0);
  lut_copy_rest(s_lut, lut, lut_entries);
  PAIR_STAMP_WAIT(0, 9, "vmcnt(0) lgkmcnt(0)");  // the tables are in LDS (this wave's part)
  if (!cull_first && out_of_range()) return;
  PAIR_STAMP_WHERE(0, item);
  if (lane < 32) {
    if (fpart) {
      s_xy[fidx] = s_xy[fidx + 64] = make_double2(fr.x, fr.y);
      s_zs[fidx] = s_zs[fidx + 64] = make_double2(fr.z, fs);
      s_ty[fidx] = s_ty[fidx + 64] = fr.w;
    } else {
      s_ixy[fidx] = make_double2(fr.x, fr.y);
      s_izs[fidx] = make_double2(fr.z, fs);
      s_ity[fidx] = fr.w;
    }
  }
  __syncthreads();
  PAIR_STAMP(0, 1);
  const double2 ixy = s_ixy[lane], izs = s_izs[lane];
  const double ity = s_ity[lane];
  const int nsteps = diag ? 8 : 16;
  const int start = (diag ? 1 : 0) + nsteps * wave;  // cyclic offset of the first j met by lane l
  const bool vi = __double2hiint(ity) >= 0;
  const double xi = ixy.x, yi = ixy.y, zi = izs.x, si = izs.y;
  const int2 mi = make_int2(__double2loint(ity) & 0xffff, __double2loint(ity) >> 16);  // {screened type, screener type}: block I is always a heavy block
  const int base = (lane + start) & 63;
  double sum_i = 0.0, sum_j = 0.0;
  // diagonal tile, cyclic distance 32 (the last step of the last wave): one end only
  if (both)
    born_walk<true>(sum_i, sum_j, s_lut, s_xy + base, s_zs + base, s_ty + base, xi, yi, zi, si, mi.x * ntj, mi.y, nsteps,
                    diag ? 32 - start : -1, vi, lane < 32, ntj, range2);
  else
    born_walk<false>(sum_i, sum_j, s_lut, s_xy + base, s_zs + base, s_ty + base, xi, yi, zi, si, 0, mi.y, nsteps, -1, vi, true, ntj, range2);
  s_red[wave][0][lane] = sum_i;
  s_red[wave][1][(lane + start + nsteps) & 63] = sum_j;  // whose sum the lane holds after the rotations
  __syncthreads();
  PAIR_STAMP(0, 2);
  if (wave < 2) {  // wave 0 adds the sums of block I, wave 1 those of block J
    if (wave == 0 && !both) return;
    const int a = a_out;
    if (a >= 0)
      hbm_add(&born_part[a], quantize((s_red[0][wave][lane] + s_red[1][wave][lane]) + (s_red[2][wave][lane] + s_red[3][wave][lane]), kQBorn, det != 0));
    PAIR_STAMP(0, 3);
  }
}

// ---- Born-radius chain rule, 64x64 tiles in "pair order" with range culling ------------------------------
// Reference loop (ReferenceAGBNPKernels.cpp:555-586) over ordered (i, heavy j != i, d < 2 nm):
//   W_j += brw_i Q,  U_j += bru_i Q,  F_i += D (brw_i + bru_i) s_j Q'/d,  F_j -= same      (D = r_j - r_i)
// Only heavy atoms descreen, so the atoms are walked in pair order (pslot): all heavy atoms first, then all
// hydrogens, each group padded to whole blocks of 64.  That leaves two kinds of tiles and no per-lane type tests:
//   heavy x heavy  symmetric tiles (I <= J), every unordered pair met once, both directions (two look-ups)
//   heavy x H      full tiles, one direction (the heavy atom descreens the hydrogen, one look-up)
//   H x H          nothing to do, never scheduled
// which halves the table look-ups (the LDS pipe is what bounds this kernel).  Machinery as in k_gb_tiles:
// block I in registers, the static record of block J from a doubled LDS copy, the sums of the j atom travel by
// DPP rotation.  A work item whose two bounding boxes are more than the table's 2 nm reach apart exits at once.
struct DbornLane {
  double x, y, z, bw, s;   // the lane's own atom i
  int row, tsr;            // screened type * ntj, screener type
  double fxi, fyi, fzi, wui, fxj, fyj, fzj, wuj;
};

template <bool kBoth>
__device__ __forceinline__ void dborn_walk(DbornLane& L, const double2* __restrict__ s_lut, const double2* __restrict__ jxy,
                                           const double2* __restrict__ jzw, const double2* __restrict__ jsm, int nsteps,
                                           int masked_step, bool vi, bool lower, int ntj, double range2) {
#pragma unroll 4
  for (int k = 0; k < nsteps; k++) {
    const double2 xy = jxy[k], zw = jzw[k], sm = jsm[k];
    const double dx = xy.x - L.x, dy = xy.y - L.y, dz = zw.x - L.z;
    const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
    const int tj = __double2loint(sm.y);  // screened type | screener type << 16
    if (d2 < range2 && vi && __double2hiint(sm.y) >= 0 && (k != masked_step || lower)) {
      const double rinv = rsqrt_pos(d2);
      const double d = d2 * rinv;
      double q2, dq2;  // i descreens j
      spline_value_deriv(s_lut, ((tj & 0xffff) * ntj + L.tsr) * kLutStride, d, q2, dq2);
      L.wui = fma(zw.y, q2, L.wui);
      double t = zw.y * L.s * dq2;
      if (kBoth) {  // j descreens i
        double q1, dq1;
        spline_value_deriv(s_lut, (L.row + (tj >> 16)) * kLutStride, d, q1, dq1);
        L.wuj = fma(L.bw, q1, L.wuj);
        t = fma(L.bw * sm.x, dq1, t);
      }
      t *= rinv;
      L.fxi = fma(dx, t, L.fxi);
      L.fyi = fma(dy, t, L.fyi);
      L.fzi = fma(dz, t, L.fzi);
      L.fxj = fma(-dx, t, L.fxj);
      L.fyj = fma(-dy, t, L.fyj);
      L.fzj = fma(-dz, t, L.fzj);
    }
    L.fxj = rot1(L.fxj);
    L.fyj = rot1(L.fyj);
    L.fzj = rot1(L.fzj);
    if (kBoth) L.wuj = rot1(L.wuj);
  }
}

__global__ __launch_bounds__(256) void k_dborn_tiles(int n, int nhb, int ntj, int lut_entries, const int* __restrict__ items,
                                                    const int* __restrict__ pslot, const double* __restrict__ pbox,
                                                    const double4* __restrict__ prec, const double4* __restrict__ srec,
                                                    const double* __restrict__ ys, const double* __restrict__ sv_vdw,
                                                    const double* __restrict__ inv_vol_h, int nh, const double2* __restrict__ lut,
                                                    double* __restrict__ db_rows, PairArgs P, double* __restrict__ energy_out,
                                                    double* __restrict__ components, int role_bytes) {
  // the first workgroup carries the energy sum (see above)
  extern __shared__ double2 s_lut[];
  if (blockIdx.x == 0) return energy_role(P, 1, energy_out, components, reinterpret_cast<char*>(s_lut));
  if (blockIdx.x == 1) return dealing_role(P, reinterpret_cast<char*>(s_lut), role_bytes);  // second half of the bookkeeping
  // block J twice over (entry m and m + 64 are slot 64 J + m): {x, y}, {z, bw}, {s, types|validity}
  __shared__ double2 s_rec[3][128];
  // one workgroup = one tile; its four waves take a quarter of the cyclic distances each and share the j records
  // and the spline tables
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  PAIR_STAMP(2, 0);
  const int item = items[blockIdx.x - 2];
  const int I = tile_I(item), J = tile_J(item);
  const bool diag = I == J;
  const bool both = J < nhb;  // heavy x heavy
  // Everything the tile reads from memory is asked for here, before anything is waited for (see k_born_tiles): the
  // slot's geometry and types (k_prep), {B, f', brw, q} and the finished Y sum (GB stage), the self volume (tree).
  struct SlotData {
    double4 r, g;
    double y, sv, iv;
  };
  auto fetch = [&](int slot) {  // (unconditional loads, clamped: nothing is waited for in here)
    SlotData d;
    const int h = min(slot, nh - 1);
    d.r = prec[slot];
    d.g = srec[slot];
    d.y = ys[slot];
    d.sv = sv_vdw[h];
    d.iv = inv_vol_h[h];
    return d;
  };
  // {bw, s} of an atom: bw = brw + bru with bru = -(1/4pi) k (q^2 + Y B) f' (ReferenceAGBNPKernels.cpp:534-542),
  // formed here from the finished GB sums instead of a per-atom kernel in between
  auto weights = [&](const SlotData& d, bool slot_is_heavy) {
    const double bru = -(1. / (4. * kPi)) * kDielFactor * (d.g.w * d.g.w + d.y * d.g.x) * d.g.y;
    return make_double2(d.g.z + bru, slot_is_heavy ? d.sv * d.iv : 0.0);  // slot h of a heavy block is heavy atom h
  };
  auto out_of_range = [&]() {  // workgroup-uniform range test on the two bounding boxes
    return !diag && box_gap2(pbox, I, J) >= P.range2;
  };
  if (P.cull_first && out_of_range()) return;  // (see k_born_tiles)
  // every slot of the tile is fetched once, block I reaches the lanes' registers through LDS (see k_born_tiles)
  const int islot = 64 * I + lane, jslot = 64 * J + lane;
  const int fpart = (lane >> 4) & 1, fidx = 16 * wave + (lane & 15);
  const int fslot = 64 * (fpart ? J : I) + fidx;
  const SlotData fd = fetch(fslot);
  const int ai = pslot[islot], aj = pslot[jslot];  // the force rows are by atom
  const LutBatch lut0 = lut_fetch(lut, lut_entries, 0);
  lut_store(s_lut, lut0, lut_entries, 0);
  lut_copy_rest(s_lut, lut, lut_entries);
  if (!P.cull_first && out_of_range()) return;
  PAIR_STAMP_WHERE(2, item);
  double2* const s_irec = s_lut + lut_entries;  // [3][64] block I, behind the tables (the launch sizes the area for both)
  if (lane < 32) {
    const bool vf = __double2hiint(fd.r.w) >= 0;
    const double2 wf = vf ? weights(fd, fslot < nh) : make_double2(0.0, 0.0);
    // .w of the record: low word screened type | screener type << 16 (only read in heavy x heavy tiles); high word >= 0 for a real atom
    const double2 r0 = make_double2(fd.r.x, fd.r.y), r1 = make_double2(fd.r.z, wf.x), r2 = make_double2(wf.y, fd.r.w);
    if (fpart) {
      s_rec[0][fidx] = s_rec[0][fidx + 64] = r0;
      s_rec[1][fidx] = s_rec[1][fidx + 64] = r1;
      s_rec[2][fidx] = s_rec[2][fidx + 64] = r2;
    } else {
      s_irec[fidx] = r0;
      s_irec[64 + fidx] = r1;
      s_irec[128 + fidx] = r2;
    }
  }
  const int nsteps = diag ? 8 : 16;
  const int start = (diag ? 1 : 0) + nsteps * wave;  // cyclic offset of the first j met by lane l
  __syncthreads();
  PAIR_STAMP(2, 1);
  const double2 i0 = s_irec[lane], i1 = s_irec[64 + lane], i2 = s_irec[128 + lane];
  const bool vi = __double2hiint(i2.y) >= 0;
  const int2 mi = make_int2(__double2loint(i2.y) & 0xffff, __double2loint(i2.y) >> 16);  // {screened type, screener type}: block I is always a heavy block
  DbornLane L;
  L.x = i0.x, L.y = i0.y, L.z = i1.x, L.bw = i1.y, L.s = i2.x;
  L.row = mi.x * ntj, L.tsr = mi.y;
  L.fxi = L.fyi = L.fzi = L.wui = L.fxj = L.fyj = L.fzj = L.wuj = 0.0;
  const int base = (lane + start) & 63;
  const double2* __restrict__ jxy = s_rec[0] + base;
  const double2* __restrict__ jzw = s_rec[1] + base;
  const double2* __restrict__ jsm = s_rec[2] + base;
  // diagonal tile, cyclic distance 32 (the last step of the last wave): one end only
  if (both)
    dborn_walk<true>(L, s_lut, jxy, jzw, jsm, nsteps, diag ? 32 - start : -1, vi, lane < 32, ntj, P.range2);
  else
    dborn_walk<false>(L, s_lut, jxy, jzw, jsm, nsteps, -1, vi, true, ntj, P.range2);
  __syncthreads();  // every wave is done with the spline tables: their LDS now carries the sums of the four waves
  PAIR_STAMP(2, 2);
  TileSums& s_sums = *reinterpret_cast<TileSums*>(s_lut);
  {
    const double vi4[4] = {L.fxi, L.fyi, L.fzi, L.wui}, vj4[4] = {L.fxj, L.fyj, L.fzj, L.wuj};
    tile_sums_store(s_sums, wave, lane, (lane + start + nsteps) & 63, vi4, vj4);  // jslot: whose sums the lane holds now
  }
  __syncthreads();
  // thread (wave q, lane l) adds quantity q of slot l of block I and of block J: rows db_fx, db_fy, db_fz by atom,
  // row db_wu by heavy index (= the slot of a heavy block: only heavy atoms collect W+U, and the tree reads it so)
  double* __restrict__ row = db_rows + (size_t)wave * n;
  const bool det = P.det != 0;
  const double qs = wave == 3 ? kQSum : kQGrad;
  if (vi) hbm_add(&row[wave == 3 ? 64 * I + lane : ai], quantize(tile_sums_fold(s_sums, wave, lane), qs, det));
  if (aj >= 0 && (both || wave < 3)) hbm_add(&row[wave == 3 ? 64 * J + lane : aj], quantize(tile_sums_fold(s_sums, 4 + wave, lane), qs, det));
  PAIR_STAMP(2, 3);
}

// ---- energy-only evaluations (agbnp_hip_energy_*, version 1): the close of the evaluation ---------------------------------
// A full evaluation's chain-rule launch carries the energy role and the dealing role, and the pseudo-volume launch's output
// workgroups close the neighbour rows' evaluation (rows_close_evaluation).  An energy-only evaluation launches neither: this
// small launch behind its GB stage does the three, so that the context is left as a full evaluation leaves it.
//   block 0  energy role (energy sum, sticky log, the host's window on it)
//   block 1  dealing role (the next evaluation's packing into work slots), with the chain-rule launch's LDS: the same dealing
//   block 2  rows_close_evaluation (one lane)
__global__ __launch_bounds__(256) void k_energy_roles(PairArgs P, double* __restrict__ energy_out, double* __restrict__ components,
                                                      int role_bytes) {
  extern __shared__ double2 s_dyn[];
  if (blockIdx.x == 0) return energy_role(P, 1, energy_out, components, reinterpret_cast<char*>(s_dyn));
  if (blockIdx.x == 1) return dealing_role(P, reinterpret_cast<char*>(s_dyn), role_bytes);
  if (threadIdx.x == 0 && P.rows_on) rows_close_evaluation(P.nl_flag, P.nl_nitems, P.row_target, P.gb_rows != 0);
}

// ---- launchers -----------------------------------------------------------------------------------------
#define AGBNP_CHECK_LAUNCH()             \
  do {                                   \
    hipError_t e__ = hipGetLastError();  \
    if (e__ != hipSuccess) return e__;   \
  } while (0)

#define AGBNP_MARK(id)                               \
  do {                                               \
    if (tl) {                                        \
      hipError_t m__ = tl->mark(id, st);             \
      if (m__ != hipSuccess) return m__;             \
    }                                                \
  } while (0)

hipError_t launch_masks(const PairArgs& P, hipStream_t st, Timeline* tl) {
  AGBNP_MARK(kKPrep);  // (booked as k_prep: it takes that launch's place in the evaluations that need it)
  const int ref_blocks = (std::max(P.nh, 1) + 255) / 256;
  hipLaunchKernelGGL(k_masks, dim3(ref_blocks + P.nb_tiles), dim3(256), 0, st, P, ref_blocks);
  return hipGetLastError();
}

hipError_t launch_prep(const PairArgs& P, hipStream_t st, Timeline* tl) {
  AGBNP_MARK(kKPrep);
  const int n = std::max(std::max(P.n, P.nslots), (int)kStatEvalWords);
  const int prep_blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_prep, dim3(prep_blocks + P.nb_tiles), dim3(256), 0, st, P, prep_blocks);
  return hipGetLastError();
}

// Grids and LDS of a context's pair-stage and output launches.  Every launcher below and the replica groups' launch sets
// (engine_group.hip, launch_set) take their numbers from here: a group kernel finds a member's role workgroups and mask tiles by the
// workgroup's number inside the grid the member would launch alone (group_args.h), so the two must never be sized apart.
PairLaunchShape pair_launch_shape(const PairArgs& P, int version) {
  PairLaunchShape s{};
  const int born_groups = (P.n + kRowGroup - 1) / kRowGroup, chain_groups = (P.nh + kRowGroup - 1) / kRowGroup;
  auto walk_blocks = [](int lists, int waves, int cap) { return (lists + waves - 1) / waves * ((cap + kRowSlice - 1) / kRowSlice); };
  s.born_walk = walk_blocks(born_groups * kBornParts, kRowWaves, P.nlh_cap);
  // the lists of the later launches are built in the Born launch
  s.born_build = (chain_groups * kChainParts + (P.gb_rows ? born_groups * kGbParts : 0) + kRowWaves - 1) / kRowWaves;
  s.born_mask_from = s.born_walk + s.born_build;
  s.born_blocks = s.born_mask_from + P.nb_tiles;
  s.born_lds = (size_t)2 * P.nti * P.ntj * kRowIntervals * sizeof(double2);
  s.gb_tile_blocks = P.gb_items_count + 1;
  s.gb_row_blocks = 1 + walk_blocks(born_groups * kGbParts, kGbRowWaves, P.nlg_cap);
  s.chain_blocks = 2 + walk_blocks(chain_groups * kChainParts, kRowWaves, P.nla_cap);  // (2: the energy and the dealing workgroup lead the launch)
  s.chain_lds = std::max(s.born_lds, sizeof(TileSums));  // (>= what the two roles borrow)
  s.role_blocks = 3;  // k_energy_roles: the energy role, the dealing role, the close of the rows' evaluation
  // (version 0: the roles' LDS, with room for the packed shapes and as many forest times of up to 6 k subtrees -- or, where that
  // is more, for the rounds rule of the packing: shapes, a round of running sums, the sorted order of ~1.25 items per subtree)
  const int nh1 = std::max(P.nh, 1);
  const int classes_ints = std::min(2 * nh1 + 64, 12288), rounds_ints = std::min(nh1 + P.tree_slots + nh1 + nh1 / 4 + 64, 14000);
  const int role_bytes = version == 1 ? 0 : (int)kRoleScratchBytes + 4 * std::max(classes_ints, rounds_ints);
  const int force_blocks = (P.n + 255) / 256 + (version == 1 ? 0 : 2);
  s.out = {force_blocks, role_bytes, -1};
  s.out_masks = {force_blocks + P.nb_tiles, role_bytes, force_blocks};
  s.out_energy = {2 + P.nb_tiles, role_bytes, 2};
  return s;
}

hipError_t launch_pair_stages(const PairArgs& P, const PairLaunchShape& S, double* energy_out, double* components, hipStream_t st, Timeline* tl) {
  const size_t lds = (size_t)P.lut_entries * sizeof(double2);
  if (lds > 32 * 1024) {  // beyond the default workgroup allowance (k_dborn_tiles adds 22 KB of static tile records and sums)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_born_tiles), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_dborn_tiles), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds + 3 * 64 * sizeof(double2)));
    if (e != hipSuccess) return e;
  }
  if (P.rows_on) {  // row form of the two range-limited stages (and, in fast mode, of the GB stage)
    auto gb = P.fast ? k_gb_tiles<true, false, false> : (P.gb_far ? k_gb_tiles<false, false, true> : k_gb_tiles<false, false, false>);
    const dim3 rows(64 * kRowWaves);
    AGBNP_MARK(kKBornRows);
    if (P.single && P.five)  // (five-launch mode, the single-precision rows of the fast mode: + the conditional mask tiles; host-named set only)
      hipLaunchKernelGGL((k_rows<kBornRows, true, true>), dim3(S.born_blocks), rows, S.born_lds, st, P, (double*)nullptr, (double*)nullptr, S.born_mask_from);
    else if (P.single)
      hipLaunchKernelGGL((k_rows<kBornRows, true>), dim3(S.born_mask_from), rows, S.born_lds, st, P, (double*)nullptr, (double*)nullptr, 0);
    else if (P.five == 2)  // (five-launch mode, device-side parity: + the conditional mask tiles)
      hipLaunchKernelGGL((k_rows<kBornRows, false, true, true>), dim3(S.born_blocks), rows, S.born_lds, st, P, (double*)nullptr, (double*)nullptr, S.born_mask_from);
    else if (P.five)  // (five-launch mode: + the conditional mask tiles)
      hipLaunchKernelGGL((k_rows<kBornRows, false, true>), dim3(S.born_blocks), rows, S.born_lds, st, P, (double*)nullptr, (double*)nullptr, S.born_mask_from);
    else
      hipLaunchKernelGGL(k_rows<kBornRows>, dim3(S.born_mask_from), rows, S.born_lds, st, P, (double*)nullptr, (double*)nullptr, 0);
    AGBNP_CHECK_LAUNCH();
    if (P.gb_rows) {
      AGBNP_MARK(kKGbRows);
      hipLaunchKernelGGL(k_rows<kGbRows>, dim3(S.gb_row_blocks), dim3(64 * kGbRowWaves), sizeof(StripSums), st, P, (double*)nullptr, (double*)nullptr, (int)sizeof(StripSums));
    } else {
      AGBNP_MARK(kKGbTiles);
      hipLaunchKernelGGL(gb, dim3(S.gb_tile_blocks), dim3(256), 0, st, P.n, P.gb_items, (const double4*)P.aposq,
                         (const double*)P.born_part, P.inv_rvdw, P.alpha, P.born, P.born_fp, P.brw, P.e_atom, P.gb_fx, P.egb_part, P);
    }
    AGBNP_CHECK_LAUNCH();
    AGBNP_MARK(kKDbornRows);
    if (P.single)
      hipLaunchKernelGGL((k_rows<kChainRows, true>), dim3(S.chain_blocks), rows, S.chain_lds, st, P, energy_out, components, (int)S.chain_lds);
    else if (P.five == 2)
      hipLaunchKernelGGL((k_rows<kChainRows, false, false, true>), dim3(S.chain_blocks), rows, S.chain_lds, st, P, energy_out, components, (int)S.chain_lds);
    else
      hipLaunchKernelGGL(k_rows<kChainRows>, dim3(S.chain_blocks), rows, S.chain_lds, st, P, energy_out, components, (int)S.chain_lds);
    AGBNP_CHECK_LAUNCH();
    return hipSuccess;
  }
  AGBNP_MARK(kKBornTiles);
  if (P.db_items_count > 0)
    hipLaunchKernelGGL(k_born_tiles, dim3(P.db_items_count), dim3(256), lds, st, P.nh, P.nhb, P.ntj, P.lut_entries, P.db_items, P.pslot,
                       (const double*)P.pbox, (const double4*)P.prec, (const double*)P.sv_vdw, P.inv_vol_h, P.lut, P.born_part, P.range2, P.det, P.cull_first);
  AGBNP_CHECK_LAUNCH();
  AGBNP_MARK(kKGbTiles);
  auto gb = P.fast ? (P.single ? k_gb_tiles<true, true, false> : k_gb_tiles<true, false, false>)
                   : (P.gb_far ? k_gb_tiles<false, false, true> : k_gb_tiles<false, false, false>);
  if (P.five)  // (five-launch mode on the tile kernels: the masks' renewal rides at the tail of this launch)
    gb = P.fast ? (P.single ? k_gb_tiles<true, true, false, true> : k_gb_tiles<true, false, false, true>)
                : (P.gb_far ? k_gb_tiles<false, false, true, true> : k_gb_tiles<false, false, false, true>);
  hipLaunchKernelGGL(gb, dim3(P.gb_items_count + 1 + (P.five ? P.nb_tiles : 0)), dim3(256), 0, st, P.n, P.gb_items, (const double4*)P.aposq,
                     (const double*)P.born_part, P.inv_rvdw, P.alpha, P.born, P.born_fp, P.brw, P.e_atom, P.gb_fx, P.egb_part, P);
  AGBNP_CHECK_LAUNCH();
  AGBNP_MARK(kKDbornTiles);
  // (+ 2: the energy workgroup and the dealing workgroup; with no heavy atom there is no tile but the roles still run)
  const size_t db_lds = std::max(lds + 3 * 64 * sizeof(double2), sizeof(TileSums));  // tables + block I's records; later the sums
  hipLaunchKernelGGL(k_dborn_tiles, dim3(P.db_items_count + 2), dim3(256), db_lds, st, P.n, P.nhb, P.ntj, P.lut_entries, P.db_items, P.pslot,
                     (const double*)P.pbox, (const double4*)P.prec, (const double4*)P.srec, (const double*)P.ys, (const double*)P.sv_vdw,
                     P.inv_vol_h, P.nh, P.lut, P.db_fx, P, energy_out, components, (int)db_lds);
  AGBNP_CHECK_LAUNCH();
  return hipSuccess;
}

// The energy-only evaluation's launches behind the cavity launch (engine_eval.hip, energy_only_fast: five-launch mode with the
// host-named set, Reference semantics, FP64 rows).  Version 1: the Born rows exactly as in a full evaluation (they also build the
// chain-rule lists after a rebuild and carry the masks' renewal tiles), the GB stage's energy-only instantiation, k_energy_roles.
// Version 0: the output launch's two role workgroups and its mask tiles, without force workgroups.
hipError_t launch_energy_only_stages(const PairArgs& P, const PairLaunchShape& S, int version, double* energy_out, double* components,
                                     hipStream_t st, Timeline* tl) {
  if (version != 1) return launch_outputs(P, S.out_energy, version, nullptr, energy_out, components, st, tl);
  if (!P.rows_on || P.gb_rows || P.single || P.fast || P.det || P.five != 1) return hipErrorInvalidValue;  // (the host engine never asks)
  AGBNP_MARK(kKBornRows);
  hipLaunchKernelGGL((k_rows<kBornRows, false, true>), dim3(S.born_blocks), dim3(64 * kRowWaves), S.born_lds, st, P, (double*)nullptr, (double*)nullptr,
                     S.born_mask_from);
  AGBNP_CHECK_LAUNCH();
  AGBNP_MARK(kKGbTiles);
  auto gb = P.gb_far ? k_gb_tiles<false, false, true, false, true> : k_gb_tiles<false, false, false, false, true>;
  hipLaunchKernelGGL(gb, dim3(S.gb_tile_blocks), dim3(256), 0, st, P.n, P.gb_items, (const double4*)P.aposq, (const double*)P.born_part,
                     P.inv_rvdw, P.alpha, P.born, P.born_fp, P.brw, P.e_atom, P.gb_fx, P.egb_part, P);
  AGBNP_CHECK_LAUNCH();
  AGBNP_MARK(kKEnergyRoles);
  hipLaunchKernelGGL(k_energy_roles, dim3(S.role_blocks), dim3(256), S.chain_lds, st, P, energy_out, components, (int)S.chain_lds);
  AGBNP_CHECK_LAUNCH();
  AGBNP_MARK(-1);
  return hipSuccess;
}

hipError_t launch_outputs(const PairArgs& P, const OutputShape& O, int version, double* force_out, double* energy_out, double* components,
                          hipStream_t st, Timeline* tl) {
  AGBNP_MARK(kKOutputs);
  hipLaunchKernelGGL(k_outputs, dim3(O.blocks), dim3(256), O.role_bytes, st, P, version, force_out, energy_out, components, O.role_bytes, O.mask_from);
  AGBNP_CHECK_LAUNCH();
  AGBNP_MARK(-1);
  return hipSuccess;
}

}  // namespace agbnp

#ifdef AGBNP_PAIR_STAMPS
extern "C" void agbnp_debug_pair_log(unsigned long long* out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(agbnp::g_pair_log), sizeof(agbnp::g_pair_log));
}
#endif
