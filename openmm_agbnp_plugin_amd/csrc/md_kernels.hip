// Integrator steps for the device-resident MD drivers of the example scripts (openmm_agbnp_plugin_amd/md.py: DeviceMD and
// ReplicaMD; the py3 counterparts of the reference's example/1dwc_benchmark.py and example/test_agbnp.py).  NOT part of the
// drop-in boundary (include/agbnp_hip.h): in the reference the integrator is OpenMM's.  A step written in torch operations is
// seventeen tiny launches around the six of the AGBNP evaluation (0.163 ms per step of 1dwc against 0.104 for the evaluation
// alone); here it is two: everything in front of the force evaluation, everything behind it -- and between the steps of a run
// both in one.
//
// Every kernel advances R >= 1 replicas of ONE system in one launch; a single trajectory is a group of one.
// State is strided ([R][n][3], [R][blocks], [R]...): replica r's buffers are fixed slices, the arguments travel as one struct by
// value (AgbnpMdGroup).  The grid is R x blocks(n) workgroups of one thread per atom; a workgroup's replica is
// blockIdx.x / blocks (uniform), and a replica's sums are taken inside its own blocks(n) workgroups, so they do not depend on
// R: the tether partials in a fixed order, the kinetic energy per workgroup in a fixed order and across workgroups by an FP64
// atomic in the order of arrival (bit-reproducible for n <= 256, to rounding beyond).
//
//   pre      Langevin (BAOAB, the reference's LangevinIntegrator(300 K, 1/ps, 1 fs), 1dwc_benchmark.py:20):
//              v += dt/2m f;  x += dt/2 v;  v = c1 v + cn xi;  x += dt/2 v,   cn = sqrt((1 - c1^2) kT[r] / m)
//            velocity Verlet (the reference's NVE check, test_agbnp.py:57):   v += dt/2m f;  x += dt v
//            then the tethers, the only force-field term besides AGBNP:  f = -k (x - x0), their energy as per-block partials
//   post     v += dt/2m f (f now holds tethers + AGBNP);  kinetic energy;  potential = tether partials + what the engine added
//            to the replica's energy word;  the replica's last workgroup to arrive writes both into the per-step logs and hands
//            the energy word and the accumulators back as zeros
//   mid      between two force evaluations of a run of steps: post of step n and pre of step n + 1 in ONE launch
//   tethers  the tethers alone (the first force evaluation of a run, and the minimiser's)
//
// The bath temperature is a device word per replica (kT[r], kJ/mol), which an exchange swaps without the host: that is why the
// noise amplitude is formed in the kernel.  Normal deviates: Philox4x32-10 keyed by seeds[r], counter = (atom, step number on
// the device lo, hi, 0|1), Box-Muller in FP64 on 53-bit uniforms: the stream of a run depends on nothing but the seed (graph
// replays included: the step number is read from device memory).  The counter's last word names the stream (kNoiseWord0 ..
// kLambdaWord below, md.py's PHILOX_* words): no two uses share one.
//
// Exchange (temperature replica exchange between neighbouring rungs of the ladder): k_md_exchange_decide, ONE workgroup,
// one thread per pair (k, k + 1), k = a mod 2, a mod 2 + 2, ...: the pairs of an attempt are disjoint, so every thread reads and
// writes its own two replicas' words; it leaves a velocity factor per replica (1 where nothing happened), and
// k_md_exchange_apply, a launch of its own behind it, rescales -- no workgroup of the second launch can see a half-made decision.
//
// Hamiltonian exchange (md.py: HamiltonianReplicaMD): slot k is rung k for the whole run -- its context (the
// parameters may differ from rung to rung), kT[k] and seed stay -- and what moves is the conformation.  The driver has added
// the cross energies to cross[k] = A_k(x of the partner's slot) (agbnp_hip_energy_group); k_md_hamiltonian_decide, again one
// workgroup with one thread per pair, judges
//   Delta = ((P_lo - T_lo) - C_lo) / kT_lo + ((P_hi - T_hi) - C_hi) / kT_hi + (1 / kT_lo - 1 / kT_hi) (T_lo - T_hi)
// (P: last[r][0], T: the slot's tether partials summed in ascending block order, C: cross[r]; a C that is 0.0 or not finite is a
// withheld cross evaluation, and the pair is void), leaves a partner (-1: none) and a velocity factor per slot, and
// k_md_hamiltonian_apply, a launch of its own behind it, exchanges x[lo] and x[hi] bit for bit and the velocities rescaled to
// the bath they arrive in.  f is left alone: the driver evaluates all slots again behind the attempt.
//
// Lambda exchange (md.py: BindingReplicaMD): replica exchange over a ladder of binding Hamiltonians
// E_lambda = E_R + E_L + lambda u.  Replica r is a conformation that keeps its binding, its bath kT[r] and its buffers; what moves
// is lambda[r], a device word that the binding group's combine launch reads (agbnp_hip_binding_execute_group: d_lambdas).  E_lambda
// is linear in lambda, so an exchange of lambda between two replicas needs no cross evaluation: k_md_lambda_exchange, ONE launch
// of one workgroup with one thread per pair of rungs, judges
//   Delta = (lambda_lo - lambda_hi) (u_lo / kT_lo - u_hi / kT_hi)
// from the u words the last evaluation of each replica added to u[r] (u_lo / kT_lo: u[lo] / kT[lo] rounded to a double, then the
// difference, then the product) and accepts iff log(uniform) <= Delta.  A u word that is 0.0 or not finite is a withheld
// evaluation (the engine adds nothing then, and the word is still the zero it was handed back as): the pair is void, recorded with
// accepted = -1, nothing swapped.  All R u words are handed back as zeros, behind a barrier: those of the replicas that sat the
// attempt out too, which the next attempt's evaluation adds to again.  No position, velocity or force moves and no second
// launch follows; the forces and E_lambda of a replica whose lambda changed are stale until the driver's next evaluation.
// A binding whose u is identically zero (version 0 with a ligand without a heavy atom) makes every pair void.
//
// FIRE minimiser (fast inertial relaxation, Bitzek et al., PRL 97, 170201; md.py: _Replicas.minimise): two
// launches per iteration around the driver's evaluation, the grid of the group kernels (R x blocks(n) workgroups, one thread per
// atom), each replica with state and convergence of its own.  An iteration is  back, front, evaluation:  the back half judges the
// evaluation in f and the energy word and leaves the coefficients of a move, the front half makes the move and the tethers, and
// the evaluation adds to f.  The grid-wide dependency between judging and moving is the launch boundary: no workgroup waits for
// another.  The minimiser's velocities are its own scratch w [R][n][3]; g.v, g.step, g.log_pe, g.log_ke, g.last, g.acc and
// g.done are neither read nor written.  Every product below is a double operation in the order written; fma(a, b, c) is a * b + c
// rounded once.
//
//   back     k_md_fire_back (f holds tethers + AGBNP, energy[r] what the engine added, tether_part the front half's partials)
//     per atom i, over d = 0, 1, 2 in turn from zeros:  p = fma(F_d, w_d, p);  q = fma(F_d, F_d, q);  s = fma(w_d, w_d, s)
//     per workgroup: the maximum of q, then block_sum of p, of q and of s (threads beyond n bring zeros); thread 0 stores
//       part[r][b] = {sum p, sum q, sum s, max q} and counts the workgroup in at arrived[r]
//     thread 0 of the replica's last workgroup to arrive, over b = 0 .. blocks - 1 in turn from zeros:
//       P += part[r][b][0];  Q += part[r][b][1];  S += part[r][b][2];  M = max(M, part[r][b][3]);  T += tether_part[r][b]
//     e = energy[r];  energy[r] = 0;  arrived[r] = 0   (in every case)
//     1. e == 0.0, or e or Q not finite:  the evaluation was withheld (the engine adds nothing then) or is not a number, the
//        iteration is void:  voids[r] += 1;  move = 0; nothing else changes -- for a converged replica too
//     2. converged[r] != 0:          move = 0; nothing else changes
//     3. otherwise  E = T + e,  fm = sqrt(M),  it = iterations[r];  if it < capacity: log_e[r][it] = E, log_fmax[r][it] = fm;
//        fmax[r] = fm;  iterations[r] = it + 1;  then
//        a. fm < tolerance:  converged[r] = 1;  move = 0
//        b. P > 0:   npos[r] += 1;  a = 1 - alpha[r];  b = alpha[r] * sqrt(S / Q) (0 where Q is 0);  the move's dt = dt[r];  move = 1;
//                    then, if npos[r] > n_min:  dt[r] = min(dt[r] * f_inc, dt_max);  alpha[r] = alpha[r] * f_alpha
//        c. else:    npos[r] = 0;  dt[r] = dt[r] * f_dec;  alpha[r] = alpha0;  a = b = 0;  the move's dt = the new dt[r];  move = 1
//     coef[r] = {a, b, the move's dt, move (0.0 or 1.0)}; where move = 0 only that word of coef[r] is written
//
//   front    k_md_fire_front
//     where coef[r].move != 0, per atom i with h = dt / mass[i] (dt: the move's), over d:
//       w_d = fma(b, F_d, a * w_d);  w_d = fma(h, F_d, w_d);  d_d = dt * w_d;      l = sqrt(fma(d_2, d_2, fma(d_1, d_1, d_0 * d_0)))
//       if l > max_move:  c = max_move / l;  d_d = d_d * c;  w_d = w_d * c          then  x_d = x_d + d_d;  w and x are stored
//     where it is 0, neither x nor w of the replica is written
//     for every replica, tether() per component on the stored positions as in k_md_group_tethers:  f = -k (x - x0), the
//     partials of the tethers' energy into tether_part
//
// A converged replica stays converged: its x and w are never written again, and the evaluations that follow repeat the one it
// converged on (one of them withheld counts in voids[r] as any other).  A void iteration is repeated at the same positions
// (the engine's contract for a withheld evaluation).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/agbnp_hip.h"

struct AgbnpMdGroup {  // (mirrored field for field by md.py::_GroupArgs)
  int n, replicas;
  double *x, *v, *f;                // [R][n][3]
  const double *x0, *hdt_m, *mass;  // [n][3], [n], [n]: the one system's tether anchors, dt / 2m, m
  const double* kT;                 // [R] bath temperatures in kJ/mol
  const unsigned long long* seeds;  // [R] Philox keys
  double c1, dt, ktether;           // exp(-friction dt), step, tether constant
  double* energy;                   // [R] the words agbnp_hip_execute_group adds the AGBNP energies to
  double* acc;                      // [R][2] kinetic-energy accumulators
  unsigned* done;                   // [R] workgroups of the replica that have arrived
  double *log_pe, *log_ke;          // [R][capacity]
  long long* step;                  // [R]
  long long capacity;
  double* last;                     // [R][2] {potential, kinetic} energy of the last step
};

struct AgbnpMdExchangeRecord {  // (md.py::EXCHANGE_RECORD); 72 bytes, no padding
  long long attempt, step;      // step: steps replica_lo had finished
  int rung, replica_lo, replica_hi, accepted;
  double u_lo, u_hi, kT_lo, kT_hi, u;  // potential energies and bath temperatures (kJ/mol) BEFORE the decision
};

struct AgbnpMdExchange {  // (md.py::_ExchangeArgs)
  int n, replicas;
  double* v;                 // [R][n][3]
  double* kT;                // [R]
  int *rung_of_replica, *replica_at_rung;  // [R] each
  const double* last;        // [R][2]
  const long long* step;     // [R]
  long long* attempts;       // [1]
  double* scale;             // [R] velocity factors of the attempt in flight
  AgbnpMdExchangeRecord* log;
  long long log_capacity;
  unsigned long long seed;
};

struct AgbnpMdHamiltonianRecord {  // (md.py::HAMILTONIAN_RECORD); 104 bytes, no padding
  long long attempt, step;      // step: steps slot lo had finished
  int rung, walker_lo, walker_hi, accepted;  // accepted: 1, 0, or -1 for a void pair (a cross energy is missing)
  double p_lo, p_hi, t_lo, t_hi, c_lo, c_hi, kT_lo, kT_hi, u;  // potential, tether, cross energies and baths (kJ/mol) BEFORE the decision
};

struct AgbnpMdHamiltonian {  // (md.py::_HamiltonianArgs)
  int n, replicas;
  double *x, *v;              // [R][n][3]
  const double* kT;           // [R] slot k's bath: never moves
  int *walker_at_rung, *rung_of_walker;  // [R] each
  double* last;               // [R][2] {potential, kinetic}; the kinetic word follows an accepted conformation
  const double* tether_part;  // [R][agbnp_md_blocks(n)] the tether partials of the evaluation last[r][0] was summed from
  double* cross;              // [R] the words agbnp_hip_energy_group added the cross energies to; handed back as zeros
  const long long* step;      // [R]
  long long* attempts;        // [1]
  int* partner;               // [R] of the attempt in flight: the slot to exchange with, -1: none
  double* scale;              // [R] of the attempt in flight: the factor of the velocities ARRIVING at the slot
  AgbnpMdHamiltonianRecord* log;
  long long log_capacity;
  unsigned long long seed;
};

struct AgbnpMdLambdaRecord {  // (md.py::LAMBDA_RECORD); 88 bytes, no padding
  long long attempt, step;      // step: steps replica_lo had finished
  int rung, replica_lo, replica_hi, accepted;  // accepted: 1, 0, or -1 for a void pair (a u word is missing)
  double u_lo, u_hi, lambda_lo, lambda_hi, kT_lo, kT_hi, uniform;  // binding energies, lambdas and baths (kJ/mol) BEFORE the decision
};

struct AgbnpMdLambda {  // (md.py::_LambdaArgs); 88 bytes: 4 bytes of padding behind replicas
  int replicas;
  double* lambda;            // [R] the words a binding group reads as d_lambdas
  int *rung_of_replica, *replica_at_rung;  // [R] each
  const double* kT;          // [R] replica r's bath: never moves
  double* u;                 // [R] the words the binding group added u to; all R are handed back as zeros
  const long long* step;     // [R]
  long long* attempts;       // [1]
  AgbnpMdLambdaRecord* log;
  long long log_capacity;
  unsigned long long seed;
};

struct AgbnpMdFire {  // (md.py::_FireArgs); 176 bytes: every field at a multiple of 8 in this order, 4 bytes of padding behind n_min (at 152)
  double* w;                 // [R][n][3] the minimiser's velocities (scratch; g.v is not used)
  double *dt, *alpha;        // [R]
  int* npos;                 // [R] consecutive iterations with F.w > 0
  long long* iterations;     // [R] judged (not void) evaluations: the index of the next log slot
  int *converged, *voids;    // [R]
  double* fmax;              // [R] the largest per-atom force norm of the last judged evaluation
  double* coef;              // [R][4] {a, b, dt, move} of the move in flight
  double* part;              // [R][agbnp_md_blocks(n)][4] per-block {sum F.w, sum F.F, sum w.w, max |F_i|^2}
  unsigned* arrived;         // [R] workgroups of the replica that have stored their partials
  double *log_e, *log_fmax;  // [R][capacity], indexed by the iteration word
  long long capacity;
  double dt_max, f_inc, f_dec, alpha0, f_alpha;
  int n_min;
  double tolerance, max_move;  // kJ/mol/nm, nm
};

namespace {

constexpr int kBlock = 256;
constexpr int kMaxReplicas = AGBNP_HIP_MAX_GROUP;
// the last word of a Philox counter names the stream: the two blocks of a step's noise, the three exchanges' deviates
constexpr uint32_t kNoiseWord0 = 0u, kNoiseWord1 = 1u, kExchangeWord = 2u, kHamiltonianWord = 3u, kLambdaWord = 4u;

__host__ __device__ constexpr int blocks_of(int n) { return (n + kBlock - 1) / kBlock; }

// a workgroup's replica r, its thread's atom i (beyond n in the replica's last workgroup) and the offset o of replica r in an
// [R][n][3] array; the grid is R x blocks workgroups
struct Place {
  int r, i;
  size_t o;
};
__device__ __forceinline__ Place place(int blocks, int n) {
  const int r = blockIdx.x / blocks, b = blockIdx.x - r * blocks, i = b * kBlock + threadIdx.x;
  return Place{r, i, (size_t)r * 3 * n};
}

struct Philox {
  uint32_t c[4];
};
__device__ __forceinline__ Philox philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
    k0 += W0, k1 += W1;
  }
  return Philox{{c0, c1, c2, c3}};
}
__device__ __forceinline__ double uniform53(uint32_t a, uint32_t b) {  // (0, 1]
  const uint64_t u = ((uint64_t)a << 21) ^ (uint64_t)(b >> 11);  // 53 bits
  return ((double)(u & ((1ull << 53) - 1ull)) + 1.0) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ void box_muller(double u1, double u2, double& z0, double& z1) {
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2.0 * u2, &s, &c);
  z0 = r * c, z1 = r * s;
}

__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
  for (int w = 0; w < kBlock / 64; w++) r += red[w];  // fixed order
  __syncthreads();
  return r;
}

// one component of an atom's tether, the position word x in a register:  f = -k (x - x0);  returns the atom's energy so far,
// e, with this component's k/2 (x - x0)^2 added in one fma.  Its callers take d = 0, 1, 2 in turn from e = 0
__device__ __forceinline__ double tether(double x, double x0, double k, double& f, double e) {
  const double dd = x - x0;
  f = -k * dd;
  return fma(0.5 * k * dd, dd, e);
}

// thread 0 counts its workgroup in at *counter, a release fence in front of the count; true, for every thread, in the last of
// the `blocks` workgroups to arrive.  What a workgroup publishes in front of the call is its caller's, and so is the acquire
// fence in front of what the last one reads
__device__ __forceinline__ bool last_to_arrive(unsigned* counter, int blocks, bool& s_last) {
  if (threadIdx.x == 0) {
    __threadfence();
    s_last = atomicAdd(counter, 1u) == (unsigned)blocks - 1u;
  }
  __syncthreads();
  return s_last;
}

// the front half of a step for atom i of one replica, velocity pv already kicked: drift (+ OU for Langevin at the replica's bath
// temperature), tethers; returns the atom's tether energy.  kind 0: Langevin (BAOAB), 1: velocity Verlet
__device__ __forceinline__ double front_half(int i, int kind, double (&px)[3], double (&pv)[3], double* __restrict__ x, double* __restrict__ v,
                                             double* __restrict__ f, const double* __restrict__ x0, double kT, double mass, double c1,
                                             double dt, double ktether, unsigned long long seed, unsigned long long s) {
  if (kind == 0) {
    const Philox a = philox4x32((uint32_t)i, (uint32_t)s, (uint32_t)(s >> 32), kNoiseWord0, (uint32_t)seed, (uint32_t)(seed >> 32));
    const Philox b = philox4x32((uint32_t)i, (uint32_t)s, (uint32_t)(s >> 32), kNoiseWord1, (uint32_t)seed, (uint32_t)(seed >> 32));
    double z[4];
    box_muller(uniform53(a.c[0], a.c[1]), uniform53(a.c[2], a.c[3]), z[0], z[1]);
    box_muller(uniform53(b.c[0], b.c[1]), uniform53(b.c[2], b.c[3]), z[2], z[3]);
    const double cn = sqrt((1.0 - c1 * c1) * kT / mass);
    for (int d = 0; d < 3; d++) {
      px[d] = fma(0.5 * dt, pv[d], px[d]);
      pv[d] = fma(c1, pv[d], cn * z[d]);
      px[d] = fma(0.5 * dt, pv[d], px[d]);
    }
  } else {
    for (int d = 0; d < 3; d++) px[d] = fma(dt, pv[d], px[d]);
  }
  double e = 0.0;
  for (int d = 0; d < 3; d++) {
    x[3 * i + d] = px[d];
    v[3 * i + d] = pv[d];
    e = tether(px[d], x0[3 * i + d], ktether, f[3 * i + d], e);
  }
  return e;
}

// the tail of the back half per replica: the replica's last workgroup to arrive sums step s's energies into the logs and hands
// the energy word and the accumulators back as zeros.  acc[2 r]: the kinetic-energy sum, done[r]: workgroups that have added theirs
__device__ __forceinline__ void group_log_step(const AgbnpMdGroup& g, int r, int blocks, const double* __restrict__ part, long long s, double ke,
                                               double* red, bool& s_last) {
  if (threadIdx.x == 0) __hip_atomic_fetch_add(&g.acc[2 * r], ke, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!last_to_arrive(&g.done[r], blocks, s_last)) return;
  double et = 0.0;
  for (int b = threadIdx.x; b < blocks; b += kBlock) et += part[b];
  et = block_sum(et, red);
  if (threadIdx.x == 0) {
    __threadfence();
    const double kin = __hip_atomic_load(&g.acc[2 * r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double pot = et + g.energy[r];
    if (s < g.capacity) g.log_pe[r * g.capacity + s] = pot, g.log_ke[r * g.capacity + s] = kin;
    g.last[2 * r] = pot, g.last[2 * r + 1] = kin;
    g.step[r] = s + 1;
    g.energy[r] = 0.0;
    g.acc[2 * r] = 0.0;
    g.done[r] = 0u;
  }
}

// one thread per atom: everything in front of the force evaluation of a step
__global__ __launch_bounds__(kBlock) void k_md_group_pre(AgbnpMdGroup g, int blocks, int kind, double* __restrict__ tether_part) {
  __shared__ double red[kBlock / 64];
  const auto [r, i, o] = place(blocks, g.n);
  double e = 0.0;
  if (i < g.n) {
    const double h = g.hdt_m[i];
    double px[3], pv[3];
    for (int d = 0; d < 3; d++) px[d] = g.x[o + 3 * i + d], pv[d] = fma(h, g.f[o + 3 * i + d], g.v[o + 3 * i + d]);
    e = front_half(i, kind, px, pv, g.x + o, g.v + o, g.f + o, g.x0, g.kT[r], g.mass[i], g.c1, g.dt, g.ktether, g.seeds[r],
                   (unsigned long long)g.step[r]);
  }
  e = block_sum(e, red);
  if (threadIdx.x == 0) tether_part[blockIdx.x] = e;
}

// everything behind it; the tether partials are the front half's (its grid is this kernel's)
__global__ __launch_bounds__(kBlock) void k_md_group_post(AgbnpMdGroup g, int blocks, const double* __restrict__ tether_part) {
  __shared__ double red[kBlock / 64];
  __shared__ bool s_last;
  const auto [r, i, o] = place(blocks, g.n);
  const long long s = g.step[r];  // (read before this workgroup counts itself in: only the last to arrive writes it)
  double ke = 0.0;
  if (i < g.n) {
    const double h = g.hdt_m[i], m = g.mass[i];
    for (int d = 0; d < 3; d++) {
      const double pv = fma(h, g.f[o + 3 * i + d], g.v[o + 3 * i + d]);
      g.v[o + 3 * i + d] = pv;
      ke = fma(0.5 * m * pv, pv, ke);
    }
  }
  ke = block_sum(ke, red);
  group_log_step(g, r, blocks, tether_part + (size_t)r * blocks, s, ke, red, s_last);
}

// Between two force evaluations of a run of steps: the back half of step n (second kick, energies logged) and the front
// half of step n + 1 in ONE launch.  The tether partials are double-buffered (the workgroup that arrives last sums step n's
// while the others already write step n + 1's): part_old is read, part_new written.
__global__ __launch_bounds__(kBlock) void k_md_group_mid(AgbnpMdGroup g, int blocks, int kind, const double* __restrict__ part_old,
                                                        double* __restrict__ part_new) {
  __shared__ double red[kBlock / 64];
  __shared__ bool s_last;
  const auto [r, i, o] = place(blocks, g.n);
  const long long s = g.step[r];
  double ke = 0.0, e = 0.0;
  if (i < g.n) {
    const double h = g.hdt_m[i], m = g.mass[i];
    double px[3], pv[3];
    for (int d = 0; d < 3; d++) {
      const double fd = g.f[o + 3 * i + d];
      const double v1 = fma(h, fd, g.v[o + 3 * i + d]);  // end of step n
      ke = fma(0.5 * m * v1, v1, ke);
      pv[d] = fma(h, fd, v1);                             // first kick of step n + 1: the same force
      px[d] = g.x[o + 3 * i + d];
    }
    e = front_half(i, kind, px, pv, g.x + o, g.v + o, g.f + o, g.x0, g.kT[r], m, g.c1, g.dt, g.ktether, g.seeds[r],
                   (unsigned long long)s + 1ull);
  }
  ke = block_sum(ke, red);
  e = block_sum(e, red);
  if (threadIdx.x == 0) part_new[blockIdx.x] = e;
  group_log_step(g, r, blocks, part_old + (size_t)r * blocks, s, ke, red, s_last);
}

// tethers alone (the first force evaluation of a run, and the minimiser's): f = -k (x - x0), partials of their energy
__global__ __launch_bounds__(kBlock) void k_md_group_tethers(AgbnpMdGroup g, int blocks, double* __restrict__ tether_part) {
  __shared__ double red[kBlock / 64];
  const auto [r, i, o] = place(blocks, g.n);
  double e = 0.0;
  if (i < g.n)
    for (int d = 0; d < 3; d++) e = tether(g.x[o + 3 * i + d], g.x0[3 * i + d], g.ktether, g.f[o + 3 * i + d], e);
  e = block_sum(e, red);
  if (threadIdx.x == 0) tether_part[blockIdx.x] = e;
}

// ---- FIRE minimiser (the header comment states the order of every operation) ----

__device__ __forceinline__ double block_max(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < kBlock / 64; w++) r = fmax(r, red[w]);
  __syncthreads();
  return r;
}

// what thread 0 of the replica's last workgroup to arrive does with the sums P = F.w, Q = F.F, S = w.w, M = max |F_i|^2, T = tethers
__device__ __forceinline__ void fire_judge(const AgbnpMdGroup& g, const AgbnpMdFire& q, int r, double P, double Q, double S, double M, double T) {
  const double e = g.energy[r];
  g.energy[r] = 0.0;
  q.arrived[r] = 0u;
  double* coef = q.coef + 4 * r;
  // the engine adds nothing for a withheld evaluation; a force that is not a number never reaches M (fmax drops it) but does reach Q
  if (e == 0.0 || !isfinite(e) || !isfinite(Q)) {
    q.voids[r] += 1;
    coef[3] = 0.0;
    return;
  }
  if (q.converged[r] != 0) {
    coef[3] = 0.0;
    return;
  }
  const double E = T + e, fm = sqrt(M);
  const long long it = q.iterations[r];
  if (it < q.capacity) q.log_e[r * q.capacity + it] = E, q.log_fmax[r * q.capacity + it] = fm;
  q.fmax[r] = fm;
  q.iterations[r] = it + 1;
  if (fm < q.tolerance) {
    q.converged[r] = 1;
    coef[3] = 0.0;
    return;
  }
  const double dt = q.dt[r], alpha = q.alpha[r];
  if (P > 0.0) {
    const int np = q.npos[r] + 1;
    q.npos[r] = np;
    coef[0] = 1.0 - alpha, coef[1] = Q > 0.0 ? alpha * sqrt(S / Q) : 0.0, coef[2] = dt, coef[3] = 1.0;
    if (np > q.n_min) q.dt[r] = fmin(dt * q.f_inc, q.dt_max), q.alpha[r] = alpha * q.f_alpha;
  } else {
    const double cut = dt * q.f_dec;
    q.npos[r] = 0, q.dt[r] = cut, q.alpha[r] = q.alpha0;
    coef[0] = 0.0, coef[1] = 0.0, coef[2] = cut, coef[3] = 1.0;
  }
}

// behind an evaluation: the four reductions per workgroup as partials; the replica's last workgroup to arrive judges.  The
// partials cross workgroups inside the launch: agent-scope stores, a release in front of the count, an acquire behind it
__global__ __launch_bounds__(kBlock) void k_md_fire_back(AgbnpMdGroup g, int blocks, AgbnpMdFire q, const double* __restrict__ tether_part) {
  __shared__ double red[kBlock / 64];
  __shared__ bool s_last;
  const auto [r, i, o] = place(blocks, g.n);
  double p = 0.0, ff = 0.0, s = 0.0;
  if (i < g.n)
    for (int d = 0; d < 3; d++) {
      const double fd = g.f[o + 3 * i + d], wd = q.w[o + 3 * i + d];
      p = fma(fd, wd, p), ff = fma(fd, fd, ff), s = fma(wd, wd, s);
    }
  const double m = block_max(ff, red);
  p = block_sum(p, red), ff = block_sum(ff, red), s = block_sum(s, red);
  if (threadIdx.x == 0) {
    double* mine = q.part + 4 * (size_t)blockIdx.x;
    __hip_atomic_store(mine + 0, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 1, ff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 2, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + 3, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!last_to_arrive(&q.arrived[r], blocks, s_last) || threadIdx.x != 0) return;
  __threadfence();
  double P = 0.0, Q = 0.0, S = 0.0, M = 0.0, T = 0.0;
  const double* all = q.part + 4 * (size_t)r * blocks;
  for (int k = 0; k < blocks; k++) {  // ascending block order
    P += __hip_atomic_load(all + 4 * k + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    Q += __hip_atomic_load(all + 4 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S += __hip_atomic_load(all + 4 * k + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    M = fmax(M, __hip_atomic_load(all + 4 * k + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    T += tether_part[(size_t)r * blocks + k];
  }
  fire_judge(g, q, r, P, Q, S, M, T);
}

// in front of the next evaluation: the move the back half decided, then tether() as in k_md_group_tethers
__global__ __launch_bounds__(kBlock) void k_md_fire_front(AgbnpMdGroup g, int blocks, AgbnpMdFire q, double* __restrict__ tether_part) {
  __shared__ double red[kBlock / 64];
  const auto [r, i, o] = place(blocks, g.n);
  const double ca = q.coef[4 * r], cb = q.coef[4 * r + 1], dt = q.coef[4 * r + 2];
  const bool move = q.coef[4 * r + 3] != 0.0;
  double e = 0.0;
  if (i < g.n) {
    double px[3];
    for (int d = 0; d < 3; d++) px[d] = g.x[o + 3 * i + d];
    if (move) {
      const double h = dt / g.mass[i];
      double w[3], dd[3];
      for (int d = 0; d < 3; d++) {
        const double fd = g.f[o + 3 * i + d];
        w[d] = fma(cb, fd, ca * q.w[o + 3 * i + d]);
        w[d] = fma(h, fd, w[d]);
        dd[d] = dt * w[d];
      }
      const double len = sqrt(fma(dd[2], dd[2], fma(dd[1], dd[1], dd[0] * dd[0])));
      if (len > q.max_move) {
        const double c = q.max_move / len;
        for (int d = 0; d < 3; d++) dd[d] *= c, w[d] *= c;
      }
      for (int d = 0; d < 3; d++) {
        px[d] += dd[d];
        q.w[o + 3 * i + d] = w[d];
        g.x[o + 3 * i + d] = px[d];
      }
    }
    for (int d = 0; d < 3; d++) e = tether(px[d], g.x0[3 * i + d], g.ktether, g.f[o + 3 * i + d], e);
  }
  e = block_sum(e, red);
  if (threadIdx.x == 0) tether_part[blockIdx.x] = e;
}

// The schedule of exchange attempt a, shared by both decide kernels (one workgroup, thread t): thread t has the pair of rungs
// (k, k + 1), k = pair_of(a, t) = a mod 2 + 2 t, where k + 1 < R; the pair's record has a fixed place in the log -- attempts
// 0 .. a - 1 left (a + 1) / 2 even ones with R / 2 pairs each and a / 2 odd ones with (R - 1) / 2 --; its deviate is uniform53
// of Philox(counter (k, a lo, a hi, word), key seed), `word` keeping the two exchanges' streams apart
__device__ __forceinline__ int pair_of(long long a, int t) { return 2 * t + (int)(a & 1); }
__device__ __forceinline__ long long record_place(long long a, int R, int t) { return ((a + 1) / 2) * (R / 2) + (a / 2) * ((R - 1) / 2) + t; }
__device__ __forceinline__ double attempt_uniform(int k, long long a, uint32_t word, unsigned long long seed) {
  const Philox p = philox4x32((uint32_t)k, (uint32_t)a, (uint32_t)((unsigned long long)a >> 32), word, (uint32_t)seed, (uint32_t)(seed >> 32));
  return uniform53(p.c[0], p.c[1]);
}

// attempt a = attempts[0]: pairs of rungs (k, k + 1), k = a mod 2, a mod 2 + 2, ...; accept iff log(u) <= Delta,
// Delta = (1 / kT_lo - 1 / kT_hi) (U_lo - U_hi), u = attempt_uniform with counter word kExchangeWord (2).  An accepted
// pair swaps temperatures and rungs; conformations stay.  The records of an attempt have fixed places in the log.
__global__ __launch_bounds__(64) void k_md_exchange_decide(AgbnpMdExchange e) {
  const int t = threadIdx.x, R = e.replicas;
  const long long a = e.attempts[0];
  if (t < R) e.scale[t] = 1.0;
  __syncthreads();
  const int k = pair_of(a, t);
  if (k + 1 < R) {
    const int lo = e.replica_at_rung[k], hi = e.replica_at_rung[k + 1];
    const double kT_lo = e.kT[lo], kT_hi = e.kT[hi], u_lo = e.last[2 * lo], u_hi = e.last[2 * hi];
    const double delta = (1.0 / kT_lo - 1.0 / kT_hi) * (u_lo - u_hi);
    const double u = attempt_uniform(k, a, kExchangeWord, e.seed);
    const bool accepted = log(u) <= delta;
    if (accepted) {
      e.kT[lo] = kT_hi, e.kT[hi] = kT_lo;
      e.rung_of_replica[lo] = k + 1, e.rung_of_replica[hi] = k;
      e.replica_at_rung[k] = hi, e.replica_at_rung[k + 1] = lo;
      e.scale[lo] = sqrt(kT_hi / kT_lo), e.scale[hi] = sqrt(kT_lo / kT_hi);
    }
    const long long at = record_place(a, R, t);
    if (at < e.log_capacity) e.log[at] = AgbnpMdExchangeRecord{a, e.step[lo], k, lo, hi, accepted ? 1 : 0, u_lo, u_hi, kT_lo, kT_hi, u};
  }
  __syncthreads();  // (every thread has read `a`)
  if (t == 0) e.attempts[0] = a + 1;
}

__global__ __launch_bounds__(kBlock) void k_md_exchange_apply(AgbnpMdExchange e, int blocks) {
  const auto [r, i, o] = place(blocks, e.n);
  const double s = e.scale[r];
  if (s == 1.0 || i >= e.n) return;
  double* v = e.v + o + 3 * i;
  for (int d = 0; d < 3; d++) v[d] *= s;
}

// attempt a = attempts[0] of a Hamiltonian exchange: pairs of slots (k, k + 1), k = a mod 2, a mod 2 + 2, ...; accept iff
// log(u) <= Delta (the header comment), u = attempt_uniform with counter word kHamiltonianWord (3): it keeps the stream
// apart from the temperature exchange's.  The records of an attempt have the fixed places k_md_exchange_decide uses.
__global__ __launch_bounds__(64) void k_md_hamiltonian_decide(AgbnpMdHamiltonian h) {
  const int t = threadIdx.x, R = h.replicas;
  const long long a = h.attempts[0];
  if (t < R) h.partner[t] = -1, h.scale[t] = 1.0;
  __syncthreads();
  const int lo = pair_of(a, t), hi = lo + 1;
  if (hi < R) {
    const int blocks = blocks_of(h.n);
    const double kT_lo = h.kT[lo], kT_hi = h.kT[hi], p_lo = h.last[2 * lo], p_hi = h.last[2 * hi];
    const double k_lo = h.last[2 * lo + 1], k_hi = h.last[2 * hi + 1], c_lo = h.cross[lo], c_hi = h.cross[hi];
    double t_lo = 0.0, t_hi = 0.0;
    for (int b = 0; b < blocks; b++) t_lo += h.tether_part[(size_t)lo * blocks + b], t_hi += h.tether_part[(size_t)hi * blocks + b];
    h.cross[lo] = 0.0, h.cross[hi] = 0.0;
    const int w_lo = h.walker_at_rung[lo], w_hi = h.walker_at_rung[hi];
    const double delta = ((p_lo - t_lo) - c_lo) / kT_lo + ((p_hi - t_hi) - c_hi) / kT_hi + (1.0 / kT_lo - 1.0 / kT_hi) * (t_lo - t_hi);
    const double u = attempt_uniform(lo, a, kHamiltonianWord, h.seed);
    // the engine adds nothing for a withheld evaluation: a cross word that is still zero is a missing cross energy
    const bool is_void = c_lo == 0.0 || c_hi == 0.0 || !isfinite(c_lo) || !isfinite(c_hi);
    const bool accepted = !is_void && log(u) <= delta;
    if (accepted) {
      h.partner[lo] = hi, h.partner[hi] = lo;
      h.scale[lo] = sqrt(kT_lo / kT_hi), h.scale[hi] = sqrt(kT_hi / kT_lo);
      h.walker_at_rung[lo] = w_hi, h.walker_at_rung[hi] = w_lo;
      if (w_lo >= 0 && w_lo < R) h.rung_of_walker[w_lo] = hi;  // (a walker is a slot number: no word outside the map is written)
      if (w_hi >= 0 && w_hi < R) h.rung_of_walker[w_hi] = lo;
      h.last[2 * lo + 1] = k_hi * kT_lo / kT_hi, h.last[2 * hi + 1] = k_lo * kT_hi / kT_lo;
    }
    const long long at = record_place(a, R, t);
    if (at < h.log_capacity)
      h.log[at] = AgbnpMdHamiltonianRecord{a, h.step[lo], lo, w_lo, w_hi, is_void ? -1 : (accepted ? 1 : 0), p_lo, p_hi, t_lo, t_hi, c_lo, c_hi,
                                           kT_lo, kT_hi, u};
  }
  __syncthreads();  // (every thread has read `a`)
  if (t == 0) h.attempts[0] = a + 1;
}

// only the workgroups of a slot whose partner is a HIGHER slot work: thread i exchanges atom i of the two conformations
__global__ __launch_bounds__(kBlock) void k_md_hamiltonian_apply(AgbnpMdHamiltonian h, int blocks) {
  const auto [r, i, o] = place(blocks, h.n);
  const int q = h.partner[r];
  if (q <= r || q >= h.replicas || i >= h.n) return;
  const double sr = h.scale[r], sq = h.scale[q];
  const size_t o_r = o + 3 * i, o_q = (size_t)q * 3 * h.n + 3 * i;
  for (int d = 0; d < 3; d++) {
    const double xr = h.x[o_r + d], xq = h.x[o_q + d], vr = h.v[o_r + d], vq = h.v[o_q + d];
    h.x[o_r + d] = xq, h.x[o_q + d] = xr;
    h.v[o_r + d] = vq * sr, h.v[o_q + d] = vr * sq;
  }
}

// attempt a = attempts[0] of a lambda exchange (the header comment): pairs of rungs (k, k + 1), k = a mod 2, a mod 2 + 2, ...,
// lo / hi the replicas on them; accept iff log(uniform) <= Delta, uniform = attempt_uniform with counter word kLambdaWord (4).
// An accepted pair swaps the two replicas' lambda words and rungs; nothing else moves.  The pairs of an attempt are disjoint, so
// every u word has at most one reader; behind a barrier all R are handed back as zeros.  The records have the fixed places k_md_exchange_decide uses.
__global__ __launch_bounds__(64) void k_md_lambda_exchange(AgbnpMdLambda e) {
  const int t = threadIdx.x, R = e.replicas;
  const long long a = e.attempts[0];
  const int k = pair_of(a, t);
  if (k + 1 < R) {
    const int lo = e.replica_at_rung[k], hi = e.replica_at_rung[k + 1];
    const double l_lo = e.lambda[lo], l_hi = e.lambda[hi], kT_lo = e.kT[lo], kT_hi = e.kT[hi], u_lo = e.u[lo], u_hi = e.u[hi];
    const double delta = (l_lo - l_hi) * (u_lo / kT_lo - u_hi / kT_hi);
    const double uniform = attempt_uniform(k, a, kLambdaWord, e.seed);
    // the engine adds nothing for a withheld evaluation: a u word that is still zero is a missing binding energy
    const bool is_void = u_lo == 0.0 || u_hi == 0.0 || !isfinite(u_lo) || !isfinite(u_hi);
    const bool accepted = !is_void && log(uniform) <= delta;
    if (accepted) {
      e.lambda[lo] = l_hi, e.lambda[hi] = l_lo;
      e.rung_of_replica[lo] = k + 1, e.rung_of_replica[hi] = k;
      e.replica_at_rung[k] = hi, e.replica_at_rung[k + 1] = lo;
    }
    const long long at = record_place(a, R, t);
    if (at < e.log_capacity)
      e.log[at] = AgbnpMdLambdaRecord{a, e.step[lo], k, lo, hi, is_void ? -1 : (accepted ? 1 : 0), u_lo, u_hi, l_lo, l_hi, kT_lo, kT_hi, uniform};
  }
  __syncthreads();  // (every thread has read `a` and its pair's u words)
  if (t < R) e.u[t] = 0.0;  // all R words, those of the replicas that sat the attempt out too: the next attempt's evaluation ADDS
  if (t == 0) e.attempts[0] = a + 1;
}

// the entry points' two bodies.  A struct of any of the three kinds is judged by its first two words
template <typename S>
bool shape_ok(const S* s) { return s && s->n > 0 && s->replicas >= 1 && s->replicas <= kMaxReplicas; }

// one launch of a per-atom kernel (AgbnpMdGroup, blocks, args...) for all the replicas of *g
template <typename K, typename... A>
int launch_group(K kernel, const AgbnpMdGroup* g, void* stream, A... args) {
  if (!shape_ok(g)) return (int)hipErrorInvalidValue;
  const int blocks = blocks_of(g->n);
  hipLaunchKernelGGL(kernel, dim3(g->replicas * blocks), dim3(kBlock), 0, (hipStream_t)stream, *g, blocks, args...);
  return (int)hipGetLastError();
}

// the two launches of an exchange attempt: decide (one workgroup of 64), then apply per atom
template <typename E, typename D, typename P>
int launch_exchange(D decide, P apply, const E* e, void* stream) {
  if (!shape_ok(e)) return (int)hipErrorInvalidValue;
  const int blocks = blocks_of(e->n);
  hipLaunchKernelGGL(decide, dim3(1), dim3(64), 0, (hipStream_t)stream, *e);
  hipLaunchKernelGGL(apply, dim3(e->replicas * blocks), dim3(kBlock), 0, (hipStream_t)stream, *e, blocks);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int agbnp_md_blocks(int n) { return blocks_of(n); }

// One launch each for all the replicas of *g (a host struct, read during the call).  tether_part / part_old / part_new:
// [R][agbnp_md_blocks(n)].  kind 0: Langevin, 1: velocity Verlet.  Return: hipError_t of the launch, 1 for a bad *g.
int agbnp_md_group_pre(const AgbnpMdGroup* g, int kind, double* tether_part, void* stream) {
  return launch_group(k_md_group_pre, g, stream, kind, tether_part);
}
int agbnp_md_group_mid(const AgbnpMdGroup* g, int kind, const double* part_old, double* part_new, void* stream) {
  return launch_group(k_md_group_mid, g, stream, kind, part_old, part_new);
}
int agbnp_md_group_post(const AgbnpMdGroup* g, const double* tether_part, void* stream) {
  return launch_group(k_md_group_post, g, stream, tether_part);
}
int agbnp_md_group_tethers(const AgbnpMdGroup* g, double* tether_part, void* stream) {
  return launch_group(k_md_group_tethers, g, stream, tether_part);
}

// The two launches of a FIRE iteration (the header comment), one each for all the replicas of *g; *q is a host struct as *g is.
// tether_part: [R][agbnp_md_blocks(n)], read by the back half, written by the front half.  Return: as the group entry points,
// a null *q included.
int agbnp_md_fire_back(const AgbnpMdGroup* g, const AgbnpMdFire* q, const double* tether_part, void* stream) {
  return q ? launch_group(k_md_fire_back, g, stream, *q, tether_part) : (int)hipErrorInvalidValue;
}
int agbnp_md_fire_front(const AgbnpMdGroup* g, const AgbnpMdFire* q, double* tether_part, void* stream) {
  return q ? launch_group(k_md_fire_front, g, stream, *q, tether_part) : (int)hipErrorInvalidValue;
}

// One exchange attempt between neighbouring rungs: two launches (decide, rescale), no synchronisation, nothing read back.
int agbnp_md_exchange(const AgbnpMdExchange* e, void* stream) {
  return launch_exchange(k_md_exchange_decide, k_md_exchange_apply, e, stream);
}

// One Hamiltonian exchange attempt between neighbouring slots: two launches (decide, exchange the conformations), no
// synchronisation, nothing read back.  The cross energies of the attempt's pairs are in h->cross when the first one runs.
int agbnp_md_hamiltonian_exchange(const AgbnpMdHamiltonian* h, void* stream) {
  return launch_exchange(k_md_hamiltonian_decide, k_md_hamiltonian_apply, h, stream);
}

// One lambda exchange attempt between neighbouring rungs: ONE launch of one 64-thread workgroup, no synchronisation, nothing read
// back.  The u words of the attempt's pairs are in e->u when it runs.  Return: hipError_t of the launch, 1 for a null *e, replicas
// outside 1 .. 16 or a null array (the log's may be null where log_capacity is 0).
int agbnp_md_lambda_exchange(const AgbnpMdLambda* e, void* stream) {
  if (!e || e->replicas < 1 || e->replicas > kMaxReplicas) return (int)hipErrorInvalidValue;
  if (!e->lambda || !e->rung_of_replica || !e->replica_at_rung || !e->kT || !e->u || !e->step || !e->attempts) return (int)hipErrorInvalidValue;
  if (!e->log && e->log_capacity > 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_md_lambda_exchange, dim3(1), dim3(64), 0, (hipStream_t)stream, *e);
  return (int)hipGetLastError();
}

}  // extern "C"
