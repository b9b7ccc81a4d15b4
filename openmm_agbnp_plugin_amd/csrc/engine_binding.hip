// Binding-energy evaluations (agbnp_hip_binding_*, include/agbnp_hip.h): one object that owns the contexts of a complex, its
// receptor and its ligand, and one call per evaluation of
//   u = E_RL(x) - E_R(x_R) - E_L(x_L),   E_lambda = E_R + E_L + lambda u,   F_lambda = lambda F^RL + (1 - lambda) F^{R|L}.
// An evaluation is one gather launch (binding_kernels.hip: both sub-systems' positions out of the caller's array -- also where
// the ligand is one contiguous range: one launch, one rule), ONE agbnp_hip_execute_group / agbnp_hip_energy_group over the three
// members through the public entry points, so the members share launch sets exactly as any group's do, and one combine launch that
// reads all three verdicts on the device and adds to the caller's buffers all or nothing.  The k-th binding evaluation since the
// last agbnp_hip_binding_finish() is the k-th evaluation of every member: the binding's log is the union of the members'.
// Binding groups (agbnp_hip_binding_execute_group and its kin) evaluate up to 16 bindings on one gather launch, one to three
// group calls and one combine launch, each binding's lambda read from device memory.
// Single and group calls are ONE host path: binding_enqueue takes `count` bindings and makes, for a single call (count == 1, a
// host lambda), the single-binding launches and otherwise the group launches, as group_enqueue makes a member's own launches
// for a launch set of one; the host entry points of both stage and deliver through binding_stage and binding_deliver.  What
// the single and the group entry points keep of their own is their argument checks.  The binding analyses -- the per-atom
// decomposition (Analysis::planes) and the set-pair matrix (Analysis::matrix) -- are ONE second, single enqueue
// (binding_analysis_enqueue) that starts as the first does (binding_enter) and ONE host form (binding_analysis_host); what a kind
// needs of either is said once (analysis_shape).  All single host forms repeat a withheld evaluation in one loop (binding_retry).
// Messages of failed binding calls are the calling thread's agbnp_hip_last_error(NULL).
#include "binding_kernels.h"
#include "engine_context.h"

struct agbnp_hip_binding {
  agbnp_hip_context* m[kBindingMembers] = {nullptr, nullptr, nullptr};  // complex, receptor, ligand
  int n = 0, nr = 0, nl = 0, device = 0;
  std::vector<int> sub2complex;  // [n] the receptor's atoms in ascending complex order, then the ligand's
  std::vector<int> complex2sub;  // [n] the inverse
  DevBuf<int> d_maps;            // [2n] both, in that order
  // [3n] the members' own positions (receptor, ligand) | [3n] the complex's forces | [3n] the receptor's and the ligand's | [3]
  // the three energies: what the members read and ADD to, cleared by every combine launch
  DevBuf<double> d_work;
  // the host entry points' staging: [3n] positions | [3n] F_lambda | E_lambda, u
  DevBuf<double> d_host;
  std::vector<double> h_host;    // [3n + 2] the outputs, read back
  int enqueued = 0;              // binding evaluations of the device entry points since the last finish
  std::vector<void*> streams;    // caller streams they went to
  std::vector<int> withheld;     // what the last finish found
  int withheld_count = 0;
  std::vector<int> carried;      // withheld device evaluations that a host entry point in between had to harvest
  int carried_count = 0, carried_seq = 0;
  // binding groups: the event that joins streams where a group call with a NULL stream runs on several, and the device words
  // the host forms stage their lambdas in (both made on first use, by the call's first binding)
  hipEvent_t group_event = nullptr;
  DevBuf<double> d_group_lambdas;
  // The binding analyses (agbnp_hip_binding_decompose_*: Analysis::planes, the result D [4][n]; agbnp_hip_binding_pair_matrix_*:
  // Analysis::matrix, D [S][S]), one buffer set per kind (of()), each buffer made at the first call that needs it.  members: the
  // complex's target | the receptor's | the ligand's | [3] the three energies -- [4n] | [4 nr] | [4 nl] planes, or [3][S][S]
  // matrices; what the members of the analysis group ADD to, cleared by every combine launch; the matrix kind's is released when S
  // changes.  host: the host form's staging, [3n] positions | D | u, remade when D's size changes (the matrix kind's S)
  struct AnalysisBuffers {
    DevBuf<double> members, host;
    std::vector<double> back;  // D and u, read back
  } analysis[2];
  AnalysisBuffers& of(Analysis kind) { return analysis[kind == Analysis::matrix]; }
  // set-pair matrices: set_of_atom the partition over the complex's atoms, [n], num_sets sets (0: none set); every member holds
  // its restriction, same numbering, same S
  std::vector<int> set_of_atom;
  int num_sets = 0;

  double* sub_pos() const { return d_work.p; }
  double* f_complex() const { return d_work.p + 3 * (size_t)n; }
  double* f_sub() const { return d_work.p + 6 * (size_t)n; }
  double* energies() const { return d_work.p + 9 * (size_t)n; }
  // the complex atom that member k's atom t is (k = 0: itself): restricts any per-atom array of the complex to a member
  int member_atom(int k, int t) const { return k == 0 ? t : sub2complex[(k == 2 ? nr : 0) + t]; }
  int member_size(int k) const { return k == 0 ? n : k == 1 ? nr : nl; }
};

namespace {
int binding_fail(int code, const std::string& msg) {
  g_create_error = msg;
  return code;
}

// a member's call failed: its message becomes the binding's
int member_fail(const agbnp_hip_binding* b, int code, const char* who) {
  for (const agbnp_hip_context* c : b->m)
    if (c && !c->err.empty()) return binding_fail(code, std::string(who) + ": " + c->err);
  return binding_fail(code, std::string(who) + ": a member's call failed");
}

void clear_member_errors(agbnp_hip_binding* b) {
  for (agbnp_hip_context* c : b->m) c->err.clear();
}

#define BINDING_TRY(who, call)                                                                                       \
  do {                                                                                                               \
    hipError_t e__ = (call);                                                                                         \
    if (e__ != hipSuccess) return binding_fail(AGBNP_HIP_ERR_DEVICE, std::string(who) + ": " #call ": " + hipGetErrorString(e__)); \
  } while (0)

// Where a call's lambdas are: ONE host value -- a single call: count == 1, the single-binding kernels, lambda by value in
// their short argument lists -- or (device non-null) a device array of `count` words, which the group kernels read when the
// combine launch runs.
struct Lambdas {
  double host;
  const double* device;
};

// where the combine launch finds the three members' verdicts on the evaluation that has just been enqueued (the members' blocks
// name this evaluation's words until their next evaluation)
BindingVerdicts binding_verdicts(const agbnp_hip_binding* b) {
  BindingVerdicts v;
  for (int m = 0; m < kBindingMembers; m++) {
    const PairArgs& P = b->m[m]->P;
    v.estatus[m] = P.estatus;
    v.epoch[m] = P.epoch;
    v.five[m] = P.five;
  }
  return v;
}

// what every enqueue starts with: the members' messages cleared, the first complex's device and the call's stream, no stream capture
int binding_enter(agbnp_hip_binding* const* bs, int count, void* stream, hipStream_t* st, const char* who) {
  for (int k = 0; k < count; k++) clear_member_errors(bs[k]);
  if (enter(bs[0]->m[0], stream, st) != AGBNP_HIP_OK) return member_fail(bs[0], AGBNP_HIP_ERR_DEVICE, who);
  if (!is_capturing(*st)) return AGBNP_HIP_OK;
  return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT,
                      std::string(who) + ": the stream is being captured; binding evaluations use group calls, which are not captured into graphs");
}

// One evaluation of every binding on `stream` (NULL: the first complex's own); the arguments have been checked.  d_forces null:
// the energy-only form; d_energies / d_bindings null: every entry null.  One gather launch, the members' evaluations through
// the public group entry points -- one call over all 3 count members where they fit a group, else one call per kind
// (complexes, receptors, ligands: same-kind members of one system share a launch set) -- and one combine launch.
// A single call (count == 1): the loops over k = 1 .. are empty and the one group call's stream is `st` itself, so no event is
// made or recorded.
int binding_enqueue(agbnp_hip_binding* const* bs, int count, const double* const* d_pos, const Lambdas& lam, double* const* d_forces,
                    double* const* d_energies, double* const* d_bindings, void* stream, const char* who) {
  agbnp_hip_binding* const b0 = bs[0];
  hipStream_t st;
  const int entered = binding_enter(bs, count, stream, &st, who);
  if (entered != AGBNP_HIP_OK) return entered;
  BindingGroupArgs G;
  std::memset(&G, 0, sizeof(G));
  G.count = count;
  G.lambdas = lam.device;
  agbnp_hip_context* ctxs[kBindingMembers * kMaxBindingGroup];
  const double* pos[kBindingMembers * kMaxBindingGroup];
  double *frc[kBindingMembers * kMaxBindingGroup], *ene[kBindingMembers * kMaxBindingGroup];
  // members in one call: binding by binding; in one call per kind: kind by kind
  const bool one_call = kBindingMembers * count <= kMaxGroup;
  for (int k = 0; k < count; k++) {
    agbnp_hip_binding* const b = bs[k];
    BindingGroupMember& B = G.m[k];
    B.maps = b->d_maps.p;
    B.work = b->d_work.p;
    B.pos = d_pos[k];
    B.forces = d_forces ? d_forces[k] : nullptr;
    B.energy = d_energies ? d_energies[k] : nullptr;
    B.binding = d_bindings ? d_bindings[k] : nullptr;
    B.n = b->n;
    G.first[k + 1] = G.first[k] + (b->n + 255) / 256;
    const double* const p[kBindingMembers] = {d_pos[k], b->sub_pos(), b->sub_pos() + 3 * (size_t)b->nr};
    double* const f[kBindingMembers] = {b->f_complex(), b->f_sub(), b->f_sub() + 3 * (size_t)b->nr};
    for (int m = 0; m < kBindingMembers; m++) {
      const int at = one_call ? kBindingMembers * k + m : count * m + k;
      ctxs[at] = b->m[m];
      pos[at] = p[m];
      frc[at] = f[m];
      ene[at] = b->energies() + m;
    }
  }
  const BindingGroupMember& B0 = G.m[0];  // (a single call's launches take their few words from here)
  // (a NULL stream: a single call on another binding runs on THAT binding's complex's stream, and the gather writes every
  // binding's own buffers -- the group's stream waits for what those streams hold, as group_device joins its members')
  for (int k = 1; k < count && !stream; k++) BINDING_TRY(who, join_streams(b0->group_event, bs[k]->m[0]->stream, st));
  if (lam.device)
    BINDING_TRY(who, launch_binding_gather_group(G, st));
  else
    BINDING_TRY(who, launch_binding_gather(B0.n, B0.pos, B0.maps, b0->sub_pos(), st));
  const int calls = one_call ? 1 : kBindingMembers, per_call = one_call ? kBindingMembers * count : count;
  for (int c = 0; c < calls; c++) {
    const int at = c * per_call;
    // (a NULL stream is the call's first member's own: the first call's is the first complex's, `st`; the receptors' and the
    // ligands' calls run on other streams than the gather and the combine, and are joined to `st` on both sides)
    const hipStream_t own = stream ? st : ctxs[at]->stream;
    BINDING_TRY(who, join_streams(b0->group_event, st, own));
    const int rc = d_forces ? agbnp_hip_execute_group(ctxs + at, per_call, pos + at, frc + at, ene + at, stream)
                            : agbnp_hip_energy_group(ctxs + at, per_call, pos + at, ene + at, stream);
    if (rc != AGBNP_HIP_OK) {
      // No combine launch will read what the failed call, and the calls before it, added to the bindings' buffers: they are
      // cleared here, as well as the device still allows, so that nothing stale is added to by a later evaluation.  After a
      // failure behind the first call the members that ran have logged an evaluation the binding has not: the message says so.
      (void)join_streams(b0->group_event, own, st);
      for (int k = 0; k < count; k++)
        (void)hipMemsetAsync(bs[k]->f_complex(), 0, sizeof(double) * (6 * (size_t)bs[k]->n + kBindingMembers), st);
      const char* note = c > 0 ? " (members of an earlier call of this group have evaluated: finish the bindings and discard that log)" : "";
      for (int k = 0; k < count; k++)
        for (const agbnp_hip_context* m : bs[k]->m)
          if (!m->err.empty()) return binding_fail(rc, std::string(who) + ": " + m->err + note);
      return binding_fail(rc, std::string(who) + ": a member's call failed" + note);
    }
    BINDING_TRY(who, join_streams(b0->group_event, own, st));
  }
  for (int k = 0; k < count; k++) G.m[k].v = binding_verdicts(bs[k]);
  if (lam.device && d_forces)
    BINDING_TRY(who, launch_binding_combine_group(G, st));
  else if (lam.device)
    BINDING_TRY(who, launch_binding_combine_energy_group(G, st));
  else if (d_forces)
    BINDING_TRY(who, launch_binding_combine(B0.n, B0.v, lam.host, B0.maps + B0.n, b0->f_complex(), b0->f_sub(), b0->energies(), B0.forces,
                                            B0.energy, B0.binding, st));
  else
    BINDING_TRY(who, launch_binding_combine_energy(B0.v, lam.host, b0->energies(), B0.energy, B0.binding, st));
  // (a NULL stream: every other binding's agbnp_hip_binding_finish(NULL) drains its own complex's stream, which waits for the combine)
  for (int k = 1; k < count && !stream; k++) BINDING_TRY(who, join_streams(b0->group_event, st, bs[k]->m[0]->stream));
  return AGBNP_HIP_OK;
}

// the matrix calls need a partition (agbnp_hip_binding_set_atom_sets)
int binding_need_sets(const agbnp_hip_binding* b, const char* who) {
  if (b->num_sets > 0) return AGBNP_HIP_OK;
  return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": no partition has been set (agbnp_hip_binding_set_atom_sets)");
}

// what the four analysis entry points check, in this order (a null binding: the code alone)
int binding_analysis_check(const agbnp_hip_binding* b, Analysis kind, const double* pos, const double* out, const char* who) {
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!pos || !out) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  return kind == Analysis::matrix ? binding_need_sets(b, who) : AGBNP_HIP_OK;
}

// What a binding analysis of a kind needs: the words of each member's target and of the result D.  (Which public group call
// runs the members and which combine launch follows are the two places binding_analysis_enqueue asks for the kind.)
struct AnalysisShape {
  size_t member[kBindingMembers];  // planes: 4n | 4nr | 4nl; matrix: S S each
  size_t out;                      // D: 4n | S S
  size_t words() const { return member[0] + member[1] + member[2] + kBindingMembers; }  // ... and the three energies
};
AnalysisShape analysis_shape(const agbnp_hip_binding* b, Analysis kind) {
  const size_t cells = (size_t)b->num_sets * (size_t)b->num_sets;
  if (kind == Analysis::matrix) return {{cells, cells, cells}, cells};
  return {{4 * (size_t)b->n, 4 * (size_t)b->nr, 4 * (size_t)b->nl}, 4 * (size_t)b->n};
}

// One analysis of b on `stream` (NULL: the complex's own); the arguments have been checked and, for a matrix, a partition is set.
// The gather launch, ONE agbnp_hip_decompose_group / agbnp_hip_pair_matrix_group over the three members through the public entry
// point -- their targets and energies into the kind's members' buffer -- and the combine launch, which reads the three verdicts
// and adds D and u all or nothing.
int binding_analysis_enqueue(agbnp_hip_binding* b, Analysis kind, const double* d_pos, double* d_out, double* d_binding, void* stream,
                             const char* who) {
  hipStream_t st;
  const int entered = binding_enter(&b, 1, stream, &st, who);
  if (entered != AGBNP_HIP_OK) return entered;
  const AnalysisShape shape = analysis_shape(b, kind);
  const size_t words = shape.words();
  DevBuf<double>& members = b->of(kind).members;
  if (members.p == nullptr) {  // (the first call of the kind, or the first matrix since S changed: agbnp_hip_binding_set_atom_sets)
    BINDING_TRY(who, members.alloc(words));
    BINDING_TRY(who, hipMemsetAsync(members.p, 0, sizeof(double) * words, st));
  }
  double* const t = members.p;
  double* const target[kBindingMembers] = {t, t + shape.member[0], t + shape.member[0] + shape.member[1]};
  double* const e = t + words - kBindingMembers;
  double* const ene[kBindingMembers] = {e, e + 1, e + 2};
  BINDING_TRY(who, launch_binding_gather(b->n, d_pos, b->d_maps.p, b->sub_pos(), st));
  const double* const pos[kBindingMembers] = {d_pos, b->sub_pos(), b->sub_pos() + 3 * (size_t)b->nr};
  // (a NULL stream is the group's first member's own: the complex's, `st`)
  const int rc = kind == Analysis::matrix ? agbnp_hip_pair_matrix_group(b->m, kBindingMembers, pos, target, ene, stream)
                                          : agbnp_hip_decompose_group(b->m, kBindingMembers, pos, target, ene, stream);
  if (rc != AGBNP_HIP_OK) {
    // no combine launch will read and clear what the members that got as far as their launches added: cleared here, as the
    // force path does
    (void)hipMemsetAsync(t, 0, sizeof(double) * words, st);
    return member_fail(b, rc, who);
  }
  if (kind == Analysis::matrix)
    BINDING_TRY(who, launch_binding_matrix_combine(b->num_sets, binding_verdicts(b), t, e, d_out, d_binding, st));
  else
    BINDING_TRY(who, launch_binding_decompose_combine(b->n, b->nr, binding_verdicts(b), b->d_maps.p + b->n, t, target[1], e, d_out,
                                                      d_binding, st));
  return AGBNP_HIP_OK;
}

// a device entry point has enqueued an evaluation of b on `stream`
void binding_note(agbnp_hip_binding* b, void* stream) {
  b->enqueued++;
  if (stream && std::find(b->streams.begin(), b->streams.end(), stream) == b->streams.end()) b->streams.push_back(stream);
}

// agbnp_hip_binding_decompose_device / agbnp_hip_binding_pair_matrix_device
int binding_analysis_device(agbnp_hip_binding* b, Analysis kind, const double* d_pos, double* d_out, double* d_binding, void* stream,
                            const char* who) {
  int rc = binding_analysis_check(b, kind, d_pos, d_out, who);
  if (rc == AGBNP_HIP_OK) rc = binding_analysis_enqueue(b, kind, d_pos, d_out, d_binding, stream, who);
  if (rc != AGBNP_HIP_OK) return rc;
  binding_note(b, stream);
  return AGBNP_HIP_OK;
}

// drains `stream`, finishes the three members and forms the union of their logs: `out` the indices (ascending), *count their
// number (a member that only counted evaluations beyond its log's bitmap raises it)
int binding_harvest(agbnp_hip_binding* b, void* stream, std::vector<int>& out, int* count, const char* who) {
  clear_member_errors(b);
  hipStream_t st;
  if (enter(b->m[0], stream, &st) != AGBNP_HIP_OK) return member_fail(b, AGBNP_HIP_ERR_DEVICE, who);
  BINDING_TRY(who, hipStreamSynchronize(st));
  out.clear();
  int most = 0, first_rc = AGBNP_HIP_OK;
  for (agbnp_hip_context* c : b->m) {
    int rep = 0;
    const int rc = agbnp_hip_finish(c, stream, &rep);
    if (rc != AGBNP_HIP_OK && first_rc == AGBNP_HIP_OK) first_rc = rc;
    most = std::max(most, rep);
    out.insert(out.end(), c->withheld.begin(), c->withheld.end());
  }
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  *count = std::max(most, (int)out.size());
  if (first_rc != AGBNP_HIP_OK) return member_fail(b, first_rc, who);  // (AGBNP_HIP_ERR_CAPACITY passes through)
  return AGBNP_HIP_OK;
}

// device evaluations that are still unfinished when a host entry point needs the log: harvested now, handed to the next finish
int binding_carry(agbnp_hip_binding* b, const char* who) {
  if (b->enqueued == 0) return AGBNP_HIP_OK;
  BINDING_TRY(who, hipSetDevice(b->device));
  for (void* s : b->streams) BINDING_TRY(who, hipStreamSynchronize((hipStream_t)s));
  std::vector<int> bad;
  int count = 0;
  const int rc = binding_harvest(b, nullptr, bad, &count, who);
  if (rc != AGBNP_HIP_OK) return rc;
  for (int k : bad) b->carried.push_back(k + b->carried_seq);
  b->carried_count += count;
  b->carried_seq += b->enqueued;
  b->enqueued = 0;
  return AGBNP_HIP_OK;
}

// The single host entry points: device evaluations still in flight are carried, then `stage` -- the device path on the binding's
// staging buffers and the complex's own stream, the outputs on their way back -- is repeated until the harvest finds the evaluation
// complete, and `deliver` hands out what came back
template <class Stage, class Deliver>
int binding_retry(agbnp_hip_binding* b, const char* who, Stage stage, Deliver deliver) {
  int rc = binding_carry(b, who);
  if (rc != AGBNP_HIP_OK) return rc;
  BINDING_TRY(who, hipSetDevice(b->device));
  for (int attempt = 0; attempt < 10; attempt++) {
    rc = stage();
    if (rc != AGBNP_HIP_OK) return rc;
    std::vector<int> bad;
    int count = 0;
    rc = binding_harvest(b, nullptr, bad, &count, who);  // (waits for the stream)
    if (rc != AGBNP_HIP_OK) return rc;
    if (count) continue;
    deliver();
    return AGBNP_HIP_OK;
  }
  return binding_fail(AGBNP_HIP_ERR_CAPACITY, std::string(who) + ": capacity negotiation did not converge");
}

// agbnp_hip_binding_decompose_host / agbnp_hip_binding_pair_matrix_host: staged in the kind's host buffer, [3n] positions | D | u
// (made on first use, and remade when D's size -- the matrix kind's S -- changes: the complex's stream is idle between host
// calls), the outputs cleared first
int binding_analysis_host(agbnp_hip_binding* b, Analysis kind, const double* pos, double* out, double* binding_energy, const char* who) {
  const int checked = binding_analysis_check(b, kind, pos, out, who);
  if (checked != AGBNP_HIP_OK) return checked;
  const size_t n3 = 3 * (size_t)b->n, cells = analysis_shape(b, kind).out;
  agbnp_hip_binding::AnalysisBuffers& buf = b->of(kind);
  auto stage = [&]() -> int {
    const hipStream_t st = b->m[0]->stream;
    if (buf.host.p == nullptr || buf.host.count != n3 + cells + 1) BINDING_TRY(who, buf.host.alloc(n3 + cells + 1));
    buf.back.resize(cells + 1);
    double* const d_out = buf.host.p + n3;
    BINDING_TRY(who, hipMemcpyAsync(buf.host.p, pos, sizeof(double) * n3, hipMemcpyHostToDevice, st));
    BINDING_TRY(who, hipMemsetAsync(d_out, 0, sizeof(double) * (cells + 1), st));
    const int rc = binding_analysis_enqueue(b, kind, buf.host.p, d_out, d_out + cells, nullptr, who);
    if (rc != AGBNP_HIP_OK) return rc;
    BINDING_TRY(who, hipMemcpyAsync(buf.back.data(), d_out, sizeof(double) * (cells + 1), hipMemcpyDeviceToHost, st));
    return AGBNP_HIP_OK;
  };
  return binding_retry(b, who, stage, [&] {
    std::memcpy(out, buf.back.data(), sizeof(double) * cells);
    if (binding_energy) *binding_energy = buf.back[cells];
  });
}

// The host entry points' evaluation, on the first complex's own stream: every binding's staging buffers made on first use, its
// positions up, its output words zeroed (the device path ADDS), the device path, the outputs on their way back to h_host.
int binding_stage(agbnp_hip_binding* const* bs, int count, const double* const* positions, const Lambdas& lam, bool energy_only,
                  const char* who) {
  const hipStream_t st = bs[0]->m[0]->stream;
  const double* d_pos[kMaxBindingGroup];
  double *d_frc[kMaxBindingGroup], *d_ene[kMaxBindingGroup], *d_u[kMaxBindingGroup];
  for (int i = 0; i < count; i++) {
    agbnp_hip_binding* const b = bs[i];
    const size_t n3 = 3 * (size_t)b->n;
    if (b->d_host.p == nullptr) BINDING_TRY(who, b->d_host.alloc(2 * n3 + 2));
    b->h_host.resize(n3 + 2);
    d_pos[i] = b->d_host.p;
    d_frc[i] = b->d_host.p + n3;
    d_ene[i] = d_frc[i] + n3;
    d_u[i] = d_ene[i] + 1;
    BINDING_TRY(who, hipMemcpyAsync(b->d_host.p, positions[i], sizeof(double) * n3, hipMemcpyHostToDevice, st));
    BINDING_TRY(who, hipMemsetAsync(d_frc[i], 0, sizeof(double) * (n3 + 2), st));
  }
  const int rc = binding_enqueue(bs, count, d_pos, lam, energy_only ? nullptr : d_frc, d_ene, d_u, nullptr, who);
  if (rc != AGBNP_HIP_OK) return rc;
  for (int i = 0; i < count; i++)
    BINDING_TRY(who, hipMemcpyAsync(bs[i]->h_host.data(), d_frc[i], sizeof(double) * bs[i]->h_host.size(), hipMemcpyDeviceToHost, st));
  return AGBNP_HIP_OK;
}

// ... and, once the stream is drained and the evaluation found complete, what came back: F_lambda ADDED to the caller's forces
// (null: the energy-only form), the two scalars stored
void binding_deliver(const agbnp_hip_binding* b, double* forces, double* energy, double* binding_energy) {
  const size_t n3 = 3 * (size_t)b->n;
  for (size_t k = 0; k < n3 && forces; k++) forces[k] += b->h_host[k];
  if (energy) *energy = b->h_host[n3];
  if (binding_energy) *binding_energy = b->h_host[n3 + 1];
}

// agbnp_hip_binding_execute_host and (forces null) agbnp_hip_binding_energy_host
int binding_host(agbnp_hip_binding* b, const double* pos, double lambda, double* forces, double* energy, double* binding_energy,
                 const char* who) {
  return binding_retry(b, who, [&] { return binding_stage(&b, 1, &pos, Lambdas{lambda, nullptr}, forces == nullptr, who); },
                       [&] { binding_deliver(b, forces, energy, binding_energy); });
}

// agbnp_hip_binding_execute_device and (energy_only, d_forces null) agbnp_hip_binding_energy_device: the single entry points'
// own short checks, then a group of one with a host lambda
int binding_device(agbnp_hip_binding* b, const double* d_pos, double lambda, double* d_forces, bool energy_only, double* d_energy,
                   double* d_binding, void* stream, const char* who) {
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!d_pos || (!energy_only && !d_forces) || (energy_only && !d_energy && !d_binding))
    return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  if (!std::isfinite(lambda)) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": lambda must be finite");
  const int rc = binding_enqueue(&b, 1, &d_pos, Lambdas{lambda, nullptr}, energy_only ? nullptr : &d_forces, &d_energy, &d_binding, stream, who);
  if (rc != AGBNP_HIP_OK) return rc;
  binding_note(b, stream);
  return AGBNP_HIP_OK;
}

// what every group form checks of its bindings, before anything is launched or changed
int check_bindings(agbnp_hip_binding* const* bs, int count, const char* who) {
  if (!bs || count < 1 || count > kMaxBindingGroup)
    return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": a binding group has 1 to 16 bindings, not " + std::to_string(count));
  for (int i = 0; i < count; i++) {
    if (!bs[i]) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null binding");
    if (bs[i]->device != bs[0]->device) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": bindings on different devices");
    for (int j = 0; j < i; j++)
      if (bs[j] == bs[i]) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": the same binding twice");
  }
  return AGBNP_HIP_OK;
}

// agbnp_hip_binding_execute_group and (energy_only, d_forces null) agbnp_hip_binding_energy_group
int binding_group_device(agbnp_hip_binding* const* bs, int count, const double* const* d_pos, const double* d_lambdas,
                         double* const* d_forces, bool energy_only, double* const* d_energies, double* const* d_bindings, void* stream,
                         const char* who) {
  int rc = check_bindings(bs, count, who);
  if (rc != AGBNP_HIP_OK) return rc;
  if (!d_pos || !d_lambdas || (!energy_only && !d_forces)) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  for (int i = 0; i < count; i++) {
    double* const ei = d_energies ? d_energies[i] : nullptr;
    double* const ui = d_bindings ? d_bindings[i] : nullptr;
    if (!d_pos[i] || (!energy_only && !d_forces[i])) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    if (energy_only && !ei && !ui)
      return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": a binding's energy and binding-energy pointers are both null");
    if (energy_only && ei == ui)
      return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": a binding's energy and binding-energy words are the same");
    const size_t ni = energy_only ? 0 : 3 * (size_t)bs[i]->n;
    double* const fi = energy_only ? nullptr : d_forces[i];
    for (int j = 0; j < i; j++) {
      double* const ej = d_energies ? d_energies[j] : nullptr;
      double* const uj = d_bindings ? d_bindings[j] : nullptr;
      const size_t nj = energy_only ? 0 : 3 * (size_t)bs[j]->n;
      double* const fj = energy_only ? nullptr : d_forces[j];
      const double* const a[3] = {fi, ei, ui};
      const double* const b[3] = {fj, ej, uj};
      const size_t na[3] = {ni, 1, 1}, nb[3] = {nj, 1, 1};
      for (int x = 0; x < 3; x++)
        for (int y = 0; y < 3; y++)
          if (spans_overlap(a[x], na[x], b[y], nb[y]))
            return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": output buffers of two bindings overlap");
    }
  }
  rc = binding_enqueue(bs, count, d_pos, Lambdas{0.0, d_lambdas}, energy_only ? nullptr : d_forces, d_energies, d_bindings, stream, who);
  if (rc != AGBNP_HIP_OK) return rc;
  for (int i = 0; i < count; i++) binding_note(bs[i], stream);
  return AGBNP_HIP_OK;
}

// agbnp_hip_binding_execute_group_host and (forces null) agbnp_hip_binding_energy_group_host: the device path on every binding's
// staging buffers and the first complex's own stream; a binding whose evaluation was withheld is repeated alone (binding_host)
int binding_group_host(agbnp_hip_binding* const* bs, int count, const double* const* positions, const double* lambdas,
                       double* const* forces, bool energy_only, double* energies, double* binding_energies, const char* who) {
  int rc = check_bindings(bs, count, who);
  if (rc != AGBNP_HIP_OK) return rc;
  if (!positions || !lambdas || (!energy_only && !forces) || (energy_only && !energies && !binding_energies))
    return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  for (int i = 0; i < count; i++) {
    if (!positions[i] || (!energy_only && !forces[i])) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    if (!std::isfinite(lambdas[i])) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": lambda must be finite");
    for (int j = 0; j < i && !energy_only; j++)
      if (spans_overlap(forces[i], 3 * (size_t)bs[i]->n, forces[j], 3 * (size_t)bs[j]->n))
        return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": output buffers of two bindings overlap");
  }
  agbnp_hip_binding* const b0 = bs[0];
  BINDING_TRY(who, hipSetDevice(b0->device));
  const hipStream_t st = b0->m[0]->stream;
  for (int i = 0; i < count; i++) {
    rc = binding_carry(bs[i], who);  // (every binding's streams are idle from here on)
    if (rc != AGBNP_HIP_OK) return rc;
  }
  if (b0->d_group_lambdas.p == nullptr) BINDING_TRY(who, b0->d_group_lambdas.alloc(kMaxBindingGroup));
  BINDING_TRY(who, hipMemcpyAsync(b0->d_group_lambdas.p, lambdas, sizeof(double) * count, hipMemcpyHostToDevice, st));
  rc = binding_stage(bs, count, positions, Lambdas{0.0, b0->d_group_lambdas.p}, energy_only, who);
  if (rc != AGBNP_HIP_OK) return rc;
  BINDING_TRY(who, hipStreamSynchronize(st));
  for (int i = 0; i < count; i++) {
    agbnp_hip_binding* const b = bs[i];
    double* const fi = energy_only ? nullptr : forces[i];
    double *const ei = energies ? &energies[i] : nullptr, *const ui = binding_energies ? &binding_energies[i] : nullptr;
    std::vector<int> bad;
    int withheld = 0;
    rc = binding_harvest(b, nullptr, bad, &withheld, who);
    // (withheld: repeated alone, as agbnp_hip_binding_execute_host / _energy_host repeats)
    if (rc == AGBNP_HIP_OK && withheld) rc = binding_host(b, positions[i], lambdas[i], fi, ei, ui, who);
    if (rc != AGBNP_HIP_OK) return rc;
    if (!withheld) binding_deliver(b, fi, ei, ui);
  }
  return AGBNP_HIP_OK;
}

// member k's subset of the complex's five parameter arrays (k = 0: all of them), in the member's own atom order
struct MemberParams {
  std::vector<double> r, g, a, q;
  std::vector<int> h;
};
MemberParams member_params(const agbnp_hip_binding* b, int k, const double* radius, const double* gamma, const double* vdw_alpha,
                           const double* charge, const int* ishydrogen) {
  MemberParams p;
  for (int t = 0; t < b->member_size(k); t++) {
    const int i = b->member_atom(k, t);
    p.r.push_back(radius[i]), p.g.push_back(gamma[i]), p.a.push_back(vdw_alpha[i]), p.q.push_back(charge[i]), p.h.push_back(ishydrogen[i]);
  }
  return p;
}
}  // namespace

extern "C" {

int agbnp_hip_binding_create(agbnp_hip_binding** out, int n, const double* radius, const double* gamma, const double* vdw_alpha,
                             const double* charge, const int* ishydrogen, const int* ligand_atoms, int num_ligand_atoms, int version,
                             int nonbonded_method, double cutoff, int device) {
  const char* who = "agbnp_hip_binding_create";
  if (out) *out = nullptr;
  // every argument is checked here, on the host, before any device call
  if (!out || n <= 0 || !radius || !gamma || !vdw_alpha || !charge || !ishydrogen || !ligand_atoms)
    return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer or non-positive particle count");
  if (num_ligand_atoms < 1 || num_ligand_atoms >= n)
    return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": the ligand has 1 to N - 1 atoms, not " + std::to_string(num_ligand_atoms));
  if (version != 0 && version != 1)
    return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": illegal version number (versions 0 and 1 only)");
  if (nonbonded_method < 0 || nonbonded_method > 2) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": illegal nonbonded method");
  if (device < 0) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative device index");
  std::vector<char> is_ligand(n, 0);
  for (int k = 0; k < num_ligand_atoms; k++) {
    const int a = ligand_atoms[k];
    if (a < 0 || a >= n) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": ligand atom index out of range: " + std::to_string(a));
    if (is_ligand[a]) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": ligand atom index given twice: " + std::to_string(a));
    is_ligand[a] = 1;
  }
  for (int i = 0; i < n; i++)
    if (!(radius[i] > 0.0)) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": particle radius must be positive");

  agbnp_hip_binding* b = new agbnp_hip_binding();
  b->n = n;
  b->nl = num_ligand_atoms;
  b->nr = n - num_ligand_atoms;
  b->device = device;
  b->sub2complex.reserve(n);
  for (int pass = 0; pass < 2; pass++)  // the receptor's atoms, then the ligand's, both in ascending complex order
    for (int i = 0; i < n; i++)
      if (is_ligand[i] == pass) b->sub2complex.push_back(i);
  b->complex2sub.resize(n);
  for (int t = 0; t < n; t++) b->complex2sub[b->sub2complex[t]] = t;

  auto bail = [&](int code) {  // (the message is the failed agbnp_hip_create's, or already set)
    agbnp_hip_binding_destroy(b);
    return code;
  };
  // the complex first: its parameter checks (the reference's equal-gamma error among them) run on the host before its first
  // device call, and a subset of equal gammas is equal
  for (int k = 0; k < kBindingMembers; k++) {
    const MemberParams p = member_params(b, k, radius, gamma, vdw_alpha, charge, ishydrogen);
    const int rc = agbnp_hip_create(&b->m[k], (int)p.h.size(), p.r.data(), p.g.data(), p.a.data(), p.q.data(), p.h.data(), version,
                                    nonbonded_method, cutoff, device);
    if (rc != AGBNP_HIP_OK) return bail(rc);
  }
  std::vector<int> maps(b->sub2complex);
  maps.insert(maps.end(), b->complex2sub.begin(), b->complex2sub.end());
  hipError_t e = b->d_maps.upload(maps);
  if (e == hipSuccess) e = b->d_work.alloc(9 * (size_t)n + 3, 0);
  if (e != hipSuccess) {
    binding_fail(AGBNP_HIP_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return bail(AGBNP_HIP_ERR_DEVICE);
  }
  *out = b;
  return AGBNP_HIP_OK;
}

int agbnp_hip_binding_execute_device(agbnp_hip_binding* b, const double* d_positions, double lambda, double* d_forces, double* d_energy,
                                     double* d_binding_energy, void* stream) {
  return binding_device(b, d_positions, lambda, d_forces, false, d_energy, d_binding_energy, stream, "agbnp_hip_binding_execute_device");
}

int agbnp_hip_binding_energy_device(agbnp_hip_binding* b, const double* d_positions, double lambda, double* d_energy,
                                    double* d_binding_energy, void* stream) {
  return binding_device(b, d_positions, lambda, nullptr, true, d_energy, d_binding_energy, stream, "agbnp_hip_binding_energy_device");
}

int agbnp_hip_binding_execute_host(agbnp_hip_binding* b, const double* positions, double lambda, double* forces, double* energy,
                                   double* binding_energy) {
  const char* who = "agbnp_hip_binding_execute_host";
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!positions || !forces) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  if (!std::isfinite(lambda)) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": lambda must be finite");
  return binding_host(b, positions, lambda, forces, energy, binding_energy, who);
}

int agbnp_hip_binding_energy_host(agbnp_hip_binding* b, const double* positions, double lambda, double* energy, double* binding_energy) {
  const char* who = "agbnp_hip_binding_energy_host";
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!positions || (!energy && !binding_energy)) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  if (!std::isfinite(lambda)) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": lambda must be finite");
  return binding_host(b, positions, lambda, nullptr, energy, binding_energy, who);
}

int agbnp_hip_binding_decompose_device(agbnp_hip_binding* b, const double* d_positions, double* d_per_atom, double* d_binding_energy,
                                       void* stream) {
  return binding_analysis_device(b, Analysis::planes, d_positions, d_per_atom, d_binding_energy, stream, "agbnp_hip_binding_decompose_device");
}

int agbnp_hip_binding_decompose_host(agbnp_hip_binding* b, const double* positions, double* per_atom, double* binding_energy) {
  return binding_analysis_host(b, Analysis::planes, positions, per_atom, binding_energy, "agbnp_hip_binding_decompose_host");
}

// The partition is checked here, entirely, before any member is touched: what a member's agbnp_hip_set_atom_sets could refuse of
// its restriction has been refused already, so a refused partition leaves the previous one in force in all three.  Each member
// gets the restriction to its atoms in its own atom order, with the complex's set numbers and S (a set without an atom in a member
// is an empty set there).  The members wait for what may be reading the tables they replace; the staging buffer of another S is
// released behind them, once the caller streams the binding has noted have drained too.
int agbnp_hip_binding_set_atom_sets(agbnp_hip_binding* b, int n, const int* set_of_atom, int num_sets) {
  const char* who = "agbnp_hip_binding_set_atom_sets";
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!set_of_atom) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  if (n != b->n) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": the number of particles differs from the complex's");
  if (num_sets < 1 || num_sets > AGBNP_HIP_MAX_SETS)
    return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": num_sets must be 1 .. AGBNP_HIP_MAX_SETS");
  for (int i = 0; i < n; i++)
    if (set_of_atom[i] < 0 || set_of_atom[i] >= num_sets)
      return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT,
                          std::string(who) + ": atom " + std::to_string(i) + " names a set outside 0 .. num_sets - 1");
  clear_member_errors(b);
  for (int k = 0; k < kBindingMembers; k++) {
    std::vector<int> own(b->member_size(k));
    for (size_t t = 0; t < own.size(); t++) own[t] = set_of_atom[b->member_atom(k, (int)t)];
    const int rc = agbnp_hip_set_atom_sets(b->m[k], (int)own.size(), own.data(), num_sets);
    if (rc != AGBNP_HIP_OK) return member_fail(b, rc, who);  // (a device error: nothing the checks above could have found)
  }
  DevBuf<double>& matrices = b->of(Analysis::matrix).members;
  if (num_sets != b->num_sets && matrices.p) {
    BINDING_TRY(who, hipSetDevice(b->device));
    BINDING_TRY(who, hipStreamSynchronize(b->m[0]->stream));
    for (void* s : b->streams) BINDING_TRY(who, hipStreamSynchronize((hipStream_t)s));
    matrices.release();
  }
  b->set_of_atom.assign(set_of_atom, set_of_atom + n);
  b->num_sets = num_sets;
  return AGBNP_HIP_OK;
}

int agbnp_hip_binding_num_atom_sets(const agbnp_hip_binding* b) { return b ? b->num_sets : 0; }

int agbnp_hip_binding_pair_matrix_device(agbnp_hip_binding* b, const double* d_positions, double* d_matrix, double* d_binding_energy,
                                         void* stream) {
  return binding_analysis_device(b, Analysis::matrix, d_positions, d_matrix, d_binding_energy, stream, "agbnp_hip_binding_pair_matrix_device");
}

int agbnp_hip_binding_pair_matrix_host(agbnp_hip_binding* b, const double* positions, double* matrix, double* binding_energy) {
  return binding_analysis_host(b, Analysis::matrix, positions, matrix, binding_energy, "agbnp_hip_binding_pair_matrix_host");
}

int agbnp_hip_binding_execute_group(agbnp_hip_binding* const* bindings, int count, const double* const* d_positions, const double* d_lambdas,
                                    double* const* d_forces, double* const* d_energies, double* const* d_binding_energies, void* stream) {
  return binding_group_device(bindings, count, d_positions, d_lambdas, d_forces, false, d_energies, d_binding_energies, stream,
                              "agbnp_hip_binding_execute_group");
}

int agbnp_hip_binding_energy_group(agbnp_hip_binding* const* bindings, int count, const double* const* d_positions, const double* d_lambdas,
                                   double* const* d_energies, double* const* d_binding_energies, void* stream) {
  return binding_group_device(bindings, count, d_positions, d_lambdas, nullptr, true, d_energies, d_binding_energies, stream,
                              "agbnp_hip_binding_energy_group");
}

int agbnp_hip_binding_execute_group_host(agbnp_hip_binding* const* bindings, int count, const double* const* positions, const double* lambdas,
                                         double* const* forces, double* energies, double* binding_energies) {
  return binding_group_host(bindings, count, positions, lambdas, forces, false, energies, binding_energies,
                            "agbnp_hip_binding_execute_group_host");
}

int agbnp_hip_binding_energy_group_host(agbnp_hip_binding* const* bindings, int count, const double* const* positions, const double* lambdas,
                                        double* energies, double* binding_energies) {
  return binding_group_host(bindings, count, positions, lambdas, nullptr, true, energies, binding_energies,
                            "agbnp_hip_binding_energy_group_host");
}

int agbnp_hip_binding_finish(agbnp_hip_binding* b, void* stream, int* must_repeat) {
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  int count = 0;
  std::vector<int> bad;
  const int rc = binding_harvest(b, stream, bad, &count, "agbnp_hip_binding_finish");
  // (evaluations that a host entry point in between had to harvest were enqueued before everything read now: they come first)
  b->withheld = b->carried;
  for (int k : bad) b->withheld.push_back(k + b->carried_seq);
  b->withheld_count = b->carried_count + count;
  b->carried.clear();
  b->carried_count = b->carried_seq = 0;
  b->enqueued = 0;
  b->streams.erase(std::remove(b->streams.begin(), b->streams.end(), stream), b->streams.end());
  if (must_repeat) *must_repeat = b->withheld_count;
  return rc;
}

int agbnp_hip_binding_withheld_evaluations(const agbnp_hip_binding* b, int* indices, int capacity) {
  if (!b) return -1;
  for (int k = 0; k < capacity && k < (int)b->withheld.size() && indices; k++) indices[k] = b->withheld[k];
  return b->withheld_count;
}

int agbnp_hip_binding_expect_jump(agbnp_hip_binding* b) {
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  for (agbnp_hip_context* c : b->m) (void)agbnp_hip_expect_jump(c);
  return AGBNP_HIP_OK;
}

int agbnp_hip_binding_update_parameters(agbnp_hip_binding* b, int n, const double* radius, const double* gamma, const double* vdw_alpha,
                                        const double* charge, const int* ishydrogen) {
  const char* who = "agbnp_hip_binding_update_parameters";
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!radius || !gamma || !vdw_alpha || !charge || !ishydrogen) return binding_fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  if (n != b->n) return binding_fail(AGBNP_HIP_ERR_PARAMETERS, "updateParametersInContext: The number of AGBNP particles has changed");
  // (a member drains its own stream and the caller streams it has noted; the binding's buffers are not touched)
  clear_member_errors(b);
  for (int k = 0; k < kBindingMembers; k++) {
    const MemberParams p = member_params(b, k, radius, gamma, vdw_alpha, charge, ishydrogen);
    const int rc = agbnp_hip_update_parameters(b->m[k], (int)p.h.size(), p.r.data(), p.g.data(), p.a.data(), p.q.data(), p.h.data());
    if (rc != AGBNP_HIP_OK) return member_fail(b, rc, who);
  }
  return AGBNP_HIP_OK;
}

int agbnp_hip_binding_set_mode(agbnp_hip_binding* b, int mode) {
  if (!b) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  clear_member_errors(b);
  for (agbnp_hip_context* c : b->m) {
    const int rc = agbnp_hip_set_mode(c, mode);
    if (rc != AGBNP_HIP_OK) return member_fail(b, rc, "agbnp_hip_binding_set_mode");
  }
  return AGBNP_HIP_OK;
}

agbnp_hip_context* agbnp_hip_binding_member(agbnp_hip_binding* b, int which) {
  if (!b || which < 0 || which >= kBindingMembers) return nullptr;
  return b->m[which];
}

void agbnp_hip_binding_destroy(agbnp_hip_binding* b) {
  if (!b) return;
  for (agbnp_hip_context* c : b->m) agbnp_hip_destroy(c);  // (each drains its own stream)
  if (b->group_event) (void)hipEventDestroy(b->group_event);
  delete b;  // (hipFree waits for what is still in flight on a caller's stream)
}

}  // extern "C"
