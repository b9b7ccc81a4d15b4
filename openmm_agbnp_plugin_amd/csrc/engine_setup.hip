// A context's life (engine_context.h): agbnp_hip_create, agbnp_hip_update_parameters, agbnp_hip_destroy; its device arrays, and
// the argument blocks P and T -- every member that never changes is written where its array is allocated, what follows from the
// mode, the diagnostics switch, the row boost or the capacity variant by derive_args, what alternates with the evaluation's
// parity by apply_parity.
#include "engine_context.h"

thread_local std::string g_create_error;

EngineSettings read_settings() {
  EngineSettings s;
  if (const char* v = getenv("AGBNP_HIP_FIVE_LAUNCHES")) s.five_launches = atoi(v) != 0;
  if (const char* v = getenv("AGBNP_HIP_ROWS")) s.rows = atoi(v) != 0 ? 1 : 0;
  if (const char* v = getenv("AGBNP_HIP_HEAL")) s.heal = atoi(v) != 0;
  if (const char* v = getenv("AGBNP_HIP_SPLIT_FIT")) s.split_fit = atoi(v) != 0;
  if (const char* v = getenv("AGBNP_HIP_GB_FAR")) s.gb_far = atoi(v) != 0 ? 1 : 0;
  if (const char* v = getenv("AGBNP_HIP_ROUND_PERMILLE")) s.round_permille = std::max(100, atoi(v));
  if (const char* v = getenv("AGBNP_HIP_REPLAN_EVERY")) s.replan_every = std::max(1, atoi(v));
  if (const char* v = getenv("AGBNP_HIP_ADAPTER_LAUNCH")) s.adapter_launch = atoi(v) != 0;
  if (getenv("AGBNP_HIP_NO_PINNED_STAGING")) s.pinned_staging = false;
  if (const char* v = getenv("AGBNP_HIP_SKIN")) s.skin = std::min(1.0, std::max(0.0, atof(v)));
  if (const char* v = getenv("AGBNP_HIP_ROW_MOVE")) s.row_move = std::max(atof(v), 0.0);
  if (const char* v = getenv("AGBNP_HIP_ROW_SLICE")) s.row_slice = atoi(v);
  if (const char* v = getenv("AGBNP_HIP_ROW_FILL")) s.row_fill = std::max(0.01, atof(v));
  if (const char* v = getenv("AGBNP_HIP_ROW_STRIDE")) s.row_stride = std::max(128, atoi(v));
  if (const char* v = getenv("AGBNP_HIP_MASK_SKIN")) s.mask_skin = std::min(0.5, std::max(0.0, atof(v)));
  if (const char* v = getenv("AGBNP_HIP_GROUP_LAUNCHES")) s.group_launches = atoi(v) != 0;
  return s;
}

namespace {

// Conservative squared cutoff of the 2-body overlap search: beyond it no pair of heavy atoms can have
// an unswitched overlap volume above VOLMINA (gaussvol.cpp:60-93 solved for d^2), so the pruned pairs
// would have been rejected by the volume test anyway.
double overlap_search_cutoff2(const std::vector<double>& a_large, const std::vector<double>& v_large) {
  std::vector<std::pair<double, double>> kinds;
  for (size_t i = 0; i < a_large.size(); i++) {
    std::pair<double, double> k(a_large[i], v_large[i]);
    if (std::find(kinds.begin(), kinds.end(), k) == kinds.end()) kinds.push_back(k);
  }
  double best = 0.0;
  for (auto& k1 : kinds)
    for (auto& k2 : kinds) {
      const double df = k1.first * k2.first / (k1.first + k2.first);
      const double pref = k1.second * k2.second * pow(df / kPi, 1.5);
      if (pref > kVolMinA) best = std::max(best, log(pref / kVolMinA) / df);
    }
  return best * (1.0 + 1e-6) + 1e-9;
}

// agbnp_hip_update_parameters -- gamma, alpha and charge are all that may change there (radii and the hydrogen flags are refused
// before), so three arrays travel instead of nine
int upload_changed_parameters(agbnp_hip_context* c) {
  const int n = c->n, nh = c->nh;
  if (c->h_xfer) {  // through the pinned staging of the host-facing paths: three copies in front of one wait
    double* q = c->h_xfer, *a = q + n, *g = a + n;
    for (int i = 0; i < n; i++) q[i] = c->charge[i], a[i] = c->alpha[i];
    for (int h = 0; h < nh; h++) g[h] = c->gamma[c->h2a[h]] / kRadiusIncrement;
    HIP_TRY(c, hipMemcpyAsync(c->d_charge.p, q, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_alpha.p, a, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    for (int t = 0; t < c->tables() && nh > 0; t++)
      HIP_TRY(c, hipMemcpyAsync(c->htable(t) + (size_t)kHvGam * c->hstride, g, sizeof(double) * nh, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return AGBNP_HIP_OK;
  }
  std::vector<double> gam_cav(nh);
  for (int h = 0; h < nh; h++) gam_cav[h] = c->gamma[c->h2a[h]] / kRadiusIncrement;
  HIP_TRY(c, c->d_charge.upload(c->charge));
  HIP_TRY(c, c->d_alpha.upload(c->alpha));
  for (int t = 0; t < c->tables() && nh > 0; t++)
    HIP_TRY(c, hipMemcpy(c->htable(t) + (size_t)kHvGam * c->hstride, gam_cav.data(), sizeof(double) * nh, hipMemcpyHostToDevice));
  return AGBNP_HIP_OK;
}

// agbnp_hip_create: every parameter array, the heavy-atom table(s) and the cutoff of the overlap search
int upload_parameters(agbnp_hip_context* c) {
  const int n = c->n, nh = c->nh;
  PairArgs& P = c->P;
  std::vector<double> inv_rvdw(n), inv_vol_h(nh), gam_cav(nh), a_large(nh), v_large(nh), a_vdw(nh), v_vdw(nh);
  const double roffset = kRadiusIncrement;  // versions 0 and 1 (ReferenceAGBNPKernels.cpp:67-70)
  for (int i = 0; i < n; i++) inv_rvdw[i] = 1. / c->r_vdw[i];
  for (int h = 0; h < nh; h++) {
    const int i = c->h2a[h];
    const double rv = c->r_vdw[i];
    const double rl = rv + roffset;
    a_large[h] = kKFC / (rl * rl);
    v_large[h] = 4. * M_PI * pow(rl, 3) / 3.;
    a_vdw[h] = kKFC / (rv * rv);
    v_vdw[h] = 4. * M_PI * pow(rv, 3) / 3.;
    inv_vol_h[h] = 1.0 / v_vdw[h];
    gam_cav[h] = c->gamma[i] / roffset;
  }
  HIP_TRY(c, c->d_charge.upload(c->charge));
  HIP_TRY(c, c->d_alpha.upload(c->alpha));
  P.charge = c->d_charge.p;
  P.alpha = c->d_alpha.p;
  HIP_TRY(c, device_array(c, &P.inv_rvdw, inv_rvdw));
  {  // the heavy table's 1/V row once more, by ATOM (0 for hydrogens): k_prep fills the rows' records without waiting for a
     // heavy index first
    std::vector<double> inv_vol_a(n, 0.0);
    for (int h = 0; h < nh; h++) inv_vol_a[c->h2a[h]] = inv_vol_h[h];
    HIP_TRY(c, device_array(c, &P.inv_vol_a, inv_vol_a));
  }
  c->hstride = (c->nhp() + 63) / 64 * 64;
  HIP_TRY(c, c->d_heavy.alloc(c->tables() * kHvRows * c->hstride, 0));
  P.hstride = c->T.hstride = (unsigned)c->hstride;
  P.table_doubles = c->T.table_doubles = (size_t)kHvRows * c->hstride;
  auto put = [&](int row, const std::vector<double>& v) {  // in place: the addresses stay valid for captured graphs
    hipError_t e = hipSuccess;
    for (int t = 0; t < c->tables() && !v.empty() && e == hipSuccess; t++)
      e = hipMemcpy(c->htable(t) + (size_t)row * c->hstride, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice);
    return e;
  };
  HIP_TRY(c, put(kHvInvVol, inv_vol_h));
  HIP_TRY(c, put(kHvGam, gam_cav));
  HIP_TRY(c, put(kHvALarge, a_large));
  HIP_TRY(c, put(kHvVLarge, v_large));
  HIP_TRY(c, put(kHvAVdw, a_vdw));
  HIP_TRY(c, put(kHvVVdw, v_vdw));
  P.rcut2 = c->T.rcut2 = overlap_search_cutoff2(a_large, v_large);
  return AGBNP_HIP_OK;
}

}  // namespace

int ensure_scratch(agbnp_hip_context* c) {
  // topology store: fixed stride per subtree, sized for the current variant
  const size_t nslots = (size_t)c->slot_cap;
  const size_t need_nodes = nslots * (size_t)tree_variant_node_cap(c->variant);
  const size_t need_atoms = nslots * (size_t)tree_variant_atom_cap(c->variant);
  if (c->d_node_pool.count < need_nodes) {
    HIP_TRY(c, c->d_node_pool.alloc(need_nodes));
    c->T.node_pool = c->d_node_pool.p;
    c->generation++;
  }
  const size_t need_pairs = c->variant <= 1 ? 4 * need_nodes : 0;  // membership pairs of the variants up to 512 nodes
  if (c->d_pair_pool.count < need_pairs) {
    HIP_TRY(c, c->d_pair_pool.alloc(need_pairs));
    c->T.pair_pool = c->d_pair_pool.p;
    c->generation++;
  }
  if (c->d_atom_pool.count < need_atoms) {
    HIP_TRY(c, c->d_atom_pool.alloc(need_atoms));
    c->T.atom_pool = c->d_atom_pool.p;
    c->generation++;
  }
  if (c->variant != kGlobalVariant) return AGBNP_HIP_OK;
  const size_t stride = tree_variant_scratch_bytes(kGlobalVariant);
  const size_t need = stride * std::min((size_t)kGlobalGrid, c->nhp());
  if (c->d_scratch.count < need) {
    HIP_TRY(c, c->d_scratch.alloc(need));
    c->generation++;
  }
  c->T.scratch = c->d_scratch.p;
  return AGBNP_HIP_OK;
}

// The members of the argument blocks that name one of the two sets of {heavy-atom table, subtree shapes, per-evaluation status
// words}.  Five-launch mode, eager (five == 1): the set of the evaluation about to be enqueued, five_evals & 1 -- the host
// counts.  From a context's first stream capture on (five == 2): set 0, and every kernel moves them to the set the DEVICE's
// count names (PairArgs::epoch, rebase_for_parity in pair_kernels.h).  The device counts in either form, so the two agree.
void apply_parity(agbnp_hip_context* c) {
  PairArgs& P = c->P;
  TreeArgs& T = c->T;
  const bool five = c->five_active;
  const bool host_names = five && !c->five_device;
  const int p = host_names ? (c->five_evals & 1) : 0;
  auto row = [&](int r) { return c->htable(p) + (size_t)r * c->hstride; };
  P.inv_vol_h = row(kHvInvVol);  // (static rows: the same in both tables)
  P.gam_cav = row(kHvGam);
  P.a_large = row(kHvALarge);
  P.v_large = row(kHvVLarge);
  P.hx = row(kHvX);
  P.hy = row(kHvY);
  P.hz = row(kHvZ);
  P.gx = row(kHvGx);
  P.gy = row(kHvGy);
  P.gz = row(kHvGz);
  P.sv_vdw = row(kHvSvVdw);
  P.sv_large = row(kHvSvLarge);
  T.hv = c->htable(p);
  P.sizes = T.sizes = c->sizes(p);
  P.estatus = five ? c->d_estatus.p + kStatBlockStride * p : c->d_status.p;
  T.status = P.estatus;  // (the tree kernels only touch words of their own evaluation)
  P.five = T.five = five ? (c->five_device ? 2 : 1) : 0;
  // (five == 1: the host names the set the trailing workgroups clear, too; five == 2: rebase_for_parity does)
  P.next_hv = host_names ? c->htable(1 - p) : nullptr;
  P.next_sizes = host_names ? c->sizes(1 - p) : nullptr;
  P.next_estatus = host_names ? c->d_estatus.p + kStatBlockStride * (1 - p) : nullptr;
  P.row_atoms = five ? c->d_row_atoms.p : nullptr;
  T.row_atoms = P.row_atoms;
  // the masks of that mode reach a skin further than the exact test of the level-2 search does
  const double reach = sqrt(c->T.rcut2) + (five ? c->cfg.mask_skin : 0.0);
  P.mask_rcut2 = five ? reach * reach : c->T.rcut2;
}

// The members of the argument blocks that follow from the mode bits, the diagnostics switch, the row boost (and rows_disabled)
// and the capacity variant -- every other member is written once, where its array is allocated.  Called by agbnp_hip_create,
// agbnp_hip_set_mode, agbnp_hip_set_diagnostics and the harvest that widens the rows' walk.
void derive_args(agbnp_hip_context* c) {
  PairArgs& P = c->P;
  // The OpenCL platform only defines USE_CUTOFF for a method other than NoCutoff (OpenCLAGBNPKernels.cpp:487,1149-1150): with
  // NoCutoff the fast mode truncates nothing and IS the reference mode (the cutoff distance "will have no effect",
  // AGBNPForce.h); CutoffPeriodic is refused by agbnp_hip_set_mode (no box vectors cross this boundary).
  const bool cut = (c->mode & AGBNP_HIP_MODE_FAST) && c->method != 0;
  P.fast = cut ? 1 : 0;
  P.single = cut && (c->mode & AGBNP_HIP_MODE_SINGLE) ? 1 : 0;
  P.det = c->T.det = (c->mode & AGBNP_HIP_MODE_DETERMINISTIC) ? 1 : 0;
  P.range2 = P.fast ? std::min(kI4MaxA * kI4MaxA, c->cutoff * c->cutoff) : kI4MaxA * kI4MaxA;
  P.gb_cut2 = P.fast ? c->cutoff * c->cutoff : 1e300;
  // far strips (pair_kernels.hip, gb_strip): only systems with more than 8192 atoms can have blocks some 4 nm apart in
  // numbers that pay for the test (1dwc, 4152 atoms: none; 2clr, 5983: 3-5 %); AGBNP_HIP_GB_FAR = 0 / 1 forces it (tests)
  P.gb_far = !P.fast && (c->cfg.gb_far >= 0 ? c->cfg.gb_far != 0 : c->n > 8192) ? 1 : 0;
  // Row form (reference mode only: the fast mode cuts every stage at the cutoff and the deterministic mode fixes the
  // order of its sums through the tiles' quantized totals)
  const bool wanted = c->cfg.rows != 0;  // (AGBNP_HIP_ROWS=0: the tile kernels everywhere)
  // (the single-precision option of the fast mode lives in the GB stage: in the GB rows where they can run, else in the
  // packed-FP32 strips of the tile form)
  const bool gb_rows_possible = P.fast && P.nlg != nullptr;
  P.rows_on = c->rows_capable && !c->rows_disabled && c->version == 1 && !P.det && (!P.single || gb_rows_possible) && wanted ? 1 : 0;
  P.gb_rows = P.rows_on && gb_rows_possible ? 1 : 0;
  const double reach = sqrt(P.range2) + c->skin, gb_reach = c->cutoff + c->skin;  // (fast mode: the range-limited stages stop at the cutoff too)
  P.nl_build2 = reach * reach;
  P.nlg_build2 = gb_reach * gb_reach;
  // what the launches walk of a list: the atoms that 1.5 x the density of a protein interior (105 atoms, 52 heavy ones
  // per nm^3) puts within reach + skin of a group of four bonded atoms (0.3 nm across), per part, in slices of 256 --
  // times row_boost after a list has outgrown it
  auto cap = [&](double radius, double density, int parts, int stride) {
    const double r = radius + 0.3, most = c->cfg.row_fill * density * (4.0 / 3.0) * M_PI * r * r * r / parts * c->row_boost;
    return std::min(std::max(256, (int)std::min(most + 255.0, 1e9) / 256 * 256), std::max(stride, 1));
  };
  P.nlh_cap = cap(reach, 52.0, kBornParts, P.nlh_stride);
  P.nla_cap = cap(reach, 105.0, kChainParts, P.nla_stride);
  P.nlg_cap = cap(gb_reach, 105.0, kGbParts, P.nlg_stride);
  const DevBuf<double>& egb = P.gb_rows ? c->d_egb_rows : c->d_egb_part;  // (the GB rows leave one energy partial per wave)
  P.egb_part = egb.p;
  P.egb_parts = (int)egb.count;
  P.tree_node_cap = tree_variant_node_cap(c->variant);
  P.tree_atom_cap = tree_variant_atom_cap(c->variant);
  P.pack_enabled = 1;  // (a freeze by agbnp_debug_set_packing ends here)
  c->T.want_sv_large = c->diagnostics ? 1 : 0;  // pass-1 self volumes cost extra HBM atomics: opt-in
  apply_parity(c);
}

// the neighbour lists (and their work items) are rebuilt by the next evaluation
int mark_rows_stale(agbnp_hip_context* c) {
  const int stale = 1;
  HIP_TRY(c, hipMemcpy(c->d_nl_flag.p + kNlStale, &stale, sizeof(int), hipMemcpyHostToDevice));
  return AGBNP_HIP_OK;
}

namespace {

// Arrays of the row form of the range-limited stages (k_rows): candidate orders sorted by type, neighbour rows at a fixed
// stride, the power-form spline coefficients.  Systems it does not take (version 0, more radius types than the per-wave
// table slices hold, more particles than the row buffers are sized for) simply keep the tile kernels.
int allocate_rows(agbnp_hip_context* c) {
  const int n = c->n, nh = c->nh;
  PairArgs& P = c->P;
  constexpr int kRowCap = 3072;      // entries per row (part): no protein holds that many heavy atoms within 2.1 nm of one point
  constexpr int kMaxTypes = 255;     // a row's type is one byte of its group's slice word
  constexpr size_t kMaxTableBytes = 40 * 1024;  // the power-form table lives in LDS whole (1dwc: 8 x 6 types, 23 KB)
  constexpr int kMaxParticles = 65536;
  if (c->version != 1 || nh == 0 || n > kMaxParticles || c->cfg.rows == 0) return AGBNP_HIP_OK;
  if (c->lut.nscreened > kMaxTypes || c->lut.nscreener > kMaxTypes) return AGBNP_HIP_OK;
  if ((size_t)c->lut.nscreened * c->lut.nscreener * (kI4Nodes - 1) * 2 * sizeof(double2) > kMaxTableBytes) return AGBNP_HIP_OK;
  c->skin = c->cfg.skin;
  c->row_move = c->cfg.row_move;
  c->row_slice = c->cfg.row_slice;
  auto sorted_by_type = [&](int count, auto type_of) {
    std::vector<unsigned> v;
    for (int k = 0; k < count; k++) v.push_back(make_row_entry((unsigned)k, (unsigned)type_of(k)));
    std::stable_sort(v.begin(), v.end(), [](unsigned a, unsigned b) { return row_entry_type(a) < row_entry_type(b); });
    while (v.size() % 64 != 0) v.push_back(~0u);
    return v;
  };
  const std::vector<unsigned> hperm = sorted_by_type(nh, [&](int h) { return c->lut.type_screener[c->h2a[h]]; });
  const std::vector<unsigned> aperm = sorted_by_type(n, [&](int a) { return c->lut.type_screened[a]; });
  HIP_TRY(c, device_array(c, &P.hperm, hperm));
  HIP_TRY(c, device_array(c, &P.aperm, aperm));
  P.hperm_n = (int)hperm.size();
  P.aperm_n = (int)aperm.size();
  // a list part takes every kBornParts-th (kChainParts-th) chunk of 64 candidates: it can hold all of them, up to the cap
  auto part_stride = [&](size_t candidates, int parts) { return std::max(128, std::min(64 * (int)((candidates / 64 + parts - 1) / parts), kRowCap)); };
  static_assert(kRowCap % 256 == 0, "a list is walked in slices of 256 entries");
  P.nlh_stride = part_stride(hperm.size(), kBornParts);
  P.nla_stride = part_stride(aperm.size(), kChainParts);
  // GB rows (fast mode; the cutoff is the force's and fixed for the life of the context): a list holds the atoms within
  // cutoff + skin of a group of four bonded atoms -- at most what twice the density of a protein interior (~105 atoms per
  // nm^3) puts into that sphere, whatever the size of the system
  {
    const double r = c->cutoff + c->skin + 0.3;
    const double most = 2.0 * 105.0 * (4.0 / 3.0) * M_PI * r * r * r / kGbParts;
    P.nlg_stride = c->method != 0 && c->cutoff > 0.0 && c->cutoff < 3.0
                       ? std::max(256, std::min(part_stride(aperm.size(), kGbParts), (int)((most + 255) / 256) * 256)) : 0;
  }
  if (c->cfg.row_stride > 0) {  // (tests: force an overflow)
    P.nlh_stride = P.nla_stride = c->cfg.row_stride;
    if (P.nlg_stride) P.nlg_stride = P.nlh_stride;
  }
  const size_t born_lists = (size_t)row_groups(n) * kBornParts, chain_lists = (size_t)row_groups(nh) * kChainParts;
  const size_t gb_lists = P.nlg_stride > 0 ? (size_t)row_groups(n) * kGbParts : 0;
  HIP_TRY(c, device_array(c, &P.nlh, born_lists * P.nlh_stride, 0));  // (entries beyond a list's length are read: valid indices)
  HIP_TRY(c, device_array(c, &P.nla, chain_lists * P.nla_stride, 0));
  HIP_TRY(c, device_array(c, &P.nlh_count, born_lists, 0));
  HIP_TRY(c, device_array(c, &P.nla_count, chain_lists, 0));
  {
    std::vector<unsigned> bs(row_groups(n), 0u), cs(row_groups(nh), 0u);
    for (int a = 0; a < n; a++) bs[a / kRowGroup] |= (unsigned)c->lut.type_screened[a] << (8 * (a % kRowGroup));
    for (int h = 0; h < nh; h++) cs[h / kRowGroup] |= (unsigned)c->lut.type_screener[c->h2a[h]] << (8 * (h % kRowGroup));
    HIP_TRY(c, device_array(c, &P.bslice, bs));
    HIP_TRY(c, device_array(c, &P.cslice, cs));
  }
  if (gb_lists > 0) {
    HIP_TRY(c, device_array(c, &P.nlg, gb_lists * P.nlg_stride, 0));
    HIP_TRY(c, device_array(c, &P.nlg_count, gb_lists, 0));
    const size_t waves = (gb_lists + 7) / 8 * 8 * (size_t)((P.nlg_stride + 255) / 256);  // one energy partial per wave of the GB rows
    HIP_TRY(c, c->d_egb_rows.alloc(waves, 0));
  }
  {
    // work items: at most every slice of every list of the largest kind
    const size_t most = std::max(std::max(born_lists * ((P.nlh_stride + 255) / 256), chain_lists * ((P.nla_stride + 255) / 256)),
                                 gb_lists * ((P.nlg_stride + 255) / 256));
    P.nl_items_cap = (int)std::min<size_t>(most + 8, 1u << 30);
    HIP_TRY(c, device_array(c, &P.nl_items, (size_t)kRowKinds * kRowBuffers * P.nl_items_cap, 0));
    HIP_TRY(c, device_array(c, &P.nl_nitems, kRowKinds * kRowBuffers, 0));
  }
  std::vector<int> flag(kNlFlagWords, 0);
  flag[kNlStale] = 1;  // (the first evaluation builds the rows)
  flag[kNlSlice] = c->row_slice > 0 ? std::min(std::max(c->row_slice, kRowSlice), kRowSliceMax) / 64 * 64 : kRowSlice;
  HIP_TRY(c, c->d_nl_flag.upload(flag));
  P.nl_flag = c->d_nl_flag.p;
  HIP_TRY(c, device_array(c, &P.nl_ref, 3 * (size_t)n, 0xff));  // NaN: every atom has "moved"
  HIP_TRY(c, device_array(c, &P.bw, n, 0));
  HIP_TRY(c, device_array(c, &P.rec_h, nh));
  HIP_TRY(c, device_array(c, &P.hrow, nh));
  HIP_TRY(c, device_array(c, &P.grec, n, 0));
  HIP_TRY(c, device_array(c, &P.hrec, nh, 0));
  // Power form of the natural cubic spline on interval k (t in [0, 1)): S = c0 + c1 t + c2 t^2 + c3 t^3 with the same
  // operations the tile kernels use on the knots {y, z = y2 dr^2 / 6} (spline_cubic in pair_kernels.hip)
  const int nti = c->lut.nscreened, ntj = c->lut.nscreener, ni = kI4Nodes - 1;
  const size_t tab = (size_t)nti * ntj * ni;
  const double dr = kI4MaxA / (kI4Nodes - 1);
  std::vector<double2> pw(4 * tab);  // four arrays of tab entries: {c0, c1} / {c2, c3} by [screened][screener], the same by [screener][screened]
  for (int ti = 0; ti < nti; ti++)
    for (int tj = 0; tj < ntj; tj++)
      for (int k = 0; k < ni; k++) {
        const size_t o = ((size_t)ti * ntj + tj) * kI4Nodes + k;
        const double y0 = c->lut.y[o], y1 = c->lut.y[o + 1], z0 = c->lut.y2[o] * dr * dr / 6.0, z1 = c->lut.y2[o + 1] * dr * dr / 6.0;
        const double2 ca = make_double2(y0, (y1 - y0) - std::fma(2.0, z0, z1)), cb = make_double2(3.0 * z0, z1 - z0);
        const size_t by_screened = ((size_t)ti * ntj + tj) * ni + k, by_screener = ((size_t)tj * nti + ti) * ni + k;
        pw[by_screened] = ca;
        pw[tab + by_screened] = cb;
        pw[2 * tab + by_screener] = ca;
        pw[3 * tab + by_screener] = cb;
      }
  HIP_TRY(c, device_array(c, &P.pw_a, pw));
  P.pw_b = P.pw_a + tab;
  P.pwt_a = P.pw_a + 2 * tab;
  P.pwt_b = P.pw_a + 3 * tab;
  c->rows_capable = true;
  return AGBNP_HIP_OK;
}

int allocate_work(agbnp_hip_context* c) {
  const int n = c->n, nh = c->nh;
  PairArgs& P = c->P;
  TreeArgs& T = c->T;
  const size_t n3 = 3 * (size_t)n;
  const int nblk = (n + 63) / 64;
  {
    // work items of the symmetric GB tile kernel: one workgroup per tile, off-diagonal tiles first
    if (nblk > kTileBlocksMax) return c->fail(AGBNP_HIP_ERR_CAPACITY, "more than 262080 particles are not supported by the tile index encoding");
    // away from the diagonal: strips of two i blocks (2p, 2p + 1) against one j block (kTileStripFlag, see gb_strip);
    // around it: single 64 x 64 tiles
    std::vector<int> items;
    items.reserve((size_t)nblk * nblk / 2 + 4);
    for (int p2 = 0; 2 * p2 + 1 < nblk; p2++)
      for (int J = 2 * p2 + 2; J < nblk; J++) items.push_back(make_tile_item(2 * p2, J, kTileStripFlag));
    for (int p2 = 0; 2 * p2 + 1 < nblk; p2++) items.push_back(make_tile_item(2 * p2, 2 * p2 + 1));
    for (int I = 0; I < nblk; I++) items.push_back(make_tile_item(I, I));
    HIP_TRY(c, device_array(c, &P.gb_items, items));
    P.gb_items_count = (int)items.size();
    HIP_TRY(c, c->d_egb_part.alloc(items.size()));  // one energy partial per tile
  }
  {
    // pair order of the chain-rule stage: heavy atoms, padding, hydrogens, padding (blocks of 64 slots), and its
    // work items: symmetric heavy x heavy tiles first (two look-ups per pair), then the heavy x H tiles
    const int nhb = (nh + 63) / 64, nlb = (n - nh + 63) / 64;
    std::vector<int> pslot((size_t)(nhb + nlb) * 64, -1);
    for (int h = 0; h < nh; h++) pslot[h] = c->h2a[h];
    int k = nhb * 64;
    for (int i = 0; i < n; i++)
      if (c->a2h[i] < 0) pslot[k++] = i;
    if (pslot.empty()) pslot.assign(64, -1);
    HIP_TRY(c, device_array(c, &P.pslot, pslot));
    P.nslots = (int)pslot.size();
    P.nhb = nhb;
    P.cull_first = P.nslots / 64 > 96 ? 1 : 0;  // beyond ~6000 atoms most tiles are further apart than the tables reach
    std::vector<int> a2s((size_t)std::max(n, 1), 0);
    for (size_t sl = 0; sl < pslot.size(); sl++)
      if (pslot[sl] >= 0) a2s[pslot[sl]] = (int)sl;
    HIP_TRY(c, device_array(c, &P.a2s, a2s));
    HIP_TRY(c, device_array(c, &P.prec, pslot.size(), 0));
    HIP_TRY(c, device_array(c, &P.srec, pslot.size(), 0));
    HIP_TRY(c, device_array(c, &P.ys, pslot.size(), 0));
    HIP_TRY(c, device_array(c, &P.pbox, 6 * pslot.size() / 64));
    // Work items, heaviest first: diagonal and heavy x heavy tiles (two look-ups per pair), then heavy x H.  The
    // launch is one round (every workgroup resident at once) and workgroup b starts on CU b mod (number of CUs), so
    // the sorted tiles are dealt over the CUs in serpentine order: every CU gets the same mix of heavy and light ones.
    std::vector<int> sorted;
    for (int I = 0; I < nhb; I++) sorted.push_back(make_tile_item(I, I));
    for (int I = 0; I < nhb; I++)
      for (int J = I + 1; J < nhb; J++) sorted.push_back(make_tile_item(I, J));
    for (int I = 0; I < nhb; I++)
      for (int J = nhb; J < nhb + nlb; J++) sorted.push_back(make_tile_item(I, J));
    std::vector<int> items(sorted.size());
    {
      const size_t width = (size_t)std::max(c->cus, 1);
      for (size_t p = 0; p < sorted.size(); p++) {
        const size_t row = p / width, col = p % width;
        const size_t row_len = std::min(width, sorted.size() - row * width);
        items[row * width + ((row & 1) ? row_len - 1 - col : col)] = sorted[p];
      }
    }
    if (items.empty()) items.push_back(0);
    HIP_TRY(c, device_array(c, &P.db_items, items));
    P.db_items_count = nh == 0 ? 0 : (int)items.size();
  }

  {
    int rc = allocate_rows(c);
    if (rc != AGBNP_HIP_OK) return rc;
    // an atom further than this from where it was at the last build makes the lists stale: half the skin -- or
    // AGBNP_HIP_ROW_MOVE (nm; measurement only: 0 rebuilds the lists at every new geometry at the default skin, which is how
    // bench.py prices a rebuild evaluation)
    const double move = c->row_move >= 0.0 ? std::min(c->row_move, 0.5 * c->skin) : 0.5 * c->skin;
    P.nl_move2 = move * move;
    P.row_target = c->row_slice > 0 ? 0 : 2 * c->cus;
  }
  HIP_TRY(c, c->d_status.alloc(kStatTotalWords, 0));
  P.status = c->d_status.p;
  if (hipHostMalloc(reinterpret_cast<void**>(&c->h_status), 4 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess)  // (fine-grained: the host sees the device's writes mid-stream)
    c->h_status[0] = c->h_status[1] = c->h_status[2] = c->h_status[3] = 0;
  else
    c->h_status = nullptr;  // (agbnp_hip_poll then reports "unknown")
  {
    void* dev = nullptr;
    P.host_status = (c->h_status && hipHostGetDevicePointer(&dev, c->h_status, 0) == hipSuccess) ? static_cast<volatile int*>(dev) : nullptr;
  }
  {
    // level-2 neighbour search: tiles of 64x64 heavy atoms (I <= J), one 64-bit mask per (atom, block)
    const int nhb = (nh + 63) / 64;
    if (nhb > kTileBlocksMax) return c->fail(AGBNP_HIP_ERR_CAPACITY, "more than 262080 heavy atoms are not supported by the tile index encoding");
    HIP_TRY(c, device_array(c, &P.nbmask, std::max<size_t>((size_t)nhb * nhb * 64, 64), 0));
    T.nbmask = P.nbmask;
    T.nhb = nhb;
    P.nb_tiles = nhb * (nhb + 1) / 2;
  }
  // up to four work items per subtree (shared subtrees), plus a launch's worth of slots: the spare slots that k_tree_cavity heals an
  // overgrown forest into are numbered from max(forests, forest workgroups of the launch) on, and at most 4 nh sets exist in all
  c->slot_cap = 4 * (int)c->nhp() + c->tree_slots[0];
  const size_t nslots = (size_t)c->slot_cap;
  HIP_TRY(c, device_array(c, &P.epart, 2 * nslots, 0));
  T.epart = P.epart;
  HIP_TRY(c, device_array(c, &P.aposq, n));
  HIP_TRY(c, device_array(c, &P.abox, 6 * (size_t)nblk));
  HIP_TRY(c, c->d_sizes.alloc(c->tables() * c->nhp(), 0));
  P.sizes_stride = T.sizes_stride = c->nhp();
  if (c->five) {
    HIP_TRY(c, c->d_estatus.alloc(2 * kStatBlockStride, 0));  // (fast mode + single keep their own Born rows: no mask tiles there, see five_active)
    HIP_TRY(c, device_array(c, &P.mask_ref, std::vector<double>(3 * c->nhp(), std::nan(""))));
    HIP_TRY(c, c->d_row_atoms.alloc((size_t)kMaxItems * nslots, 0));
  }
  P.mask_move2 = 0.25 * c->cfg.mask_skin * c->cfg.mask_skin;
  HIP_TRY(c, device_array(c, &P.born_part, n));
  HIP_TRY(c, device_array(c, &P.born, n));
  HIP_TRY(c, device_array(c, &P.born_fp, n));
  HIP_TRY(c, device_array(c, &P.brw, n));
  HIP_TRY(c, device_array(c, &P.e_atom, n));
  HIP_TRY(c, device_array(c, &P.gb_fx, n3));
  P.gb_fy = P.gb_fx + n;
  P.gb_fz = P.gb_fx + 2 * (size_t)n;
  HIP_TRY(c, device_array(c, &P.db_fx, 4 * (size_t)n));
  P.db_fy = P.db_fx + n;
  P.db_fz = P.db_fx + 2 * (size_t)n;
  T.db_wu = P.db_wu = P.db_fx + n3;
  HIP_TRY(c, c->d_components.alloc(4));
  HIP_TRY(c, device_array(c, &P.pack_items, nslots + 1, 0));  // (packing_role's scratch)
  {
    int rc = upload_identity_packing(c);  // the first evaluation: nothing is known about the tree yet
    if (rc != AGBNP_HIP_OK) return rc;
    P.order = c->d_order.p;
    P.forest_time = c->d_ftime.p;
    T.rows = P.rows = c->d_rows.p;
    int* const tail = c->d_forest.p + nslots;  // (the packing block: PackingWord, agbnp_common.h)
    P.forest_start = c->d_forest.p;
    P.nforests = tail + kPackForestsNext;
    P.cur_nforests = tail + kPackForestsNow;
    P.pack_state = tail + kPackState;
    T.packing = c->d_forest.p;
    // the device's evaluation counter exists twice, each copy beside what its readers read first (a cold scalar load of its own
    // costs a launch 0.1-0.3 us): the pair launches' in the neighbour rows' flag line (without rows: in words of its own), the
    // tree launches' behind the forest counts; the bookkeeping role advances both
    if (P.nl_flag)
      P.epoch = P.nl_flag + kNlEpoch;
    else if (c->five)
      HIP_TRY(c, device_array(c, &P.epoch, kNlFlagWords, 0));
    T.epoch = P.epoch_tree = P.pack_state + kPsEpoch;
  }
  P.ncus = c->cus;
  P.tree_slot_cap = T.slot_cap = c->slot_cap;
  P.round_permille = c->cfg.round_permille;
  P.replan_every = c->cfg.replan_every;
  // a full device has slot_cap = 2 x subtrees work slots: more parts per subtree than that could plan more work items
  // than forest_start / order / the topology pools hold
  P.split_big = std::max(1, std::min(3, c->slot_cap / (int)c->nhp()));
  P.split_permille = 550;
  P.split_fit = c->cfg.split_fit && c->slot_cap >= 4 * (int)c->nhp() ? 1 : 0;
  // (the tree launches' word: bit 0 the above, bit 1 = forests that outgrow their store are healed inside the launch -- round 6;
  // AGBNP_HIP_HEAL=0: they void the evaluation as in rounds 2-5, for the tests of the withheld-evaluation protocol)
  T.split_fit = P.split_fit | (c->cfg.heal ? 2 : 0);
  T.scratch_stride = tree_variant_scratch_bytes(kGlobalVariant);
  HIP_TRY(c, device_array(c, &T.hdr, nslots, 0));
  HIP_TRY(c, c->d_pos_in.alloc(n3));
  HIP_TRY(c, c->d_ctx_slot.alloc(std::max(n, 1), 0));
  HIP_TRY(c, c->d_hslot.alloc(c->nhp(), 0));
  HIP_TRY(c, c->d_force_tmp.alloc(n3 + 1, 0));  // (+ the energy of agbnp_hip_execute_host)
  HIP_TRY(c, c->d_energy_tmp.alloc(1, 0));
  HIP_TRY(c, c->d_eo_force.alloc(n3, 0));
  c->h_force_tmp.resize(n3 + 1);
  const bool pinned = c->cfg.pinned_staging;  // (tests: the pageable fall-back of the host-facing paths)
  if (!pinned || hipHostMalloc(reinterpret_cast<void**>(&c->h_report), sizeof(agbnp_hip_context::HostReport), hipHostMallocDefault) != hipSuccess) c->h_report = nullptr;
  if (!pinned || hipHostMalloc(reinterpret_cast<void**>(&c->h_xfer), sizeof(double) * (6 * (size_t)n + 8), hipHostMallocDefault) != hipSuccess) c->h_xfer = nullptr;
  (void)hipGetLastError();  // (without pinned memory the host-facing paths fall back to pageable transfers)
  return AGBNP_HIP_OK;
}

}  // namespace

// one work item per work slot (what a context starts with, and what an overflowed evaluation is repeated on): every subtree
// whole, or -- once a lone subtree has outgrown the store (fallback_parts) -- shared among two or four items
int upload_identity_packing(agbnp_hip_context* c) {
  const size_t parts = (size_t)std::max(1, std::min(c->fallback_parts, std::max(1, c->slot_cap / (int)c->nhp())));
  const size_t nhp = c->nhp() * parts, nslots = (size_t)c->slot_cap;
  std::vector<int> ident((size_t)kRowStride * nslots, -1);  // slot s: its one work item, -1 = no item, and the number 1
  for (size_t k = 0; k < nslots; k++) {
    const size_t item = std::min(k, nhp - 1);
    ident[slot_row_item(k, 0)] = make_work_item((int)(item / parts), (int)(item % parts), (int)parts);
    ident[slot_row_count(k)] = 1;
  }
  HIP_TRY(c, c->d_rows.upload(ident));
  if (c->five) {  // (five-launch mode: the atom of every item's root, beside the rows)
    std::vector<int> atoms((size_t)kMaxItems * nslots, 0);
    for (size_t k = 0; k < nslots && c->nh > 0; k++) atoms[(size_t)kMaxItems * k] = c->h2a[std::min(k, nhp - 1) / parts];
    HIP_TRY(c, c->d_row_atoms.upload(atoms));
    set_row_atoms_kind(c, 0);  // (a context that came through agbnp_hip_execute_openmm: its captured graphs are stale until enqueue has rewritten the words)
  }
  HIP_TRY(c, c->d_order.upload(std::vector<int>((size_t)kMaxItems * nslots + 8, 0)));  // (the bookkeeping's working copies)
  HIP_TRY(c, c->d_ftime.upload(std::vector<int>(nslots + 1, 0)));
  // the packing block (PackingWord, agbnp_common.h): every persistent word 0 but the age -- huge: this one is no plan
  std::vector<int> forest(packing_words(nslots), 0);
  const int nitems = c->nh > 0 ? (int)nhp : 0;
  for (size_t k = 0; k <= nslots; k++) forest[k] = (int)std::min(k, (size_t)nitems);
  forest[nslots + kPackForestsNext] = nitems;
  forest[nslots + kPackForestsNow] = nitems;
  forest[nslots + kPackState + kPsAge] = 1 << 20;
  if (c->d_forest.p == nullptr)
    return c->d_forest.upload(forest) == hipSuccess ? AGBNP_HIP_OK : c->fail(AGBNP_HIP_ERR_DEVICE, "upload of the forest packing failed");
  // a context that has run: the forest counts and the age in place, the other persistent words kept
  HIP_TRY(c, hipMemcpy(c->d_forest.p, forest.data(), sizeof(int) * (nslots + kPackState), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_forest.p + nslots + kPackState + kPsAge, &forest[nslots + kPackState + kPsAge], sizeof(int), hipMemcpyHostToDevice));
  return AGBNP_HIP_OK;
}

extern "C" {

int agbnp_hip_create(agbnp_hip_context** out, int n, const double* radius, const double* gamma, const double* vdw_alpha,
                     const double* charge, const int* ishydrogen, int version, int nonbonded_method, double cutoff, int device) {
  auto bail = [&](int code, const std::string& msg, agbnp_hip_context* c) {
    g_create_error = msg;
    delete c;
    if (out) *out = nullptr;
    return code;
  };
  if (!out || n <= 0 || !radius || !gamma || !vdw_alpha || !charge || !ishydrogen)
    return bail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_create: null pointer or non-positive particle count", nullptr);
  if (version < 0 || version > 2) return bail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "AGBNPForce::setVersion(): illegal version number", nullptr);
  if (version == 2)
    return bail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_create: AGBNP version 2 is outside this engine's scope (versions 0 and 1 only)", nullptr);
  if (nonbonded_method < 0 || nonbonded_method > 2)
    return bail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_create: illegal nonbonded method", nullptr);

  agbnp_hip_context* c = new agbnp_hip_context();
  PairArgs& P = c->P;
  c->n = P.n = n;
  c->version = version;
  c->method = nonbonded_method;
  c->cutoff = cutoff;
  c->device = device;
  c->cfg = read_settings();
  c->five = (version == 0 || version == 1) && c->cfg.five_launches;  // (default since round 5, version 0 since round 6)
  c->five_active = c->five;
  c->r_vdw.assign(radius, radius + n);
  c->gamma.resize(n);
  c->alpha.assign(vdw_alpha, vdw_alpha + n);
  c->charge.assign(charge, charge + n);
  c->ish.resize(n);
  c->a2h.assign(n, -1);
  // parameter checks of ReferenceAGBNPKernels.cpp:96-117
  double common_gamma = -1;
  for (int i = 0; i < n; i++) {
    const bool h = ishydrogen[i] != 0;
    c->ish[i] = h ? 1 : 0;
    c->gamma[i] = h ? 0.0 : gamma[i];
    if (!(radius[i] > 0.0)) return bail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_create: particle radius must be positive", c);
    if (common_gamma < 0 && !h) {
      common_gamma = gamma[i];
    } else if (!h && pow(common_gamma - gamma[i], 2) > FLT_MIN) {
      return bail(AGBNP_HIP_ERR_PARAMETERS, "initialize(): AGBNP does not support multiple gamma values.", c);
    }
    if (!h) {
      c->a2h[i] = (int)c->h2a.size();
      c->h2a.push_back(i);
    }
  }
  c->nh = P.nh = c->T.nh = (int)c->h2a.size();
  c->lut.build(c->r_vdw, c->ish);

  int ndev = 0;
  hipError_t he = hipGetDeviceCount(&ndev);
  if (he != hipSuccess || ndev <= 0)
    return bail(AGBNP_HIP_ERR_DEVICE, "agbnp_hip_create: no HIP device available (this engine has no CPU fallback)", c);
  if (device < 0 || device >= ndev) return bail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_create: device index out of range", c);
#define CREATE_TRY(call)                                                                      \
  do {                                                                                        \
    hipError_t e__ = (call);                                                                  \
    if (e__ != hipSuccess) return bail(AGBNP_HIP_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e__), c); \
  } while (0)
  CREATE_TRY(hipSetDevice(device));
  {
    // resident tree workgroups per capacity variant: what one "round" of the forest packing is
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    c->cus = cus;
    for (int v = 0; v < kGlobalVariant; v++) c->tree_slots[v] = tree_variant_wgs_per_cu(v) * cus;
    c->tree_slots[kGlobalVariant] = kGlobalGrid;
  }
  CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));

  CREATE_TRY(device_array(c, &P.a2h, c->a2h));
  std::vector<int> h2a_pad = c->h2a;
  if (h2a_pad.empty()) h2a_pad.push_back(0);
  CREATE_TRY(device_array(c, &P.h2a, h2a_pad));
  std::vector<int2> ameta(n);
  for (int i = 0; i < n; i++) ameta[i] = make_int2(c->lut.type_screened[i], c->lut.type_screener[i]);
  CREATE_TRY(device_array(c, &P.ameta, ameta));
  const double dr = kI4MaxA / (kI4Nodes - 1);
  std::vector<double2> lut(std::max<size_t>(1, c->lut.y.size() / kI4Nodes * kLutStride), make_double2(0.0, 0.0));
  for (size_t k = 0; k < c->lut.y.size(); k++)  // rows padded to kLutStride entries (LDS bank spreading)
    lut[k / kI4Nodes * kLutStride + k % kI4Nodes] = make_double2(c->lut.y[k], c->lut.y2[k] * dr * dr / 6.0);
  CREATE_TRY(device_array(c, &P.lut, lut));
  P.nti = c->lut.nscreened;
  P.ntj = c->lut.nscreener;
  P.lut_entries = P.nti * P.ntj * kLutStride;
  if (lut.size() * sizeof(double2) > 128 * 1024)  // + 24 KB of tile records in k_dborn_tiles
    return bail(AGBNP_HIP_ERR_CAPACITY, "agbnp_hip_create: too many distinct radius pairs for the LDS-resident I4 tables", c);

  int rc = upload_parameters(c);
  if (rc != AGBNP_HIP_OK) return bail(rc, c->err, c);
  rc = allocate_work(c);
  if (rc != AGBNP_HIP_OK) return bail(rc, c->err, c);
  derive_args(c);
  *out = c;
  return AGBNP_HIP_OK;
}

int agbnp_hip_update_parameters(agbnp_hip_context* c, int n, const double* radius, const double* gamma, const double* vdw_alpha,
                                const double* charge, const int* ishydrogen) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (!radius || !gamma || !vdw_alpha || !charge || !ishydrogen) return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "null pointer");
  if (n != c->n) return c->fail(AGBNP_HIP_ERR_PARAMETERS, "updateParametersInContext: The number of AGBNP particles has changed");
  for (int i = 0; i < n; i++) {
    if ((c->r_vdw[i] - radius[i]) * (c->r_vdw[i] - radius[i]) > 1.e-6)
      return c->fail(AGBNP_HIP_ERR_PARAMETERS, "updateParametersInContext: AGBNP plugin does not support changing atomic radii.");
    if (ishydrogen[i] && c->ish[i] == 0)
      return c->fail(AGBNP_HIP_ERR_PARAMETERS, "updateParametersInContext: AGBNP plugin does not support changing heavy/hydrogen atoms.");
  }
  for (int i = 0; i < n; i++) {
    c->gamma[i] = ishydrogen[i] ? 0.0 : gamma[i];
    c->alpha[i] = vdw_alpha[i];
    c->charge[i] = charge[i];
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // the parameter arrays are rewritten in place (their addresses stay valid for captured graphs), so nothing of this
  // context may be in flight: the context's own stream is drained here, and a caller who enqueues on streams of its own
  // (agbnp_hip_execute_device / _openmm with a stream argument) calls agbnp_hip_finish on them first -- as it must anyway
  // to learn about withheld evaluations.  (Not hipDeviceSynchronize: that would stall every other context of the device.)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (void* st : c->user_streams) HIP_TRY(c, hipStreamSynchronize((hipStream_t)st));
  return upload_changed_parameters(c);  // (the arrays are rewritten in place: no kernel argument changes)
}

int agbnp_hip_set_mode(agbnp_hip_context* c, int mode) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  if (mode & ~(AGBNP_HIP_MODE_FAST | AGBNP_HIP_MODE_DETERMINISTIC | AGBNP_HIP_MODE_SINGLE))
    return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_mode: unknown mode bits");
  if ((mode & AGBNP_HIP_MODE_SINGLE) && !(mode & AGBNP_HIP_MODE_FAST))
    return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_mode: single precision is an option of the fast mode (the Reference semantics are FP64)");
  if ((mode & AGBNP_HIP_MODE_FAST) && c->method == 2)
    return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_mode: the fast mode does not take CutoffPeriodic (no periodic box crosses this boundary)");
  if ((mode & AGBNP_HIP_MODE_FAST) && c->method != 0 && !(c->cutoff > 0.0))
    return c->fail(AGBNP_HIP_ERR_INVALID_ARGUMENT, "agbnp_hip_set_mode: the fast mode needs a positive cutoff distance");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (this context's own work; other contexts of the device are not stalled)
  if (mode != c->mode) c->generation++;  // other kernel arguments: a captured graph is stale
  c->mode = mode;
  derive_args(c);
  if (c->rows_capable) return mark_rows_stale(c);  // the neighbour lists were built for the reach of the mode that is being left
  return AGBNP_HIP_OK;
}

int agbnp_hip_set_diagnostics(agbnp_hip_context* c, int enabled) {
  if (!c) return AGBNP_HIP_ERR_INVALID_ARGUMENT;
  c->diagnostics = enabled != 0;
  derive_args(c);
  return AGBNP_HIP_OK;
}

void agbnp_hip_destroy(agbnp_hip_context* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
  }
  for (hipEvent_t e : c->timeline.events) (void)hipEventDestroy(e);
  if (c->group_event) (void)hipEventDestroy(c->group_event);
  if (c->h_status) (void)hipHostFree(c->h_status);
  if (c->h_report) (void)hipHostFree(c->h_report);
  if (c->h_xfer) (void)hipHostFree(c->h_xfer);
  delete c;
}

}  // extern "C"
