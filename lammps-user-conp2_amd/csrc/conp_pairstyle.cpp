// The pair style lj/cut/coul/long on the device (conp_pair.hip) and its half neighbour list, uploaded or built on
// the device (conp_neigh.hip, section 17).  set_params copies the per-type-pair tables (one 8-double record per pair), set_list
// uploads the list and sizes every buffer a compute call needs: the device entry then allocates nothing.
#include "conp_pairstyle.hpp"

#include <cmath>

namespace conp {
using namespace dev;

void PairStyle::set_params(const conp_pair_params *p) {
  if (p->ntypes != env.ntypes) throw ConpError(CONP_ERR_ARG, "conp_pair_set_params: ntypes differs from the handle's");
  if (!p->cutsq) throw ConpError(CONP_ERR_ARG, "conp_pair_set_params: cutsq is NULL");
  if (p->cut_ljsq && (!p->lj1 || !p->lj2 || !p->lj3 || !p->lj4 || !p->offset))
    throw ConpError(CONP_ERR_ARG, "conp_pair_set_params: cut_ljsq without lj1..lj4 and offset");
  const int nt1 = env.ntypes + 1;
  std::vector<double> tab((size_t)nt1 * nt1 * PAIR_TAB_W, 0.0);
  for (int k = 0; k < nt1 * nt1; ++k) {
    double *t = &tab[(size_t)k * PAIR_TAB_W];
    t[0] = p->cutsq[k];
    if (p->cut_ljsq) { t[1] = p->cut_ljsq[k]; t[2] = p->lj1[k]; t[3] = p->lj2[k]; t[4] = p->lj3[k]; t[5] = p->lj4[k]; t[6] = p->offset[k]; }
    // (no LJ part: cut_ljsq stays 0, and rsq < 0 never holds)
  }
  ctx.sync();                                       // no kernel may be reading the old table
  d_tab.upload(tab, ctx.stream);
  ctx.sync();                                       // `tab` leaves scope
  ntab = nt1 * nt1;
  cut_coul = p->cut_coul;
  cutsq_max = 0.0;
  for (int k = 0; k < nt1 * nt1; ++k) cutsq_max = std::max(cutsq_max, p->cutsq[k]);
  for (int k = 0; k < 4; ++k) { special_lj[k] = p->special_lj[k]; special_coul[k] = p->special_coul[k]; }
  have_params = true;
}

void PairStyle::set_list(const conp_neighlist *l, int nall_) {
  have_list = false;                       // a list that is refused leaves the handle without one
  list_built = false;
  ++list_gen;
  if (nall_ < 0 || l->inum < 0 || l->inum > nall_ || l->nneigh < 0) throw ConpError(CONP_ERR_ARG, "conp_pair_set_list: bad sizes");
  if (l->inum > 0 && (!l->ilist || !l->numneigh || !l->first)) throw ConpError(CONP_ERR_ARG, "conp_pair_set_list: null list array");
  if (l->nneigh > 0 && !l->neigh) throw ConpError(CONP_ERR_ARG, "conp_pair_set_list: null neighbour array");
  for (int ii = 0; ii < l->inum; ++ii) {        // every index a kernel will use is checked here, once per list
    const int i = l->ilist[ii];
    if (i < 0 || i >= nall_) throw ConpError(CONP_ERR_ARG, "conp_pair_set_list: list owner outside [0, nall)");
    const int64_t a = l->first[i], n = l->numneigh[i];
    if (a < 0 || n < 0 || a + n > l->nneigh) throw ConpError(CONP_ERR_ARG, "conp_pair_set_list: a row leaves the neighbour array");
    for (int64_t k = a; k < a + n; ++k)
      if ((l->neigh[k] & 0x3FFFFFFF) >= nall_) throw ConpError(CONP_ERR_ARG, "conp_pair_set_list: neighbour index outside [0, nall)");
  }
  ctx.sync();
  d_ilist.upload(l->ilist, (size_t)l->inum, ctx.stream);
  d_numneigh.upload(l->numneigh, (size_t)(l->inum > 0 ? nall_ : 0), ctx.stream);
  d_first.upload(l->first, (size_t)(l->inum > 0 ? nall_ : 0), ctx.stream);
  d_neigh.upload(l->neigh, (size_t)l->nneigh, ctx.stream);
  d_part.reserve((size_t)std::max(l->inum, 1) * 8);
  d_xq.reserve((size_t)std::max(nall_, 1));
  d_ev.reserve(8);
  ctx.sync();                                       // the caller's arrays need not stay
  nall = nall_; inum = l->inum; nneigh = l->nneigh;
  have_list = true;
}

// The cell grid of a build: cells at least cutneigh (1 + 2^-20) wide, so that the 27 cells around an atom's hold every atom
// within cutneigh of it whatever the rounding of the index arithmetic; at most 4 nall + 64 cells (a dilute or a very long box
// gets wider cells: the numbers of cells are halved, the largest first, until they fit).
static NeighGrid neigh_grid(const double ext[6], double cutneigh, int nall_) {
  NeighGrid g;
  const double w = cutneigh * (1.0 + 1.0 / 1048576.0);
  for (int c = 0; c < 3; ++c) {
    const double len = ext[3 + c] - ext[c];
    g.lo[c] = ext[c];
    g.n[c] = w > 0.0 && len > w ? (int)std::min(len / w, 1024.0) : 1;
  }
  const int64_t cap = 4 * (int64_t)nall_ + 64;
  while ((int64_t)g.n[0] * g.n[1] * g.n[2] > cap) {
    int c = 0;
    if (g.n[1] > g.n[c]) c = 1;
    if (g.n[2] > g.n[c]) c = 2;
    g.n[c] = (g.n[c] + 1) / 2;
  }
  for (int c = 0; c < 3; ++c) {
    const double len = ext[3 + c] - ext[c];
    g.inv[c] = g.n[c] > 1 ? g.n[c] / len : 0.0;      // one cell: every atom gets index 0
  }
  return g;
}

// neigh_modify exclude type / group / molecule/intra / molecule/inter: the rules are checked and kept on the
// host (they travel in the kernel arguments), the symmetric type table goes to the device
void PairStyle::set_exclusions(const conp_pair_exclusions *e) {
  have_excl = false;                       // a refused call leaves the handle without rules
  const std::string who = "conp_pair_set_exclusions: ";
  if (!have_params) throw ConpError(CONP_ERR_STATE, who + "before conp_pair_set_params");
  NeighExclArgs x{};
  x.nt1 = env.ntypes + 1;
  std::vector<unsigned char> tab((size_t)x.nt1 * x.nt1, 0);
  if (e) {
    if (e->ntype_pairs < 0 || e->ngroup_pairs < 0 || e->nmol < 0) throw ConpError(CONP_ERR_ARG, who + "negative count");
    if (e->ngroup_pairs > NEIGH_EXCL_MAX || e->nmol > NEIGH_EXCL_MAX)
      throw ConpError(CONP_ERR_ARG, who + "more than 16 group or molecule rules");
    if ((e->ntype_pairs > 0 && (!e->type_i || !e->type_j)) || (e->ngroup_pairs > 0 && (!e->group_bit1 || !e->group_bit2)) ||
        (e->nmol > 0 && (!e->mol_bit || !e->mol_intra)))
      throw ConpError(CONP_ERR_ARG, who + "a positive count with a null array");
    if (e->ntype_pairs > 0 && e->ntypes != env.ntypes) throw ConpError(CONP_ERR_ARG, who + "ntypes differs from conp_pair_set_params'");
    for (int k = 0; k < e->ntype_pairs; ++k) {
      const int ti = e->type_i[k], tj = e->type_j[k];
      if (ti < 1 || ti > env.ntypes || tj < 1 || tj > env.ntypes) throw ConpError(CONP_ERR_ARG, who + "a type outside [1, ntypes]");
      tab[(size_t)ti * x.nt1 + tj] = tab[(size_t)tj * x.nt1 + ti] = 1;
    }
    for (int k = 0; k < e->ngroup_pairs; ++k) {
      if (e->group_bit1[k] == 0 || e->group_bit2[k] == 0) throw ConpError(CONP_ERR_ARG, who + "a group bit mask of 0");
      x.gbit1[k] = e->group_bit1[k]; x.gbit2[k] = e->group_bit2[k];
    }
    for (int k = 0; k < e->nmol; ++k) {
      if (e->mol_bit[k] == 0) throw ConpError(CONP_ERR_ARG, who + "a molecule bit mask of 0");
      x.mbit[k] = e->mol_bit[k];
      if (e->mol_intra[k]) x.mintra |= 1u << k;
    }
    x.ntype = e->ntype_pairs > 0; x.ngroup = e->ngroup_pairs; x.nmol = e->nmol;
  }
  ctx.sync();                                       // no kernel may be reading the old table
  d_ex_type.upload(tab, ctx.stream);
  ctx.sync();                                       // `tab` leaves scope
  excl = x;
  have_excl = true;
}

void PairStyle::build_list(const double *dx, const conp_pair_build_args *a, const conp_pair_exclude_atoms *at, bool exclude) {
  have_list = false;                       // a build that is refused leaves the handle without a list
  list_built = false;
  ++list_gen;
  const std::string who = exclude ? "conp_pair_build_list_exclude_device: " : "conp_pair_build_list_device: ";
  const char *entry = exclude ? "conp_pair_build_list_exclude_device" : "conp_pair_build_list_device";
  if (!have_params) throw ConpError(CONP_ERR_STATE, std::string(entry) + " before conp_pair_set_params");
  if (exclude && !have_excl) throw ConpError(CONP_ERR_STATE, std::string(entry) + " before conp_pair_set_exclusions");
  if (!dx || !a || (exclude && !at)) throw ConpError(CONP_ERR_ARG, "null argument");
  if (a->nlocal < 0 || a->nall < 0 || a->nlocal > a->nall || a->nall > 0x3FFFFFFF)
    throw ConpError(CONP_ERR_ARG, who + "bad sizes");
  if (!(a->cutneigh * a->cutneigh >= cutsq_max) || !(a->cutneigh > 0.0) || !std::isfinite(a->cutneigh))
    throw ConpError(CONP_ERR_ARG, who + "cutneigh^2 is below the largest cutsq of conp_pair_set_params");
  const int nsp = (a->d_tag != nullptr) + (a->d_nspecial != nullptr) + (a->d_special != nullptr);
  if (nsp != 0 && nsp != 3) throw ConpError(CONP_ERR_ARG, who + "d_tag, d_nspecial, d_special: all three or none");
  if (nsp == 3 && a->maxspecial < 0) throw ConpError(CONP_ERR_ARG, who + "negative maxspecial");
  for (int c = 0; c < 3; ++c)
    if (!(a->prd_half[c] >= 0.0)) throw ConpError(CONP_ERR_ARG, who + "prd_half is negative or not a number");
  NeighExclArgs ex = excl;                          // rules in force: the rows are built with the exclusion test
  const bool filter = exclude && (ex.ntype || ex.ngroup || ex.nmol);
  if (filter) {
    if (ex.ntype && !at->d_type) throw ConpError(CONP_ERR_ARG, who + "type rules need d_type");
    if ((ex.ngroup || ex.nmol) && !at->d_mask) throw ConpError(CONP_ERR_ARG, who + "group and molecule rules need d_mask");
    if (ex.nmol && !at->d_molecule) throw ConpError(CONP_ERR_ARG, who + "molecule rules need d_molecule");
    ex.type = ex.ntype ? at->d_type : nullptr;
    ex.mask = ex.ngroup || ex.nmol ? at->d_mask : nullptr;
    ex.molecule = ex.nmol ? at->d_molecule : nullptr;
    ex.ex_type = d_ex_type.p;
  }
  const int nl = a->nlocal, na = a->nall;
  ctx.sync();                                       // no kernel may be reading the old list
  d_ilist.reserve((size_t)std::max(nl, 1));
  d_numneigh.reserve((size_t)std::max(na, 1));
  d_first.reserve((size_t)std::max(na, 1));
  d_part.reserve((size_t)std::max(nl, 1) * 8);
  d_xq.reserve((size_t)std::max(na, 1));
  d_ev.reserve(8);
  d_nb_ext.reserve(8); d_nb_total.reserve(1);
  d_nb_xbuild.reserve((size_t)std::max(nl, 1) * 3);
  d_nb_cell.reserve((size_t)std::max(na, 1)); d_nb_slot.reserve((size_t)std::max(na, 1));
  d_nb_unsorted.reserve((size_t)std::max(na, 1)); d_nb_sorted.reserve((size_t)std::max(na, 1));
  long long total = 0;
  if (na > 0) {
    launch_neigh_extent(ctx.stream, na, dx, d_nb_ext.p);
    double ext[7];
    HIP_TRY(hipMemcpyAsync(ext, d_nb_ext.p, sizeof ext, hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    bool finite = ext[6] == 0.0;
    for (int c = 0; c < 3; ++c) finite = finite && std::isfinite(ext[3 + c] - ext[c]);
    if (!finite) throw ConpError(CONP_ERR_NUMERIC, who + "a coordinate is not finite");
    const NeighGrid g = neigh_grid(ext, a->cutneigh, na);
    const int ncell = g.n[0] * g.n[1] * g.n[2];
    d_nb_count.reserve((size_t)ncell); d_nb_start.reserve((size_t)ncell + 1);
    launch_neigh_bin(ctx.stream, na, dx, g, d_nb_cell.p, d_nb_slot.p, d_nb_count.p, d_nb_start.p, d_nb_total.p, d_nb_unsorted.p,
                     d_nb_sorted.p);
    NeighRowArgs r;
    r.nlocal = nl; r.newton = env.newton_pair != 0; r.x = dx; r.cutneighsq = a->cutneigh * a->cutneigh; r.g = g;
    r.cell = d_nb_cell.p; r.start = d_nb_start.p; r.sorted = d_nb_sorted.p;
    r.tag = a->d_tag; r.nspecial = a->d_nspecial; r.special = a->d_special; r.maxspecial = a->maxspecial;
    r.flagged[0] = 0;
    for (int k = 1; k < 4; ++k) r.flagged[k] = !(special_lj[k] == 1.0 && special_coul[k] == 1.0);
    for (int c = 0; c < 3; ++c) r.prd_half[c] = a->prd_half[c];
    r.numneigh = d_numneigh.p; r.first = d_first.p; r.neigh = nullptr;
    HIP_TRY(hipMemsetAsync(d_numneigh.p, 0, (size_t)na * sizeof(int), ctx.stream));      // rows of i >= nlocal: 0
    HIP_TRY(hipMemsetAsync(d_first.p, 0, (size_t)na * sizeof(int), ctx.stream));
    if (filter) launch_neigh_rows_exclude(ctx.stream, r, ex, false);
    else launch_neigh_rows(ctx.stream, r, false);
    launch_neigh_scan(ctx.stream, nl, d_numneigh.p, d_first.p, d_nb_total.p);
    HIP_TRY(hipMemcpyAsync(&total, d_nb_total.p, sizeof total, hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    if (total >= (1ll << 31)) throw ConpError(CONP_ERR_NUMERIC, who + "2^31 pairs or more (first is int)");
    d_neigh.reserve((size_t)std::max<long long>(total, 1));
    r.neigh = d_neigh.p;
    if (filter) launch_neigh_rows_exclude(ctx.stream, r, ex, true);
    else launch_neigh_rows(ctx.stream, r, true);
    launch_neigh_iota(ctx.stream, nl, d_ilist.p);
    if (nl > 0) HIP_TRY(hipMemcpyAsync(d_nb_xbuild.p, dx, (size_t)nl * 3 * sizeof(double), hipMemcpyDeviceToDevice, ctx.stream));
    HIP_TRY(hipGetLastError());
    ctx.sync();
  }
  nall = na; inum = nl; nneigh = total; build_nlocal = nl; build_cutneigh = a->cutneigh;
  have_list = true;
  list_built = true;
}

void PairStyle::list_moved(const double *dx, double trigger, int *dflag) {
  if (!dx || !dflag) throw ConpError(CONP_ERR_ARG, "null argument");
  if (!(trigger >= 0.0)) throw ConpError(CONP_ERR_ARG, "conp_pair_list_moved_device: trigger is negative or not a number");
  if (!have_list || !list_built)
    throw ConpError(CONP_ERR_STATE, "conp_pair_list_moved_device: the handle's list is not one of conp_pair_build_list_device");
  launch_neigh_moved(ctx.stream, build_nlocal, dx, d_nb_xbuild.p, trigger * trigger, dflag);
  HIP_TRY(hipGetLastError());
}

void PairStyle::get_list(int *inum_, int *nall_, int64_t *nneigh_, int *ilist, int *numneigh, int *first, int *neigh) {
  if (!have_list) throw ConpError(CONP_ERR_STATE, "conp_pair_get_list: the handle has no list");
  if (inum_) *inum_ = inum;
  if (nall_) *nall_ = nall;
  if (nneigh_) *nneigh_ = nneigh;
  const bool rows = inum > 0 && nall > 0;      // (an uploaded list without owners has no per-atom arrays)
  if (ilist && inum > 0) HIP_TRY(hipMemcpyAsync(ilist, d_ilist.p, (size_t)inum * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
  if (numneigh && nall > 0) {
    if (rows) HIP_TRY(hipMemcpyAsync(numneigh, d_numneigh.p, (size_t)nall * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    else std::memset(numneigh, 0, (size_t)nall * sizeof(int));
  }
  if (first && nall > 0) {
    if (rows) HIP_TRY(hipMemcpyAsync(first, d_first.p, (size_t)nall * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    else std::memset(first, 0, (size_t)nall * sizeof(int));
  }
  if (neigh && nneigh > 0) HIP_TRY(hipMemcpyAsync(neigh, d_neigh.p, (size_t)nneigh * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
}

// pack + force kernel (+ finish) on the stream; eatom / vatom are overwritten: zeroed first, then accumulated
void PairStyle::enqueue(const double *dx, const double *dq, const int *dtype, int nlocal_, double *df, double *dev, double *dea, double *dva,
                        const TransposedView *tv) {
  PairArgs a;
  a.inum = inum; a.ilist = d_ilist.p; a.numneigh = d_numneigh.p; a.first = d_first.p; a.neigh = d_neigh.p;
  a.nlocal = nlocal_; a.newton = env.newton_pair != 0;
  a.xq = d_xq.p; a.type = dtype; a.nt1 = env.ntypes + 1; a.ntab = ntab; a.tab = d_tab.p;
  a.cut_coulsq = cut_coul * cut_coul; a.g_ewald = env.g_ewald; a.qqrd2e = env.qqrd2e;
  for (int k = 0; k < 4; ++k) { a.special_lj[k] = special_lj[k]; a.special_coul[k] = special_coul[k]; }
  a.f = df; a.eatom = dea; a.vatom = dva; a.part = d_part.p;
  if (dea && nall > 0) HIP_TRY(hipMemsetAsync(dea, 0, (size_t)nall * sizeof(double), ctx.stream));
  if (dva && nall > 0) HIP_TRY(hipMemsetAsync(dva, 0, (size_t)nall * 6 * sizeof(double), ctx.stream));
  ctx.prof.begin(tv ? "pair_force_ordered" : "pair_force", ctx.stream);
  launch_pair_pack(ctx.stream, nall, dx, dq, d_xq.p);
  if (tv) launch_pair_force_ordered(ctx.stream, a, *tv, dev);
  else launch_pair_force(ctx.stream, a, dev);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void PairStyle::compute_host(const conp_atoms *at, const double *dx, const double *dq, double *f, double *eng, double *vir, double *eatom,
                             double *vatom) {
  const int n = at->nlocal + at->nghost;
  if (!dx) {                                    // not the atoms the fix holds: staged here
    ctx.sync();
    d_x.upload(at->x, (size_t)n * 3, ctx.stream); d_q.upload(at->q, (size_t)n, ctx.stream);
    dx = d_x.p; dq = d_q.p;
  }
  d_type.upload(at->type, (size_t)n, ctx.stream);
  const size_t nf = f ? (size_t)n * 3 : 0, ne = eatom ? (size_t)n : 0, nv = vatom ? (size_t)n * 6 : 0;
  const bool ev = eng || vir;
  if (f) { d_f.reserve(std::max<size_t>(nf, 1)); if (nf) HIP_TRY(hipMemsetAsync(d_f.p, 0, nf * sizeof(double), ctx.stream)); }
  if (eatom) d_ea.reserve(std::max<size_t>(ne, 1));
  if (vatom) d_va.reserve(std::max<size_t>(nv, 1));
  enqueue(dx, dq, d_type.p, at->nlocal, f ? d_f.p : nullptr, ev ? d_ev.p : nullptr, eatom ? d_ea.p : nullptr,
          vatom ? d_va.p : nullptr);
  out_h.resize(nf + ne + nv + 8);
  double *h = out_h.data();
  if (nf) HIP_TRY(hipMemcpyAsync(h, d_f.p, nf * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  if (ne) HIP_TRY(hipMemcpyAsync(h + nf, d_ea.p, ne * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  if (nv) HIP_TRY(hipMemcpyAsync(h + nf + ne, d_va.p, nv * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  if (ev) HIP_TRY(hipMemcpyAsync(h + nf + ne + nv, d_ev.p, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
  for (size_t k = 0; k < nf; ++k) f[k] += h[k];
  if (ne) std::memcpy(eatom, h + nf, ne * sizeof(double));
  if (nv) std::memcpy(vatom, h + nf + ne, nv * sizeof(double));
  const double *e8 = h + nf + ne + nv;
  if (eng) { eng[0] = e8[0]; eng[1] = e8[1]; }
  if (vir) for (int k = 0; k < 6; ++k) vir[k] = e8[2 + k];
}

}  // namespace conp
