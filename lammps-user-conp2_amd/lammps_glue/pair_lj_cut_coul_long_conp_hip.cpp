#include "pair_lj_cut_coul_long_conp_hip.h"

#ifndef CONP_GLUE_MOCK
#include "fix_conp.h"
#include "modify.h"
#include "neigh_list.h"
#include "neighbor.h"
#endif

using namespace LAMMPS_NS;
using conp_glue::fail_if;

PairLJCutCoulLongConpHip::PairLJCutCoulLongConpHip(LAMMPS *lmp) : PairLJCutCoulLong(lmp) {
  no_virial_fdotr = 1;      /* the global virial is Pair::ev_tally's sum over pairs, formed on the device */
}

void PairLJCutCoulLongConpHip::find_handle() {
  handle_ = nullptr; fixhip = nullptr; fixconp = nullptr;
  for (int f = 0; f < modify->nfix && handle_ == nullptr; ++f) {
    if (auto *fh = dynamic_cast<FixConpHip *>(modify->fix[f])) {
      if (fh->handle() != nullptr) { fixhip = fh; handle_ = fh->handle(); }
    } else if (auto *fc = dynamic_cast<FixConp *>(modify->fix[f])) {
      auto *km = dynamic_cast<KSpaceModuleHip *>(fc->kspmod);
      if (km != nullptr && km->handle() != nullptr) { fixconp = fc; handle_ = km->handle(); }
    }
  }
}

/* the base class's tables, flattened [(ntypes + 1)^2] each (row and column 0 are not used by LAMMPS: zeros), then cut_coul and the
 * special factors: everything conp_pair_set_params is given */
void PairLJCutCoulLongConpHip::flatten_tables() {
  const int nt1 = atom->ntypes + 1;
  const size_t n = (size_t)nt1 * nt1;
  double **src[7] = {cutsq, cut_ljsq, lj1, lj2, lj3, lj4, offset};
  tables.assign(7 * n + 9, 0.0);
  for (int k = 0; k < 7; ++k)
    for (int i = 1; i < nt1; ++i)
      for (int j = 1; j < nt1; ++j) tables[k * n + (size_t)i * nt1 + j] = src[k][i][j];
  tables[7 * n] = cut_coul;
  for (int k = 0; k < 4; ++k) { tables[7 * n + 1 + k] = force->special_lj[k]; tables[7 * n + 5 + k] = force->special_coul[k]; }
}

void PairLJCutCoulLongConpHip::send_params() {
  const int nt1 = atom->ntypes + 1;
  const size_t n = (size_t)nt1 * nt1;
  conp_pair_params p;
  p.ntypes = atom->ntypes;
  p.cutsq = &tables[0]; p.cut_coul = tables[7 * n];
  p.cut_ljsq = &tables[n]; p.lj1 = &tables[2 * n]; p.lj2 = &tables[3 * n]; p.lj3 = &tables[4 * n]; p.lj4 = &tables[5 * n];
  p.offset = &tables[6 * n];
  for (int k = 0; k < 4; ++k) { p.special_lj[k] = tables[7 * n + 1 + k]; p.special_coul[k] = tables[7 * n + 5 + k]; }
  fail_if(error, conp_pair_set_params(handle_, &p));
  tables_sent = tables;
  params_set = true;
}

/* the style's half list with firstneigh flattened (special bits kept: the library strips them) */
void PairLJCutCoulLongConpHip::send_list() {
  const int nall = atom->nlocal + atom->nghost;
  first_flat.assign((size_t)nall, 0);
  neigh_flat.clear();
  for (int ii = 0; ii < list->inum; ++ii) {
    const int i = list->ilist[ii];
    first_flat[i] = (int)neigh_flat.size();
    neigh_flat.insert(neigh_flat.end(), list->firstneigh[i], list->firstneigh[i] + list->numneigh[i]);
  }
  conp_neighlist l;
  l.inum = list->inum; l.ilist = list->ilist; l.numneigh = list->numneigh; l.first = first_flat.data();
  l.nneigh = (int64_t)neigh_flat.size();
  if (neigh_flat.empty()) neigh_flat.push_back(0);
  l.neigh = neigh_flat.data();
  fail_if(error, conp_pair_set_list(handle_, &l, nall));
  list_set = true;
  ++n_list_uploads;
}

void PairLJCutCoulLongConpHip::compute(int eflag, int vflag) {
  ev_init(eflag, vflag);
  if (ncoultablebits != 0)
    error->all(FLERR, "pair_style lj/cut/coul/long/conp/hip does not support Coulomb tables: use pair_modify table 0");
  if (handle_ == nullptr) { find_handle(); params_set = list_set = false; }
  if (handle_ == nullptr)
    error->all(FLERR, "pair_style lj/cut/coul/long/conp/hip needs a conp/hip fix (or fix conp with the hip provider)");
  if (list == nullptr) error->all(FLERR, "pair_style lj/cut/coul/long/conp/hip has no neighbor list");
  const bool rebuilt = !list_set || neighbor->ago == 0;
  if (!params_set || rebuilt) {
    flatten_tables();
    if (!params_set || tables != tables_sent) send_params();
  }
  if (rebuilt) send_list();
  conp_atoms at = av.flat(atom, [this](int i) { return fixconp ? fixconp->electrode_check(i) : fixhip->electrode_check(i); });
  const int nall = atom->nlocal + atom->nghost;
  /* atom->f, vatom: one contiguous block behind the row pointers (Memory::create); f is accumulated in place, the others overwritten */
  double eng[2] = {0.0, 0.0}, vir[6] = {0, 0, 0, 0, 0, 0};
  fail_if(error, conp_pair_compute(handle_, &at, nall ? &atom->f[0][0] : nullptr, eflag_global ? eng : nullptr,
                                   vflag_global ? vir : nullptr, eflag_atom ? eatom : nullptr,
                                   vflag_atom && nall ? &vatom[0][0] : nullptr));
  if (eflag_global) { eng_vdwl += eng[0]; eng_coul += eng[1]; }
  if (vflag_global) for (int k = 0; k < 6; ++k) virial[k] += vir[k];
}
