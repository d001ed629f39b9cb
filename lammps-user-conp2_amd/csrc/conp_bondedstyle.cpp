// Harmonic bonds and angles on the device (conp_bonded.hip).  set_params copies the per-type coefficients,
// set_lists checks and uploads the topology lists, builds the per-atom slot table the gather kernel walks, and sizes every buffer
// a compute call needs: the device entry then allocates nothing.
#include "conp_bondedstyle.hpp"

#include <cmath>

namespace conp {
using namespace dev;

void BondedStyle::set_params(const conp_bonded_params *p) {
  if (p->nbondtypes < 0 || p->nangletypes < 0) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_params: negative type count");
  if (p->nbondtypes > 0 && (!p->bond_k || !p->bond_r0)) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_params: null bond table");
  if (p->nangletypes > 0 && (!p->angle_k || !p->angle_theta0)) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_params: null angle table");
  std::vector<double> bc(2 * ((size_t)p->nbondtypes + 1), 0.0), ac(2 * ((size_t)p->nangletypes + 1), 0.0);
  for (int t = 1; t <= p->nbondtypes; ++t) { bc[2 * (size_t)t] = p->bond_k[t]; bc[2 * (size_t)t + 1] = p->bond_r0[t]; }
  for (int t = 1; t <= p->nangletypes; ++t) { ac[2 * (size_t)t] = p->angle_k[t]; ac[2 * (size_t)t + 1] = p->angle_theta0[t]; }
  ctx.sync();                                       // no kernel may be reading the old tables
  d_bcoef.upload(bc, ctx.stream);
  d_acoef.upload(ac, ctx.stream);
  ctx.sync();                                       // `bc`, `ac` leave scope
  nbondtypes = p->nbondtypes; nangletypes = p->nangletypes; newton_bond = p->newton_bond != 0;
  have_params = true;
  have_lists = false;                               // types of the lists were checked against the old tables
}

void BondedStyle::set_lists(const conp_bonded_lists *l) {
  have_lists = false;                      // lists that are refused leave the handle without any
  if (!have_params) throw ConpError(CONP_ERR_STATE, "conp_bonded_set_lists before conp_bonded_set_params");
  if (l->nlocal < 0 || l->nall < 0 || l->nlocal > l->nall || l->nbond < 0 || l->nangle < 0)
    throw ConpError(CONP_ERR_ARG, "conp_bonded_set_lists: bad sizes");
  if ((int64_t)l->nbond + l->nangle > 0x1FFFFFFF) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_lists: 2^29 terms or more");
  if ((l->nbond > 0 && !l->bond) || (l->nangle > 0 && !l->angle)) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_lists: null list array");
  for (int c = 0; c < 3; ++c)
    if (!(l->prd[c] >= 0.0) || !std::isfinite(l->prd[c])) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_lists: prd is negative or not finite");
  const int na = l->nall, nb = l->nbond, nan = l->nangle;
  // every index a kernel will use is checked here, once per list; the same pass counts an atom's slots
  std::vector<int> ptr((size_t)na + 1, 0);
  for (int b = 0; b < nb; ++b) {
    const int *e = l->bond + 3 * (size_t)b;
    for (int r = 0; r < 2; ++r) {
      if (e[r] < 0 || e[r] >= na) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_lists: bond member outside [0, nall)");
      ++ptr[(size_t)e[r] + 1];
    }
    if (e[2] < 1 || e[2] > nbondtypes) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_lists: bond type outside [1, nbondtypes]");
  }
  for (int a = 0; a < nan; ++a) {
    const int *e = l->angle + 4 * (size_t)a;
    for (int r = 0; r < 3; ++r) {
      if (e[r] < 0 || e[r] >= na) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_lists: angle member outside [0, nall)");
      ++ptr[(size_t)e[r] + 1];
    }
    if (e[3] < 1 || e[3] > nangletypes) throw ConpError(CONP_ERR_ARG, "conp_bonded_set_lists: angle type outside [1, nangletypes]");
  }
  for (int i = 0; i < na; ++i) ptr[(size_t)i + 1] += ptr[i];
  // the slots of an atom: term * 4 + role, bonds first in list order, then angles in list order
  const size_t nslot = 2 * (size_t)nb + 3 * (size_t)nan;
  std::vector<int> slot(nslot), at_(ptr.begin(), ptr.end() - 1);
  for (int b = 0; b < nb; ++b)
    for (int r = 0; r < 2; ++r) slot[(size_t)at_[l->bond[3 * (size_t)b + r]]++] = b * 4 + r;
  for (int a = 0; a < nan; ++a)
    for (int r = 0; r < 3; ++r) slot[(size_t)at_[l->angle[4 * (size_t)a + r]]++] = (nb + a) * 4 + r;
  const size_t nterm = (size_t)nb + nan;
  ctx.sync();                                       // no kernel may be reading the old lists
  d_bond.upload(l->bond, 3 * (size_t)nb, ctx.stream);
  d_angle.upload(l->angle, 4 * (size_t)nan, ctx.stream);
  d_slot_ptr.upload(ptr, ctx.stream);
  d_slot.upload(slot, ctx.stream);
  d_term.reserve(std::max<size_t>(nterm, 1) * BONDED_TERM_W);
  d_part.reserve(std::max<size_t>((nterm + BONDED_BLOCK - 1) / BONDED_BLOCK, 1) * 8);
  d_ev.reserve(8);
  ctx.sync();                                       // the caller's arrays, `ptr` and `slot` need not stay
  nlocal = l->nlocal; nall = na; nbond = nb; nangle = nan;
  for (int c = 0; c < 3; ++c) prd[c] = l->prd[c];
  have_lists = true;
}

// term kernel (+ finish) and gather kernel on the stream; every output is overwritten or, for df, added to once per atom
void BondedStyle::enqueue(const double *dx, double *df, double *dev, double *dea, double *dva) {
  BondedArgs a;
  a.nbond = nbond; a.nangle = nangle; a.nlocal = nlocal; a.nall = nall; a.newton = newton_bond;
  a.bond = d_bond.p; a.angle = d_angle.p; a.bcoef = d_bcoef.p; a.acoef = d_acoef.p;
  for (int c = 0; c < 3; ++c) a.prd[c] = prd[c];
  a.x = dx; a.term = d_term.p; a.part = d_part.p; a.slot_ptr = d_slot_ptr.p; a.slot = d_slot.p;
  a.f = df; a.eatom = dea; a.vatom = dva;
  ctx.prof.begin("bonded", ctx.stream);
  launch_bonded(ctx.stream, a, dev);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void BondedStyle::compute_host(const conp_atoms *at, double *f, double *eng, double *vir, double *eatom, double *vatom) {
  const size_t n = (size_t)nall;
  ctx.sync();
  d_x.upload(at->x, n * 3, ctx.stream);
  const size_t nf = f ? n * 3 : 0, ne = eatom ? n : 0, nv = vatom ? n * 6 : 0;
  const bool ev = eng || vir;
  // (the caller's f goes up and comes back: the kernel's one add per atom is then the device entry's, bit for bit, and rows of
  //  atoms in no term return as they came)
  if (f) d_f.upload(f, nf, ctx.stream);
  if (eatom) d_ea.reserve(std::max<size_t>(ne, 1));
  if (vatom) d_va.reserve(std::max<size_t>(nv, 1));
  enqueue(d_x.p, f ? d_f.p : nullptr, ev ? d_ev.p : nullptr, eatom ? d_ea.p : nullptr, vatom ? d_va.p : nullptr);
  out_h.resize(nf + ne + nv + 8);
  double *h = out_h.data();
  if (nf) HIP_TRY(hipMemcpyAsync(h, d_f.p, nf * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  if (ne) HIP_TRY(hipMemcpyAsync(h + nf, d_ea.p, ne * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  if (nv) HIP_TRY(hipMemcpyAsync(h + nf + ne, d_va.p, nv * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  if (ev) HIP_TRY(hipMemcpyAsync(h + nf + ne + nv, d_ev.p, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
  if (nf) std::memcpy(f, h, nf * sizeof(double));
  if (ne) std::memcpy(eatom, h + nf, ne * sizeof(double));
  if (nv) std::memcpy(vatom, h + nf + ne, nv * sizeof(double));
  const double *e8 = h + nf + ne + nv;
  if (eng) { eng[0] = e8[0]; eng[1] = e8[1]; }
  if (vir) for (int k = 0; k < 6; ++k) vir[k] = e8[2 + k];
}

}  // namespace conp
