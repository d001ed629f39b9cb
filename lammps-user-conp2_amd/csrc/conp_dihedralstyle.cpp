// Dihedrals (opls, harmonic) and impropers (harmonic, cvff) on the device (conp_dihedral.hip).  set_params
// checks and copies the per-type coefficient rows, set_lists checks and uploads the topology lists, builds the per-atom slot table the
// gather kernel walks, and sizes every buffer a compute call needs: the device entry then allocates nothing.
#include "conp_dihedralstyle.hpp"

#include <cmath>

namespace conp {
using namespace dev;

namespace {

// the rows [ntypes + 1][4] of one list's style, row 0 zeroed; cosine: the rows are K d n 0 with n in 0..nmax
std::vector<double> checked_rows(const char *what, int ntypes, const double *coef, bool cosine, int nmax) {
  std::vector<double> rows(4 * ((size_t)ntypes + 1), 0.0);
  for (int t = 1; t <= ntypes; ++t) {
    const double *r = coef + 4 * (size_t)t;
    for (int k = 0; k < 4; ++k) {
      if (!std::isfinite(r[k])) throw ConpError(CONP_ERR_ARG, std::string("conp_dihedral_set_params: ") + what + " coefficient is not finite");
      rows[4 * (size_t)t + k] = r[k];
    }
    if (!cosine) continue;
    if (r[1] != 1.0 && r[1] != -1.0) throw ConpError(CONP_ERR_ARG, std::string("conp_dihedral_set_params: ") + what + " d is neither +1 nor -1");
    if (r[2] != std::floor(r[2]) || r[2] < 0.0 || r[2] > (double)nmax)
      throw ConpError(CONP_ERR_ARG, std::string("conp_dihedral_set_params: ") + what + " n is not an integer in 0.." + std::to_string(nmax));
  }
  return rows;
}

}  // namespace

void DihedralStyle::set_params(const conp_dihedral_params *p) {
  if (p->dihedral_style < DIHEDRAL_NONE || p->dihedral_style > DIHEDRAL_HARMONIC || p->improper_style < IMPROPER_NONE || p->improper_style > IMPROPER_CVFF)
    throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_params: unknown style");
  if (p->ndihedraltypes < 0 || p->nimpropertypes < 0) throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_params: negative type count");
  if ((p->dihedral_style == DIHEDRAL_NONE && p->ndihedraltypes > 0) || (p->improper_style == IMPROPER_NONE && p->nimpropertypes > 0))
    throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_params: types for a style that is 0");
  if ((p->ndihedraltypes > 0 && !p->dihedral_coef) || (p->nimpropertypes > 0 && !p->improper_coef))
    throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_params: null coefficient table");
  const std::vector<double> dc = checked_rows("dihedral", p->ndihedraltypes, p->dihedral_coef, p->dihedral_style == DIHEDRAL_HARMONIC, CONP_DIHEDRAL_MAX_N);
  const std::vector<double> ic = checked_rows("improper", p->nimpropertypes, p->improper_coef, p->improper_style == IMPROPER_CVFF, 6);
  ctx.sync();                                       // no kernel may be reading the old tables
  d_dcoef.upload(dc, ctx.stream);
  d_icoef.upload(ic, ctx.stream);
  ctx.sync();                                       // `dc`, `ic` leave scope
  dstyle = p->dihedral_style; istyle = p->improper_style;
  ndihedraltypes = p->ndihedraltypes; nimpropertypes = p->nimpropertypes; newton_bond = p->newton_bond != 0;
  have_params = true;
  have_lists = false;                               // types of the lists were checked against the old tables
}

void DihedralStyle::set_lists(const conp_dihedral_lists *l) {
  have_lists = false;                      // lists that are refused leave the handle without any
  if (!have_params) throw ConpError(CONP_ERR_STATE, "conp_dihedral_set_lists before conp_dihedral_set_params");
  if (l->nlocal < 0 || l->nall < 0 || l->nlocal > l->nall || l->ndihedral < 0 || l->nimproper < 0)
    throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_lists: bad sizes");
  if ((int64_t)l->ndihedral + l->nimproper > 0x1FFFFFFF) throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_lists: 2^29 terms or more");
  if ((l->ndihedral > 0 && !l->dihedral) || (l->nimproper > 0 && !l->improper)) throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_lists: null list array");
  if ((l->ndihedral > 0 && dstyle == DIHEDRAL_NONE) || (l->nimproper > 0 && istyle == IMPROPER_NONE))
    throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_lists: a list for a style that is 0");
  for (int c = 0; c < 3; ++c)
    if (!(l->prd[c] >= 0.0) || !std::isfinite(l->prd[c])) throw ConpError(CONP_ERR_ARG, "conp_dihedral_set_lists: prd is negative or not finite");
  const int na = l->nall, nd = l->ndihedral, ni = l->nimproper;
  // every index a kernel will use is checked here, once per list; the same pass counts an atom's slots
  std::vector<int> ptr((size_t)na + 1, 0);
  auto check = [&](const int *list, int n, int ntypes, const char *what) {
    for (int t = 0; t < n; ++t) {
      const int *e = list + 5 * (size_t)t;
      for (int r = 0; r < 4; ++r) {
        if (e[r] < 0 || e[r] >= na) throw ConpError(CONP_ERR_ARG, std::string("conp_dihedral_set_lists: ") + what + " member outside [0, nall)");
        ++ptr[(size_t)e[r] + 1];
      }
      if (e[4] < 1 || e[4] > ntypes) throw ConpError(CONP_ERR_ARG, std::string("conp_dihedral_set_lists: ") + what + " type outside [1, ntypes]");
    }
  };
  check(l->dihedral, nd, ndihedraltypes, "dihedral");
  check(l->improper, ni, nimpropertypes, "improper");
  for (int i = 0; i < na; ++i) ptr[(size_t)i + 1] += ptr[i];
  // the slots of an atom: term * 4 + role, dihedrals first in list order, then impropers in list order, roles in member order
  const size_t nterm = (size_t)nd + ni;
  std::vector<int> slot(4 * nterm), at_(ptr.begin(), ptr.end() - 1);
  for (int t = 0; t < nd; ++t)
    for (int r = 0; r < 4; ++r) slot[(size_t)at_[l->dihedral[5 * (size_t)t + r]]++] = t * 4 + r;
  for (int t = 0; t < ni; ++t)
    for (int r = 0; r < 4; ++r) slot[(size_t)at_[l->improper[5 * (size_t)t + r]]++] = (nd + t) * 4 + r;
  ctx.sync();                                       // no kernel may be reading the old lists
  d_dihedral.upload(l->dihedral, 5 * (size_t)nd, ctx.stream);
  d_improper.upload(l->improper, 5 * (size_t)ni, ctx.stream);
  d_slot_ptr.upload(ptr, ctx.stream);
  d_slot.upload(slot, ctx.stream);
  d_term.reserve(std::max<size_t>(nterm, 1) * DIHEDRAL_TERM_W);
  d_part.reserve(std::max<size_t>((nterm + DIHEDRAL_BLOCK - 1) / DIHEDRAL_BLOCK, 1) * 8);
  d_ev.reserve(8);
  ctx.sync();                                       // the caller's arrays, `ptr` and `slot` need not stay
  nlocal = l->nlocal; nall = na; ndihedral = nd; nimproper = ni;
  for (int c = 0; c < 3; ++c) prd[c] = l->prd[c];
  have_lists = true;
}

// term kernel (+ finish) and gather kernel on the stream; every output is overwritten or, for df, added to once per atom
void DihedralStyle::enqueue(const double *dx, double *df, double *dev, double *dea, double *dva) {
  DihedralArgs a;
  a.ndihedral = ndihedral; a.nimproper = nimproper; a.nlocal = nlocal; a.nall = nall; a.newton = newton_bond;
  a.dstyle = dstyle; a.istyle = istyle;
  a.dihedral = d_dihedral.p; a.improper = d_improper.p; a.dcoef = d_dcoef.p; a.icoef = d_icoef.p;
  for (int c = 0; c < 3; ++c) a.prd[c] = prd[c];
  a.x = dx; a.term = d_term.p; a.part = d_part.p; a.slot_ptr = d_slot_ptr.p; a.slot = d_slot.p;
  a.f = df; a.eatom = dea; a.vatom = dva;
  ctx.prof.begin("dihedral", ctx.stream);
  launch_dihedral(ctx.stream, a, dev);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void DihedralStyle::compute_host(const conp_atoms *at, double *f, double *eng, double *vir, double *eatom, double *vatom) {
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
