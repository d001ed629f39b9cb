// The PPPM mesh of a `pppm` handle on the device (conp_pppm.hip; DESIGN.md sections 8, 13, 14, 15): the update's k-space b, density
// bricks, the mesh potential and its per-atom gathers, forces, energy and virial, host arrays or device arrays.
#include "conp_pppmmesh.hpp"

namespace conp {
using namespace dev;

void PppmMesh::build(const conp_env &e) {
  if (e.pppm_nx <= 0 || e.pppm_ny <= 0 || e.pppm_nz <= 0 || e.pppm_order <= 0)
    throw ConpError(CONP_ERR_ARG, "Fix conp couldn't detect a pppm/conp kspace style (which is required with the pppm flag)");
  // a mesh line is transformed in LDS: one that does not fit there (about 3400 points; 5120 for a length that is not
  // 2,3,5-smooth) could not be launched at all -- refused here instead of at the first update
  for (const int n : {e.pppm_nx, e.pppm_ny, e.pppm_nz})
    if (pppm_line_lds_bytes(n) > PPPM_LDS_MAX)
      throw ConpError(CONP_ERR_ARG, "pppm mesh of " + std::to_string(n) + " points along one axis: a line of it does not fit in the "
                                    "LDS of a workgroup (" + std::to_string(pppm_line_lds_bytes(n)) + " > " + std::to_string(PPPM_LDS_MAX) + " bytes)");
  const double lo[3] = {e.boxlo_x, e.boxlo_y, e.boxlo_z}, prd[3] = {e.xprd, e.yprd, e.zprd};
  pppm.build(e.pppm_nx, e.pppm_ny, e.pppm_nz, e.pppm_order, e.g_ewald, e.slab_volfactor, lo, prd);
  d_pp_coeff.upload(pppm.rho_coeff, ctx.stream); d_pp_green.upload(pppm.greensfn, ctx.stream);
  d_pp_tw0.upload(pppm.twid[0], ctx.stream); d_pp_tw1.upload(pppm.twid[1], ctx.stream); d_pp_tw2.upload(pppm.twid[2], ctx.stream);
  d_pp_re.reserve(pppm.nfft); d_pp_im.reserve(pppm.nfft); im_clean = false;
  dpppm.nx = pppm.nx; dpppm.ny = pppm.ny; dpppm.nz = pppm.nz; dpppm.order = pppm.order; dpppm.nlower = pppm.nlower;
  dpppm.nfft = pppm.nfft; dpppm.shift = pppm.shift; dpppm.shiftone = pppm.shiftone; dpppm.delvolinv = pppm.delvolinv;
  for (int c = 0; c < 3; ++c) { dpppm.delinv[c] = pppm.delinv[c]; dpppm.boxlo[c] = pppm.boxlo[c]; }
  dpppm.rho_coeff = d_pp_coeff.p; dpppm.greensfn = d_pp_green.p;
  dpppm.twid[0] = d_pp_tw0.p; dpppm.twid[1] = d_pp_tw1.p; dpppm.twid[2] = d_pp_tw2.p;
}

void PppmMesh::map_electrode(const double *xele, int ne) {
  std::vector<int> eg((size_t)ne * 3);
  std::vector<double> ew((size_t)ne * 24, 0.0);
  for (int i = 0; i < ne; ++i)
    for (int c = 0; c < 3; ++c) {
      const double xlo = xele[3 * (size_t)i + c] - pppm.boxlo[c];
      const int n = static_cast<int>(xlo * pppm.delinv[c] + pppm.shift) - PppmPlan::OFFSET;
      eg[3 * (size_t)i + c] = n;
      pppm.rho1d(n + pppm.shiftone - xlo * pppm.delinv[c], &ew[(size_t)i * 24 + 8 * c]);
    }
  d_pp_egrid.upload(eg, ctx.stream); d_pp_ew.upload(ew, ctx.stream);
  ctx.sync();                      // (the host vectors go out of scope)
}

void PppmMesh::b(int nl, const int *eidx, const double *ex, const double *eq, int ne, int ne_pad, double *d_slab_part, int *n_slab_part,
                 DevBuf<double> &d_bk, const BRowArgs *pairs, double *d_breal, BRowArgs *fin, bool rank0) {
  ctx.prof.begin("pppm_b", ctx.stream);
  if (rank0)
    launch_pppm_b(ctx.stream, dpppm, nl, eidx, ex, eq, ne, ne_pad, d_pp_egrid.p, d_pp_ew.p, d_pp_re.p, d_pp_im.p, d_slab_part,
                  n_slab_part, d_bk.p, &im_clean, pairs, d_breal, fin, keep ? (d_pp_elyte.reserve((size_t)dpppm.nfft), d_pp_elyte.p) : nullptr);
  else
    d_bk.zero(ctx.stream);
  ++elyte_spreads;
  elyte_valid = keep && rank0;
  dev_u_valid = false;             // (the update's mesh pass went through d_pp_re)
  ctx.prof.end(ctx.stream);
}

// Spatially decomposed ranks: the mesh potentials and density bricks are those of ALL atoms.  Every rank gathers the charged owned
// atoms of all ranks -- (x, q, kind), ONE gather per query -- and spreads them onto its own copy of the whole mesh: a REPLICATED
// mesh (the reference's ranks own bricks of it and exchange ghost planes, pppm_conp.cpp:114,122 GridComm; the mesh of the `pppm`
// mode is 10^5..10^6 points), so the collective call gives every rank the same brick and the potentials of its own atoms.  The
// gathered atoms live in buffers of their OWN (d_pp_xg / d_pp_qg / d_pp_iota): the per-update electrolyte gather of the decomposed b
// path keeps the handle's to itself.  n[kind] / first[kind]: the atoms of a kind are one run of d_pp_iota (0 electrolyte,
// 1 electrode); kind 2 = all = the whole list.
PppmMesh::Gather PppmMesh::gather_all(const conp_atoms *at) {
  std::vector<double> pack;
  for (int i = 0; i < at->nlocal; ++i) {
    if (at->q[i] == 0) continue;
    pack.push_back(at->x[3 * (size_t)i]); pack.push_back(at->x[3 * (size_t)i + 1]); pack.push_back(at->x[3 * (size_t)i + 2]);
    pack.push_back(at->q[i]); pack.push_back(at->echeck[i] != 0 ? 1.0 : 0.0);
  }
  std::vector<int> counts(ranks->nranks(), 0);
  ranks->allgather_int((int)(pack.size() / 5), counts.data());
  int n = 0;
  for (int v : counts) n += v;
  std::vector<double> all((size_t)std::max(n, 1) * 5), xs((size_t)std::max(n, 1) * 3), qs(std::max(n, 1));
  if (pack.empty()) pack.resize(5);
  ranks->gatherv(pack.data(), counts, 5, all.data());
  std::vector<int> iota;
  iota.reserve(std::max(n, 1));
  Gather g{};
  for (int kind = 0; kind < 2; ++kind) {
    g.first[kind] = (int)iota.size();
    for (int k = 0; k < n; ++k) if ((all[5 * (size_t)k + 4] != 0.0) == (kind == 1)) iota.push_back(k);
    g.n[kind] = (int)iota.size() - g.first[kind];
  }
  g.first[2] = 0; g.n[2] = n;
  for (int k = 0; k < n; ++k) {
    xs[3 * (size_t)k] = all[5 * (size_t)k]; xs[3 * (size_t)k + 1] = all[5 * (size_t)k + 1]; xs[3 * (size_t)k + 2] = all[5 * (size_t)k + 2];
    qs[k] = all[5 * (size_t)k + 3];
  }
  if (iota.empty()) iota.push_back(0);
  d_pp_iota.upload(iota, ctx.stream);
  iota_n = 0;
  d_pp_xg.upload(xs, ctx.stream); d_pp_qg.upload(qs, ctx.stream);
  ctx.sync();                      // (the host vectors go out of scope)
  return g;
}
// the index list of the owned atoms that carry charge, by kind (0 electrolyte, 1 electrode, 2 all), into d_idx
int PppmMesh::list(const conp_atoms *at, int kind, DevBuf<int> &d_idx) {
  std::vector<int> idx;
  for (int i = 0; i < at->nlocal; ++i) {
    if (at->q[i] == 0) continue;
    if (kind == 0 && at->echeck[i] != 0) continue;
    if (kind == 1 && at->echeck[i] == 0) continue;
    idx.push_back(i);
  }
  const int n = (int)idx.size();
  if (idx.empty()) idx.push_back(0);
  d_idx.upload(idx, ctx.stream);
  return n;
}
void PppmMesh::density(int n, const int *d_list, const double *dx, const double *dq, double *rho) {
  d_pp_scratch.reserve(2048);
  launch_pppm_density(ctx.stream, dpppm, n, d_list, dx, dq, rho, d_pp_scratch.p);
}

void PppmMesh::spread_charged(const conp_atoms *at, const int *d_list, int n, const double *dx, const double *dq) {
  if (ranks) {
    const Gather g = gather_all(at);
    density(g.n[2], d_pp_iota.p, d_pp_xg.p, d_pp_qg.p, d_pp_re.p);
  } else
    density(n, d_list, dx, dq, d_pp_re.p);
  ++elyte_spreads;
  u_valid = dev_u_valid = false;   // (d_pp_re holds a density now)
}

void PppmMesh::total_potential(const conp_atoms *at, const double *dx, const double *dq) {
  const int n = ranks ? 0 : list(at, 2, d_pp_fidx);
  spread_charged(at, d_pp_fidx.p, n, dx, dq);
  launch_pppm_poisson(ctx.stream, dpppm, d_pp_re.p, d_pp_im.p); im_clean = false;
  HIP_TRY(hipGetLastError());
  ctx.sync();                      // (list's host vector went out of scope)
  u_valid = true;
}

void PppmMesh::probe(const std::vector<int> &idx, const double *dx, const double *dq, double self_coef, double *out) {
  if (idx.empty()) return;
  const int lo = idx.front(), n = idx.back() + 1 - lo;      // (ascending: the kernel writes d_pp_out[lo .. lo + n) only)
  d_pp_fidx.upload(idx, ctx.stream);
  d_pp_out.reserve((size_t)lo + n);
  launch_pppm_probe(ctx.stream, dpppm, (int)idx.size(), d_pp_fidx.p, dx, dq, d_pp_re.p, self_coef, d_pp_out.p);
  std::vector<double> h(n);
  HIP_TRY(hipMemcpyAsync(h.data(), d_pp_out.p + lo, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
  for (size_t k = 0; k < idx.size(); ++k) out[k] = h[idx[k] - lo];
}

// the bricks of PPPMCONP's make_rho override (pppm_conp.cpp:434-450): electrode, electrolyte, and their sum
void PppmMesh::make_rho(const conp_atoms *at, const double *dx, const double *dq, double *density_out, double *ele_density,
                        double *elyte_density) {
  const size_t nf = (size_t)dpppm.nfft;
  d_pp_ele.reserve(nf);
  std::vector<double> e(nf), l(nf);
  DevBuf<int> d_idx0, d_idx1;
  Gather g{};
  if (ranks) g = gather_all(at);                            // ONE gather, the atoms tagged with their kind
  if (ranks)
    density(g.n[1], d_pp_iota.p + g.first[1], d_pp_xg.p, d_pp_qg.p, d_pp_ele.p);
  else {
    const int n = list(at, 1, d_idx1);                      // ele_make_rho (pppm_conp.cpp:385-426)
    density(n, d_idx1.p, dx, dq, d_pp_ele.p);
  }
  HIP_TRY(hipMemcpyAsync(e.data(), d_pp_ele.p, nf * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  if (elyte_valid && !ranks) {
    // the brick b left for this step (elyte_mapped, pppm_conp.cpp:437-442): no second spread of the electrolyte
    HIP_TRY(hipMemcpyAsync(l.data(), d_pp_elyte.p, nf * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  } else {
    if (ranks)
      density(g.n[0], d_pp_iota.p + g.first[0], d_pp_xg.p, d_pp_qg.p, d_pp_re.p);
    else {
      const int n = list(at, 0, d_idx0);                    // elyte_make_rho (:172-228)
      density(n, d_idx0.p, dx, dq, d_pp_re.p);
    }
    ++elyte_spreads;
    u_valid = dev_u_valid = false;                          // (d_pp_re holds a density now)
    HIP_TRY(hipMemcpyAsync(l.data(), d_pp_re.p, nf * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  }
  ctx.sync();
  if (ele_density) std::memcpy(ele_density, e.data(), nf * sizeof(double));
  if (elyte_density) std::memcpy(elyte_density, l.data(), nf * sizeof(double));
  if (density_out) for (size_t k = 0; k < nf; ++k) density_out[k] = l[k] + e[k];
}

PppmMesh::Geom PppmMesh::geometry() const {
  const double L = env.zprd * env.slab_volfactor;
  return Geom{L, xprd * yprd * L, {2.0 * MY_PI / xprd, 2.0 * MY_PI / yprd, 2.0 * MY_PI / L}};
}
// The mesh solve of the force entries, from the density brick in d_pp_re, in two halves (the device entry gathers the per-atom
// virial between them).  mesh_spectra: forward transform; with vb, the six v_ab fields into d_pp_v[] and their pointers into vb
// (rho^ is still in (re, im) then: the kspace launch overwrites it).  mesh_forces: pppm_kspace_kernel -- the seven sums into
// d_pp_kpart[0..6]; d_ev: energy and virial from them (kspace_finish_kernel) -- then, with want_u, u and E_z back into
// (d_pp_re, d_pp_im) and, with fields, E_x and E_y into (d_pp_ex, d_pp_ey).  The event brackets record under conp_fix_profile only.
void PppmMesh::mesh_spectra(const Geom &gm, bool fields, double **vb) {
  const size_t nf = (size_t)dpppm.nfft;
  if (fields) { d_pp_ex.reserve(nf); d_pp_ey.reserve(nf); }
  d_pp_kpart.reserve((size_t)7 * (pppm_kspace_workgroups(dpppm.nfft) + 1));
  ctx.prof.begin("pppm_f_forward", ctx.stream);
  launch_pppm_forward(ctx.stream, dpppm, d_pp_re.p, d_pp_im.p);
  ctx.prof.end(ctx.stream);
  if (!vb) return;
  for (int c = 0; c < 6; ++c) { d_pp_v[c].reserve(nf); vb[c] = d_pp_v[c].p; }
  launch_pppm_vatom_spectra(ctx.stream, dpppm, gm.uk, env.g_ewald, d_pp_re.p, d_pp_im.p, vb);
  for (int c = 0; c < 6; c += 2) launch_pppm_backward(ctx.stream, dpppm, vb[c], vb[c + 1]);
}
void PppmMesh::mesh_forces(const Geom &gm, bool fields, bool want_u, double *d_ev) {
  ctx.prof.begin("pppm_f_kspace", ctx.stream);
  launch_pppm_kspace(ctx.stream, dpppm, gm.uk, env.g_ewald, gm.V, d_pp_re.p, d_pp_im.p, fields ? d_pp_ex.p : nullptr,
                     fields ? d_pp_ey.p : nullptr, d_pp_kpart.p + 7, d_pp_kpart.p);
  ctx.prof.end(ctx.stream);
  im_clean = false;
  if (d_ev) launch_kspace_finish(ctx.stream, kspace_finish_args(env, gm.V, gm.L), d_pp_kpart.p, d_kf_sums.p, d_ev);
  if (!want_u) return;
  ctx.prof.begin("pppm_f_backward", ctx.stream);
  launch_pppm_backward(ctx.stream, dpppm, d_pp_re.p, d_pp_im.p);
  if (fields) launch_pppm_backward(ctx.stream, dpppm, d_pp_ex.p, d_pp_ey.p);
  ctx.prof.end(ctx.stream);
}

// ---- PPPM forces, energy, virial ----
// PPPM::compute with ik differentiation on the mesh, at the positions and charges of `at`: the brick of every charged atom is spread
// afresh on every call (a kept electrolyte brick is that of the update's positions: never contracted with atoms that may have moved),
// forward transform, pppm_kspace_kernel, two packed backward transforms, pppm_force_gather_kernel on the charged owned atoms.
// COLLECTIVE under decomposed ranks like total_potential (one tagged gather, a replicated mesh) plus the four sums.  Leaves u in
// d_pp_re (u_valid), as total_potential does.  vatom: [nlocal][6], overwritten: the per-atom virial.
void PppmMesh::forces(const conp_atoms *at, const double *dx, const double *dq, double *fout, double *energy, double *virial,
                      double *eatom, double *vatom) {
  const Geom gm = geometry();
  std::vector<int> idx;
  double four[4];                                     // Q, Q2, M, M2
  charged_owned(at, idx, four);
  const int n = (int)idx.size();
  if (idx.empty()) idx.push_back(0);
  d_pp_fidx.upload(idx, ctx.stream);
  if (!ranks) ctx.prof.begin("pppm_f_spread", ctx.stream);
  spread_charged(at, d_pp_fidx.p, n, dx, dq);
  if (!ranks) ctx.prof.end(ctx.stream);
  if (ranks) ranks->sum(four, 4);
  const bool fields = fout != nullptr && n > 0, want_v = vatom != nullptr && n > 0, per_atom = n > 0 && (fout || eatom);
  double *vb[6];
  mesh_spectra(gm, fields, want_v ? vb : nullptr);
  mesh_forces(gm, fields, true, nullptr);
  double s7[7];
  HIP_TRY(hipMemcpyAsync(s7, d_pp_kpart.p, 7 * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  if (want_v) {
    d_pp_vo.reserve(6 * (size_t)at->nlocal);
    launch_pppm_vatom_gather(ctx.stream, dpppm, n, d_pp_fidx.p, dx, dq, vb, env.qqrd2e, d_pp_vo.p);
  }
  if (per_atom) {
    if (fout) d_pp_fo.reserve(3 * (size_t)at->nlocal);
    if (eatom) d_pp_eo.reserve(at->nlocal);
    ctx.prof.begin("pppm_f_gather", ctx.stream);
    launch_pppm_force_gather(ctx.stream, dpppm, n, d_pp_fidx.p, dx, dq, fout ? d_pp_ex.p : nullptr, d_pp_ey.p, d_pp_im.p, d_pp_re.p,
                             kspace_out_args(env, gm.V, gm.L, four), fout ? d_pp_fo.p : nullptr, eatom ? d_pp_eo.p : nullptr);
    ctx.prof.end(ctx.stream);
  }
  if (eatom) std::fill(eatom, eatom + at->nlocal, 0.0);
  if (vatom) std::fill(vatom, vatom + 6 * (size_t)at->nlocal, 0.0);
  download_scatter(ctx, at->nlocal, idx, n, per_atom && fout ? d_pp_fo.p : nullptr, per_atom && eatom ? d_pp_eo.p : nullptr,
                   want_v ? d_pp_vo.p : nullptr, fout, eatom, vatom);
  u_valid = true;
  if (ranks) {
    // every rank spread the same atoms, but a mesh point's contributions arrive in no fixed order (atomic adds): the bricks agree to
    // rounding only.  Rank 0's sums are everybody's (x + 0 + .. + 0 = x): the same energy and virial on every rank, bit for bit.
    if (ranks->rank() != 0) std::fill(s7, s7 + 7, 0.0);
    ranks->sum(s7, 7);
  }
  if (energy) *energy = kspace_energy(env, s7[0], four[0], four[1], four[2], four[3], gm.V, gm.L);
  if (virial) for (int c = 0; c < 6; ++c) virial[c] = env.qqrd2e * s7[1 + c];
}

// ---- device-resident k-space forces ----
// forces on the caller's device arrays: the brick of the n owned atoms through the identity list, the mesh solve, the gather on
// every owned atom; the seven sums stay on the device (kspace_finish_kernel reads them).  dvatom: [n][6], overwritten.
void PppmMesh::identity_list(int n) {
  if (iota_n >= n) return;
  std::vector<int> iota(n);
  for (int i = 0; i < n; ++i) iota[i] = i;
  d_pp_iota.upload(iota, ctx.stream);
  ctx.sync();                        // (iota goes out of scope)
  iota_n = n;
}
void PppmMesh::forces_device(int n, const double *dx, const double *dq, double *df, double *dev, double *deatom, double *dvatom) {
  const Geom gm = geometry();
  if (n <= 0) { if (dev) HIP_TRY(hipMemsetAsync(dev, 0, 7 * sizeof(double), ctx.stream)); return; }
  identity_list(n);
  u_valid = dev_u_valid = false;     // d_pp_re is overwritten from here on
  density(n, d_pp_iota.p, dx, dq, d_pp_re.p);
  ++elyte_spreads;
  kspace_four_sums(ctx, d_kf_sums, n, dx, dq);
  const bool fields = df != nullptr, per_atom = df || deatom;
  double *vb[6];
  mesh_spectra(gm, fields, dvatom ? vb : nullptr);
  if (dvatom) launch_pppm_vatom_gather(ctx.stream, dpppm, n, nullptr, dx, dq, vb, env.qqrd2e, dvatom);
  mesh_forces(gm, fields, per_atom, dev);
  if (per_atom)
    launch_pppm_force_gather_device(ctx.stream, dpppm, n, dx, dq, fields ? d_pp_ex.p : nullptr, d_pp_ey.p, d_pp_im.p, d_pp_re.p,
                                    kspace_out_args(env, gm.V, gm.L, nullptr), d_kf_sums.p, df, deatom);
  HIP_TRY(hipGetLastError());
  dev_u_valid = per_atom;            // u of (dx, dq) is back in d_pp_re: potential_device may reuse it
}
// ---- compute potential/atom on the device ----
// total_potential + probe on the caller's device arrays: the brick of the n owned atoms through the identity list (a zero charge
// spreads zeros), the Poisson solve, the stencil gather at the targets, written by owned index.
void PppmMesh::potential_device(int n, const double *dx, const double *dq, int nt, const int *d_targets, bool reuse, double self_coef,
                                double *d_u) {
  if (!reuse) {
    identity_list(n);
    u_valid = dev_u_valid = false;   // d_pp_re is overwritten from here on (a kept electrolyte brick is not: as in forces_device)
    density(n, d_pp_iota.p, dx, dq, d_pp_re.p);
    ++elyte_spreads;
    launch_pppm_poisson(ctx.stream, dpppm, d_pp_re.p, d_pp_im.p); im_clean = false;
  }
  if (nt > 0) launch_pppm_probe(ctx.stream, dpppm, nt, d_targets, dx, dq, d_pp_re.p, self_coef, d_u);
  HIP_TRY(hipGetLastError());
}

}  // namespace conp
