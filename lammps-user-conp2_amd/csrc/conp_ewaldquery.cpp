// The exact-Ewald query entries on the device (conp_potential.hip; DESIGN.md sections 11, 12, 14, 15): the structure factor of the
// call's atoms in buffers of the query's own, its projection onto atoms, forces, energy and virial, host arrays or device arrays.
#include "conp_ewaldquery.hpp"

namespace conp {
using namespace dev;

// Atoms per block of phase tables: Rp, Tz, seeds and axis tables of a block stay within EW_TABLES (the 16384 / 262144 box takes
// blocks of a few hundred atoms instead of a 2-GB table over all of them); the split slices of G within EW_SLICES.  With G and
// w o G (R_pad C_pad doubles each: 5 MB at the headline size) that bounds the scratch of these entries.
constexpr size_t EW_TABLES = (size_t)80 << 20, EW_SLICES = (size_t)40 << 20;
int EwaldQuery::block(int n) const {
  const KPlan &pl = plan;
  const size_t per_atom = ((size_t)pl.R_pad + pl.C_pad + 6 + 2 * ((size_t)pl.kxmax + 2) + 2 * ((size_t)pl.kymax + 1)) * sizeof(double);
  int cap = (int)std::max<size_t>(64, std::min<size_t>(8192, EW_TABLES / per_atom / 64 * 64));
  if (debug_ew_block() > 0) cap = debug_ew_block();      // test hook (conp_debug_set_ew_block): several blocks on a deck
  return std::min(cap, std::max(64, (n + 63) / 64 * 64));
}
void EwaldQuery::reserve(int nb_pad) {
  const KPlan &pl = plan;
  const size_t nrp = (size_t)pl.R_pad * nb_pad, ntz = (size_t)pl.C_pad * nb_pad;
  const size_t nxe = (size_t)(pl.kxmax + 2) * nb_pad, nye = (size_t)(pl.kymax + 1) * nb_pad;
  const bool grew = nrp > d_ew_Rp.n || ntz > d_ew_Tz.n || nxe > d_ew_Xe.n || nye > d_ew_Ye.n;
  d_ew_Rp.reserve(nrp); d_ew_Tz.reserve(ntz); d_ew_Xe.reserve(nxe); d_ew_Ye.reserve(nye);
  d_ew_seeds.reserve((size_t)6 * nb_pad);
  // padding rows / columns (planar vectors past np, the kz = 0 sin column, columns past nz) are never written: zero them once per
  // layout (block width, plan); afterwards every block overwrites the same entries
  if (!grew && tables_nb == nb_pad) return;
  HIP_TRY(hipMemsetAsync(d_ew_Rp.p, 0, nrp * sizeof(double), ctx.stream));
  HIP_TRY(hipMemsetAsync(d_ew_Tz.p, 0, ntz * sizeof(double), ctx.stream));
  HIP_TRY(hipMemsetAsync(d_ew_Xe.p, 0, nxe * sizeof(double2), ctx.stream));
  HIP_TRY(hipMemsetAsync(d_ew_Ye.p, 0, nye * sizeof(double2), ctx.stream));
  tables_nb = nb_pad;
}
// phase tables of the nb atoms at xb (device, [nb][3]), nb_pad columns (stale columns >= nb of an earlier block stay finite)
void EwaldQuery::tables_at(const double *xb, int nb, int nb_pad) {
  launch_ew_seeds(ctx.stream, nb, xb, kt.unitk[0], kt.unitk[1], kt.unitk[2], d_ew_seeds.p);
  launch_ele_tables(ctx.stream, dplan, plan.kzt, nb, nb_pad, d_ew_seeds.p, d_ew_Xe.p, d_ew_Ye.p, d_ew_Tz.p, d_ew_Rp.p);
}

// ---- the steps the k-space potential and force entries share (DESIGN.md sections 11-15) ----
// split the atoms of a block over slices of G so that the launch keeps ~6 workgroups on every CU (the LDS limit of ew_sk_kernel;
// each waits on its chunk loads) -- every split owns a slice: no atomics
int EwaldQuery::nsplit(int nb_pad) const {
  const KPlan &pl = plan;
  const int wgs = std::max(1, pl.C_pad / 64 * pl.n_row_tiles);
  int nsplit = std::max(1, std::min({6 * num_cus / wgs + 1, 32, nb_pad / 64}));
  while (nsplit > 1 && (size_t)nsplit * pl.R_pad * pl.C_pad * sizeof(double) > EW_SLICES) --nsplit;
  return nsplit;
}
// S of the n atoms at x (device, [n][3]) with the charges q (device, zeros behind n up to whole blocks) into d_ew_G: block by block
// the phase tables and ew_sk_kernel into the slices, then the slices' sum.  After reserve(nb_pad).
void EwaldQuery::build_S(const double *x, const double *q, int n, int nb_pad) {
  const size_t gsz = (size_t)plan.R_pad * plan.C_pad;
  const int nsplit = this->nsplit(nb_pad);
  d_ew_Gp.reserve(gsz * nsplit); d_ew_G.reserve(gsz); d_ew_Gwf.reserve(gsz);
  HIP_TRY(hipMemsetAsync(d_ew_Gp.p, 0, gsz * nsplit * sizeof(double), ctx.stream));
  for (int b0 = 0; b0 < n; b0 += nb_pad) {
    tables_at(x + 3 * (size_t)b0, std::min(nb_pad, n - b0), nb_pad);
    launch_ew_sk(ctx.stream, dplan, nb_pad, nsplit, d_ew_Rp.p, d_ew_Tz.p, q + b0, d_ew_Gp.p);
  }
  launch_ew_sk_sum(ctx.stream, dplan, nsplit, d_ew_Gp.p, d_ew_G.p);
}
// once per plan: (ug, kx, ky, kz) of the reference's k list into d_ew_kv; the tile lists of the projection into d_ew_tiles / d_ew_ctptr
void EwaldQuery::kv_ready() {
  if (!kv_ready_) {
    const int K = kt.kcount;
    std::vector<double> kv((size_t)4 * K);
    for (int k = 0; k < K; ++k) {
      kv[k] = kt.ug[k];
      kv[(size_t)K + k] = kt.unitk[0] * kt.kxvecs[k]; kv[2 * (size_t)K + k] = kt.unitk[1] * kt.kyvecs[k];
      kv[3 * (size_t)K + k] = kt.unitk[2] * kt.kzvecs[k];
    }
    d_ew_kv.upload(kv, ctx.stream);
    ctx.sync();                     // (kv goes out of scope)
    kv_ready_ = true;
  }
}
void EwaldQuery::tiles_ready() {
  if (!tiles_ready_) {
    d_ew_tiles.upload(tiles_h, ctx.stream); d_ew_ctptr.upload(ct_ptr_h, ctx.stream);
    ctx.sync();
    tiles_ready_ = true;
  }
}
// the seven sums (sum_k ug |S_k|^2, the six virial sums) of d_ew_G into d_ew_ev[0..6]
void EwaldQuery::energy_virial() {
  kv_ready();
  const int K = kt.kcount;
  d_ew_ev.reserve((size_t)7 * (ew_energy_virial_workgroups(K) + 1));
  launch_ew_energy_virial(ctx.stream, K, plan.C_pad, KPlan::PT, d_sf_row_a.p, d_sf_col_c.p, d_k_sign.p, d_ew_kv.p,
                          env.g_ewald, d_ew_G.p, d_ew_ev.p + 7, d_ew_ev.p);
}
// x, q of the owned atoms idx, padded to whole blocks (padding atoms carry no charge), and idx itself into d_ew_x, d_ew_q, d_ew_idx.
// The copies are asynchronous: they are staged in h, which the caller keeps until it has synchronised.
void EwaldQuery::upload_compact(const conp_atoms *at, const std::vector<int> &idx, int nb_pad, Staged &h) {
  const int n = (int)idx.size(), ntot = (n + nb_pad - 1) / nb_pad * nb_pad;
  h.x.assign(3 * (size_t)ntot, 0.0); h.q.assign(ntot, 0.0);
  for (int k = 0; k < n; ++k) {
    const int i = idx[k];
    for (int c = 0; c < 3; ++c) h.x[3 * (size_t)k + c] = at->x[3 * (size_t)i + c];
    h.q[k] = at->q[i];
  }
  reserve(nb_pad);
  d_ew_x.upload(h.x, ctx.stream); d_ew_q.upload(h.q, ctx.stream); d_ew_idx.upload(idx, ctx.stream);
}
// The block loop of the force and per-atom virial kernels over n atoms at x (device) with the charges d_ew_q, from d_ew_Gwf / d_ew_G.
// Host path: x = d_ew_x, idx = d_ew_idx (the outputs are indexed through it, o is complete), every block's tables are rebuilt.
// Device path: x = the caller's array, idx = NULL (block b0 writes the atoms [b0, b0 + nb) of the caller's outputs; Q, M, M2 come
// from d_kf_sums); one block: build_S's tables are still there.  fo, eo, vo NULL: that output is not formed.
void EwaldQuery::force_blocks(int n, int nb_pad, const double *x, const int *idx, const EwForceOut &o, double *fo, double *eo, double *vo) {
  const KPlan &pl = plan;
  const double *uk = kt.unitk, *q = d_ew_q.p;
  d_ew_bk.reserve((size_t)16 * nb_pad);
  if (vo) {
    d_ew_Gwf2.reserve((size_t)pl.R_pad * pl.C_pad); d_ew_vk.reserve((size_t)24 * nb_pad);
    launch_ew_gw2(ctx.stream, dplan, pl.kzt, uk[0], uk[1], uk[2], env.g_ewald, d_ew_G.p, d_ew_Gwf2.p);
  }
  for (int b0 = 0; b0 < n; b0 += nb_pad) {
    const int nb = std::min(nb_pad, n - b0);
    const double *xb = x + 3 * (size_t)b0;
    if (idx || n > nb_pad) tables_at(xb, nb, nb_pad);
    launch_ew_force(ctx.stream, dplan, pl.kzt, uk[0], uk[1], uk[2], nb_pad, d_ew_ctptr.p, d_ew_tiles.p, d_ew_Gwf.p,
                    d_ew_Rp.p, d_ew_Tz.p, d_ew_bk.p);
    if (idx) launch_ew_force_out(ctx.stream, nb, nb_pad, d_ew_bk.p, idx + b0, q + b0, xb, o, fo, eo);
    else if (fo || eo) launch_ew_force_out_device(ctx.stream, nb, nb_pad, d_ew_bk.p, q + b0, xb, o, d_kf_sums.p, b0, fo, eo);
    if (!vo) continue;
    launch_ew_vatom(ctx.stream, dplan, pl.kzt, uk[0], uk[1], uk[2], nb_pad, d_ew_ctptr.p, d_ew_tiles.p, d_ew_Gwf2.p,
                    d_ew_Rp.p, d_ew_Tz.p, d_ew_vk.p);
    if (idx) launch_ew_vatom_out(ctx.stream, nb, nb_pad, d_ew_bk.p, d_ew_vk.p, idx + b0, q + b0, env.qqrd2e, vo);
    else launch_ew_vatom_out_device(ctx.stream, nb, nb_pad, d_ew_bk.p, d_ew_vk.p, q + b0, env.qqrd2e, b0, vo);
  }
}

// w o G of every charged owned atom at the positions and charges of `at` (not the update's cached arrays) into d_ew_Gwf.
// Decomposed ranks: each rank contracts its own atoms, G is summed through the host's all-reduce (km_ewald.cpp:784-785) --
// COLLECTIVE.  Replicated-atom handles (several ranks without conp_fix_set_comm) hold every atom on every rank: no collective.
void EwaldQuery::structure_factor(const conp_atoms *at) {
  // (not upload_compact: no atom at all still takes one block of padding here, and no index list is wanted)
  std::vector<double> xs, qs;
  for (int i = 0; i < at->nlocal; ++i) {
    if (at->q[i] == 0) continue;
    xs.insert(xs.end(), at->x + 3 * (size_t)i, at->x + 3 * (size_t)i + 3);
    qs.push_back(at->q[i]);
  }
  const int n = (int)qs.size();
  const int nb_pad = block(n);
  const int ntot = std::max(nb_pad, (n + nb_pad - 1) / nb_pad * nb_pad);
  xs.resize(3 * (size_t)ntot, 0.0); qs.resize(ntot, 0.0);     // padding atoms carry no charge
  reserve(nb_pad);
  d_ew_x.upload(xs, ctx.stream); d_ew_q.upload(qs, ctx.stream);
  build_S(d_ew_x.p, d_ew_q.p, n, nb_pad);
  if (ranks) {
    const size_t gsz = (size_t)plan.R_pad * plan.C_pad;
    std::vector<double> g(gsz);
    HIP_TRY(hipMemcpyAsync(g.data(), d_ew_G.p, gsz * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    ranks->sum(g.data(), (int64_t)gsz);
    HIP_TRY(hipMemcpyAsync(d_ew_G.p, g.data(), gsz * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
    ctx.sync();
  }
  launch_ew_gw(ctx.stream, dplan, d_ew_G.p, d_ew_Gwf.p);
  HIP_TRY(hipGetLastError());
  ctx.sync();                       // (the host vectors go out of scope)
  g_valid = true; u_valid = false; dev_valid = false;
}
// g_i and u_i = g_i + 2 g_ewald q_i / sqrt(pi) of the owned atoms idx (local indices), at their positions in `at`, from d_ew_Gwf:
// block by block, the block's phase tables, b_project_kernel, ew_out_kernel.  Rank-local.  g, u: [nlocal], only idx written.
void EwaldQuery::project(const conp_atoms *at, const std::vector<int> &idx, double *g, double *u) {
  const int n = (int)idx.size();
  if (n == 0) return;
  const int nb_pad = block(n);
  Staged staged;
  upload_compact(at, idx, nb_pad, staged);
  tiles_ready();
  d_ew_bk.reserve((size_t)4 * nb_pad);
  d_ew_g.reserve(at->nlocal); d_ew_u.reserve(at->nlocal);
  const double selfc = 2.0 * env.g_ewald / MY_PIS;
  for (int b0 = 0; b0 < n; b0 += nb_pad) {
    const int nb = std::min(nb_pad, n - b0);
    tables(b0, nb, nb_pad);
    launch_b_project(ctx.stream, dplan, nb_pad, d_ew_ctptr.p, d_ew_tiles.p, d_ew_Gwf.p, d_ew_Rp.p, d_ew_Tz.p, d_ew_bk.p);
    launch_ew_out(ctx.stream, nb, nb_pad, d_ew_bk.p, d_ew_idx.p + b0, d_ew_q.p + b0, selfc, d_ew_g.p, d_ew_u.p);
  }
  std::vector<double> hg(at->nlocal), hu(at->nlocal);
  HIP_TRY(hipMemcpyAsync(hg.data(), d_ew_g.p, (size_t)at->nlocal * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  HIP_TRY(hipMemcpyAsync(hu.data(), d_ew_u.p, (size_t)at->nlocal * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  HIP_TRY(hipGetLastError());
  ctx.sync();
  for (int i : idx) { if (g) g[i] = hg[i]; if (u) u[i] = hu[i]; }
}
// ---- exact Ewald forces, energy, virial ----
// f_i += qqrd2e q_i grad g_i (+ slab) on every charged owned atom, from d_ew_Gwf at the atoms' positions in `at`: project's
// blocking with ew_force_kernel in b_project_kernel's place; energy and virial from d_ew_G.  The sums of q, q^2, q z, q z^2 over the
// owned atoms are all-reduced under decomposed ranks (COLLECTIVE there); S itself is the caller's business (g_valid).
// vatom: [nlocal][6], overwritten: the per-atom virial.
void EwaldQuery::forces(const conp_atoms *at, double *fout, double *energy, double *virial, double *eatom, double *vatom) {
  const double V = kt.volume, L = env.zprd * env.slab_volfactor;
  std::vector<int> idx;
  double four[4];                                     // Q, Q2, M, M2
  charged_owned(at, idx, four);
  if (ranks) ranks->sum(four, 4);
  if (energy || virial) {
    energy_virial();
    double s7[7];
    HIP_TRY(hipMemcpyAsync(s7, d_ew_ev.p, 7 * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipGetLastError());
    ctx.sync();
    if (energy) *energy = kspace_energy(env, s7[0], four[0], four[1], four[2], four[3], V, L);
    if (virial) for (int c = 0; c < 6; ++c) virial[c] = env.qqrd2e * s7[1 + c];
  }
  if (eatom) std::fill(eatom, eatom + at->nlocal, 0.0);
  if (vatom) std::fill(vatom, vatom + 6 * (size_t)at->nlocal, 0.0);
  const int n = (int)idx.size();
  if (n == 0 || (!fout && !eatom && !vatom)) return;
  const int nb_pad = block(n);
  Staged staged;
  upload_compact(at, idx, nb_pad, staged);
  tiles_ready();
  d_ew_f.reserve(3 * (size_t)at->nlocal); d_ew_e.reserve(at->nlocal);
  if (vatom) d_ew_v.reserve(6 * (size_t)at->nlocal);
  double *const d_v = vatom ? d_ew_v.p : nullptr;
  force_blocks(n, nb_pad, d_ew_x.p, d_ew_idx.p, kspace_out_args(env, V, L, four), d_ew_f.p, d_ew_e.p, d_v);
  download_scatter(ctx, at->nlocal, idx, n, d_ew_f.p, d_ew_e.p, d_v, fout, eatom, vatom);
}
// ---- device-resident k-space forces ----
// structure_factor + forces on the caller's device arrays, every one of the n owned atoms a column and a target (a zero charge adds
// zeros): nothing but launches, device-to-device copies and memsets on the handle's stream once the buffers have their sizes.
// dvatom: [n][6], overwritten.
void EwaldQuery::forces_device(int n, const double *dx, const double *dq, double *df, double *dev, double *deatom, double *dvatom) {
  const double V = kt.volume, L = env.zprd * env.slab_volfactor;
  if (n <= 0) { if (dev) HIP_TRY(hipMemsetAsync(dev, 0, 7 * sizeof(double), ctx.stream)); return; }
  const int nb_pad = block(n);
  const int ntot = (n + nb_pad - 1) / nb_pad * nb_pad;
  reserve(nb_pad);
  // q once into the padded buffer: the last block's padding columns carry no charge; x is read in place, block by block
  d_ew_q.reserve(ntot);
  HIP_TRY(hipMemcpyAsync(d_ew_q.p, dq, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx.stream));
  if (ntot > n) HIP_TRY(hipMemsetAsync(d_ew_q.p + n, 0, (size_t)(ntot - n) * sizeof(double), ctx.stream));
  invalidate();                                  // the host entries' scratch is overwritten from here on
  build_S(dx, d_ew_q.p, n, nb_pad);
  launch_ew_gw(ctx.stream, dplan, d_ew_G.p, d_ew_Gwf.p);
  kspace_four_sums(ctx, d_kf_sums, n, dx, dq);
  if (dev) {
    energy_virial();
    launch_kspace_finish(ctx.stream, kspace_finish_args(env, V, L), d_ew_ev.p, d_kf_sums.p, dev);
  }
  if (df || deatom || dvatom) {
    tiles_ready();
    force_blocks(n, nb_pad, dx, nullptr, kspace_out_args(env, V, L, nullptr), df, deatom, dvatom);
  }
  HIP_TRY(hipGetLastError());
  dev_valid = true;                              // d_ew_Gwf is that of (dx, dq): potential_device may reuse it
}
// ---- compute potential/atom on the device ----
// project on the caller's device arrays.  Without reuse: S of the n owned atoms as forces_device forms it, every atom a column.  Then
// the targets in blocks of block(nt): their x and q gathered into the padded block buffers, the block's phase tables,
// b_project_kernel, ew_out_kernel scattering u through d_targets.  The force entry's next call forms everything it reads afresh.
void EwaldQuery::potential_device(int n, const double *dx, const double *dq, int nt, const int *d_targets, bool reuse, double *d_u) {
  if (!reuse) {
    const int nb_pad = block(n);
    const int ntot = (n + nb_pad - 1) / nb_pad * nb_pad;
    reserve(nb_pad);
    d_ew_q.reserve(ntot);
    HIP_TRY(hipMemcpyAsync(d_ew_q.p, dq, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx.stream));
    if (ntot > n) HIP_TRY(hipMemsetAsync(d_ew_q.p + n, 0, (size_t)(ntot - n) * sizeof(double), ctx.stream));
    invalidate();                                // d_ew_G, d_ew_Gwf and the host entries' scratch are overwritten from here on
    build_S(dx, d_ew_q.p, n, nb_pad);
    launch_ew_gw(ctx.stream, dplan, d_ew_G.p, d_ew_Gwf.p);
  }
  if (nt > 0) {
    const int nb_pad = block(nt);
    const int ntot = (nt + nb_pad - 1) / nb_pad * nb_pad;
    reserve(nb_pad);
    d_ew_x.reserve(3 * (size_t)ntot); d_ew_q.reserve(ntot);
    launch_pot_gather(ctx.stream, nt, ntot, d_targets, dx, dq, d_ew_x.p, d_ew_q.p);
    tiles_ready();
    d_ew_bk.reserve((size_t)4 * nb_pad);
    d_ew_g.reserve(n);
    const double selfc = 2.0 * env.g_ewald / MY_PIS;
    for (int b0 = 0; b0 < nt; b0 += nb_pad) {
      const int nb = std::min(nb_pad, nt - b0);
      tables(b0, nb, nb_pad);
      launch_b_project(ctx.stream, dplan, nb_pad, d_ew_ctptr.p, d_ew_tiles.p, d_ew_Gwf.p, d_ew_Rp.p, d_ew_Tz.p, d_ew_bk.p);
      launch_ew_out(ctx.stream, nb, nb_pad, d_ew_bk.p, d_targets + b0, d_ew_q.p + b0, selfc, d_ew_g.p, d_u);
    }
  }
  HIP_TRY(hipGetLastError());
}

}  // namespace conp
