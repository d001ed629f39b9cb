// struct EwaldQuery: the exact-Ewald query entries -- per-atom potential, forces, energy, virial, per-atom virial and their
// device-resident twins (conp_ewaldquery.cpp, conp_potential.hip; DESIGN.md sections 11, 12, 14, 15).
#pragma once
#include "conp_host.hpp"
#include "conp_kspace_common.hpp"

namespace conp {

struct EwaldQuery {
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  // the handle's k tables and plan (km_conp_setup rebuilds them in place, then calls replan()) and what it uploaded of them
  const KTables &kt;  const KPlan &plan;  const DevPlan &dplan;
  const std::vector<SkTile> &tiles_h;  const std::vector<int> &ct_ptr_h;
  const dev::DevBuf<int> &d_sf_row_a, &d_sf_col_c, &d_k_sign;
  KspaceEnv env{};
  int num_cus = 256;
  RankOps *ranks = nullptr;         // spatially decomposed atoms (conp_fix_set_comm): the host's all-reduce; else NULL

  // The structure factor of every charged owned atom (all ranks' under decomposition) in buffers of its own -- the update's schedule,
  // tables and G are not touched.  g_valid: d_ew_Gwf holds w o G of the atoms a collective entry last saw; u_valid: u_h holds u_i of
  // every owned atom (the per-atom entry's cache).  Both are dropped by every update, re-neighbour, set_matrix and k-table setup.
  bool g_valid = false, u_valid = false;
  std::vector<double> u_h;
  // dev_valid: d_ew_Gwf holds w o G of the arrays the last forces_device saw, which potential_device may reuse (DESIGN.md section
  // 27).  Dropped with the other two, and by every other writer of d_ew_G / d_ew_Gwf (structure_factor, potential_device's own S).
  bool dev_valid = false;
  void invalidate() { g_valid = u_valid = dev_valid = false; }
  // the handle has a new plan: the caches go, and the phase tables' zeroed padding, d_ew_kv and the tile lists are the old plan's
  void replan() { invalidate(); tables_nb = 0; kv_ready_ = tiles_ready_ = false; }

  void structure_factor(const conp_atoms *at);
  void project(const conp_atoms *at, const std::vector<int> &idx, double *g, double *u);
  void forces(const conp_atoms *at, double *fout, double *energy, double *virial, double *eatom, double *vatom);
  void forces_device(int n, const double *dx, const double *dq, double *df, double *dev, double *deatom, double *dvatom);
  // d_u[t] = u_t = g_t + 2 g_ewald q_t / sqrt(pi) at the nt owned targets d_targets (device, ascending) of the n owned atoms (dx, dq);
  // reuse: from d_ew_Gwf as forces_device left it (dev_valid), else S of the call's atoms is formed first.  Enqueues only.
  void potential_device(int n, const double *dx, const double *dq, int nt, const int *d_targets, bool reuse, double *d_u);

  int tables_nb = 0;                // block width the phase-table buffers were zeroed for (padding entries stay zero); 0: none
  bool kv_ready_ = false, tiles_ready_ = false;      // d_ew_kv / d_ew_tiles, d_ew_ctptr hold the current plan's
  dev::DevBuf<double> d_ew_G, d_ew_Gp, d_ew_Gwf, d_ew_x, d_ew_q, d_ew_seeds, d_ew_Rp, d_ew_Tz, d_ew_bk, d_ew_g, d_ew_u;
  dev::DevBuf<double> d_ew_kv, d_ew_ev, d_ew_f, d_ew_e;      // forces: (ug, k) per listed k, the seven sums, outputs
  dev::DevBuf<double> d_ew_Gwf2, d_ew_vk, d_ew_v;            // vatom: (c o w) o G, ew_vatom_kernel's parts, the per-atom virial
  dev::DevBuf<double2> d_ew_Xe, d_ew_Ye;
  dev::DevBuf<int> d_ew_idx, d_ew_ctptr;
  dev::DevBuf<SkTile> d_ew_tiles;
  // the device-resident force entry: Q, Q2, M, M2 of the call's atoms with the workgroups' partial rows behind
  dev::DevBuf<double> d_kf_sums;

  struct Staged { std::vector<double> x, q; };
  int block(int n) const;  void reserve(int nb_pad);
  void tables_at(const double *xb, int nb, int nb_pad);
  void tables(int b0, int nb, int nb_pad) { tables_at(d_ew_x.p + 3 * (size_t)b0, nb, nb_pad); }   // ... of atoms [b0, b0 + nb) of d_ew_x
  int nsplit(int nb_pad) const;
  void build_S(const double *x, const double *q, int n, int nb_pad);
  void kv_ready(), tiles_ready(), energy_virial();
  void upload_compact(const conp_atoms *at, const std::vector<int> &idx, int nb_pad, Staged &h);
  void force_blocks(int n, int nb_pad, const double *x, const int *idx, const EwForceOut &o, double *fo, double *eo, double *vo);
};

}  // namespace conp
