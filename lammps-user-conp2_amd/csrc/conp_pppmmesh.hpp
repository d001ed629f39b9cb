// struct PppmMesh: the PPPM mesh of a `pppm` handle -- the update's k-space b, the density bricks, the mesh potential and its
// per-atom gathers, forces, energy, virial, per-atom virial and their device-resident twins (conp_pppmmesh.cpp, conp_pppm.hip;
// DESIGN.md sections 8, 13, 14, 15).  Every method takes the device x and q it reads: the host entries pass the handle's copies
// after the handle's upload, the update and the device entries the caller's arrays.
#pragma once
#include "conp_host.hpp"
#include "conp_kspace_common.hpp"

namespace conp {

struct PppmMesh {
  explicit PppmMesh(dev::DevCtx &c) : ctx(c) {}
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  KspaceEnv env{};
  double xprd = 0, yprd = 0;
  RankOps *ranks = nullptr;         // spatially decomposed atoms (conp_fix_set_comm): the host's collectives; else NULL

  // fix_conp.cpp:401-404: the `pppm` keyword needs the pppm/conp kspace style; here: its mesh and order via conp_env
  void build(const conp_env &e);
  bool ready() const { return dpppm.nfft > 0; }
  // aaa_map_rho (pppm_conp.cpp:318-344): stencil weights and lower-left mesh index of the ne electrode atoms at xele [ne][3] (host)
  void map_electrode(const double *xele, int ne);

  // PPPMCONP's per-step caches (pppm_conp.cpp: elyte_density_brick + elyte_mapped, u_brick): keep -- a host that overrides
  // PPPM::make_rho asked for the electrolyte brick of every b_cal (conp_pppm_keep_density); elyte_valid -- d_pp_elyte holds the
  // brick of the LAST b_cal and nothing has moved since; u_valid -- d_pp_re holds the mesh potential of the total density
  // (total_potential and forces leave it), so probe only gathers from it.  Otherwise d_pp_re holds a density or nothing usable.
  // dev_u_valid -- d_pp_re holds the mesh potential forces_device left (called with d_f or d_eatom), which potential_device may
  // reuse; dropped with the other caches and by every other writer of d_pp_re.
  bool keep = false, elyte_valid = false, u_valid = false, dev_u_valid = false;
  int elyte_spreads = 0;            // how often the electrolyte atoms were spread onto the mesh (b and the density queries)
  // positions / charges may have changed (an update, a re-neighbour): the caches are this step's or nobody's
  void invalidate() { elyte_valid = u_valid = dev_u_valid = false; }
  void keep_density(bool on) { keep = on; invalidate(); }

  // The update's entry (pppm_conp.cpp:269-316): the k-space b of the ne electrode atoms from the nl electrolyte atoms eidx of
  // (ex, eq) into d_bk -- on rank 0, the mesh is not sharded; the others zero d_bk.  pairs, d_breal, fin: launch_pppm_b's (NULL:
  // the rows of b are completed behind the mesh).  Enqueues only: the device update is graph-captured around it.
  void b(int nl, const int *eidx, const double *ex, const double *eq, int ne, int ne_pad, double *d_slab_part, int *n_slab_part,
         dev::DevBuf<double> &d_bk, const BRowArgs *pairs, double *d_breal, BRowArgs *fin, bool rank0);
  // The density brick of every charged atom into d_pp_re: under ranks all ranks' atoms (gather_all: COLLECTIVE), else the n atoms
  // d_list (the charged owned ones, ascending) of (dx, dq).
  void spread_charged(const conp_atoms *at, const int *d_list, int n, const double *dx, const double *dq);
  // u_brick of the total density into d_pp_re (what PPPM::compute leaves there with per-atom energies on).  COLLECTIVE under ranks.
  void total_potential(const conp_atoms *at, const double *dx, const double *dq);
  // out[k] = the mesh potential at atom idx[k] (ascending) of (dx, dq) minus self_coef q, from the brick as it is.  Synchronises.
  void probe(const std::vector<int> &idx, const double *dx, const double *dq, double self_coef, double *out);
  void make_rho(const conp_atoms *at, const double *dx, const double *dq, double *density, double *ele_density, double *elyte_density);
  void forces(const conp_atoms *at, const double *dx, const double *dq, double *fout, double *energy, double *virial, double *eatom,
              double *vatom);
  void forces_device(int n, const double *dx, const double *dq, double *df, double *dev, double *deatom, double *dvatom);
  // d_u[t] = the mesh potential at the nt owned targets d_targets (device, ascending) of the n owned atoms (dx, dq) minus
  // self_coef q_t; reuse: from the brick as forces_device left it (dev_u_valid), else density and mesh solve first.  Enqueues only.
  void potential_device(int n, const double *dx, const double *dq, int nt, const int *d_targets, bool reuse, double self_coef, double *d_u);

 private:
  PppmPlan pppm;
  PppmDev dpppm{};
  bool im_clean = false;            // the mesh's imaginary brick is all zero (left so by the b path's last backward pass)
  dev::DevBuf<double> d_pp_coeff, d_pp_green, d_pp_tw0, d_pp_tw1, d_pp_tw2, d_pp_re, d_pp_im, d_pp_ew, d_pp_scratch;
  dev::DevBuf<int> d_pp_egrid;
  dev::DevBuf<double> d_pp_elyte, d_pp_ele, d_pp_xg, d_pp_qg;
  dev::DevBuf<double> d_pp_ex, d_pp_ey, d_pp_kpart, d_pp_fo, d_pp_eo;      // forces: E_x, E_y bricks, the seven sums, outputs
  dev::DevBuf<double> d_pp_v[6], d_pp_vo;      // vatom: the six v_ab bricks (xx, yy, zz, xy, xz, yz), the per-atom virial (section 15)
  dev::DevBuf<double> d_pp_out;                // probe's output, indexed by atom
  dev::DevBuf<int> d_pp_fidx, d_pp_iota;
  // the device-resident force entry: Q, Q2, M, M2 of the call's atoms with the workgroups' partial rows behind
  // them; how many leading entries of d_pp_iota are the identity list 0, 1, 2, ... (gather_all, the only other writer, resets it)
  dev::DevBuf<double> d_kf_sums;
  int iota_n = 0;

  struct Gather { int n[3], first[3]; };
  Gather gather_all(const conp_atoms *at);
  int list(const conp_atoms *at, int kind, dev::DevBuf<int> &d_idx);
  void identity_list(int n);                   // d_pp_iota's first n entries are 0, 1, 2, ... afterwards
  void density(int n, const int *d_list, const double *dx, const double *dq, double *rho);
  struct Geom { double L, V, uk[3]; };         // the mesh's box: L = the slab-extended z period, V, the unit wave vectors
  Geom geometry() const;
  void mesh_spectra(const Geom &gm, bool fields, double **vb /*[6], or NULL: no per-atom virial*/);
  void mesh_forces(const Geom &gm, bool fields, bool want_u, double *d_ev /*[7], or NULL*/);
};

}  // namespace conp
