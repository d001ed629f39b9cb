// struct PairStyle: lj/cut/coul/long pair forces over the pair style's own half list (conp_pairstyle.cpp, DESIGN.md sections 16, 17).
#pragma once
#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

struct PairStyle {
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  struct Env { int ntypes, newton_pair; double g_ewald, qqrd2e; } env{};      // what the pair style reads of conp_env
  bool have_params = false, have_list = false;
  unsigned long long list_gen = 0;        // counts the lists the handle has held: a transposed index (section 26) belongs to one
  int nall = 0, inum = 0, ntab = 0;
  double cut_coul = 0.0, special_lj[4] = {1, 1, 1, 1}, special_coul[4] = {1, 1, 1, 1};
  dev::DevBuf<double> d_tab, d_part, d_x, d_q, d_f, d_ev, d_ea, d_va;
  dev::DevBuf<double4> d_xq;
  dev::DevBuf<int> d_ilist, d_numneigh, d_first, d_neigh, d_type;
  std::vector<double> out_h;
  // the list built on the device (conp_neigh.hip): scratch of the build, and the owned coordinates it saw
  bool list_built = false;
  int build_nlocal = 0;
  int64_t nneigh = 0;
  double build_cutneigh = 0.0, cutsq_max = 0.0;
  dev::DevBuf<double> d_nb_ext, d_nb_xbuild;
  dev::DevBuf<double4> d_nb_sorted;
  dev::DevBuf<int> d_nb_cell, d_nb_slot, d_nb_count, d_nb_start, d_nb_unsorted;
  dev::DevBuf<long long> d_nb_total;

  // neigh_modify exclude: the rules of conp_pair_set_exclusions; the table and the device pointers of `excl`
  // are filled in per build
  bool have_excl = false;
  NeighExclArgs excl{};
  dev::DevBuf<unsigned char> d_ex_type;

  void set_params(const conp_pair_params *p);
  void set_list(const conp_neighlist *l, int nall_);
  void set_exclusions(const conp_pair_exclusions *e);      // a refused call leaves the handle without rules
  // exclude: conp_pair_build_list_exclude_device (the rules of set_exclusions, the class arrays of `at`); else the plain build
  void build_list(const double *dx, const conp_pair_build_args *a, const conp_pair_exclude_atoms *at = nullptr, bool exclude = false);
  void list_moved(const double *dx, double trigger, int *dflag);
  void get_list(int *inum_, int *nall_, int64_t *nneigh_, int *ilist, int *numneigh, int *first, int *neigh);
  void need_ready(const char *who) const {
    if (!have_params) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_pair_set_params");
    if (!have_list) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_pair_set_list");
  }
  // tv: the list's transposed index -- the atomic-free kernel of section 26; NULL: the atomic kernel
  void enqueue(const double *dx, const double *dq, const int *dtype, int nlocal_, double *df, double *dev, double *dea, double *dva,
               const TransposedView *tv = nullptr);
  // dx, dq: device arrays of the call's atoms, or NULL (at->x, at->q are staged); downloads and adds into f, overwrites the rest
  void compute_host(const conp_atoms *at, const double *dx, const double *dq, double *f, double *eng, double *vir, double *eatom, double *vatom);
};

}  // namespace conp
