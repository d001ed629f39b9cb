// glue_driver -- a miniature host that drives FixConpHip the way LAMMPS does, on top of the interface mock.
// It exists to EXECUTE the C++ glue (constructor / init / init_list / setup_* / post_neighbor / pre_force / post_force /
// compute_scalar / modify_param, log-file writing, error->all propagation, and the MPI-backed conp_comm callbacks) against
// libconp_hip.so on a real GPU; the numerical content is checked by tests/test_gpu_glue.py against the ctypes path through the
// same library.
//
// usage: glue_driver CASEFILE                      one rank, FixConpHip (INTEGRATION.md mode A)
//        glue_driver CASEFILE compute              mode A, then `compute potential/atom/hip kspace` on the conp/hip fix (Ewald)
//        glue_driver CASEFILE kspace [vatom]       mode A with `kspace_style ewald/conp/hip` as force->kspace: on every step, after the
//                                                  fix's pre_force, compute(eflag, vflag) on the fix's handle; output per step
//                                                  "kf STEP TAG FX FY FZ", "kea STEP TAG E" per owned atom, "ke STEP ENERGY", "kv STEP W[6]".
//                                                  With the word `vatom` compute() is asked for the per-atom virial too (vflag | 4)
//                                                  and "kva STEP TAG V[6]" (xx yy zz xy xz yz) follows per owned atom
//        glue_driver CASEFILE pair [vatom|table]   mode A with `pair_style lj/cut/coul/long/conp/hip` as force->pair: on every step, after the
//                                                  fix's pre_force, compute(eflag, vflag) on the fix's handle with atom->f cleared; the
//                                                  style's tables come from the optional block behind the steps (below).  Output per step:
//                                                  "pf STEP INDEX FX FY FZ" and "pea STEP INDEX E" for all nlocal + nghost atoms,
//                                                  "pe STEP EVDWL ECOUL", "pv STEP W[6]", "pls STEP N" (list uploads so far); with `vatom`
//                                                  also "pva STEP INDEX V[6]"; `table` leaves pair_modify table at LAMMPS' default 12:
//                                                  compute() stops with the style's message
//        glue_driver CASEFILE pppmforce [vatom|ad|nohandle]
//                                                  mode A with the `pppm` keyword and `kspace_style pppm/conp/hip ACC device` as
//                                                  force->kspace: on every step, after the fix's pre_force, compute(eflag, vflag) on
//                                                  the fix's handle (conp_pppm_compute_forces); output as in the kspace mode.  The third
//                                                  word asks for the per-atom virial / sets kspace_modify diff ad / hides the fix
//                                                  from Modify::fix: each stops with the style's message
//        glue_driver CASEFILE pppmhost             the provider mode with `kspace_style pppm/conp/hip ACC` (no `device`) parsed by the
//                                                  style's settings(): the same output as `provider`
//        glue_driver CASEFILE provider             mode B: the reference's FixConp keeps its loops, only `kspmod` is replaced:
//                                                  a stand-in for the fix's public members is registered with KSpaceModuleHip
//                                                  (register_fix, fix_conp.cpp:409) and conp_setup / conp_post_neighbor / a_cal /
//                                                  b_cal run; output "a I J VALUE" (local row I, global column J), "b I VALUE"
//        glue_driver ranks N CASE_0 .. CASE_N-1 [provider]
//                                                  N rank THREADS, one per sub-domain case file (LAMMPS' spatial decomposition:
//                                                  owned atoms + ghosts + lists of that rank), collectives through the MPI mock;
//                                                  every output line is prefixed "rank R "
// case file (whitespace-separated tokens, written by the test):
//   ntypes nlocal nghost natoms
//   xprd yprd zprd boxlo_x boxlo_y boxlo_z
//   g_ewald accuracy slab_volfactor slabflag nx_pppm ny_pppm nz_pppm order      (mesh 0 0 0 0 = not a PPPM style)
//   qqrd2e qqr2e qe2f dielectric newton_pair cut_coul
//   cutsq[(ntypes+1)^2]
//   ngroups  { name bit } ...
//   per atom (nlocal + nghost): tag type mask q x y z
//   nlists   { inum  { i numneigh j... } ... } ...      list 0 = only / ele-ele list, list 1 = ele-electrolyte list
//   variable: name value   ("-" = none)
//   nmodify { ntok tok... } ...                          fix_modify lines
//   narg tok...                                          the fix command
//   nsteps { ntimestep potdiff_value reneighbor(0/1) has_x(0/1) [x y z per atom] } ...
//   optional, read by the `pair` mode only:  "pair" cut_coul  cutsq cut_ljsq lj1 lj2 lj3 lj4 offset [(ntypes+1)^2 each]
//                                            special_lj[4] special_coul[4]
// output (stdout): "scalar STEP VALUE", "q STEP TAG VALUE" for owned electrode atoms, "f STEP ..." sums, "ERROR: msg" + exit 2.
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <algorithm>
#include <vector>

#define CONP_GLUE_MOCK 1
#include "compute_potential_atom_hip.h"
#include "ewald_conp_hip.h"
#include "fix_conp_hip.h"
#include "kspacemodule_hip.h"
#include "pair_lj_cut_coul_long_conp_hip.h"
#include "pppm_conp_hip.h"

using namespace LAMMPS_NS;

namespace {

struct Out {
  std::string text;
  void f(const char *fmt, ...) {
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    text += line;
  }
};

// one rank: its own mock LAMMPS instance, atoms and lists from its case file
static bool g_kspace_vatom = false;   // `... kspace vatom`: compute() is asked for the per-atom virial too, "kva" lines follow
static bool g_kspace = false;    // `glue_driver CASEFILE kspace`: EwaldConpHip is the kspace style, compute() on every step
static bool g_pppmforce = false; // `glue_driver CASEFILE pppmforce`: PPPMConpHip in device mode is the kspace style, compute() on every step
static std::string g_pppm_variant; // its third word
static bool g_pppmhost = false;  // `glue_driver CASEFILE pppmhost`
static bool g_pair = false;      // `glue_driver CASEFILE pair`: PairLJCutCoulLongConpHip is the pair style, compute() on every step
static std::string g_pair_variant; // its third word
static bool g_compute = false;   // `glue_driver CASEFILE compute`: after the steps, compute potential/atom/hip on the conp/hip fix

int run_case(const char *path, bool provider, int me, int nprocs, MockCommRank *world, Out &out) {
  std::ifstream in(path);
  if (!in) { out.f("ERROR: cannot open %s\n", path); return 1; }

  LAMMPS lmp{};
  Memory memory; Error error; Atom atom{}; Force force{}; Domain domain{}; Update update{}; Comm comm{}; Group group{};
  Variable variable; Input input{}; Neighbor neighbor{}; Modify modify; KSpace kspace(&lmp); Pair pair(&lmp);
  lmp.world = world;
  lmp.memory = &memory; lmp.error = &error; lmp.atom = &atom; lmp.force = &force; lmp.domain = &domain; lmp.update = &update;
  lmp.comm = &comm; lmp.group = &group; lmp.input = &input; lmp.neighbor = &neighbor; lmp.modify = &modify;
  lmp.screen = me == 0 ? stdout : nullptr; lmp.logfile = nullptr;
  input.variable = &variable;
  force.kspace = &kspace; force.pair = &pair;
  comm.me = me; comm.nprocs = nprocs;
  char style[] = "verlet";
  update.integrate_style = style;

  int ntypes, nlocal, nghost;
  long natoms;
  in >> ntypes >> nlocal >> nghost >> natoms;
  const int nall = nlocal + nghost;
  in >> domain.xprd >> domain.yprd >> domain.zprd >> domain.boxlo[0] >> domain.boxlo[1] >> domain.boxlo[2];
  domain.zprd_half = 0.5 * domain.zprd;
  in >> kspace.g_ewald >> kspace.accuracy >> kspace.slab_volfactor >> kspace.slabflag >> kspace.nx_pppm >> kspace.ny_pppm >>
      kspace.nz_pppm >> kspace.order;
  kspace.energy = 0.0;
  in >> force.qqrd2e >> force.qqr2e >> force.qe2f >> force.dielectric >> force.newton_pair >> pair.cut_coul;
  const int nt1 = ntypes + 1;
  std::vector<double> cutsq_store((size_t)nt1 * nt1);
  std::vector<double *> cutsq_rows(nt1);
  for (auto &v : cutsq_store) in >> v;
  for (int i = 0; i < nt1; ++i) cutsq_rows[i] = cutsq_store.data() + (size_t)i * nt1;
  pair.cutsq = cutsq_rows.data();
  pair.eng_coul = 0.0;
  for (double &v : pair.virial) v = 0.0;

  int ngroups;
  in >> ngroups;
  std::vector<int> bitmask(32, 0);
  group.bitmask = bitmask.data();
  group.ngroup = ngroups;
  for (int g = 0; g < ngroups; ++g) in >> group.names[g] >> bitmask[g];

  std::vector<int> tag(nall), type(nall), mask(nall);
  std::vector<double> q(nall), xs((size_t)nall * 3), fs((size_t)nall * 3, 0.0);
  std::vector<double *> xrows(nall), frows(nall);
  int maxtag = 0;
  for (int i = 0; i < nall; ++i) {
    in >> tag[i] >> type[i] >> mask[i] >> q[i] >> xs[3 * (size_t)i] >> xs[3 * (size_t)i + 1] >> xs[3 * (size_t)i + 2];
    xrows[i] = &xs[3 * (size_t)i]; frows[i] = &fs[3 * (size_t)i];
    if (tag[i] > maxtag) maxtag = tag[i];
  }
  std::vector<int> map_array(maxtag + 1, -1);
  for (int i = nall - 1; i >= 0; --i) map_array[tag[i]] = i;      // owned atoms win over their ghosts, like Atom::map
  atom.nlocal = nlocal; atom.nghost = nghost; atom.ntypes = ntypes; atom.natoms = natoms;
  atom.x = xrows.data(); atom.f = frows.data(); atom.q = q.data(); atom.type = type.data(); atom.mask = mask.data();
  atom.tag = tag.data(); atom.map_array = map_array.data(); atom.map_size = maxtag + 1;

  int nlists;
  in >> nlists;
  struct ListStore { std::vector<int> ilist, numneigh, neigh; std::vector<size_t> first; std::vector<int *> firstneigh; NeighList nl{}; };
  std::vector<ListStore> lists(nlists);
  for (auto &L : lists) {
    int inum;
    in >> inum;
    L.numneigh.assign(nall, 0); L.first.assign(nall, 0);
    for (int ii = 0; ii < inum; ++ii) {
      int i, n;
      in >> i >> n;
      L.ilist.push_back(i); L.numneigh[i] = n; L.first[i] = L.neigh.size();
      for (int k = 0; k < n; ++k) { int j; in >> j; L.neigh.push_back(j); }
    }
    if (L.neigh.empty()) L.neigh.push_back(0);
    L.firstneigh.assign(nall, L.neigh.data());
    for (int i = 0; i < nall; ++i) L.firstneigh[i] = L.neigh.data() + L.first[i];
    L.nl.inum = inum; L.nl.ilist = L.ilist.data(); L.nl.numneigh = L.numneigh.data(); L.nl.firstneigh = L.firstneigh.data();
  }

  std::string vname;
  double vvalue;
  in >> vname >> vvalue;
  if (vname != "-") { variable.name = vname; variable.value = vvalue; }

  int nmodify;
  in >> nmodify;
  std::vector<std::vector<std::string>> modify_lines(nmodify);
  for (auto &ml : modify_lines) { int n; in >> n; ml.resize(n); for (auto &t : ml) in >> t; }

  int narg;
  in >> narg;
  std::vector<std::string> toks(narg);
  for (auto &t : toks) in >> t;
  std::vector<char *> fargv;
  for (auto &t : toks) fargv.push_back(const_cast<char *>(t.c_str()));

  std::vector<NeighRequest *> requests(8, nullptr);
  neighbor.requests = requests.data();

  if (provider) {
    // Mode B.  What FixConp::linalg_init / post_neighbor do around the provider (fix_conp.cpp:401-416, 468-539), with a stand-in
    // that carries the fix's PUBLIC members: the index maps are made the way the fix makes them (one more handle serves as the
    // fix's bookkeeping here; in a LAMMPS tree the reference's own FixConp fills them).
    auto must = [&](int rc) { if (rc != CONP_OK) throw std::runtime_error(conp_last_error()); };
    conp_fix_args fa;
    std::vector<const char *> cargv;
    for (auto &t : toks) cargv.push_back(t.c_str());
    must(conp_parse_fix_args(narg, cargv.data(), ntypes, &fa));
    const int gb = bitmask[group.find(toks[1])], jgb = bitmask[group.find(toks[4])];
    FixConp fixstub(&lmp);
    fixstub.eta = fa.eta;
    fixstub.check = [&](int i) { return (mask[i] & gb) ? 1 : ((mask[i] & jgb) ? -1 : 0); };
    // the fix's own maps: FixConp::post_neighbor's algorithm (conp_host_index restates it bit-exactly; one rank here -- in the
    // `ranks` mode the stand-in's numbering comes from a bookkeeping handle that talks to the other ranks)
    conp_env env;
    std::memset(&env, 0, sizeof(env));
    env.qqrd2e = force.qqrd2e; env.qqr2e = force.qqr2e; env.qe2f = force.qe2f; env.dielectric = force.dielectric;
    env.newton_pair = force.newton_pair; env.g_ewald = kspace.g_ewald; env.accuracy = kspace.accuracy;
    env.slab_volfactor = kspace.slab_volfactor; env.slabflag = kspace.slabflag;
    env.xprd = domain.xprd; env.yprd = domain.yprd; env.zprd = domain.zprd;
    env.boxlo_x = domain.boxlo[0]; env.boxlo_y = domain.boxlo[1]; env.boxlo_z = domain.boxlo[2];
    env.ntypes = ntypes; env.cutsq = cutsq_store.data(); env.cut_coul = pair.cut_coul; env.nranks = nprocs; env.rank = me;
    env.pppm_nx = kspace.nx_pppm; env.pppm_ny = kspace.ny_pppm; env.pppm_nz = kspace.nz_pppm; env.pppm_order = kspace.order;
    conp_fix *book = nullptr;
    must(conp_fix_create(&fa, &env, &book));
    // (the bookkeeping handle of a multi-rank run would need the comm too; the provider test with ranks uses FixConpHip instead)
    std::vector<std::vector<int>> firsts(nlists);
    for (int l = 0; l < nlists; ++l) {
      ListStore &L = lists[l];
      firsts[l].assign(L.first.begin(), L.first.end());
      conp_neighlist v;
      v.inum = L.nl.inum; v.ilist = L.ilist.data(); v.numneigh = L.numneigh.data(); v.first = firsts[l].data();
      v.neigh = L.neigh.data(); v.nneigh = (int64_t)L.neigh.size();
      must(conp_fix_init_list(book, nlists == 1 ? 2 : l, &v));
    }
    std::vector<int> ec(nall);
    for (int i = 0; i < nall; ++i) ec[i] = fixstub.check(i);
    conp_atoms a;
    a.nlocal = nlocal; a.nghost = nghost; a.x = xs.data(); a.q = q.data(); a.type = type.data(); a.tag = tag.data();
    a.echeck = ec.data();
    must(conp_fix_setup_post_neighbor(book, &a));
    conp_info info;
    must(conp_fix_info(book, &info));
    std::vector<int> ele2tag(info.elenum), ele2eleall(info.elenum), eleall2tag(info.elenum_all), eleall2ele(info.elenum_all + 1),
        echk(info.elenum_all), ebuf(info.elenum_all), tag2eleall(info.maxtag_all + 1);
    must(conp_fix_get_maps(book, ele2tag.data(), ele2eleall.data(), eleall2tag.data(), eleall2ele.data(), echk.data(), ebuf.data(),
                           tag2eleall.data()));
    conp_fix_destroy(book);
    fixstub.elenum = info.elenum; fixstub.elenum_all = info.elenum_all; fixstub.elytenum = info.elytenum;
    fixstub.ele2tag = ele2tag.data(); fixstub.ele2eleall = ele2eleall.data(); fixstub.eleall2tag = eleall2tag.data();
    fixstub.tag2eleall = tag2eleall.data();
    // fix_conp.cpp:401-410: with the `pppm` keyword the provider IS the kspace style, found by dynamic_cast; else
    // kspmod = new ...(lmp); then kspmod->register_fix(this); kspmod->conp_setup(lowmemflag);
    KSpaceModule *kspmod = nullptr;
    PPPMConpHip *pppm_style = nullptr;
    if (fa.pppm) {
      pppm_style = new PPPMConpHip(&lmp);                       // what `kspace_style pppm/conp/hip` creates
      pppm_style->g_ewald = kspace.g_ewald; pppm_style->accuracy = kspace.accuracy; pppm_style->slab_volfactor = kspace.slab_volfactor;
      pppm_style->slabflag = kspace.slabflag; pppm_style->energy = 0.0;
      pppm_style->nx_pppm = kspace.nx_pppm; pppm_style->ny_pppm = kspace.ny_pppm; pppm_style->nz_pppm = kspace.nz_pppm;
      pppm_style->order = kspace.order;
      if (g_pppmhost) {
        char acc[] = "1e-4";
        char *sargv[1] = {acc};
        pppm_style->settings(1, sargv);
        if (pppm_style->device_compute()) throw std::runtime_error("pppm/conp/hip without `device` selected the device compute()");
      }
      force.kspace = pppm_style;
      kspmod = dynamic_cast<KSpaceModule *>(force.kspace);      // fix_conp.cpp:402
      if (kspmod == nullptr) throw std::runtime_error("Fix conp couldn't detect a pppm/conp kspace style (which is required with the pppm flag)");
    } else kspmod = new KSpaceModuleHip(&lmp);
    fixstub.kspmod = kspmod;
    kspmod->register_fix(&fixstub);
    kspmod->conp_setup(true);
    kspmod->conp_post_neighbor(true, true);        // fix_conp.cpp:538
    kspmod->a_read();                              // km_ewald.cpp:147-151 a_cal calls a_read first
    std::vector<double> aaa((size_t)info.elenum * info.elenum_all, 0.0), bbb(info.elenum, 0.0);
    kspmod->a_cal(aaa.data());
    kspmod->b_cal(bbb.data());
    for (int i = 0; i < info.elenum; ++i) {
      out.f("b %d %.17g\n", i, bbb[i]);
      for (int j = 0; j < info.elenum_all; ++j) out.f("a %d %d %.17g\n", i, j, aaa[(size_t)i * info.elenum_all + j]);
    }
    for (int i = 0; i < info.elenum; ++i) out.f("m %d %d\n", i, ele2eleall[i]);
    if (pppm_style) {
      // the step goes on: FixConp::update_charge has written the electrode charges, then LAMMPS calls force->kspace->compute() --
      // PPPM::compute's particle_map() / make_rho() are the provider's overrides (pppm_conp.cpp:428-450).  What the base class is
      // handed, how often the base's own steps ran, and whether the library spread the electrolyte a second time:
      conp_info i0, i1;
      must(conp_fix_info(pppm_style->handle(), &i0));
      pppm_style->compute(1, 0);
      must(conp_fix_info(pppm_style->handle(), &i1));
      out.f("rho_calls %d %d spreads %d %d\n", pppm_style->base_particle_map_calls, pppm_style->base_make_rho_calls, i0.pppm_elyte_spreads,
            i1.pppm_elyte_spreads);
      if (const char *rp = std::getenv("GLUE_RHO_OUT")) {
        std::ofstream rf(rp, std::ios::binary);
        rf.write(reinterpret_cast<const char *>(pppm_style->density_fft.data()), (std::streamsize)(pppm_style->density_fft.size() * sizeof(double)));
      }
      kspmod->conp_pre_force();                      // next step (pppm_conp.h:42): the kept brick is dropped ...
      std::vector<double> bbb2(info.elenum, 0.0);
      kspmod->b_cal(bbb2.data());                    // ... and b_cal makes this step's
      double dmax = 0.0;
      for (int i = 0; i < info.elenum; ++i) dmax = std::max(dmax, std::abs(bbb2[i] - bbb[i]));
      out.f("b_again %.17g\n", dmax);
    }
    if (pppm_style) {      // what ComputePotentialAtom asks of the provider (compute_potential_atom.cpp:165-175), group 1 = eleleft
      std::vector<double> recv(nlocal, 0.0);
      kspmod->compute_group_potential(gb, recv.data());
      for (int i = 0; i < nlocal; ++i) if (mask[i] & gb) out.f("u %d %.17g\n", tag[i], recv[i]);
      int i0 = 0;
      while (i0 < nlocal && !(mask[i0] & gb)) ++i0;
      out.f("up %d %.17g\n", tag[i0], kspmod->compute_particle_potential(i0));
      force.kspace = &kspace;
      delete pppm_style;                           // LAMMPS deletes its kspace style, not the fix (fix_conp.cpp:207)
    } else {
      // the Ewald provider's potentials (exact k sums, conp_ewald_*), group 1 = eleleft, at the charges the atoms carry
      std::vector<double> recv(nlocal, 0.0);
      kspmod->compute_group_potential(gb, recv.data());
      for (int i = 0; i < nlocal; ++i) if (mask[i] & gb) out.f("u %d %.17g\n", tag[i], recv[i]);
      for (int i = 0; i < nlocal; ++i) out.f("up %d %.17g\n", tag[i], kspmod->compute_particle_potential(i));
      // `compute pot all potential/atom/hip kspace`: no pppm style, so setup() finds the provider's handle through the fix list
      // (Modify::fix -> FixConp::kspmod -> KSpaceModuleHip) and the compute runs on the exact Ewald sums
      Fix *fixes[1] = {&fixstub};
      modify.fix = fixes; modify.nfix = 1;
      std::vector<std::string> ctoks = {"pot", "all", "potential/atom/hip", "kspace"};
      std::vector<char *> cargv;
      for (auto &t : ctoks) cargv.push_back(const_cast<char *>(t.c_str()));
      atom.nmax = std::max(atom.nmax, nall);
      update.eflag_atom = update.ntimestep;                     // (per-atom energy tallied on this step, :121-123)
      {
        ComputePotentialAtomHip cpa(&lmp, (int)cargv.size(), cargv.data());
        cpa.setup();
        cpa.compute_peratom();
        for (int i = 0; i < nlocal; ++i) out.f("cp %d %.17g\n", tag[i], cpa.vector_atom[i]);
      }
      modify.nfix = 0; modify.fix = nullptr;
      delete kspmod;                               // fix_conp.cpp:207: the fix deletes its Ewald provider; the handle goes with it
    }
    return 0;
  }

  // `kspace_style ewald/conp/hip 1e-6` + `kspace_modify gewald G force A slab S`: the style object is force->kspace before any init()
  // runs, its own init() comes before the fixes' (LAMMPS::init: force->init(), then modify->init()), and FixConpHip::init reads
  // g_ewald & co. from it
  std::unique_ptr<EwaldConpHip> ew;
  if (g_kspace) {
    ew.reset(new EwaldConpHip(&lmp));
    char acc[] = "1e-6";
    char *sargv[1] = {acc};
    ew->settings(1, sargv);
    ew->g_ewald = kspace.g_ewald; ew->accuracy_absolute = kspace.accuracy; ew->two_charge_force = force.qqr2e;
    ew->slab_volfactor = kspace.slab_volfactor; ew->slabflag = kspace.slabflag; ew->energy = 0.0;
    force.kspace = ew.get();
    ew->init();
  }
  // `kspace_style pppm/conp/hip 1e-4 device`: the mesh is what PPPM::init would have chosen (the case file's); FixConpHip::init reads
  // it off force->kspace
  std::unique_ptr<PPPMConpHip> pf;
  if (g_pppmforce) {
    pf.reset(new PPPMConpHip(&lmp));
    char acc[] = "1e-4", dev[] = "device";
    char *sargv[2] = {acc, dev};
    pf->settings(2, sargv);
    pf->g_ewald = kspace.g_ewald; pf->accuracy = kspace.accuracy; pf->slab_volfactor = kspace.slab_volfactor;
    pf->slabflag = kspace.slabflag; pf->energy = 0.0;
    pf->nx_pppm = kspace.nx_pppm; pf->ny_pppm = kspace.ny_pppm; pf->nz_pppm = kspace.nz_pppm; pf->order = kspace.order;
    if (g_pppm_variant == "ad") pf->differentiation_flag = 1;
    force.kspace = pf.get();
  }
  FixConpHip fix(&lmp, narg, fargv.data());
  Fix *fixes[1] = {&fix};
  if (g_pppmforce) { atom.nmax = std::max(atom.nmax, nall); if (g_pppm_variant != "nohandle") { modify.fix = fixes; modify.nfix = 1; } }
  if (g_kspace) { modify.fix = fixes; modify.nfix = 1; atom.nmax = std::max(atom.nmax, nall); }
  for (auto &ml : modify_lines) {                    // fix_modify arrives before init(), as in an input script
    std::vector<char *> margv;
    for (auto &t : ml) margv.push_back(const_cast<char *>(t.c_str()));
    const int used = fix.modify_param((int)margv.size(), margv.data());
    if (used == 0) throw std::runtime_error("Illegal fix_modify command");
  }
  fix.init();
  // Neighbor::init hands every request its list (Neighbor::init -> Fix::init_list); an occasional skip list is the
  // ele-ele list (list 0), the perpetual one the ele-electrolyte list (last list)
  for (int r = 0; r < neighbor.nrequest; ++r) {
    const bool occasional = requests[r]->occasional != 0;
    ListStore &L = (neighbor.nrequest == 1 || occasional) ? lists.front() : lists.back();
    L.nl.index = r; L.nl.occasional = requests[r]->occasional;
    fix.init_list(0, &L.nl);
  }
  update.ntimestep = 0;
  int nsteps;
  in >> nsteps;
  struct Step { long ts; double pd; int reneigh, has_x; std::vector<double> x; };
  std::vector<Step> steps(nsteps);
  for (auto &st : steps) {
    in >> st.ts >> st.pd >> st.reneigh >> st.has_x;
    if (st.has_x) { st.x.resize(xs.size()); for (double &v : st.x) in >> v; }
  }
  // `pair_style lj/cut/coul/long/conp/hip` + pair_coeff + `pair_modify table 0` + special_bonds: the tables init_one() would leave
  // in the base class come from the case file's optional block; the style's list is the generic half list (list 0)
  std::unique_ptr<PairLJCutCoulLongConpHip> ps;
  if (g_pair) {
    std::string word;
    in >> word;
    if (word != "pair") throw std::runtime_error("the pair mode needs the case file's pair block");
    ps.reset(new PairLJCutCoulLongConpHip(&lmp));
    ps->mock_allocate(ntypes);
    in >> ps->cut_coul;
    for (int k = 0; k < 7; ++k)
      for (int i = 0; i < nt1; ++i)
        for (int j = 0; j < nt1; ++j) in >> ps->mock_table(k)[i][j];
    for (double &v : force.special_lj) in >> v;
    for (double &v : force.special_coul) in >> v;
    if (!in) throw std::runtime_error("the case file's pair block is short");
    ps->ncoultablebits = g_pair_variant == "table" ? 12 : 0;
    ps->list = &lists.front().nl;
    force.pair = ps.get();
    modify.fix = fixes; modify.nfix = 1; atom.nmax = std::max(atom.nmax, nall);
  }
  // Verlet::setup order: modify->setup_post_neighbor(), then modify->setup_pre_force()
  bool first = true;
  for (int s = 0; s < nsteps; ++s) {
    const long ts = steps[s].ts; const double pd = steps[s].pd; const int reneigh = steps[s].reneigh;
    if (steps[s].has_x) std::copy(steps[s].x.begin(), steps[s].x.end(), xs.begin());
    neighbor.ago = (first || reneigh) ? 0 : neighbor.ago + 1;      // Neighbor::decide / build: 0 on a step that rebuilt the lists
    if (first || reneigh) ++neighbor.ncalls;
    update.ntimestep = ts; update.laststep = -1;
    if (s == nsteps - 1) update.laststep = ts;
    variable.value = pd;
    if (first) {
      fix.setup_post_neighbor();
      fix.setup_pre_force(0);
      first = false;
    } else {
      if (reneigh) { fix.pre_exchange(); fix.post_neighbor(); }      // Verlet::run: pre_exchange ... neighbor->build ... post_neighbor
      fix.pre_force(0);
    }
    if (g_kspace) {
      // what Verlet does after the fixes' pre_force, on EVERY step, whether or not the fix updated the charges on it:
      // force->kspace->compute(eflag, vflag), here with the global and per-atom energy and the global virial; atom->f starts from zero
      std::fill(fs.begin(), fs.end(), 0.0);
      ew->compute(3, g_kspace_vatom ? 5 : 1);
      for (int i = 0; i < nlocal; ++i) {
        out.f("kf %ld %d %.17g %.17g %.17g\n", ts, tag[i], fs[3 * (size_t)i], fs[3 * (size_t)i + 1], fs[3 * (size_t)i + 2]);
        out.f("kea %ld %d %.17g\n", ts, tag[i], ew->eatom[i]);
      }
      if (g_kspace_vatom)
        for (int i = 0; i < nlocal; ++i)
          out.f("kva %ld %d %.17g %.17g %.17g %.17g %.17g %.17g\n", ts, tag[i], ew->vatom[i][0], ew->vatom[i][1], ew->vatom[i][2],
                ew->vatom[i][3], ew->vatom[i][4], ew->vatom[i][5]);
      out.f("ke %ld %.17g\n", ts, ew->energy);
      out.f("kv %ld %.17g %.17g %.17g %.17g %.17g %.17g\n", ts, ew->virial[0], ew->virial[1], ew->virial[2], ew->virial[3], ew->virial[4],
            ew->virial[5]);
    }
    if (g_pair) {
      // Verlet after the fixes' pre_force: force_clear(), then force->pair->compute(eflag, vflag)
      std::fill(fs.begin(), fs.end(), 0.0);
      const bool va = g_pair_variant == "vatom";
      ps->compute(3, va ? 5 : 1);
      for (int i = 0; i < nall; ++i) {
        out.f("pf %ld %d %.17g %.17g %.17g\n", ts, i, fs[3 * (size_t)i], fs[3 * (size_t)i + 1], fs[3 * (size_t)i + 2]);
        out.f("pea %ld %d %.17g\n", ts, i, ps->eatom[i]);
        if (va)
          out.f("pva %ld %d %.17g %.17g %.17g %.17g %.17g %.17g\n", ts, i, ps->vatom[i][0], ps->vatom[i][1], ps->vatom[i][2],
                ps->vatom[i][3], ps->vatom[i][4], ps->vatom[i][5]);
      }
      out.f("pe %ld %.17g %.17g\n", ts, ps->eng_vdwl, ps->eng_coul);
      out.f("pv %ld %.17g %.17g %.17g %.17g %.17g %.17g\n", ts, ps->virial[0], ps->virial[1], ps->virial[2], ps->virial[3],
            ps->virial[4], ps->virial[5]);
      out.f("pls %ld %d\n", ts, ps->list_uploads());
    }
    if (g_pppmforce) {
      // Verlet after the fixes' pre_force, on every step: force->kspace->compute(eflag, vflag); atom->f starts from zero
      std::fill(fs.begin(), fs.end(), 0.0);
      pf->compute(3, g_pppm_variant == "vatom" ? 5 : 1);
      for (int i = 0; i < nlocal; ++i) {
        out.f("kf %ld %d %.17g %.17g %.17g\n", ts, tag[i], fs[3 * (size_t)i], fs[3 * (size_t)i + 1], fs[3 * (size_t)i + 2]);
        out.f("kea %ld %d %.17g\n", ts, tag[i], pf->eatom[i]);
      }
      out.f("ke %ld %.17g\n", ts, pf->energy);
      out.f("kv %ld %.17g %.17g %.17g %.17g %.17g %.17g\n", ts, pf->virial[0], pf->virial[1], pf->virial[2], pf->virial[3], pf->virial[4],
            pf->virial[5]);
    }
    std::fill(fs.begin(), fs.end(), 0.0);
    if (fix.setmask() & FixConst::POST_FORCE) fix.post_force(0);
    fix.end_of_step();
    out.f("scalar %ld %.17g\n", ts, fix.compute_scalar());
    for (int i = 0; i < nlocal; ++i)
      if (mask[i] & (fix.groupbit | bitmask[group.find(toks[4])])) out.f("q %ld %d %.17g\n", ts, tag[i], q[i]);
    double fsum[3] = {0, 0, 0}, fabs_ = 0;
    for (int i = 0; i < nlocal; ++i) for (int c = 0; c < 3; ++c) { fsum[c] += fs[3 * (size_t)i + c]; fabs_ += std::abs(fs[3 * (size_t)i + c]); }
    out.f("f %ld %.17g %.17g %.17g %.17g eng_coul %.17g kspace_energy %.17g\n", ts, fsum[0], fsum[1], fsum[2], fabs_,
          force.pair->eng_coul, kspace.energy);
  }
  if (g_compute) {
    // `compute pot all potential/atom/hip kspace` without a pppm style: setup() takes the conp/hip fix's handle (Modify::fix)
    Fix *fixes[1] = {&fix};
    modify.fix = fixes; modify.nfix = 1;
    std::vector<std::string> ctoks = {"pot", "all", "potential/atom/hip", "kspace"};
    std::vector<char *> cargv;
    for (auto &t : ctoks) cargv.push_back(const_cast<char *>(t.c_str()));
    atom.nmax = std::max(atom.nmax, nall);
    update.eflag_atom = update.ntimestep;
    {
      ComputePotentialAtomHip cpa(&lmp, (int)cargv.size(), cargv.data());
      cpa.setup();
      cpa.compute_peratom();
      for (int i = 0; i < nlocal; ++i) out.f("cp %d %.17g\n", tag[i], cpa.vector_atom[i]);
    }
    modify.nfix = 0; modify.fix = nullptr;
  }
  // GLUE_DRIVER_TIME=N: wall time of N more pre_force calls -- the PCIe-inclusive rate a LAMMPS run would see through the glue
  if (const char *tn = std::getenv("GLUE_DRIVER_TIME")) {
    const int n = std::atoi(tn);
    for (int k = 0; k < 3; ++k) { update.ntimestep += 1; fix.pre_force(0); }
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < n; ++k) { update.ntimestep += 1; fix.pre_force(0); }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (n > 0 ? n : 1);
    out.f("time_pre_force_ms %.6f\n", ms);
    const auto t1 = std::chrono::steady_clock::now();
    for (int k = 0; k < n; ++k) { std::fill(fs.begin(), fs.end(), 0.0); fix.post_force(0); }      // same step as the last pre_force
    const double ms2 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() / (n > 0 ? n : 1);
    out.f("time_post_force_ms %.6f\n", ms2);
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: glue_driver CASEFILE [provider] | glue_driver ranks N CASE_0 .. CASE_N-1\n"); return 1; }
  if (std::string(argv[1]) == "ranks") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 0;
    if (n < 1 || argc < 3 + n) { std::fprintf(stderr, "glue_driver ranks N needs N case files\n"); return 1; }
    const bool provider = argc > 3 + n && std::string(argv[3 + n]) == "provider";
    MockWorld world(n);
    std::vector<MockCommRank> ranks(n);
    std::vector<Out> outs(n);
    std::vector<int> rcs(n, 0);
    std::vector<std::thread> threads;
    for (int r = 0; r < n; ++r) {
      ranks[r] = MockCommRank{&world, r};
      threads.emplace_back([&, r] {
        try {
          rcs[r] = run_case(argv[3 + r], provider, r, n, &ranks[r], outs[r]);
        } catch (const std::exception &e) {
          outs[r].f("ERROR: %s\n", e.what());
          rcs[r] = 2;
          world.fail();                      // the other ranks sit in a collective: wake them, they fail too
        }
      });
    }
    for (auto &t : threads) t.join();
    int rc = 0;
    for (int r = 0; r < n; ++r) {
      size_t pos = 0;
      while (pos < outs[r].text.size()) {
        const size_t e = outs[r].text.find('\n', pos);
        const std::string line = outs[r].text.substr(pos, e == std::string::npos ? std::string::npos : e - pos);
        std::printf("rank %d %s\n", r, line.c_str());
        if (e == std::string::npos) break;
        pos = e + 1;
      }
      if (rcs[r]) rc = rcs[r];
    }
    return rc;
  }
  Out out;
  int rc = 0;
  try {
    MockCommRank *single = nullptr;
    g_compute = argc > 2 && std::string(argv[2]) == "compute";
    g_kspace = argc > 2 && std::string(argv[2]) == "kspace";
    g_kspace_vatom = g_kspace && argc > 3 && std::string(argv[3]) == "vatom";
    g_pppmforce = argc > 2 && std::string(argv[2]) == "pppmforce";
    g_pppm_variant = g_pppmforce && argc > 3 ? argv[3] : "";
    g_pppmhost = argc > 2 && std::string(argv[2]) == "pppmhost";
    g_pair = argc > 2 && std::string(argv[2]) == "pair";
    g_pair_variant = g_pair && argc > 3 ? argv[3] : "";
    rc = run_case(argv[1], argc > 2 && (std::string(argv[2]) == "provider" || g_pppmhost), 0, 1, single, out);
  } catch (const std::exception &e) {
    out.f("ERROR: %s\n", e.what());
    rc = 2;
  }
  std::fputs(out.text.c_str(), stdout);
  return rc;
}
