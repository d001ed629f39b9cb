// INTERFACE MOCK -- NOT LAMMPS.  Declares just enough of the LAMMPS 27May2021 class surface for the glue in this directory:
// `make check` type-checks the glue against it, and mock_runtime.cpp gives the declarations minimal bodies so that
// glue_driver.cpp can drive FixConpHip through the same hook sequence LAMMPS' Modify / Verlet use (tests/test_gpu_glue.py).
// LAMMPS itself is not in the build image; against a real LAMMPS tree the glue includes the real headers instead
// (INTEGRATION.md).  This is a test host for OUR glue, not a way to build the reference.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mpi_mock.h"

#define FLERR __FILE__, __LINE__
#define NEIGHMASK 0x3FFFFFFF

namespace LAMMPS_NS {
typedef int tagint;
typedef int64_t bigint;

class Error { public: [[noreturn]] void all(const char *, int, const std::string &); [[noreturn]] void one(const char *, int, const std::string &); void warning(const char *, int, const std::string &); };
class Memory {};
class Atom { public: int nlocal, nghost, ntypes, nmax = 0; bigint natoms; double **x, **f, *q; int *type, *mask, *molecule = nullptr; tagint *tag; int map(tagint);
             int *map_array = nullptr; int map_size = 0; };
class KSpace;
class NeighList;
class Pair;
class Force { public: double qqrd2e, qqr2e, qe2f, dielectric; int newton_pair, newton = 0; KSpace *kspace; Pair *pair;
              double special_lj[4] = {1.0, 1.0, 1.0, 1.0}, special_coul[4] = {1.0, 1.0, 1.0, 1.0};   // special_bonds (force.h), [0] is 1.0
              Pair *pair_match(const std::string &, int, int nsub = 0); };
class Domain { public: double xprd, yprd, zprd, zprd_half, boxlo[3]; int triclinic = 0; };
class Update { public: bigint ntimestep, laststep, eflag_atom = 0; char *integrate_style; };
class Comm { public: int me, nprocs; };
class Group { public: int *bitmask; int find(const std::string &); int ngroup = 0; std::string names[32]; };
class Variable { public: int find(const char *); int equalstyle(int); double compute_equal(int);
                 std::string name; double value = 0.0; };   // the mock knows one equal-style variable
class Input { public: Variable *variable; };
class NeighRequest { public: int pair, fix, half, full, occasional, skip, intel; int *iskip, **ijskip; };
class NeighList { public: int index, inum, occasional; int *ilist, *numneigh, **firstneigh; };
class Neighbor { public: NeighRequest **requests; int nrequest = 0;
                 int ago = 0; bigint ncalls = 0;   // steps since the last build (0 on a re-neighbouring step) and the number of builds (neighbor.h)
                 int request(void *, int instance = 0); void build(int); void build_one(NeighList *, int preflag = 0); };
class Fix;
class Modify { public: int find_fix(const std::string &); int nfix = 0; Fix **fix = nullptr; };   // (Modify::fix / nfix, modify.h)

class LAMMPS { public: MPI_Comm world = nullptr; Memory *memory; Error *error; Atom *atom; Force *force; Domain *domain; Update *update; Comm *comm; Group *group; Input *input; Neighbor *neighbor; Modify *modify; FILE *screen, *logfile; };

class Pointers {
 public:
  explicit Pointers(LAMMPS *ptr)
      : lmp(ptr), world(ptr->world), memory(ptr->memory), error(ptr->error), atom(ptr->atom), force(ptr->force), domain(ptr->domain),
        update(ptr->update), comm(ptr->comm), group(ptr->group), input(ptr->input), neighbor(ptr->neighbor),
        modify(ptr->modify), screen(ptr->screen), logfile(ptr->logfile) {}
  virtual ~Pointers() {}
 protected:
  LAMMPS *lmp; MPI_Comm &world; Memory *&memory; Error *&error; Atom *&atom; Force *&force; Domain *&domain; Update *&update; Comm *&comm;
  Group *&group; Input *&input; Neighbor *&neighbor; Modify *&modify; FILE *&screen; FILE *&logfile;
};

// Pair (pair.h) as far as the glue touches it: what the fix reads (cutsq, extract("cut_coul"), the accumulators it adds its
// post-force correction to) and what a pair style's compute() fills after ev_init() has decoded eflag / vflag like KSpace's:
// eng_vdwl, eng_coul, virial (zeroed by ev_init), eatom [nmax], vatom [nmax][6] (one contiguous block behind row pointers, zeroed).
class Pair : protected Pointers {
 public:
  explicit Pair(LAMMPS *l) : Pointers(l) {}
  virtual ~Pair() {}
  double **cutsq = nullptr;
  double eng_vdwl = 0.0, eng_coul = 0.0, virial[6] = {0, 0, 0, 0, 0, 0};
  double *eatom = nullptr, **vatom = nullptr;
  double cut_coul = 0.0;
  int ncoultablebits = 12;                       // pair_modify table N (pair.h; LAMMPS' default is 12, `table 0` switches tables off)
  int no_virial_fdotr = 0;
  int evflag = 0, eflag_either = 0, eflag_global = 0, eflag_atom = 0, vflag_either = 0, vflag_global = 0, vflag_atom = 0, vflag_fdotr = 0;
  NeighList *list = nullptr;
  virtual void compute(int, int) {}
  virtual void *extract(const char *, int &);
  void ev_tally(int, int, int, int, double, double, double, double, double, double);
 protected:
  void ev_init(int eflag, int vflag);
 private:
  std::vector<double> eatom_store, vatom_store;
  std::vector<double *> vatom_rows;
};

// LAMMPS' PairLJCutCoulLong (pair_lj_cut_coul_long.h) as far as the conp/hip style reads it: the per-type-pair tables init_one()
// leaves behind ([ntypes + 1][ntypes + 1] behind row pointers) and cut_coul.  compute() is the CPU pair loop in LAMMPS; the mock
// only counts its calls.  mock_allocate() stands for allocate(): it makes the tables, the test host fills them.
class PairLJCutCoulLong : public Pair {
 public:
  explicit PairLJCutCoulLong(LAMMPS *l) : Pair(l) {}
  void compute(int, int) override { ++base_compute_calls; }
  void *extract(const char *, int &) override;
  int base_compute_calls = 0;
  void mock_allocate(int ntypes);
 protected:
  double cut_lj_global = 0.0;
  double **cut_lj = nullptr, **cut_ljsq = nullptr, **epsilon = nullptr, **sigma = nullptr;
  double **lj1 = nullptr, **lj2 = nullptr, **lj3 = nullptr, **lj4 = nullptr, **offset = nullptr;
  double cut_coulsq = 0.0;
 public:
  // (the test host's way to the protected tables, in the order cutsq, cut_ljsq, lj1, lj2, lj3, lj4, offset)
  double **mock_table(int k) { double **tabs[7] = {cutsq, cut_ljsq, lj1, lj2, lj3, lj4, offset}; return tabs[k]; }
 private:
  std::vector<double> table_store;
  std::vector<double *> table_rows;
};

// KSpace (kspace.h) as far as the glue touches it: the settings the handles read, and what a style's compute() fills -- energy,
// virial, eatom, vatom ([nmax][6] behind row pointers, one contiguous block as Memory::create makes it) -- after ev_init() has decoded eflag / vflag (ENERGY_GLOBAL = 1, ENERGY_ATOM = 2; VIRIAL_PAIR = 1, VIRIAL_FDOTR = 2,
// VIRIAL_ATOM = 4, VIRIAL_CENTROID = 8).  What `kspace_style NAME args` and `kspace_modify` leave in the base class: settings(), and
// accuracy_relative / accuracy_absolute (`kspace_modify force`), from which a style's init() forms `accuracy` in force units with
// two_charge_force (the force between two unit charges one Angstrom apart; the host sets it, KSpace's constructor does in LAMMPS)
class KSpace : protected Pointers {
 public:
  explicit KSpace(LAMMPS *l) : Pointers(l) {}
  double g_ewald, accuracy, slab_volfactor, energy; int slabflag; int nx_pppm = 0, ny_pppm = 0, nz_pppm = 0, order = 0;
  int compute_flag = 1, tip4pflag = 0; double qsum = 0.0;
  double virial[6] = {0, 0, 0, 0, 0, 0}; double *eatom = nullptr; double **vatom = nullptr;
  int evflag = 0, eflag_global = 0, eflag_atom = 0, vflag_global = 0, vflag_atom = 0;
  double accuracy_relative = 0.0, accuracy_absolute = -1.0, two_charge_force = 0.0;
  virtual ~KSpace() {}
  virtual void settings(int, char **) {}
  virtual void init() {}
  virtual void setup();
  virtual void compute(int, int) {}
 protected:
  void ev_init(int eflag, int vflag);
 private:
  std::vector<double> eatom_store, vatom_store;
  std::vector<double *> vatom_rows;
};

// LAMMPS' PPPM kspace style and Compute base, as far as pppm_conp_hip.* / compute_potential_atom_hip.* touch them
// PPPM::compute (pppm.cpp @ 27May2021) begins with  particle_map(); make_rho();  -- both virtual -- then sums the ghost planes into
// their owners (gc->reverse_comm), copies the owned brick to the FFT layout (brick2fft) and solves.  The mock runs the two virtuals
// on a brick that covers the rank's share of the mesh plus `order` ghost planes on every side (one rank: the whole mesh), folds the
// ghost planes back periodically and keeps the result (`density_fft`, [nz][ny][nx]): what the real class would transform.
typedef double FFT_SCALAR;
class PPPM : public KSpace {
 public:
  explicit PPPM(LAMMPS *l) : KSpace(l) {}
  void compute(int eflag, int vflag) override;
  void settings(int, char **) override;         // kspace_style pppm ACCURACY
  int differentiation_flag = 0;                 // kspace_modify diff: 0 ik, 1 ad
  virtual void particle_map() { ++base_particle_map_calls; }
  virtual void make_rho();                      // (the real one clears the brick and spreads every charged atom: counted here)
  int base_particle_map_calls = 0, base_make_rho_calls = 0;
  FFT_SCALAR ***density_brick = nullptr;        // [nzlo_out..nzhi_out][nylo_out..nyhi_out][nxlo_out..nxhi_out]
  int nxlo_in = 0, nxhi_in = -1, nylo_in = 0, nyhi_in = -1, nzlo_in = 0, nzhi_in = -1;
  int nxlo_out = 0, nxhi_out = -1, nylo_out = 0, nyhi_out = -1, nzlo_out = 0, nzhi_out = -1, ngrid = 0;
  std::vector<double> density_fft;
  void mock_allocate();
 private:
  std::vector<FFT_SCALAR> brick_store;
  std::vector<FFT_SCALAR *> brick_rows;
  std::vector<FFT_SCALAR **> brick_planes;
};
class Compute : protected Pointers {
 public:
  Compute(LAMMPS *l, int narg, char **arg) : Pointers(l) {
    igroup = narg > 1 ? l->group->find(arg[1]) : 0;
    groupbit = igroup >= 0 ? l->group->bitmask[igroup] : 0;
  }
  virtual ~Compute() {}
  int igroup, groupbit, peratom_flag = 0, size_peratom_cols = 0, peatomflag = 0, timeflag = 0, comm_reverse = 0;
  bigint invoked_peratom = -1;
  double *vector_atom = nullptr;
  virtual void init() {}
  virtual void setup() {}
  virtual void compute_peratom() {}
  virtual double memory_usage() { return 0.0; }
};

namespace FixConst { enum { PRE_EXCHANGE = 1 << 1, POST_NEIGHBOR = 1 << 3, PRE_FORCE = 1 << 5, POST_FORCE = 1 << 7, END_OF_STEP = 1 << 10 }; }

class Fix : protected Pointers {
 public:
  Fix(LAMMPS *l, int narg, char **arg) : Pointers(l) {      // like Fix::Fix: arg[1] is the fix group
    igroup = narg > 1 ? l->group->find(arg[1]) : 0;
    groupbit = igroup >= 0 ? l->group->bitmask[igroup] : 0;
    instance_me = 0;
  }
  virtual ~Fix() {}
  int igroup, groupbit, instance_me, scalar_flag, extscalar, global_freq, respa_level;
  virtual int setmask() = 0;
  virtual void init() {}
  virtual void init_list(int, NeighList *) {}
  virtual void setup_post_neighbor() {}
  virtual void setup_pre_force(int) {}
  virtual void pre_exchange() {}
  virtual void setup_pre_exchange() {}
  virtual void post_run() {}
  virtual void post_neighbor() {}
  virtual void pre_force(int) {}
  virtual void post_force(int) {}
  virtual void end_of_step() {}
  virtual double compute_scalar() { return 0.0; }
  virtual int modify_param(int, char **) { return 0; }
};

namespace utils {
int inumeric(const char *, int, const char *, bool, LAMMPS *);
double numeric(const char *, int, const char *, bool, LAMMPS *);
void logmesg(LAMMPS *, const std::string &);
}  // namespace utils
}  // namespace LAMMPS_NS
