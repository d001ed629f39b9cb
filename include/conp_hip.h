/* =============================================================================================
 * conp_hip.h -- C ABI of libconp_hip.so: the MI355X-native constant-potential charge solver that
 * drops into LAMMPS behind the `fix conp` / KSpaceModule surface of srtee/lammps-USER-CONP2.
 *
 * Boundary rules
 *   - plain C: opaque handle, scalars, caller-owned pointers + sizes; no C++/torch types;
 *   - every function returns 0 on success or a negative conp_status; the message is available from
 *     conp_last_error() (thread-local).  The reference aborts through error->all(FLERR,msg)
 *     (fix_conp.cpp:86,107,127,...): the LAMMPS glue turns a non-zero status into exactly that call;
 *   - calls are synchronous with respect to the host thread unless the name ends in _async/_device;
 *     internally everything is ordered on one HIP stream (conp_fix_set_stream);
 *   - the library never falls back to a CPU path: without a usable gfx950 device every compute
 *     entry point fails with CONP_ERR_NO_DEVICE.
 *
 * Each entry point cites the reference interface it replaces (file:line in /root/reference).
 * INTEGRATION.md shows the binding a maintainer adds to fix_conp.cpp / kspacemodule.h.
 * ===========================================================================================*/
#ifndef CONP_HIP_H
#define CONP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CONP_ABI_VERSION 1

typedef enum {
  CONP_OK = 0,
  CONP_ERR_ARG = -1,        /* illegal fix command / argument (fix_conp.cpp:86,107,127,143,...) */
  CONP_ERR_STATE = -2,      /* call out of order (e.g. pre_force before setup) */
  CONP_ERR_NO_DEVICE = -3,  /* no gfx950 device / HIP runtime failure */
  CONP_ERR_NUMERIC = -4,    /* "Inversion failed!" (fix_conp.cpp:956) */
  CONP_ERR_IO = -5          /* A-matrix file problems (fix_conp.cpp:737,745) */
} conp_status;

enum { CONP_FF_NORMAL = 0, CONP_FF_FFIELD = 1, CONP_FF_NOSLAB = 2 };   /* fix_conp.cpp:68 */
enum { CONP_SOLVER_CG = 0, CONP_SOLVER_INV = 1 };                      /* fix_conp.cpp:67 */

typedef struct conp_fix conp_fix; /* opaque: one `fix conp` instance on one GPU */

/* ---- parsed `fix ID group1 conp Nevery group2 eta DV logfile [keywords]` (fix_conp.cpp:79-201) ---- */
typedef struct {
  int everynum;            /* arg[3]  :102 */
  double eta;              /* arg[5]  :110 */
  double potdiff;          /* arg[6] if numeric :116 */
  int potdiff_is_variable; /* arg[6] = v_name :112-114 (the glue evaluates the variable each step :1143) */
  int ff_flag;             /* ffield / noslab :126-133 */
  int zneutr, matout, pppm, split, qinit, lowmem, nullneutral, ehgo; /* :160-169 */
  int a_matrix_f;          /* 0 none, 1 org, 2 inv :134-145 */
  char a_matrix_file[512];
  int smartlist, eletypenum, eletypes[32]; /* etypes :146-159 */
  int minimizer, maxiter;  /* new keywords `cg [maxiter N] [tol X]`; defaults 1 / 100 (:88-90) */
  double tolerance;        /* default 1e-6 (:89) */
  char logfile[512];       /* arg[7] :119 */
  char group2[128];        /* arg[4] :104 */
  char potdiff_var[128];   /* name after "v_" when potdiff_is_variable (potdiffstr :113) */
  int conq;                /* 1 when arg[2] names the conq style (fix_conq.h:21): DV is then the prescribed charge QR */
  int cond;                /* 1 when arg[2] names the cond style (fix_cond.h): DV is the prescribed charge, potential from the cell dipole */
} conp_fix_args;

/* Parses arg[3..narg-1] of the fix command exactly like the reference constructor (same keywords, same
 * error conditions; unknown keyword -> CONP_ERR_ARG with the reference's message).  ntypes bounds etypes. */
int conp_parse_fix_args(int narg, const char *const *arg, int ntypes, conp_fix_args *out);

/* ---- constants LAMMPS supplies (force->, domain->, kspace->; SURVEY.md 8b "inputs crossing") ---- */
typedef struct {
  double qqrd2e, qqr2e, qe2f, dielectric;         /* force-> (km_ewald.cpp:79, fix_conp.cpp:412) */
  int newton_pair;                                /* force->newton_pair (fix_conp.cpp:198) */
  double g_ewald, accuracy, slab_volfactor;       /* force->kspace-> (km_ewald.cpp:66-69); accuracy ABSOLUTE */
  int slabflag;
  double xprd, yprd, zprd, boxlo_z;               /* domain-> (km_ewald.cpp:81-83, fix_conp.cpp:616-619) */
  double boxlo_x, boxlo_y;                        /* domain->boxlo (pppm_conp.cpp:146-148; only the pppm path needs x, y) */
  int ntypes;
  const double *cutsq;                            /* coulpair->cutsq flattened [(ntypes+1)*(ntypes+1)] (fix_conp.cpp:1235) */
  double cut_coul;                                /* *coulpair->extract("cut_coul") (fix_conp.cpp:1237) */
  int one_electrode;                              /* groupbit == jgroupbit (fix_conp.cpp:295) */
  int device;                                     /* HIP device ordinal of this rank; -1: rank modulo the visible devices;
                                                     -(2 + l): node-local rank l modulo the visible devices (MPI hosts) */
  int rank, nranks;                               /* shard id for the multi-GPU path (section "sharding") */
  /* `pppm` keyword (fix_conp.cpp:162, 401-404): mesh and stencil order of the pppm/conp kspace style, i.e. LAMMPS PPPM's
   * nx_pppm, ny_pppm, nz_pppm, order (pppm_conp.cpp:242, 206); ignored without the keyword */
  int pppm_nx, pppm_ny, pppm_nz, pppm_order;
  /* 1: every ghost atom is a periodic image of an owned atom and moves with it -- what LAMMPS' forward communication
   * guarantees between re-neighbourings (orthogonal box).  The host-buffer hooks then upload the owned x, q only and rebuild
   * the ghosts on the device as x_owner + n*prd (the arithmetic of Comm's pack_comm: same bits).  Checked at every
   * (setup_)post_neighbor; a ghost that is not an exact image switches the handle back to full uploads.  0: x, q of ghosts
   * are read from the caller's arrays at every hook, like the reference reads atom->x. */
  int ghost_images;
} conp_env;

/* FixConp::FixConp + FixConp::init (fix_conp.cpp:79-201, 245-300) */
int conp_fix_create(const conp_fix_args *args, const conp_env *env, conp_fix **out);
void conp_fix_destroy(conp_fix *fix);   /* FixConp::~FixConp :205-229 */
const char *conp_last_error(void);
int conp_abi_version(void);

/* FixConp::modify_param (fix_conp.cpp:1482-1515): `fix_modify ID ehgo kappa X` and `fix_modify ID ehgo coeff types eta u0|auto`
 * (arg[0] = "ehgo").  Only valid with the `ehgo` keyword; *consumed = number of arguments used (3 or 5), like the reference's
 * return value.  The per-type tables are finalised at setup (ehgo_setup_tables :1517-1559); without any coefficient the fix falls
 * back to the plain eta model, as the reference does (with its warning text in conp_last_error()). */
int conp_fix_modify_param(conp_fix *fix, int narg, const char *const *arg, int *consumed);

/* ---- LAMMPS-owned per-atom arrays, re-fetched before every hook (may be reallocated on re-neighbour) ---- */
typedef struct {
  int nlocal, nghost;
  const double *x;     /* atom->x flattened [nall][3] */
  double *q;           /* atom->q [nall]; electrode entries (owned + ghost) are overwritten by pre_force */
  const int *type;     /* atom->type [nall] */
  const int *tag;      /* atom->tag [nall] (tagint == int, fix_conp.cpp:474) */
  const int *echeck;   /* electrode_check(i) for i < nall: +1 group1, -1 group2, 0 else (fix_conp.cpp:599-605) */
} conp_atoms;

/* LAMMPS half neighbour list (NeighList inum/ilist/numneigh/firstneigh) with firstneigh flattened by the glue:
 * neighbours of i are neigh[first[i] .. first[i]+numneigh[i]); entries may carry special-bond bits (NEIGHMASK). */
typedef struct {
  int inum;
  const int *ilist;     /* [inum] */
  const int *numneigh;  /* [nall] */
  const int *first;     /* [nall] */
  const int *neigh;
  int64_t nneigh;       /* length of neigh */
} conp_neighlist;

/* FixConp::init_list (fix_conp.cpp:365-378): which = 0 alist (ele-ele, occasional), 1 blist (ele-elyte, perpetual),
 * 2 both (generic list without etypes).  The pointers must stay valid until the next hook returns. */
int conp_fix_init_list(conp_fix *fix, int which, const conp_neighlist *list);

/* ---- Fix hooks ---- */
int conp_fix_setup_post_neighbor(conp_fix *fix, const conp_atoms *atoms); /* fix_conp.cpp:382-385 (linalg_init + post_neighbor) */
int conp_fix_setup_pre_force(conp_fix *fix, const conp_atoms *atoms, int64_t ntimestep, double potdiff); /* :387-391 */
int conp_fix_post_neighbor(conp_fix *fix, const conp_atoms *atoms);       /* :468-539 */
int conp_fix_pre_force(conp_fix *fix, const conp_atoms *atoms, int64_t ntimestep, double potdiff); /* :543-573 */
/* The fix scalar of the LAST update, whichever entry made it: the host-buffer hooks bring it over themselves, after a
 * device-resident update (conp_fix_pre_force_device, conp_fix_scatter_device) this call forms what is missing and fetches it. */
double conp_fix_compute_scalar(const conp_fix *fix);                      /* :592-595 */
/* FixConp::post_force -> force_cal (fix_conp.cpp:577-580, 1163-1201) + blist_coul_cal_post_force (:1368-1444), ETA pair mode:
 * adds the real-space Gaussian-correction forces to f[nall][3] (host, accumulated like atom->f) and returns what the reference
 * adds to force->kspace->energy (Gaussian self energy) and, through Pair::ev_tally, to eng_coul and the global virial
 * (xx,yy,zz,xy,xz,yz).  The reference's arithmetic is kept as written, including `del*forcecoul` and the `eta^2 r^2 < 5.8` gate. */
int conp_fix_post_force(conp_fix *fix, const conp_atoms *atoms, double *f, double *kspace_energy_add, double *eng_coul_add,
                        double *virial_add /*[6]*/);
/* The same for a host that can say which step it is in: when `ntimestep` is the step of the last conp_fix_pre_force that wrote
 * charges and `atoms->x` is the array handed over there, positions and charges are already on the device (nothing moves between
 * pre_force and post_force of a LAMMPS step) and are not uploaded again.  Any other step (Nevery > 1, a re-neighbour) uploads. */
int conp_fix_post_force_step(conp_fix *fix, const conp_atoms *atoms, int64_t ntimestep, double *f, double *kspace_energy_add,
                             double *eng_coul_add, double *virial_add /*[6]*/);

/* finer-grained pieces of the same path (same names as the reference's methods) */
int conp_fix_linalg_setup(conp_fix *fix, const conp_atoms *atoms);        /* :426-464 a_cal, b_setq_cal, equation_solve, get_setq */
int conp_fix_a_cal(conp_fix *fix, const conp_atoms *atoms);               /* :777-861 */
int conp_fix_b_cal(conp_fix *fix, const conp_atoms *atoms);               /* :677-695 */
int conp_fix_equation_solve(conp_fix *fix);                               /* :698-718 */
int conp_fix_update_charge(conp_fix *fix, const conp_atoms *atoms, double potdiff); /* :1120-1161 */

/* ---- several MPI ranks (LAMMPS spatial decomposition) ------------------------------------------------------------------
 * The reference runs on N ranks: every rank owns the atoms of its sub-domain, and FixConp / KSpaceModuleEwald exchange through
 * MPI_Allreduce (maxtag fix_conp.cpp:415, newtonbuf :1356, structure factors km_ewald.cpp:784-785, sum q^2 :77),
 * MPI_Allgather / MPI_Allgatherv (elenum_list :492, eleall2tag :523, elebuf2eleall :535, b_comm :643, A rows :822).
 * The library makes the same exchanges through callbacks the host supplies (the glue implements them with MPI on `world`,
 * lammps_glue/fix_conp_hip.cpp), so that it needs no MPI itself.  After conp_fix_set_comm the atoms and lists handed to the
 * hooks are THIS RANK's (owned + ghost); the library
 *   - numbers the electrode atoms globally like post_neighbor does (rank-major, :492-525),
 *   - all-gathers the charged electrolyte atoms' (x, q) every update and computes its shard of the k-vectors for ALL electrode
 *     rows, adds its own real-space rows, all-reduces b, solves its rows, all-gathers q,
 *   - shards the once-per-run A build by tiles and all-reduces the matrix before the (replicated, :947-949) inverse.
 * Every callback returns 0 on success.  All ranks must enter every hook together (as with the reference's collectives). */
typedef struct {
  void *ctx;
  int rank, nranks;
  int (*allreduce_sum)(void *ctx, double *buf, int64_t n);                      /* in place, MPI_SUM, MPI_DOUBLE */
  int (*allreduce_max_int)(void *ctx, int *buf, int n);                         /* in place, MPI_MAX, MPI_INT */
  int (*allgather_int)(void *ctx, int value, int *out /*[nranks]*/);            /* MPI_Allgather of one int */
  /* MPI_Allgatherv of bytes: rank r contributes counts[r] bytes, stored at recv + displs[r] */
  int (*allgatherv)(void *ctx, const void *send, int64_t nbytes, void *recv, const int64_t *counts, const int64_t *displs);
} conp_comm;
/* call between conp_fix_create and conp_fix_setup_post_neighbor; overrides conp_env.rank / nranks */
int conp_fix_set_comm(conp_fix *fix, const conp_comm *comm);

/* Data plane on RCCL (one rank per GPU): the all-reduce of b and the all-gather of q of a device-resident update, and the
 * all-reduce of the sharded A build, run inside the library on its own stream over xGMI.  Rank 0 makes an id with
 * conp_rccl_unique_id, the host distributes the 128 bytes (MPI_Bcast, torch.distributed ...), every rank calls
 * conp_fix_comm_init_rccl before setup.  Without it a multi-rank handle uses the conp_comm callbacks (host buffers), or leaves
 * the two collectives to the caller (conp_fix_b_cal_device / _solve_device / _scatter_device). */
#define CONP_RCCL_ID_BYTES 128
int conp_rccl_unique_id(void *id_out /*[CONP_RCCL_ID_BYTES]*/);
int conp_fix_comm_init_rccl(conp_fix *fix, const void *id /*[CONP_RCCL_ID_BYTES]*/);
/* conp_rccl_available: 0 when librccl loads with every entry point the library calls -- local and cheap; ranks agree on it (MIN over
 * ranks) BEFORE the collective conp_fix_comm_init_rccl, so that a rank without RCCL cannot strand its partners inside
 * ncclCommInitRank.  conp_fix_comm_destroy_rccl: all ranks together give the communicator back (an initialisation that failed
 * somewhere: the host then makes the two exchanges itself). */
int conp_rccl_available(void);
int conp_fix_comm_destroy_rccl(conp_fix *fix);

/* ---- KSpaceModule provider surface (kspacemodule.h:30-40), Ewald provider (km_ewald.cpp) ---- */
int conp_km_conp_setup(conp_fix *fix, double qsqsum, int64_t natoms);     /* km_ewald.cpp:63-132 (qsqsum: Allreduce'd sum q^2 :72-78) */
int conp_km_a_cal(conp_fix *fix, const conp_atoms *atoms, double *aaa /*[Ne*Ne], host, overwritten: k-space part only*/); /* :147-151 */
int conp_km_b_cal(conp_fix *fix, const conp_atoms *atoms, double *bbb /*[Ne] eleall order, host*/);                          /* :153-167 */

/* ---- PPPMCONP beyond the b vector (`pppm` keyword; pppm_conp.cpp:385-534), SURVEY 8f-2 --------------------------------------
 * All three take the atoms as they are NOW (after pre_force wrote the electrode charges) and work on the handle's mesh
 * (conp_env.pppm_*).  Mesh arrays are [nz][ny][nx], periodic (one rank: LAMMPS' ghost planes folded in).
 *   conp_pppm_make_rho            : ele_make_rho (:385-426) + the make_rho override (:434-450): density = electrolyte brick +
 *                                   electrode brick, what PPPMCONP hands to PPPM::compute instead of re-spreading every atom.
 *                                   Any output may be NULL.
 *   conp_pppm_compute_group_potential (:487-534): recv[i] = - sum over the order^3 stencil of w * u_brick for owned atoms with
 *                                   sel[i] != 0.  u_brick is what PPPM::compute leaves there when per-atom energies are
 *                                   tallied (ComputePotentialAtom insists on that step, compute_potential_atom.cpp:128-130):
 *                                   the mesh potential of the TOTAL density; the library forms it from the same bricks.
 *   conp_pppm_compute_particle_potential (:452-485): the same for atom i, plus 2 g_ewald q_i / sqrt(pi).  RANK-LOCAL: reads the
 *                                   cached mesh potential (one rank: forms it on demand; several ranks: CONP_ERR_STATE unless a
 *                                   collective entry formed it since the last update). */
int conp_pppm_make_rho(conp_fix *fix, const conp_atoms *atoms, double *density, double *ele_density, double *elyte_density);
/* PPPMCONP keeps the electrolyte brick of every b_cal for its make_rho override (pppm_conp.cpp:172-228, 434-450; elyte_mapped is
 * reset by conp_pre_force, pppm_conp.h:42).  on != 0: from the next b_cal on the brick of the update stays on the device and
 * conp_pppm_make_rho adds the fresh electrode brick to it instead of spreading the electrolyte a second time (one rank; under ranks
 * the bricks are re-made from one gather).  The call itself drops whatever is cached: the glue calls it from conp_pre_force(). */
int conp_pppm_keep_density(conp_fix *fix, int on);
/* The mesh potential of the total density -- what PPPM::compute leaves in u_brick when per-atom energies are tallied.  COLLECTIVE
 * under ranks.  Afterwards conp_pppm_compute_particle_potential is a rank-local stencil gather from the cached brick, like the
 * reference's (:452-485; compute_potential_atom.cpp:168-174 calls it a different number of times on every rank), until the next
 * update or re-neighbouring.  conp_pppm_compute_group_potential and conp_compute_potential_atom leave the same cache. */
int conp_pppm_compute(conp_fix *fix, const conp_atoms *atoms);
int conp_pppm_compute_group_potential(conp_fix *fix, const conp_atoms *atoms, const int *sel /*[nlocal]*/, double *recv /*[nlocal]*/);
int conp_pppm_compute_particle_potential(conp_fix *fix, const conp_atoms *atoms, int i, double *u);

/* ---- Ewald per-atom potential: the same three entries for the Ewald provider ------------------------------------------------
 * The reference's KSpaceModuleEwald inherits `return 0.` for both potentials (kspacemodule.h:38-39), so its compute potential/atom
 * (compute_potential_atom.cpp:165-175) needs a mesh.  Here the k sum is exact, with the handle's own k list and ug:
 *   S_k = sum_j q_j e^{i k r_j} over every charged owned atom (electrolyte and electrode, the charges in `atoms`),
 *   g_i = - sum_{k in the half list} 2 ug_k [cos(k r_i) Re S_k + sin(k r_i) Im S_k]      (no self term, as the mesh version)
 *   u_i = g_i + 2 g_ewald q_i / sqrt(pi)
 * Targets are any owned atoms, zero-charge probes included.  conp_ewald_compute forms and caches S (COLLECTIVE with decomposed
 * ranks: each rank contracts its own atoms, S is summed through conp_comm.allreduce_sum; a replicated-atom handle -- several
 * ranks without conp_fix_set_comm -- computes locally, no collective).  conp_ewald_compute_group_potential (collective):
 * recv[i] = g_i for owned atoms with sel[i] != 0, from the cached S if a collective entry formed it since the last update, else
 * from a fresh one.  conp_ewald_compute_particle_potential: u_i, RANK-LOCAL from the cache (one
 * rank forms it on demand; several ranks: CONP_ERR_STATE unless a collective entry formed it since the last update).  The cache
 * is dropped by every update, re-neighbouring and set_matrix.  On a `pppm` handle all three return CONP_ERR_STATE;
 * conp_compute_potential_atom takes its k-space part from here on an Ewald handle (from the mesh on a `pppm` one). */
int conp_ewald_compute(conp_fix *fix, const conp_atoms *atoms);
int conp_ewald_compute_group_potential(conp_fix *fix, const conp_atoms *atoms, const int *sel /*[nlocal]*/, double *recv /*[nlocal]*/);
int conp_ewald_compute_particle_potential(conp_fix *fix, const conp_atoms *atoms, int i, double *u);

/* ---- Ewald reciprocal-space forces, energy, virial: what a KSpace style's compute() does after the charge update -------------
 * The textbook Ewald sum over the handle's own half list (conp_fix_get_ktables; ug_k = 4 pi / V exp(-k^2 / 4 g^2) / k^2, V with the
 * slab factor), at the positions and charges of `atoms`; S_k as above, qs = env.qqrd2e, g = env.g_ewald, Q = sum q, Q2 = sum q^2,
 * M = sum q z, M2 = sum q z^2 over all ranks' owned atoms:
 *   f_i   += qs q_i sum_k 2 ug_k k [sin(k r_i) Re S_k - cos(k r_i) Im S_k]                        (accumulated, like atom->f)
 *   energy = qs [sum_k ug_k |S_k|^2 - g Q2 / sqrt(pi) - (pi / 2) Q^2 / (g^2 V)]
 *   virial = qs sum_k ug_k |S_k|^2 (delta_ab - 2 (1 / k^2 + 1 / (4 g^2)) k_a k_b)                 (xx, yy, zz, xy, xz, yz)
 *   eatom_i = qs [-q_i u_i / 2 - (pi / 2) q_i Q / (g^2 V)]                                        (sum_i eatom_i = energy)
 * With env.slabflag (L = zprd slab_volfactor): energy += qs 2 pi (M^2 - Q M2 - Q^2 L^2 / 12) / V,
 * f_iz += qs (-4 pi / V) q_i (M - Q z_i), eatom_i += qs (2 pi / V) q_i (z_i M - (M2 + Q z_i^2) / 2 - Q L^2 / 12).
 * Uses the cached S if a collective entry formed it since the last update, else forms it (the cache is valid afterwards).
 * The cached S is that of the x and q the collective entry saw and is valid for exactly those: only an update (b_cal), a
 * re-neighbouring, set_matrix or new k tables drop it -- a pre_force that skips its update (everynum > 1) does not, nor does a call
 * with moved atoms or changed charges, which would contract the old S with the new phases and return CONP_OK.  A caller whose atoms
 * may have changed since S was formed (a KSpace style's compute() on every MD or minimizer step) calls conp_ewald_compute(fix, atoms)
 * first: that forms S of the atoms it is given, unconditionally.
 * COLLECTIVE with decomposed ranks (S unless cached, and the four sums, through conp_comm.allreduce_sum): every rank returns the
 * same global energy and virial, and the forces and eatom of its owned atoms.  A replicated-atom handle computes locally.
 * Zero-charge atoms: f untouched, eatom 0.  Any output may be NULL.  On a `pppm` handle: CONP_ERR_STATE. */
int conp_ewald_compute_forces(conp_fix *fix, const conp_atoms *atoms,
                              double *f      /* [nlocal][3], accumulated; NULL: none */,
                              double *energy /* 1, NULL ok */,
                              double *virial /* [6], NULL ok */,
                              double *eatom  /* [nlocal], overwritten, NULL ok */);

/* ---- PPPM reciprocal-space forces, energy, virial: the mesh twin of conp_ewald_compute_forces --------------
 * PPPM::compute with ik differentiation (LAMMPS pppm.cpp @ 27May2021: make_rho, poisson_ik, fieldforce_ik, fieldforce_peratom's
 * energy, slabcorr) on the handle's mesh, at the positions and charges of `atoms`.  rho^ = forward transform of the density brick,
 * G = the handle's greensfn, N = nx ny nz, V = xprd yprd zprd slab_volfactor, qs = env.qqrd2e, g = env.g_ewald,
 * k = (2 pi / xprd mx, 2 pi / yprd my, 2 pi / (zprd slab_volfactor) mz) with m = i - n floor(2 i / n) per axis, Q, Q2, M, M2 as above:
 *   energy  = qs [(V / 2) sum_k G_k |rho^_k|^2 / N^2 - g Q2 / sqrt(pi) - (pi / 2) Q^2 / (g^2 V)]
 *   virial  = qs (V / 2) sum_k G_k |rho^_k|^2 / N^2 (delta_ab - 2 (1 / k^2 + 1 / (4 g^2)) k_a k_b)   (k = 0: nothing; xx, yy, zz, xy, xz, yz)
 *   E_a     = Re IFFT[-i k_a G_k rho^_k / N]          (minus the gradient of the mesh potential u = IFFT[G rho^ / N])
 *   f_i    += qs q_i sum_stencil w E(mesh point)      (the order^3 stencil weights of the b vector's gather; accumulated)
 *   eatom_i = qs [q_i u_i / 2 - g q_i^2 / sqrt(pi) - (pi / 2) q_i Q / (g^2 V)],  u_i = sum_stencil w u     (sum_i eatom_i = energy)
 * With env.slabflag the three slab terms of conp_ewald_compute_forces (PPPM::slabcorr and Ewald::slabcorr are the same formulas).
 * The density is the one conp_pppm_make_rho returns for the same `atoms`.  It is spread from the atoms of THIS call, every call: the
 * electrolyte brick kept by conp_pppm_keep_density is that of the update's positions, and the handle cannot tell whether the atoms
 * have moved since (a pre_force that skips its update does not drop it), so it is never used here -- the entry never contracts a
 * stale brick with moved atoms, whatever was kept.  conp_info.pppm_elyte_spreads counts one spread per call.
 * Afterwards the mesh-potential cache is what conp_pppm_compute leaves: conp_pppm_compute_particle_potential works without another
 * mesh solve.
 * COLLECTIVE with decomposed ranks, the mesh replicated as for conp_pppm_compute: one tagged gather of all ranks' charged atoms, the
 * four sums through conp_comm.allreduce_sum, and one more allreduce_sum that hands rank 0's seven mesh sums to everybody; every rank
 * returns the same energy and virial (bit for bit) and the forces and eatom of its owned atoms.
 * Zero-charge atoms: f untouched, eatom 0.  Any output may be NULL.  On an Ewald handle: CONP_ERR_STATE. */
int conp_pppm_compute_forces(conp_fix *fix, const conp_atoms *atoms,
                             double *f      /* [nlocal][3], accumulated; NULL: none */,
                             double *energy /* 1, NULL ok */,
                             double *virial /* [6] xx,yy,zz,xy,xz,yz, NULL ok */,
                             double *eatom  /* [nlocal], overwritten, NULL ok */);

/* ---- `compute potential/atom` (compute_potential_atom.cpp:120-345), SURVEY 8f-4 --------------------------------------------
 * per-atom electrostatic potential in volts: pair part over the pair style's half list (:223-308, optional Gaussian `eta`
 * correction for atoms with etasel != 0 = eta_check :313-318), k-space part through the PPPM provider (:165-175 -> the
 * particle potential above), slab correction (:323-345), times qqr2e / qe2f (:214).
 * sel[i] = mask[i] & groupbit for i < nlocal + nghost; potential has nlocal (+ nghost when newton_pair) entries. */
typedef struct {
  int pairflag, kspaceflag, qsumflag;   /* `pair` / `kspace` / not `noqsum` (:59-88) */
  double eta;                           /* 0: no `eta` keyword */
} conp_potential_args;
int conp_compute_potential_atom(conp_fix *fix, const conp_atoms *atoms, const conp_neighlist *pairlist, const int *sel,
                                const int *etasel /*NULL without eta*/, const conp_potential_args *args, double *potential);

/* ---- state read-back for parity tests and for the glue (public members fix_conp.h:58-85) ---- */
typedef struct {
  int elenum, elenum_all, elytenum, maxtag_all, runstage;
  int kcount, kcount_flat, kcount_expand, kxmax, kymax, kzmax, kmax, kmax3d;
  int kcount_dims[7];
  int cg_iterations;
  int n_zclasses;          /* distinct electrode z values when the planar fast path of the projection is active, else 0 */
  double unitk[3], volume, gsqmx, ug_tot, totsetq, scalar_output, totinve, slabcorr;
  int64_t n_blist_pairs, n_alist_pairs, n_elyte_charged;
  int inverse_path;        /* how the last inverse (fix_conp.cpp:947-949) was formed: 0 none yet, 1 positive-definite elimination (no
                              pivot search), 2 partial pivoting */
  int inverse_retries;     /* 1: the multi-workgroup pivot panel timed out at its grid barrier and the one-workgroup panel redid it */
  int pppm_elyte_spreads;  /* `pppm`: how often the electrolyte atoms have been spread onto the mesh so far (b_cal, density and potential queries) */
  int zn_cols, zn_grid, zn_rows; /* the z-window form of the structure-factor contraction (conp_zn.hip) is in use: window columns (32 / 48), z grid points,
                              G rows this rank contracts; all 0: the full kernels */
  int zn_ranges;           /* z-window: chunk ranges of this rank's item list (one projected piece per range and row tile), 0: the full kernels */
  int hc_arithmetic;       /* 1: the sums over the projected pieces form the piece addresses themselves (no list look-ups) */
  int zc_final;            /* planar electrodes: the finishing dot kernel completes b (0: it is not used) -- 1: electrode phases loaded per thread,
                              2: their rows staged in LDS */
  int zc_row_tiles;        /* row tiles (of 64 planar vectors) that kernel walks on this rank */
} conp_info;
int conp_fix_info(const conp_fix *fix, conp_info *out);
/* integer tables; pass NULL for those not wanted.  Sizes: kcount / kcount_expand */
int conp_fix_get_ktables(const conp_fix *fix, int *kxvecs, int *kyvecs, int *kzvecs, double *ug, int *kxy_list, int *kz_list);
/* maps: ele2tag[elenum] ele2eleall[elenum] eleall2tag[Ne] eleall2ele[Ne+1] elecheck_eleall[Ne] elebuf2eleall[Ne] tag2eleall[maxtag+1] */
int conp_fix_get_maps(const conp_fix *fix, int *ele2tag, int *ele2eleall, int *eleall2tag, int *eleall2ele,
                      int *elecheck_eleall, int *elebuf2eleall, int *tag2eleall);
int conp_fix_get_matrix(conp_fix *fix, double *aaa_all /*[Ne*Ne]*/);   /* A, or projected A^-1 after inv() */
int conp_fix_set_matrix(conp_fix *fix, const double *aaa_all, int runstage); /* a_read 'org'/'inv' path :721-773 (file parsing is the glue's) */
int conp_fix_get_vectors(conp_fix *fix, double *bbb_all, double *eleallq, double *elesetq); /* each [Ne] or NULL */
int conp_fix_get_sfac(conp_fix *fix, double *sfacrl, double *sfacim);  /* [kcount], reference k order (km_ewald.cpp:782-786) */
int conp_fix_get_ele_trig(conp_fix *fix, double *csk, double *snk);    /* [Ne][kcount_flat] (km_ewald.cpp:261-268 lowmem) */
/* inv_project on a caller-supplied matrix (bit-exact electroneutrality projection, fix_conp.cpp:982-1067) */
int conp_inv_project(conp_fix *fix, int n, double *aaa, int nullneutral, int zneutr, const double *eleallz, double zhalf,
                     double *totinve_out);

/* On-disk matrix formats of the reference.  write: which = 0 -> "amatrix" layout (fix_conp.cpp:833-849: a tag row
 * of %20d, then rows of %20.12f), which = 1 -> "inv_a_matrix" layout (:960-977: %20d tags, %20.10f entries); the current device
 * matrix is written.  read: FixConp::a_read (:721-773) for the `org F` / `inv F` keywords -- the first Ne tokens are the tags
 * that define the permanent electrode numbering, the following Ne*Ne tokens the matrix; errors "Too many entries in A matrix
 * file" / "Too few entries in A matrix file" as in the reference.  Call it between setup_post_neighbor and setup_pre_force
 * (it stands for a_cal); the keyword decides whether the inverse is still computed (org) or taken as given (inv). */
int conp_fix_write_matrix_file(conp_fix *fix, const char *path, int which);
int conp_fix_read_matrix_file(conp_fix *fix, const conp_atoms *atoms, const char *path);

/* the LU-quality inverse that stands where the reference calls dgetrf_/dgetri_ (fix_conp.cpp:947-949), on a caller-supplied
 * row-major n x n matrix (host pointer, overwritten).  CONP_ERR_NUMERIC ("Inversion failed!") on a singular matrix. */
int conp_invert(conp_fix *fix, int n, double *aaa);

/* ---- host-only logic, callable without a GPU (CPU unit tests of the integer contracts) ---------------------------------
 * conp_host_ktables: the k-vector tables of KSpaceModuleEwald::conp_setup (km_ewald.cpp:63-132, 285-424) for the given
 * parameters.  Call once with NULL arrays to get the counts in info[16] = {kcount, kcount_flat, kcount_expand, kxmax, kymax,
 * kzmax, kmax, kmax3d, kcount_dims[0..6], n_planar}, then with arrays of those sizes.  plan_* (optional) return the GPU plan:
 * per k the planar-vector index, kz index and sign. */
int conp_host_ktables(double g_ewald, double accuracy, double slab_volfactor, int slabflag, double xprd, double yprd, double zprd,
                      double qsqsum, int64_t natoms, double qqrd2e, double dielectric, int *info /*[16]*/, int *kxvecs,
                      int *kyvecs, int *kzvecs, double *ug, int *kxy_list, int *kz_list, int *plan_p, int *plan_m, int *plan_sign);
/* conp_host_index: FixConp::post_neighbor's maps (fix_conp.cpp:468-539) for a sequence of two neighbour builds: atoms as they
 * are at the first post_neighbor (tag0/echeck0, n0 owned atoms) and at a later one (tag1/echeck1, n1).  Outputs like
 * conp_fix_get_maps, for the state after the second call; sizes[4] = {elenum, elenum_all, elytenum, maxtag_all}. */
int conp_host_index(int n0, const int *tag0, const int *echeck0, int n1, const int *tag1, const int *echeck1, int *sizes,
                    int *ele2tag, int *ele2eleall, int *eleall2tag, int *eleall2ele, int *elebuf2eleall, int *tag2eleall);
/* conp_host_pair_rows: the electrode-row regrouping of a LAMMPS half list (which = 1: blist_coul_cal membership,
 * fix_conp.cpp:1313-1353; which = 0: alist_coul_cal, :1242-1276; which = 2: post-force pairs :1411).  Returns the number of
 * pairs; with non-NULL arrays fills row_ptr[Ne+1] (which 0/1), ele_atom/oth_atom[npairs], col[npairs] (which 0). */
int64_t conp_host_pair_rows(int which, const conp_neighlist *list, const conp_atoms *atoms, int newton, int *row_ptr,
                            int *ele_atom, int *oth_atom, int *col);

/* ---- device-resident operation (bench, GPU-resident MD engines, multi-GPU) -------------------------------------
 * x/q are DEVICE pointers with the same layout as conp_atoms.x/q; nothing crosses PCIe.  One charge update =
 *   conp_fix_b_cal_device  (this rank's shard of b into the bound b buffer: its k-shard for ALL rows + its rows of
 *                           the real-space term; slab term on rank 0) -> [caller: all-reduce b over ranks] ->
 *   conp_fix_solve_device  (rows [row0,row1) of q = S b (+ dV S d) into the bound q buffer) ->
 *                          [caller: all-gather q] -> conp_fix_scatter_device (q[i] for owned+ghost electrode atoms).
 * With nranks == 1 conp_fix_pre_force_device runs all three back to back.
 * Large planar systems take the z-window form of the structure-factor contraction (conp_info.zn_cols > 0): every electrolyte atom
 * must stay within 2.5 A (in z) of its position at the last conp_fix_post_neighbor -- LAMMPS re-neighbours long before that.  The
 * device-resident entries do not synchronise, so an atom that left its window is seen one call later: that call returns
 * CONP_ERR_NUMERIC (the charges of the updates since the list build are invalid; call conp_fix_post_neighbor and repeat), and the
 * handle uses the full kernels until the next list build.  This holds for replayed graphs (CONP_GRAPH=1) too.  When the next call
 * is conp_fix_post_neighbor (or conp_fix_post_neighbor_device), it completes the list build at the new positions and then returns
 * CONP_ERR_NUMERIC (the handle is ready; repeat the update).  conp_fix_pre_force (host arrays) repeats the update by itself. */
int conp_fix_set_stream(conp_fix *fix, void *hip_stream);
int conp_fix_bind_device_buffers(conp_fix *fix, double *d_b /*[Ne]*/, double *d_q /*[Ne]*/);
/* this rank's electrode rows: blocks of ceil(Ne / nranks) rows, so that rank r's rows start at r * ceil(Ne / nranks) */
int conp_fix_row_range(const conp_fix *fix, int *row0, int *row1);
int conp_fix_b_cal_device(conp_fix *fix, const double *d_x, const double *d_q);
int conp_fix_solve_device(conp_fix *fix, double potdiff);
int conp_fix_scatter_device(conp_fix *fix, double *d_q_atoms, double potdiff);
int conp_fix_pre_force_device(conp_fix *fix, const double *d_x, double *d_q, double potdiff);
/* ---- device-resident k-space forces: conp_ewald_compute_forces / conp_pppm_compute_forces without a host round trip (DESIGN.md
 * section 14) -- the force half of a device-resident step.
 * Pointers and layout: ALL pointers are device pointers.  d_x / d_q have the layout of conp_fix_pre_force_device (owned atoms first,
 * then ghosts); nlocal is that of the last (setup_)post_neighbor.
 * Formulas: those of conp_ewald_compute_forces / conp_pppm_compute_forces above (DESIGN.md sections 12, 13); d_ev[0] is their energy,
 * d_ev[1..6] their virial.
 * Asynchronous (the names end in _device): everything is enqueued on the handle's stream (conp_fix_set_stream) and the results are
 * valid once the stream has reached that point.  After the first call at a given size a call makes no device allocation, no copy to
 * the host and no stream or device synchronisation (the first call may allocate) -- a conp_fix_pre_force_device followed by a force
 * entry on the same stream needs no synchronisation between them.
 * No cache: S (`pppm`: the density brick) is formed from the d_x, d_q of the call, every call -- the handle cannot know whether
 * device arrays have changed, so the cached S and an electrolyte brick kept by conp_pppm_keep_density are never used.  Afterwards the
 * host entries' caches (the structure factor and per-atom potentials of conp_ewald_*, the mesh potential of conp_pppm_compute) are
 * dropped: the scratch they describe has been overwritten, and the host entries form what they need again from their own `atoms`.
 * conp_info.pppm_elyte_spreads counts one spread per PPPM call.
 * Targets: every owned atom, no compaction -- the launch shapes depend on nlocal only.  A zero-charge atom adds exactly 0.0 to its
 * force, its d_eatom entry is 0, and it contributes nothing to S or to Q, Q2, M, M2.
 * Ranks: a handle with conp_fix_set_comm (decomposed) returns CONP_ERR_STATE (device-resident entries take replicated atoms); a
 * replicated-atom handle computes locally, as the host entries do.
 * Errors: CONP_ERR_STATE on the other provider's handle and before the k tables / the mesh exist; CONP_ERR_ARG for a NULL d_x or
 * d_q; all three outputs NULL: CONP_OK, nothing done. */
int conp_ewald_compute_forces_device(conp_fix *fix, const double *d_x, const double *d_q,
                                     double *d_f     /* [nlocal][3], accumulated; NULL: none */,
                                     double *d_ev    /* [7]: energy, then virial xx,yy,zz,xy,xz,yz; overwritten; NULL ok */,
                                     double *d_eatom /* [nlocal], overwritten; NULL ok */);
int conp_pppm_compute_forces_device(conp_fix *fix, const double *d_x, const double *d_q, double *d_f, double *d_ev, double *d_eatom);

/* ---- per-atom virial of the k-space force entries: the missing output of a KSpace style's compute() ------
 * Each entry is its sibling above with one more trailing output, vatom [nlocal][6] in the order xx, yy, zz, xy, xz, yz, so that
 * S / the density brick and the forward transform are formed once per step for all outputs.  Notation of the siblings: the half
 * list with ug_k, qs = env.qqrd2e, g = env.g_ewald, S_k of the atoms of the call,
 *   vg_ab(k) = delta_ab - 2 (1 / k^2 + 1 / (4 g^2)) k_a k_b.
 * Ewald (LAMMPS Ewald::compute's vatom), with A_i(k) = cos(k r_i) Re S_k + sin(k r_i) Im S_k:
 *   vatom_i,ab = qs q_i sum_k ug_k vg_ab(k) A_i(k)                  (sum_i vatom_i,ab = the entry's virial, as sum_i q_i A_i = |S_k|^2)
 * PPPM (poisson_peratom / fieldforce_peratom of pppm.cpp @ 27May2021, ik), with phi_k = G_k rho^_k / N:
 *   v_ab = Re IFFT[vg_ab(k) phi_k]   (k = 0: nothing),   vatom_i,ab = qs q_i / 2 sum_stencil w v_ab(mesh point)
 * with the stencil weights of the force gather.  For an even mesh length an off-diagonal component on the plane where exactly one
 * of its two axes sits at m = -n / 2 has an imaginary inverse, which the real part drops (both axes there: kept).
 * The slab correction adds nothing to the per-atom virial (as in LAMMPS).  A zero-charge atom's six entries are exactly 0.0.  The
 * array is overwritten, like eatom.
 * vatom == NULL: the sibling -- the Ewald entries return the same bits, the PPPM entries agree to the rounding the spread's atomic
 * adds allow.  Everything else is the sibling's contract word for word: the cache rules of the host entries; for the _device entries
 * no cache and no allocation / host copy / synchronisation after the first call, all outputs NULL -> CONP_OK, nothing done;
 * CONP_ERR_STATE on the other provider's handle, and for a decomposed handle on the _device entries.  The host entries are COLLECTIVE
 * under decomposed ranks exactly as the siblings are; the per-atom virial needs no collective of its own (S / the mesh is global). */
int conp_ewald_compute_forces_vatom(conp_fix *fix, const conp_atoms *atoms, double *f, double *energy, double *virial, double *eatom,
                                    double *vatom /* [nlocal][6] xx,yy,zz,xy,xz,yz, overwritten, NULL ok */);
int conp_pppm_compute_forces_vatom(conp_fix *fix, const conp_atoms *atoms, double *f, double *energy, double *virial, double *eatom,
                                   double *vatom /* [nlocal][6], overwritten, NULL ok */);
int conp_ewald_compute_forces_vatom_device(conp_fix *fix, const double *d_x, const double *d_q, double *d_f, double *d_ev, double *d_eatom,
                                           double *d_vatom /* [nlocal][6], overwritten; NULL ok */);
int conp_pppm_compute_forces_vatom_device(conp_fix *fix, const double *d_x, const double *d_q, double *d_f, double *d_ev, double *d_eatom,
                                          double *d_vatom /* [nlocal][6], overwritten; NULL ok */);

/* ---- real-space pair forces: `pair_style lj/cut/coul/long` (and coul/long) on the device -----------------
 * The pair loop of LAMMPS' pair_lj_cut_coul_long.cpp @ 27May2021 with ncoultablebits = 0 over the pair style's half list, with
 * Pair::ev_tally's energy, virial and per-atom tallies.  g = env.g_ewald, qs = env.qqrd2e, newton = env.newton_pair.  For every listed
 * pair (owner i, neighbour entry jraw): sb = (jraw >> 30) & 3, j = jraw & 0x3FFFFFFF, fc = special_coul[sb], fl = special_lj[sb],
 * del = x_i - x_j, rsq = |del|^2; the pair is skipped unless rsq < cutsq[ti][tj]; rsq is not guarded against zero (as in LAMMPS).
 *   r2inv = 1 / rsq
 *   if rsq < cut_coul^2:          (plain cut_coul^2 -- not the min(cut_coul, 5.8 / g)^2 of the fix's own pair kernels)
 *     r = sqrt(rsq), x = g r, e = exp(-x^2), t = 1 / (1 + 0.3275911 x)
 *     erfc = t (0.254829592 + t (-0.284496736 + t (1.421413741 + t (-1.453152027 + t 1.061405429)))) e      (part of the definition)
 *     pre = qs q_i q_j / r;  forcecoul = pre (erfc + 1.12837917 x e);  ecoul = pre erfc
 *     if fc < 1: forcecoul -= (1 - fc) pre;  ecoul -= (1 - fc) pre
 *   if cut_ljsq != NULL and rsq < cut_ljsq[ti][tj]:
 *     r6inv = r2inv^3;  forcelj = r6inv (lj1 r6inv - lj2);  evdwl = fl (r6inv (lj3 r6inv - lj4) - offset)
 *   fpair = (forcecoul + fl forcelj) r2inv
 *   f_i += del fpair;   if newton or j < nlocal: f_j -= del fpair
 * Tally: w = 1 with newton on, else (i < nlocal) / 2 + (j < nlocal) / 2;  eng_vdwl += w evdwl, eng_coul += w ecoul,
 * virial += w fpair (dx^2, dy^2, dz^2, dx dy, dx dz, dy dz);  eatom gets (evdwl + ecoul) / 2 and vatom fpair / 2 times the six products,
 * once for i (if newton or i < nlocal) and once for j (if newton or j < nlocal).  Hence sum eatom = eng_vdwl + eng_coul and
 * sum vatom = virial; with newton on the ghost entries of f, eatom, vatom carry what LAMMPS' reverse communication would fold back,
 * with newton off ghost entries are not touched.
 * Order: conp_pair_set_params (once per run, or after pair_coeff changes) -> conp_pair_set_list or conp_pair_build_list_device
 * (at every re-neighbour) ->
 * conp_pair_compute / conp_pair_compute_device (every step).  Before set_params or set_list both compute entries return
 * CONP_ERR_STATE.  The list and nall are those of the last conp_pair_set_list; the tables and the list are copied (uploaded), the
 * caller's arrays need not stay.  conp_pair_set_list may synchronise and allocate; it checks that every index of the list is < nall, and a list it refuses (CONP_ERR_ARG) leaves the handle without one.
 * The entries work on Ewald and on `pppm` handles.  They are rank-local, never collective: with decomposed ranks each rank passes
 * its own atoms and list, and the sums over ranks and the reverse communication of ghost forces stay with the caller, as in LAMMPS.
 * No cache: every call uses the x and q it is given.
 * Reproducibility: eng and virial are summed in a fixed order and are bit-identical from run to run on the same input; f, eatom and
 * vatom are accumulated with atomic adds and reproduce to rounding only. */
typedef struct {
  int ntypes;                         /* must equal env.ntypes */
  const double *cutsq;                /* [(ntypes+1)^2] the PAIR style's cutsq = max(cut_lj, cut_coul)^2 per type pair */
  double cut_coul;
  const double *cut_ljsq, *lj1, *lj2, *lj3, *lj4, *offset;   /* [(ntypes+1)^2] each; cut_ljsq == NULL: no LJ part (coul/long) */
  double special_lj[4], special_coul[4];                     /* [0] is 1.0 */
} conp_pair_params;
int conp_pair_set_params(conp_fix *fix, const conp_pair_params *p);             /* copied; once per run or after pair_coeff changes */
int conp_pair_set_list(conp_fix *fix, const conp_neighlist *list, int nall);    /* the pair style's half list, uploaded; at every re-neighbour */
/* Host arrays.  atoms->nlocal + atoms->nghost must equal the nall of conp_pair_set_list (else CONP_ERR_ARG); type is atoms->type.
 * x and q go to the device once, through the handle's upload path when nall is that of the last (setup_)post_neighbor (so
 * env.ghost_images 0 and 1 both work), else by a plain copy.  Synchronous.  NULL atoms: CONP_ERR_ARG; all outputs NULL: CONP_OK,
 * nothing done. */
int conp_pair_compute(conp_fix *fix, const conp_atoms *atoms,
                      double *f      /* [nall][3] accumulated like atom->f; NULL: none */,
                      double *eng    /* [2] eng_vdwl, eng_coul; NULL ok */,
                      double *virial /* [6] xx,yy,zz,xy,xz,yz; NULL ok */,
                      double *eatom  /* [nall] overwritten; NULL ok */,
                      double *vatom  /* [nall][6] overwritten; NULL ok */);
/* Device arrays: ALL pointers are ordinary device memory, d_x / d_q / d_f in the layout of conp_fix_pre_force_device (owned atoms
 * first, then ghosts; d_f [nall][3]).  type and nlocal are those of the last (setup_)post_neighbor, whose atom count must equal the
 * nall of conp_pair_set_list (else CONP_ERR_STATE); those types were checked against [0, ntypes] there (one outside: CONP_ERR_ARG here).  Everything is enqueued on the handle's stream (conp_fix_set_stream); after the
 * first call at a given nall and list size a call makes no device allocation, no copy to the host and no synchronisation (the
 * contract of DESIGN.md section 14): conp_fix_pre_force_device, a k-space force entry and this one follow each other on one stream
 * without a synchronisation between them.  NULL d_x or d_q: CONP_ERR_ARG; all outputs NULL: CONP_OK, nothing done. */
int conp_pair_compute_device(conp_fix *fix, const double *d_x, const double *d_q,
                             double *d_f /* [nall][3] accumulated */, double *d_ev /* [8]: eng_vdwl, eng_coul, virial[6]; overwritten */,
                             double *d_eatom /* [nall] */, double *d_vatom /* [nall][6] */);

/* ---- the pair style's half list built on the device ----------------------------------------------------
 * conp_pair_build_list_device fills the list conp_pair_compute[_device] reads from d_x alone, in place of conp_pair_set_list: an
 * engine whose coordinates live on the device re-neighbours without copying them back.  The list is LAMMPS' half/bin/newtoff
 * (env.newton_pair == 0) or half/bin/newton list as a set, with the orientation of conp_amd/neighbor.py::_half_pairs:
 *   owners i < nlocal, candidates j < nall, j != i;  del = x_i - x_j, rsq = delx^2 + dely^2 + delz^2 (products as written);
 *   the pair is listed iff rsq < cutneigh^2 and
 *     newton off, or j < nlocal:  j > i
 *     newton on and j >= nlocal:  z_j > z_i, or z_j == z_i and y_j > y_i, or both equal and x_j > x_i   (the stored doubles)
 *   One global cutneigh (per-type-pair list cutoffs and triclinic boxes: not supported); cutneigh^2 below the largest entry of the
 *   cutsq table of conp_pair_set_params is refused.
 * Special bonds (optional: d_tag, d_nspecial, d_special all non-NULL), LAMMPS' per-atom form, all DEVICE pointers: d_tag [nall],
 * d_nspecial [nlocal][3] cumulative (1-2, 1-2 + 1-3, all), d_special [nlocal][maxspecial] tags.  For a listed pair `which` is the
 * class (1, 2, 3) of the FIRST position of tag[j] in special[i][0 .. nspecial[i][2]), 0 if absent.  The entry is j | (which << 30)
 * when which > 0, special_lj[which] and special_coul[which] of conp_pair_set_params are not both 1.0, and the pair passes LAMMPS'
 * minimum_image_check: no dimension c with prd_half[c] > 0 has |del_c| > prd_half[c] (the image of a bonded partner more than half
 * a box away is an ordinary neighbour); else plain j.  Nothing is dropped: with coul/long LAMMPS keeps excluded pairs for the
 * k-space correction.  prd_half: half the box length per dimension, 0 for a non-periodic one.  Counts in d_nspecial outside
 * [0, maxspecial] are clamped.
 * Result: ilist = 0 .. nlocal-1; numneigh[i] and first[i] (the exclusive scan of numneigh) for i < nlocal, 0 for i >= nlocal; a row
 * is ordered by the traversal of the cells around i (cell members in ascending atom index): the arrays are a pure function of the
 * input, byte-identical from build to build.
 * conp_pair_build_list_device replaces the handle's list as conp_pair_set_list does, and reserves what the compute entries need
 * (their contract of no allocation, host copy or synchronisation holds after it); it may itself allocate and synchronise (the pair
 * count reaches the host to size neigh).  Before conp_pair_set_params: CONP_ERR_STATE.  NULL d_x or a, nlocal > nall, a negative
 * size, a too small cutneigh, some but not all of the three special pointers, a negative maxspecial or prd_half: CONP_ERR_ARG.  A
 * coordinate of d_x[0 .. nall) that is not finite (it never becomes a cell index), or 2^31 pairs or more (`first` is int):
 * CONP_ERR_NUMERIC.  A refused build leaves the handle without a list.  Works on Ewald and `pppm` handles; rank-local.
 * conp_pair_list_moved_device is Neighbor::check_distance on the device: *d_flag (DEVICE memory, overwritten) = 1 if an owned atom
 * has |x - x_build|^2 > trigger^2, x_build the owned coordinates the last build saw, else 0 (a coordinate that is not a number
 * counts as moved).  LAMMPS passes skin / 2.  Enqueued on the handle's stream: no allocation, no synchronisation.  CONP_ERR_STATE
 * when the handle's list did not come from a build; NULL d_x or d_flag, a negative trigger: CONP_ERR_ARG.
 * conp_pair_get_list downloads the list the handle holds, built or uploaded (synchronous): the sizes, and with non-NULL arrays
 * ilist [inum], numneigh [nall], first [nall], neigh [nneigh] -- the host copy conp_fix_init_list / conp_fix_post_neighbor take.
 * Without a list: CONP_ERR_STATE. */
typedef struct {
  int nlocal, nall;
  double cutneigh;
  const int *d_tag, *d_nspecial, *d_special;  /* all three or none */
  int maxspecial;
  double prd_half[3];
} conp_pair_build_args;
int conp_pair_build_list_device(conp_fix *fix, const double *d_x, const conp_pair_build_args *a);
int conp_pair_list_moved_device(conp_fix *fix, const double *d_x, double trigger, int *d_flag);
int conp_pair_get_list(conp_fix *fix, int *inum, int *nall, int64_t *nneigh,
                       int *ilist, int *numneigh, int *first, int *neigh);   /* arrays NULL: sizes only */

/* ---- ghost atoms built, updated and folded back on the device ---------------------------------------------
 * Comm::borders, Comm::forward_comm and Comm::reverse_comm of LAMMPS for ONE rank in a periodic orthogonal box, and the remap into
 * the box that precedes a ghost build: what keeps the ghost part of d_x, d_q and d_f (nlocal owned atoms, then nghost periodic
 * images) without a host round trip.  All d_ pointers are ordinary device memory; everything runs on the handle's stream
 * (conp_fix_set_stream).  The entries work on Ewald and `pppm` handles; they are rank-local, never collective (ghosts owned by
 * other ranks and triclinic boxes: not supported).  This state is separate from conp_env.ghost_images of the host-array hooks.
 *
 * The build rule (conp_amd/neighbor.py::make_ghosts, bit for bit).  On the host, in double: prd_c = boxhi_c - boxlo_c,
 * lo_c = boxlo_c - cutghost, hi_c = boxhi_c + cutghost; m_c = ceil(cutghost / prd_c) in a periodic dimension, 0 in another.  Shifts
 * are the triples (sx, sy, sz), s_c in -m_c .. m_c, enumerated with sx slowest and sz fastest, each ascending, without (0, 0, 0).
 * For owner o and shift s:  xi_c = x[o][c] + ((double)s_c * prd_c) -- the product first, then the sum, no contraction, also for
 * s_c = 0: the arithmetic of Comm::pack_comm.  The image is a ghost iff lo_c <= xi_c < hi_c in all three dimensions.  Ghosts are
 * ordered by shift in that enumeration and, within a shift, by ascending owner: the map is a pure function of the input,
 * byte-identical from build to build.  Owned atoms outside the box are not an error (the rule is applied as written); a coordinate
 * that is not a number or infinite fails every comparison: that atom has no images.
 *
 * conp_ghost_build_device keeps owner[g] and img[g][3] of every ghost and, per owner, the list of its ghosts in ascending ghost
 * index; *nghost reaches the host, so the build may allocate and synchronise (like conp_pair_build_list_device), and it reserves
 * whatever fill and fold need.  CONP_ERR_ARG: NULL a or nghost, NULL d_x with nlocal > 0, negative nlocal, cutghost negative or not
 * a number, a box bound that is not finite, boxhi_c <= boxlo_c in a periodic dimension, more than 4096 shifts.  CONP_ERR_NUMERIC:
 * nlocal + nghost >= 2^30 (neighbour entries keep 30 bits; counted before anything is allocated for the ghosts).  A refused build
 * leaves the handle without ghosts.
 * conp_ghost_fill_device: for every ghost x[nlocal + g] = x[owner] + img * prd (the arithmetic above, the prd of the build) and
 * q[nlocal + g] = q[owner]; NULL d_q: coordinates only.  conp_ghost_fill_int_device copies `width` (1 .. 8) ints per ghost from the
 * owner's row: tag, type, mask.  conp_ghost_fold_device: for every owner and component v[o] = (((v[o] + v[g1]) + v[g2]) + ...) over
 * its ghosts in ascending ghost index, summed by one thread in that order without atomics -- a pure function of the input; ghost
 * rows are left as they are (as LAMMPS does: the caller clears f each step); width 1 (eatom), 3 (f) or 6 (vatom), any other:
 * CONP_ERR_ARG.  These three make no allocation, no copy to the host and no synchronisation (the contract of DESIGN.md section 14).
 * conp_ghost_get downloads the map (synchronous); NULL arrays: the sizes only.
 * Fill, fill_int, fold and get before a successful build: CONP_ERR_STATE.  A NULL array that is required (nlocal + nghost > 0):
 * CONP_ERR_ARG.  Without ghosts (nlocal 0, no periodic dimension, cutghost 0) fill and fold are no-ops returning CONP_OK.
 * conp_atoms_wrap_device is Domain::remap for owned atoms, per periodic dimension c:  if x < boxlo_c: x += prd_c, image_c -= 1;
 * then if x >= boxhi_c: x -= prd_c, x = max(x, boxlo_c), image_c += 1.  One pass: atoms must have moved less than a box length.
 * d_image: optional plain int counters [nlocal][3].  Enqueued only, no allocation; needs no earlier ghost build.  CONP_ERR_ARG: NULL
 * d_x with nlocal > 0, NULL boxlo / boxhi / periodic, negative nlocal, boxhi_c <= boxlo_c in a periodic dimension.
 *
 * Intended order, all on one stream.  At a re-neighbour: conp_pair_list_moved_device (the decision) -> conp_atoms_wrap_device ->
 * conp_ghost_build_device -> conp_ghost_fill_device and conp_ghost_fill_int_device for tag -> conp_pair_build_list_device.  At
 * every step: conp_ghost_fill_device -> conp_fix_pre_force_device, the k-space force entry and conp_pair_compute_device ->
 * conp_ghost_fold_device on d_f, and on d_eatom / d_vatom when they are tallied.  The fix itself is re-neighboured from the same
 * arrays by conp_fix_post_neighbor_device (below), right behind conp_pair_build_list_device. */
typedef struct {
  int nlocal;
  double boxlo[3], boxhi[3];
  int periodic[3];
  double cutghost;
} conp_ghost_build_args;
int conp_ghost_build_device(conp_fix *fix, const double *d_x /*[nlocal][3]*/, const conp_ghost_build_args *a, int *nghost);
int conp_ghost_fill_device(conp_fix *fix, double *d_x /*[nall][3]*/, double *d_q /*[nall] or NULL*/);
int conp_ghost_fill_int_device(conp_fix *fix, int *d_v /*[nall][width]*/, int width);
int conp_ghost_fold_device(conp_fix *fix, double *d_v /*[nall][width]*/, int width);
int conp_ghost_get(conp_fix *fix, int *nlocal, int *nghost, int *owner /*[nghost] or NULL*/, int *img /*[nghost][3] or NULL*/);
int conp_atoms_wrap_device(conp_fix *fix, double *d_x /*[nlocal][3]*/, int nlocal, const double boxlo[3], const double boxhi[3],
                           const int periodic[3], int *d_image /*[nlocal][3] or NULL*/);

/* ---- the fix re-neighboured on the device -----------------------------------------------------------------
 * conp_fix_post_neighbor_device is FixConp::post_neighbor for an engine whose atoms live on the device: it rebuilds everything
 * conp_fix_post_neighbor leaves on the device for the update and for post_force, from the handle's own half list
 * (conp_pair_build_list_device), its own ghost map (conp_ghost_build_device) and the d_x [nall][3], d_q [nall] of the call -- of
 * which only the owned rows are read (ghost rows must already be filled: the updates that follow read them).  No per-atom and no
 * per-pair data crosses PCIe.  The re-neighbour sequence of a device-resident engine is
 *   conp_atoms_wrap_device -> conp_ghost_build_device -> conp_ghost_fill_device (+ conp_ghost_fill_int_device for tag) ->
 *   conp_pair_build_list_device -> conp_fix_post_neighbor_device,
 * and the run needs host arrays once, at setup.
 * Preconditions (one that fails: CONP_ERR_STATE, a NULL d_x or d_q: CONP_ERR_ARG; a refused call leaves the handle exactly as it was):
 *   - conp_fix_setup_post_neighbor and conp_fix_linalg_setup / conp_fix_setup_pre_force have run with host arrays (the electrode
 *     numbering, the A matrix and its inverse stay host-side work, once per run);
 *   - the handle is not decomposed (no conp_fix_set_comm; replicated-atom rank handles are allowed);
 *   - a successful conp_pair_build_list_device and a successful conp_ghost_build_device exist, both for the nlocal of the last host
 *     (setup_)post_neighbor; the list's nall is nlocal + nghost of the ghost map; the list's cutneigh is at least env.cut_coul (its
 *     newton setting is env.newton_pair by construction);
 *   - the owned atoms keep the local order and the identity (tag, type, electrode membership) they had at that host call.  This one
 *     cannot be checked: an engine that sorts or exchanges atoms calls conp_fix_post_neighbor with host arrays.
 * What it rebuilds, each piece in the form and order of the host route (the kernels behind it are the same):
 *   1. the per-atom tables for the new nall: owned rows stay, the ghost rows of type and of the atom -> electrode-row table are copied
 *      from their owners;
 *   2. the charge scatter list: the (atom, row) pairs of owned and ghost electrode atoms in ascending atom index, and its CSR by
 *      electrode row -- per row the owned atom, then its ghosts in ascending ghost index;
 *   3. the fix's half list: device-to-device COPIES of the pair style's buffers, then the electrode rows of the real-space b regrouped
 *      from them.  Lifetime: the copies belong to the fix.  A later conp_pair_build_list_device (or conp_pair_set_list) replaces the
 *      pair style's list only; conp_fix_pre_force_device and conp_fix_post_force[_device] keep working with the list, the ghosts and the nall
 *      of THIS call until the next conp_fix_post_neighbor[_device] -- as after a host conp_fix_post_neighbor;
 *   4. the electrolyte list: owned atoms with no electrode row and q != 0, ascending.  (Owned atoms keep their identity, and every
 *      owned electrode atom of a handle that is not decomposed has a row: "no row" is the host's electrode_check == 0.);
 *   5. the z-window order, when the handle takes that path (conp_info.zn_cols): with n grid cells, gscale = n / lz and the owned z of
 *      the call, in double without contraction:  u = z gscale;  u -= n floor(u (1 / n));  c = (int)u, and c >= n: c = n - 1,
 *      u = nextafter(n, 0).  From the occupancy of the cells the start cell c0 behind the longest run of empty cells -- the ring is
 *      walked twice from cell 0, the first of several equally long runs wins, a box without an empty cell starts at 0.  The list is
 *      sorted by (c - c0) mod n with a STABLE counting sort: atoms of one cell keep ascending atom index.  Per chunk of 16 sorted
 *      atoms the lowest and highest  i0 = (int)ceil(ur - 7.5),  ur = u - c0 (+ n if negative).  The occupancy and the chunk bounds go
 *      to the host, which cuts the ranges and window origins from them exactly as conp_fix_post_neighbor does;
 *   6. a z-window flag that an earlier device-resident update raised is taken as conp_fix_post_neighbor takes it: the build is
 *      completed, then the call returns CONP_ERR_NUMERIC once (the handle is ready; repeat the update).
 * Contract: at most four stream synchronisations (the flag of the earlier updates; the two list lengths with the cell occupancy; the
 * chunk bounds, on the z-window path only; the closing one) and host traffic of O(grid cells + nl / 16 + schedule items) -- nothing
 * of the size of nall or of the pair count; device allocations only when something grew; a pure function of its input: two calls on
 * the same input leave byte-identical tables.
 * Host mirrors: the host copies of the lists (electrolyte list, scatter list, the fix's half list and its rows) are NOT refreshed.
 * Until the next conp_fix_post_neighbor with host arrays these entries return CONP_ERR_STATE, with a message that says so, instead of
 * computing with stale indices: conp_fix_pre_force, conp_fix_setup_pre_force, conp_fix_b_cal, conp_km_b_cal, conp_fix_update_charge,
 * conp_fix_post_force, conp_fix_post_force_step.  Entries that upload the atoms they are given and read no mirror keep working
 * (conp_pair_compute, the conp_ewald_* / conp_pppm_* entries, conp_compute_potential_atom, conp_fix_a_cal), and so does every device
 * entry: conp_fix_pre_force_device, conp_fix_b_cal_device / _solve_device / _scatter_device, the _device force entries,
 * conp_fix_post_force_device (below), conp_fix_compute_scalar, conp_fix_get_vectors.
 * conp_fix_get_step_tables downloads what (2) - (5) left on the device, after either route (synchronous; for tests).  sizes[8] =
 * {nl, electrode atoms in the scatter list, Ne, b-row pairs, chunk origins (nl padded to 32, / 16; 0 when the list is not z-ordered),
 * 1 if the list is z-ordered, nall, start cell}.  Arrays may be NULL: elyte_idx [nl], ele_pairs [2 sizes[1]], csr_ptr [Ne + 1],
 * csr_of / csr_row [sizes[1]], b_rowptr [Ne + 1], b_ele / b_oth [sizes[3]], g0c [sizes[4]] the window origin of every chunk. */
int conp_fix_post_neighbor_device(conp_fix *fix, const double *d_x /*[nall][3]*/, const double *d_q /*[nall]*/);
int conp_fix_get_step_tables(conp_fix *fix, int64_t *sizes /*[8] or NULL*/, int *elyte_idx, int *ele_pairs, int *csr_ptr, int *csr_of,
                             int *csr_row, int *b_rowptr, int *b_ele, int *b_oth, int *g0c);

/* ---- the Gaussian correction on the device -----------------------------------------------------------------
 * conp_fix_post_force_device is conp_fix_post_force for an engine whose atoms live on the device: the last hook of a step that
 * needed host arrays.  All pointers are device pointers laid out as for conp_pair_compute_device: owned atoms first, then ghosts;
 * the ghost rows of d_x and d_q must be filled (conp_ghost_fill_device); nall and nlocal are those of the last
 * conp_fix_post_neighbor[_device].  d_f [nall][3] is ADDED to -- there is no staging array, no flag and no read-back; with newton on
 * the term lands on ghost electrolyte atoms too, and the caller folds d_f with conp_ghost_fold_device.  d_out [9] is OVERWRITTEN:
 *   d_out[0]     what the reference adds to force->kspace->energy:  qqrd2e eta sum q^2 / (sqrt 2 sqrt pi) over the owned electrode
 *                atoms, with active EHGO  qqrd2e sum u0_type q^2  -- conp_fix_post_force's two expressions, same operations;
 *   d_out[1]     eng_coul_add;
 *   d_out[2..7]  the virial xx, yy, zz, xy, xz, yz;
 *   d_out[8]     the number of contributing pairs (inside the eta^2 r^2 < 5.8 gate), as a double: whether the term acted.
 * Either output may be NULL; with both NULL the call returns CONP_OK and does nothing.
 * The pair set and the arithmetic are conp_fix_post_force's: every listed pair of the FIX's half list with exactly one electrode
 * member (no newton / ghost filter on membership), `del*forcecoul`, the 5.8 gate on the fix's eta, the EHGO branch, the force on the
 * j side under newton or j < nlocal, the energy weights 1 / 0.5 / 0.5, no contraction.
 * It reads device tables only (the fix's list, the atom -> electrode-row table, the types, the real-space parameters), so it works
 * after a host conp_fix_post_neighbor and after conp_fix_post_neighbor_device alike (the stale host mirrors of section 19 do not
 * concern it), and a later conp_pair_build_list_device does not change what it walks (the lifetime rule above).
 * Order guarantee: energy, virial and the pair count meet no atomic -- every lane adds its pairs in list order, waves, workgroups and
 * the rows they store are added in a fixed order -- so d_out is byte-identical from call to call on the same input, and d_out[0] is
 * byte-identical to conp_fix_post_force's kspace_energy_add for the same charges.  Forces are added with atomics (contributions are
 * rare, and one atom can be several pairs' j): they reproduce to the rounding of those adds.
 * Contract: everything is enqueued on the handle's stream; after the first call at a given list size a call makes no device
 * allocation, no copy to the host and no synchronisation.  CONP_ERR_ARG: NULL d_x or d_q.  CONP_ERR_STATE: before setup; a decomposed
 * handle (conp_fix_set_comm: sum q^2 needs an all-reduce; replicated-atom rank handles compute locally).  A refused call changes
 * nothing.  The entry shares no state with conp_fix_post_force[_step], which behave as before.
 * A device step: conp_fix_pre_force_device -> conp_*_compute_forces_device -> conp_pair_compute_device ->
 * conp_fix_post_force_device -> conp_ghost_fold_device. */
int conp_fix_post_force_device(conp_fix *fix, const double *d_x /*[nall][3]*/, const double *d_q /*[nall]*/,
                               double *d_f /*[nall][3], added to; NULL: none*/, double *d_out /*[9], overwritten; NULL: none*/);

/* ---- atomic-free pair and Gaussian-correction forces --------------------------------------------------------
 * conp_pair_compute_device and conp_fix_post_force_device add forces (and eatom, vatom) with float atomics: those outputs reproduce
 * to rounding only.  The entries below are their twins without a float atomic: every output is byte-identical from call to call and
 * from run to run on the same input.  They need the TRANSPOSED list: a half list names each pair once, in its owner's row, and to sum
 * an atom's terms in a fixed order the atom must also find the pairs in which it is the j.
 * The transposed list of a flattened half list (inum, ilist, numneigh, first, neigh) over nall atoms is three device arrays:
 *   own_row  [nall]       the ii with ilist[ii] == a, or -1 (numneigh and first are read for listed owners only);
 *   tr_ptr   [nall + 1]   tr_ptr[a + 1] - tr_ptr[a] = the listed slots p = first[i] + jj with (neigh[p] & 0x3FFFFFFF) == a;
 *   tr_entry [n]          n = tr_ptr[nall] listed slots; for atom a its slots in ASCENDING SLOT ORDER p, each as
 *                         i | (neigh[p] & 0xC0000000): the owner with the special bits of that slot.
 * The arrays are a pure function of the list -- a stable sort of the listed slots by j --, byte-identical from build to build.
 * conp_pair_transpose_list_device transposes the pair style's list, uploaded (conp_pair_set_list) or built
 * (conp_pair_build_list[_exclude]_device): call it after the list at every re-neighbouring.  conp_fix_transpose_list_device
 * transposes the FIX's own half list: call it after conp_fix_(setup_)post_neighbor or conp_fix_post_neighbor_device.  Both may
 * allocate and synchronise (the slot count reaches the host), like the other re-neighbouring entries.  Without a list:
 * CONP_ERR_STATE.  An owner that occurs twice in ilist (or lies outside [0, nall)): CONP_ERR_ARG; 2^31 slots or more:
 * CONP_ERR_NUMERIC; a refused call leaves no index.  An index is dropped by whatever replaces its list: the pair style's by
 * conp_pair_set_list and both builds (refused ones too), the fix's by conp_fix_(setup_)post_neighbor and
 * conp_fix_post_neighbor_device.  The lifetime rule of section 19 carries over: a later pair-list build touches neither the fix's
 * list nor its index.
 * conp_pair_get_transposed_list downloads an index (synchronous; for tests): which 0 the pair style's, 1 the fix's; the sizes, and
 * with non-NULL arrays own_row [nall], tr_ptr [nall + 1], tr_entry [n].  which outside {0, 1}: CONP_ERR_ARG; no valid index of that
 * kind: CONP_ERR_STATE.
 *
 * conp_pair_compute_ordered_device: the signature, arguments, refusals and contract of conp_pair_compute_device (one stream; after
 * the first call at a list size no allocation, no copy to the host, no synchronisation; d_f added to, d_ev / d_eatom / d_vatom
 * overwritten; all outputs NULL: CONP_OK), and CONP_ERR_STATE when the pair style's index is missing or belongs to an earlier list.
 * The arithmetic of a pair is conp_pair_compute_device's, operation for operation; a pair gives j exactly the negative of what it
 * gives i.  SUMMATION ORDER, per atom a that can receive (every atom with newton on, a < nlocal with newton off), one wavefront of
 * 64 lanes:
 *   1. lane l adds, starting from +0.0, the terms of a's own row at jj = l, l + 64, ... (the pairs in which a is the owner: del =
 *      x_a - x_j, +del fpair), then the terms of a's transposed entries k = l, l + 64, ... counted from tr_ptr[a] (the pairs in which
 *      a is the j, evaluated in their OWNER's orientation: del = x_owner - x_a, types [type_owner][type_a], prefactor qqrd2e q_owner
 *      q_a / r; a receives -(del fpair), and the same half of eatom / vatom as the owner);
 *   2. the 64 lane sums are added by the shuffle tree  v += lane[l + 32]; += [l + 16]; += 8; 4; 2; 1  (lane 0 holds the result);
 *   3. lane 0 stores  out[a] = out[a] + sum  once per output.  A row is written exactly when the atomic entry writes it: a is a listed
 *      owner with a non-empty row, or the j of a listed pair inside its cutoff; every other row keeps its bytes, and with newton off
 *      no ghost row is written.
 * d_ev: the lane assignment over an owner's row is conp_pair_compute_device's, every owner's eight sums are stored as one row and the
 * rows are added by the same finishing kernel: d_ev is byte-identical to conp_pair_compute_device's for the same input.
 *
 * conp_fix_post_force_ordered_device: the signature, pair set, gates, EHGO branch and refusals of conp_fix_post_force_device, and
 * CONP_ERR_STATE without a valid index of the fix's list.  d_out is formed by conp_fix_post_force_device's own kernels: the same
 * bytes.  The forces are gathered per atom that is no electrode atom (the term lands on the pair's other member only), in the order
 * above: own row (+del forcecoul, no newton gate), then the transposed entries under newton || a < nlocal (-(del forcecoul), owner's
 * orientation), the shuffle tree, one plain add per atom with a contributing pair.  The membership test precedes every coordinate
 * load.
 * A reproducible device step: conp_fix_pre_force_device -> conp_ewald_compute_forces_device -> conp_pair_compute_ordered_device ->
 * conp_fix_post_force_ordered_device -> conp_ghost_fold_device.  (The PPPM mesh spread still uses float atomics.) */
int conp_pair_transpose_list_device(conp_fix *fix);
int conp_fix_transpose_list_device(conp_fix *fix);
int conp_pair_get_transposed_list(conp_fix *fix, int which, int *nall, int64_t *n, int *own_row, int *tr_ptr, int *tr_entry);
int conp_pair_compute_ordered_device(conp_fix *fix, const double *d_x, const double *d_q,
                                     double *d_f /*[nall][3], added to; NULL: none*/, double *d_ev /*[8]; NULL ok*/,
                                     double *d_eatom /*[nall]; NULL ok*/, double *d_vatom /*[nall][6]; NULL ok*/);
int conp_fix_post_force_ordered_device(conp_fix *fix, const double *d_x /*[nall][3]*/, const double *d_q /*[nall]*/,
                                       double *d_f /*[nall][3], added to; NULL: none*/, double *d_out /*[9], overwritten; NULL: none*/);

/* ---- `compute potential/atom` on the device -----------------------------------------------------------------
 * conp_compute_potential_atom without the host: device pointers in the layout of conp_fix_pre_force_device, everything enqueued on
 * the handle's stream; after the first call at a given size no device allocation, no copy to the host, no synchronisation.
 * Rank-local, on one rank: a decomposed handle (conp_fix_set_comm) gets CONP_ERR_STATE.
 * ntotal = nlocal + (newton_pair ? nghost : 0) of the last (setup_)post_neighbor[_device].
 * d_flags [nall]: bit 0 -- the row is selected (mask & groupbit); bit 1 -- eta_check.  The caller keeps its ghost rows with
 * conp_ghost_fill_int_device, like tag and mask.  d_targets [ntargets]: the selected OWNED rows, ascending; it must name exactly
 * the owned rows with bit 0 set -- not checked.
 * RESULT.  A selected row of [0, ntotal) gets what conp_compute_potential_atom gives that row, in volts; every other row of
 * [0, ntotal) is written 0.0 (the reference clears the array; the host entry's partial sums on unselected rows are not reproduced);
 * rows from ntotal on are not touched.  With newton on a ghost row holds its pair partial times qqr2e / qe2f: the caller finishes
 * with conp_ghost_fold_device(fix, d_pot, 1), as for d_eatom.
 * PAIR PART (args->pairflag): over the pair style's current list (conp_pair_set_list or either device build) and its transposed
 * index (conp_pair_transpose_list_device); without a list, or with an index that is missing or belongs to an earlier list:
 * CONP_ERR_STATE, as conp_pair_compute_ordered_device.  Constants and types are the host entry's: the fix's cutsq table, the
 * reference's min(cut_coul, 5.8 / g)^2, env.g_ewald, the types of the last post_neighbor.  The arithmetic of a pair is the host
 * entry's, operation for operation, no contraction: rsq floored at 1e-10, both cutoff tests, the five-term erfc polynomial, the
 * eta branch with ne2 = eta bit of owner + eta bit of neighbour behind its 5.8 gate; special bits are masked off and ignored.  No
 * float atomic: each selected row a is gathered by one wavefront in the order of section 26 -- own row jj = l, l + 64, ... with the
 * term q_j dudq, then the transposed entries from tr_ptr[a] with the term q_owner dudq at rsq in the owner's orientation, the
 * shuffle tree, one store.  A partner with q == 0 contributes nothing.  Unselected rows do no pair work.  Every byte of d_pot is
 * the same from call to call and from run to run on an Ewald handle.
 * K-SPACE PART (args->kspaceflag), on the ntargets owned targets: u_i of conp_ewald_compute_particle_potential on an Ewald handle
 * (the exact sum over every owned atom of the call), the mesh potential of conp_pppm_compute_particle_potential on a `pppm` handle
 * (the brick of every owned atom; its spread uses float atomics).  Then, in the host entry's order,
 *   pot = (((pair - u) + [eta bit] eta q sqrt(2) / sqrt(pi)) + z slabcorr) - [qsumflag] (2 pi / V) Q z^2,   times qqr2e / qe2f,
 * under env.slabflag with slabcorr = 2 (2 pi / V) M; Q = sum q and M = sum q z over the owned atoms of the call, summed on the
 * device in a fixed order.
 * reuse_kspace != 0 skips the structure factor (the mesh solve) and projects from what the last device k-space force entry left on
 * this handle: conp_ewald_compute_forces[_vatom]_device, or conp_pppm_compute_forces[_vatom]_device called with d_f or d_eatom --
 * the per-step case update -> forces -> potential at the same x and q.  The handle keeps one validity bit: those entries set it;
 * every update, every re-neighbouring entry, set_matrix, new k tables, the host query entries (conp_ewald_* / conp_pppm_* with host
 * arrays, conp_compute_potential_atom) and a call of this entry without reuse clear it.  Reuse without a valid bit:
 * CONP_ERR_STATE, nothing changed.  As with the cached S above, the handle cannot tell that atoms moved or charges changed without
 * an update: reusing after that is the caller's error and returns CONP_OK.  With or without reuse the force entries' next call is
 * unaffected.
 * REFUSALS.  CONP_ERR_ARG: NULL fix, d_x, d_q or args; ntargets < 0 or > nlocal; NULL d_targets with ntargets > 0; NULL d_flags
 * when the pair part runs or eta != 0.  CONP_ERR_STATE: before (setup_)post_neighbor, and the cases above.  NULL d_pot: CONP_OK,
 * nothing done.  Both flags zero: [0, ntotal) is zeroed.
 * A step with the potentials: ... -> conp_ghost_fold_device(d_f, 3) -> conp_potential_atom_device(reuse_kspace = 1) ->
 * conp_ghost_fold_device(d_pot, 1). */
int conp_potential_atom_device(conp_fix *fix, const double *d_x /*[nall][3]*/, const double *d_q /*[nall]*/,
                               const int *d_flags /*[nall]: bit 0 selected (mask & groupbit), bit 1 eta_check*/,
                               int ntargets, const int *d_targets /*[ntargets] selected OWNED atoms, ascending*/,
                               const conp_potential_args *args, int reuse_kspace, double *d_pot /*[ntotal], overwritten*/);

/* ---- bonded forces: `bond_style harmonic` and `angle_style harmonic` on the device -------------------------
 * The bond and angle loops of LAMMPS' bond_harmonic.cpp and angle_harmonic.cpp @ 27May2021 with Bond::ev_tally's and
 * Angle::ev_tally's energy, virial and per-atom tallies.  All arithmetic is double, in the order written, no contraction.
 * newton = newton_bond of conp_bonded_set_params; nlocal, nall, prd those of conp_bonded_set_lists.
 * Closest image of x_b seen from x_a, per dimension c with prd[c] > 0:  d = x_a[c] - x_b[c];  s = +1 if d > prd[c] / 2, s = -1 if
 * d < -prd[c] / 2, else s = 0;  x_b'[c] = x_b[c] + ((double)s * prd[c])  -- the product first, then the sum, also for s = 0: the ghost
 * arithmetic of conp_ghost_fill_device, so an image has the bits a ghost would have.  One pass: partners more than 1.5 box lengths
 * apart are the caller's error.  With prd[c] = 0: x_b'[c] = x_b[c].
 * Bond (i1, i2, t), x2' the closest image of x2 from x1:
 *   del = x1 - x2';  rsq = delx^2 + dely^2 + delz^2;  r = sqrt(rsq);  dr = r - r0[t];  rk = k[t] dr
 *   fbond = (r > 0) ? -2 rk / r : 0;  ebond = rk dr
 *   f[i1] += del fbond  if newton or i1 < nlocal;   f[i2] -= del fbond  if newton or i2 < nlocal
 *   v = fbond (delx^2, dely^2, delz^2, delx dely, delx delz, dely delz)
 *   Tally: with newton ebond and v are counted whole, else ebond / 2 and v / 2 once per owned member.  eatom gets ebond / 2 and vatom
 *   v / 2, for i1 and for i2, each under the force's condition.
 * Angle (i1, i2, i3, t), i2 the centre, x1' and x3' the closest images from x2:
 *   del1 = x1' - x2;  del2 = x3' - x2;  rsq1 = |del1|^2;  rsq2 = |del2|^2;  r1 = sqrt(rsq1);  r2 = sqrt(rsq2)
 *   c = (del1 . del2) / (r1 r2), clamped to [-1, 1];  s = sqrt(1 - c c);  if s < 0.001: s = 0.001;  s = 1 / s
 *   dtheta = acos(c) - theta0[t];  tk = k[t] dtheta;  eangle = tk dtheta
 *   a = -2 tk s;  a11 = a c / rsq1;  a12 = -a / (r1 r2);  a22 = a c / rsq2
 *   f1 = a11 del1 + a12 del2;  f3 = a22 del2 + a12 del1
 *   f[i1] += f1;  f[i2] -= f1 + f3;  f[i3] += f3,  each if newton or i < nlocal
 *   v = (delx1 f1x + delx2 f3x, dely1 f1y + dely2 f3y, delz1 f1z + delz2 f3z,
 *        delx1 f1y + delx2 f3y, delx1 f1z + delx2 f3z, dely1 f1z + dely2 f3z)
 *   Tally: whole with newton, else (1.0 / 3.0) eangle and (1.0 / 3.0) v once per owned member.  eatom gets eangle (1.0 / 3.0) and
 *   vatom v (1.0 / 3.0) per member, under the force's condition.
 * Hence with newton sum eatom = ebond + eangle and sum vatom = virial.
 * The two ways to hand over lists:
 *   - a LAMMPS-like host passes neighbor->bondlist / anglelist with ghost indices and prd = {0, 0, 0} at every re-neighbour; the ghost
 *     rows of f, eatom, vatom then carry what the reverse communication (conp_ghost_fold_device) folds back;
 *   - a device-resident engine passes owned indices and the box lengths ONCE: nothing lands on a ghost row, no fold is needed, and
 *     the lists survive every device re-neighbour for as long as the owned atoms keep their local order and identity -- the
 *     precondition conp_fix_post_neighbor_device already has.
 * Order and reproducibility: no output meets an atomic.  conp_bonded_set_lists builds a per-atom table of the (term, role) slots an
 * atom takes part in, bonds first in list order, then angles in list order; an atom's contributions to f, eatom and vatom are summed
 * from 0.0 by one thread in that order and added to f once; energy and virial are added over terms in a fixed order.  Every output
 * is a pure function of the input: byte-identical from call to call and between the host and the device entry.  Rows of atoms in
 * no term (or, with newton off, of ghosts): f is untouched bit for bit, eatom / vatom are exactly 0.0.
 * Order: conp_bonded_set_params (once per run, or after bond_coeff / angle_coeff changes) -> conp_bonded_set_lists -> the compute
 * entries.  CONP_ERR_STATE: a compute entry before set_params or set_lists; set_lists before set_params.  conp_bonded_set_params
 * after conp_bonded_set_lists DROPS the lists (they were checked against the old tables): set them again.
 * CONP_ERR_ARG: a NULL struct; a NULL array with a positive count; a negative count; nlocal > nall; an index outside [0, nall); a
 * type outside [1, ntypes]; a negative or non-finite prd; NULL d_x / atoms; atoms->nlocal + nghost != nall.  A refused
 * conp_bonded_set_lists leaves the handle without lists.  All outputs NULL: CONP_OK, nothing done.  Empty lists: the outputs are
 * zeroed, f is untouched.
 * The entries need nothing of the fix but its stream: they work from conp_fix_create on, on Ewald and `pppm` handles, and they are
 * rank-local, never collective (decomposed handles are allowed).
 * Device entry: everything is enqueued on the handle's stream; conp_bonded_set_lists reserves all scratch, so a compute call makes
 * no device allocation, no copy to the host and no synchronisation.  A device step: conp_ghost_fill_device ->
 * conp_fix_pre_force_device -> conp_*_compute_forces_device -> conp_pair_compute_device -> conp_bonded_compute_device ->
 * conp_fix_post_force_device -> conp_ghost_fold_device.
 * Host entry: stages atoms->x (only x is read), is synchronous and adds into f. */
typedef struct {
  int nbondtypes, nangletypes;          /* either may be 0 */
  const double *bond_k, *bond_r0;       /* [nbondtypes + 1], entry 0 unused (bond_coeff K r0) */
  const double *angle_k, *angle_theta0; /* [nangletypes + 1], theta0 in RADIANS (LAMMPS converts at angle_coeff) */
  int newton_bond;                      /* force->newton_bond */
} conp_bonded_params;

typedef struct {
  int nlocal, nall;                     /* every index below is < nall; i < nlocal is an owned atom */
  int nbond;  const int *bond;          /* [nbond][3]  i1, i2, type      -- neighbor->bondlist */
  int nangle; const int *angle;         /* [nangle][4] i1, i2, i3, type  -- neighbor->anglelist, i2 the centre */
  double prd[3];                        /* > 0: closest image in that dimension (above); 0: coordinates as they are */
} conp_bonded_lists;

int conp_bonded_set_params(conp_fix *fix, const conp_bonded_params *p);   /* copied */
int conp_bonded_set_lists(conp_fix *fix, const conp_bonded_lists *l);     /* host arrays, copied and uploaded; may allocate and synchronise */
int conp_bonded_compute(conp_fix *fix, const conp_atoms *atoms, double *f /*[nall][3] accumulated*/, double *eng /*[2] ebond, eangle*/,
                        double *virial /*[6]*/, double *eatom /*[nall] overwritten*/, double *vatom /*[nall][6] overwritten*/);
int conp_bonded_compute_device(conp_fix *fix, const double *d_x /*[nall][3]*/, double *d_f /*[nall][3] accumulated*/,
                               double *d_ev /*[8] ebond, eangle, virial xx,yy,zz,xy,xz,yz; overwritten*/,
                               double *d_eatom /*[nall]*/, double *d_vatom /*[nall][6]*/);

/* ---- torsional forces: `dihedral_style opls | harmonic` and `improper_style harmonic | cvff` on the device --
 * What an all-atom force field (OPLS-AA, CL&P, ...) adds to the bonds and angles above.  The 1-4 pair scaling of such a force field
 * is the pair list's business: it travels in the special bits of the pair entries (special_lj / special_coul) and is not touched
 * here.  A sibling of the conp_bonded_* entries with the same contract; this text is the definition, one geometry for all four
 * styles.  All arithmetic is double, in the order written (sums and products left to right), no contraction.
 * newton = newton_bond of conp_dihedral_set_params; nlocal, nall, prd those of conp_dihedral_set_lists.
 * Term (i1, i2, i3, i4, t), of either list.  Images by the closest-image rule of the bonded block above, bit for bit:
 *   x1' the closest image of x1 seen from x2;  x3' that of x3 seen from x2;  x4' that of x4 seen from x3'.
 *   F = x1' - x2;  G = x2 - x3';  H = x4' - x3'
 *   A = F x G = (Fy Gz - Fz Gy, Fz Gx - Fx Gz, Fx Gy - Fy Gx);  B = H x G likewise;  C = B x A likewise
 *   A2 = Ax Ax + Ay Ay + Az Az;  B2 = B . B;  g = sqrt(G . G)          (every dot product: x + y, then + z)
 *   Degenerate term, A2 == 0 or B2 == 0 or g == 0 (collinear members): the term contributes exactly nothing -- its forces, its
 *   energy and its virial are 0.0.
 *   phi = atan2((C . G) / g, A . B)                      trans is pi, cis is 0: LAMMPS' convention for these styles
 *   Gradient of phi:  ga = g / A2;  gb = g / B2;  sa = (F . G) / (A2 g);  sb = (H . G) / (B2 g)
 *     d1 = -(ga A);  d4 = gb B;  s = sa A - sb B;  d3 = (-d4) - s;  (d2 = (-d1) + s is not formed)
 *   With the style's energy e(phi) and derivative de(phi) below and p = -de:
 *     f1 = p d1;  f3 = p d3;  f4 = p d4;  f2 = -((f1 + f3) + f4)
 *     f[i_m] += f_m  if newton or i_m < nlocal
 *     v = six(F, f1) + six(-G, f3) + six(H - G, f4),  six(u, w) = (ux wx, uy wy, uz wz, ux wy, ux wz, uy wz): the form of
 *     Dihedral::ev_tally, sum over the members of (x_m - x_2) (x) f_m
 *   Tally: with newton e and v are counted whole, else 0.25 e and 0.25 v once per owned member.  eatom gets 0.25 e and vatom 0.25 v
 *   per member, each under the force's condition.  Hence with newton sum eatom = edihedral + eimproper and sum vatom = virial.
 * This formulation has no 1 / sin(phi) and needs no clamp; it is exact to rounding through phi = 0 and phi = pi.
 * Styles (the coefficient rows are [4] per type, row 0 unused):
 *   dihedral opls, K1 K2 K3 K4 as dihedral_coeff gives them (the halves are applied here); s_k = sin(k phi), c_k = cos(k phi) with
 *     the argument formed as (double)k * phi:
 *     e  = 0.5 (K1 (1 + c_1) + K2 (1 - c_2) + K3 (1 + c_3) + K4 (1 - c_4))
 *     de = 0.5 (2 (K2 s_2) - K1 s_1 - 3 (K3 s_3) + 4 (K4 s_4))
 *   dihedral harmonic and improper cvff, K d n (d = +1 or -1, n an integer):  a = n phi
 *     e = K (1 + d cos(a));  de = -(K d n sin(a))
 *   improper harmonic, K chi0 (chi0 in RADIANS):  u = fabs(phi) - chi0
 *     e = K u u;  de = 2 K (phi - copysign(chi0, phi))         LAMMPS' acos(c) - chi0, smooth through the planar minimum
 * n: 0..6 for cvff (LAMMPS' range); 0..CONP_DIHEDRAL_MAX_N for dihedral harmonic.
 * The two ways to hand over lists are those of the bonded block: neighbor->dihedrallist / improperlist with ghost indices and
 * prd = {0, 0, 0} at every re-neighbour, or owned indices and the box lengths once.
 * Order and reproducibility: no output meets an atomic.  conp_dihedral_set_lists builds a per-atom table of the (term, role) slots
 * an atom takes part in, dihedrals first in list order, then impropers in list order, the roles of a term in member order; an atom's
 * contributions to f, eatom and vatom are summed from 0.0 by one thread in that order and added to f once; energy and virial are
 * added over terms in a fixed order.  Every output is a pure function of the input: byte-identical from call to call and between
 * the host and the device entry.  Rows of atoms in no term (or, with newton off, of ghosts): f is untouched bit for bit, eatom /
 * vatom are exactly 0.0.
 * Order: conp_dihedral_set_params (once per run, or after dihedral_coeff / improper_coeff changes) -> conp_dihedral_set_lists -> the
 * compute entries.  CONP_ERR_STATE: a compute entry before set_params or set_lists; set_lists before set_params.
 * conp_dihedral_set_params after conp_dihedral_set_lists DROPS the lists (they were checked against the old tables): set them again.
 * CONP_ERR_ARG: a NULL struct; a NULL array with a positive count; a negative count; nlocal > nall; an index outside [0, nall); a
 * type outside [1, ntypes]; an unknown style; a positive type count or a non-empty list for a style that is 0; a coefficient that
 * is not finite; d other than +1 or -1; n not an integer or outside its range above; a negative or non-finite prd; NULL d_x /
 * atoms; atoms->nlocal + nghost != nall.  A refused conp_dihedral_set_lists leaves the handle without lists; a refused
 * conp_dihedral_set_params leaves tables and lists as they were.  All outputs NULL: CONP_OK, nothing done.  Empty lists: the
 * outputs are zeroed, f is untouched.
 * The entries need nothing of the fix but its stream: they work from conp_fix_create on, on Ewald and `pppm` handles, and they are
 * rank-local, never collective (decomposed handles are allowed).
 * Device entry: everything is enqueued on the handle's stream; conp_dihedral_set_lists reserves all scratch, so a compute call
 * makes no device allocation, no copy to the host and no synchronisation.  A device step: ... -> conp_pair_compute_device ->
 * conp_bonded_compute_device -> conp_dihedral_compute_device -> conp_fix_post_force_device -> conp_ghost_fold_device.
 * Host entry: stages atoms->x (only x is read), is synchronous and adds into f.
 * Out of scope: dihedral charmm (its 1-4 weights), multi/harmonic, fourier, class2, hybrid; SHAKE flag 4. */
#define CONP_DIHEDRAL_MAX_N 12          /* the largest multiplicity n of `dihedral_style harmonic` */
typedef struct {
  int dihedral_style;                   /* 0 none, 1 opls, 2 harmonic */
  int ndihedraltypes;                   /* 0 with style 0 */
  const double *dihedral_coef;          /* [ndihedraltypes + 1][4], row 0 unused: opls K1 K2 K3 K4; harmonic K, d, n, 0 */
  int improper_style;                   /* 0 none, 1 harmonic, 2 cvff */
  int nimpropertypes;                   /* 0 with style 0 */
  const double *improper_coef;          /* [nimpropertypes + 1][4], row 0 unused: harmonic K, chi0 (RADIANS), 0, 0; cvff K, d, n, 0 */
  int newton_bond;                      /* force->newton_bond */
} conp_dihedral_params;

typedef struct {
  int nlocal, nall;                     /* every index below is < nall; i < nlocal is an owned atom */
  int ndihedral; const int *dihedral;   /* [ndihedral][5] i1, i2, i3, i4, type  -- neighbor->dihedrallist */
  int nimproper; const int *improper;   /* [nimproper][5] i1, i2, i3, i4, type  -- neighbor->improperlist */
  double prd[3];                        /* as conp_bonded_lists */
} conp_dihedral_lists;

int conp_dihedral_set_params(conp_fix *fix, const conp_dihedral_params *p);   /* copied */
int conp_dihedral_set_lists(conp_fix *fix, const conp_dihedral_lists *l);     /* host arrays, copied and uploaded; may allocate and synchronise */
int conp_dihedral_compute(conp_fix *fix, const conp_atoms *atoms, double *f /*[nall][3] accumulated*/,
                          double *eng /*[2] edihedral, eimproper*/, double *virial /*[6]*/, double *eatom /*[nall] overwritten*/,
                          double *vatom /*[nall][6] overwritten*/);
int conp_dihedral_compute_device(conp_fix *fix, const double *d_x /*[nall][3]*/, double *d_f /*[nall][3] accumulated*/,
                                 double *d_ev /*[8] edihedral, eimproper, virial xx,yy,zz,xy,xz,yz; overwritten*/,
                                 double *d_eatom /*[nall]*/, double *d_vatom /*[nall][6]*/);

/* ---- time integration: `fix nve` and `fix nvt` on the device ------------------------------------------------
 * Velocity Verlet with one Nose-Hoover chain per thermostatted group: LAMMPS' FixNH / FixNVE / ComputeTemp @ 27May2021 at the
 * reference decks' keywords (`fix ID group nvt temp Tstart Tstop Tdamp`: tchain 3, tloop 1, drag 0, no barostat, per-type masses, no
 * bias).  All arithmetic is double, in the order written (products left to right), no contraction.
 * An atom i < nlocal belongs to at most one group g = group[i] (-1: not integrated, the electrode of the decks).  Per group: style
 * (nve or nvt), dof, t_period, and on the device the chain state eta[3], eta_dot[3], eta_dotdot[3], t_current, t_target.  eta_dot[3]
 * below is the constant 0 behind the chain's end.
 * Constants: dtv = dt;  dtf = 0.5 dt ftm2v;  dthalf = 0.5 dt;  dt4 = 0.25 dt;  dt8 = 0.125 dt;  t_freq = 1 / t_period;
 *   kt = boltz t_target;  ke_target = dof kt.
 * temp(g):  t = sum over the atoms i of g of (vx^2 + vy^2 + vz^2) mass[type[i]];  t_current = t (mvv2e / (dof boltz)).
 *   (LAMMPS adds in ascending i; the library adds per workgroup and then over workgroups, in a fixed order of its own.)
 * nve_v:  dtfm = dtf / mass[type[i]];  v += dtfm f.        nve_x:  x += dtv v.
 * Masses:  eta_mass[0] = dof kt / t_freq^2;  eta_mass[k >= 1] = kt / t_freq^2   (kt from the STORED t_target).
 * Setup (conp_integrate_setup_device):  t_current = temp(g) for every group; for an nvt group also: store t_target, the masses,
 *   eta_dotdot[k >= 1] = (eta_mass[k-1] eta_dot[k-1]^2 - kt) / eta_mass[k].
 * Initial (conp_integrate_initial_device), per group:  nvt: store t_target, the chain half-step, v *= factor_eta;  then nve_v, nve_x.
 * Final (conp_integrate_final_device), per group:  nve_v;  t_current = temp(g);  nvt: the chain half-step, v *= factor_eta.
 * Chain half-step (FixNH::nhc_temp_integrate):
 *    1. the masses from the stored t_target
 *    2. eta_dotdot[0] = (dof boltz t_current - ke_target) / eta_mass[0]
 *    3. for k = 2, 1:  e = exp(-dt8 eta_dot[k+1]);  eta_dot[k] *= e;  eta_dot[k] += eta_dotdot[k] dt4;  eta_dot[k] *= e
 *    4. e = exp(-dt8 eta_dot[1]);  eta_dot[0] *= e;  eta_dot[0] += eta_dotdot[0] dt4;  eta_dot[0] *= e
 *    5. factor_eta = exp(-dthalf eta_dot[0])
 *    6. t_current *= factor_eta factor_eta      (the temperature of the scaled velocities, not summed again)
 *    7. eta_dotdot[0] as in 2, from the new t_current
 *    8. eta[k] += dthalf eta_dot[k], k = 0, 1, 2
 *    9. eta_dot[0] *= e;  eta_dot[0] += eta_dotdot[0] dt4;  eta_dot[0] *= e      (e of step 4)
 *   10. for k = 1, 2:  e = exp(-dt8 eta_dot[k+1]);  eta_dot[k] *= e;
 *                      eta_dotdot[k] = (eta_mass[k-1] eta_dot[k-1]^2 - kt) / eta_mass[k];  eta_dot[k] += eta_dotdot[k] dt4;  eta_dot[k] *= e
 * Thermostat energy (FixNH::compute_scalar):  ke_target eta[0] + 0.5 eta_mass[0] eta_dot[0]^2
 *                                             + sum over k >= 1 of (kt eta[k] + 0.5 eta_mass[k] eta_dot[k]^2).
 * d_out [ngroups][4], overwritten, per group:  t_current;  ke = 0.5 mvv2e t;  the thermostat energy;  eta_dot[0].
 *   conp_integrate_temperature_device: temp(g) and ke of d_v as it is, energy and eta_dot[0] of the chain as it is; nothing is stored.
 *   conp_integrate_final_device: the values of the velocities the entry leaves: t_current after step 6 and, formed the same way,
 *   ke = (0.5 mvv2e t) (factor_eta factor_eta), t summed after nve_v.  For an nve group factor_eta is 1 and is not applied; its
 *   thermostat energy and eta_dot[0] are exactly 0.0.  A group without atoms: t_current and ke are exactly 0.0.
 * t_target is a HOST array [ngroups], read at call time and passed to the kernels by value: the engine evaluates the ramp
 *   Tstart -> Tstop.  Entries of nve groups are checked and otherwise unused.
 * State (conp_integrate_get_state / _set_state): [ngroups][8] per group eta[3], eta_dot[3], t_current, t_target -- what FixNH writes
 *   to a restart file, plus the two temperatures.  Both are host entries and synchronise.  set_state seeds every group's row,
 *   forms eta_dotdot[k >= 1] as setup does (a finished half-step leaves exactly these values, so a handle seeded with another's
 *   get_state continues byte for byte) and counts as the setup; call conp_integrate_setup_device after it to take t_current from the
 *   velocities instead, as a LAMMPS restart does.  Rows of nve groups: eta and eta_dot are stored as 0.
 * Order: conp_integrate_set_params (copies and uploads the arrays, reserves all scratch, zeroes every chain; may allocate and
 *   synchronise; afterwards the owned atoms keep their local order, the precondition conp_fix_post_neighbor_device already has) ->
 *   conp_integrate_setup_device (once per run, with the velocities of the run's start) -> per step conp_integrate_initial_device ->
 *   the force entries -> conp_integrate_final_device.  A device step: conp_integrate_initial_device -> conp_ghost_fill_device ->
 *   conp_fix_pre_force_device -> ... -> conp_ghost_fold_device -> conp_integrate_final_device.
 * CONP_ERR_STATE: any other entry before conp_integrate_set_params; initial or final before setup (or set_state) when a group is nvt.
 * CONP_ERR_ARG: a NULL struct or array; ngroups outside [1, CONP_INTEGRATE_MAX_GROUPS]; nlocal < 0; a type outside [1, ntypes]; a
 *   group outside [-1, ngroups); a style other than 0 and 1; a mass, dt, ftm2v, mvv2e, boltz, dof or (nvt) t_period that is not
 *   positive and finite; a t_target that is negative or not finite, or 0 for an nvt group; a state entry that is not finite; a NULL
 *   d_x, d_v or d_f.  A refused conp_integrate_set_params leaves the handle WITHOUT an integrator; every other refused call changes
 *   nothing.  nlocal == 0: CONP_OK, nothing advances, d_out is zeroed.  d_out NULL: conp_integrate_final_device writes none,
 *   conp_integrate_temperature_device does nothing.
 * Reproducibility: no sum meets an atomic; every output is a pure function of the input and the state, byte-identical from run to
 *   run.  Atoms with group -1 and rows from nlocal on are neither read nor written: x and v stay bit for bit.
 * The step entries enqueue on the handle's stream and make no device allocation, no copy to the host and no synchronisation.
 * They need nothing of the fix but its stream: they work from conp_fix_create on, on Ewald and `pppm` handles, and are rank-local,
 * never collective (decomposed handles are allowed: a group's temperature is then this rank's).
 * There are no host-array twins of the step entries: a host engine has its own integrator and would gain nothing from staging
 * x, v and f through the device. */
#define CONP_INTEGRATE_MAX_GROUPS 8
#define CONP_INTEGRATE_CHAIN 3                 /* LAMMPS' default tchain; tloop = 1, drag = 0 */
typedef struct {
  int nlocal, ntypes, ngroups;                 /* 1 <= ngroups <= CONP_INTEGRATE_MAX_GROUPS */
  const int *type;                             /* [nlocal], 1..ntypes                       */
  const int *group;                            /* [nlocal], -1 = not integrated, else 0..ngroups-1 */
  const double *mass;                          /* [ntypes + 1], entry 0 unused, > 0, finite  */
  const int *style;                            /* [ngroups] 0 = nve, 1 = nvt                 */
  const double *dof;                           /* [ngroups] temperature->dof of the group (the engine subtracts extra_dof and constraints) */
  const double *t_period;                      /* [ngroups] Tdamp; read for nvt groups only  */
  double dt, ftm2v, mvv2e, boltz;              /* update->dt and force->...                   */
} conp_integrate_params;

int conp_integrate_set_params(conp_fix *fix, const conp_integrate_params *p);
int conp_integrate_setup_device(conp_fix *fix, const double *d_v /*[nlocal][3]*/, const double *t_target /*HOST [ngroups]*/);
int conp_integrate_initial_device(conp_fix *fix, double *d_x /*[nlocal][3]*/, double *d_v /*[nlocal][3]*/, const double *d_f /*[nlocal][3]*/,
                                  const double *t_target /*HOST [ngroups]*/);
int conp_integrate_final_device(conp_fix *fix, double *d_v /*[nlocal][3]*/, const double *d_f /*[nlocal][3]*/,
                                double *d_out /*[ngroups][4], overwritten; NULL: none*/);
int conp_integrate_temperature_device(conp_fix *fix, const double *d_v /*[nlocal][3]*/, double *d_out /*[ngroups][4], overwritten*/);
int conp_integrate_get_state(conp_fix *fix, double *state /*HOST [ngroups][8]*/);
int conp_integrate_set_state(conp_fix *fix, const double *state /*HOST [ngroups][8]*/);

/* ---- constraints: `fix shake` on the device -----------------------------------------------------------------
 * Bond and angle constraints of small clusters: LAMMPS' FixShake @ 27May2021 at the reference decks' keywords (`fix ID group shake
 * tol iter 0 t ... b ... [a ...]`), without rRESPA, per-atom rmass or RATTLE.  All arithmetic is double, in the order written
 * (products left to right), no contraction.
 * Clusters: [ncluster][7] = flag, i0, i1, i2, t0, t1, t2 with LAMMPS' shake_flag:
 *   flag 2: one bond i0-i1 of length d0 = bond_distance[t0];
 *   flag 3: two bonds from the centre i0: i0-i1 (d0 = bond_distance[t0]) and i0-i2 (d1 = bond_distance[t1]);
 *   flag 1: the two bonds of flag 3 and the angle: the distance i1-i2 is d2 = angle_distance[t2]
 *           (= sqrt(d0^2 + d1^2 - 2 d0 d1 cos(theta0)) of the angle type).
 *   Fields a flag does not use are ignored.  Flag 4 (three bonds) is refused.  Every index is an owned atom in [0, nlocal), the
 *   indices of a cluster are distinct and an atom belongs to AT MOST ONE cluster: conp_shake_set_params checks all of it, and
 *   because of it no output meets an atomic.  The engine subtracts 1, 2 or 3 from a group's dof per cluster of flag 2, 3 or 1.
 * Constants:  dtv = dt;  dtfsq = dt dt ftm2v in conp_shake_post_force_device, dtfsq = 0.5 dt dt ftm2v in conp_shake_setup_device and
 *   conp_shake_correct_device;  im_k = 1.0 / mass[type[i_k]];  dtfmsq_k = dtfsq / mass[type[i_k]].
 * Difference a - b with minimum image, per dimension c:  d = a[c] - b[c];  where prd[c] > 0 and fabs(d) > 0.5 prd[c]:  d += prd[c] if
 *   d < 0, else d -= prd[c].  One pass, for r and s alike.
 * Unconstrained position of a cluster atom:  xs = x + dtv v + dtfmsq f  (left to right), formed in the cluster's thread; for
 *   conp_shake_correct_device v and f count as 0 and xs = x.
 * r01 = x0 - x1, r02 = x0 - x2, r12 = x1 - x2;  s01, s02, s12 the same differences of xs;  rNNsq, sNNsq their squares (x x + y y + z z),
 *   r0102 = r01 . r02, r0112 = r01 . r12, r0212 = r02 . r12, and s.r dot products the same way.
 * Flag 2:  a = (im0 + im1) (im0 + im1) r01sq;  b = 2.0 (im0 + im1) (s01 . r01);  c = s01sq - d0 d0;  determ = b b - 4.0 a c;
 *   determ < 0: determ = 0, counted;  lamda = (-b + sqrt(determ)) / (2.0 a) if b > 0, else (-b - sqrt(determ)) / (2.0 a);
 *   lamda /= dtfsq;  f0 += lamda r01;  f1 -= lamda r01;
 *   v = lamda (r01x r01x, r01y r01y, r01z r01z, r01x r01y, r01x r01z, r01y r01z), each (lamda r_a) r_b.
 * Flag 3:  a11 = 2.0 (im0 + im1) (s01 . r01);  a12 = 2.0 im0 (s01 . r02);  a21 = 2.0 im0 (s02 . r01);  a22 = 2.0 (im0 + im2) (s02 . r02);
 *   determ = a11 a22 - a12 a21;  determ == 0: the cluster adds nothing and is counted (LAMMPS aborts; a kernel cannot);
 *   determinv = 1.0 / determ;  a11inv = a22 determinv;  a12inv = -a12 determinv;  a21inv = -a21 determinv;  a22inv = a11 determinv;
 *   quad1_0101 = (im0 + im1) (im0 + im1) r01sq;  quad1_0202 = im0 im0 r02sq;  quad1_0102 = 2.0 (im0 + im1) im0 r0102;
 *   quad2_0202 = (im0 + im2) (im0 + im2) r02sq;  quad2_0101 = im0 im0 r01sq;  quad2_0102 = 2.0 (im0 + im2) im0 r0102;
 *   lamda01 = lamda02 = 0, niter = 0, done = false;  while not done and niter < max_iter:
 *     quad1 = quad1_0101 l01 l01 + quad1_0202 l02 l02 + quad1_0102 l01 l02;  quad2 likewise (0101, 0202, 0102);
 *     b1 = d0 d0 - s01sq - quad1;  b2 = d1 d1 - s02sq - quad2;
 *     l01_new = a11inv b1 + a12inv b2;  l02_new = a21inv b1 + a22inv b2;
 *     done = true;  if fabs(l01_new - l01) > tolerance or fabs(l02_new - l02) > tolerance: done = false;
 *     l01 = l01_new;  l02 = l02_new;  if fabs(l01) > 1e150 or fabs(l02) > 1e150: done = true;  niter++
 *   l01 /= dtfsq;  l02 /= dtfsq;  f0 += l01 r01 + l02 r02;  f1 -= l01 r01;  f2 -= l02 r02;
 *   v_ab = l01 r01_a r01_b + l02 r02_a r02_b  for ab = xx, yy, zz, xy, xz, yz.
 * Flag 1, three unknowns l01, l02, l12:
 *   a11 = 2.0 (im0 + im1) (s01 . r01);  a12 = 2.0 im0 (s01 . r02);         a13 = -2.0 im1 (s01 . r12);
 *   a21 = 2.0 im0 (s02 . r01);          a22 = 2.0 (im0 + im2) (s02 . r02);  a23 = 2.0 im2 (s02 . r12);
 *   a31 = -2.0 im1 (s12 . r01);         a32 = 2.0 im2 (s12 . r02);          a33 = 2.0 (im1 + im2) (s12 . r12);
 *   determ = a11 a22 a33 + a12 a23 a31 + a13 a21 a32 - a11 a23 a32 - a12 a21 a33 - a13 a22 a31;  determ == 0 as for flag 3;
 *   determinv = 1.0 / determ;
 *   a11inv = determinv (a22 a33 - a23 a32);   a12inv = -determinv (a12 a33 - a13 a32);  a13inv = determinv (a12 a23 - a13 a22);
 *   a21inv = -determinv (a21 a33 - a23 a31);  a22inv = determinv (a11 a33 - a13 a31);   a23inv = -determinv (a11 a23 - a13 a21);
 *   a31inv = determinv (a21 a32 - a22 a31);   a32inv = -determinv (a11 a32 - a12 a31);  a33inv = determinv (a11 a22 - a12 a21);
 *   quadK = qK_0101 l01 l01 + qK_0202 l02 l02 + qK_1212 l12 l12 + qK_0102 l01 l02 + qK_0112 l01 l12 + qK_0212 l02 l12, with
 *     q1: (im0 + im1) (im0 + im1) r01sq;  im0 im0 r02sq;  im1 im1 r12sq;  2.0 (im0 + im1) im0 r0102;  -2.0 (im0 + im1) im1 r0112;
 *         -2.0 im0 im1 r0212
 *     q2: im0 im0 r01sq;  (im0 + im2) (im0 + im2) r02sq;  im2 im2 r12sq;  2.0 (im0 + im2) im0 r0102;  2.0 im0 im2 r0112;
 *         2.0 (im0 + im2) im2 r0212
 *     q3: im1 im1 r01sq;  im2 im2 r02sq;  (im1 + im2) (im1 + im2) r12sq;  -2.0 im1 im2 r0102;  -2.0 (im1 + im2) im1 r0112;
 *         2.0 (im1 + im2) im2 r0212
 *   b1, b2 as for flag 3;  b3 = d2 d2 - s12sq - quad3;  lK_new = aK1inv b1 + aK2inv b2 + aK3inv b3;  the loop, its stop rule and the
 *   1e150 guard as for flag 3, over three values;  each l /= dtfsq;
 *   f0 += l01 r01 + l02 r02;  f1 -= l01 r01 - l12 r12;  f2 -= l02 r02 + l12 r12;
 *   v_ab = l01 r01_a r01_b + l02 r02_a r02_b + l12 r12_a r12_b.
 * conp_shake_post_force_device and conp_shake_setup_device add the constraint force into d_f (FixShake::post_force and ::setup; they
 *   differ in dtfsq alone).  conp_shake_correct_device (FixShake::correct_coordinates) forms the same force from 0.0 with v = f = 0
 *   and moves the cluster atoms: x_k += dtfmsq_k fc_k.
 * d_out [9], overwritten:  the virial xx, yy, zz, xy, xz, yz (every cluster counts whole: all its atoms are owned);  the number of
 *   clusters that left the loop at max_iter without done;  the number with a zero (flags 3, 1) or negative (flag 2) determinant;
 *   the largest niter (0 for flag 2).  The counts are integer-valued doubles.
 * d_vatom [nlocal][6], overwritten: each atom of a cluster gets v / n, n = 2 (flag 2) or 3 (flags 3, 1), as Fix::v_tally gives it;
 *   rows of atoms in no cluster are exactly 0.0.
 * conp_shake_check_device: d_out[0] = the largest |r - d| / d over the bond constraints, d_out[1] the same over the 1-2 distances
 *   of the flag-1 clusters (r by minimum image); 0.0 where there is none.
 * Order and reproducibility: one thread per cluster reads a cluster atom's f (or x), adds to it once and stores it.  The virial is
 *   summed over clusters in the caller's order: per workgroup in a fixed tree, then over the workgroups in ascending order by one
 *   finishing workgroup; counts and maxima do not depend on order.  Every output is a pure function of the input, byte-identical
 *   from call to call.  Atoms in no cluster and rows from nlocal on are neither read nor written (d_vatom: zeroed).
 * Order: conp_shake_set_params (copies and uploads, reserves all scratch; may allocate and synchronise; afterwards the owned atoms
 *   keep their local order).  At the start of a run: conp_shake_correct_device -> the force entries -> conp_shake_setup_device ->
 *   conp_integrate_setup_device.  Per step: conp_integrate_initial_device -> ... -> conp_ghost_fold_device ->
 *   conp_shake_post_force_device -> conp_integrate_final_device: the constraint force needs the folded total force, as LAMMPS'
 *   post_force runs behind reverse_comm.  The constraint is met by the NEXT nve_x, not by the velocities; with `fix nvt` the
 *   scaling between the two half-steps is ignored, exactly as LAMMPS ignores it.
 * CONP_ERR_STATE: any other entry before conp_shake_set_params.
 * CONP_ERR_ARG: a NULL struct, or a NULL array with a positive count; a negative count; a type outside [1, ntypes]; a flag outside
 *   {1, 2, 3}; an index outside [0, nlocal) or repeated in a cluster; an atom in two clusters; a distance type out of range; a
 *   distance (of any type), mass, dt, ftm2v or tolerance that is not positive and finite; max_iter < 1; a negative or non-finite prd;
 *   a NULL d_x, d_v or d_f.  A refused conp_shake_set_params leaves the handle WITHOUT constraints; every other refused call changes
 *   nothing.  ncluster == 0: CONP_OK, d_out is zeroed, nothing else is touched.  d_out NULL: the finishing launch is skipped (one
 *   launch per call); conp_shake_check_device then does nothing.
 * The step entries enqueue on the handle's stream and make no device allocation, no copy to the host and no synchronisation.
 * They need nothing of the fix but its stream: they work from conp_fix_create on, on Ewald and `pppm` handles, and are rank-local,
 * never collective.  Out of scope: flag 4, RATTLE, rRESPA, rmass, clusters with ghost members, the `stats` print-out. */
typedef struct {
  int nlocal, ntypes;
  const int *type;                      /* [nlocal] 1..ntypes */
  const double *mass;                   /* [ntypes + 1], entry 0 unused */
  int nbondtypes, nangletypes;
  const double *bond_distance;          /* [nbondtypes + 1]  constraint length per bond type (bond r0), entry 0 unused */
  const double *angle_distance;         /* [nangletypes + 1] 1-2 distance per angle type: sqrt(d1^2 + d2^2 - 2 d1 d2 cos(theta0)) */
  int ncluster;
  const int *cluster;                   /* [ncluster][7]  flag, i0, i1, i2, t0, t1, t2 */
  double tolerance; int max_iter;       /* fix shake's tol and iter */
  double dt, ftm2v;                     /* update->dt, force->ftm2v */
  double prd[3];                        /* > 0: minimum image in that dimension; 0: differences as they are */
} conp_shake_params;

int conp_shake_set_params(conp_fix *fix, const conp_shake_params *p);
int conp_shake_correct_device(conp_fix *fix, double *d_x /*[nlocal][3], cluster atoms moved*/);
int conp_shake_setup_device(conp_fix *fix, const double *d_x /*[nlocal][3]*/, const double *d_v /*[nlocal][3]*/,
                            double *d_f /*[nlocal][3], added to*/, double *d_out /*[9], overwritten; NULL: none*/);
int conp_shake_post_force_device(conp_fix *fix, const double *d_x /*[nlocal][3]*/, const double *d_v /*[nlocal][3]*/,
                                 double *d_f /*[nlocal][3], added to*/, double *d_out /*[9], overwritten; NULL: none*/,
                                 double *d_vatom /*[nlocal][6], overwritten; NULL: none*/);
int conp_shake_check_device(conp_fix *fix, const double *d_x /*[nlocal][3]*/, double *d_out /*[2], overwritten*/);

/* ---- `fix efield` with a constant field, and the per-group sums of the thermo columns, on the device ----
 * Two rank-local members of the handle that need nothing of the fix but its stream (the coupled field also reads one device slot
 * of it): they work from conp_fix_create on, on Ewald and `pppm` handles, and are never collective.  All arithmetic is double in the
 * order written below, products left to right, without contraction; no sum meets an atomic: per workgroup a fixed tree, then the
 * rows of the workgroups in a fixed order by a finishing workgroup.  Every output is a pure function of the input, byte-identical
 * from call to call.  Row offsets are formed in size_t.  Rows from nlocal on are neither read nor written.  The step entries
 * (conp_efield_post_force_device, conp_observe_device) enqueue on the handle's stream and make no device allocation, no copy to
 * the host and no synchronisation; the set_params entries copy and upload their arrays, reserve all scratch, and may allocate and
 * synchronise.
 *
 * Unwrapped coordinates, both entries: with d_image, u_c = x_c + ((double)image_c prd_c), the ghost arithmetic of
 * conp_ghost_fill_device; with a NULL d_image, u_c = x_c.
 *
 * conp_efield_*: the force q E on the selected owned atoms (the decks' `fix efield all efield 0 0 $(-v/lz)` beside
 * `fix conp ... ffield`).
 *   The field: ex = qe2f e[0], ey = qe2f e[1], formed on the host.  couple == 0: ez = qe2f e[2].  couple == 1: every thread forms
 *     ez = qe2f (e[2] + couple_scale s) on the device, where s is the double the last update of a conq or cond handle left as the
 *     fix scalar -- the value conp_fix_compute_scalar would return, read where the charge write stored it, without a host copy
 *     (the decks: `variable efi equal -f_e/lz`, couple_scale = -1 / lz, e[2] = 0).  e is HOST memory, read at call time.
 *   Per atom i < nlocal with sel[i] != 0:  fx = q ex, fy = q ey, fz = q ez;  f[i] += (fx, fy, fz);
 *     energy term -((fx ux + fy uy) + fz uz);  v = (fx ux, fy uy, fz uz, fx uy, fx uz, fy uz).
 *   d_out [11]: the energy, sum fx, sum fy, sum fz, the six sums of v, the number of selected atoms.  d_vatom [nlocal][6]: v for a
 *     selected atom, exactly 0.0 for an unselected row below nlocal (zeroed by the same launch).  Unselected rows of d_f are
 *     neither read nor written.  One launch without d_out, two with it.
 *   The rule is the constant-field branch of LAMMPS' FixEfield (energy and virial from unwrapped coordinates).  With an equal-style
 *     variable LAMMPS tallies no energy: an engine that mimics that branch ignores d_out[0].
 *   CONP_ERR_STATE: conp_efield_post_force_device before conp_efield_set_params; couple == 1 before the handle's first update.
 *   CONP_ERR_ARG: a NULL struct; NULL sel with nlocal > 0; negative nlocal; qe2f, an e component or couple_scale that is not
 *     finite; a negative or non-finite prd; NULL d_x, d_q, d_f or e; couple outside {0, 1}; couple == 1 on a handle that is neither
 *     conq nor cond (the engine knows a conp handle's potdiff itself).  A refused conp_efield_set_params leaves the handle WITHOUT a
 *     field; every other refused call changes nothing.  nlocal == 0: CONP_OK, d_out is zeroed.
 *   Order in a step: behind the update (conp_fix_pre_force_device), before conp_shake_post_force_device; the field touches owned
 *     rows only, so its place relative to conp_ghost_fold_device is free.
 *
 * conp_observe_*: per-group sums for groups that may overlap (`compute reduce sum v_q`, the cell dipole `v_qz`, `compute temp`).
 *   Bit g of mask[i] makes atom i a member of group g.  d_out [ngroups][CONP_OBSERVE_W], per group over its members i < nlocal:
 *     column 0 the member count (as a double), 1 sum q, 2-4 sum q ux, sum q uy, sum q uz,
 *     5 sum m ((vx vx + vy vy) + vz vz), 6-8 sum m vx, sum m vy, sum m vz, 9 sum m, with m = mass[type[i]].
 *   Columns 5-8 are exactly 0.0 with a NULL d_v; an empty group is a row of 0.0.  The engine forms the temperature
 *     col5 mvv2e / (dof boltz), `reduce ave` and the centre-of-mass velocity itself.  Two launches.
 *   CONP_ERR_STATE: conp_observe_device before conp_observe_set_params.
 *   CONP_ERR_ARG: a NULL struct, or a NULL array with a positive count; a negative count; ngroups outside
 *     [1, CONP_OBSERVE_MAX_GROUPS]; a mask bit at or above ngroups; a type outside [1, ntypes]; a mass that is not positive and
 *     finite; a negative or non-finite prd; a NULL d_x, d_q or d_out.  A refused conp_observe_set_params leaves the handle WITHOUT
 *     groups; every other refused call changes nothing.  nlocal == 0: CONP_OK, d_out is zeroed.
 * fix zmirror: conp_zmirror_* below.  Out of scope: fix setforce, atom-style and region-restricted fields, dipole torques, pressure assembly. */
#define CONP_OBSERVE_MAX_GROUPS 16
#define CONP_OBSERVE_W 10
typedef struct {
  int nlocal;
  const int *sel;                       /* [nlocal] 0 / 1: the atoms of the fix's group; HOST, copied */
  double qe2f;                          /* force->qe2f */
  double prd[3];                        /* box lengths that d_image counts */
} conp_efield_params;
typedef struct {
  int nlocal, ntypes, ngroups;
  const int *type;                      /* [nlocal] 1..ntypes */
  const int *mask;                      /* [nlocal], bit g = member of group g */
  const double *mass;                   /* [ntypes + 1], entry 0 unused */
  double prd[3];                        /* box lengths that d_image counts */
} conp_observe_params;

int conp_efield_set_params(conp_fix *fix, const conp_efield_params *p);
int conp_efield_post_force_device(conp_fix *fix, const double *d_x /*[nlocal][3]*/, const double *d_q /*[nlocal]*/,
                                  const int *d_image /*[nlocal][3] or NULL*/, double *d_f /*[nlocal][3], added to*/,
                                  const double *e /*HOST [3], V/length, read at call time*/, int couple, double couple_scale,
                                  double *d_out /*[11], overwritten; NULL: none*/, double *d_vatom /*[nlocal][6], overwritten; NULL: none*/);
int conp_observe_set_params(conp_fix *fix, const conp_observe_params *p);
int conp_observe_device(conp_fix *fix, const double *d_x /*[nlocal][3]*/, const double *d_q /*[nlocal]*/,
                        const double *d_v /*[nlocal][3] or NULL*/, const int *d_image /*[nlocal][3] or NULL*/,
                        double *d_out /*[ngroups][CONP_OBSERVE_W], overwritten*/);

/* ---- `neigh_modify exclude` in the device list build, and `fix zmirror` --------------------------------------
 * What the reference's tests/zmirror deck needs beyond sections 16-24; both are rank-local members of the handle.
 *
 * conp_pair_set_exclusions / conp_pair_build_list_exclude_device: conp_pair_build_list_device with LAMMPS'
 * Neighbor::exclusion(i, j, type_i, type_j, mask, molecule) as written.  A candidate pair that passes the distance and the
 * orientation test of conp_pair_build_list_device is DROPPED if any of these holds:
 *   type rules:      ex_type[type_i][type_j] is set -- every (type_i[k], type_j[k]) sets [i][j] and [j][i], as LAMMPS does;
 *   group rules:     for some m, (mask_i & group_bit1[m] and mask_j & group_bit2[m]) or (mask_i & group_bit2[m] and mask_j & group_bit1[m]);
 *   molecule rules:  for some m, mask_i & mol_bit[m] and mask_j & mol_bit[m], and molecule_i == molecule_j (mol_intra[m] != 0:
 *                    molecule/intra) or molecule_i != molecule_j (mol_intra[m] == 0: molecule/inter).
 * The test applies to every candidate, owned or ghost: d_type, d_mask, d_molecule are DEVICE arrays [nall] whose ghost rows the
 * engine fills with conp_ghost_fill_int_device (the handle's own type table is stale for new ghosts at this point of a
 * re-neighbouring and is not used).  A dropped pair is absent -- not kept with special bits --, and the test comes before the
 * special-bond classification.  A d_type[j] outside [0, ntypes] is clamped for the table look-up (type 0 matches no rule).
 * Everything else is the contract of conp_pair_build_list_device word for word: the set rule, newton on and off, the special bits
 * and minimum_image_check, ilist / numneigh / first, byte-identical results from build to build, the reservations for the compute
 * entries, conp_pair_list_moved_device, conp_pair_get_list, use by conp_fix_post_neighbor_device, and what a refused build leaves
 * behind.  A row is the plain build's row with the excluded entries removed and the order kept.
 * With no rule in force (conp_pair_set_exclusions with all counts 0, or with NULL, which clears every rule) the build is the plain
 * build, byte for byte, and reads no per-atom array (the three pointers of `at` may be NULL; `at` itself may not).
 *   Limits: at most 16 group rules and 16 molecule rules; any number of type pairs.
 *   CONP_ERR_STATE: either entry before conp_pair_set_params; the build entry before a successful conp_pair_set_exclusions.
 *   CONP_ERR_ARG, conp_pair_set_exclusions: a negative count; more than 16 group or molecule rules; a count > 0 with a NULL array;
 *     with ntype_pairs > 0 an ntypes that differs from conp_pair_set_params', or a type outside [1, ntypes]; a group or molecule bit
 *     mask of 0.  A refused conp_pair_set_exclusions leaves the handle WITHOUT rules: the build entry answers CONP_ERR_STATE until a
 *     call succeeds.  A second call replaces the rules of the first.  The handle's list is not touched.
 *   CONP_ERR_ARG, the build entry: a NULL at; a NULL per-atom array that a rule in force needs -- d_type with type rules, d_mask
 *     with group or molecule rules, d_molecule with molecule rules; and every refusal of conp_pair_build_list_device.
 *   conp_pair_build_list_device itself ignores the rules: it stays the plain build.
 *
 * conp_zmirror_*: FixZmirror of the reference on one rank.  After the first half of the integrator, x of every atom of the receiving
 * group (jgroupbit) is set to (x, y, zoffset - z) of its partner in the sending group (groupbit), zoffset = 2 boxlo_z + zprd formed
 * in that order on the host.  conp_zmirror_set_params restates FixZmirror::setup and the one-rank branch of post_integrate: the tag
 * ranges [send_mintag, send_maxtag], [recv_mintag, recv_maxtag] over the two groups; for every owned atom i of the sending group, in
 * ascending i, the target is the owned atom with tag  tag[i] - send_mintag + recv_mintag.  The (source, target) pairs go to the
 * device once: owned indices are stable in the device engine (conp_atoms_wrap_device remaps in place).  tag and mask are HOST
 * arrays [nlocal], read once.
 *   conp_zmirror_post_integrate_device: if ntimestep % nevery == 0, one launch, one thread per pair:
 *     x[dst] = (x[src][0], x[src][1], zoffset - x[src][2]), bit-equal to float64 as written; otherwise nothing is launched and the
 *     call returns CONP_OK.  Enqueued on the handle's stream: no allocation, no copy, no synchronisation.  Velocities, image
 *     counters, ghost rows (conp_ghost_fill_device follows) and every row that is no target stay untouched.
 *   No target is a source (refused below), so the copy in place equals the reference's snapshot of the sources before it writes.
 *   On one rank the reference repeats the copy at end_of_step; the repeat is the identity, because x has not changed since
 *   post_integrate, and has no entry here.  v of the mirrored atoms is NOT updated: the engine keeps them out
 *   of every integrator group (conp_integrate_*) and chooses its SHAKE clusters accordingly.
 *   conp_zmirror_get_map: *npairs and, with non-NULL arrays, src [npairs] and dst [npairs] (host).
 *   CONP_ERR_STATE: conp_zmirror_post_integrate_device or conp_zmirror_get_map before conp_zmirror_set_params.
 *   CONP_ERR_ARG: a NULL struct, tag or mask; negative nlocal; nevery < 1; zprd or boxlo_z not finite; a tag that occurs twice; an
 *     empty sending or receiving group; unequal tag ranges (the reference's "Groups do not have same number of tags"); a target tag
 *     that no owned atom has; a target outside the receiving group; a target that is itself in the sending group; a NULL d_x.  A
 *     refused conp_zmirror_set_params leaves the handle WITHOUT a mirror; every other refused call changes nothing.
 *   Order in a step: conp_integrate_initial_device -> conp_zmirror_post_integrate_device -> conp_ghost_fill_device ->
 *     conp_fix_pre_force_device -> ...; at a re-neighbouring: ... -> conp_ghost_build_device -> conp_ghost_fill_device /
 *     conp_ghost_fill_int_device (tag, type, mask, molecule) -> conp_pair_build_list_exclude_device -> conp_fix_post_neighbor_device.
 * Out of scope: per-type-pair list cutoffs, triclinic boxes, the multi-rank comm_and_remap, mirrored velocities. */
typedef struct {
  int ntypes;                           /* must equal the ntypes of conp_pair_set_params when ntype_pairs > 0 */
  int ntype_pairs;
  const int *type_i, *type_j;           /* HOST [ntype_pairs], 1-based */
  int ngroup_pairs;
  const int *group_bit1, *group_bit2;   /* HOST [ngroup_pairs], LAMMPS group bit masks (1 << g) */
  int nmol;
  const int *mol_bit, *mol_intra;       /* HOST [nmol]; intra != 0: molecule/intra, 0: molecule/inter */
} conp_pair_exclusions;
typedef struct {
  const int *d_type, *d_mask, *d_molecule;      /* DEVICE, each [nall]; NULL where no rule in force reads it */
} conp_pair_exclude_atoms;
int conp_pair_set_exclusions(conp_fix *fix, const conp_pair_exclusions *e /* NULL: clears every rule */);
int conp_pair_build_list_exclude_device(conp_fix *fix, const double *d_x, const conp_pair_build_args *a,
                                        const conp_pair_exclude_atoms *at);
typedef struct {
  int nlocal;
  const int *tag, *mask;                /* HOST [nlocal], read once */
  int groupbit, jgroupbit;              /* sending group, receiving group */
  int nevery;                           /* >= 1 */
  double boxlo_z, zprd;                 /* zoffset = 2 boxlo_z + zprd */
} conp_zmirror_params;
int conp_zmirror_set_params(conp_fix *fix, const conp_zmirror_params *p);
int conp_zmirror_post_integrate_device(conp_fix *fix, double *d_x /*[>= nlocal][3]*/, long long ntimestep);
int conp_zmirror_get_map(conp_fix *fix, int *npairs, int *src, int *dst);   /* arrays NULL: count only */

/* per-kernel timing of the last N updates via HIP events on the library's stream (bench.py roofline leg).
 * enable: 0 off, 1 a pair of events around every kernel, 2 around every 4th launch of the dominant kernel (sk_gemm) only --
 * cheap enough to stay on inside a timed region (an event pair drains the queue around the kernel it brackets). */
int conp_fix_profile(conp_fix *fix, int enable);
int conp_fix_profile_read(conp_fix *fix, int *nkernels, const char **names /*[16]*/, double *avg_ms /*[16]*/, int *counts /*[16]*/);
/* ---- page-locked host memory (optional; no reference counterpart: the reference has no device) ----
 * The host-buffer hooks copy x, q (and, at a re-neighbour, the flattened neighbour list) out of the host's arrays.  Out of
 * PAGEABLE memory such a copy is staged by the runtime and blocks the calling thread (about 70 us for the 1.2 MB of x, q at the
 * headline size); out of page-locked memory it is an asynchronous DMA transfer that overlaps the enqueue of the update's kernels.
 *   conp_fix_pin_host_arrays   page-locks the host's OWN arrays in place: x [3 n] and q [n], n >= nlocal + nghost of the calls
 *       that follow.  The host promises that both stay where they are, and allocated, until conp_fix_unpin_host_arrays (or the
 *       handle's destruction).  LAMMPS: atom->x / atom->q move only when the per-atom arrays grow, which happens between
 *       pre_exchange and post_neighbor of a re-neighbouring step -- the glue unpins in pre_exchange and pins again in
 *       post_neighbor.  Arrays that were not pinned (or other pointers than the pinned ones) take the staged copy as before:
 *       same results either way.  A runtime that refuses the registration returns CONP_ERR_NO_DEVICE and changes nothing.
 *   conp_host_alloc / conp_host_free   page-locked memory for arrays the host BUILDS for the hooks (the glue's flattened
 *       neighbour list: conp_neighlist.first / .neigh). */
int conp_fix_pin_host_arrays(conp_fix *fix, const double *x, const double *q, int n);
int conp_fix_unpin_host_arrays(conp_fix *fix);
void *conp_host_alloc(size_t bytes);
void conp_host_free(void *p);

/* Diagnostic (no reference counterpart): with CONP_GUARD=1 in the environment every device buffer of the library sits between two
 * 4-KB zones of a known byte pattern; this reads all zones back.  Returns the number of damaged zones (0 = no kernel has stored
 * outside its buffers so far), -1 when guard zones are off; conp_last_error() names the damaged buffers. */
int conp_debug_check_guards(void);

/* Test hooks (no reference counterpart): alternative code paths of the SAME computation, results inside the parity tolerances of
 * DESIGN.md section 2 -- what tests/ compares the default paths with (A/B inside one process).  Process-wide bit mask, read when a
 * handle is created (CONP_PATH_ROWS_HOST, CONP_PATH_PPPM_SPREAD_LAUNCH, CONP_PATH_ZC_PHASE_LOADS: at every call; CONP_PATH_HC_TABLES: at
 * every list build).  The first handle created with a
 * non-zero mask says so on stderr.  conp_debug_set_sk_workgroups: workgroup count of the structure-factor launch (0 = the
 * library's choice), for the tests that cover heavily split tiles on a small deck.  conp_debug_set_ew_block: cap of the atom block of
 * the conp_ewald_* entries' phase tables (0 = the library's choice; else n rounded up to a multiple of 64), process-wide and read at
 * every call, for the tests that run several blocks and a ragged last one on a deck.  Not meant for production runs. */
enum {
  CONP_PATH_PARTIAL_TILES = 1 << 0,      /* planar electrodes: partial tiles + reducing launch instead of the projecting epilogue */
  CONP_PATH_A_GENERAL = 1 << 1,          /* A k-space part: the general (planar, kz) contraction instead of the z-class one */
  CONP_PATH_INV_PIVOTED = 1 << 2,        /* inverse: pivoted elimination instead of the positive-definite path */
  CONP_PATH_CG_TWO_LAUNCH = 1 << 3,      /* CG: matvec + update launches per iteration instead of one */
  CONP_PATH_GEMV_ROWS = 1 << 4,          /* solve: row-by-row product also from 2048 electrode atoms up (no packed symmetric tiles) */
  CONP_PATH_PHASE_LAUNCH = 1 << 5,       /* small systems: stand-alone phase-table launch instead of the prologue inside sk_gemm */
  CONP_PATH_PPPM_SPREAD_LAUNCH = 1 << 6, /* pppm: density brick + spreading launch also for deck-sized systems */
  CONP_PATH_ROWS_HOST = 1 << 7,          /* re-neighbour: electrode rows regrouped on the host */
  CONP_PATH_TIME_SPLIT = 1 << 8,         /* host-buffer hooks: k-space and real-space halves of b_cal in launches of their own (timing log) */
  /* 1 << 9, 1 << 10, 1 << 11: retired (test paths of forms measured slower and removed); ignored when set */
  CONP_PATH_SK_CLASSIC = 1 << 12,        /* large planar systems: sk_gemm over all kz columns instead of the z-window contraction (conp_zn.hip) */
  CONP_PATH_ZN_WIDE = 1 << 13,           /* z-window: 48 window columns also where 32 would do (the second template form on medium boxes) */
  CONP_PATH_ZC_PHASE_LOADS = 1 << 14,    /* planar electrodes: the finishing dot kernel loads its electrode phases per thread instead of staging the rows in LDS */
  CONP_PATH_HC_TABLES = 1 << 15,         /* z-window: the piece sums read their piece lists also where the addresses are arithmetic */
  CONP_PATH_SOLVE_NO_LATTICE = 1 << 16   /* solve: packed symmetric tiles also where the electrodes are a lattice (no block-circulant table) */
};
void conp_debug_set_paths(unsigned mask);
void conp_debug_set_sk_workgroups(int n);
void conp_debug_set_ew_block(int n);
/* cap of the basis atoms whose table slabs the lattice form of the solve stages at a time (0 = as many as fit), process-wide and read
 * once per matrix: for the tests that run several stages on a small box */
void conp_debug_set_lat_stage(int n);

/* Which form the fused solve (one-rank `fix conp`, inverse solver) multiplies the current matrix in -- decided at the first update
 * after the matrix changed.  form_out = {form, nx, ny, nbasis}: form 0 full rows, 1 packed symmetric tiles (from 2048 electrode
 * atoms up), 2 the block-circulant table of lattice-periodic electrodes, -1 not decided yet; nx, ny, nbasis the lattice the
 * electrode positions proposed (0 where they proposed none, or the form was not looked for).  dev_out = {max |S_ij - T[basis_i]
 * [basis_j][cell_j - cell_i]|, max |S_ij|} of the pass that tested the matrix against that lattice (form 2: dev <= 1e-10 max). */
int conp_fix_get_solve_form(conp_fix *fix, int *form_out /*[4]*/, double *dev_out /*[2]*/);
/* the host's lattice search on its own (no device): the smallest axis-aligned translations (lx / nx, 0, 0), (0, ly / ny, 0) that map
 * the n points x [n][3] onto themselves, periodic in x and y, matched within 1e-4.  Returns 1 and dims = {nx, ny, nbasis},
 * row [nbasis][nx][ny] -> point, pos [n][3] = (basis, cx, cy) of every point; 0 when the points are no such lattice. */
int conp_host_find_lattice(int n, const double *x, double lx, double ly, int *dims /*[3]*/, int *row /*[n]*/, int *pos /*[3 n]*/);


/* ---- the fix's log file (fix_conp.cpp:119 `outf`) ----
 * The library buffers the lines the reference prints there -- "A matrix calculating ..." / "A matrix calculation time  = %g"
 * (:787, :857), the CG "Iteration %d: res = %g" / "***** Converged at iteration ..." lines (:919-928) -- and the host appends
 * them to its file.  conp_fix_write_timing adds the three lines FixConp::pre_force prints on the last step of a run
 * (:553-568: B vector / Coulomb / Kspace calculation time, seconds accumulated over the host-buffer pre_force calls, measured
 * with HIP events around the k-space and real-space halves of b_cal).  conp_fix_log_drain returns the buffered text
 * (valid until the next call on this fix) and empties the buffer. */
int conp_fix_write_timing(conp_fix *fix);
const char *conp_fix_log_drain(conp_fix *fix);
/* same for the two lines the reference sends to utils::logmesg (screen + LAMMPS log): "conp output: <e,e> = %.8g" after the
 * inverse's row sums (fix_conp.cpp:1006-1009) and "conp output: <d,d> = %.8g" at the end of linalg_setup (:458-461) */
const char *conp_fix_mesg_drain(conp_fix *fix);

#ifdef __cplusplus
}
#endif
#endif /* CONP_HIP_H */
