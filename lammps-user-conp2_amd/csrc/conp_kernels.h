// Launch wrappers of the gfx950 kernels (conp_kernels.hip).  All pointers are device pointers unless noted.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include "../../include/conp_hip.h"      // CONP_PATH_* (the test hooks of the C ABI)

namespace conp {

// Alternative code paths.  (i) What the parity tests compare the default paths with is selected through the C ABI
// (conp_debug_set_paths, include/conp_hip.h: a process-wide bit mask, CONP_PATH_*) -- path_on().  (ii) The library reads from the
// environment only operational knobs: CONP_GUARD, CONP_GRAPH, CONP_PANEL_SINGLE / _MAXG / _SPIN, CONP_HOST_THREADS,
// CONP_TIME_HOST / _REN.  Decided experiments ("measured, not kept") are recorded in DESIGN-LOG.md, not kept as switches.
bool path_on(unsigned bit);
int debug_sk_workgroups();
int debug_ew_block();                        // conp_debug_set_ew_block: cap of the Ewald entries' block width (0: the library's choice)
int debug_lat_stage();                       // conp_debug_set_lat_stage: cap of the basis atoms the lattice solve stages at a time (0: what fits)
const char *env_knob(const char *name);      // operational knob: getenv + one line on stderr the first time a set knob is read

// raise a kernel's dynamic-LDS limit, only when a launch needs more than it was last given: per-update launches must not
// pay a runtime call each (the decks' updates are bound by host launch cost)
// The attribute is per device: the cache is indexed by the calling thread's current device (handles on several GPUs in one
// process are supported, conp_env.device), and atomic because hosts may drive handles from different threads (a lost race
// only sets the attribute twice).
struct DynLdsCache { std::atomic<size_t> granted[64]; };
template <typename K>
void ensure_dyn_lds(K kernel, size_t bytes, DynLdsCache &cache) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::atomic<size_t> &g = cache.granted[dev & 63];
  if (bytes <= g.load(std::memory_order_relaxed)) return;
  // a refusal is not remembered: the launch that follows fails and the caller's hipGetLastError reports it
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess)
    g.store(bytes, std::memory_order_relaxed);
}

struct DevPlan {              // device copy of KPlan geometry
  int np, nz, n_row_tiles, n_col_tiles, R_pad, C_pad, kxmax, kymax;
  const int *p_ikx, *p_iky, *p_sgn;   // [n_row_tiles*64] padded (padding: 0,0,0 -> sgn 0 marks "no vector")
  const int *nb_act;                  // [n_col_tiles][n_row_tiles] active 16-kz blocks of the column tile per row tile (KPlan::nba_rc)
  const double *wfull;                // [R_pad][C_pad]
};

// the z-window form (conp_zn.hip): item = (row tile: 64 planar vectors, chunk range [c0, c1) of the z-ordered electrolyte list, window
// origin g0 on the grid, slot of its piece [class][128 rows] in the pieces buffer)
struct ZnItem { int rt, c0, c1, g0, slot, paired; };     // paired: the row tile holds 32 whole (+ky, -ky) pairs (KPlan::paired_lo / _hi)
// what elyte_phase_kernel's z-axis threads need to write the window matrix of an update instead of the z phase seeds
struct ZnWindow { double *Bt; const int *g0c; int *flag; int ncol, n, W; double beta, gscale; };

// One sk_gemm segment: a BAND of planar vectors x one column tile x a chunk range [c0, c1) of 16 atoms.  A band = rf consecutive row
// fragments (16 planar vectors each) g0 .. g0 + rf - 1 of the plan, rf = 4 (up to 20 column fragments, e.g. one row tile of the plan)
// or 5 (up to 16 column fragments): 20 accumulator fragments per wave either way.  nbf = active 8-kz column fragments per row
// fragment, rf x 8 bit.
struct SkItem { int g0, rf, ct, c0, c1; unsigned long long nbf; };
// parameter block of sk_gemm's projecting epilogue (device memory): weights [R_pad][C_pad], z-class phases class-major [nzc][C_pad]
struct SkProj { const double *wfull, *tzt; int nzc, cpad; };
// sk_gemm's work list, one fixed-size row per workgroup: the segments it runs, each with its output slots -- one per row tile of the
// plan the band touches (sga: row tile g0 >> 2, sgb: the next one or -1), numbered tile-major (SkTile::item0), for the partial-tile
// mode; sg = the segment's own index, the slot of its band-local piece in the projecting mode -- and the first entry's nseg = how
// many are used.  One load replaces the seg_ptr -> seg_idx -> items chain at the top of every workgroup.
struct SkWItem { int g0, rf, ct, c0, c1, sg, sga, sgb, nseg, slab_slot /*SkFuse: where this segment's sum of q z goes, or -1*/; unsigned long long nbf; };
struct SkTile { int rt, ct, nba, item0, nsplit; unsigned nbf; };     // one (row tile, col tile) of the plan: its output slots are item0 .. item0+nsplit-1

struct RealParams {           // real-space pair kernels
  double g_ewald, eta, cut_coulsq;    // cut_coulsq already min(cut_coul^2, (5.8/g)^2)  fix_conp.cpp:1237-1240
  int ntypes;
  const double *cutsq;                // [(ntypes+1)^2]
  int ehgo;                           // EHGO pair mode (fix_conp.cpp:1561-1573): per type-pair eta_ij, fo_ij
  const double *eta_ij, *fo_ij;       // [(ntypes+1)^2]
  const double *u0_i;                 // [ntypes+1] (post-force self energy :1182-1199)
};

// everything one electrode row of b needs besides the k-space partials' origin (b_real_combine_kernel; the fused tail of
// b_zc_dot_kernel): real-space rows [row0, row1), the four k-space partial slots, the slab term
struct BRowArgs {
  int ne, ne_pad, row0, row1;
  const int *row_ptr, *ele_atom, *oth_atom;
  const double *x, *q;
  const int *type;
  RealParams rp;
  int add_k;
  const double *bk;
  int slab;
  const double *ele_z, *slab_part;
  int n_slab_part;
  double slab_pref;
  double *b_out, *slab_out;
  const double *breal;      // NULL: the real-space pair sums are formed by whoever assembles the row; else they are read here
};
inline BRowArgs make_brow(int ne, int ne_pad, int row0, int row1, const int *row_ptr, const int *ele_atom, const int *oth_atom,
                          const double *x, const double *q, const int *type, RealParams rp, int add_k, const double *bk, int slab,
                          const double *ele_z, const double *slab_part, int n_slab_part, double slab_pref, double *b_out,
                          double *slab_out) {
  BRowArgs a;
  a.ne = ne; a.ne_pad = ne_pad; a.row0 = row0; a.row1 = row1; a.row_ptr = row_ptr; a.ele_atom = ele_atom; a.oth_atom = oth_atom;
  a.x = x; a.q = q; a.type = type; a.rp = rp; a.add_k = add_k; a.bk = bk; a.slab = slab; a.ele_z = ele_z; a.slab_part = slab_part;
  a.n_slab_part = n_slab_part; a.slab_pref = slab_pref; a.b_out = b_out; a.slab_out = slab_out; a.breal = nullptr;
  return a;
}

// Small systems (round 4): the phase tables of a segment's atoms are computed by the segment's own workgroup in front of its chunk
// loop (sk_phase_prologue: the arithmetic of elyte_phase_kernel; several bands compute the same atoms' entries -- identical values
// to identical addresses), the real-space pair sums ride in spare workgroups of the same launch: no elyte_phase launch at all.
struct SkFuse {
  int on;                         // 0: the tables were filled by elyte_phase_kernel
  int nl, kzt, nwg_sk;            // charged electrolyte atoms; kz values per column tile; workgroups that run segments (the rest: pair rows)
  const int *elyte_idx;
  const double *x, *q;
  double ux, uy, uz;
  double2 *Xt, *Yt, *Zs;
  double *qc, *slab_part;         // slab_part[SkWItem::slab_slot]: sum of q z over the segment's atoms (segments of band 0 of column tile 0)
  BRowArgs rows;
  double *breal_out;
};

struct PppmDev {              // device view of PppmPlan
  int nx, ny, nz, order, nlower, nfft;
  double shift, shiftone, delinv[3], delvolinv, boxlo[3];
  const double *rho_coeff, *greensfn, *twid[3];
};
// pppm_conp.cpp:269-316 on the device (conp_pppm.hip): bk slot 0 <- PPPM k-space b of all electrode atoms
void launch_pppm_b(hipStream_t s, const PppmDev &pd, int nl, const int *elyte_idx, const double *x, const double *q, int ne,
                   int ne_pad, const int *egrid, const double *ew, double *re, double *im, double *slab_part, int *n_slab_part,
                   double *bk, bool *im_clean /* in/out: `im` is all zero -- then it receives the charges and no clearing launch is needed */,
                   const BRowArgs *pairs = nullptr /*with breal_out: the real-space pair sums of these rows ride in the spread launch*/,
                   double *breal_out = nullptr, BRowArgs *fin = nullptr /*the gather completes the rows of b (needs fin->breal)*/,
                   double *keep_rho = nullptr /*[nfft]: receives the electrolyte density brick of this update*/);

// PPPM coupling beyond b (pppm_conp.cpp:385-534) and the pair part of compute potential/atom (compute_potential_atom.cpp:223-308)
void launch_pppm_density(hipStream_t s, const PppmDev &pd, int n, const int *idx, const double *x, const double *q, double *rho,
                         double *slab_scratch /*[>= 1025]*/);
void launch_pppm_poisson(hipStream_t s, const PppmDev &pd, double *re /*rho in, u_brick out*/, double *im);
// dynamic LDS (bytes) of the transform of one mesh line of n points; a workgroup of gfx950 has PPPM_LDS_MAX at most
size_t pppm_line_lds_bytes(int n);
constexpr size_t PPPM_LDS_MAX = 160 * 1024;
void launch_pppm_probe(hipStream_t s, const PppmDev &pd, int n, const int *idx, const double *x, const double *q, const double *u,
                       double self, double *out /*indexed by atom*/);
// reciprocal-space forces, energy and virial through the mesh (conp_pppm_compute_forces)
struct EwForceOut;
int pppm_kspace_workgroups(int nfft);
// forward: rho (in `re`: the brick of every charged atom) -> rho^ in (re, im).  kspace: sums[7] = (V / 2) sum G |rho^|^2 / N^2 and the
// six virial sums (without qqrd2e); (re, im) <- the packed spectrum of u and E_z, (pre, pim) <- that of E_x and E_y (both NULL: no
// field bricks).  backward: a packed brick -> its two real fields.
void launch_pppm_forward(hipStream_t s, const PppmDev &pd, double *re, double *im);
void launch_pppm_kspace(hipStream_t s, const PppmDev &pd, const double uk[3], double g_ewald, double volume, double *re, double *im,
                        double *pre, double *pim, double *part /*[pppm_kspace_workgroups][7]*/, double *sums /*[7]*/);
void launch_pppm_backward(hipStream_t s, const PppmDev &pd, double *re, double *im);
void launch_pppm_force_gather(hipStream_t s, const PppmDev &pd, int n, const int *idx, const double *x, const double *q, const double *ex,
                              const double *ey, const double *ez, const double *u /*NULL with eo == NULL*/, const EwForceOut &o,
                              double *fo /*[nlocal][3], written at idx; NULL: none*/, double *eo /*[nlocal]; NULL: none*/);
void launch_potential_pair(hipStream_t s, int inum, const int *ilist, const int *numneigh, const int *first, const int *neigh,
                           int nlocal, int newton, const double *x, const double *q, const int *type, const int *sel,
                           const int *etasel, int ntypes, const double *cutsq, double cut_coulsq, double g_ewald, double eta,
                           double *potential);

// ---- exact Ewald per-atom potential (conp_potential.hip): structure factor of any atom list, projection onto any atom list -------
void launch_ew_seeds(hipStream_t s, int n, const double *x /*[n][3]*/, double ux, double uy, double uz, double *seeds /*[6][n]*/);
void launch_ew_sk(hipStream_t s, const DevPlan &pl, int nb_pad, int nsplit, const double *Rp /*[R_pad][nb_pad]*/,
                  const double *Tz /*[C_pad][nb_pad]*/, const double *q /*[nb_pad], 0 in padding*/, double *Gp /*[nsplit][R_pad][C_pad] +=*/);
void launch_ew_sk_sum(hipStream_t s, const DevPlan &pl, int nsplit, const double *Gp, double *G /*[R_pad][C_pad]*/);
void launch_ew_gw(hipStream_t s, const DevPlan &pl, const double *G, double *Gwf /*w o G, b_project_kernel's order*/);
void launch_ew_out(hipStream_t s, int n, int nb_pad, const double *bk /*[4][nb_pad]*/, const int *idx, const double *q, double selfc,
                   double *g_out /*indexed by atom*/, double *u_out);

// exact Ewald forces, energy and virial (conp_ewald_compute_forces)
// out: [4 quantities: g, dg/dx, dg/dy, dg/dz][4 parts][nb_pad], the parts to be added as (p0 + p1) + (p2 + p3)
void launch_ew_force(hipStream_t s, const DevPlan &pl, int kzt, double ux, double uy, double uz, int nb_pad, const int *ct_ptr,
                     const SkTile *tiles, const double *Gwf, const double *Rp, const double *Tz, double *out);
int ew_energy_virial_workgroups(int K);
// sums[7] = sum_k ug |S_k|^2 and the six virial sums (xx, yy, zz, xy, xz, yz), without qqrd2e.  kv: [4][K] = ug, kx, ky, kz of the
// reference's k list; part: [ew_energy_virial_workgroups(K)][7] scratch
void launch_ew_energy_virial(hipStream_t s, int K, int C_pad, int PT, const int *sf_row_a, const int *sf_col_c, const int *k_sign,
                             const double *kv, double g_ewald, const double *G, double *part, double *sums);
struct EwForceOut {
  double qs, selfc, ecoef /*(pi / 2) Q / (g^2 V)*/;
  int slab;
  double fz_pref /*-4 pi / V*/, e_pref /*2 pi / V*/, M, M2, Q, L2_12 /*L^2 / 12*/;
};
// the tail both k-space force entries share (Ewald::slabcorr and PPPM::slabcorr are the same formulas): atom a with charge qi at
// height z, g = minus its k-space potential (no self term), (fx, fy, fz) = qi times the field -> slab force, per-atom energy, qqrd2e
// ADD: the device-resident entries accumulate into the caller's force array (one lane owns one atom: load, add, store); the host
// entries overwrite a scratch array
template <bool ADD = false>
__device__ __forceinline__ void kspace_atom_out(const EwForceOut &o, double qi, double z, double g, double fx, double fy, double fz,
                                                size_t a, double *__restrict__ fo, double *__restrict__ eo) {
  double e = -0.5 * qi * (g + o.selfc * qi) - o.ecoef * qi;
  if (o.slab) {
    fz += o.fz_pref * qi * (o.M - o.Q * z);
    e += o.e_pref * qi * (z * o.M - 0.5 * (o.M2 + o.Q * z * z) - o.Q * o.L2_12);
  }
  if (fo) {
    if (ADD) { fo[3 * a] += o.qs * fx; fo[3 * a + 1] += o.qs * fy; fo[3 * a + 2] += o.qs * fz; }
    else { fo[3 * a] = o.qs * fx; fo[3 * a + 1] = o.qs * fy; fo[3 * a + 2] = o.qs * fz; }
  }
  if (eo) eo[a] = o.qs * e;
}
// the device-resident entries' EwForceOut: Q, M, M2 from the four sums on the device (four = Q, Q2, M, M2), and o.ecoef arrives
// as (pi / 2) / (g^2 V), without its factor Q
__device__ __forceinline__ EwForceOut kspace_out_from_sums(EwForceOut o, const double *__restrict__ four) {
  o.Q = four[0]; o.M = four[2]; o.M2 = four[3];
  o.ecoef *= o.Q;
  return o;
}
void launch_ew_force_out(hipStream_t s, int n, int nb_pad, const double *bk /*[4][4][nb_pad]*/, const int *idx, const double *q,
                         const double *x /*[n][3]*/, const EwForceOut &o, double *fo /*[nlocal][3], written at idx*/,
                         double *eo /*[nlocal]*/);

// ---- device-resident k-space forces (conp_ewald_compute_forces_device / conp_pppm_compute_forces_device) ----
// sums[4] = Q, Q2, M, M2 = the sums of q, q^2, q z, q z^2 over the atoms [0, n), in ew_energy_virial_kernel's fixed order (no
// atomics).  part: [kspace_four_sums_workgroups(n)][4] scratch
int kspace_four_sums_workgroups(int n);
void launch_kspace_four_sums(hipStream_t s, int n, const double *x /*[n][3]*/, const double *q, double *part, double *sums);
// ev[7] = energy and the six virial components from the seven k-space sums s7 (launch_ew_energy_virial / launch_pppm_kspace) and
// the four sums: what the host entries evaluate after their synchronisation
struct KspaceFinish {
  double qs, g_pis /*g / sqrt(pi)*/, qcoef /*(pi / 2) / (g^2 V)*/, slab_pref /*2 pi / V*/, L2_12 /*L^2 / 12*/;
  int slab;
};
void launch_kspace_finish(hipStream_t s, const KspaceFinish &a, const double *s7, const double *four, double *ev);
// launch_ew_force_out for the atoms [base, base + n) themselves (no index list): q, x are the block's, Q, M, M2 and the factor of
// o.ecoef come from `four` (kspace_out_from_sums), fo is ADDED to, eo overwritten
void launch_ew_force_out_device(hipStream_t s, int n, int nb_pad, const double *bk, const double *q, const double *x, const EwForceOut &o,
                                const double *four, int base, double *fo /*[nlocal][3], +=; NULL: none*/, double *eo /*[nlocal]; NULL: none*/);
// launch_pppm_force_gather likewise, every atom [0, n) a target
void launch_pppm_force_gather_device(hipStream_t s, const PppmDev &pd, int n, const double *x, const double *q, const double *ex,
                                     const double *ey, const double *ez, const double *u, const EwForceOut &o, const double *four,
                                     double *fo, double *eo);

// ---- per-atom virial of both k-space force entries (conp_*_compute_forces_vatom[_device]) --------------------
// (c o w) o G in launch_ew_gw's order, c = 1 / k^2 + 1 / (4 g^2) of the entry's planar vector and kz
void launch_ew_gw2(hipStream_t s, const DevPlan &pl, int kzt, double ux, double uy, double uz, double g_ewald, const double *G,
                   double *Gwf2);
// out: [6 quantities: KK_xx, KK_yy, KK_xy, KK_zz, KK_xz, KK_yz][4 parts][nb_pad], KK_ab = sum_k 2 ug c k_a k_b A_i(k); two launches
void launch_ew_vatom(hipStream_t s, const DevPlan &pl, int kzt, double ux, double uy, double uz, int nb_pad, const int *ct_ptr,
                     const SkTile *tiles, const double *Gwf2, const double *Rp, const double *Tz, double *out);
// vo[idx[i]][6] (or vo[base + i][6]) = qs q_i (delta_ab (-g_i / 2) - KK_ab), xx yy zz xy xz yz; bk: launch_ew_force's output
void launch_ew_vatom_out(hipStream_t s, int n, int nb_pad, const double *bk, const double *vk, const int *idx, const double *q, double qs,
                         double *vo);
void launch_ew_vatom_out_device(hipStream_t s, int n, int nb_pad, const double *bk, const double *vk, const double *q, double qs, int base,
                                double *vo);
// the six packed spectra vg_ab phi from rho^ (re, im; read BEFORE launch_pppm_kspace overwrites them):
// (v[0], v[1]) <- xx + i yy, (v[2], v[3]) <- zz + i xy, (v[4], v[5]) <- xz + i yz; launch_pppm_backward on each pair gives the fields
void launch_pppm_vatom_spectra(hipStream_t s, const PppmDev &pd, const double uk[3], double g_ewald, const double *re, const double *im,
                               double *const v[6]);
// v: the six fields in the order xx, yy, zz, xy, xz, yz.  idx == NULL: every atom [0, n) a target.  vo: [nlocal][6], written at idx
void launch_pppm_vatom_gather(hipStream_t s, const PppmDev &pd, int n, const int *idx, const double *x, const double *q,
                              double *const v[6], double qs, double *vo);

// ---- the z-window form of the structure-factor contraction (conp_zn.hip, round 5) ------------------------------------------------
// item = (row tile: 64 planar vectors, chunk range [c0, c1) of the z-ordered electrolyte list, window origin g0 on the grid, slot of
// its piece [class][128 rows] in the pieces buffer)
void launch_zn_ptable(hipStream_t s, const DevPlan &pl, int kzt, int nzc, int n, const double *tzt /*[nzc][C_pad]*/,
                      const double *phihat /*[nz]*/, const double2 *cs /*[n]: (cos, sin)(2 pi k / n)*/, double *P /*[R_pad][nzc][n]*/);
// rough electrodes: the ranges' raw windows (launch_zn_gemm with P == nullptr) -> rows on the z grid -> G, w o G (sk_reduce's outputs)
void launch_zn_dtable(hipStream_t s, const DevPlan &pl, int kzt, int n, const double *phihat, const double2 *cs, double *Dt /*[n][C_pad]*/);
void launch_zn_windows_to_g(hipStream_t s, const DevPlan &pl, int kzt, int n, int n_own, const int *own_rt, int nrg, int ncol, const int *cov_ptr,
                            const int2 *cov_ent, const double *raw, double *grid, const double *Dt, double *G, double *Gwf);
void launch_zn_gemm(hipStream_t s, const DevPlan &pl, int ncf /*2 or 3 column fragments*/, const ZnItem *items, int nitems, const double2 *Xt,
                    const double2 *Yt, const double *Bt, const double *P, int n, int nzc, double *pieces, int piece_stride);

// ---- per-step electrolyte path -----------------------------------------------------------------
void launch_ghost_fill(hipStream_t s, int nlocal, int nghost, const int *owner, const int *img, double px, double py, double pz,
                       double *x, double *q);
void launch_elyte_phase(hipStream_t s, int nl, int nl_pad, const int *elyte_idx, const double *x, const double *q,
                        double ux, double uy, double uz, int kxmax, int kymax, int nz, int kzt, int nrz, double2 *Xt,
                        double2 *Yt, double2 *Zs, double *qc, double *slab_part, int *n_slab_part,
                        const BRowArgs *rows /*NULL, or: the real-space pair sums of these rows ride along, into breal_out*/,
                        double *breal_out, int j0 /*tables for the atoms [j0, j1) of the compact list only (a rank's share)*/, int j1,
                        const ZnWindow *zw = nullptr /*the z-window form: the window matrix instead of the z phase seeds*/);
bool zc_final_fits(int n_own, int nzc);
void launch_sk_gemm(hipStream_t s, const DevPlan &pl, const SkWItem *witems /*[nwg][maxseg]*/, int maxseg, int nwg, int nl_pad,
                    const double2 *Xt, const double2 *Yt, const double2 *Zs, const double *qc, double *part, const SkProj *proj = nullptr,
                    const SkFuse *fuse = nullptr /*small systems: phase tables and pair sums inside this launch (DEVICE copy of the block)*/,
                    int fuse_rows = 0 /*its rows.ne*/);
int sk_hc_stride();           // doubles per segment of sk_gemm's projected output
int sk_hc_max_classes();      // most z classes the projecting mode takes
void launch_project_zclass_pieces(hipStream_t s, const DevPlan &pl, int ne_pad, int n_own, const int *own_rt, int nzc, const double *Hp,
                                  const int *slot_ptr, const int *slot_idx, bool presum /*hc_sum first: many pieces, or bands that are
                                  not row tiles of the plan*/, const int *frag_ptr /*[nfrag + 1]*/, const int2 *frag_ents /*per row fragment of the plan: its pieces
                                  (offset of the fragment's first 'a' row, the band's rf)*/, int nfrag, const double *Rp, const double2 *Xe,
                                  const double2 *Ye, const int *own_pv, const int *zclass, double *Hc, double *bk_part, const BRowArgs *fin,
                                  const BRowArgs *pairs = nullptr /*with breal_out: the pair sums ride in hc_sum's launch*/,
                                  double *breal_out = nullptr,
                                  bool wide = false /*many pieces per fragment: 32 threads per element in the sum*/,
                                  int arith_nrg = 0 /*> 0: fragment g's pieces are ((g >> 2) arith_nrg + j) arith_stride + 16 (g & 3),
                                  rf = 4, j = 0 .. arith_nrg - 1 (hc_frag_lists_arithmetic): the sum forms the addresses itself*/,
                                  int arith_stride = 0);
// true when every row fragment's list is exactly that: the z-window form's pieces in slot order
bool hc_frag_lists_arithmetic(const int *frag_ptr, const int2 *ents, int nfrag, int nrg, int stride);
// dynamic LDS of the electrode phase rows b_zc_final_kernel stages behind its class table, 0: the per-thread loads are used
size_t zc_final_phase_lds(int n_own, int nzc, int kxmax, int kymax);
void launch_sk_reduce(hipStream_t s, const DevPlan &pl, const SkTile *tiles, int ntiles, int max_nsplit, double *part, double *G,
                      double *Gwf);
void launch_sfac_gather(hipStream_t s, int kcount, int C_pad, int PT, const int *sf_row_a, const int *sf_col_c,
                        const int *k_sign, const double *G, double *sfacrl, double *sfacim);
void launch_b_project(hipStream_t s, const DevPlan &pl, int ne_pad, const int *ct_ptr /*[n_col_tiles+1]*/, const SkTile *tiles,
                      const double *Gwf, const double *Rp, const double *Tz, double *bk_part /*[4][ne_pad] overwritten*/);
// planar-electrode fast path of the projection (<= 64 distinct electrode z values)
void launch_reduce_project_zclass(hipStream_t s, const DevPlan &pl, const SkTile *tiles, int ntiles, int max_nsplit, double *part,
                                  double *G, int ne_pad, int n_own, const int *own_rt, int nzc, const double *Tzc, const double *Rp,
                                  const double2 *Xe /*[kxmax+2][ne_pad] electrode axis phases, last row zero*/, const double2 *Ye /*[kymax+1][ne_pad]*/,
                                  const int *own_pv /*[n_own][64] packed planar vectors of the own row tiles*/, const int *zclass, double *Hc, double *bk_part,
                                  const BRowArgs *fin /*non-NULL (needs fin->breal): the dot kernel finishes b itself*/);
void launch_b_project_zclass(hipStream_t s, const DevPlan &pl, int ne_pad, const int *rt_mine, int n_own, const int *own_rt, int nzc, const double *Gwf,
                             const double *Tzc /*[C_pad][64]*/, const double *Rp, const double2 *Xe, const double2 *Ye,
                             const int *own_pv, const int *zclass /*[ne_pad]*/,
                             double *Hc /*[4][R_pad][64]*/, double *bk_part /*[4][ne_pad]*/, const BRowArgs *fin);
// this rank's contribution to b in one launch: k-space halves + slab (rank 0) + real-space rows row0..row1
void launch_b_real_combine(hipStream_t s, int ne, int ne_pad, int row0, int row1, const int *row_ptr, const int *ele_atom,
                           const int *oth_atom, const double *x, const double *q, const int *type, RealParams rp, int add_k,
                           const double *bk, int slab, const double *ele_z, const double *slab_part, int n_slab_part,
                           double slab_pref, double *b_out, double *slab_out,
                           const double *breal = nullptr /*pair sums formed earlier in this update, or NULL: formed here*/);
// the same GEMV + charge write with the matrix taken as symmetric: packed lower-triangle tiles, half the bytes (conp_kernels.hip)
size_t sym_packed_doubles(int ne_pad);
// stat [2] (device): receives the bit patterns of max |S_ij| and max |S_ij - S_ji| -- how symmetric the matrix is
void launch_sym_pack(hipStream_t s, int ne, int ne_pad, const double *S, double *Spk, unsigned long long *stat);
void launch_sym_gemv_finish(hipStream_t s, int n, int ne_pad, const double *Spk, const double *b, double *yp /*[ne_pad / 128][ne_pad]*/,
                            double *y, const double *elesetq, const double *eleinitq, double potdiff, const int *atoms_ptr,
                            const int *atoms_of, const int *atoms_row /*row of every CSR entry*/, double *q_ele, double *q_atoms);
// the same GEMV + charge write for lattice-periodic electrodes: S_ij = T[basis_i][basis_j][cell_j - cell_i] (conp_kernels.hip,
// "GEMV with the projected inverse as a BLOCK-CIRCULANT matrix").  lat_row [nb][nx][ny] -> row, lat_pos [ne][3] = (basis, cx, cy).
struct LatShape {
  int R = 0;        // rows per thread, consecutive along y (4 where ny is a multiple of 4, else 1); 0: the form cannot run
  int sy = 0;       // LDS stride of a row of ny table / b entries
  int G = 0;        // basis atoms (table slabs + b vectors) staged at a time
  int CB = 0;       // cells per workgroup
  size_t lds = 0;   // bytes of dynamic LDS
};
LatShape lat_shape(int nx, int ny, int nb);
void launch_lat_table(hipStream_t s, int ne, int nb, int ncell, const double *S, const int *lat_row, double *T /*[nb][nb][nx][ny]*/);
// stat [2] (device): receives the bit patterns of max |S_ij| and max |S_ij - T[..]| -- how block-circulant the matrix is
void launch_lat_dev(hipStream_t s, int ne, int nx, int ny, int nb, const double *S, const int *lat_pos, const double *T,
                    unsigned long long *stat);
void launch_lat_gemv(hipStream_t s, const LatShape &sh, int nx, int ny, int nb, const double *T, const int *lat_row, const double *b,
                     double *y, const double *elesetq, const double *eleinitq, double potdiff, const int *atoms_ptr,
                     const int *atoms_of, double *q_ele, double *q_atoms);
void launch_gemv_rows(hipStream_t s, int n, int row0, int row1, const double *S, const double *b, double *y);
// all rows + the charge write of plain `fix conp` in one launch (atoms_ptr / atoms_of: electrode row -> its owned and ghost atoms)
void launch_gemv_finish(hipStream_t s, int n, const double *S, const double *b, double *y, const double *elesetq,
                        const double *eleinitq, double potdiff, const int *atoms_ptr, const int *atoms_of, double *q_ele,
                        double *q_atoms);
void launch_charge_finish(hipStream_t s, int ne, int nall, const int *atom2eleall, const int *elecheck, const double *eleallq,
                          const double *elesetq, const double *eleinitq, double potdiff, const double *d_potdiff, double *q_ele,
                          double *q_atoms, double *left_out);
void launch_cond_potdiff(hipStream_t s, int ne, const double *setzvec, const double *eleallq, const double *slab_part,
                         int n_slab_part, double lz, double rightcharge, double vmult, double *out);
void launch_conq_potdiff(hipStream_t s, const double *left, double rightcharge, double totsetq, int one_electrode, double *out);
size_t b_rows_scratch_bytes(int ne, size_t nneigh);
void launch_atom2eleall(hipStream_t s, int nall, int npairs, const int *pairs /*[npairs][2] = (atom, eleall)*/, int *atom2eleall /*[nall]*/);
void launch_build_b_rows(hipStream_t s, int inum, size_t nneigh, const int *ilist, const int *numneigh, const int *first,
                         const int *neigh, const int *arow, int nlocal, int newton, int ne, void *scratch, size_t scratch_bytes,
                         int *row_ptr, int *ele, int *oth, unsigned *np_pinned /*page-locked host word: the number of pairs, valid
                         after the stream has been synchronised*/);
void launch_post_force(hipStream_t s, int inum, const int *ilist, const int *numneigh, const int *first, const int *neigh, int nlocal,
                       int nall, int newton, const double *x,
                       const double *q, const int *type, const int *atom2eleall, RealParams rp, double qqrd2e, double *f,
                       double *acc /*[9]: eng_coul, virial[6], sum q^2 of owned electrode atoms, contributing pairs*/, bool clear_f);
// the device entry: forces added into f (NULL: none), out[9] = self energy, eng_coul, virial[6], contributing
// pairs (NULL: none); part: one row of 8 doubles per workgroup of four owners, (inum + 3) / 4 rows, every one written before it is read
void launch_post_force_device(hipStream_t s, int inum, const int *ilist, const int *numneigh, const int *first, const int *neigh,
                              int nlocal, int newton, const double *x, const double *q, const int *type, const int *atom2eleall,
                              RealParams rp, double qqrd2e, double k_self, double k_div, double *f, double *part, double *out);
// ---- pair forces of lj/cut/coul/long over the pair style's half list (conp_pair.hip) ----
constexpr int PAIR_TAB_W = 8;            // doubles per type pair: cutsq, cut_ljsq, lj1, lj2, lj3, lj4, offset, (pad)
constexpr int PAIR_LDS_ENTRIES = 256;    // type pairs, (ntypes + 1)^2, the LDS form of the table holds (16 KB); more: read from global
struct PairArgs {
  int inum;
  const int *ilist, *numneigh, *first, *neigh;
  int nlocal, newton;
  const double4 *xq;                     // [nall] (x, y, z, q), launch_pair_pack
  const int *type;                       // [nall]
  int nt1, ntab;                         // ntypes + 1, its square
  const double *tab;                     // [ntab][PAIR_TAB_W]
  double cut_coulsq, g_ewald, qqrd2e;
  double special_lj[4], special_coul[4];
  double *f;                             // [nall][3] accumulated, or NULL
  double *eatom, *vatom;                 // [nall], [nall][6]: accumulated (the caller zeroes them), or NULL
  double *part;                          // [inum][8] scratch rows of the eight sums (needed with ev != NULL)
};
void launch_pair_pack(hipStream_t s, int nall, const double *x, const double *q, double4 *xq);
// ev [8] = eng_vdwl, eng_coul, virial xx, yy, zz, xy, xz, yz (overwritten, summed in a fixed order), or NULL
void launch_pair_force(hipStream_t s, const PairArgs &a, double *ev);
// ---- the transposed half list and the atomic-free twins of the two pair entries (conp_transpose.hip) ----
struct TransposeArgs {                   // any flattened half list on the device; numneigh / first are read for listed owners only
  int inum;
  const int *ilist, *numneigh, *first, *neigh;
  int nall;
};
struct TransposedView {                  // own_row [nall], tr_ptr [nall + 1], tr_entry [tr_ptr[nall]] (conp_transpose.hpp)
  const int *own_row, *tr_ptr, *tr_entry;
  int nall;
};
// own_row (cleared to -1 by the caller); *flag |= 1: an owner listed twice, |= 2: an owner outside [0, nall)
void launch_tr_owners(hipStream_t s, const TransposeArgs &a, int *own_row, int *flag);
void launch_tr_count(hipStream_t s, const TransposeArgs &a, int *cnt /*[nall], cleared by the caller*/);
void launch_tr_close(hipStream_t s, int nall, const long long *total, int *tr_ptr);      // tr_ptr[nall] = *total
// keys [tr_ptr[nall]]: (slot << 32 | entry) of every listed slot, grouped by j in arrival order; cursor [nall] cleared by the caller
void launch_tr_fill(hipStream_t s, const TransposeArgs &a, const int *tr_ptr, int *cursor, long long *keys);
void launch_tr_sort(hipStream_t s, int nall, const int *tr_ptr, const long long *keys, int *tr_entry);   // by rank: ascending slot
// conp_pair_compute_ordered_device: launch_pair_force without a float atomic (one wavefront per receiving atom)
void launch_pair_force_ordered(hipStream_t s, const PairArgs &a, const TransposedView &t, double *ev);
// conp_fix_post_force_ordered_device: the forces of launch_post_force_device gathered per atom, one plain add per receiving atom
void launch_post_force_ordered(hipStream_t s, const TransposedView &t, const int *numneigh, const int *first, const int *neigh, int nlocal,
                               int newton, const double *x, const double *q, const int *type, const int *atom2eleall, RealParams rp,
                               double qqrd2e, double *f);
// ---- compute potential/atom on the device (conp_potatom.hip) ----
struct PotPairArgs {
  int ntotal, nlocal, ntypes;            // rows [0, ntotal) are written: nlocal (+ nghost with newton on)
  const int *numneigh, *first, *neigh;   // the pair style's half list (rows of listed owners only are read)
  const double *x, *q;                   // [nall][3], [nall]
  const int *type, *flags;               // [nall]; flags bit 0: selected, bit 1: eta_check
  const double *cutsq;                   // [ntypes + 1][ntypes + 1]
  double cut_coulsq, g_ewald, eta;
  double scale_owned, scale_ghost;       // what a selected owned / ghost row's sum is multiplied by before the store
  double *pot;                           // [ntotal] overwritten: 0.0 on unselected rows
};
// the pair part gathered per selected row in section 26's order, one store per row, no float atomic
void launch_pot_pair(hipStream_t s, const PotPairArgs &a, const TransposedView &t);
// x, q of the nt targets into xg [ntot][3], qg [ntot]; entries from nt on: the origin, no charge
void launch_pot_gather(hipStream_t s, int nt, int ntot, const int *targets, const double *x, const double *q, double *xg, double *qg);
struct PotFinishArgs {
  int nt, slab, qsum;
  const int *targets, *flags;            // [nt] owned rows; flags may be NULL with eta == 0
  const double *x, *q, *u;               // u [nlocal]: the k-space potential by owned index
  const double *four;                    // Q, Q2, M, M2 of the owned atoms (read under slab)
  double eta, pi2vol, evs;               // 2 pi / V, qqr2e / qe2f
  double *pot;                           // pot[i] = ((((pot[i] - u[i]) + eta self term) + z slabcorr) - qsum term) evs at the targets
};
void launch_pot_finish(hipStream_t s, const PotFinishArgs &a);
// ---- bonded forces of bond_style / angle_style harmonic (conp_bonded.hip) ----
constexpr int BONDED_BLOCK = 256;        // threads of a workgroup: one per term (term kernel), one per atom (gather kernel)
constexpr int BONDED_FINISH = 256;       // threads of the finishing workgroup: rows r, r + 256, ... per thread
constexpr int BONDED_TERM_W = 13;        // doubles per term record: f on member 1 [3], f on member 3 [3] (bond: 0), energy, v[6]
struct BondedArgs {
  int nbond, nangle, nlocal, nall, newton;
  const int *bond, *angle;               // [nbond][3] i1, i2, type; [nangle][4] i1, i2, i3, type
  const double *bcoef, *acoef;           // [nbondtypes + 1][2] k, r0; [nangletypes + 1][2] k, theta0
  double prd[3];                         // > 0: closest image along that dimension
  const double *x;                       // [nall][3]
  double *term;                          // [nbond + nangle][BONDED_TERM_W] scratch: bonds first, then angles
  double *part;                          // [ceil((nbond + nangle) / BONDED_BLOCK)][8] scratch rows (needed with ev != NULL)
  const int *slot_ptr, *slot;            // [nall + 1], [2 nbond + 3 nangle]: an atom's slots, term * 4 + role, in list order
  double *f;                             // [nall][3] accumulated, or NULL
  double *eatom, *vatom;                 // [nall], [nall][6] overwritten, or NULL
};
// ev [8] = ebond, eangle, virial xx, yy, zz, xy, xz, yz (overwritten, summed in a fixed order), or NULL
void launch_bonded(hipStream_t s, const BondedArgs &a, double *ev);
// ---- dihedral_style opls / harmonic and improper_style harmonic / cvff (conp_dihedral.hip) ----
constexpr int DIHEDRAL_BLOCK = 256;      // threads of a workgroup: one per term (term kernel), one per atom (gather kernel)
constexpr int DIHEDRAL_FINISH = 256;     // threads of the finishing workgroup: rows r, r + 256, ... per thread
constexpr int DIHEDRAL_TERM_W = 16;      // doubles per term record: f on member 1 [3], on 3 [3], on 4 [3], energy, v[6]: 128 bytes
enum { DIHEDRAL_NONE = 0, DIHEDRAL_OPLS = 1, DIHEDRAL_HARMONIC = 2 };
enum { IMPROPER_NONE = 0, IMPROPER_HARMONIC = 1, IMPROPER_CVFF = 2 };
struct DihedralArgs {
  int ndihedral, nimproper, nlocal, nall, newton;
  int dstyle, istyle;                    // DIHEDRAL_*, IMPROPER_*
  const int *dihedral, *improper;        // [ndihedral][5], [nimproper][5]: i1, i2, i3, i4, type
  const double *dcoef, *icoef;           // [ntypes + 1][4]: opls K1 K2 K3 K4; harmonic / cvff K d n 0; improper harmonic K chi0 0 0
  double prd[3];                         // > 0: closest image along that dimension
  const double *x;                       // [nall][3]
  double *term;                          // [ndihedral + nimproper][DIHEDRAL_TERM_W] scratch, 128-byte aligned: dihedrals first
  double *part;                          // [ceil((ndihedral + nimproper) / DIHEDRAL_BLOCK)][8] scratch rows (needed with ev != NULL)
  const int *slot_ptr, *slot;            // [nall + 1], [4 (ndihedral + nimproper)]: an atom's slots, term * 4 + role, in list order
  double *f;                             // [nall][3] accumulated, or NULL
  double *eatom, *vatom;                 // [nall], [nall][6] overwritten, or NULL
};
// ev [8] = edihedral, eimproper, virial xx, yy, zz, xy, xz, yz (overwritten, summed in a fixed order), or NULL
void launch_dihedral(hipStream_t s, const DihedralArgs &a, double *ev);
// ---- velocity Verlet and the Nose-Hoover chain (conp_integrate.hip) ----
constexpr int INTEGRATE_BLOCK = 256;     // threads of a workgroup: one per atom
constexpr int INTEGRATE_FINISH = 256;    // threads of the finishing workgroup: partial rows r, r + 256, ... per thread
constexpr int INTEGRATE_G = CONP_INTEGRATE_MAX_GROUPS;
constexpr int INTEGRATE_STATE_W = 12;    // doubles of a group's state row: eta[3], eta_dot[3], eta_dotdot[3], t_current, t_target, unused
enum { INTEGRATE_TEMPERATURE = 0, INTEGRATE_SETUP = 1, INTEGRATE_FINAL = 2 };      // what the finishing workgroup does with the sums
struct IntegrateArgs {
  int nlocal, ngroups;
  const int *type, *group;               // [nlocal]; group -1: the atom is neither read nor written
  const double *mass;                    // [ntypes + 1]
  double dtv, dtf, dthalf, dt4, dt8, mvv2e, boltz;
  int style[INTEGRATE_G];                // 0 = nve, 1 = nvt
  double dof[INTEGRATE_G], t_freq[INTEGRATE_G], t_target[INTEGRATE_G];
  double *x, *v;                         // [nlocal][3]
  const double *f;                       // [nlocal][3]
  const double *state_in;                // [ngroups][INTEGRATE_STATE_W]
  double *state_out;                     // initial: the OTHER state buffer (every workgroup reads state_in); finish, seed: may be state_in
  double *part;                          // [ceil(nlocal / INTEGRATE_BLOCK)][INTEGRATE_G] scratch rows
  double *factor;                        // [INTEGRATE_G] scratch: factor_eta of the final chain half-step (1.0 for nve)
  double *out;                           // [ngroups][4] t_current, ke, thermostat energy, eta_dot[0]; or NULL
};
// chain half-step in every workgroup, v *= factor_eta, nve_v, nve_x: one launch
void launch_integrate_initial(hipStream_t s, const IntegrateArgs &a);
// update: nve_v with the per-workgroup sums of m v^2 (else the sums alone); then the finishing workgroup in `mode`; scale: v *= factor
void launch_integrate_sums(hipStream_t s, const IntegrateArgs &a, bool update, int mode, bool scale);
// state_out rows from raw [ngroups][8] rows (eta, eta_dot, t_current, t_target) in a.state_in: eta_dotdot[k >= 1] as setup forms it
void launch_integrate_seed(hipStream_t s, const IntegrateArgs &a);
// ---- SHAKE bond and angle constraints (conp_shake.hip) ----
constexpr int SHAKE_BLOCK = 64;          // threads of a workgroup: one per cluster (and, with d_vatom, one per atom row to zero): one wave, no barrier
constexpr int SHAKE_FINISH = 256;        // threads of the finishing workgroup: partial rows r, r + 256, ... per thread
constexpr int SHAKE_PART_W = 9;          // doubles of a partial row: virial [6], unconverged, bad determinant, largest niter
enum { SHAKE_FORCE = 0, SHAKE_CORRECT = 1 };                 // add the constraint force into f, or move x by it (v = f = 0)
struct ShakeArgs {
  int ncluster, nlocal, max_iter;
  const int *cluster;                    // [ncluster][7] flag, i0, i1, i2, t0, t1, t2
  const int *type;                       // [nlocal]
  const int *member;                     // [nlocal] 1: the atom is in a cluster (its d_vatom row is the cluster's to write)
  const double *mass, *bond_d, *angle_d; // [ntypes + 1], [nbondtypes + 1], [nangletypes + 1]
  double dtv, dtfsq, tolerance;
  double prd[3];
  double *x;                             // [nlocal][3]; stored by SHAKE_CORRECT only
  const double *v;                       // [nlocal][3]; NULL with SHAKE_CORRECT
  double *f;                             // [nlocal][3] added to; NULL with SHAKE_CORRECT
  double *vatom;                         // [nlocal][6] overwritten, or NULL
  double *part;                          // [workgroups][SHAKE_PART_W] scratch rows, or NULL (no d_out)
};
// one launch over max(ncluster, vatom ? nlocal : 0) threads; out [9] != NULL: the finishing workgroup behind it
void launch_shake(hipStream_t s, const ShakeArgs &a, int mode, double *out);
// out [2] = largest |r - d| / d over the bonds, over the 1-2 distances of the flag-1 clusters
void launch_shake_check(hipStream_t s, const ShakeArgs &a, double *out);
inline int shake_rows(int nthreads) { return (nthreads + SHAKE_BLOCK - 1) / SHAKE_BLOCK; }     // workgroups, and rows of a.part
// ---- fix efield and the per-group thermo sums (conp_efield.hip) ----
constexpr int EFIELD_BLOCK = 256;        // threads of a workgroup: one per atom
constexpr int EFIELD_FINISH = 256;       // threads of the finishing workgroup: partial rows r, r + 256, ... per thread
constexpr int EFIELD_W = 11;             // doubles of a partial row and of d_out: energy, sum f [3], virial [6], selected atoms
constexpr int OBSERVE_BLOCK = 256;       // threads of a workgroup: one per atom
constexpr int OBSERVE_FINISH = 256;      // threads of a finishing workgroup (one per group): partial rows r, r + 256, ... per thread
constexpr int OBSERVE_W = CONP_OBSERVE_W;
struct EfieldArgs {
  int nlocal;
  const int *sel;                        // [nlocal] 0 / 1
  const double *x, *q;                   // [nlocal][3], [nlocal]
  const int *image;                      // [nlocal][3] or NULL: u = x
  double *f;                             // [nlocal][3] added to (selected rows only)
  double ex, ey, ez;                     // qe2f e; ez is used where scalar == NULL
  double qe2f, e2, couple_scale;         // scalar != NULL: ez = qe2f (e2 + couple_scale *scalar), formed by every thread
  const double *scalar;                  // the fix scalar's slot of the handle (conq, cond), or NULL
  double prd[3];
  double *vatom;                         // [nlocal][6] overwritten (unselected rows: 0.0), or NULL
  double *part;                          // [ceil(nlocal / EFIELD_BLOCK)][EFIELD_W] scratch rows, or NULL (no d_out)
};
// one launch over the owned atoms; out [EFIELD_W] != NULL: the finishing workgroup behind it
void launch_efield(hipStream_t s, const EfieldArgs &a, double *out);
struct ObserveArgs {
  int nlocal, ngroups;
  const int *type, *mask;                // [nlocal]; bit g of mask: member of group g
  const double *mass;                    // [ntypes + 1]
  const double *x, *q;                   // [nlocal][3], [nlocal]
  const double *v;                       // [nlocal][3] or NULL: columns 5-8 are 0.0
  const int *image;                      // [nlocal][3] or NULL: u = x
  double prd[3];
  double *part;                          // [ceil(nlocal / OBSERVE_BLOCK)][ngroups][OBSERVE_W] scratch rows
};
// the per-workgroup rows, then ngroups finishing workgroups: out [ngroups][OBSERVE_W]
void launch_observe(hipStream_t s, const ObserveArgs &a, double *out);
inline int efield_rows(int nlocal) { return (nlocal + EFIELD_BLOCK - 1) / EFIELD_BLOCK; }
inline int observe_rows(int nlocal) { return (nlocal + OBSERVE_BLOCK - 1) / OBSERVE_BLOCK; }
// ---- fix zmirror (conp_zmirror.hip) ----
constexpr int ZMIRROR_BLOCK = 256;       // threads of a workgroup: one per (source, target) pair
// x[dst] = (x[src][0], x[src][1], zoffset - x[src][2]) for the npairs records of `map` (x: source, y: target)
void launch_zmirror(hipStream_t s, int npairs, const int2 *map, double zoffset, double *x);
// ---- the pair style's half list built on the device (conp_neigh.hip) ----
struct NeighGrid { double lo[3], inv[3]; int n[3]; };     // cell of v along c: clamp((v - lo[c]) * inv[c], 0, n[c] - 1); cells are >= cutneigh wide
struct NeighRowArgs {
  int nlocal, newton;
  const double *x;                       // [nall][3]
  double cutneighsq;
  NeighGrid g;
  const int *cell, *start;               // [nall] cell of an atom; [ncell + 1] first member of a cell in `sorted`
  const double4 *sorted;                 // [nall] (x, y, z, atom index), cell by cell, ascending index inside a cell
  const int *tag, *nspecial, *special;   // special bonds: [nall], [nlocal][3] cumulative, [nlocal][maxspecial] tags; tag NULL: none
  int maxspecial;
  int flagged[4];                        // class 1..3: its factors on the handle are not both 1.0 (the bits are stored)
  double prd_half[3];                    // LAMMPS' minimum_image_check: 0 in a non-periodic dimension
  int *numneigh;                         // [nall]: written by the count pass, read by the fill pass
  const int *first;                      // [nall] (fill pass)
  int *neigh;                            // (fill pass)
};
void launch_neigh_extent(hipStream_t s, int nall, const double *x, double *ext /*[7]: lo[3], hi[3], 1.0 if a coordinate is not finite*/);
// cell / slot / unsorted [nall], count [ncell], start [ncell + 1], total: the member count (= nall)
void launch_neigh_bin(hipStream_t s, int nall, const double *x, const NeighGrid &g, int *cell, int *slot, int *count, int *start,
                      long long *total, int *unsorted, double4 *sorted);
void launch_neigh_rows(hipStream_t s, const NeighRowArgs &a, bool fill);
// neigh_modify exclude: the rules travel in the kernel arguments, the type table is a device array
constexpr int NEIGH_EXCL_MAX = 16;       // group rules, and molecule rules
struct NeighExclArgs {
  int ntype, ngroup, nmol;               // rules in force of each kind (ntype: 0 or 1 -- the table is consulted or not)
  int nt1;                               // ntypes + 1: the width of ex_type
  const unsigned char *ex_type;          // [nt1][nt1] 0 / 1, row and column 0 clear
  int gbit1[NEIGH_EXCL_MAX], gbit2[NEIGH_EXCL_MAX];
  int mbit[NEIGH_EXCL_MAX];
  unsigned mintra;                       // bit m: molecule rule m is molecule/intra, else molecule/inter
  const int *type, *mask, *molecule;     // [nall] each; NULL where no rule in force reads it
};
// the rows of launch_neigh_rows without the candidates Neighbor::exclusion drops (an excluded lane votes 0)
void launch_neigh_rows_exclude(hipStream_t s, const NeighRowArgs &a, const NeighExclArgs &ex, bool fill);
void launch_neigh_scan(hipStream_t s, int n, const int *in, int *out /*[n] exclusive*/, long long *total);
void launch_neigh_iota(hipStream_t s, int n, int *out);
void launch_neigh_moved(hipStream_t s, int nlocal, const double *x, const double *xb, double trigsq, int *flag);
// ---- ghost atoms built, updated and folded back on the device (conp_ghost.hip) ----
struct GhostBuildArgs {
  int nlocal, nblock, nshift;            // owners, blocks of 64 owners, shifts
  const double *x;                       // [nlocal][3]
  const int *shift;                      // [nshift][3], sx slowest, sz fastest, without (0, 0, 0)
  double prd[3], lo[3], hi[3];           // box lengths; box bounds widened by cutghost
  int *count;                            // [nshift][nblock] images kept (count pass)
  int *nimg;                             // [nlocal] images per owner: written by the count pass, read by the fill pass
  const int *start, *ofirst;             // exclusive scans of count and nimg (fill pass)
  int nghost;                            // (fill pass)
  int *owner, *img, *list;               // [nghost], [nghost][3], [nghost]: an owner's ghosts at list[ofirst[o] .. + nimg[o]), ascending
};
void launch_ghost_images(hipStream_t s, const GhostBuildArgs &a, bool fill);
void launch_ghost_fill_xq(hipStream_t s, int nlocal, int nghost, const int *owner, const int *img, double px, double py, double pz, double *x,
                          double *q /*[nall] or NULL*/);
void launch_ghost_fill_int(hipStream_t s, int nlocal, int nghost, int width, const int *owner, int *v /*[nlocal + nghost][width]*/);
void launch_ghost_fold(hipStream_t s, int nlocal, int width, const int *ofirst, const int *nimg, const int *list, double *v /*[nlocal + nghost][width]*/);
struct AtomsWrapArgs { int nlocal, periodic[3]; double lo[3], hi[3], prd[3]; };
void launch_atoms_wrap(hipStream_t s, const AtomsWrapArgs &a, double *x /*[nlocal][3]*/, int *image /*[nlocal][3] or NULL*/);
// ---- the fix's re-neighbouring on the device (conp_reneigh.hip) ----
void launch_ren_ghost_rows(hipStream_t s, int nlocal, int nghost, const int *owner, int *type /*[nall]*/, int *atom2eleall /*[nall]*/);
// pred 0: atoms i < n with atom2eleall[i] >= 0 -> out[k] = (i, atom2eleall[i]); pred 1: atom2eleall[i] < 0 and q[i] != 0 -> out[k] = i.
// count / start: one entry per block of 64 atoms; the fill pass stores at most `cap` entries
void launch_ren_compact(hipStream_t s, int pred, bool fill, int n, const int *atom2eleall, const double *q, int *count, const int *start,
                        int cap, int *out);
void launch_ren_csr_count(hipStream_t s, int nlocal, int ne, const int *atom2eleall, const int *nimg /*[nlocal] or NULL: no ghosts*/,
                          int *own_of /*[ne]*/, int *cnt /*[ne + 1], zeroed by the caller*/);
void launch_ren_csr_fill(hipStream_t s, int nlocal, int ne, int cap, const int *own_of, const int *ptr /*[ne + 1]*/, const int *ofirst,
                         const int *nimg, const int *list, int *of /*[cap]*/, int *rowof /*[cap]*/);
// the z grid of Fix::zn_order_list: n cells, window width w, gscale = n / lz, rn = 1 / n, n_below = nextafter(n, 0)
struct ZnOrderArgs { int n, w; double gscale, rn, n_below; };
void launch_ren_zcell(hipStream_t s, const ZnOrderArgs &a, int nl_max, const long long *nl_dev, const int *list, const double *x,
                      int *cell /*[nl]*/, double *uw /*[nl]*/, int *occ /*[n], zeroed by the caller*/);
// count / start: [n][ceil(nl / 256)], key-major; the count pass needs `count` zeroed
void launch_ren_zsort(hipStream_t s, const ZnOrderArgs &a, bool fill, int nl, int c_start, const int *list, const int *cell, const double *uw,
                      int *count, const int *start, int *sorted /*[nl]*/, int *i0s /*[nl]*/);
void launch_ren_chunk_bounds(hipStream_t s, int nl, const int *i0s, int *lo /*[ceil(nl / 16)]*/, int *hi);
void launch_left_sum(hipStream_t s, int ne, const int *elecheck, const double *v, double *out);
void launch_results_out(hipStream_t s, int ne, const int *elecheck, const double *v, double *scal, bool do_left, const double *qele,
                        double *host_q /*page-locked host memory*/, double *host_scal);

// ---- once-per-run matrix work ------------------------------------------------------------------
// electrode phase tables on the device (conp_tables.hip; km_ewald.cpp:426-531).  seeds: [6][ne] = (cos, sin)(unitk_c x_ic) per axis,
// from the host's libm; the target buffers must be zeroed (padding rows and atoms stay zero).
void launch_ele_tables(hipStream_t s, const DevPlan &pl, int kzt, int ne, int ne_pad, const double *seeds, double2 *Xe /*[kxmax+2][ne_pad]*/,
                       double2 *Ye /*[kymax+1][ne_pad]*/, double *Tz /*[C_pad][ne_pad]*/, double *Rp /*[R_pad][ne_pad]*/);
// Tzc[t][c] = Tz[t][rep[c]] ([C_pad][64]) and its class-major copy TzcT ([nzc][C_pad])
void launch_ele_zclass(hipStream_t s, int C_pad, int ne_pad, int nzc, const int *rep, const double *Tz, double *Tzc, double *TzcT);
int a_kspace_nsplit(int ne_pad, int num_cus, int nchunk, int nranks);
// planar electrodes: the same matrix through the z-class factorisation (contraction over the planar rows only)
void launch_a_kspace_zclass(hipStream_t s, const DevPlan &pl, int ne, int ne_pad, int nzc, const double *Rp, const double *Tzc,
                            const int *zclass, double *Wz /*[R_pad * nzc * nzc] scratch*/, double *A, int rank, int nranks);
// rank r of nranks computes the lower-triangle tiles r, r + nranks, ... into its zero-initialised A
void launch_a_kspace(hipStream_t s, const DevPlan &pl, int ne, int ne_pad, const double *Rp, const double *Tz, double *A, int nsplit,
                     const int *chunk_group, int rank, int nranks);
void launch_a_diag_slab(hipStream_t s, int ne, double diag_k, double diag_self, const double *diag_self_atom /*[ne] or NULL*/,
                        int slab, double pref, const double *ele_z, double *A);
void launch_a_real(hipStream_t s, int ne, int row0, int row1, const int *row_ptr, const int *ele_atom, const int *oth_atom,
                   const int *col, const double *x, const int *type, RealParams rp, double *A);
void launch_a_symmetrise(hipStream_t s, int ne, double *A);
void launch_inv_project(hipStream_t s, int n, double *A, int use_mask, const unsigned char *mask, double *ainve,
                        double *totinve /*device scalar*/, int apply);
void launch_inv_project_apply(hipStream_t s, int n, double *A, const double *ainve, const double *totinve);
// in-place inverse (conp_inverse.hip): blocked Gauss-Jordan with partial pivoting; *info != 0 -> singular
size_t inverse_workspace_doubles(int n);
// returns true when the multi-workgroup panel was used (then info == -7 means "a grid barrier timed out": restore M, repeat
// with multi_wg = false)
// symmetric positive definite matrices: no pivot search, no grid barrier (conp_inverse.hip); info = -8: not positive definite
void launch_symmetry_check(hipStream_t s, int n, const double *M, int *flag_dev);
void launch_inverse_spd(hipStream_t s, int n, double *M, double *work, int *info /*[1]*/);
bool launch_inverse(hipStream_t s, int n, double *M, double *work, int *piv_all /*[n]*/, int *info /*[1]*/, int num_cus,
                    bool multi_wg, int max_wg /*0: no cap*/, unsigned spin_limit /*polls of the panel's grid barrier before info = -7*/);
// CG (fix_conp.cpp:864-930): state vectors on device; returns via *d_done
void launch_cg_init(hipStream_t s, int n, const double *A, const double *b, double *q, double *res, double *p,
                    double *scal /*[8]*/);
void launch_cg_iter(hipStream_t s, int n, const double *A, double *q, double *res, double *p, double *ap, double *scal,
                    double tolerance, int *done, int iter, double *hist);
// one launch per CG iteration (update of iteration iter - 1 repeated by every workgroup + its rows of the matvec); see the kernel
bool cg_step_fits(int n);
void launch_cg_step(hipStream_t s, int n, const double *A, const double *b, double *q, double *res2 /*[2][n]*/, double *p2 /*[2][n]*/,
                    double *ap2 /*[2][n]*/, double *scal, double tolerance, int *done, int iter, double *hist, int mode,
                    double *host_ctl = nullptr /*page-locked host memory: mode 4 stores n_ctl doubles of scal there*/, int n_ctl = 0);

}  // namespace conp
