// Velocity Verlet and the Nose-Hoover chain thermostat of `fix nve` / `fix nvt` -- the conp_integrate_* entries of include/conp_hip.h,
// DESIGN.md section 22.
//
// The arithmetic is LAMMPS' FixNH / FixNVE / ComputeTemp @ 27May2021 at tchain 3, tloop 1, drag 0, restated in the header.  Products
// are kept as written (fp contract off).  The chain lives in a state row per group on the device; nothing is read back, and no
// output meets an atomic:
//
//   integrate_initial_kernel   one thread per atom.  The first ngroups threads of EVERY workgroup redo the chain half-step of their
//                              group from the state buffer the launch reads (a dozen scalar operations and four exp) and leave
//                              factor_eta in LDS; workgroup 0 alone stores the new rows, into the OTHER state buffer, so no workgroup
//                              reads what another writes.  Then v *= factor_eta (nvt), nve_v, nve_x.
//   integrate_sums_kernel      <UPDATE>: nve_v (final) or nothing (setup, temperature); the atom's m v^2 goes, per group, through a
//                              fixed tree over the workgroup into one row of partial sums per workgroup.
//   integrate_finish_kernel    one workgroup: adds the rows in a fixed order (the scheme of bonded_finish_kernel), then thread g
//                              finishes group g: the temperature, and by mode the setup, or the chain half-step with factor_eta
//                              left in a.factor, and the d_out row.
//   integrate_scale_kernel     v *= factor_eta for the atoms of nvt groups.
//   integrate_seed_kernel      conp_integrate_set_state: the state rows from the caller's, eta_dotdot[k >= 1] as setup forms it.
//
// Atoms with group -1 and rows from nlocal on are neither loaded nor stored.  No thread returns before a barrier.
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

__device__ __forceinline__ double integrate_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// a group's chain in registers: eta_dot[3] is the constant 0 behind the chain's end
struct Chain {
  double eta[3], ed[4], edd[3], t_current, t_target;
};

__device__ __forceinline__ Chain chain_load(const double *row) {
  Chain c;
#pragma unroll
  for (int k = 0; k < 3; ++k) { c.eta[k] = row[k]; c.ed[k] = row[3 + k]; c.edd[k] = row[6 + k]; }
  c.ed[3] = 0.0;
  c.t_current = row[9]; c.t_target = row[10];
  return c;
}

__device__ __forceinline__ void chain_store(double *row, const Chain &c) {
#pragma unroll
  for (int k = 0; k < 3; ++k) { row[k] = c.eta[k]; row[3 + k] = c.ed[k]; row[6 + k] = c.edd[k]; }
  row[9] = c.t_current; row[10] = c.t_target; row[11] = 0.0;
}

// eta_mass[*] from the stored t_target
__device__ __forceinline__ void chain_masses(const Chain &c, double dof, double t_freq, double boltz, double &kt, double (&em)[3]) {
#pragma clang fp contract(off)
  kt = boltz * c.t_target;
  const double tf2 = t_freq * t_freq;
  em[0] = dof * kt / tf2;
  em[1] = kt / tf2;
  em[2] = kt / tf2;
}

// eta_dotdot[k >= 1] of FixNH::setup
__device__ __forceinline__ void chain_setup(Chain &c, double dof, double t_freq, double boltz) {
#pragma clang fp contract(off)
  double kt, em[3];
  chain_masses(c, dof, t_freq, boltz, kt, em);
#pragma unroll
  for (int k = 1; k < 3; ++k) c.edd[k] = (em[k - 1] * c.ed[k - 1] * c.ed[k - 1] - kt) / em[k];
}

// FixNH::nhc_temp_integrate, steps 1-10 of the header -> factor_eta
__device__ __forceinline__ double chain_half_step(Chain &c, double dof, double t_freq, const IntegrateArgs &a) {
#pragma clang fp contract(off)
  double kt, em[3];
  chain_masses(c, dof, t_freq, a.boltz, kt, em);
  const double ke_target = dof * kt;
  c.edd[0] = (dof * a.boltz * c.t_current - ke_target) / em[0];
  double e = 1.0;
#pragma unroll
  for (int k = 2; k >= 1; --k) {
    e = exp(-a.dt8 * c.ed[k + 1]);
    c.ed[k] *= e;
    c.ed[k] += c.edd[k] * a.dt4;
    c.ed[k] *= e;
  }
  e = exp(-a.dt8 * c.ed[1]);
  c.ed[0] *= e;
  c.ed[0] += c.edd[0] * a.dt4;
  c.ed[0] *= e;
  const double factor = exp(-a.dthalf * c.ed[0]);
  c.t_current *= factor * factor;
  c.edd[0] = (dof * a.boltz * c.t_current - ke_target) / em[0];
#pragma unroll
  for (int k = 0; k < 3; ++k) c.eta[k] += a.dthalf * c.ed[k];
  c.ed[0] *= e;
  c.ed[0] += c.edd[0] * a.dt4;
  c.ed[0] *= e;
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    e = exp(-a.dt8 * c.ed[k + 1]);
    c.ed[k] *= e;
    c.edd[k] = (em[k - 1] * c.ed[k - 1] * c.ed[k - 1] - kt) / em[k];
    c.ed[k] += c.edd[k] * a.dt4;
    c.ed[k] *= e;
  }
  return factor;
}

// FixNH::compute_scalar at tchain 3 without a barostat
__device__ __forceinline__ double chain_energy(const Chain &c, double dof, double t_freq, double boltz) {
#pragma clang fp contract(off)
  double kt, em[3];
  chain_masses(c, dof, t_freq, boltz, kt, em);
  const double ke_target = dof * kt;
  double energy = ke_target * c.eta[0] + 0.5 * em[0] * c.ed[0] * c.ed[0];
#pragma unroll
  for (int k = 1; k < 3; ++k) energy += kt * c.eta[k] + 0.5 * em[k] * c.ed[k] * c.ed[k];
  return energy;
}

__global__ __launch_bounds__(INTEGRATE_BLOCK) void integrate_initial_kernel(IntegrateArgs a) {
#pragma clang fp contract(off)
  __shared__ double fac[INTEGRATE_G];
  if (threadIdx.x < a.ngroups) {
    const int g = threadIdx.x;
    Chain c = chain_load(a.state_in + (size_t)g * INTEGRATE_STATE_W);
    double factor = 1.0;
    if (a.style[g]) {
      c.t_target = a.t_target[g];
      factor = chain_half_step(c, a.dof[g], a.t_freq[g], a);
    }
    if (blockIdx.x == 0) chain_store(a.state_out + (size_t)g * INTEGRATE_STATE_W, c);
    fac[g] = factor;
  }
  __syncthreads();
  const int i = blockIdx.x * INTEGRATE_BLOCK + threadIdx.x;
  if (i < a.nlocal) {
    const int g = a.group[i];
    if (g >= 0) {
      const size_t o = 3 * (size_t)i;
      const double factor = fac[g];
      const double dtfm = a.dtf / a.mass[a.type[i]];
      double vx = a.v[o], vy = a.v[o + 1], vz = a.v[o + 2];
      if (factor != 1.0) { vx *= factor; vy *= factor; vz *= factor; }
      vx += dtfm * a.f[o]; vy += dtfm * a.f[o + 1]; vz += dtfm * a.f[o + 2];
      a.v[o] = vx; a.v[o + 1] = vy; a.v[o + 2] = vz;
      a.x[o] += a.dtv * vx; a.x[o + 1] += a.dtv * vy; a.x[o + 2] += a.dtv * vz;
    }
  }
}

template <bool UPDATE>
__global__ __launch_bounds__(INTEGRATE_BLOCK) void integrate_sums_kernel(IntegrateArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[INTEGRATE_BLOCK / 64][INTEGRATE_G];
  const int i = blockIdx.x * INTEGRATE_BLOCK + threadIdx.x;
  int g = -1;
  double mv2 = 0.0;
  if (i < a.nlocal) {
    g = a.group[i];
    if (g >= 0) {
      const size_t o = 3 * (size_t)i;
      const double m = a.mass[a.type[i]];
      double vx = a.v[o], vy = a.v[o + 1], vz = a.v[o + 2];
      if (UPDATE) {
        const double dtfm = a.dtf / m;
        vx += dtfm * a.f[o]; vy += dtfm * a.f[o + 1]; vz += dtfm * a.f[o + 2];
        a.v[o] = vx; a.v[o + 1] = vy; a.v[o + 2] = vz;
      }
      mv2 = (vx * vx + vy * vy + vz * vz) * m;
    }
  }
  for (int k = 0; k < a.ngroups; ++k) {
    const double s = integrate_wave_sum(g == k ? mv2 : 0.0);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < INTEGRATE_G) {
    double t = 0.0;
    if (threadIdx.x < a.ngroups)
      for (int w = 0; w < INTEGRATE_BLOCK / 64; ++w) t += red[w][threadIdx.x];
    a.part[INTEGRATE_G * (size_t)blockIdx.x + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(INTEGRATE_FINISH) void integrate_finish_kernel(IntegrateArgs a, int nrows, int mode) {
#pragma clang fp contract(off)
  __shared__ double red[INTEGRATE_FINISH / 64][INTEGRATE_G];
  double s[INTEGRATE_G];
#pragma unroll
  for (int k = 0; k < INTEGRATE_G; ++k) s[k] = 0.0;
  for (int r = threadIdx.x; r < nrows; r += INTEGRATE_FINISH) {
#pragma unroll
    for (int k = 0; k < INTEGRATE_G; ++k) s[k] += a.part[INTEGRATE_G * (size_t)r + k];
  }
#pragma unroll
  for (int k = 0; k < INTEGRATE_G; ++k) s[k] = integrate_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < INTEGRATE_G; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < a.ngroups) {
    const int g = threadIdx.x;
    double t = 0.0;
    for (int w = 0; w < INTEGRATE_FINISH / 64; ++w) t += red[w][g];
    const double dof = a.dof[g], t_freq = a.t_freq[g];
    const bool nvt = a.style[g] != 0;
    double t_current = t * (a.mvv2e / (dof * a.boltz));
    double ke = 0.5 * a.mvv2e * t;
    Chain c = chain_load(a.state_in + (size_t)g * INTEGRATE_STATE_W);
    if (mode == INTEGRATE_SETUP) {
      c.t_current = t_current;
      if (nvt) {
        c.t_target = a.t_target[g];
        chain_setup(c, dof, t_freq, a.boltz);
      }
      chain_store(a.state_out + (size_t)g * INTEGRATE_STATE_W, c);
    } else if (mode == INTEGRATE_FINAL) {
      c.t_current = t_current;
      double factor = 1.0;
      if (nvt) {
        factor = chain_half_step(c, dof, t_freq, a);
        ke *= factor * factor;          // of the velocities the scale leaves, as FixNH forms its t_current
      }
      chain_store(a.state_out + (size_t)g * INTEGRATE_STATE_W, c);
      a.factor[g] = factor;
      t_current = c.t_current;
    }
    if (a.out) {
      double *o = a.out + 4 * (size_t)g;
      o[0] = t_current;
      o[1] = ke;
      o[2] = nvt ? chain_energy(c, dof, t_freq, a.boltz) : 0.0;
      o[3] = nvt ? c.ed[0] : 0.0;
    }
  }
}

__global__ __launch_bounds__(INTEGRATE_BLOCK) void integrate_scale_kernel(IntegrateArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * INTEGRATE_BLOCK + threadIdx.x;
  if (i < a.nlocal) {
    const int g = a.group[i];
    if (g >= 0) {
      const double factor = a.factor[g];
      if (factor != 1.0) {
        const size_t o = 3 * (size_t)i;
        a.v[o] *= factor; a.v[o + 1] *= factor; a.v[o + 2] *= factor;
      }
    }
  }
}

__global__ __launch_bounds__(64) void integrate_seed_kernel(IntegrateArgs a) {
#pragma clang fp contract(off)
  if (threadIdx.x < a.ngroups) {
    const int g = threadIdx.x;
    const double *raw = a.state_in + 8 * (size_t)g;
    Chain c;
    const bool nvt = a.style[g] != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { c.eta[k] = nvt ? raw[k] : 0.0; c.ed[k] = nvt ? raw[3 + k] : 0.0; c.edd[k] = 0.0; }
    c.ed[3] = 0.0;
    c.t_current = raw[6]; c.t_target = raw[7];
    if (nvt) chain_setup(c, a.dof[g], a.t_freq[g], a.boltz);
    chain_store(a.state_out + (size_t)g * INTEGRATE_STATE_W, c);
  }
}

inline int integrate_rows(int nlocal) { return (nlocal + INTEGRATE_BLOCK - 1) / INTEGRATE_BLOCK; }

}  // namespace

void launch_integrate_initial(hipStream_t s, const IntegrateArgs &a) {
  hipLaunchKernelGGL(integrate_initial_kernel, dim3(integrate_rows(a.nlocal)), dim3(INTEGRATE_BLOCK), 0, s, a);
}

void launch_integrate_sums(hipStream_t s, const IntegrateArgs &a, bool update, int mode, bool scale) {
  const int nrows = integrate_rows(a.nlocal);
  if (nrows > 0) {
    if (update) hipLaunchKernelGGL((integrate_sums_kernel<true>), dim3(nrows), dim3(INTEGRATE_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((integrate_sums_kernel<false>), dim3(nrows), dim3(INTEGRATE_BLOCK), 0, s, a);
  }
  hipLaunchKernelGGL(integrate_finish_kernel, dim3(1), dim3(INTEGRATE_FINISH), 0, s, a, nrows, mode);
  if (scale && nrows > 0) hipLaunchKernelGGL(integrate_scale_kernel, dim3(nrows), dim3(INTEGRATE_BLOCK), 0, s, a);
}

void launch_integrate_seed(hipStream_t s, const IntegrateArgs &a) {
  hipLaunchKernelGGL(integrate_seed_kernel, dim3(1), dim3(64), 0, s, a);
}

}  // namespace conp
