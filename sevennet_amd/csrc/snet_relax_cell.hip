// Batched variable-cell FIRE relaxation step (unit masses): one workgroup per system, every per-system sum in a fixed order.
//
// The rule is that of ASE's UnitCellFilter under ASE's FIRE (written out in include/snet_hip.h, snet_fire_cell_step): the n atoms
// in the frame of the reference cell and the three rows of n F, F the deformation gradient, are one system of n + 3 rows for
// the FIRE step of snet_relax.hip.  Positions, cells, both velocity arrays and the per-system state stay on the device between
// steps; the host reads back n_active only.  Nothing of a system is written before its new cell has passed the guard.
#include "snet_system.h"

namespace {

using namespace snet;   // the shared device helpers (snet_system.h)

constexpr int FIRE_THREADS = 256;
constexpr int FIRE_WAVES = FIRE_THREADS / 64;

// (ticket << 32) | systems still active, of the launch in flight (as g_fire_arrivals of snet_relax.hip, and apart from it)
__device__ unsigned long long g_fire_cell_arrivals = 0ull;

struct FireCellParams {
  FireParams fire;
  double pressure, min_height;
  int mask_bits, hydrostatic, constant_volume;
};

// the force g = f F and the velocity v of atom i in the reference frame, F the deformation gradient; HOLD: both are 0, by selection,
// for an atom with a bit of its mask set (whole atoms only), so that it keeps its coordinates in the reference frame.  The
// selection stands behind the product: a free atom's g is formed from the same operands, in the same text, as without a mask.
template <bool HOLD>
__device__ __forceinline__ void load_atom(const float *__restrict__ forces, const double *__restrict__ forces_extra,
                                          const double *__restrict__ vel, const int32_t *__restrict__ hold, int64_t i,
                                          const double *F, double (&g)[3], double (&v)[3]) {
  double f[3];
  load_force(forces, forces_extra, i, f);
  row_mul(f, F, g);
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = vel[3 * i + k];
  if constexpr (HOLD) {
    const int h = held_bits(hold, i) != 0 ? 7 : 0;
    zero_held(h, g);
    zero_held(h, v);
  }
}

// HOLD = false (snet_fire_cell_step) never reads `hold`
template <bool HOLD>
__global__ __launch_bounds__(FIRE_THREADS) void fire_cell_step_kernel(
    double *__restrict__ pos, double *__restrict__ vel, double *__restrict__ cell, double *__restrict__ vel_cell,
    const double *__restrict__ cell0, const float *__restrict__ forces, const double *__restrict__ forces_extra,
    const int32_t *__restrict__ hold, const double *__restrict__ virial, const double *__restrict__ virial_extra, int64_t n, const int32_t *__restrict__ seg_ptr,
    int n_sys, double *__restrict__ dt_s, double *__restrict__ alpha_s, int32_t *__restrict__ n_pos_s, int32_t *__restrict__ active_s,
    int32_t *__restrict__ n_steps_s, int32_t *__restrict__ status_s, double *__restrict__ fmax_sys, int32_t *__restrict__ n_active,
    FireCellParams p) {
  __shared__ double sm[FIRE_WAVES][4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  bool still_active = false;
  if (active_s[s] == 1) {   // (uniform over the workgroup; so is everything below that is not indexed by an atom)
    const Segment seg = segment(seg_ptr, s, n);
    const int64_t a0 = seg.a0, a1 = seg.a1;
    const double n_at = (double)(a1 - a0);
    // every thread reads the system's state before the first barrier; thread 0 writes it after the last
    double C[9], C0[9], vc[9], w6[6];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      C[k] = cell[9 * (int64_t)s + k];
      C0[k] = cell0[9 * (int64_t)s + k];
      vc[k] = vel_cell[9 * (int64_t)s + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) w6[k] = virial[6 * (int64_t)s + k] + (virial_extra ? virial_extra[6 * (int64_t)s + k] : 0.0);
    double dt = dt_s[s], alpha = alpha_s[s];
    int n_pos = n_pos_s[s];
    // F = (C0^-1 C)^T, F^-1, and the cell force G
    double F[9], Finv[9], G[9];
    {
      double C0inv[9], Ct[9];
      inv3(C0, det3(C0), C0inv);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Ct[3 * i + j] = C[3 * j + i];
      mul_abt(Ct, C0inv, F);   // C^T C0^-T
      inv3(F, det3(F), Finv);
      const double pv = p.pressure * fabs(det3(C));
      const double W[9] = {w6[0] - pv, w6[3], w6[5], w6[3], w6[1] - pv, w6[4], w6[5], w6[4], w6[2] - pv};
      mul_abt(W, Finv, G);     // W F^-T
      if (p.hydrostatic) {
        const double t = (G[0] + G[4] + G[8]) / 3.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) G[k] = 0.0;
        G[0] = G[4] = G[8] = t;
      }
      const int voigt[9] = {0, 5, 4, 5, 1, 3, 4, 3, 2};   // xx,yy,zz,yz,xz,xy
#pragma unroll
      for (int k = 0; k < 9; ++k) G[k] *= ((p.mask_bits >> voigt[k]) & 1) ? 1.0 : 0.0;
      if (p.constant_volume) {
        const double t = (G[0] + G[4] + G[8]) / 3.0;
        G[0] -= t, G[4] -= t, G[8] -= t;
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) G[k] /= n_at;
    }
    // pass 1 over the n + 3 rows: max |g_i|^2, g.v, |g|^2, |v|^2
    double f2max = 0.0;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = a0 + tid; i < a1; i += FIRE_THREADS) {
      double g[3], v[3];
      load_atom<HOLD>(forces, forces_extra, vel, hold, i, F, g, v);
      const double vx = v[0], vy = v[1], vz = v[2];
      const double f2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
      f2max = max_nan(f2, f2max);
      acc[0] += g[0] * vx + g[1] * vy + g[2] * vz;
      acc[1] += f2;
      acc[2] += vx * vx + vy * vy + vz * vz;
    }
    block_max_nan_put(f2max, sm);
    block_sum<3>(acc, sm);   // (its first barrier also publishes the four maxima; sm[.][3] is not rewritten in this launch)
    f2max = block_max_nan_get(sm);
#pragma unroll
    for (int r = 0; r < 3; ++r) {   // the cell rows, after the atoms
      const double *g = G + 3 * r, *v = vc + 3 * r;
      const double f2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
      f2max = max_nan(f2, f2max);
      acc[0] += g[0] * v[0] + g[1] * v[1] + g[2] * v[2];
      acc[1] += f2;
      acc[2] += v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    }
    const double fm = sqrt(f2max);
    if (fm < p.fire.fmax) {
      if (tid == 0) {
        fmax_sys[s] = fm;
        active_s[s] = 0;
        status_s[s] = 1;
      }
    } else {
      const FireMix mix = fire_decide(acc[0], p.fire, dt, alpha, n_pos);   // (every thread decides: the same bits in all)
      const double keep = mix.keep, push = mix.push;
      const double nF = sqrt(acc[1]), nV = sqrt(acc[2]);
      // pass 2: |dt v|^2 of the new velocities, which are not stored yet
      double d2[1] = {0.0};
      for (int64_t i = a0 + tid; i < a1; i += FIRE_THREADS) {
        double g[3], v[3];
        load_atom<HOLD>(forces, forces_extra, vel, hold, i, F, g, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double dr = dt * new_velocity(v[k], g[k], keep, push, nF, nV, dt);
          d2[0] += dr * dr;
        }
      }
      block_sum<1>(d2, sm);
      double vc_new[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        vc_new[k] = new_velocity(vc[k], G[k], keep, push, nF, nV, dt);
        const double dq = dt * vc_new[k];
        d2[0] += dq * dq;
      }
      const double nD = sqrt(d2[0]);
      const bool clip = nD > p.fire.max_step;
      const double scale = clip ? p.fire.max_step / nD : 1.0;
      // the new deformation gradient and cell, and the guard on them
      double Fn[9], Cn[9];
      bool ok = finite_d(nD);   // (a non-finite step length fails)
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        double dq = dt * vc_new[k];
        if (clip) dq = dq * scale;
        Fn[k] = F[k] + dq / n_at;
        ok = ok && finite_d(Fn[k]);
      }
      mul_abt(C0, Fn, Cn);   // C0 F_new^T
      ok = ok && det3(Fn) > 0.0 && min_height3(Cn) >= p.min_height;   // (a NaN fails both comparisons)
      if (!ok) {
        if (tid == 0) {
          fmax_sys[s] = fm;
          active_s[s] = 0;
          status_s[s] = 2;
        }
      } else {
        still_active = true;
        if (tid == 0) {
          fmax_sys[s] = fm;
          dt_s[s] = dt;
          alpha_s[s] = alpha;
          n_pos_s[s] = n_pos;
          n_steps_s[s] += 1;
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            cell[9 * (int64_t)s + k] = Cn[k];
            vel_cell[9 * (int64_t)s + k] = vc_new[k];
          }
        }
        // pass 3: the velocities (the values of pass 2 again) and the move  r = (r F^-T + dq) F_new^T
        for (int64_t i = a0 + tid; i < a1; i += FIRE_THREADS) {
          double g[3], r[3], q[3], v0[3];
          load_atom<HOLD>(forces, forces_extra, vel, hold, i, F, g, v0);
#pragma unroll
          for (int k = 0; k < 3; ++k) r[k] = pos[3 * i + k];
          row_mul_t(r, Finv, q);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double v = new_velocity(v0[k], g[k], keep, push, nF, nV, dt);
            vel[3 * i + k] = v;
            double dq = dt * v;
            if (clip) dq = dq * scale;
            q[k] += dq;
          }
          row_mul_t(q, Fn, r);
#pragma unroll
          for (int k = 0; k < 3; ++k) pos[3 * i + k] = r[k];
        }
      }
    }
  }
  if (tid == 0) count_active(&g_fire_cell_arrivals, still_active, n_sys, n_active);
}

template <bool HOLD>
int fire_cell_step_launch(const char *name, double *pos, double *vel, double *cell, double *vel_cell, const double *cell0,
                          const float *forces, const double *forces_extra, const double *virial, const double *virial_extra,
                          int64_t n_atoms, const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos,
                          int32_t *active, int32_t *n_steps, int32_t *status, double *fmax_sys, int32_t *n_active, double fmax,
                          double dt_start, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha,
                          double max_step, double scalar_pressure, int32_t cell_mask_bits, int32_t hydrostatic_strain,
                          int32_t constant_volume, double min_height, const int32_t *hold, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), std::string(name) + ": bad shape");
  SNET_REQUIRE(pos && vel && cell && vel_cell && cell0 && forces && virial && seg_ptr && dt && alpha && n_pos && active && n_steps &&
                   status && fmax_sys && n_active && (hold || !HOLD),
               std::string(name) + ": null argument");
  FireCellParams p;
  p.fire = FireParams{fmax, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step, n_min};
  SNET_REQUIRE(fire_params_ok(fmax, dt_start, p.fire), std::string(name) + ": FIRE parameters out of range");
  SNET_REQUIRE(scalar_pressure - scalar_pressure == 0.0 && cell_mask_bits >= 0 && cell_mask_bits < 64 && min_height >= 0 &&
                   !(hydrostatic_strain && constant_volume),
               std::string(name) + ": cell parameters out of range");
  p.pressure = scalar_pressure, p.min_height = min_height, p.mask_bits = cell_mask_bits;
  p.hydrostatic = hydrostatic_strain != 0, p.constant_volume = constant_volume != 0;
  fire_cell_step_kernel<HOLD><<<(unsigned)n_sys, FIRE_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, vel, cell, vel_cell, cell0, forces, forces_extra, hold, virial, virial_extra, n_atoms, seg_ptr, n_sys, dt, alpha, n_pos,
      active, n_steps, status, fmax_sys, n_active, p);
  SNET_CHECK_LAUNCH(name);
  return 0;
}

}  // namespace

extern "C" int snet_fire_cell_step(double *pos, double *vel, double *cell, double *vel_cell, const double *cell0, const float *forces,
                                   const double *forces_extra, const double *virial, const double *virial_extra, int64_t n_atoms,
                                   const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                                   int32_t *n_steps, int32_t *status, double *fmax_sys, int32_t *n_active, double fmax,
                                   double dt_start, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha_start,
                                   double f_alpha, double max_step, double scalar_pressure, int32_t cell_mask_bits,
                                   int32_t hydrostatic_strain, int32_t constant_volume, double min_height, void *stream) {
  return fire_cell_step_launch<false>("snet_fire_cell_step", pos, vel, cell, vel_cell, cell0, forces, forces_extra, virial, virial_extra,
                                      n_atoms, seg_ptr, n_sys, dt, alpha, n_pos, active, n_steps, status, fmax_sys, n_active, fmax,
                                      dt_start, dt_max, n_min, f_inc, f_dec, alpha_start, f_alpha, max_step, scalar_pressure,
                                      cell_mask_bits, hydrostatic_strain, constant_volume, min_height, nullptr, stream);
}

extern "C" int snet_fire_cell_step_fixed(double *pos, double *vel, double *cell, double *vel_cell, const double *cell0,
                                         const float *forces, const double *forces_extra, const double *virial,
                                         const double *virial_extra, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_sys, double *dt,
                                         double *alpha, int32_t *n_pos, int32_t *active, int32_t *n_steps, int32_t *status,
                                         double *fmax_sys, int32_t *n_active, double fmax, double dt_start, double dt_max, int32_t n_min,
                                         double f_inc, double f_dec, double alpha_start, double f_alpha, double max_step,
                                         double scalar_pressure, int32_t cell_mask_bits, int32_t hydrostatic_strain,
                                         int32_t constant_volume, double min_height, const int32_t *hold, void *stream) {
  return fire_cell_step_launch<true>("snet_fire_cell_step_fixed", pos, vel, cell, vel_cell, cell0, forces, forces_extra, virial,
                                     virial_extra, n_atoms, seg_ptr, n_sys, dt, alpha, n_pos, active, n_steps, status, fmax_sys, n_active,
                                     fmax, dt_start, dt_max, n_min, f_inc, f_dec, alpha_start, f_alpha, max_step, scalar_pressure,
                                     cell_mask_bits, hydrostatic_strain, constant_volume, min_height, hold, stream);
}
