// Batched variable-cell FIRE relaxation step (unit masses): one workgroup per system, every per-system sum in a fixed order.
//
// The rule is that of ASE's UnitCellFilter under ASE's FIRE (written out in include/snet_hip.h, snet_fire_cell_step): the n atoms
// in the frame of the reference cell and the three rows of n F, F the deformation gradient, are one system of n + 3 rows for
// the FIRE step of snet_relax.hip.  Positions, cells, both velocity arrays and the per-system state stay on the device between
// steps; the host reads back n_active only.  Nothing of a system is written before its new cell has passed the guard.
#include "snet_common.h"

namespace {

constexpr int FIRE_THREADS = 256;
constexpr int FIRE_WAVES = FIRE_THREADS / 64;

// (ticket << 32) | systems still active, of the launch in flight (as g_fire_arrivals of snet_relax.hip, and apart from it)
__device__ unsigned long long g_fire_cell_arrivals = 0ull;

struct FireCellParams {
  double fmax, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step, pressure, min_height;
  int n_min, mask_bits, hydrostatic, constant_volume;
};

// max that keeps a NaN (a NaN force must not pass for a converged system)
__device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double wave_max_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v = max_nan(v, __shfl_xor(v, o, 64));
  return v;
}

using snet::block_sum;    // per-system sums in a fixed order (snet_common.h)
using snet::load_force;   // fp32 forces + optional fp64 forces_extra, in fp64

// 3x3 matrices, row-major (det3 and min_height3: snet_common.h)
using snet::det3;
using snet::min_height3;
__device__ __forceinline__ void inv3(const double *a, double det, double *inv) {
  const double id = 1.0 / det;
  inv[0] = (a[4] * a[8] - a[5] * a[7]) * id;
  inv[1] = (a[2] * a[7] - a[1] * a[8]) * id;
  inv[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  inv[3] = (a[5] * a[6] - a[3] * a[8]) * id;
  inv[4] = (a[0] * a[8] - a[2] * a[6]) * id;
  inv[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  inv[6] = (a[3] * a[7] - a[4] * a[6]) * id;
  inv[7] = (a[1] * a[6] - a[0] * a[7]) * id;
  inv[8] = (a[0] * a[4] - a[1] * a[3]) * id;
}
// out = a b^T
__device__ __forceinline__ void mul_abt(const double *a, const double *b, double *out) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}
// out = x m (row vector times matrix) and out = x m^T
__device__ __forceinline__ void row_mul(const double *x, const double *m, double *out) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = x[0] * m[j] + x[1] * m[3 + j] + x[2] * m[6 + j];
}
__device__ __forceinline__ void row_mul_t(const double *x, const double *m, double *out) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = x[0] * m[3 * j] + x[1] * m[3 * j + 1] + x[2] * m[3 * j + 2];
}
// FIRE's velocity update of one component: mixing (keep, push) as decided for the system, then v += dt g
__device__ __forceinline__ double new_velocity(double v_old, double g, double keep, double push, double nF, double nV, double dt) {
  double v = 0.0;
  if (push > 0.0 || keep > 0.0) v = keep * v_old + push * g / nF * nV;
  return v + dt * g;
}

__global__ __launch_bounds__(FIRE_THREADS) void fire_cell_step_kernel(
    double *__restrict__ pos, double *__restrict__ vel, double *__restrict__ cell, double *__restrict__ vel_cell,
    const double *__restrict__ cell0, const float *__restrict__ forces, const double *__restrict__ forces_extra,
    const double *__restrict__ virial, const double *__restrict__ virial_extra, int64_t n, const int32_t *__restrict__ seg_ptr,
    int n_sys, double *__restrict__ dt_s, double *__restrict__ alpha_s, int32_t *__restrict__ n_pos_s, int32_t *__restrict__ active_s,
    int32_t *__restrict__ n_steps_s, int32_t *__restrict__ status_s, double *__restrict__ fmax_sys, int32_t *__restrict__ n_active,
    FireCellParams p) {
  __shared__ double sm[FIRE_WAVES][4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  bool still_active = false;
  if (active_s[s] == 1) {   // (uniform over the workgroup; so is everything below that is not indexed by an atom)
    const snet::Segment seg = snet::segment(seg_ptr, s, n);
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
      double f[3], g[3];
      load_force(forces, forces_extra, i, f);
      row_mul(f, F, g);
      const double vx = vel[3 * i + 0], vy = vel[3 * i + 1], vz = vel[3 * i + 2];
      const double f2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
      f2max = max_nan(f2, f2max);
      acc[0] += g[0] * vx + g[1] * vy + g[2] * vz;
      acc[1] += f2;
      acc[2] += vx * vx + vy * vy + vz * vz;
    }
    {
      const double t = wave_max_d(f2max);
      if ((tid & 63) == 0) sm[tid >> 6][3] = t;
    }
    block_sum<3>(acc, sm);   // (its first barrier also publishes the four maxima; sm[.][3] is not rewritten in this launch)
    f2max = max_nan(max_nan(sm[0][3], sm[1][3]), max_nan(sm[2][3], sm[3][3]));
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
    if (fm < p.fmax) {
      if (tid == 0) {
        fmax_sys[s] = fm;
        active_s[s] = 0;
        status_s[s] = 1;
      }
    } else {
      double keep, push;
      if (acc[0] > 0.0) {
        keep = 1.0 - alpha;
        push = alpha;   // v <- keep v + ((push g) / |g|) |v|
        if (n_pos > p.n_min) {
          dt = fmin(dt * p.f_inc, p.dt_max);
          alpha = alpha * p.f_alpha;
        }
        n_pos += 1;
      } else {
        keep = 0.0;
        push = 0.0;
        alpha = p.alpha_start;
        dt = dt * p.f_dec;
        n_pos = 0;
      }
      const double nF = sqrt(acc[1]), nV = sqrt(acc[2]);
      // pass 2: |dt v|^2 of the new velocities, which are not stored yet
      double d2[1] = {0.0};
      for (int64_t i = a0 + tid; i < a1; i += FIRE_THREADS) {
        double f[3], g[3];
        load_force(forces, forces_extra, i, f);
        row_mul(f, F, g);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double dr = dt * new_velocity(vel[3 * i + k], g[k], keep, push, nF, nV, dt);
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
      const bool clip = nD > p.max_step;
      const double scale = clip ? p.max_step / nD : 1.0;
      // the new deformation gradient and cell, and the guard on them
      double Fn[9], Cn[9];
      bool ok = nD - nD == 0.0;   // (a non-finite step length fails)
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        double dq = dt * vc_new[k];
        if (clip) dq = dq * scale;
        Fn[k] = F[k] + dq / n_at;
        ok = ok && (Fn[k] - Fn[k] == 0.0);
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
          double f[3], g[3], r[3], q[3];
          load_force(forces, forces_extra, i, f);
          row_mul(f, F, g);
#pragma unroll
          for (int k = 0; k < 3; ++k) r[k] = pos[3 * i + k];
          row_mul_t(r, Finv, q);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double v = new_velocity(vel[3 * i + k], g[k], keep, push, nF, nV, dt);
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
  if (tid == 0) {   // count the active systems: one integer atomic per workgroup, the last arrival publishes the sum
    const unsigned long long old = atomicAdd(&g_fire_cell_arrivals, (1ull << 32) | (still_active ? 1ull : 0ull));
    if ((unsigned)(old >> 32) == (unsigned)(n_sys - 1)) {
      *n_active = (int32_t)((unsigned)(old & 0xffffffffull) + (still_active ? 1u : 0u));
      atomicExch(&g_fire_cell_arrivals, 0ull);
    }
  }
}

}  // namespace

extern "C" int snet_fire_cell_step(double *pos, double *vel, double *cell, double *vel_cell, const double *cell0, const float *forces,
                                   const double *forces_extra, const double *virial, const double *virial_extra, int64_t n_atoms,
                                   const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                                   int32_t *n_steps, int32_t *status, double *fmax_sys, int32_t *n_active, double fmax,
                                   double dt_start, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha_start,
                                   double f_alpha, double max_step, double scalar_pressure, int32_t cell_mask_bits,
                                   int32_t hydrostatic_strain, int32_t constant_volume, double min_height, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), "snet_fire_cell_step: bad shape");
  SNET_REQUIRE(pos && vel && cell && vel_cell && cell0 && forces && virial && seg_ptr && dt && alpha && n_pos && active && n_steps &&
                   status && fmax_sys && n_active,
               "snet_fire_cell_step: null argument");
  SNET_REQUIRE(fmax >= 0 && dt_start > 0 && dt_max >= dt_start && n_min >= 0 && f_inc >= 1 && f_dec > 0 && f_dec < 1 &&
                   alpha_start > 0 && alpha_start <= 1 && f_alpha > 0 && f_alpha <= 1 && max_step > 0,
               "snet_fire_cell_step: FIRE parameters out of range");
  SNET_REQUIRE(scalar_pressure - scalar_pressure == 0.0 && cell_mask_bits >= 0 && cell_mask_bits < 64 && min_height >= 0 &&
                   !(hydrostatic_strain && constant_volume),
               "snet_fire_cell_step: cell parameters out of range");
  FireCellParams p;
  p.fmax = fmax, p.dt_max = dt_max, p.f_inc = f_inc, p.f_dec = f_dec, p.alpha_start = alpha_start, p.f_alpha = f_alpha;
  p.max_step = max_step, p.n_min = n_min, p.pressure = scalar_pressure, p.min_height = min_height, p.mask_bits = cell_mask_bits;
  p.hydrostatic = hydrostatic_strain != 0, p.constant_volume = constant_volume != 0;
  fire_cell_step_kernel<<<(unsigned)n_sys, FIRE_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, vel, cell, vel_cell, cell0, forces, forces_extra, virial, virial_extra, n_atoms, seg_ptr, n_sys, dt, alpha, n_pos, active,
      n_steps, status, fmax_sys, n_active, p);
  SNET_CHECK_LAUNCH("snet_fire_cell_step");
  return 0;
}
