// Batched FIRE relaxation step (fixed cell, unit masses): one workgroup per system, every per-system sum in a fixed order.
//
// FIRE: Bitzek, Koskinen, Gaehler, Moseler, Gumbsch, Phys. Rev. Lett. 97, 170201 (2006), in the form of ASE's optimizer (the
// step is dt * v after the velocity update, clipped to max_step over the whole system).  Positions, velocities and the
// per-system state (dt, alpha, n_pos, active, n_steps) stay on the device between steps; the host reads back n_active only.
#include "snet_common.h"

namespace {

constexpr int FIRE_THREADS = 256;
constexpr int FIRE_WAVES = FIRE_THREADS / 64;

// (ticket << 32) | systems still active, of the launch in flight; the last workgroup to arrive writes n_active and puts it
// back to zero, so every launch starts from zero.  One word per device: launches on one device follow each other in stream
// order (as the scratch of the two-stage reductions, they must not overlap on two streams).
__device__ unsigned long long g_fire_arrivals = 0ull;

struct FireParams {
  double fmax, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step;
  int n_min;
};

// max that keeps a NaN (a NaN force must not pass for a converged system)
__device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double wave_max_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v = max_nan(v, __shfl_xor(v, o, 64));
  return v;
}

using snet::block_sum;    // per-system sums in a fixed order (snet_common.h)
using snet::load_force;   // fp32 forces + optional fp64 forces_extra, in fp64

__global__ __launch_bounds__(FIRE_THREADS) void fire_step_kernel(double *__restrict__ pos, double *__restrict__ vel,
                                                                 const float *__restrict__ forces, const double *__restrict__ forces_extra,
                                                                 int64_t n, const int32_t *__restrict__ seg_ptr, int n_sys,
                                                                 double *__restrict__ dt_s, double *__restrict__ alpha_s,
                                                                 int32_t *__restrict__ n_pos_s, int32_t *__restrict__ active_s,
                                                                 int32_t *__restrict__ n_steps_s, double *__restrict__ fmax_sys,
                                                                 int32_t *__restrict__ n_active, FireParams p) {
  __shared__ double sm[FIRE_WAVES][4];
  __shared__ double sc[4];   // decided by thread 0: mixing (keep, push), dt; sc[3] < 0: frozen
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  bool still_active = false;
  if (active_s[s] == 1) {   // (uniform over the workgroup)
    const snet::Segment seg = snet::segment(seg_ptr, s, n);
    const int64_t a0 = seg.a0, a1 = seg.a1;
    // pass 1: max |F_i|^2, F.v, |F|^2, |v|^2
    double f2max = 0.0;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = a0 + tid; i < a1; i += FIRE_THREADS) {
      double F[3];
      load_force(forces, forces_extra, i, F);
      const double vx = vel[3 * i + 0], vy = vel[3 * i + 1], vz = vel[3 * i + 2];
      const double f2 = F[0] * F[0] + F[1] * F[1] + F[2] * F[2];
      f2max = max_nan(f2, f2max);
      acc[0] += F[0] * vx + F[1] * vy + F[2] * vz;
      acc[1] += f2;
      acc[2] += vx * vx + vy * vy + vz * vz;
    }
    {
      const double t = wave_max_d(f2max);
      if ((tid & 63) == 0) sm[tid >> 6][3] = t;
    }
    block_sum<3>(acc, sm);   // (its first barrier also publishes the four maxima; its second lets thread 0 go on alone)
    if (tid == 0) {
      // sm[.][3] is not rewritten before the barrier below
      const double fm = sqrt(max_nan(max_nan(sm[0][3], sm[1][3]), max_nan(sm[2][3], sm[3][3])));
      fmax_sys[s] = fm;
      if (fm < p.fmax) {
        active_s[s] = 0;
        sc[3] = -1.0;
      } else {
        double dt = dt_s[s], alpha = alpha_s[s];
        int n_pos = n_pos_s[s];
        double keep, push;
        if (acc[0] > 0.0) {
          keep = 1.0 - alpha;
          push = alpha;   // v <- keep v + ((push F) / |F|) |v|
          if (n_pos > p.n_min) {
            dt = fmin(dt * p.f_inc, p.dt_max);
            alpha_s[s] = alpha * p.f_alpha;
          }
          n_pos += 1;
        } else {
          keep = 0.0;
          push = 0.0;
          alpha_s[s] = p.alpha_start;
          dt = dt * p.f_dec;
          n_pos = 0;
        }
        dt_s[s] = dt;
        n_pos_s[s] = n_pos;
        n_steps_s[s] += 1;
        sc[0] = keep;
        sc[1] = push;
        sc[2] = dt;
        sc[3] = 1.0;
      }
    }
    __syncthreads();
    if (sc[3] > 0.0) {
      still_active = true;
      const double keep = sc[0], push = sc[1], dt = sc[2];
      const double nF = sqrt(acc[1]), nV = sqrt(acc[2]);
      // pass 2: the new velocities, and |dt v|^2
      double d2[1] = {0.0};
      for (int64_t i = a0 + tid; i < a1; i += FIRE_THREADS) {
        double F[3];
        load_force(forces, forces_extra, i, F);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double v = 0.0;
          if (push > 0.0 || keep > 0.0) v = keep * vel[3 * i + k] + push * F[k] / nF * nV;
          v = v + dt * F[k];
          vel[3 * i + k] = v;
          const double dr = dt * v;
          d2[0] += dr * dr;
        }
      }
      block_sum<1>(d2, sm);
      const double nD = sqrt(d2[0]);
      const bool clip = nD > p.max_step;
      const double scale = clip ? p.max_step / nD : 1.0;
      // pass 3: the move (every thread re-reads the velocities it wrote itself)
      for (int64_t i = a0 + tid; i < a1; i += FIRE_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double dr = dt * vel[3 * i + k];
          if (clip) dr = dr * scale;
          pos[3 * i + k] += dr;
        }
      }
    }
  }
  if (tid == 0) {   // count the active systems: one integer atomic per workgroup, the last arrival publishes the sum
    const unsigned long long old = atomicAdd(&g_fire_arrivals, (1ull << 32) | (still_active ? 1ull : 0ull));
    if ((unsigned)(old >> 32) == (unsigned)(n_sys - 1)) {
      *n_active = (int32_t)((unsigned)(old & 0xffffffffull) + (still_active ? 1u : 0u));
      atomicExch(&g_fire_arrivals, 0ull);
    }
  }
}

}  // namespace

extern "C" int snet_fire_step(double *pos, double *vel, const float *forces, const double *forces_extra, int64_t n_atoms,
                              const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                              int32_t *n_steps, double *fmax_sys, int32_t *n_active, double fmax, double dt_start, double dt_max,
                              int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha, double max_step,
                              void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), "snet_fire_step: bad shape");
  SNET_REQUIRE(pos && vel && forces && seg_ptr && dt && alpha && n_pos && active && n_steps && fmax_sys && n_active,
               "snet_fire_step: null argument");
  SNET_REQUIRE(fmax >= 0 && dt_start > 0 && dt_max >= dt_start && n_min >= 0 && f_inc >= 1 && f_dec > 0 && f_dec < 1 &&
                   alpha_start > 0 && alpha_start <= 1 && f_alpha > 0 && f_alpha <= 1 && max_step > 0,
               "snet_fire_step: FIRE parameters out of range");
  FireParams p;
  p.fmax = fmax, p.dt_max = dt_max, p.f_inc = f_inc, p.f_dec = f_dec, p.alpha_start = alpha_start, p.f_alpha = f_alpha;
  p.max_step = max_step, p.n_min = n_min;
  fire_step_kernel<<<(unsigned)n_sys, FIRE_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, vel, forces, forces_extra, n_atoms, seg_ptr, n_sys, dt, alpha, n_pos, active, n_steps, fmax_sys, n_active, p);
  SNET_CHECK_LAUNCH("snet_fire_step");
  return 0;
}
