// Batched FIRE relaxation step (fixed cell, unit masses): one workgroup per system, every per-system sum in a fixed order.
//
// FIRE: Bitzek, Koskinen, Gaehler, Moseler, Gumbsch, Phys. Rev. Lett. 97, 170201 (2006), in the form of ASE's optimizer (the
// step is dt * v after the velocity update, clipped to max_step over the whole system).  Positions, velocities and the
// per-system state (dt, alpha, n_pos, active, n_steps) stay on the device between steps; the host reads back n_active only.
// snet_fire_step_fixed is the same kernel text under a mask of held components (template <bool HOLD>).
#include "snet_system.h"

namespace {

constexpr int FIRE_THREADS = 256;
constexpr int FIRE_WAVES = FIRE_THREADS / 64;

// (ticket << 32) | systems still active, of the launch in flight; the last workgroup to arrive writes n_active and puts it
// back to zero, so every launch starts from zero.  One word per device: launches on one device follow each other in stream
// order (as the scratch of the two-stage reductions, they must not overlap on two streams).
__device__ unsigned long long g_fire_arrivals = 0ull;

using namespace snet;   // the shared device helpers (snet_system.h)

// HOLD (snet_fire_step_fixed): the components in the mask `hold` enter every pass with force and velocity 0, by selection; their
// velocities are stored as 0 and their positions are not written.  HOLD = false (snet_fire_step) never reads `hold`.
template <bool HOLD>
__global__ __launch_bounds__(FIRE_THREADS) void fire_step_kernel(double *__restrict__ pos, double *__restrict__ vel,
                                                                 const float *__restrict__ forces, const double *__restrict__ forces_extra,
                                                                 const int32_t *__restrict__ hold, int64_t n,
                                                                 const int32_t *__restrict__ seg_ptr, int n_sys,
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
    const Segment seg = segment(seg_ptr, s, n);
    const int64_t a0 = seg.a0, a1 = seg.a1;
    // pass 1: max |F_i|^2, F.v, |F|^2, |v|^2
    double f2max = 0.0;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = a0 + tid; i < a1; i += FIRE_THREADS) {
      double F[3], v[3] = {vel[3 * i + 0], vel[3 * i + 1], vel[3 * i + 2]};
      if constexpr (HOLD) {
        const int h = held_bits(hold, i);
        load_force_free(forces, forces_extra, i, h, F);
        zero_held(h, v);
      } else {
        load_force(forces, forces_extra, i, F);
      }
      const double vx = v[0], vy = v[1], vz = v[2];
      const double f2 = F[0] * F[0] + F[1] * F[1] + F[2] * F[2];
      f2max = max_nan(f2, f2max);
      acc[0] += F[0] * vx + F[1] * vy + F[2] * vz;
      acc[1] += f2;
      acc[2] += vx * vx + vy * vy + vz * vz;
    }
    block_max_nan_put(f2max, sm);
    block_sum<3>(acc, sm);   // (its first barrier also publishes the four maxima; its second lets thread 0 go on alone)
    if (tid == 0) {
      const double fm = sqrt(block_max_nan_get(sm));   // (sm[.][3] is not rewritten before the barrier below)
      fmax_sys[s] = fm;
      if (fm < p.fmax) {
        active_s[s] = 0;
        sc[3] = -1.0;
      } else {
        double dt = dt_s[s], alpha = alpha_s[s];
        int n_pos = n_pos_s[s];
        const FireMix mix = fire_decide(acc[0], p, dt, alpha, n_pos);
        dt_s[s] = dt;
        alpha_s[s] = alpha;
        n_pos_s[s] = n_pos;
        n_steps_s[s] += 1;
        sc[0] = mix.keep;
        sc[1] = mix.push;
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
        int h = 0;
        if constexpr (HOLD) {
          h = held_bits(hold, i);
          load_force_free(forces, forces_extra, i, h, F);
        } else {
          load_force(forces, forces_extra, i, F);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double v = new_velocity(vel[3 * i + k], F[k], keep, push, nF, nV, dt);
          if constexpr (HOLD) v = is_held(h, k) ? 0.0 : v;   // (whatever the array held on entry)
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
        int h = 0;
        if constexpr (HOLD) h = held_bits(hold, i);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double dr = dt * vel[3 * i + k];
          if (clip) dr = dr * scale;
          if (!HOLD || !is_held(h, k)) pos[3 * i + k] += dr;
        }
      }
    }
  }
  if (tid == 0) count_active(&g_fire_arrivals, still_active, n_sys, n_active);
}

template <bool HOLD>
int fire_step_launch(const char *name, double *pos, double *vel, const float *forces, const double *forces_extra, int64_t n_atoms,
                     const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active, int32_t *n_steps,
                     double *fmax_sys, int32_t *n_active, double fmax, double dt_start, double dt_max, int32_t n_min, double f_inc,
                     double f_dec, double alpha_start, double f_alpha, double max_step, const int32_t *hold, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), std::string(name) + ": bad shape");
  SNET_REQUIRE(pos && vel && forces && seg_ptr && dt && alpha && n_pos && active && n_steps && fmax_sys && n_active && (hold || !HOLD),
               std::string(name) + ": null argument");
  const FireParams p{fmax, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step, n_min};
  SNET_REQUIRE(fire_params_ok(fmax, dt_start, p), std::string(name) + ": FIRE parameters out of range");
  fire_step_kernel<HOLD><<<(unsigned)n_sys, FIRE_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, vel, forces, forces_extra, hold, n_atoms, seg_ptr, n_sys, dt, alpha, n_pos, active, n_steps, fmax_sys, n_active, p);
  SNET_CHECK_LAUNCH(name);
  return 0;
}

}  // namespace

extern "C" int snet_fire_step(double *pos, double *vel, const float *forces, const double *forces_extra, int64_t n_atoms,
                              const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                              int32_t *n_steps, double *fmax_sys, int32_t *n_active, double fmax, double dt_start, double dt_max,
                              int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha, double max_step,
                              void *stream) {
  return fire_step_launch<false>("snet_fire_step", pos, vel, forces, forces_extra, n_atoms, seg_ptr, n_sys, dt, alpha, n_pos, active,
                                 n_steps, fmax_sys, n_active, fmax, dt_start, dt_max, n_min, f_inc, f_dec, alpha_start, f_alpha, max_step,
                                 nullptr, stream);
}

extern "C" int snet_fire_step_fixed(double *pos, double *vel, const float *forces, const double *forces_extra, int64_t n_atoms,
                                    const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                                    int32_t *n_steps, double *fmax_sys, int32_t *n_active, double fmax, double dt_start, double dt_max,
                                    int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha, double max_step,
                                    const int32_t *hold, void *stream) {
  return fire_step_launch<true>("snet_fire_step_fixed", pos, vel, forces, forces_extra, n_atoms, seg_ptr, n_sys, dt, alpha, n_pos,
                                active, n_steps, fmax_sys, n_active, fmax, dt_start, dt_max, n_min, f_inc, f_dec, alpha_start, f_alpha,
                                max_step, hold, stream);
}
