// Batched NVE / Langevin MD step (BAOAB folded around the force call) and Maxwell-Boltzmann velocity initialisation: one
// workgroup per system, fp64, every per-system sum in the fixed order of snet::block_sum, no atomics and no value that
// crosses workgroups.  The step rule and the noise stream are written out in include/snet_hip.h (snet_mdb_step) and restated
// in fp64 numpy in tests/md_ref.py.
//
// BAOAB: Leimkuhler, Matthews, Appl. Math. Res. Express 2013, 34 (2013).  Noise: Philox4x32-10 of Salmon, Moraes, Dror, Shaw,
// "Parallel random numbers: as easy as 1, 2, 3", SC11 (the Random123 constants), keyed by the seed and counted by (atom index
// within its system, the caller's system id, the system's step, stream tag): what an atom draws does not depend on the batch
// its system is in, on the slot it has there or on the launch grid.
#include "snet_system.h"

namespace {

using namespace snet;   // the shared device helpers (snet_system.h) and the noise stream (snet_philox.h)

constexpr int MD_THREADS = 256;
constexpr int MD_WAVES = MD_THREADS / 64;

// HOLD (snet_mdb_step_fixed): the atoms go through baoab_atom<true> under their mask words; HOLD = false never reads `hold`
template <bool HOLD>
__global__ __launch_bounds__(MD_THREADS) void mdb_step_kernel(double *__restrict__ pos, double *__restrict__ vel,
                                                               const float *__restrict__ forces, const double *__restrict__ forces_extra,
                                                               const int32_t *__restrict__ hold, const double *__restrict__ mass, int64_t n,
                                                               const int32_t *__restrict__ seg_ptr, const int32_t *__restrict__ sys_id,
                                                               const double *__restrict__ kT, int32_t *__restrict__ step_index,
                                                               double *__restrict__ e_kin, double dt, double c1, double c2,
                                                               uint64_t seed, int phase) {
  __shared__ double sm[MD_WAVES][4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const Segment seg = segment(seg_ptr, s, n);
  const uint32_t step = (uint32_t)step_index[s];   // (step_index is rewritten behind the barriers below)
  const BaoabStep p{(phase & 1) != 0, (phase & 2) != 0, dt, c1, c2, 0.5 * dt * MD_ACC, kT[s] * MD_ACC, 1.0, seed, (uint32_t)sys_id[s], step};
  double mv2[1] = {0.0};
  for (int64_t i = seg.a0 + tid; i < seg.a1; i += MD_THREADS) {
    if constexpr (HOLD)
      mv2[0] += baoab_atom<true>(p, pos, vel, forces, forces_extra, mass, i, (uint32_t)(i - seg.a0), held_bits(hold, i));
    else
      mv2[0] += baoab_atom(p, pos, vel, forces, forces_extra, mass, i, (uint32_t)(i - seg.a0));
  }
  block_sum<1>(mv2, sm);   // (its barriers: every thread has read step_index[s] before thread 0 writes it)
  if (tid == 0) {
    e_kin[s] = 0.5 * mv2[0] / MD_ACC;
    if (p.start) step_index[s] = (int32_t)(step + 1u);
  }
}

// HOLD (snet_mdb_init_velocities_fixed): held components are 0; a system with one or more of them is anchored: its centre of
// mass is left alone and the kinetic energy becomes (3 n - held components) kT / 2.  A system with none goes the way of HOLD = false.
template <bool HOLD>
__global__ __launch_bounds__(MD_THREADS) void mdb_init_velocities_kernel(double *__restrict__ vel, const double *__restrict__ mass,
                                                                          const int32_t *__restrict__ hold, int64_t n,
                                                                          const int32_t *__restrict__ seg_ptr,
                                                                          const int32_t *__restrict__ sys_id, const double *__restrict__ kT,
                                                                          uint64_t seed, int remove_com) {
  __shared__ double sm[MD_WAVES][4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const Segment seg = segment(seg_ptr, s, n);
  const int64_t ns = seg.a1 - seg.a0;
  const double kt = kT[s], kt_acc = kt * MD_ACC;
  const uint32_t sys = (uint32_t)sys_id[s];
  double n_held = 0.0;   // held components of the system (HOLD and remove_com only: nothing else asks)
  if constexpr (HOLD) {
    if (remove_com) {        // (uniform over the grid)
      double cnt[1] = {0.0};
      for (int64_t i = seg.a0 + tid; i < seg.a1; i += MD_THREADS) cnt[0] += (double)__popc((unsigned)held_bits(hold, i));
      snet::block_sum<1>(cnt, sm);   // (small integers: exact)
      n_held = cnt[0];
    }
  }
  const bool anchored = HOLD && n_held > 0.0;   // (uniform over the workgroup)
  if (remove_com && ns == 1 && !anchored) {   // nothing is left of one atom's velocity once the centre of mass rests
    if (tid < 3) vel[3 * seg.a0 + tid] = 0.0;
    return;
  }
  // pass 1: the draw, and sum m v, sum m
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = seg.a0 + tid; i < seg.a1; i += MD_THREADS) {
    const double m = mass[i];
    double xi[3];
    normals3(seed, (uint32_t)(i - seg.a0), sys, 0u, STREAM_INIT, xi);
    const double sigma = sqrt(kt_acc / m);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double v = sigma * xi[k];
      if constexpr (HOLD) v = is_held(held_bits(hold, i), k) ? 0.0 : v;
      vel[3 * i + k] = v;
      acc[k] += m * v;
    }
    acc[3] += m;
  }
  if (!remove_com) return;   // (uniform over the grid)
  snet::block_sum<4>(acc, sm);
  double com[3] = {acc[0] / acc[3], acc[1] / acc[3], acc[2] / acc[3]};
  if constexpr (HOLD) {
    if (anchored) com[0] = com[1] = com[2] = 0.0;   // the held atoms anchor the frame: no shift (v - 0.0 keeps v's bits)
  }
  // pass 2: the centre of mass comes to rest (every thread re-reads the velocities it wrote itself), and sum m |v|^2
  double mv2[1] = {0.0};
  for (int64_t i = seg.a0 + tid; i < seg.a1; i += MD_THREADS) {
    const double m = mass[i];
    double v2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = vel[3 * i + k] - com[k];
      vel[3 * i + k] = v;
      v2 += v * v;
    }
    mv2[0] += m * v2;
  }
  snet::block_sum<1>(mv2, sm);
  // pass 3: the kinetic energy becomes (3 n - 3) kT / 2 exactly; anchored: (3 n - held components) kT / 2, and with none free 0
  double dof = (double)(3 * ns - 3);
  if constexpr (HOLD) {
    if (anchored) dof = (double)(3 * ns) - n_held;
  }
  const double e_now = 0.5 * mv2[0] / MD_ACC, e_want = 0.5 * dof * kt;
  const double scale = e_now > 0.0 ? sqrt(e_want / e_now) : 0.0;
  for (int64_t i = seg.a0 + tid; i < seg.a1; i += MD_THREADS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) vel[3 * i + k] *= scale;
  }
}

template <bool HOLD>
int mdb_step_launch(const char *name, double *pos, double *vel, const float *forces, const double *forces_extra, const double *mass,
                    int64_t n_atoms, const int32_t *seg_ptr, const int32_t *sys_id, int32_t n_sys, const double *kT, int32_t *step_index,
                    double *e_kin, double dt, double c1, double c2, uint64_t seed, int32_t phase, const int32_t *hold, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), std::string(name) + ": bad shape");
  SNET_REQUIRE(pos && vel && forces && mass && seg_ptr && sys_id && kT && step_index && e_kin && (hold || !HOLD),
               std::string(name) + ": null argument");
  SNET_REQUIRE(dt > 0 && c1 >= 0 && c1 <= 1 && c2 >= 0 && c2 <= 1 && phase >= 0 && phase <= 3,
               std::string(name) + ": parameters out of range (dt > 0, 0 <= c1 <= 1, 0 <= c2 <= 1, phase in 0..3)");
  mdb_step_kernel<HOLD><<<(unsigned)n_sys, MD_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, vel, forces, forces_extra, hold, mass, n_atoms, seg_ptr, sys_id, kT, step_index, e_kin, dt, c1, c2, seed, phase);
  SNET_CHECK_LAUNCH(name);
  return 0;
}

template <bool HOLD>
int mdb_init_velocities_launch(const char *name, double *vel, const double *mass, int64_t n_atoms, const int32_t *seg_ptr,
                               const int32_t *sys_id, int32_t n_sys, const double *kT, uint64_t seed, int32_t remove_com,
                               const int32_t *hold, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), std::string(name) + ": bad shape");
  SNET_REQUIRE(vel && mass && seg_ptr && sys_id && kT && (hold || !HOLD), std::string(name) + ": null argument");
  mdb_init_velocities_kernel<HOLD><<<(unsigned)n_sys, MD_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      vel, mass, hold, n_atoms, seg_ptr, sys_id, kT, seed, remove_com);
  SNET_CHECK_LAUNCH(name);
  return 0;
}

}  // namespace

extern "C" int snet_mdb_step(double *pos, double *vel, const float *forces, const double *forces_extra, const double *mass,
                             int64_t n_atoms, const int32_t *seg_ptr, const int32_t *sys_id, int32_t n_sys, const double *kT,
                             int32_t *step_index, double *e_kin, double dt, double c1, double c2, uint64_t seed, int32_t phase,
                             void *stream) {
  return mdb_step_launch<false>("snet_mdb_step", pos, vel, forces, forces_extra, mass, n_atoms, seg_ptr, sys_id, n_sys, kT, step_index,
                                e_kin, dt, c1, c2, seed, phase, nullptr, stream);
}

extern "C" int snet_mdb_step_fixed(double *pos, double *vel, const float *forces, const double *forces_extra, const double *mass,
                                   int64_t n_atoms, const int32_t *seg_ptr, const int32_t *sys_id, int32_t n_sys, const double *kT,
                                   int32_t *step_index, double *e_kin, double dt, double c1, double c2, uint64_t seed, int32_t phase,
                                   const int32_t *hold, void *stream) {
  return mdb_step_launch<true>("snet_mdb_step_fixed", pos, vel, forces, forces_extra, mass, n_atoms, seg_ptr, sys_id, n_sys, kT,
                               step_index, e_kin, dt, c1, c2, seed, phase, hold, stream);
}

extern "C" int snet_mdb_init_velocities(double *vel, const double *mass, int64_t n_atoms, const int32_t *seg_ptr,
                                        const int32_t *sys_id, int32_t n_sys, const double *kT, uint64_t seed, int32_t remove_com,
                                        void *stream) {
  return mdb_init_velocities_launch<false>("snet_mdb_init_velocities", vel, mass, n_atoms, seg_ptr, sys_id, n_sys, kT, seed, remove_com,
                                           nullptr, stream);
}

extern "C" int snet_mdb_init_velocities_fixed(double *vel, const double *mass, int64_t n_atoms, const int32_t *seg_ptr,
                                              const int32_t *sys_id, int32_t n_sys, const double *kT, uint64_t seed, int32_t remove_com,
                                              const int32_t *hold, void *stream) {
  return mdb_init_velocities_launch<true>("snet_mdb_init_velocities_fixed", vel, mass, n_atoms, seg_ptr, sys_id, n_sys, kT, seed,
                                          remove_com, hold, stream);
}
