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

__global__ __launch_bounds__(MD_THREADS) void mdb_step_kernel(double *__restrict__ pos, double *__restrict__ vel,
                                                               const float *__restrict__ forces, const double *__restrict__ forces_extra,
                                                               const double *__restrict__ mass, int64_t n,
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
  for (int64_t i = seg.a0 + tid; i < seg.a1; i += MD_THREADS)
    mv2[0] += baoab_atom(p, pos, vel, forces, forces_extra, mass, i, (uint32_t)(i - seg.a0));
  block_sum<1>(mv2, sm);   // (its barriers: every thread has read step_index[s] before thread 0 writes it)
  if (tid == 0) {
    e_kin[s] = 0.5 * mv2[0] / MD_ACC;
    if (p.start) step_index[s] = (int32_t)(step + 1u);
  }
}

__global__ __launch_bounds__(MD_THREADS) void mdb_init_velocities_kernel(double *__restrict__ vel, const double *__restrict__ mass, int64_t n,
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
  if (remove_com && ns == 1) {   // nothing is left of one atom's velocity once the centre of mass rests
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
      const double v = sigma * xi[k];
      vel[3 * i + k] = v;
      acc[k] += m * v;
    }
    acc[3] += m;
  }
  if (!remove_com) return;   // (uniform over the grid)
  snet::block_sum<4>(acc, sm);
  const double com[3] = {acc[0] / acc[3], acc[1] / acc[3], acc[2] / acc[3]};
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
  // pass 3: the kinetic energy becomes (3 n - 3) kT / 2 exactly
  const double e_now = 0.5 * mv2[0] / MD_ACC, e_want = 0.5 * (double)(3 * ns - 3) * kt;
  const double scale = e_now > 0.0 ? sqrt(e_want / e_now) : 0.0;
  for (int64_t i = seg.a0 + tid; i < seg.a1; i += MD_THREADS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) vel[3 * i + k] *= scale;
  }
}

}  // namespace

extern "C" int snet_mdb_step(double *pos, double *vel, const float *forces, const double *forces_extra, const double *mass,
                             int64_t n_atoms, const int32_t *seg_ptr, const int32_t *sys_id, int32_t n_sys, const double *kT,
                             int32_t *step_index, double *e_kin, double dt, double c1, double c2, uint64_t seed, int32_t phase,
                             void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), "snet_mdb_step: bad shape");
  SNET_REQUIRE(pos && vel && forces && mass && seg_ptr && sys_id && kT && step_index && e_kin, "snet_mdb_step: null argument");
  SNET_REQUIRE(dt > 0 && c1 >= 0 && c1 <= 1 && c2 >= 0 && c2 <= 1 && phase >= 0 && phase <= 3,
               "snet_mdb_step: parameters out of range (dt > 0, 0 <= c1 <= 1, 0 <= c2 <= 1, phase in 0..3)");
  mdb_step_kernel<<<(unsigned)n_sys, MD_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, vel, forces, forces_extra, mass, n_atoms, seg_ptr, sys_id, kT, step_index, e_kin, dt, c1, c2, seed, phase);
  SNET_CHECK_LAUNCH("snet_mdb_step");
  return 0;
}

extern "C" int snet_mdb_init_velocities(double *vel, const double *mass, int64_t n_atoms, const int32_t *seg_ptr,
                                        const int32_t *sys_id, int32_t n_sys, const double *kT, uint64_t seed, int32_t remove_com,
                                        void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), "snet_mdb_init_velocities: bad shape");
  SNET_REQUIRE(vel && mass && seg_ptr && sys_id && kT, "snet_mdb_init_velocities: null argument");
  mdb_init_velocities_kernel<<<(unsigned)n_sys, MD_THREADS, 0, static_cast<hipStream_t>(stream)>>>(vel, mass, n_atoms, seg_ptr, sys_id,
                                                                                                  kT, seed, remove_com);
  SNET_CHECK_LAUNCH("snet_mdb_init_velocities");
  return 0;
}
