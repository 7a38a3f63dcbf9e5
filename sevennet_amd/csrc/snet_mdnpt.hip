// Batched isotropic NPT MD step: the BAOAB step of snet_mdstep.hip with the stochastic cell rescaling of Bernetti and Bussi,
// J. Chem. Phys. 153, 114107 (2020), isotropic form, between the kicks and the drift.  One workgroup per system, fp64, every
// per-system sum in the fixed order of block_sum, no atomics and no value that crosses workgroups.  The rule is written
// out in include/snet_hip.h (snet_mdb_npt_step) and restated in fp64 numpy in tests/md_npt_ref.py.
//
// The barostat is first order in the cell: one normal deviate per system and step (snet_philox.h, stream tag 2, atom word 0),
// no barostat momentum.  Nothing of a system is written before its next cell has passed the guard.
#include "snet_system.h"

namespace {

using namespace snet;   // the shared device helpers (snet_system.h) and the noise stream (snet_philox.h)

constexpr int NPT_THREADS = 256;
constexpr int NPT_WAVES = NPT_THREADS / 64;

struct NptParams {
  double dt, c1, c2, max_log_volume_step, min_height;
  uint64_t seed;
  int phase;
};

__global__ __launch_bounds__(NPT_THREADS) void mdb_npt_step_kernel(
    double *__restrict__ pos, double *__restrict__ vel, double *__restrict__ cell, const float *__restrict__ forces,
    const double *__restrict__ forces_extra, const double *__restrict__ virial, const double *__restrict__ virial_extra,
    const double *__restrict__ mass, int64_t n, const int32_t *__restrict__ seg_ptr, const int32_t *__restrict__ sys_id,
    const double *__restrict__ kT, const double *__restrict__ p0, const double *__restrict__ beta_over_tau,
    int32_t *__restrict__ step_index, double *__restrict__ e_kin, double *__restrict__ volume, double *__restrict__ pressure,
    int32_t *__restrict__ active, int32_t *__restrict__ status, NptParams p) {
  __shared__ double sm[NPT_WAVES][4];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const Segment seg = segment(seg_ptr, s, n);
  // a system that has left the run (active == 0) is measured and not moved: phase 0.  (uniform over the workgroup; every
  // thread reads the system's state before the first barrier, thread 0 writes it after the last)
  const int phase = active[s] == 1 ? p.phase : 0;
  const bool finish = (phase & 1) != 0, start = (phase & 2) != 0;
  const double dt = p.dt, half_kick = 0.5 * dt * MD_ACC, kt = kT[s];
  const uint32_t sys = (uint32_t)sys_id[s], step = (uint32_t)step_index[s];
  double C[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) C[k] = cell[9 * (int64_t)s + k];
  double trw = 0.0;
  {
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = virial[6 * (int64_t)s + k] + (virial_extra ? virial_extra[6 * (int64_t)s + k] : 0.0);
    trw = (w[0] + w[1]) + w[2];
  }
  // pass 1: the kinetic energy of v_k (after the finishing kick, which is not stored yet)
  double mv2[1] = {0.0};
  for (int64_t i = seg.a0 + tid; i < seg.a1; i += NPT_THREADS) {
    const double m = mass[i];
    double v[3] = {vel[3 * i + 0], vel[3 * i + 1], vel[3 * i + 2]};
    double F[3] = {0.0, 0.0, 0.0};
    if (phase != 0) load_force(forces, forces_extra, i, F);
    if (finish) half_kick3(v, F, half_kick, m);
    mv2[0] += m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  }
  block_sum<1>(mv2, sm);
  const double ek = 0.5 * mv2[0] / MD_ACC;
  const double vol = fabs(det3(C));
  const double press = (2.0 * ek + trw) / (3.0 * vol);
  // the barostat step and the guard on the next cell
  double mu = 1.0;
  double Cn[9];
  bool ok = true;
  if (start) {
    const double bt = beta_over_tau[s];
    double de = -bt * (p0[s] - press) * dt;
    const double amp = sqrt(2.0 * kt * bt * dt / vol);
    if (amp != 0.0) {   // (kT == 0 or no coupling: no random number is generated)
      double xi[3];
      normals3(p.seed, 0u, sys, step, STREAM_BAROSTAT, xi);
      de += amp * xi[0];
    }
    mu = exp(de / 3.0);
    ok = finite_d(de) && fabs(de) <= p.max_log_volume_step;   // (a NaN fails both)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      Cn[k] = mul_rounded(mu, C[k]);
      ok = ok && finite_d(Cn[k]);
    }
    ok = ok && min_height3(Cn) >= p.min_height;
  }
  if (tid == 0) {
    e_kin[s] = ek;
    volume[s] = vol;
    pressure[s] = press;
  }
  if (!ok) {   // refused: pos, vel, cell and step_index keep their bits, now and in every later launch
    if (tid == 0) {
      active[s] = 0;
      status[s] = 2;
    }
    return;
  }
  if (phase == 0) return;
  // pass 2: the atom step of snet_mdb_step (the kicks again: the same arithmetic on the same bits) with the rescaling by mu
  const BaoabStep bs{finish, start, dt, p.c1, p.c2, half_kick, kt * MD_ACC, mu, p.seed, sys, step};
  for (int64_t i = seg.a0 + tid; i < seg.a1; i += NPT_THREADS)
    baoab_atom(bs, pos, vel, forces, forces_extra, mass, i, (uint32_t)(i - seg.a0));
  if (start && tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) cell[9 * (int64_t)s + k] = Cn[k];
    step_index[s] = (int32_t)(step + 1u);
  }
}

}  // namespace

extern "C" int snet_mdb_npt_step(double *pos, double *vel, double *cell, const float *forces, const double *forces_extra,
                                 const double *virial, const double *virial_extra, const double *mass, int64_t n_atoms,
                                 const int32_t *seg_ptr, const int32_t *sys_id, int32_t n_sys, const double *kT, const double *p0,
                                 const double *beta_over_tau, int32_t *step_index, double *e_kin, double *volume, double *pressure,
                                 int32_t *active, int32_t *status, double dt, double c1, double c2, uint64_t seed, int32_t phase,
                                 double max_log_volume_step, double min_height, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31), "snet_mdb_npt_step: bad shape");
  SNET_REQUIRE(pos && vel && cell && forces && virial && mass && seg_ptr && sys_id && kT && p0 && beta_over_tau && step_index &&
                   e_kin && volume && pressure && active && status,
               "snet_mdb_npt_step: null argument");
  SNET_REQUIRE(dt > 0 && c1 >= 0 && c1 <= 1 && c2 >= 0 && c2 <= 1 && phase >= 0 && phase <= 3,
               "snet_mdb_npt_step: parameters out of range (dt > 0, 0 <= c1 <= 1, 0 <= c2 <= 1, phase in 0..3)");
  SNET_REQUIRE(max_log_volume_step > 0 && min_height >= 0,
               "snet_mdb_npt_step: barostat parameters out of range (max_log_volume_step > 0, min_height >= 0)");
  NptParams p;
  p.dt = dt, p.c1 = c1, p.c2 = c2, p.max_log_volume_step = max_log_volume_step, p.min_height = min_height;
  p.seed = seed, p.phase = phase;
  mdb_npt_step_kernel<<<(unsigned)n_sys, NPT_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, vel, cell, forces, forces_extra, virial, virial_extra, mass, n_atoms, seg_ptr, sys_id, kT, p0, beta_over_tau, step_index,
      e_kin, volume, pressure, active, status, p);
  SNET_CHECK_LAUNCH("snet_mdb_npt_step");
  return 0;
}
