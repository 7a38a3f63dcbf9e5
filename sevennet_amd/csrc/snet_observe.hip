// MD observables accumulated on the device: the radial distribution function as integer pair counts (snet_obs_rdf) and the
// mean-square displacement and velocity autocorrelation against a ring of origin frames (snet_obs_correlate).  fp64, one small
// launch per sample for all systems; the rules are written out in include/snet_hip.h and restated in fp64 numpy in
// tests/observe_ref.py.  The RDF adds integers only (LDS histogram, one integer atomicAdd per non-zero bin), the correlation sums
// go through snet::block_sum in its fixed order and no two workgroups of a launch write one slot: neither depends on the order
// workgroups run in or on the batch a system is in.
#include "snet_system.h"

namespace {

using namespace snet;   // the shared device helpers (snet_system.h)

constexpr int OBS_THREADS = 256;
constexpr int OBS_WAVES = OBS_THREADS / 64;
constexpr int OBS_MAX_KINDS = 8;      // kinds per system
constexpr int OBS_MAX_HIST = 8192;    // kinds^2 bins uint32 words of LDS
constexpr int OBS_MAX_REACH = 4;      // lattice shifts per axis: -reach .. reach
constexpr int OBS_DESC = 8;           // int32 words per system of sys_desc

// sys_desc[b] = (kinds, first word of the system's counts, pbc bits, reach_x, reach_y, reach_z, 0, 0); tile[t] = (system, first
// row within the system, rows).  A descriptor that does not fit (see the checks below) counts nothing.
__global__ __launch_bounds__(OBS_THREADS) void obs_rdf_kernel(const double *__restrict__ pos, int64_t n, const int32_t *__restrict__ seg_ptr,
                                                              int n_sys, const int32_t *__restrict__ kind,
                                                              const double *__restrict__ cell, const int32_t *__restrict__ sys_desc,
                                                              const int32_t *__restrict__ tile, double dr, int bins,
                                                              int kinds_max, int reach_max,
                                                              unsigned long long *__restrict__ counts, int64_t n_counts) {
#pragma clang fp contract(off)
  __shared__ uint32_t hist[OBS_MAX_HIST];
  const int tid = threadIdx.x;
  const int b = tile[3 * blockIdx.x];
  if (b < 0 || b >= n_sys) return;   // (uniform over the workgroup, as every return below)
  const int32_t *sd = sys_desc + OBS_DESC * b;
  const int S = sd[0];
  const int64_t off = sd[1];
  const int pbc = sd[2] & 7;
  const int reach[3] = {(pbc & 1) ? sd[3] : 0, (pbc & 2) ? sd[4] : 0, (pbc & 4) ? sd[5] : 0};
  if (S < 1 || S > kinds_max) return;   // (kinds_max^2 bins fits `hist`: the entry point has checked)
  const int n_hist = S * S * bins;
  if (off < 0 || off + n_hist > n_counts) return;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (reach[k] < 0 || reach[k] > reach_max) return;
  const Segment seg = segment(seg_ptr, b, n);
  const int64_t ns = seg.a1 - seg.a0;
  int64_t r0 = tile[3 * blockIdx.x + 1], nr = tile[3 * blockIdx.x + 2];
  if (r0 < 0 || nr < 0 || r0 + nr > ns) return;
  for (int q = tid; q < n_hist; q += OBS_THREADS) hist[q] = 0u;
  __syncthreads();
  const double q_end = (double)bins;
  double c[9], inv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) c[k] = cell[9 * b + k];
  if (pbc) inv3(c, det3(c), inv);   // (a cell with a periodic axis is invertible: the host has checked)
  for (int64_t p = tid; p < nr * ns; p += OBS_THREADS) {
    const int64_t i = seg.a0 + r0 + p / ns, j = seg.a0 + p % ns;
    const int ka = kind[i], kb = kind[j];
    if (ka < 0 || ka >= S || kb < 0 || kb >= S) continue;
    double d[3] = {pos[3 * j] - pos[3 * i], pos[3 * j + 1] - pos[3 * i + 1], pos[3 * j + 2] - pos[3 * i + 2]};
    if (pbc) {   // to fractional coordinates, the nearest image on periodic axes, and back
      double f[3];
      row_mul(d, inv, f);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if ((pbc >> k) & 1) f[k] = f[k] - rint(f[k]);
      row_mul(f, c, d);
    }
    uint32_t *h = hist + (ka * S + kb) * bins;
    for (int n0 = -reach[0]; n0 <= reach[0]; ++n0)
      for (int n1 = -reach[1]; n1 <= reach[1]; ++n1)
        for (int n2 = -reach[2]; n2 <= reach[2]; ++n2) {
          if (i == j && n0 == 0 && n1 == 0 && n2 == 0) continue;
          const double s[3] = {(double)n0, (double)n1, (double)n2};
          double t[3];
          row_mul(s, c, t);
          const double x = d[0] + t[0], y = d[1] + t[1], z = d[2] + t[2];
          const double r = sqrt((x * x + y * y) + z * z);
          const double q = r / dr;
          if (q < q_end) atomicAdd(&h[(int)q], 1u);   // (false for a NaN)
        }
  }
  __syncthreads();
  for (int q = tid; q < n_hist; q += OBS_THREADS)
    if (hist[q]) atomicAdd(&counts[off + q], (unsigned long long)hist[q]);
}

// the mass-weighted centre of x over the rows of `seg` (block_sum's order); every thread returns the same bits
__device__ __forceinline__ void mass_centre(const double *__restrict__ x, const double *__restrict__ mass, const Segment &seg,
                                            double (*sm)[4], double (&com)[3]) {
#pragma clang fp contract(off)
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = seg.a0 + threadIdx.x; i < seg.a1; i += OBS_THREADS) {
    const double m = mass[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = acc[k] + m * x[3 * i + k];
    acc[3] = acc[3] + m;
  }
  block_sum<4>(acc, sm);
#pragma unroll
  for (int k = 0; k < 3; ++k) com[k] = acc[k] / acc[3];
}

// workgroup (system b, ring slot): the origin in that slot against the current frame, per kind.  Origin number q (sample
// q origin_every) sits in slot q % ring; the caller has stored the origin of this sample, if it is one, before the launch.
__global__ __launch_bounds__(OBS_THREADS) void obs_correlate_kernel(const double *__restrict__ pos, const double *__restrict__ vel,
                                                                    const double *__restrict__ ring_pos,
                                                                    const double *__restrict__ ring_vel,
                                                                    const double *__restrict__ mass, const int32_t *__restrict__ hold,
                                                                    int64_t n, const int32_t *__restrict__ seg_ptr,
                                                                    const int32_t *__restrict__ kind,
                                                                    const int32_t *__restrict__ kind_ptr, int64_t n_kinds, int sample,
                                                                    int origin_every, int ring, int lags, int remove_com,
                                                                    double *__restrict__ msd_sum, double *__restrict__ vacf_sum) {
#pragma clang fp contract(off)
  __shared__ double sm[OBS_WAVES][4];
  const int b = blockIdx.x, slot = blockIdx.y;
  const int tid = threadIdx.x;
  const int q_last = sample / origin_every;
  if (q_last < slot) return;   // (the slot has not been written yet)
  const int q = q_last - (q_last - slot) % ring;
  const int64_t lag = (int64_t)sample - (int64_t)q * origin_every;
  if (lag >= lags) return;
  const int64_t k0 = kind_ptr[b], k1 = kind_ptr[b + 1];
  if (k0 < 0 || k1 < k0 || k1 - k0 > OBS_MAX_KINDS || k1 > n_kinds) return;
  const Segment seg = segment(seg_ptr, b, n);
  const int64_t ns = seg.a1 - seg.a0;
  const double *xo = ring_pos + 3 * n * slot, *vo = ring_vel + 3 * n * slot;
  double cx[3] = {0.0, 0.0, 0.0}, cv[3] = {0.0, 0.0, 0.0}, cxo[3] = {0.0, 0.0, 0.0}, cvo[3] = {0.0, 0.0, 0.0};
  bool rest = false;   // one free atom in its own centre-of-mass frame: nothing is left of its motion
  if (remove_com) {    // (uniform over the grid)
    double held[1] = {0.0};
    if (hold)
      for (int64_t i = seg.a0 + tid; i < seg.a1; i += OBS_THREADS) held[0] += (double)__popc((unsigned)held_bits(hold, i));
    block_sum<1>(held, sm);   // (small integers: exact)
    if (held[0] == 0.0) {     // a system with held components is anchored: no correction (snet_mdb_init_velocities_fixed)
      rest = ns == 1;
      if (!rest && ns > 0) {
        mass_centre(pos, mass, seg, sm, cx);
        mass_centre(vel, mass, seg, sm, cv);
        mass_centre(xo, mass, seg, sm, cxo);
        mass_centre(vo, mass, seg, sm, cvo);
      }
    }
  }
  for (int64_t kk = k0; kk < k1; ++kk) {
    double acc[2] = {0.0, 0.0};
    if (!rest) {
      for (int64_t i = seg.a0 + tid; i < seg.a1; i += OBS_THREADS) {
        if (kind[i] != (int)(kk - k0)) continue;
        double d2 = 0.0, vv = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double d = (pos[3 * i + k] - cx[k]) - (xo[3 * i + k] - cxo[k]);
          d2 = d2 + d * d;
          vv = vv + (vel[3 * i + k] - cv[k]) * (vo[3 * i + k] - cvo[k]);
        }
        acc[0] = acc[0] + d2;
        acc[1] = acc[1] + vv;
      }
    }
    block_sum<2>(acc, sm);
    if (tid == 0) {   // the only workgroup of this launch at (kind, lag); earlier launches are ordered by the stream
      msd_sum[kk * lags + lag] = msd_sum[kk * lags + lag] + acc[0];
      vacf_sum[kk * lags + lag] = vacf_sum[kk * lags + lag] + acc[1];
    }
  }
}

}  // namespace

extern "C" int snet_obs_rdf(const double *pos, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_sys, const int32_t *kind,
                            const double *cell, const int32_t *sys_desc, const int32_t *tile, int32_t n_tiles, double dr, int32_t bins,
                            int32_t kinds_max, int32_t reach_max, uint64_t *counts, int64_t n_counts, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_tiles >= 0 && n_atoms >= 0 && n_atoms < (1ll << 31) && n_counts >= 0, "snet_obs_rdf: bad shape");
  SNET_REQUIRE(pos && seg_ptr && kind && cell && sys_desc && tile && counts, "snet_obs_rdf: null argument");
  SNET_REQUIRE(dr > 0 && dr <= 1.7976931348623157e308 && bins >= 1 && kinds_max >= 1 && kinds_max <= OBS_MAX_KINDS &&
                   (int64_t)kinds_max * kinds_max * bins <= OBS_MAX_HIST && reach_max >= 0 && reach_max <= OBS_MAX_REACH,
               "snet_obs_rdf: parameters out of range (dr > 0 and finite, bins >= 1, 1 <= kinds_max <= 8, kinds_max^2 bins <= 8192, "
               "0 <= reach_max <= 4)");
  if (n_tiles == 0) return 0;
  obs_rdf_kernel<<<(unsigned)n_tiles, OBS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, n_atoms, seg_ptr, n_sys, kind, cell, sys_desc, tile, dr, bins, kinds_max, reach_max, reinterpret_cast<unsigned long long *>(counts), n_counts);
  SNET_CHECK_LAUNCH("snet_obs_rdf");
  return 0;
}

extern "C" int snet_obs_correlate(const double *pos, const double *vel, const double *ring_pos, const double *ring_vel,
                                  const double *mass, const int32_t *hold, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_sys,
                                  const int32_t *kind, const int32_t *kind_ptr, int64_t n_kinds, int32_t sample, int32_t origin_every,
                                  int32_t ring, int32_t lags, int32_t remove_com, double *msd_sum, double *vacf_sum, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31) && n_kinds >= 0, "snet_obs_correlate: bad shape");
  SNET_REQUIRE(pos && vel && ring_pos && ring_vel && mass && seg_ptr && kind && kind_ptr && msd_sum && vacf_sum,
               "snet_obs_correlate: null argument");
  SNET_REQUIRE(sample >= 0 && origin_every >= 1 && lags >= 1 && ring >= 1 && ring <= 65535 &&
                   (int64_t)ring * origin_every >= lags && (int64_t)(ring - 1) * origin_every < lags,
               "snet_obs_correlate: parameters out of range (sample >= 0, origin_every >= 1, lags >= 1, ring = ceil(lags / "
               "origin_every) <= 65535)");
  obs_correlate_kernel<<<dim3((unsigned)n_sys, (unsigned)ring), OBS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, vel, ring_pos, ring_vel, mass, hold, n_atoms, seg_ptr, kind, kind_ptr, n_kinds, sample, origin_every, ring, lags, remove_com,
      msd_sum, vacf_sum);
  SNET_CHECK_LAUNCH("snet_obs_correlate");
  return 0;
}
