// Batched nudged-elastic-band forces: one workgroup per moving image, every per-image sum in a fixed order.
//
// Improved tangent: Henkelman, Jonsson, J. Chem. Phys. 113, 9978 (2000); climbing image: Henkelman, Uberuaga, Jonsson, J. Chem.
// Phys. 113, 9901 (2000).  The rule is written out in include/snet_hip.h (snet_neb_forces).  The kernel turns the true forces and
// the image energies of the interior images of many bands into NEB forces where they are; snet_fire_step (snet_relax.hip), called
// with one segment per band, then moves all images of a band as the one system ASE's FIRE(NEB(images)) optimizes.
#include "snet_system.h"

namespace {

constexpr int NEB_THREADS = 256;
constexpr int NEB_WAVES = NEB_THREADS / 64;

using namespace snet;   // the shared device helpers (snet_system.h)

struct NebCell {
  double c[9], inv[9];
  bool px, py, pz;
};

// minimum-image form of d: s = d inv(cell), s_k -= rint(s_k) on the periodic axes, d = s cell (row vectors); without a periodic
// axis d keeps its bits
__device__ __forceinline__ void mic(const NebCell &q, double (&d)[3]) {
  if (!(q.px || q.py || q.pz)) return;
  double s[3];
  row_mul(d, q.inv, s);
  if (q.px) s[0] -= rint(s[0]);
  if (q.py) s[1] -= rint(s[1]);
  if (q.pz) s[2] -= rint(s[2]);
  row_mul(s, q.c, d);
}

__global__ __launch_bounds__(NEB_THREADS) void neb_forces_kernel(
    const double *__restrict__ pos, const float *__restrict__ forces, const double *__restrict__ forces_extra,
    const double *__restrict__ energy, const double *__restrict__ energy_extra, int64_t n, const int32_t *__restrict__ seg_ptr,
    int n_img, const int32_t *__restrict__ img_ptr, int n_bands, const double *__restrict__ pos_end,
    const int32_t *__restrict__ end_ptr, int64_t n_end, const double *__restrict__ e_end, const double *__restrict__ cells,
    const double *__restrict__ inv_cells, const int32_t *__restrict__ pbc, const int32_t *__restrict__ fixed,
    const double *__restrict__ k_spring, int climb, int32_t *__restrict__ active, int32_t *__restrict__ status,
    double *__restrict__ f_neb, int32_t *__restrict__ imax) {
  __shared__ double sm[NEB_WAVES][4];
  const int j = blockIdx.x;   // the moving image
  const int tid = threadIdx.x;
  // the band of image j: the last b with img_ptr[b] <= j (uniform over the workgroup; img_ptr is non-decreasing)
  int lo = 0, hi = n_bands - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (img_ptr[mid] <= j) lo = mid; else hi = mid - 1;
  }
  const int b = lo;
  const int j0 = img_ptr[b], j1 = img_ptr[b + 1];
  const Segment seg = segment(seg_ptr, j, n);
  const int64_t a0 = seg.a0, a1 = seg.a1, na = a1 - a0;
  if (j < j0 || j >= j1 || j1 > n_img) return;   // an image no band owns: nothing of it is read or written
  const bool first = j == j0, last = j == j1 - 1;
  // the neighbours' rows: another image of the band, or an endpoint (rows e0 .. e0 + na: initial, e0 + na .. e0 + 2 na: final)
  const int64_t e0 = end_ptr[b];
  const double *prev = nullptr, *next = nullptr;
  bool layout_ok = e0 >= 0 && e0 + 2 * na <= n_end && (int64_t)end_ptr[b + 1] - e0 == 2 * na;
  if (!first) {
    const Segment sp = segment(seg_ptr, j - 1, n);
    layout_ok = layout_ok && sp.a1 - sp.a0 == na;
    prev = pos + 3 * sp.a0;
  } else {
    prev = pos_end + 3 * e0;
  }
  if (!last) {
    const Segment sn = segment(seg_ptr, j + 1, n);
    layout_ok = layout_ok && sn.a1 - sn.a0 == na;
    next = pos + 3 * sn.a0;
  } else {
    next = pos_end + 3 * (e0 + na);
  }
  bool write_zero = active[b] != 1;   // (uniform over the workgroup)
  if (!write_zero && !layout_ok) {    // images of unequal size, or endpoint rows that are not there: refused before any neighbour is read
    if (tid == 0) status[b] = 3, active[b] = 0;
    write_zero = true;
  }
  double Ei = 0.0, Em = 0.0, Ep = 0.0;
  int top = 0;
  if (!write_zero) {
    auto e_of = [&](int q) { return energy[q] + (energy_extra ? energy_extra[q] : 0.0); };
    Ei = e_of(j);
    Em = first ? e_end[2 * b] : e_of(j - 1);
    Ep = last ? e_end[2 * b + 1] : e_of(j + 1);
    // the interior image of highest energy, lowest index on ties
    double best = e_of(j0);
    for (int q = j0 + 1; q < j1; ++q) {
      const double e = e_of(q);
      if (e > best) best = e, top = q - j0;
    }
    if (!(finite_d(Ei) && finite_d(Em) && finite_d(Ep))) {
      if (tid == 0) status[b] = 2, active[b] = 0;
      write_zero = true;
    }
  }
  if (write_zero) {
    for (int64_t i = 3 * a0 + tid; i < 3 * a1; i += NEB_THREADS) f_neb[i] = 0.0;
    return;
  }
  if (first && tid == 0) imax[b] = top;
  NebCell q;
#pragma unroll
  for (int c = 0; c < 9; ++c) q.c[c] = cells[9 * b + c], q.inv[c] = inv_cells[9 * b + c];
  q.px = pbc[3 * b] != 0, q.py = pbc[3 * b + 1] != 0, q.pz = pbc[3 * b + 2] != 0;
  // weights of t+ and t- in the tangent, from the energies alone
  double wp, wm;
  if (Ep > Ei && Ei > Em) {
    wp = 1.0, wm = 0.0;
  } else if (Ep < Ei && Ei < Em) {
    wp = 0.0, wm = 1.0;
  } else {
    const double dp = fabs(Ep - Ei), dm = fabs(Em - Ei);
    const double dmax = fmax(dp, dm), dmin = fmin(dp, dm);
    if (Ep > Em) wp = dmax, wm = dmin; else wp = dmin, wm = dmax;
  }
  // pass 1: |t+|^2, |t-|^2, |tau|^2, F.tau
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = tid; i < na; i += NEB_THREADS) {
    double F[3], tp[3], tm[3];
    load_force(forces, forces_extra, a0 + i, F);
    if (fixed && fixed[a0 + i] != 0) F[0] = F[1] = F[2] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double r = pos[3 * (a0 + i) + c];
      tp[c] = next[3 * i + c] - r;
      tm[c] = r - prev[3 * i + c];
    }
    mic(q, tp);
    mic(q, tm);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double t = wp * tp[c] + wm * tm[c];
      acc[0] += tp[c] * tp[c];
      acc[1] += tm[c] * tm[c];
      acc[2] += t * t;
      acc[3] += F[c] * t;
    }
  }
  block_sum<4>(acc, sm);
  if (!(finite_d(acc[0]) && finite_d(acc[1]) && finite_d(acc[2]) && finite_d(acc[3]))) {   // (the same bits in every thread)
    if (tid == 0) status[b] = 2, active[b] = 0;
    for (int64_t i = 3 * a0 + tid; i < 3 * a1; i += NEB_THREADS) f_neb[i] = 0.0;
    return;
  }
  const double nt = sqrt(acc[2]);
  const double inv_nt = nt > 0.0 ? 1.0 / nt : 0.0;   // a zero norm leaves tau = 0
  const double f_tau = acc[3] * inv_nt;              // F . tau, tau normalised
  const bool climbing = climb != 0 && j - j0 == top;
  // coefficient of tau in F_neb
  const double along = climbing ? -2.0 * f_tau : -f_tau + k_spring[b] * (sqrt(acc[0]) - sqrt(acc[1]));
  // pass 2: the NEB forces (every thread recomputes the tangent rows it summed)
  for (int64_t i = tid; i < na; i += NEB_THREADS) {
    double F[3], tp[3], tm[3];
    const bool fix = fixed && fixed[a0 + i] != 0;
    load_force(forces, forces_extra, a0 + i, F);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double r = pos[3 * (a0 + i) + c];
      tp[c] = next[3 * i + c] - r;
      tm[c] = r - prev[3 * i + c];
    }
    mic(q, tp);
    mic(q, tm);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double tau = (wp * tp[c] + wm * tm[c]) * inv_nt;
      f_neb[3 * (a0 + i) + c] = fix ? 0.0 : F[c] + along * tau;
    }
  }
}

}  // namespace

extern "C" int snet_neb_forces(const double *pos, const float *forces, const double *forces_extra, const double *energy,
                               const double *energy_extra, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_img,
                               const int32_t *img_ptr, int32_t n_bands, const double *pos_end, const int32_t *end_ptr,
                               int64_t n_end, const double *e_end, const double *cells, const double *inv_cells, const int32_t *pbc,
                               const int32_t *fixed, const double *k, int32_t climb, int32_t *active, int32_t *status, double *f_neb,
                               int32_t *imax, void *stream) {
  SNET_REQUIRE(n_bands >= 1 && n_img >= n_bands && n_atoms >= 0 && n_atoms < (1ll << 31) && n_end >= 0 && n_end < (1ll << 31),
               "snet_neb_forces: bad shape");
  SNET_REQUIRE(pos && forces && energy && seg_ptr && img_ptr && pos_end && end_ptr && e_end && cells && inv_cells && pbc && k &&
                   active && status && f_neb && imax,
               "snet_neb_forces: null argument");
  neb_forces_kernel<<<(unsigned)n_img, NEB_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, forces, forces_extra, energy, energy_extra, n_atoms, seg_ptr, n_img, img_ptr, n_bands, pos_end, end_ptr, n_end, e_end,
      cells, inv_cells, pbc, fixed, k, climb, active, status, f_neb, imax);
  SNET_CHECK_LAUNCH("snet_neb_forces");
  return 0;
}
