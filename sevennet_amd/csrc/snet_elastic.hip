// Batched second-order elastic tensors: the homogeneously strained copies of many crystals are written on the device, and the
// engine's virials and forces on them are reduced to the raw stress-strain matrix S = d sigma / d epsilon, the internal-strain
// tensor L = d F / d epsilon at fixed scaled coordinates, the clamped-ion tensor C = (S + S^T) / 2 and the asymmetry max |S - S^T|.
// The rule is written out in include/snet_hip.h (snet_el_strain, snet_el_rows, snet_el_finish) and restated in fp64 numpy in
// tests/elastic_ref.py.
//
// One 256-thread workgroup per unit of work (a copy, a column of S, a system), fp64, no atomics and no sum over threads: every
// element of the copies, of S, L and C is computed by one thread in a written-out order, and the one reduction, the maximum of the
// asymmetry, does not depend on its order.  No product is contracted with the sum that follows it, so the results equal the numpy
// restatement of the same expressions bit for bit.
#include "snet_system.h"

namespace {

using namespace snet;   // the shared device helpers (snet_system.h)

constexpr int EL_THREADS = 256;

__global__ __launch_bounds__(EL_THREADS) void el_strain_kernel(
    const double *__restrict__ pos0, int64_t n0, const int32_t *__restrict__ seg_ptr0, int n_sys, const int32_t *__restrict__ desc,
    const int32_t *__restrict__ copy_ptr, double delta, double *__restrict__ pos_out, int64_t n_out, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
  const int c = blockIdx.x;   // the copy
  const int tid = threadIdx.x;
  const int b = desc[3 * c], j = desc[3 * c + 1], q = desc[3 * c + 2];
  const CopySlot slot = copy_slot(b, copy_ptr, c, n_out, seg_ptr0, n_sys, n0);
  const Range base = slot.base, out = slot.out;
  if (!(slot.ok && j >= 0 && j < 6 && q >= -2 && q <= 2)) {
    if (tid == 0) status[c] = 1;   // refused before a row is read or written (uniform over the workgroup)
    return;
  }
  const int64_t na = base.a1 - base.a0;
  const double s = copy_step(q, delta);   // rounded here, as snet_vib_displace rounds its shift
  const double h = s * 0.5;             // (exact)
  // the axes of the pattern: j < 3 stretches axis j; yz, xz, xy shear the pair (a, bb)
  const int a = j < 3 ? j : (j == 3 ? 1 : 0), bb = j < 3 ? j : (j == 5 ? 1 : 2);
  for (int64_t i = tid; i < na; i += EL_THREADS) {
    const double *__restrict__ x = pos0 + 3 * (base.a0 + i);
    double y[3] = {x[0], x[1], x[2]};
    if (q != 0) {   // (q = 0 is the unstrained copy, bit for bit)
      if (j < 3) {
        y[a] = x[a] + s * x[a];
      } else {
        y[a] = x[a] + h * x[bb];
        y[bb] = x[bb] + h * x[a];
      }
    }
    double *__restrict__ o = pos_out + 3 * (out.a0 + i);
    o[0] = y[0], o[1] = y[1], o[2] = y[2];
  }
}

__global__ __launch_bounds__(EL_THREADS) void el_rows_kernel(
    const double *__restrict__ virial, const double *__restrict__ virial_extra, const double *__restrict__ volume,
    const float *__restrict__ forces, const double *__restrict__ forces_extra, int64_t n, const int32_t *__restrict__ seg_ptr,
    int n_copies, const int32_t *__restrict__ group, int nfree, double delta, const int32_t *__restrict__ atom_ptr, int64_t n_base,
    int n_sys, double *__restrict__ S, double *__restrict__ L, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const RowGroup rg = row_group(group, blockIdx.x, nfree, n_copies, seg_ptr, n, n_sys);   // the (system, column) group
  if (!rg.has_sys) return;   // no system to report to: nothing is read or written
  const int j0 = rg.j0, b = rg.b, j = rg.r;
  const Range at = checked_range(atom_ptr, b, n_base);
  const int64_t na = at.a1 - at.a0;
  if (!(rg.ok && j >= 0 && j < 6 && at.ok && na > 0 && rg.na == na)) {   // (the copies are of the system's size)
    if (tid == 0) status[b] = 3;   // (uniform over the workgroup)
    return;
  }
  // the copies come in the order q = -1, +1 (nfree 2) or q = -2, -1, +1, +2 (nfree 4); S and L are plain derivatives, which
  // fd_stencil gives for the copies in the opposite order: copy w goes to place nfree - 1 - w
  int64_t a0[4] = {0, 0, 0, 0};
#pragma unroll
  for (int w = 0; w < 4; ++w) a0[w] = nfree == 2 ? rg.a0[w ^ 1] : rg.a0[3 - w];   // (entries 2, 3 are not read with nfree 2)
  const double h2 = 2.0 * delta, h12 = 12.0 * delta;
  bool bad = false;
  if (tid < 6) {   // column j of S: sigma_i = -((virial + virial_extra)[perm i] / V') of each copy, then the stencil
    const int p = tid < 3 ? tid : (tid == 3 ? 4 : (tid == 4 ? 5 : 3));   // ASE Voigt (xx,yy,zz,yz,xz,xy) from the engine's (xx,yy,zz,xy,yz,zx)
    double sg[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w >= nfree) break;
      const int64_t c = (int64_t)j0 + w;
      double t = virial[6 * c + p];
      if (virial_extra) t = t + virial_extra[6 * c + p];
      const double V = volume[c];
      if (!finite_d(t) || !finite_d(V) || !(V > 0.0)) bad = true;
      const double sigma = -(t / V);
      if (nfree == 2) sg[w ^ 1] = sigma; else sg[3 - w] = sigma;
    }
    S[36 * (int64_t)b + 6 * tid + j] = fd_stencil(sg, nfree, h2, h12);
  }
  double *__restrict__ row = L + 18 * at.a0 + (int64_t)j * 3 * na;
  for (int64_t c = tid; c < 3 * na; c += EL_THREADS) {
    double F[4];
    if (!load_copy_forces(forces, forces_extra, a0, c, nfree, F)) bad = true;
    row[c] = fd_stencil(F, nfree, h2, h12);
  }
  if (bad) status[b] = 2;   // (every writer of a system's status writes a non-zero value: any of them marks it failed)
}

__global__ __launch_bounds__(EL_THREADS) void el_finish_kernel(const double *__restrict__ S, const int32_t *__restrict__ status,
                                                               double *__restrict__ C, double *__restrict__ asym) {
#pragma clang fp contract(off)
  __shared__ double sm[4];
  const int b = blockIdx.x;   // the system
  const int tid = threadIdx.x;
  const double nan_d = __builtin_nan("");
  const bool failed = status[b] != 0;
  double worst = 0.0;
  if (tid < 36) {
    const int r = tid / 6, c = tid % 6;
    const double x = S[36 * (int64_t)b + 6 * r + c], y = S[36 * (int64_t)b + 6 * c + r];
    C[36 * (int64_t)b + tid] = failed ? nan_d : (x + y) * 0.5;   // (x + y and y + x have the same bits: C[r,c] and C[c,r] do too)
    if (!failed) worst = fabs(x - y);
  }
  worst = block_max(worst, sm);
  if (tid == 0) asym[b] = failed ? nan_d : worst;
}

}  // namespace

extern "C" int snet_el_strain(const double *pos0, int64_t n0, const int32_t *seg_ptr0, int32_t n_sys, const int32_t *desc,
                              const int32_t *copy_ptr, int32_t n_copies, double delta, double *pos_out, int64_t n_out,
                              int32_t *status, void *stream) {
  SNET_REQUIRE(!pos0 || pos0 != pos_out, "snet_el_strain: aliased argument");
  return launch_copy_writer("snet_el_strain", el_strain_kernel, pos0, n0, seg_ptr0, n_sys, desc, copy_ptr, n_copies, delta, pos_out,
                            n_out, status, stream);
}

extern "C" int snet_el_rows(const double *virial, const double *virial_extra, const double *volume, const float *forces,
                            const double *forces_extra, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_copies,
                            const int32_t *group, int32_t n_groups, int32_t nfree, double delta, const int32_t *atom_ptr,
                            int64_t n_base, int32_t n_sys, double *S, double *L, int32_t *status, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_copies >= 1 && n_groups >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31) && n_base >= 1 &&
                   n_base < (1ll << 31),
               "snet_el_rows: bad shape");
  SNET_REQUIRE(nfree == 2 || nfree == 4, "snet_el_rows: nfree must be 2 or 4");
  SNET_REQUIRE(virial && volume && forces && seg_ptr && group && atom_ptr && S && L && status, "snet_el_rows: null argument");
  el_rows_kernel<<<(unsigned)n_groups, EL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      virial, virial_extra, volume, forces, forces_extra, n_atoms, seg_ptr, n_copies, group, nfree, delta, atom_ptr, n_base, n_sys, S, L,
      status);
  SNET_CHECK_LAUNCH("snet_el_rows");
  return 0;
}

extern "C" int snet_el_finish(const double *S, int32_t n_sys, const int32_t *status, double *C, double *asymmetry, void *stream) {
  SNET_REQUIRE(n_sys >= 1, "snet_el_finish: bad shape");
  SNET_REQUIRE(S && status && C && asymmetry && S != C, "snet_el_finish: null or aliased argument");
  el_finish_kernel<<<(unsigned)n_sys, EL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(S, status, C, asymmetry);
  SNET_CHECK_LAUNCH("snet_el_finish");
  return 0;
}
