// Batched finite-difference Hessians: the displaced copies of many structures are written on the device, and the engine's forces
// on them are reduced to the rows of the central-difference matrix D, then to the Hessian H = (D + D^T) / 2, its mass-weighted
// form and the asymmetry max |D - D^T|.  The rule is written out in include/snet_hip.h (snet_vib_displace, snet_vib_rows,
// snet_vib_finish) and restated in fp64 numpy in tests/vib_ref.py.
//
// One 256-thread workgroup per unit of work (a copy, a row of D, a system), fp64, no atomics and no sum over threads: every
// element of D, H and Hm is computed by one thread from at most four forces in a written-out order, and the one reduction, the
// maximum of the asymmetry, does not depend on its order.  No product is contracted with the sum that follows it, so the
// results equal the numpy restatement of the same expressions bit for bit.
#include "snet_system.h"

namespace {

using namespace snet;   // the shared device helpers (snet_system.h)

constexpr int VIB_THREADS = 256;

__global__ __launch_bounds__(VIB_THREADS) void vib_displace_kernel(
    const double *__restrict__ pos0, int64_t n0, const int32_t *__restrict__ seg_ptr0, int n_sys, const int32_t *__restrict__ desc,
    const int32_t *__restrict__ copy_ptr, double delta, double *__restrict__ pos_out, int64_t n_out, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
  const int j = blockIdx.x;   // the copy
  const int tid = threadIdx.x;
  const int b = desc[4 * j], atom = desc[4 * j + 1], axis = desc[4 * j + 2], q = desc[4 * j + 3];
  const CopySlot slot = copy_slot(b, copy_ptr, j, n_out, seg_ptr0, n_sys, n0);
  const Range base = slot.base, out = slot.out;
  if (!(slot.ok && axis >= 0 && axis < 3 && q >= -2 && q <= 2 && atom >= 0 && atom < base.a1 - base.a0)) {
    if (tid == 0) status[j] = 1;   // refused before a row is read or written (uniform over the workgroup)
    return;
  }
  const int64_t na = base.a1 - base.a0;
  const double shift = copy_step(q, delta);   // rounded, then added: x + q delta as numpy forms it
  for (int64_t i = tid; i < 3 * na; i += VIB_THREADS) {
    const double x = pos0[3 * base.a0 + i];
    pos_out[3 * out.a0 + i] = (q != 0 && i == 3 * (int64_t)atom + axis) ? x + shift : x;
  }
}

__global__ __launch_bounds__(VIB_THREADS) void vib_rows_kernel(
    const float *__restrict__ forces, const double *__restrict__ forces_extra, int64_t n, const int32_t *__restrict__ seg_ptr,
    int n_copies, const int32_t *__restrict__ group, int nfree, double delta, const int32_t *__restrict__ sel,
    const int32_t *__restrict__ sel_ptr, int64_t n_sel, const int64_t *__restrict__ d_off, int n_sys, double *__restrict__ D,
    int64_t d_size, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const RowGroup rg = row_group(group, blockIdx.x, nfree, n_copies, seg_ptr, n, n_sys);
  if (!rg.has_sys) return;   // no system to report to: nothing is read or written
  const int b = rg.b, r = rg.r;
  const int64_t na = rg.na;
  const Range s = checked_range(sel_ptr, b, n_sel);
  const int64_t m3 = 3 * (s.a1 - s.a0), off = d_off[b];
  if (!(rg.ok && s.ok && m3 > 0 && r >= 0 && r < m3 && off >= 0 && off <= d_size && m3 * m3 <= d_size - off)) {
    if (tid == 0) status[b] = 3;   // (uniform over the workgroup)
    return;
  }
  double *__restrict__ row = D + off + (int64_t)r * m3;
  const double h2 = 2.0 * delta, h12 = 12.0 * delta;
  bool bad_atom = false, bad_force = false;
  for (int64_t c = tid; c < m3; c += VIB_THREADS) {
    const int64_t atom = sel[s.a0 + c / 3];
    if (atom < 0 || atom >= na) {
      bad_atom = true;
      continue;
    }
    double F[4];
    if (!load_copy_forces(forces, forces_extra, rg.a0, 3 * atom + c % 3, nfree, F)) bad_force = true;
    row[c] = fd_stencil(F, nfree, h2, h12);
  }
  if (bad_atom) status[b] = 3;          // (every writer of a system's status writes a non-zero value: any of them marks it failed)
  else if (bad_force) status[b] = 2;
}

__global__ __launch_bounds__(VIB_THREADS) void vib_finish_kernel(
    const double *__restrict__ D, const int64_t *__restrict__ d_off, const int32_t *__restrict__ sel_ptr, int64_t n_sel,
    const double *__restrict__ w, int64_t d_size, int32_t *__restrict__ status, double *__restrict__ H,
    double *__restrict__ Hm, double *__restrict__ asym) {
#pragma clang fp contract(off)
  __shared__ double sm[4];
  const int b = blockIdx.x;   // the system
  const int tid = threadIdx.x;
  const Range s = checked_range(sel_ptr, b, n_sel);
  const int64_t m3 = 3 * (s.a1 - s.a0), off = d_off[b];
  if (!(s.ok && m3 > 0 && off >= 0 && off <= d_size && m3 * m3 <= d_size - off)) {   // a block outside the buffers: nothing of it is touched
    if (tid == 0) status[b] = 3, asym[b] = __builtin_nan("");
    return;
  }
  const double nan_d = __builtin_nan("");
  const bool failed = status[b] != 0;
  double worst = 0.0;
  for (int64_t e = tid; e < m3 * m3; e += VIB_THREADS) {
    const int64_t r = e / m3, c = e % m3;
    if (failed) {
      H[off + e] = nan_d, Hm[off + e] = nan_d;
      continue;
    }
    const double x = D[off + r * m3 + c], y = D[off + c * m3 + r];
    const double h = (x + y) * 0.5;   // (x + y and y + x have the same bits: H[r,c] and H[c,r] do too)
    H[off + e] = h;
    Hm[off + e] = h * (w[s.a0 + r / 3] * w[s.a0 + c / 3]);
    worst = fmax(worst, fabs(x - y));
  }
  worst = block_max(worst, sm);
  if (tid == 0) asym[b] = failed ? nan_d : worst;
}

}  // namespace

extern "C" int snet_vib_displace(const double *pos0, int64_t n0, const int32_t *seg_ptr0, int32_t n_sys, const int32_t *desc,
                                 const int32_t *copy_ptr, int32_t n_copies, double delta, double *pos_out, int64_t n_out,
                                 int32_t *status, void *stream) {
  return launch_copy_writer("snet_vib_displace", vib_displace_kernel, pos0, n0, seg_ptr0, n_sys, desc, copy_ptr, n_copies, delta,
                            pos_out, n_out, status, stream);
}

extern "C" int snet_vib_rows(const float *forces, const double *forces_extra, int64_t n_atoms, const int32_t *seg_ptr,
                             int32_t n_copies, const int32_t *group, int32_t n_groups, int32_t nfree, double delta,
                             const int32_t *sel, const int32_t *sel_ptr, int64_t n_sel, const int64_t *d_off, int32_t n_sys, double *D,
                             int64_t d_size, int32_t *status, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_copies >= 1 && n_groups >= 1 && n_atoms >= 0 && n_atoms < (1ll << 31) && n_sel >= 1 && n_sel <= 1000000000ll && d_size >= 1,   // (9 n_sel^2 stays below 2^63)
               "snet_vib_rows: bad shape");
  SNET_REQUIRE(nfree == 2 || nfree == 4, "snet_vib_rows: nfree must be 2 or 4");
  SNET_REQUIRE(forces && seg_ptr && group && sel && sel_ptr && d_off && D && status, "snet_vib_rows: null argument");
  vib_rows_kernel<<<(unsigned)n_groups, VIB_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      forces, forces_extra, n_atoms, seg_ptr, n_copies, group, nfree, delta, sel, sel_ptr, n_sel, d_off, n_sys, D, d_size, status);
  SNET_CHECK_LAUNCH("snet_vib_rows");
  return 0;
}

extern "C" int snet_vib_finish(const double *D, const int64_t *d_off, const int32_t *sel_ptr, int64_t n_sel, const double *w,
                               int32_t n_sys, int64_t d_size, int32_t *status, double *H, double *Hm, double *asymmetry, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_sel >= 1 && n_sel <= 1000000000ll && d_size >= 1, "snet_vib_finish: bad shape");
  SNET_REQUIRE(D && d_off && sel_ptr && w && status && H && Hm && asymmetry, "snet_vib_finish: null argument");
  vib_finish_kernel<<<(unsigned)n_sys, VIB_THREADS, 0, static_cast<hipStream_t>(stream)>>>(D, d_off, sel_ptr, n_sel, w, d_size, status, H,
                                                                                       Hm, asymmetry);
  SNET_CHECK_LAUNCH("snet_vib_finish");
  return 0;
}
