// Batched finite-difference Hessians: the displaced copies of many structures are written on the device, and the engine's forces
// on them are reduced to the rows of the central-difference matrix D, then to the Hessian H = (D + D^T) / 2, its mass-weighted
// form and the asymmetry max |D - D^T|.  The rule is written out in include/snet_hip.h (snet_vib_displace, snet_vib_rows,
// snet_vib_finish) and restated in fp64 numpy in tests/vib_ref.py.
//
// One 256-thread workgroup per unit of work (a copy, a row of D, a system), fp64, no atomics and no sum over threads: every
// element of D, H and Hm is computed by one thread from at most four forces in a written-out order, and the one reduction, the
// maximum of the asymmetry, does not depend on its order.  No product is contracted with the sum that follows it, so the
// results equal the numpy restatement of the same expressions bit for bit.
#include "snet_common.h"

namespace {

constexpr int VIB_THREADS = 256;
constexpr int VIB_WAVES = VIB_THREADS / 64;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }   // (false for a NaN)

// rows [a0, a1) of a [n,3] array by seg_ptr[s], seg_ptr[s+1], or ok = false where they are not inside it (nothing is clamped:
// a range that does not fit is refused)
struct VibRange {
  int64_t a0, a1;
  bool ok;
};
__device__ __forceinline__ VibRange vib_range(const int32_t *__restrict__ ptr, int s, int64_t n) {
  const int64_t a0 = ptr[s], a1 = ptr[s + 1];
  return VibRange{a0, a1, a0 >= 0 && a1 >= a0 && a1 <= n};
}

__global__ __launch_bounds__(VIB_THREADS) void vib_displace_kernel(
    const double *__restrict__ pos0, int64_t n0, const int32_t *__restrict__ seg_ptr0, int n_sys, const int32_t *__restrict__ desc,
    const int32_t *__restrict__ copy_ptr, double delta, double *__restrict__ pos_out, int64_t n_out, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
  const int j = blockIdx.x;   // the copy
  const int tid = threadIdx.x;
  const int b = desc[4 * j], atom = desc[4 * j + 1], axis = desc[4 * j + 2], q = desc[4 * j + 3];
  bool ok = b >= 0 && b < n_sys && axis >= 0 && axis < 3 && q >= -2 && q <= 2;
  const VibRange out = vib_range(copy_ptr, j, n_out);
  ok = ok && out.ok;
  VibRange base{0, 0, false};
  if (ok) {   // (seg_ptr0 is read only for a system that exists)
    base = vib_range(seg_ptr0, b, n0);
    ok = base.ok && base.a1 - base.a0 == out.a1 - out.a0 && atom >= 0 && atom < base.a1 - base.a0;
  }
  if (!ok) {   // refused before a row is read or written (uniform over the workgroup)
    if (tid == 0) status[j] = 1;
    return;
  }
  const int64_t na = base.a1 - base.a0;
  const double shift = (double)q * delta;   // rounded here, then added: x + q delta as numpy forms it
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
  const int g = blockIdx.x;   // the row group
  const int tid = threadIdx.x;
  const int j0 = group[3 * g], b = group[3 * g + 1], r = group[3 * g + 2];
  if (b < 0 || b >= n_sys) return;   // no system to report to: nothing is read or written
  bool ok = j0 >= 0 && (int64_t)j0 + nfree <= n_copies;
  const VibRange s = vib_range(sel_ptr, b, n_sel);
  const int64_t m3 = 3 * (s.a1 - s.a0), off = d_off[b];
  ok = ok && s.ok && m3 > 0 && r >= 0 && r < m3 && off >= 0 && off <= d_size && m3 * m3 <= d_size - off;
  int64_t a0[4] = {0, 0, 0, 0}, na = 0;
  if (ok) {   // the copies of the group: inside the force arrays and all of one size
    for (int c = 0; c < nfree; ++c) {
      const VibRange seg = vib_range(seg_ptr, j0 + c, n);
      ok = ok && seg.ok && (c == 0 || seg.a1 - seg.a0 == na);
      a0[c] = seg.a0;
      if (c == 0) na = seg.a1 - seg.a0;
    }
  }
  if (!ok) {   // (uniform over the workgroup)
    if (tid == 0) status[b] = 3;
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
    const int k = (int)(c % 3);
    double F[4];
    for (int w = 0; w < nfree; ++w) {
      const int64_t i = 3 * (a0[w] + atom) + k;
      F[w] = (double)forces[i];
      if (forces_extra) F[w] = F[w] + forces_extra[i];
      if (!finite_d(F[w])) bad_force = true;
    }
    // copies in the order q = -1, +1 (nfree 2) or q = -2, -1, +1, +2 (nfree 4)
    row[c] = nfree == 2 ? (F[0] - F[1]) / h2 : (((8.0 * F[1] - F[0]) - 8.0 * F[2]) + F[3]) / h12;
  }
  if (bad_atom) status[b] = 3;          // (every writer of a system's status writes a non-zero value: any of them marks it failed)
  else if (bad_force) status[b] = 2;
}

__global__ __launch_bounds__(VIB_THREADS) void vib_finish_kernel(
    const double *__restrict__ D, const int64_t *__restrict__ d_off, const int32_t *__restrict__ sel_ptr, int64_t n_sel,
    const double *__restrict__ w, int64_t d_size, int32_t *__restrict__ status, double *__restrict__ H,
    double *__restrict__ Hm, double *__restrict__ asym) {
#pragma clang fp contract(off)
  __shared__ double sm[VIB_WAVES];
  const int b = blockIdx.x;   // the system
  const int tid = threadIdx.x;
  const VibRange s = vib_range(sel_ptr, b, n_sel);
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
  // the maximum over the workgroup (exact in any order)
  for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o));
  if ((tid & 63) == 0) sm[tid >> 6] = worst;
  __syncthreads();
  if (tid == 0) asym[b] = failed ? nan_d : fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}

}  // namespace

extern "C" int snet_vib_displace(const double *pos0, int64_t n0, const int32_t *seg_ptr0, int32_t n_sys, const int32_t *desc,
                                 const int32_t *copy_ptr, int32_t n_copies, double delta, double *pos_out, int64_t n_out,
                                 int32_t *status, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_copies >= 1 && n0 >= 0 && n0 < (1ll << 31) && n_out >= 0 && n_out < (1ll << 31),
               "snet_vib_displace: bad shape");
  SNET_REQUIRE(pos0 && seg_ptr0 && desc && copy_ptr && pos_out && status, "snet_vib_displace: null argument");
  vib_displace_kernel<<<(unsigned)n_copies, VIB_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos0, n0, seg_ptr0, n_sys, desc, copy_ptr, delta, pos_out, n_out, status);
  SNET_CHECK_LAUNCH("snet_vib_displace");
  return 0;
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
