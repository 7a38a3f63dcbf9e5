// Device helpers of the fp64 driver kernels that give one 256-thread workgroup to a system (or a copy, a row, an image):
// snet_relax.hip, snet_relax_cell.hip, snet_mdstep.hip, snet_mdnpt.hip, snet_neb.hip, snet_vib.hip, snet_phonon.hip and
// snet_elastic.hip.  One definition each of what those kernels share.  snet_observe.hip (the MD observables) stands on them too:
// `segment`, `block_sum`, `held_bits` and the 3x3 helpers.  Its own sums are written under contract(off); the products inside
// det3 / inv3 / row_mul contract as they do everywhere, which its integer pair counts do not see (a pair is never that close to a
// bin edge where the counts are compared) and its correlation sums do not go through.
//
// Contraction is part of the arithmetic.  vib, phonon and elastic equal their numpy restatements bit for bit because no product
// of theirs is contracted with the sum that follows it; relax, relax_cell, mdstep, mdnpt and neb compute under the HIP default.
// The pragma belongs to the text where it stands, not to the kernel a helper is inlined into: a helper of the first group
// (checked_range .. fd_stencil below, marked "contract(off)") carries the pragma in its own body, every other helper stands
// under no pragma, and nothing here is used by both groups with arithmetic that could be contracted (finite_d, the maxima and
// the ranges hold no product).
#pragma once
#include "snet_common.h"
#include "snet_philox.h"

namespace snet {

constexpr double MD_ACC = 9.648533212e-3;   // eV / (A amu) in A / fs^2

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }   // (false for a NaN)

// ---- reductions over a 256-thread workgroup -----------------------------------------------------------------------------------
// sums of NV per-thread values, in a fixed order: xor tree inside a wave, then waves 0..3 in sequence.  Every thread returns the
// same bits.  `sm` is reused by the next call: the trailing barrier protects it.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*sm)[4]) {
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const double t = wave_sum_d(v[c]);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][c] = t;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NV; ++c) v[c] = ((sm[0][c] + sm[1][c]) + sm[2][c]) + sm[3][c];
  __syncthreads();
}
// the maximum (exact in any order): one barrier, none after it -- a second call on the same `sm` needs one in between
__device__ __forceinline__ double block_max(double x, double *sm) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = x;
  __syncthreads();
  return fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}
// max that keeps a NaN (a NaN force must not pass for a converged system)
__device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double wave_max_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v = max_nan(v, __shfl_xor(v, o, 64));
  return v;
}
// the NaN-keeping maximum in two halves around a block_sum<3>(., sm) on the same `sm`: the four wave maxima go to the column the
// sums leave free, block_sum's first barrier publishes them, and no barrier is added
__device__ __forceinline__ void block_max_nan_put(double v, double (*sm)[4]) {
  const double t = wave_max_d(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][3] = t;
}
__device__ __forceinline__ double block_max_nan_get(const double (*sm)[4]) {
  return max_nan(max_nan(sm[0][3], sm[1][3]), max_nan(sm[2][3], sm[3][3]));
}

// ---- row ranges -----------------------------------------------------------------------------------------------------------------
// Rows [a0, a1) of an array of n rows by ptr[s], ptr[s + 1], in two forms.  The steppers (relax, relax_cell, mdstep, mdnpt, neb)
// own their seg_ptr and have no status word to refuse through: `segment` clamps to [0, n], so that a bad range moves nothing out
// of bounds.  The finite-difference kernels (vib, phonon, elastic) take descriptors from the caller and report per system:
// `checked_range` clamps nothing and says ok = false, and the kernel refuses before a row is read or written.
struct Segment {
  int64_t a0, a1;
};
__device__ __forceinline__ Segment segment(const int32_t *__restrict__ seg_ptr, int s, int64_t n) {
  int64_t a0 = seg_ptr[s], a1 = seg_ptr[s + 1];
  a0 = a0 < 0 ? 0 : (a0 > n ? n : a0);
  a1 = a1 > n ? n : (a1 < a0 ? a0 : a1);
  return Segment{a0, a1};
}
struct Range {
  int64_t a0, a1;
  bool ok;
};
__device__ __forceinline__ Range checked_range(const int32_t *__restrict__ ptr, int s, int64_t n) {
  const int64_t a0 = ptr[s], a1 = ptr[s + 1];
  return Range{a0, a1, a0 >= 0 && a1 >= a0 && a1 <= n};
}

// ---- finite differences over copies (vib, phonon, elastic): contract(off) --------------------------------------------------------
// copy j of base system b: rows `out` of the copies, rows `base` of the base array, ok where both lie inside their arrays and are
// of one size (seg_ptr0 is read only for a system that exists)
struct CopySlot {
  Range base, out;
  bool ok;
};
__device__ __forceinline__ CopySlot copy_slot(int b, const int32_t *__restrict__ copy_ptr, int j, int64_t n_out,
                                              const int32_t *__restrict__ seg_ptr0, int n_sys, int64_t n0) {
  CopySlot s{Range{0, 0, false}, checked_range(copy_ptr, j, n_out), false};
  if (b >= 0 && b < n_sys && s.out.ok) {
    s.base = checked_range(seg_ptr0, b, n0);
    s.ok = s.base.ok && s.base.a1 - s.base.a0 == s.out.a1 - s.out.a0;
  }
  return s;
}
// the signed step of a copy, rounded here and then used: q delta as numpy forms it
__device__ __forceinline__ double copy_step(int q, double delta) {
#pragma clang fp contract(off)
  const double s = (double)q * delta;
  return s;
}
// group g = (first copy j0, system b, row r): the nfree copies are rows a0[c] .. a0[c] + na of the force arrays; ok where the copies
// exist, lie inside the arrays and are of one size.  Without a system to report to nothing but the group is read.
struct RowGroup {
  int j0, b, r;
  int64_t a0[4], na;
  bool has_sys, ok;
};
__device__ __forceinline__ RowGroup row_group(const int32_t *__restrict__ group, int g, int nfree, int n_copies,
                                              const int32_t *__restrict__ seg_ptr, int64_t n, int n_sys) {
  RowGroup q{group[3 * g], group[3 * g + 1], group[3 * g + 2], {0, 0, 0, 0}, 0, false, false};
  q.has_sys = q.b >= 0 && q.b < n_sys;
  if (!q.has_sys) return q;
  q.ok = q.j0 >= 0 && (int64_t)q.j0 + nfree <= n_copies;
  if (q.ok) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {   // (nfree is 2 or 4: written over all four so that a0 stays in registers)
      if (c >= nfree) break;
      const Range seg = checked_range(seg_ptr, q.j0 + c, n);
      q.ok = q.ok && seg.ok && (c == 0 || seg.a1 - seg.a0 == q.na);
      q.a0[c] = seg.a0;
      if (c == 0) q.na = seg.a1 - seg.a0;
    }
  }
  return q;
}
// F[w] = forces[3 a0[w] + c] (+ forces_extra[...]) of the nfree copies; false where one of them is not finite
__device__ __forceinline__ bool load_copy_forces(const float *__restrict__ forces, const double *__restrict__ forces_extra,
                                                 const int64_t (&a0)[4], int64_t c, int nfree, double (&F)[4]) {
#pragma clang fp contract(off)
  bool fin = true;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w >= nfree) break;
    const int64_t i = 3 * a0[w] + c;
    F[w] = (double)forces[i];
    if (forces_extra) F[w] = F[w] + forces_extra[i];
    if (!finite_d(F[w])) fin = false;
  }
  return fin;
}
// minus the central difference of v over copies in the order q = -1, +1 (nfree 2) or q = -2, -1, +1, +2 (nfree 4), h2 = 2 delta,
// h12 = 12 delta: the derivative of an energy from its forces.  Handed the copies in the opposite order it is the plain difference.
__device__ __forceinline__ double fd_stencil(const double (&v)[4], int nfree, double h2, double h12) {
#pragma clang fp contract(off)
  const double d = nfree == 2 ? (v[0] - v[1]) / h2 : (((8.0 * v[1] - v[0]) - 8.0 * v[2]) + v[3]) / h12;
  return d;
}

// the shared checks and the launch of a copy writer (snet_vib_displace, snet_el_strain: one argument list)
using CopyWriter = void (*)(const double *, int64_t, const int32_t *, int, const int32_t *, const int32_t *, double, double *, int64_t,
                            int32_t *);
inline int launch_copy_writer(const char *name, CopyWriter kernel, const double *pos0, int64_t n0, const int32_t *seg_ptr0,
                              int32_t n_sys, const int32_t *desc, const int32_t *copy_ptr, int32_t n_copies, double delta,
                              double *pos_out, int64_t n_out, int32_t *status, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_copies >= 1 && n0 >= 0 && n0 < (1ll << 31) && n_out >= 0 && n_out < (1ll << 31),
               std::string(name) + ": bad shape");
  SNET_REQUIRE(pos0 && seg_ptr0 && desc && copy_ptr && pos_out && status, std::string(name) + ": null argument");
  kernel<<<(unsigned)n_copies, 256, 0, static_cast<hipStream_t>(stream)>>>(pos0, n0, seg_ptr0, n_sys, desc, copy_ptr, delta, pos_out,
                                                                          n_out, status);
  SNET_CHECK_LAUNCH(name);
  return 0;
}

// ---- the steppers (relax, relax_cell, mdstep, mdnpt, neb): HIP's default contraction -------------------------------------------
// force on atom i in fp64: the model's fp32 forces[3 i + k] widened, plus the fp64 forces_extra[3 i + k] when there is one
__device__ __forceinline__ void load_force(const float *__restrict__ forces, const double *__restrict__ forces_extra, int64_t i,
                                           double (&F)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) F[k] = (double)forces[3 * i + k];
  if (forces_extra) {
#pragma unroll
    for (int k = 0; k < 3; ++k) F[k] += forces_extra[3 * i + k];
  }
}
// the hold mask of the *_fixed entry points: bit k of hold[i] & 7 says that Cartesian component k of atom i is held
__device__ __forceinline__ int held_bits(const int32_t *__restrict__ hold, int64_t i) { return hold[i] & 7; }
__device__ __forceinline__ bool is_held(int h, int k) { return ((h >> k) & 1) != 0; }
// x with its held components replaced by 0, by selection: what a held component carried (a NaN force, a stale velocity) goes nowhere
__device__ __forceinline__ void zero_held(int h, double (&x)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = is_held(h, k) ? 0.0 : x[k];
}
// load_force under a mask
__device__ __forceinline__ void load_force_free(const float *__restrict__ forces, const double *__restrict__ forces_extra, int64_t i,
                                                int h, double (&F)[3]) {
  load_force(forces, forces_extra, i, F);
  zero_held(h, F);
}

// FIRE (snet_fire_step, snet_fire_cell_step)
struct FireParams {
  double fmax, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step;
  int n_min;
};
inline bool fire_params_ok(double fmax, double dt_start, const FireParams &p) {
  return fmax >= 0 && dt_start > 0 && p.dt_max >= dt_start && p.n_min >= 0 && p.f_inc >= 1 && p.f_dec > 0 && p.f_dec < 1 &&
         p.alpha_start > 0 && p.alpha_start <= 1 && p.f_alpha > 0 && p.f_alpha <= 1 && p.max_step > 0;
}
// the mixing of this step, v <- keep v + ((push g) / |g|) |v|, by the sign of the power g.v; updates the system's dt, alpha, n_pos
struct FireMix {
  double keep, push;
};
__device__ __forceinline__ FireMix fire_decide(double power, const FireParams &p, double &dt, double &alpha, int &n_pos) {
  if (power > 0.0) {
    const FireMix mix{1.0 - alpha, alpha};
    if (n_pos > p.n_min) {
      dt = fmin(dt * p.f_inc, p.dt_max);
      alpha = alpha * p.f_alpha;
    }
    n_pos += 1;
    return mix;
  }
  alpha = p.alpha_start;
  dt = dt * p.f_dec;
  n_pos = 0;
  return FireMix{0.0, 0.0};
}
// FIRE's velocity update of one component: the mixing as decided for the system, then v += dt g
__device__ __forceinline__ double new_velocity(double v_old, double g, double keep, double push, double nF, double nV, double dt) {
  double v = 0.0;
  if (push > 0.0 || keep > 0.0) v = keep * v_old + push * g / nF * nV;
  return v + dt * g;
}
// count the active systems (one thread per workgroup calls this): one integer atomic on *word = (ticket << 32) | still active, the
// last arrival publishes the sum and puts the word back to zero, so every launch starts from zero
__device__ __forceinline__ void count_active(unsigned long long *word, bool still_active, int n_sys, int32_t *__restrict__ n_active) {
  const unsigned long long old = atomicAdd(word, (1ull << 32) | (still_active ? 1ull : 0ull));
  if ((unsigned)(old >> 32) == (unsigned)(n_sys - 1)) {
    *n_active = (int32_t)((unsigned)(old & 0xffffffffull) + (still_active ? 1u : 0u));
    atomicExch(word, 0ull);
  }
}

// BAOAB (snet_mdb_step, snet_mdb_npt_step)
// a product that is never contracted with the sum that follows it: with mu == 1 the scaled position is the position, and the
// drift after it rounds as without a barostat
__device__ __forceinline__ double mul_rounded(double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return p;
}
__device__ __forceinline__ void half_kick3(double (&v)[3], const double (&F)[3], double half_kick, double m) {
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] += half_kick * F[k] / m;
}
struct BaoabStep {
  bool finish, start;          // phase bits: the half kick that ends a step, the half kick and drift that begin the next
  double dt, c1, c2, half_kick, kt_acc;
  double mu;                   // the barostat's rescaling between kicks and drift; the literal 1.0 compiles to no rescaling
  uint64_t seed;
  uint32_t sys, step;
};
// one atom (i, number `a` of its system) through the step; returns m |v|^2 after the finishing kick.  Nothing is stored where
// neither phase bit is set.  HOLD (snet_mdb_step_fixed): the components in the mask bits h enter with velocity and force 0, so
// that they are neither kicked nor counted in m |v|^2; their positions are not written and their velocities are stored as 0.
// The noise is drawn as without a mask, and every update is component-wise: a free component sees the arithmetic of HOLD = false.
template <bool HOLD = false>
__device__ __forceinline__ double baoab_atom(const BaoabStep &p, double *__restrict__ pos, double *__restrict__ vel,
                                             const float *__restrict__ forces, const double *__restrict__ forces_extra,
                                             const double *__restrict__ mass, int64_t i, uint32_t a, int h = 0) {
  const double m = mass[i];
  double v[3] = {vel[3 * i + 0], vel[3 * i + 1], vel[3 * i + 2]};
  double F[3] = {0.0, 0.0, 0.0};
  if (p.finish || p.start) load_force(forces, forces_extra, i, F);
  if constexpr (HOLD) {
    zero_held(h, v);
    zero_held(h, F);
  }
  if (p.finish) half_kick3(v, F, p.half_kick, m);
  const double mv2 = m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (p.start) {
    double x[3] = {pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2]};
    half_kick3(v, F, p.half_kick, m);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = mul_rounded(p.mu, x[k]);
      v[k] = v[k] / p.mu;
    }
    if (p.c2 == 0.0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) x[k] += p.dt * v[k];
    } else {
      double xi[3];
      normals3(p.seed, a, p.sys, p.step, STREAM_THERMOSTAT, xi);
      const double sigma = p.c2 * sqrt(p.kt_acc / m);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        x[k] += 0.5 * p.dt * v[k];
        v[k] = p.c1 * v[k] + sigma * xi[k];
        x[k] += 0.5 * p.dt * v[k];
      }
    }
    if constexpr (HOLD) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (!is_held(h, k)) pos[3 * i + k] = x[k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) pos[3 * i + k] = x[k];
    }
  }
  if (p.finish || p.start) {
    if constexpr (HOLD) zero_held(h, v);   // (the thermostat's noise on a held component goes nowhere)
#pragma unroll
    for (int k = 0; k < 3; ++k) vel[3 * i + k] = v[k];
  }
  return mv2;
}

// ---- 3x3 matrices, row-major ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double det3(const double *a) {
  return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}
// the smallest face-to-face height of the cell c: |det c| / |a_j x a_k| over the three axes
__device__ __forceinline__ double min_height3(const double *c) {
  const double vol = fabs(det3(c));
  double h = INFINITY;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double *u = c + 3 * ((i + 1) % 3), *w = c + 3 * ((i + 2) % 3);
    const double x = u[1] * w[2] - u[2] * w[1], y = u[2] * w[0] - u[0] * w[2], z = u[0] * w[1] - u[1] * w[0];
    h = fmin(h, vol / sqrt(x * x + y * y + z * z));
  }
  return h;
}
__device__ __forceinline__ void inv3(const double *a, double det, double *inv) {
  const double id = 1.0 / det;
  inv[0] = (a[4] * a[8] - a[5] * a[7]) * id;
  inv[1] = (a[2] * a[7] - a[1] * a[8]) * id;
  inv[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  inv[3] = (a[5] * a[6] - a[3] * a[8]) * id;
  inv[4] = (a[0] * a[8] - a[2] * a[6]) * id;
  inv[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  inv[6] = (a[3] * a[7] - a[4] * a[6]) * id;
  inv[7] = (a[1] * a[6] - a[0] * a[7]) * id;
  inv[8] = (a[0] * a[4] - a[1] * a[3]) * id;
}
// out = a b^T
__device__ __forceinline__ void mul_abt(const double *a, const double *b, double *out) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}
// out = x m (row vector times matrix) and out = x m^T; out must not be x
__device__ __forceinline__ void row_mul(const double *x, const double *m, double *out) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = x[0] * m[j] + x[1] * m[3 + j] + x[2] * m[6 + j];
}
__device__ __forceinline__ void row_mul_t(const double *x, const double *m, double *out) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = x[0] * m[3 * j] + x[1] * m[3 * j + 1] + x[2] * m[3 * j + 2];
}

}  // namespace snet
