// Batched supercell phonons: the rows of the force-constant matrix of the home-cell atoms against all atoms of the supercell,
// the acoustic sum rule, the nearest images of every (home atom, supercell atom) pair and the dynamical matrices D(q) of many
// q-points.  The rule is written out in include/snet_hip.h (snet_ph_rows, snet_ph_finish, snet_ph_images, snet_ph_dynmat) and
// restated in fp64 numpy in tests/phonon_ref.py.
//
// One 256-thread workgroup per unit of work (a row of Phi, a system, a home atom, a (q, home atom) pair, a q-point), fp64, no
// atomics: every output element is written by one thread, every sum runs in a written-out order, and the two reductions over a
// workgroup are maxima, which do not depend on their order.  No product is contracted with the sum that follows it.  A
// descriptor that does not fit the buffers is refused with a status word: nothing is clamped, nothing out of range is touched.
#include "snet_system.h"

#pragma clang fp contract(off)   // (this file's own text; the helpers of snet_system.h carry theirs)

namespace {

using namespace snet;   // the shared device helpers (snet_system.h)

constexpr int PH_THREADS = 256;
constexpr int PH_TILE = 1024;                // phases of one pass of ph_dynmat_rows_kernel: 2 x 8 KiB of LDS
constexpr int64_t PH_MAX = 1ll << 31;

// system b of a launch: its m home atoms are entries [h0, h0 + m) of the per-home-atom arrays and its N supercell atoms rows
// [a0, a0 + N) of the per-atom arrays; ok = false where these do not lie inside [0, n_home] / [0, n_atoms], m < 1 or N is no
// multiple of m
struct PhSys {
  int64_t h0, m, a0, N;
  bool ok;
};
__device__ __forceinline__ PhSys ph_sys(const int32_t *__restrict__ m_ptr, const int32_t *__restrict__ sc_ptr, int b, int64_t n_home,
                                        int64_t n_atoms) {
  const int64_t h0 = m_ptr[b], h1 = m_ptr[b + 1], a0 = sc_ptr[b], a1 = sc_ptr[b + 1];
  const int64_t m = h1 - h0, N = a1 - a0;
  const bool ok = h0 >= 0 && m >= 1 && h1 <= n_home && a0 >= 0 && N >= m && a1 <= n_atoms && N % m == 0;
  return PhSys{h0, m, a0, N, ok};
}

// `count` elements from `off` lie inside a buffer of `size` elements, count = f a b with a b < 2^62 (no product overflows)
__device__ __forceinline__ bool ph_fits(int64_t off, int64_t size, int64_t f, int64_t a, int64_t b) {
  return off >= 0 && off <= size && a * b <= (size - off) / f;
}

// d = d0 + n S (rows of S are the supercell's lattice vectors), each component in the order written
__device__ __forceinline__ void ph_image(const double *d0, const double *S, int n1, int n2, int n3, double *d) {
  for (int c = 0; c < 3; ++c) d[c] = d0[c] + (((double)n1 * S[c] + (double)n2 * S[3 + c]) + (double)n3 * S[6 + c]);
}

// ------------------------------------------------------------------------------------------------ rows of Phi
__global__ __launch_bounds__(PH_THREADS) void ph_rows_kernel(
    const float *__restrict__ forces, const double *__restrict__ forces_extra, int64_t n, const int32_t *__restrict__ seg_ptr,
    int n_copies, const int32_t *__restrict__ group, int nfree, double delta, const int32_t *__restrict__ m_ptr,
    const int32_t *__restrict__ sc_ptr, const int64_t *__restrict__ p_off, int n_sys, double *__restrict__ phi, int64_t p_size,
    int32_t *__restrict__ status) {
  const int tid = threadIdx.x;
  const RowGroup rg = row_group(group, blockIdx.x, nfree, n_copies, seg_ptr, n, n_sys);
  if (!rg.has_sys) return;   // no system to report to: nothing is read or written
  const int b = rg.b, r = rg.r;
  const PhSys s = ph_sys(m_ptr, sc_ptr, b, PH_MAX, PH_MAX);   // (m and N only: the forces are indexed through seg_ptr)
  const int64_t off = p_off[b];
  if (!(rg.ok && s.ok && r >= 0 && r < 3 * s.m && ph_fits(off, p_size, 9, s.m, s.N) && rg.na == s.N)) {   // (each copy a whole supercell)
    if (tid == 0) status[b] = 3;   // (uniform over the workgroup)
    return;
  }
  double *__restrict__ row = phi + off + (int64_t)r * 3 * s.N;
  const double h2 = 2.0 * delta, h12 = 12.0 * delta;
  bool bad_force = false;
  for (int64_t c = tid; c < 3 * s.N; c += PH_THREADS) {
    double F[4];
    if (!load_copy_forces(forces, forces_extra, rg.a0, c, nfree, F)) bad_force = true;
    row[c] = fd_stencil(F, nfree, h2, h12);   // the stencil of snet_vib_rows
  }
  if (bad_force) status[b] = 2;   // (every writer of a system's status writes a non-zero value: any of them marks it failed)
}

// ------------------------------------------------------------------------------------------------ the sum rule
__global__ __launch_bounds__(PH_THREADS) void ph_finish_kernel(
    const double *__restrict__ phi, const int64_t *__restrict__ p_off, const int32_t *__restrict__ m_ptr,
    const int32_t *__restrict__ sc_ptr, int64_t p_size, int acoustic, int32_t *__restrict__ status, double *__restrict__ phi_out,
    double *__restrict__ asr) {
  __shared__ double sm[4];
  const int b = blockIdx.x;   // the system
  const int tid = threadIdx.x;
  const PhSys s = ph_sys(m_ptr, sc_ptr, b, PH_MAX, PH_MAX);
  const int64_t off = p_off[b];
  const double nan_d = __builtin_nan("");
  if (!(s.ok && ph_fits(off, p_size, 9, s.m, s.N))) {   // a block outside the buffers: nothing of it is touched
    if (tid == 0) status[b] = 3, asr[b] = nan_d;
    return;
  }
  const int64_t n3 = 3 * s.N, total = 3 * s.m * n3;
  if (status[b] != 0) {
    for (int64_t e = tid; e < total; e += PH_THREADS) phi_out[off + e] = nan_d;
    if (tid == 0) asr[b] = nan_d;
    return;
  }
  // every element but the self terms Phi[(a,i),(a,k)] is copied; those are written below, by the thread that sums their column
  for (int64_t e = tid; e < total; e += PH_THREADS) {
    const int64_t r = e / n3, c = e % n3;
    if (c / 3 != r / 3) phi_out[off + e] = phi[off + e];
  }
  double worst = 0.0;
  for (int64_t p = tid; p < 9 * s.m; p += PH_THREADS) {
    const int64_t r = p / 3, k = p % 3, a = r / 3;
    const double *__restrict__ row = phi + off + r * n3;
    double all = 0.0, others = 0.0;
    for (int64_t j = 0; j < s.N; ++j) {   // ascending j
      const double x = row[3 * j + k];
      all = all + x;
      if (j != a) others = others + x;
    }
    worst = fmax(worst, fabs(all));
    phi_out[off + r * n3 + 3 * a + k] = acoustic ? -others : row[3 * a + k];
  }
  worst = block_max(worst, sm);
  if (tid == 0) asr[b] = worst;
}

// ------------------------------------------------------------------------------------------------ nearest images
__global__ __launch_bounds__(PH_THREADS) void ph_images_kernel(
    const double *__restrict__ pos, int64_t n_atoms, const int32_t *__restrict__ sc_ptr, const int32_t *__restrict__ m_ptr,
    const int32_t *__restrict__ home_sys, int64_t n_home, const double *__restrict__ S, const double *__restrict__ S_inv,
    const int64_t *__restrict__ i_off, int n_sys, double symprec, int32_t *__restrict__ img_base, int32_t *__restrict__ img_mask,
    int64_t i_size, int32_t *__restrict__ status) {
  const int h = blockIdx.x;   // the home atom, over all systems
  const int tid = threadIdx.x;
  const int b = home_sys[h];
  if (b < 0 || b >= n_sys) return;   // no system to report to
  const PhSys s = ph_sys(m_ptr, sc_ptr, b, n_home, n_atoms);
  const int64_t off = i_off[b], a = h - s.h0;
  if (!(s.ok && a >= 0 && a < s.m && ph_fits(off, i_size, 1, s.m, s.N))) {
    if (tid == 0) status[b] = 3;
    return;
  }
  double Sb[9], Si[9], ra[3];
  for (int c = 0; c < 9; ++c) Sb[c] = S[9 * (int64_t)b + c], Si[c] = S_inv[9 * (int64_t)b + c];
  for (int c = 0; c < 3; ++c) ra[c] = pos[3 * (s.a0 + a) + c];
  bool bad = false;
  for (int64_t j = tid; j < s.N; j += PH_THREADS) {
    double d0[3], f[3];
    for (int c = 0; c < 3; ++c) d0[c] = pos[3 * (s.a0 + j) + c] - ra[c];
    bool fin = true;
    for (int c = 0; c < 3; ++c) {
      f[c] = (d0[0] * Si[c] + d0[1] * Si[3 + c]) + d0[2] * Si[6 + c];
      fin = fin && fabs(f[c]) <= 1.0e9;   // (false for a NaN)
    }
    const int64_t e = off + a * s.N + j;
    if (!fin) {   // a position or a cell that is not a number, or not of this lattice: no image is kept
      bad = true;
      img_base[3 * e] = img_base[3 * e + 1] = img_base[3 * e + 2] = 0;
      img_mask[e] = 0;
      continue;
    }
    int n0[3];
    for (int c = 0; c < 3; ++c) n0[c] = -(int)rint(f[c]);
    double len[27], shortest = 0.0;
    for (int t = 0; t < 27; ++t) {
      double d[3];
      ph_image(d0, Sb, n0[0] + t / 9 - 1, n0[1] + (t / 3) % 3 - 1, n0[2] + t % 3 - 1, d);
      len[t] = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      shortest = t == 0 ? len[0] : fmin(shortest, len[t]);
    }
    int32_t mask = 0;
    const double limit = shortest + symprec;
    for (int t = 0; t < 27; ++t)
      if (len[t] <= limit) mask |= 1 << t;
    img_base[3 * e] = n0[0], img_base[3 * e + 1] = n0[1], img_base[3 * e + 2] = n0[2];
    img_mask[e] = mask;
  }
  if (bad) status[b] = 3;
}

// ------------------------------------------------------------------------------------------------ D(q)
// what both dynmat kernels check before they touch anything: the system of q-point gq and where its blocks lie
struct PhDyn {
  PhSys s;
  int64_t ql, phi0, img0, out0;   // q within its system; first element of Phi, of the image arrays, of the [3m,3m] block of R / D
  bool ok;
};
__device__ __forceinline__ PhDyn ph_dyn(int gq, int b, int64_t n_q, const int32_t *__restrict__ m_ptr, const int32_t *__restrict__ sc_ptr,
                                        int64_t n_home, int64_t n_atoms, const int64_t *__restrict__ p_off, int64_t p_size,
                                        const int64_t *__restrict__ i_off, int64_t i_size, const int32_t *__restrict__ q_ptr,
                                        const int64_t *__restrict__ d_off, int64_t d_size) {
  PhDyn y;
  y.s = ph_sys(m_ptr, sc_ptr, b, n_home, n_atoms);
  const int64_t q0 = q_ptr[b], q1 = q_ptr[b + 1];
  y.ql = gq - q0;
  y.phi0 = p_off[b], y.img0 = i_off[b];
  y.ok = y.s.ok && y.s.m <= 65535 && q0 >= 0 && q1 <= n_q && gq >= q0 && gq < q1 && ph_fits(y.phi0, p_size, 9, y.s.m, y.s.N) &&
         ph_fits(y.img0, i_size, 1, y.s.m, y.s.N) && ph_fits(d_off[b], d_size, 9, (q1 - q0) * y.s.m, y.s.m);
  y.out0 = y.ok ? d_off[b] + y.ql * 9 * y.s.m * y.s.m : 0;
  return y;
}

// rows 3 a .. 3 a + 2 of R(q): the phases of the pairs (a, j) are computed once per q, one thread each, staged in LDS a tile at a
// time and reused for the nine Cartesian entries of the pair; element (i, (beta, k)) is summed over the cells by one thread, in
// ascending order, and carried through the tiles in its own place in R
__global__ __launch_bounds__(PH_THREADS) void ph_dynmat_rows_kernel(
    const double *__restrict__ phi, const int64_t *__restrict__ p_off, int64_t p_size, const double *__restrict__ pos, int64_t n_atoms,
    const int32_t *__restrict__ sc_ptr, const int32_t *__restrict__ m_ptr, const double *__restrict__ w, int64_t n_home,
    const double *__restrict__ S, const int32_t *__restrict__ img_base, const int32_t *__restrict__ img_mask,
    const int64_t *__restrict__ i_off, int64_t i_size, const double *__restrict__ q_cart, const int32_t *__restrict__ q_sys,
    const int32_t *__restrict__ q_ptr, int n_q, const int64_t *__restrict__ d_off, int n_sys, int32_t *__restrict__ status,
    double *__restrict__ R, int64_t d_size) {
  __shared__ double ph_re[PH_TILE], ph_im[PH_TILE];
  const int gq = blockIdx.x, tid = threadIdx.x;
  const int64_t a = blockIdx.y;
  const int b = q_sys[gq];
  if (b < 0 || b >= n_sys) return;   // no system to report to
  const PhDyn y = ph_dyn(gq, b, n_q, m_ptr, sc_ptr, n_home, n_atoms, p_off, p_size, i_off, i_size, q_ptr, d_off, d_size);
  if (!y.ok) {   // (uniform over the workgroup, and over the workgroups of this q-point)
    if (tid == 0 && a == 0) status[b] = 3;
    return;
  }
  const int64_t m = y.s.m, N = y.s.N, m3 = 3 * m;
  if (a >= m) return;
  double Sb[9], ra[3], qv[3];
  for (int c = 0; c < 9; ++c) Sb[c] = S[9 * (int64_t)b + c];
  for (int c = 0; c < 3; ++c) ra[c] = pos[3 * (y.s.a0 + a) + c], qv[c] = q_cart[3 * (int64_t)gq + c];
  const double wa = w[y.s.h0 + a];
  double *__restrict__ Rq = R + 2 * y.out0;
  for (int64_t j0 = 0; j0 < N; j0 += PH_TILE) {
    const int64_t jn = N - j0 < PH_TILE ? N - j0 : PH_TILE;
    for (int64_t t = tid; t < jn; t += PH_THREADS) {
      const int64_t j = j0 + t, e = y.img0 + a * N + j;
      double d0[3];
      for (int c = 0; c < 3; ++c) d0[c] = pos[3 * (y.s.a0 + j) + c] - ra[c];
      const int n0[3] = {img_base[3 * e], img_base[3 * e + 1], img_base[3 * e + 2]};
      const int32_t mask = img_mask[e];
      double sum_re = 0.0, sum_im = 0.0;
      int kept = 0;
      for (int bit = 0; bit < 27; ++bit) {   // ascending (x, y, z)
        if (!((mask >> bit) & 1)) continue;
        double d[3], sn, cs;
        ph_image(d0, Sb, n0[0] + bit / 9 - 1, n0[1] + (bit / 3) % 3 - 1, n0[2] + bit % 3 - 1, d);
        sincos((qv[0] * d[0] + qv[1] * d[1]) + qv[2] * d[2], &sn, &cs);
        sum_re = sum_re + cs, sum_im = sum_im + sn;
        ++kept;
      }
      ph_re[t] = sum_re / (double)kept, ph_im[t] = sum_im / (double)kept;   // (no image kept: NaN, and so is what it enters)
    }
    __syncthreads();
    const bool first = j0 == 0, last = j0 + PH_TILE >= N;
    for (int64_t el = tid; el < 3 * m3; el += PH_THREADS) {
      const int64_t i = el / m3, col = el % m3, beta = col / 3, k = col % 3;
      const int64_t at = 2 * ((3 * a + i) * m3 + col);
      double acc_re = first ? 0.0 : Rq[at], acc_im = first ? 0.0 : Rq[at + 1];
      const double *__restrict__ row = phi + y.phi0 + (3 * a + i) * 3 * N + k;
      int64_t c = j0 > beta ? (j0 - beta + m - 1) / m : 0;
      for (int64_t j = c * m + beta; j < j0 + jn; j += m) {   // the cells in ascending order
        const double x = row[3 * j];
        acc_re = acc_re + x * ph_re[j - j0];
        acc_im = acc_im + x * ph_im[j - j0];
      }
      if (last) {
        const double ww = wa * w[y.s.h0 + beta];
        acc_re = ww * acc_re, acc_im = ww * acc_im;
      }
      Rq[at] = acc_re, Rq[at + 1] = acc_im;
    }
    __syncthreads();
  }
}

// D = (R + R^H) / 2 and max |R - R^H| of one q-point
__global__ __launch_bounds__(PH_THREADS) void ph_dynmat_sym_kernel(
    const int64_t *__restrict__ p_off, int64_t p_size, int64_t n_atoms, const int32_t *__restrict__ sc_ptr,
    const int32_t *__restrict__ m_ptr, int64_t n_home, const int64_t *__restrict__ i_off, int64_t i_size,
    const int32_t *__restrict__ q_sys, const int32_t *__restrict__ q_ptr, int n_q, const int64_t *__restrict__ d_off, int n_sys,
    const double *__restrict__ R, double *__restrict__ D, int64_t d_size, double *__restrict__ herm) {
  __shared__ double sm[4];
  const int gq = blockIdx.x, tid = threadIdx.x;
  const int b = q_sys[gq];
  if (b < 0 || b >= n_sys) return;
  const PhDyn y = ph_dyn(gq, b, n_q, m_ptr, sc_ptr, n_home, n_atoms, p_off, p_size, i_off, i_size, q_ptr, d_off, d_size);
  if (!y.ok) return;   // (the rows kernel has set the status)
  const int64_t m3 = 3 * y.s.m;
  const double *__restrict__ Rq = R + 2 * y.out0;
  double *__restrict__ Dq = D + 2 * y.out0;
  double worst = 0.0, not_finite = 0.0;
  for (int64_t e = tid; e < m3 * m3; e += PH_THREADS) {
    const int64_t r = e / m3, c = e % m3;
    const double x_re = Rq[2 * e], x_im = Rq[2 * e + 1], y_re = Rq[2 * (c * m3 + r)], y_im = Rq[2 * (c * m3 + r) + 1];
    Dq[2 * e] = (x_re + y_re) * 0.5;       // (x + y and y + x, x - y and -(y - x) have the same bits: D equals D^H bit for bit)
    Dq[2 * e + 1] = (x_im - y_im) * 0.5;
    const double diff = hypot(x_re - y_re, x_im + y_im);
    if (finite_d(diff)) worst = fmax(worst, diff);
    else not_finite = 1.0;
  }
  worst = block_max(worst, sm);
  __syncthreads();
  not_finite = block_max(not_finite, sm);
  if (tid == 0) herm[gq] = not_finite != 0.0 ? __builtin_nan("") : worst;
}

}  // namespace

extern "C" int snet_ph_rows(const float *forces, const double *forces_extra, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_copies,
                            const int32_t *group, int32_t n_groups, int32_t nfree, double delta, const int32_t *m_ptr,
                            const int32_t *sc_ptr, const int64_t *p_off, int32_t n_sys, double *phi, int64_t p_size, int32_t *status,
                            void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_copies >= 1 && n_groups >= 1 && n_atoms >= 0 && n_atoms < PH_MAX && p_size >= 1, "snet_ph_rows: bad shape");
  SNET_REQUIRE(nfree == 2 || nfree == 4, "snet_ph_rows: nfree must be 2 or 4");
  SNET_REQUIRE(forces && seg_ptr && group && m_ptr && sc_ptr && p_off && phi && status, "snet_ph_rows: null argument");
  ph_rows_kernel<<<(unsigned)n_groups, PH_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      forces, forces_extra, n_atoms, seg_ptr, n_copies, group, nfree, delta, m_ptr, sc_ptr, p_off, n_sys, phi, p_size, status);
  SNET_CHECK_LAUNCH("snet_ph_rows");
  return 0;
}

extern "C" int snet_ph_finish(const double *phi, const int64_t *p_off, const int32_t *m_ptr, const int32_t *sc_ptr, int32_t n_sys,
                              int64_t p_size, int32_t acoustic, int32_t *status, double *phi_out, double *asr_defect, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && p_size >= 1, "snet_ph_finish: bad shape");
  SNET_REQUIRE(phi && p_off && m_ptr && sc_ptr && status && phi_out && asr_defect && phi != phi_out, "snet_ph_finish: null or aliased argument");
  ph_finish_kernel<<<(unsigned)n_sys, PH_THREADS, 0, static_cast<hipStream_t>(stream)>>>(phi, p_off, m_ptr, sc_ptr, p_size, acoustic != 0,
                                                                                      status, phi_out, asr_defect);
  SNET_CHECK_LAUNCH("snet_ph_finish");
  return 0;
}

extern "C" int snet_ph_images(const double *pos, int64_t n_atoms, const int32_t *sc_ptr, const int32_t *m_ptr, const int32_t *home_sys,
                              int32_t n_home, const double *S, const double *S_inv, const int64_t *i_off, int32_t n_sys, double symprec,
                              int32_t *img_base, int32_t *img_mask, int64_t i_size, int32_t *status, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_home >= 1 && n_atoms >= 1 && n_atoms < PH_MAX && i_size >= 1, "snet_ph_images: bad shape");
  SNET_REQUIRE(symprec >= 0.0, "snet_ph_images: symprec must not be negative");
  SNET_REQUIRE(pos && sc_ptr && m_ptr && home_sys && S && S_inv && i_off && img_base && img_mask && status, "snet_ph_images: null argument");
  ph_images_kernel<<<(unsigned)n_home, PH_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      pos, n_atoms, sc_ptr, m_ptr, home_sys, n_home, S, S_inv, i_off, n_sys, symprec, img_base, img_mask, i_size, status);
  SNET_CHECK_LAUNCH("snet_ph_images");
  return 0;
}

extern "C" int snet_ph_dynmat(const double *phi, const int64_t *p_off, int64_t p_size, const double *pos, int64_t n_atoms,
                              const int32_t *sc_ptr, const int32_t *m_ptr, const double *w, int32_t n_home, const double *S,
                              const int32_t *img_base, const int32_t *img_mask, const int64_t *i_off, int64_t i_size, const double *q_cart,
                              const int32_t *q_sys, const int32_t *q_ptr, int32_t n_q, const int64_t *d_off, int32_t n_sys, int32_t max_m,
                              int32_t *status, double *R, double *D, int64_t d_size, double *hermiticity, void *stream) {
  SNET_REQUIRE(n_sys >= 1 && n_home >= 1 && n_q >= 1 && n_atoms >= 1 && n_atoms < PH_MAX && p_size >= 1 && i_size >= 1 && d_size >= 1,
               "snet_ph_dynmat: bad shape");
  SNET_REQUIRE(max_m >= 1 && max_m <= 65535, "snet_ph_dynmat: at most 65535 atoms in the primitive cell");
  SNET_REQUIRE(phi && p_off && pos && sc_ptr && m_ptr && w && S && img_base && img_mask && i_off && q_cart && q_sys && q_ptr && d_off &&
                   status && R && D && hermiticity && R != D,
               "snet_ph_dynmat: null or aliased argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  ph_dynmat_rows_kernel<<<dim3((unsigned)n_q, (unsigned)max_m), PH_THREADS, 0, st>>>(
      phi, p_off, p_size, pos, n_atoms, sc_ptr, m_ptr, w, n_home, S, img_base, img_mask, i_off, i_size, q_cart, q_sys, q_ptr, n_q, d_off,
      n_sys, status, R, d_size);
  SNET_CHECK_LAUNCH("snet_ph_dynmat (rows)");
  ph_dynmat_sym_kernel<<<(unsigned)n_q, PH_THREADS, 0, st>>>(p_off, p_size, n_atoms, sc_ptr, m_ptr, n_home, i_off, i_size, q_sys, q_ptr,
                                                             n_q, d_off, n_sys, R, D, d_size, hermiticity);
  SNET_CHECK_LAUNCH("snet_ph_dynmat (symmetrise)");
  return 0;
}
