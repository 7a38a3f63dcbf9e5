// DFT-D3 dispersion on gfx950.  Own HIP implementation of what the reference's CUDA library
// computes (sevenn/pair_e3gnn/pair_d3_for_ase.cu: coordination numbers :1004-1057, C6 interpolation and dC6/dCN
// :765-845, two-body energy / forces / virial for zero and Becke-Johnson damping :1263-1694, CN-gradient forces
// :1797-1961), behind a C-ABI shaped like its ten pair_* functions (:2034-2082).
//
// Layout instead of the reference's scheme (one thread per UNORDERED pair looping over all lattice translations,
// float arithmetic, float atomics into double accumulators, managed pointer-to-pointer tables):
//   * one workgroup per atom i; its 256 threads stride over the flattened (j, translation) list of ROW i -- every
//     ordered pair is visited once from each side, so each atom's energy share, force, dE/dCN and virial share are
//     plain block reductions in a fixed order: no atomics, bit-reproducible;
//   * fp64 throughout (the reference's known answers carry float32 summation error of a few 1e-5 relative on lattice
//     sums of 1e5 translations; MI355X vector fp64 runs at half the fp32 rate);
//   * flat device tables: wrapped positions [n,3] (bohr), translations [T,3], per-pair C6 and dC6/dCN_i [n,n], the
//     reference-C6 grid of the elements present [nt,nt,5,5,3];
//   * batches: the grid covers the atoms of B systems; workgroup i reads its system's D3Sys (atom range, the offsets,
//     counts and zero-translation indices of its two translation lists, t_chunks) and offsets every per-atom pointer to
//     that system's first atom, so its traversal is the single-system one: a batch equals B single calls bit for bit
//     (snet_d3_compute is the B = 1 case of the same routine).
// Units inside: bohr / hartree (0.52917726 A, 27.21138505 eV); outputs eV, eV/A, eV/A^3.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "snet_common.h"

namespace {
using namespace snet;

constexpr double AU_TO_ANG = 0.52917726, AU_TO_EV = 27.21138505, K1 = 16.0, K3 = -4.0;
constexpr int NTH = 256, MAXREF = 5;

struct Func {
  double s6, a1, s8, a2, alp6, alp8;
  int damping;  // 0 zero, 1 Becke-Johnson
};

// one system of a batch: atoms [a0, a0 + n), vdW translations [tv0, tv0 + Tv) and CN translations [tc0, tc0 + Tc) of the
// concatenated lists (zv, zc: the index of the zero translation within each), t_chunks of d3_pair_kernel
struct D3Sys {
  int64_t a0, tv0, tc0;
  int32_t n, Tv, zv, Tc, zc, t_chunks;
};

__device__ __forceinline__ double block_sum(double v, double *sh) {
  // fixed-order tree over the workgroup's 256 threads (deterministic)
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// CN_i = sum over (j, tau) != (i, 0) with r^2 <= cn_cut of 1 / (1 + exp(-K1 ((rcov_i + rcov_j) / r - 1)))
__global__ __launch_bounds__(NTH) void d3_cn_kernel(const D3Sys *__restrict__ sys, const int32_t *__restrict__ sys_of,
                                                    const double *__restrict__ x, const double *__restrict__ tau,
                                                    const double *__restrict__ rcov, double cn_cut, double *__restrict__ cn) {
  __shared__ double sh[4];
  const D3Sys S = sys[sys_of[blockIdx.x]];
  const int i = (int)(blockIdx.x - S.a0), n = S.n, T = S.Tc, t_zero = S.zc;
  x += 3 * S.a0; tau += 3 * S.tc0; rcov += S.a0; cn += S.a0;
  const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2], rci = rcov[i];
  double acc = 0.0;
  const int64_t total = (int64_t)n * T;
  for (int64_t k = threadIdx.x; k < total; k += NTH) {
    const int j = (int)(k / T), t = (int)(k - (int64_t)j * T);
    if (j == i && t == t_zero) continue;
    const double dx = x[3 * j] - xi + tau[3 * t], dy = x[3 * j + 1] - yi + tau[3 * t + 1], dz = x[3 * j + 2] - zi + tau[3 * t + 2];
    const double r2 = dx * dx + dy * dy + dz * dz;
    if (r2 <= cn_cut) acc += 1.0 / (1.0 + exp(-K1 * ((rci + rcov[j]) / sqrt(r2) - 1.0)));
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) cn[i] = acc;
}

// C6_ij(CN_i, CN_j) and dC6_ij / dCN_i: Gaussian-weighted average over the reference grid (L = exp(K3 ((CN_i - a)^2 + (CN_j - b)^2))).
// Evaluated where it is used (d3_pair_kernel), once per (i, j, chunk of images): no [n, n] tables in memory (the reference keeps
// n (n + 1) / 2 fp32 entries, pair_d3.cu; the 16 n^2 bytes of fp64 tables this file kept until round 4 would have been 160 GB at 100 k atoms)
__device__ __forceinline__ void d3_c6(double cni, double cnj, const double *__restrict__ g, int mxi, int mxj, double &c6, double &dc6) {
  double num = 0.0, den = 0.0, dnum = 0.0, dden = 0.0, rmin = 1e300, cmin = 0.0;
  for (int a = 0; a < mxi; ++a)
    for (int b = 0; b < mxj; ++b) {
      const double *e = g + (a * MAXREF + b) * 3;
      if (e[0] <= 0.0) continue;
      const double rr = (e[1] - cni) * (e[1] - cni) + (e[2] - cnj) * (e[2] - cnj);
      if (rr < rmin) { rmin = rr; cmin = e[0]; }
      const double w = exp(K3 * rr);
      num += e[0] * w;
      den += w;
      const double dw = w * 2.0 * K3 * (cni - e[1]);
      dnum += e[0] * dw;
      dden += dw;
    }
  if (den > 1e-99) {
    c6 = num / den;
    dc6 = (dnum - c6 * dden) / den;
  } else {  // all weights underflow: the nearest reference value, no CN dependence (reference :833-837)
    c6 = cmin;
    dc6 = 0.0;
  }
}

// phi(r) with E_pair = -C6 phi, and phi'(r)
__device__ __forceinline__ void d3_phi(const Func &F, double r2, double r42, double r0, double &phi, double &dphi) {
  const double r = sqrt(r2);
  if (F.damping == 1) {
    const double R0 = F.a1 * sqrt(3.0 * r42) + F.a2, R2 = R0 * R0, R6 = R2 * R2 * R2, R8 = R6 * R2;
    const double r6 = r2 * r2 * r2, r8 = r6 * r2;
    const double t6 = 1.0 / (r6 + R6), t8 = 1.0 / (r8 + R8);
    phi = F.s6 * t6 + 3.0 * F.s8 * r42 * t8;
    dphi = -(6.0 * F.s6 * r6 * t6 * t6 + 24.0 * F.s8 * r42 * r8 * t8 * t8) / r;
  } else {
    const double ir = 1.0 / r, ir2 = ir * ir, ir6 = ir2 * ir2 * ir2, ir8 = ir6 * ir2;
    const double t6 = pow(F.a1 * r0 * ir, F.alp6), t8 = pow(F.a2 * r0 * ir, F.alp8);
    const double f6 = 1.0 / (1.0 + 6.0 * t6), f8 = 1.0 / (1.0 + 6.0 * t8);
    phi = F.s6 * f6 * ir6 + 3.0 * F.s8 * r42 * f8 * ir8;
    const double df6 = 6.0 * F.alp6 * t6 * f6 * f6 * ir, df8 = 6.0 * F.alp8 * t8 * f8 * f8 * ir;
    dphi = F.s6 * ir6 * (df6 - 6.0 * f6 * ir) + 3.0 * F.s8 * r42 * ir8 * (df8 - 8.0 * f8 * ir);
  }
}

// row i of the two-body sum at fixed C6: e_i = -1/2 sum C6 phi; f_i = -sum C6 phi' d / r; dE/dCN_i = -sum phi dC6_ij/dCN_i;
// strain derivative share s_i[ab] = -1/2 sum C6 phi' d_a d_b / r
__global__ __launch_bounds__(NTH) void d3_pair_kernel(const D3Sys *__restrict__ sys, const int32_t *__restrict__ sys_of,
                                                      const double *__restrict__ x, const double *__restrict__ tau,
                                                      const double *__restrict__ r2r4, const double *__restrict__ r0ab,
                                                      const int32_t *__restrict__ type, int nt, const double *__restrict__ cn,
                                                      const int32_t *__restrict__ mxc, const double *__restrict__ ref,
                                                      double vdw_cut, Func F,
                                                      double *__restrict__ e_atom, double *__restrict__ f, double *__restrict__ dedcn,
                                                      double *__restrict__ s_atom) {
  __shared__ double sh[4];
  const D3Sys S = sys[sys_of[blockIdx.x]];
  const int i = (int)(blockIdx.x - S.a0), n = S.n, T = S.Tv, t_zero = S.zv, t_chunks = S.t_chunks;
  x += 3 * S.a0; tau += 3 * S.tv0; r2r4 += S.a0; type += S.a0; cn += S.a0;
  e_atom += S.a0; f += 3 * S.a0; dedcn += S.a0; s_atom += 6 * S.a0;
  const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2], q_i = r2r4[i];
  double e = 0.0, fx = 0.0, fy = 0.0, fz = 0.0, dc = 0.0, s[6] = {0, 0, 0, 0, 0, 0};
  // work item = (atom j, chunk of the T images): C6_ij is evaluated once per item; t_chunks = 1 for large n, more for small cells whose
  // many images would otherwise leave most of the block's threads without an atom j
  const int ti = type[i], ch = (T + t_chunks - 1) / t_chunks;
  const double cni = cn[i];
  const int64_t total = (int64_t)n * t_chunks;
  for (int64_t k = threadIdx.x; k < total; k += NTH) {
    const int j = (int)(k / t_chunks), t_beg = (int)(k - (int64_t)j * t_chunks) * ch, t_end = min(T, t_beg + ch);
    const int tj = type[j];
    const double xj = x[3 * j] - xi, yj = x[3 * j + 1] - yi, zj = x[3 * j + 2] - zi;
    const double r42 = q_i * r2r4[j], r0 = r0ab[(size_t)ti * nt + tj];
    double c = 0.0, dcv = 0.0;
    bool have_c6 = false;
    for (int t = t_beg; t < t_end; ++t) {
      if (j == i && t == t_zero) continue;
      const double dx = xj + tau[3 * t], dy = yj + tau[3 * t + 1], dz = zj + tau[3 * t + 2];
      const double r2 = dx * dx + dy * dy + dz * dz;
      if (r2 > vdw_cut) continue;
      if (!have_c6) {
        d3_c6(cni, cn[j], ref + ((size_t)ti * nt + tj) * (MAXREF * MAXREF * 3), mxc[ti], mxc[tj], c, dcv);
        have_c6 = true;
      }
      double phi, dphi;
      d3_phi(F, r2, r42, r0, phi, dphi);
      e -= 0.5 * c * phi;
      dc -= phi * dcv;
      const double g = c * dphi / sqrt(r2);   // C6 phi' / r
      if (j != i) { fx -= g * dx; fy -= g * dy; fz -= g * dz; }
      s[0] -= 0.5 * g * dx * dx; s[1] -= 0.5 * g * dy * dy; s[2] -= 0.5 * g * dz * dz;
      s[3] -= 0.5 * g * dx * dy; s[4] -= 0.5 * g * dx * dz; s[5] -= 0.5 * g * dy * dz;
    }
  }
  e = block_sum(e, sh); fx = block_sum(fx, sh); fy = block_sum(fy, sh); fz = block_sum(fz, sh); dc = block_sum(dc, sh);
  for (int q = 0; q < 6; ++q) s[q] = block_sum(s[q], sh);
  if (threadIdx.x == 0) {
    e_atom[i] = e; f[3 * i] = fx; f[3 * i + 1] = fy; f[3 * i + 2] = fz; dedcn[i] = dc;
    for (int q = 0; q < 6; ++q) s_atom[6 * i + q] = s[q];
  }
}

// CN-gradient part: f_i += sum (dE/dCN_i + dE/dCN_j) cnt'(r) d / r ;  s_i[ab] += sum dE/dCN_i cnt'(r) d_a d_b / r
__global__ __launch_bounds__(NTH) void d3_cn_force_kernel(const D3Sys *__restrict__ sys, const int32_t *__restrict__ sys_of,
                                                          const double *__restrict__ x, const double *__restrict__ tau,
                                                          const double *__restrict__ rcov, double cn_cut,
                                                          const double *__restrict__ dedcn, double *__restrict__ f,
                                                          double *__restrict__ s_atom) {
  __shared__ double sh[4];
  const D3Sys S = sys[sys_of[blockIdx.x]];
  const int i = (int)(blockIdx.x - S.a0), n = S.n, T = S.Tc, t_zero = S.zc;
  x += 3 * S.a0; tau += 3 * S.tc0; rcov += S.a0; dedcn += S.a0; f += 3 * S.a0; s_atom += 6 * S.a0;
  const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2], rci = rcov[i], di = dedcn[i];
  double fx = 0.0, fy = 0.0, fz = 0.0, s[6] = {0, 0, 0, 0, 0, 0};
  const int64_t total = (int64_t)n * T;
  for (int64_t k = threadIdx.x; k < total; k += NTH) {
    const int j = (int)(k / T), t = (int)(k - (int64_t)j * T);
    if (j == i && t == t_zero) continue;
    const double dx = x[3 * j] - xi + tau[3 * t], dy = x[3 * j + 1] - yi + tau[3 * t + 1], dz = x[3 * j + 2] - zi + tau[3 * t + 2];
    const double r2 = dx * dx + dy * dy + dz * dz;
    if (r2 > cn_cut) continue;
    const double r = sqrt(r2), rc = rci + rcov[j];
    const double ex = exp(-K1 * (rc / r - 1.0));
    const double dcnt = -K1 * rc * ex / (r2 * (1.0 + ex) * (1.0 + ex));   // d cnt / d r
    const double gi = di * dcnt / r;
    if (j != i) {
      const double g = (di + dedcn[j]) * dcnt / r;
      fx += g * dx; fy += g * dy; fz += g * dz;
    }
    s[0] += gi * dx * dx; s[1] += gi * dy * dy; s[2] += gi * dz * dz;
    s[3] += gi * dx * dy; s[4] += gi * dx * dz; s[5] += gi * dy * dz;
  }
  fx = block_sum(fx, sh); fy = block_sum(fy, sh); fz = block_sum(fz, sh);
  for (int q = 0; q < 6; ++q) s[q] = block_sum(s[q], sh);
  if (threadIdx.x == 0) {
    f[3 * i] += fx; f[3 * i + 1] += fy; f[3 * i + 2] += fz;
    for (int q = 0; q < 6; ++q) s_atom[6 * i + q] += s[q];
  }
}

// ---- device-resident evaluation (snet_d3_plan / snet_d3_compute_device): what d3_run does on the host per call -- the molecule
// box, the cell in bohr with its inverse, both translation lists, the wrap, the per-system sums -- as four small kernels around
// the three above.  They are plain IEEE fp64 with the operations of the host code in its order, and floating-point contraction
// is switched off in each (the x86 host build has no fused multiply-add to contract into), so they reproduce the host's bits.

// what the plan fixes per system: the atom range, the slots and capacities of its two translation lists, the box rule
struct D3PlanSys {
  int64_t a0, tv0, tc0;
  int32_t n, cap_v, cap_c, box, pbc[3], pad;
  double cell[9];   // the plan's cell (A): read where the call passes no cells
};
// what d3_prepare_kernel derives per system and call: the cell in bohr, its inverse, the volume (A^3), the status word
struct D3Geo {
  double a[9], inv[9], vol;
  int32_t status, pad;
};

// repetition counts of `translations` below for one cutoff radius rc: |n_k| <= int(rc / height_k) + 1 along periodic axes.
// false: a count that is not finite or beyond 1e5 (a cell that has collapsed along that axis)
__host__ __device__ inline bool d3_reps(const double *a, const int32_t *pbc, double rc, int rep[3]) {
#pragma clang fp contract(off)
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double *u = a + 3 * ((k + 1) % 3), *v = a + 3 * ((k + 2) % 3), *w = a + 3 * k;
    const double cp[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double h = fabs((cp[0] * w[0] + cp[1] * w[1] + cp[2] * w[2]) / sqrt(cp[0] * cp[0] + cp[1] * cp[1] + cp[2] * cp[2]));
    rep[k] = 0;
    if (pbc[k]) {
      const double q = fabs(rc / h);
      if (q < 1e5) rep[k] = (int)q + 1;   // (a NaN fails the comparison)
      else ok = false;
    }
  }
  return ok;
}
__host__ __device__ inline int64_t d3_rep_count(const int rep[3]) {
  return (int64_t)(2 * rep[0] + 1) * (2 * rep[1] + 1) * (2 * rep[2] + 1);
}

// translation t of the (p, q, r) loop nest of `translations` below, into tau[3 t ..]
__device__ __forceinline__ void d3_put_translation(const double *a, const int rep[3], int64_t t, double *tau) {
#pragma clang fp contract(off)
  const int n1 = 2 * rep[1] + 1, n2 = 2 * rep[2] + 1;
  const int r = (int)(t % n2) - rep[2], q = (int)((t / n2) % n1) - rep[1], p = (int)(t / ((int64_t)n1 * n2)) - rep[0];
  for (int c = 0; c < 3; ++c) tau[3 * t + c] = p * a[c] + q * a[3 + c] + r * a[6 + c];
}

// one workgroup per system: its cell (the molecule box from the positions' extent where the plan says so), D3Geo, both
// translation lists into the system's slots, D3Sys.  A system whose cell is not finite or singular, or whose lists would not
// fit their capacity, gets status 1 and empty lists: the three kernels above then loop over nothing for its atoms.
__global__ __launch_bounds__(NTH) void d3_prepare_kernel(const D3PlanSys *__restrict__ plan, const double *__restrict__ pos,
                                                         const double *__restrict__ cells, double box_pad, double rc_v, double rc_c,
                                                         D3Sys *__restrict__ sys, D3Geo *__restrict__ geo, double *__restrict__ tv,
                                                         double *__restrict__ tc) {
#pragma clang fp contract(off)
  __shared__ double sh[NTH / 64][6];
  const int s = blockIdx.x, tid = threadIdx.x;
  const D3PlanSys P = plan[s];
  double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int32_t pbc[3] = {1, 1, 1};
  if (P.box) {   // (uniform over the workgroup) extent + box_pad + 1 A along each axis, periodic
    double m[6] = {INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY};   // min x,y,z | min of -x,-y,-z
    for (int i = tid; i < P.n; i += NTH)
      for (int k = 0; k < 3; ++k) {
        const double v = pos[3 * (P.a0 + i) + k];
        m[k] = fmin(m[k], v);
        m[3 + k] = fmin(m[3 + k], -v);
      }
    for (int k = 0; k < 6; ++k) {
      for (int o = 32; o > 0; o >>= 1) m[k] = fmin(m[k], __shfl_xor(m[k], o, 64));
      if ((tid & 63) == 0) sh[tid >> 6][k] = m[k];
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) {
      const double lo = fmin(fmin(sh[0][k], sh[1][k]), fmin(sh[2][k], sh[3][k]));
      const double hi = -fmin(fmin(sh[0][3 + k], sh[1][3 + k]), fmin(sh[2][3 + k], sh[3][3 + k]));
      c[4 * k] = hi - lo + box_pad + 1.0;
    }
  } else {
    const double *src = cells ? cells + 9 * (int64_t)s : P.cell;
    for (int k = 0; k < 9; ++k) c[k] = src[k];
    for (int k = 0; k < 3; ++k) pbc[k] = P.pbc[k];
  }
  D3Geo G;
  double *a = G.a;
  bool ok = true;
  for (int k = 0; k < 9; ++k) {
    a[k] = c[k] / AU_TO_ANG;
    ok = ok && (a[k] - a[k] == 0.0);
  }
  const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
  ok = ok && fabs(det) > 1e-12;
  const double inv[9] = {(a[4] * a[8] - a[5] * a[7]) / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                         (a[5] * a[6] - a[3] * a[8]) / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                         (a[3] * a[7] - a[4] * a[6]) / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det};
  for (int k = 0; k < 9; ++k) G.inv[k] = inv[k];
  G.vol = fabs(det) * AU_TO_ANG * AU_TO_ANG * AU_TO_ANG;
  int rv[3], rc[3];
  ok = d3_reps(a, pbc, rc_v, rv) && ok;
  ok = d3_reps(a, pbc, rc_c, rc) && ok;
  int64_t Tv = 0, Tc = 0;
  if (ok) {
    Tv = d3_rep_count(rv);
    Tc = d3_rep_count(rc);
    ok = Tv <= P.cap_v && Tc <= P.cap_c;
  }
  if (!ok) Tv = Tc = 0;
  for (int64_t t = tid; t < Tv; t += NTH) d3_put_translation(a, rv, t, tv + 3 * P.tv0);
  for (int64_t t = tid; t < Tc; t += NTH) d3_put_translation(a, rc, t, tc + 3 * P.tc0);
  if (tid == 0) {
    D3Sys S;
    S.a0 = P.a0, S.tv0 = P.tv0, S.tc0 = P.tc0, S.n = P.n;
    S.Tv = (int32_t)Tv, S.Tc = (int32_t)Tc;
    S.zv = ok ? (rv[0] * (2 * rv[1] + 1) + rv[1]) * (2 * rv[2] + 1) + rv[2] : 0;
    S.zc = ok ? (rc[0] * (2 * rc[1] + 1) + rc[1]) * (2 * rc[2] + 1) + rc[2] : 0;
    const int64_t want = (4 * NTH + (int64_t)P.n - 1) / P.n;   // >= 4 work items per thread where the images allow it (d3_run)
    const int64_t have = Tv < want ? Tv : want;
    S.t_chunks = (int32_t)(have > 1 ? have : 1);
    sys[s] = S;
    G.status = ok ? 0 : 1;
    G.pad = 0;
    geo[s] = G;
  }
}

// one thread per atom: the position in bohr wrapped into its system's cell (d3_run's loop; load_atom_info, :1170-1219)
__global__ __launch_bounds__(NTH) void d3_wrap_kernel(const int32_t *__restrict__ sys_of, const D3Geo *__restrict__ geo,
                                                      const double *__restrict__ pos, int n_atoms, double *__restrict__ x) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * NTH + threadIdx.x;
  if (i >= n_atoms) return;
  const D3Geo *G = geo + sys_of[i];
  const double *p = pos + 3 * i, *a = G->a, *inv = G->inv;
  if (G->status != 0) {   // (nothing reads a flagged system's coordinates: its lists are empty)
    x[3 * i] = x[3 * i + 1] = x[3 * i + 2] = 0.0;
    return;
  }
  double fr[3];
  for (int c = 0; c < 3; ++c) {
    fr[c] = 0.0;
    for (int k = 0; k < 3; ++k) fr[c] += p[k] / AU_TO_ANG * inv[3 * k + c];
    fr[c] -= floor(fr[c]);
  }
  for (int c = 0; c < 3; ++c) x[3 * i + c] = fr[0] * a[c] + fr[1] * a[3 + c] + fr[2] * a[6 + c];
}

// one workgroup per system: the energy and the six strain shares summed sequentially in atom order (one thread per sum, as the
// host loop of d3_run), scaled to eV; the virial in the engine's convention (xx,yy,zz,xy,yz,zx; stress = -virial / V) from the
// strain derivative in this file's order (xx,yy,zz,xy,xz,yz); the forces scaled to eV/A.  NaN for a flagged system.
__global__ __launch_bounds__(NTH) void d3_reduce_kernel(const D3Sys *__restrict__ sys, const D3Geo *__restrict__ geo,
                                                        const double *__restrict__ e_atom, const double *__restrict__ s_atom,
                                                        const double *__restrict__ f, const double *__restrict__ cn,
                                                        double *__restrict__ energy, double *__restrict__ forces,
                                                        double *__restrict__ virial, double *__restrict__ cn_out,
                                                        double *__restrict__ volume, int32_t *__restrict__ status) {
#pragma clang fp contract(off)
  const int s = blockIdx.x, tid = threadIdx.x;
  const D3Sys S = sys[s];
  const bool bad = geo[s].status != 0;
  if (tid < 7) {
    const double *src = tid == 0 ? e_atom + S.a0 : s_atom + 6 * S.a0 + (tid - 1);
    const int stride = tid == 0 ? 1 : 6;
    double acc = 0.0;
    for (int i = 0; i < S.n; ++i) acc += src[(int64_t)i * stride];
    if (tid == 0) {
      energy[s] = bad ? NAN : acc * AU_TO_EV;
    } else {
      const int slot[6] = {0, 1, 2, 3, 5, 4};   // xx,yy,zz,xy,xz,yz -> xx,yy,zz,xy,yz,zx
      virial[6 * (int64_t)s + slot[tid - 1]] = bad ? NAN : -(acc * AU_TO_EV);
    }
  }
  for (int k = tid; k < 3 * S.n; k += NTH) forces[3 * S.a0 + k] = bad ? NAN : f[3 * S.a0 + k] * (AU_TO_EV / AU_TO_ANG);
  if (cn_out)
    for (int k = tid; k < S.n; k += NTH) cn_out[S.a0 + k] = cn[S.a0 + k];
  if (tid == 0) {
    if (volume) volume[s] = geo[s].vol;
    if (status) status[s] = geo[s].status;
  }
}

template <class T>
struct Dev {
  T *p = nullptr;
  size_t cap = 0;
  bool ensure(size_t n) {
    if (n <= cap) return true;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return false;
    cap = n ? n : 1;
    return true;
  }
  bool put(const std::vector<T> &h, hipStream_t st) {
    return ensure(h.size()) && (h.empty() || hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st) == hipSuccess);
  }
  ~Dev() { if (p) (void)hipFree(p); }
};

}  // namespace

struct snet_d3 {
  // published tables (from the parameter blob)
  std::vector<double> r0ab, r2r4, rcov;       // [94*94] (A), [94], [94] (bohr)
  std::vector<double> c6ref;                   // [95][95][5][5][3]
  std::vector<int> mxc;                        // [95]
  bool have_tables = false;
  Func func{1.0, 0.4289, 0.7875, 4.4407, 14.0, 16.0, 1};
  bool have_func = false;
  double vdw_cut = 9000.0, cn_cut = 1600.0;    // bohr^2
  std::vector<int32_t> z;
  std::vector<double> pos;                     // A
  double cell[9] = {0};
  int pbc[3] = {0, 0, 0};
  bool have_cell = false;
  // results
  double energy = 0.0, stress[9] = {0};
  std::vector<double> forces, cn;
  // device buffers: the packed inputs (fp64 tables, int32 tables, per-system records) and the work array [e | s | f | cn | dE/dCN]
  Dev<double> d_in, d_work;
  Dev<int32_t> d_int;
  Dev<D3Sys> d_sys;
  // the plan of snet_d3_plan, with device buffers of its own (snet_d3_compute(_batch) between two planned calls disturbs nothing):
  // p_x = x [3N] | tv [3 cap_v] | tc [3 cap_c], written by the kernels of each call; p_tab = rcov [N] | r2r4 [N] | r0 [nt nt] |
  // ref [nt nt 5 5 3] and p_int = type [N] | sys_of [N] | mxc [nt], uploaded once; p_work as d_work
  struct Plan {
    bool ready = false;
    int32_t B = 0, N = 0, nt = 0;
    int64_t cap_v = 0, cap_c = 0;
    Dev<double> p_x, p_tab, p_work;
    Dev<int32_t> p_int;
    Dev<D3PlanSys> p_plan;
    Dev<D3Sys> p_sys;
    Dev<D3Geo> p_geo;
  } plan;
};

extern "C" {

int snet_d3_create(snet_d3 **out) {
  SNET_REQUIRE(out != nullptr, "snet_d3_create: null argument");
  *out = new snet_d3;
  return 0;
}
void snet_d3_destroy(snet_d3 *d) { delete d; }

int snet_d3_set_tables(snet_d3 *d, const double *r0ab, const double *c6ab, int64_t n_c6, const double *r2r4, const double *rcov) {
  SNET_REQUIRE(d && r0ab && c6ab && r2r4 && rcov && n_c6 > 0, "snet_d3_set_tables: null argument");
  d->r0ab.assign(r0ab, r0ab + 94 * 94);
  d->r2r4.assign(r2r4, r2r4 + 94);
  d->rcov.assign(rcov, rcov + 94);
  d->c6ref.assign((size_t)95 * 95 * MAXREF * MAXREF * 3, 0.0);
  d->mxc.assign(95, 0);
  auto at = [&](int zi, int zj, int a, int b) { return &d->c6ref[((((size_t)zi * 95 + zj) * MAXREF + a) * MAXREF + b) * 3]; };
  for (int64_t k = 0; k < n_c6; ++k) {   // row: C6, Z_i + 100 ref_i, Z_j + 100 ref_j, CN_i, CN_j (reference :361-391)
    const double *row = c6ab + 5 * k;
    const int a1 = (int)row[1], a2 = (int)row[2];
    const int zi = (a1 - 1) % 100 + 1, ri = (a1 - 1) / 100, zj = (a2 - 1) % 100 + 1, rj = (a2 - 1) / 100;
    SNET_REQUIRE(zi >= 1 && zi <= 94 && zj >= 1 && zj <= 94 && ri < MAXREF && rj < MAXREF, "snet_d3_set_tables: bad C6 table row");
    double *p = at(zi, zj, ri, rj), *q = at(zj, zi, rj, ri);
    p[0] = row[0]; p[1] = row[3]; p[2] = row[4];
    q[0] = row[0]; q[1] = row[4]; q[2] = row[3];
    d->mxc[zi] = std::max(d->mxc[zi], ri + 1);
    d->mxc[zj] = std::max(d->mxc[zj], rj + 1);
  }
  d->have_tables = true;
  d->plan.ready = false;   // (a plan holds slices of the tables)
  return 0;
}

int snet_d3_settings(snet_d3 *d, double vdw_cutoff_au2, double cn_cutoff_au2, int32_t damping, const double *func5) {
  SNET_REQUIRE(d && func5, "snet_d3_settings: null argument");
  SNET_REQUIRE(damping == 0 || damping == 1, "snet_d3_settings: damping must be 0 (damp_zero) or 1 (damp_bj); the reference's "
                                               "damp_zerom / damp_bjm compute nothing either (pair_d3_for_ase.cu:1783-1784)");
  SNET_REQUIRE(vdw_cutoff_au2 > 0 && cn_cutoff_au2 > 0, "snet_d3_settings: cutoffs (bohr^2) must be positive");
  d->vdw_cut = vdw_cutoff_au2;
  d->cn_cut = cn_cutoff_au2;
  // func5 = (s6, rs6, s18, rs18, alp) of the functional; a1 = rs6, a2 = rs8 = rs18, s8 = s18, alp8 = alp + 2 (:608-628)
  d->func = Func{func5[0], func5[1], func5[2], func5[3], func5[4], func5[4] + 2.0, damping};
  d->have_func = true;
  d->plan.ready = false;   // (a plan's capacities come from the cutoffs)
  return 0;
}

int snet_d3_set_atoms(snet_d3 *d, int32_t n, const int32_t *atomic_numbers, const double *positions) {
  SNET_REQUIRE(d && n > 0 && atomic_numbers && positions, "snet_d3_set_atoms: need n > 0 atoms");
  for (int i = 0; i < n; ++i)
    SNET_REQUIRE(atomic_numbers[i] >= 1 && atomic_numbers[i] <= 94, "snet_d3_set_atoms: D3 parameters exist for Z = 1 .. 94");
  d->z.assign(atomic_numbers, atomic_numbers + n);
  d->pos.assign(positions, positions + 3 * (size_t)n);
  return 0;
}

int snet_d3_set_cell(snet_d3 *d, const double *cell9, const int32_t *pbc3) {
  SNET_REQUIRE(d && cell9 && pbc3, "snet_d3_set_cell: null argument");
  std::memcpy(d->cell, cell9, sizeof(d->cell));
  for (int k = 0; k < 3; ++k) d->pbc[k] = pbc3[k] != 0;
  d->have_cell = true;
  return 0;
}

// appends the lattice translations within reach of r2_cut to `tau`; t_zero: the index of (0, 0, 0) among those appended
static void translations(const double a[9], const int pbc[3], double r2_cut, std::vector<double> &tau, int &t_zero) {
  // |n_k| <= int(r_cut / height_k) + 1 along periodic axes (set_lattice_repetition_criteria, :979-1001)
  const double rc = std::sqrt(r2_cut);
  int rep[3];
  for (int k = 0; k < 3; ++k) {
    const double *u = a + 3 * ((k + 1) % 3), *v = a + 3 * ((k + 2) % 3), *w = a + 3 * k;
    const double cp[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double h = std::fabs((cp[0] * w[0] + cp[1] * w[1] + cp[2] * w[2]) / std::sqrt(cp[0] * cp[0] + cp[1] * cp[1] + cp[2] * cp[2]));
    rep[k] = pbc[k] ? (int)std::fabs(rc / h) + 1 : 0;
  }
  const size_t base = tau.size();
  t_zero = -1;
  for (int p = -rep[0]; p <= rep[0]; ++p)
    for (int q = -rep[1]; q <= rep[1]; ++q)
      for (int r = -rep[2]; r <= rep[2]; ++r) {
        if (p == 0 && q == 0 && r == 0) t_zero = (int)((tau.size() - base) / 3);
        for (int c = 0; c < 3; ++c) tau.push_back(p * a[c] + q * a[3 + c] + r * a[6 + c]);
      }
}

// B systems [atom_ptr[s], atom_ptr[s+1]) in one set of three launches.  Host work per system as for one: wrap into the cell,
// build both translation lists, and -- after one readback -- sum the per-atom energy and virial shares in atom order.
// Outputs: energy[B] (eV), forces[3N] (eV/A), stress[9B] (dE/dstrain / V, eV/A^3), cn[N].  `batch` names the system in errors.
static int d3_run(snet_d3 *d, int32_t B, const int64_t *atom_ptr, const int32_t *z, const double *pos, const double *cells,
                  const int32_t *pbc3, double *energy, double *forces, double *stress, double *cn_out, hipStream_t st,
                  const char *who, bool batch) {
  auto sys_msg = [&](int s, const std::string &m) {
    return std::string(who) + ": " + (batch ? "system " + std::to_string(s) + ": " : std::string()) + m;
  };
  SNET_REQUIRE(d->have_tables && d->have_func, std::string(who) + ": tables and settings must be set first");
  SNET_REQUIRE(B >= 1 && atom_ptr[0] == 0, std::string(who) + ": need n_sys >= 1 and atom_ptr[0] == 0");
  for (int s = 0; s < B; ++s) SNET_REQUIRE(atom_ptr[s + 1] > atom_ptr[s], sys_msg(s, "no atoms (atom_ptr must increase)"));
  SNET_REQUIRE(atom_ptr[B] <= (int64_t)INT32_MAX, std::string(who) + ": more than 2^31 - 1 atoms in total");
  const int N = (int)atom_ptr[B];
  for (int s = 0; s < B; ++s)
    for (int64_t i = atom_ptr[s]; i < atom_ptr[s + 1]; ++i)
      SNET_REQUIRE(z[i] >= 1 && z[i] <= 94, sys_msg(s, "Z = " + std::to_string(z[i]) + ": D3 parameters exist for Z = 1 .. 94"));
  std::vector<double> x(3 * (size_t)N), tv, tc, vol(B);
  std::vector<D3Sys> sys(B);
  std::vector<int32_t> sys_of(N);
  for (int s = 0; s < B; ++s) {
    const int64_t a0 = atom_ptr[s];
    const int n = (int)(atom_ptr[s + 1] - a0);
    double a[9];
    for (int k = 0; k < 9; ++k) a[k] = cells[9 * (size_t)s + k] / AU_TO_ANG;
    const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
    SNET_REQUIRE(std::fabs(det) > 1e-12, sys_msg(s, "singular cell (give molecules a box: the reference's calculator does, calculator.py:533-548)"));
    double inv[9] = {(a[4] * a[8] - a[5] * a[7]) / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
                     (a[5] * a[6] - a[3] * a[8]) / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
                     (a[3] * a[7] - a[4] * a[6]) / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det};
    // wrap into the cell (load_atom_info, :1170-1219): fractional = x inv(cell), rows of `a` are the lattice vectors
    for (int i = 0; i < n; ++i) {
      const double *p = pos + 3 * (a0 + i);
      double fr[3];
      for (int c = 0; c < 3; ++c) {
        fr[c] = 0.0;
        for (int k = 0; k < 3; ++k) fr[c] += p[k] / AU_TO_ANG * inv[3 * k + c];
        fr[c] -= std::floor(fr[c]);
      }
      for (int c = 0; c < 3; ++c) x[3 * (a0 + i) + c] = fr[0] * a[c] + fr[1] * a[3 + c] + fr[2] * a[6 + c];
      sys_of[a0 + i] = s;
    }
    const int p3[3] = {pbc3[3 * s] != 0, pbc3[3 * s + 1] != 0, pbc3[3 * s + 2] != 0};
    D3Sys &S = sys[s];
    S.a0 = a0;
    S.n = n;
    S.tv0 = (int64_t)(tv.size() / 3);
    translations(a, p3, d->vdw_cut, tv, S.zv);
    S.Tv = (int)((int64_t)(tv.size() / 3) - S.tv0);
    S.tc0 = (int64_t)(tc.size() / 3);
    translations(a, p3, d->cn_cut, tc, S.zc);
    S.Tc = (int)((int64_t)(tc.size() / 3) - S.tc0);
    // >= 4 work items per thread where the images allow it: from this system's own n and T, as for a single call
    S.t_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(S.Tv, (4 * NTH + (int64_t)n - 1) / n));
    vol[s] = std::fabs(det) * AU_TO_ANG * AU_TO_ANG * AU_TO_ANG;
  }
  // elements present in the batch -> dense type index and their slice of the reference-C6 grid
  std::vector<int> type_of(95, -1), elems;
  std::vector<int32_t> type(N);
  for (int i = 0; i < N; ++i) {
    if (type_of[z[i]] < 0) { type_of[z[i]] = (int)elems.size(); elems.push_back(z[i]); }
    type[i] = type_of[z[i]];
  }
  const int nt = (int)elems.size();
  const size_t nref = (size_t)nt * nt * MAXREF * MAXREF * 3;
  // packed fp64 inputs: x [3N] | tv | tc | rcov [N] | r2r4 [N] | r0 [nt nt] | ref [nt nt 5 5 3]
  const size_t o_tv = 3 * (size_t)N, o_tc = o_tv + tv.size(), o_rcov = o_tc + tc.size(), o_r2r4 = o_rcov + N, o_r0 = o_r2r4 + N,
               o_ref = o_r0 + (size_t)nt * nt, n_in = o_ref + nref;
  std::vector<double> in(n_in);
  std::memcpy(in.data(), x.data(), sizeof(double) * x.size());
  std::memcpy(in.data() + o_tv, tv.data(), sizeof(double) * tv.size());
  std::memcpy(in.data() + o_tc, tc.data(), sizeof(double) * tc.size());
  for (int i = 0; i < N; ++i) { in[o_rcov + i] = d->rcov[z[i] - 1]; in[o_r2r4 + i] = d->r2r4[z[i] - 1]; }
  // packed int32 inputs: type [N] | sys_of [N] | mxc [nt]
  std::vector<int32_t> ints(2 * (size_t)N + nt);
  std::memcpy(ints.data(), type.data(), sizeof(int32_t) * N);
  std::memcpy(ints.data() + N, sys_of.data(), sizeof(int32_t) * N);
  for (int p = 0; p < nt; ++p) {
    ints[2 * (size_t)N + p] = d->mxc[elems[p]];
    for (int q = 0; q < nt; ++q) {
      std::memcpy(&in[o_ref + ((size_t)p * nt + q) * MAXREF * MAXREF * 3], &d->c6ref[((size_t)elems[p] * 95 + elems[q]) * MAXREF * MAXREF * 3],
                  sizeof(double) * MAXREF * MAXREF * 3);
      in[o_r0 + (size_t)p * nt + q] = d->r0ab[(size_t)(elems[p] - 1) * 94 + elems[q] - 1] / AU_TO_ANG;
    }
  }
  // work array: e [N] | s [6N] | f [3N] | cn [N] (read back in one copy) | dE/dCN [N]
  const size_t o_s = N, o_f = 7 * (size_t)N, o_cn = 10 * (size_t)N, o_dc = 11 * (size_t)N;
  bool ok = d->d_in.put(in, st) && d->d_int.put(ints, st) && d->d_sys.put(sys, st) && d->d_work.ensure(12 * (size_t)N);
  SNET_REQUIRE(ok, std::string(who) + ": device allocation / upload failed");
  const double *X = d->d_in.p, *TV = X + o_tv, *TC = X + o_tc, *RCOV = X + o_rcov, *R2R4 = X + o_r2r4, *R0 = X + o_r0, *REF = X + o_ref;
  const int32_t *TYPE = d->d_int.p, *SYS_OF = TYPE + N, *MXC = TYPE + 2 * (size_t)N;
  double *W = d->d_work.p;
  d3_cn_kernel<<<N, NTH, 0, st>>>(d->d_sys.p, SYS_OF, X, TC, RCOV, d->cn_cut, W + o_cn);
  d3_pair_kernel<<<N, NTH, 0, st>>>(d->d_sys.p, SYS_OF, X, TV, R2R4, R0, TYPE, nt, W + o_cn, MXC, REF, d->vdw_cut, d->func,
                                    W, W + o_f, W + o_dc, W + o_s);
  d3_cn_force_kernel<<<N, NTH, 0, st>>>(d->d_sys.p, SYS_OF, X, TC, RCOV, d->cn_cut, W + o_dc, W + o_f, W + o_s);
  SNET_CHECK_LAUNCH(who);
  std::vector<double> out(11 * (size_t)N);
  ok = hipMemcpyAsync(out.data(), W, sizeof(double) * out.size(), hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipStreamSynchronize(st) == hipSuccess;
  SNET_REQUIRE(ok, std::string(who) + ": readback failed");
  const double *e = out.data(), *sa = e + o_s, *f = e + o_f, *cn = e + o_cn;
  for (int s = 0; s < B; ++s) {
    double et = 0.0, sv[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = atom_ptr[s]; i < atom_ptr[s + 1]; ++i) {   // fixed order: reproducible totals
      et += e[i];
      for (int q = 0; q < 6; ++q) sv[q] += sa[6 * (size_t)i + q];
    }
    energy[s] = et * AU_TO_EV;
    const double k = AU_TO_EV / vol[s];
    const double full[9] = {sv[0], sv[3], sv[4], sv[3], sv[1], sv[5], sv[4], sv[5], sv[2]};
    for (int q = 0; q < 9; ++q) stress[9 * (size_t)s + q] = full[q] * k;
  }
  for (size_t q = 0; q < 3 * (size_t)N; ++q) forces[q] = f[q] * (AU_TO_EV / AU_TO_ANG);
  std::memcpy(cn_out, cn, sizeof(double) * N);
  return 0;
}

int snet_d3_compute(snet_d3 *d, void *stream) {
  SNET_REQUIRE(d != nullptr, "snet_d3_compute: null handle");
  SNET_REQUIRE(d->have_tables && d->have_func && d->have_cell && !d->z.empty(),
               "snet_d3_compute: tables, settings, atoms and cell must be set first");
  const int64_t atom_ptr[2] = {0, (int64_t)d->z.size()};
  d->forces.resize(3 * d->z.size());
  d->cn.resize(d->z.size());
  return d3_run(d, 1, atom_ptr, d->z.data(), d->pos.data(), d->cell, d->pbc, &d->energy, d->forces.data(), d->stress, d->cn.data(),
                static_cast<hipStream_t>(stream), "snet_d3_compute", false);
}

int snet_d3_compute_batch(snet_d3 *d, int32_t n_sys, const int64_t *atom_ptr, const int32_t *atomic_numbers, const double *positions,
                          const double *cells, const int32_t *pbc, double *energy, double *forces, double *stress, double *cn,
                          void *stream) {
  SNET_REQUIRE(d && atom_ptr && atomic_numbers && positions && cells && pbc && energy && forces && stress && cn,
               "snet_d3_compute_batch: null argument");
  return d3_run(d, n_sys, atom_ptr, atomic_numbers, positions, cells, pbc, energy, forces, stress, cn, static_cast<hipStream_t>(stream),
                "snet_d3_compute_batch", true);
}

int snet_d3_plan(snet_d3 *d, int32_t n_sys, const int64_t *atom_ptr, const int32_t *atomic_numbers, const double *cells,
                 const int32_t *pbc, const int32_t *box_rule, int32_t cells_move, void *stream) {
  const std::string who = "snet_d3_plan";
  SNET_REQUIRE(d && atom_ptr && atomic_numbers && cells && pbc && box_rule, who + ": null argument");
  SNET_REQUIRE(d->have_tables && d->have_func, who + ": tables and settings must be set first");
  SNET_REQUIRE(n_sys >= 1 && atom_ptr[0] == 0, who + ": need n_sys >= 1 and atom_ptr[0] == 0");
  auto sys_msg = [&](int s, const std::string &m) { return who + ": system " + std::to_string(s) + ": " + m; };
  for (int s = 0; s < n_sys; ++s) SNET_REQUIRE(atom_ptr[s + 1] > atom_ptr[s], sys_msg(s, "no atoms (atom_ptr must increase)"));
  SNET_REQUIRE(atom_ptr[n_sys] <= (int64_t)INT32_MAX, who + ": more than 2^31 - 1 atoms in total");
  const int B = n_sys, N = (int)atom_ptr[B];
  const int32_t *z = atomic_numbers;
  auto &P = d->plan;
  P.ready = false;
  std::vector<D3PlanSys> ps(B);
  std::vector<int32_t> ints(2 * (size_t)N);   // type [N] | sys_of [N] | mxc [nt] (appended below)
  const double rc_v = std::sqrt(d->vdw_cut), rc_c = std::sqrt(d->cn_cut);
  int64_t tot_v = 0, tot_c = 0;
  for (int s = 0; s < B; ++s) {
    D3PlanSys &S = ps[s];
    S.a0 = atom_ptr[s];
    S.n = (int32_t)(atom_ptr[s + 1] - S.a0);
    S.box = box_rule[s] != 0;
    S.pad = 0;
    for (int64_t i = atom_ptr[s]; i < atom_ptr[s + 1]; ++i) {
      SNET_REQUIRE(z[i] >= 1 && z[i] <= 94, sys_msg(s, "Z = " + std::to_string(z[i]) + ": D3 parameters exist for Z = 1 .. 94"));
      ints[(size_t)N + i] = s;
    }
    for (int k = 0; k < 9; ++k) S.cell[k] = cells[9 * (size_t)s + k];
    int64_t cv = 27, cc = 27;   // the molecule box is wider than both cutoffs: one image each way
    for (int k = 0; k < 3; ++k) S.pbc[k] = S.box ? 1 : pbc[3 * s + k] != 0;
    if (!S.box) {
      double a[9];
      for (int k = 0; k < 9; ++k) a[k] = S.cell[k] / AU_TO_ANG;
      const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
      SNET_REQUIRE(std::fabs(det) > 1e-12, sys_msg(s, "singular cell (give molecules a box: the reference's calculator does, calculator.py:533-548)"));
      int rv[3], rc[3];
      SNET_REQUIRE(d3_reps(a, S.pbc, rc_v, rv) && d3_reps(a, S.pbc, rc_c, rc), sys_msg(s, "a periodic height of the cell is below cutoff / 1e5"));
      if (cells_move)   // room for every periodic axis' repetition count to grow by one
        for (int k = 0; k < 3; ++k) { rv[k] += S.pbc[k]; rc[k] += S.pbc[k]; }
      cv = d3_rep_count(rv);
      cc = d3_rep_count(rc);
    }
    S.tv0 = tot_v;
    S.tc0 = tot_c;
    tot_v += cv;
    tot_c += cc;
    SNET_REQUIRE(3 * (tot_v + tot_c) <= ((int64_t)1 << 27),
                 sys_msg(s, "the translation lists up to this system need " + std::to_string(3 * (tot_v + tot_c)) +
                                " doubles, more than the 2^27 a plan may hold (use fewer or larger cells per plan)"));
    S.cap_v = (int32_t)cv;
    S.cap_c = (int32_t)cc;
  }
  // elements present -> dense type index and their slices of the tables, as d3_run
  std::vector<int> type_of(95, -1), elems;
  for (int i = 0; i < N; ++i) {
    if (type_of[z[i]] < 0) { type_of[z[i]] = (int)elems.size(); elems.push_back(z[i]); }
    ints[i] = type_of[z[i]];
  }
  const int nt = (int)elems.size();
  const size_t o_r2r4 = N, o_r0 = 2 * (size_t)N, o_ref = o_r0 + (size_t)nt * nt;
  std::vector<double> tab(o_ref + (size_t)nt * nt * MAXREF * MAXREF * 3);
  for (int i = 0; i < N; ++i) { tab[i] = d->rcov[z[i] - 1]; tab[o_r2r4 + i] = d->r2r4[z[i] - 1]; }
  for (int p = 0; p < nt; ++p) {
    ints.push_back(d->mxc[elems[p]]);
    for (int q = 0; q < nt; ++q) {
      std::memcpy(&tab[o_ref + ((size_t)p * nt + q) * MAXREF * MAXREF * 3], &d->c6ref[((size_t)elems[p] * 95 + elems[q]) * MAXREF * MAXREF * 3],
                  sizeof(double) * MAXREF * MAXREF * 3);
      tab[o_r0 + (size_t)p * nt + q] = d->r0ab[(size_t)(elems[p] - 1) * 94 + elems[q] - 1] / AU_TO_ANG;
    }
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (the uploads read host vectors that die with this call: wait for them)
  const bool ok = P.p_tab.put(tab, st) && P.p_int.put(ints, st) && P.p_plan.put(ps, st) && P.p_sys.ensure(B) && P.p_geo.ensure(B) &&
                  P.p_x.ensure(3 * ((size_t)N + tot_v + tot_c)) && P.p_work.ensure(12 * (size_t)N) &&
                  hipStreamSynchronize(st) == hipSuccess;
  SNET_REQUIRE(ok, who + ": device allocation / upload failed");
  P.B = B, P.N = N, P.nt = nt, P.cap_v = tot_v, P.cap_c = tot_c;
  P.ready = true;
  return 0;
}

int snet_d3_compute_device(snet_d3 *d, const double *positions, const double *cells, double *energy, double *forces, double *virial,
                           double *cn, double *volume, int32_t *status, void *stream) {
  SNET_REQUIRE(d && positions && energy && forces && virial, "snet_d3_compute_device: null argument");
  SNET_REQUIRE(d->plan.ready, "snet_d3_compute_device: no plan (snet_d3_plan first, and again after new tables or settings)");
  auto &P = d->plan;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t N = P.N;
  double *X = P.p_x.p, *TV = X + 3 * N, *TC = TV + 3 * P.cap_v;
  const double *RCOV = P.p_tab.p, *R2R4 = RCOV + N, *R0 = R2R4 + N, *REF = R0 + (size_t)P.nt * P.nt;
  const int32_t *TYPE = P.p_int.p, *SYS_OF = TYPE + N, *MXC = SYS_OF + N;
  // work array as d3_run: e [N] | s [6N] | f [3N] | cn [N] | dE/dCN [N]
  double *W = P.p_work.p;
  const size_t o_s = N, o_f = 7 * N, o_cn = 10 * N, o_dc = 11 * N;
  const double box_pad = std::sqrt(std::max(d->vdw_cut, d->cn_cut)) * AU_TO_ANG;
  d3_prepare_kernel<<<P.B, NTH, 0, st>>>(P.p_plan.p, positions, cells, box_pad, std::sqrt(d->vdw_cut), std::sqrt(d->cn_cut), P.p_sys.p,
                                         P.p_geo.p, TV, TC);
  d3_wrap_kernel<<<(P.N + NTH - 1) / NTH, NTH, 0, st>>>(SYS_OF, P.p_geo.p, positions, P.N, X);
  d3_cn_kernel<<<P.N, NTH, 0, st>>>(P.p_sys.p, SYS_OF, X, TC, RCOV, d->cn_cut, W + o_cn);
  d3_pair_kernel<<<P.N, NTH, 0, st>>>(P.p_sys.p, SYS_OF, X, TV, R2R4, R0, TYPE, P.nt, W + o_cn, MXC, REF, d->vdw_cut, d->func, W,
                                      W + o_f, W + o_dc, W + o_s);
  d3_cn_force_kernel<<<P.N, NTH, 0, st>>>(P.p_sys.p, SYS_OF, X, TC, RCOV, d->cn_cut, W + o_dc, W + o_f, W + o_s);
  d3_reduce_kernel<<<P.B, NTH, 0, st>>>(P.p_sys.p, P.p_geo.p, W, W + o_s, W + o_f, W + o_cn, energy, forces, virial, cn, volume, status);
  SNET_CHECK_LAUNCH("snet_d3_compute_device");
  return 0;
}

double snet_d3_energy(const snet_d3 *d) { return d ? d->energy : 0.0; }
const double *snet_d3_forces(const snet_d3 *d) { return (d && !d->forces.empty()) ? d->forces.data() : nullptr; }
const double *snet_d3_stress(const snet_d3 *d) { return d ? d->stress : nullptr; }
const double *snet_d3_coordination_numbers(const snet_d3 *d) { return (d && !d->cn.empty()) ? d->cn.data() : nullptr; }

}  // extern "C"
