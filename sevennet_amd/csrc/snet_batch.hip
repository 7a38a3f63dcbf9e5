// Batched evaluation of many small structures in one engine call: the graph build of B systems in one count launch and one
// fill launch, and the per-system fp64 reductions (energy, virial) that replace the single totals of the one-structure path.
//
// Neighbor list: one lane per center atom, looping over the atoms of its own system (atom_ptr) and, for each of them, over
// exactly the image shifts S that can bring it within the cutoff: along a periodic axis k the fractional coordinate of
// d = r_j - r_i + S.cell is df_k + S_k with |.| <= rc / h_k inside the cutoff sphere (h_k = distance between the opposite
// faces), so S_k runs over [ceil(-df_k - rc/h_k), floor(-df_k + rc/h_k)].  No wrapping is needed: shifts are relative to the
// caller's positions, edge_vec = r_j - r_i + S.cell is computed in fp64 and stored as fp32 (sevenn/train/dataload.py:32-129,
// as snet_neighbor.hip).  Open axes are neither wrapped nor imaged (S_k = 0); a zero cell row of an open axis is padded with a
// lattice vector along that axis (dataload.py:37-48) so that the inverse exists -- the edge set does not depend on its length.
// Cells thinner than the cutoff meet themselves through several images.  O(n_s^2 * images) per system: the path for small
// and medium systems (the host routes larger ones to the cell list, sevennet_amd/batch.py).
#include "snet_common.h"

namespace snet {
double *reduce_scratch(int64_t n_doubles, hipStream_t st);
void launch_final_sum(const double *partial, int n, int stride, int ncomp, double *out, hipStream_t st);
}  // namespace snet

namespace {

constexpr double MAX_IMAGE_REACH = 64.0;   // rc / h_k above this: the host list's business (as snet_nl_grid)

struct SysCell {
  double a[9], inv[9];
  double reach[3];   // rc / h_k on periodic axes, 0 on open ones
  bool ok;
};

__device__ SysCell load_cell(const double *__restrict__ cells, const int32_t *__restrict__ pbc, int s, double rc) {
  SysCell C;
  for (int k = 0; k < 9; ++k) C.a[k] = cells[9 * (int64_t)s + k];
  int per[3];
  for (int k = 0; k < 3; ++k) {
    per[k] = pbc[3 * (int64_t)s + k] != 0;
    const double n2 = C.a[3 * k] * C.a[3 * k] + C.a[3 * k + 1] * C.a[3 * k + 1] + C.a[3 * k + 2] * C.a[3 * k + 2];
    if (!per[k] && n2 < 1e-24) {
      C.a[3 * k] = C.a[3 * k + 1] = C.a[3 * k + 2] = 0.0;
      C.a[3 * k + k] = 5.0 * rc;
    }
  }
  const double *a = C.a;
  const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
                     a[2] * (a[3] * a[7] - a[4] * a[6]);
  C.ok = fabs(det) > 1e-12;
  const double id = C.ok ? 1.0 / det : 0.0;
  C.inv[0] = (a[4] * a[8] - a[5] * a[7]) * id;
  C.inv[1] = (a[2] * a[7] - a[1] * a[8]) * id;
  C.inv[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  C.inv[3] = (a[5] * a[6] - a[3] * a[8]) * id;
  C.inv[4] = (a[0] * a[8] - a[2] * a[6]) * id;
  C.inv[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  C.inv[6] = (a[3] * a[7] - a[4] * a[6]) * id;
  C.inv[7] = (a[1] * a[6] - a[0] * a[7]) * id;
  C.inv[8] = (a[0] * a[4] - a[1] * a[3]) * id;
  for (int k = 0; k < 3; ++k) {   // |column k of inv| = 1 / h_k
    const double c2 = C.inv[k] * C.inv[k] + C.inv[3 + k] * C.inv[3 + k] + C.inv[6 + k] * C.inv[6 + k];
    C.reach[k] = per[k] ? rc * sqrt(c2) : 0.0;
    if (C.reach[k] > MAX_IMAGE_REACH) C.ok = false;
  }
  return C;
}

// one lane per center atom; FILL = false counts, FILL = true writes src / center / edge_vec / shifts at row_ptr[i]
template <bool FILL>
__global__ __launch_bounds__(128) void batch_nl_kernel(const double *__restrict__ pos, const int32_t *__restrict__ atom_ptr,
                                                       int32_t n_sys, const double *__restrict__ cells,
                                                       const int32_t *__restrict__ pbc, int64_t n, double rc,
                                                       int32_t *__restrict__ count, const int32_t *__restrict__ row_ptr,
                                                       int32_t *__restrict__ src, int32_t *__restrict__ center,
                                                       float *__restrict__ edge_vec, int32_t *__restrict__ shifts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = n_sys - 1;   // the system of atom i: the last s with atom_ptr[s] <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (atom_ptr[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  int64_t a0 = atom_ptr[lo], a1 = atom_ptr[lo + 1];
  a0 = a0 < 0 ? 0 : a0;
  a1 = a1 > n ? n : a1;
  const SysCell C = load_cell(cells, pbc, lo, rc);
  int cnt = 0;
  int64_t out = FILL ? row_ptr[i] : 0;
  const int64_t out_end = FILL ? row_ptr[i + 1] : 0;   // the fill never writes past the row the count pass sized
  if (C.ok) {
    const double rc2 = rc * rc, eps = 1e-9;
    const double xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
    for (int64_t j = a0; j < a1; ++j) {
      const double d0x = pos[3 * j] - xi, d0y = pos[3 * j + 1] - yi, d0z = pos[3 * j + 2] - zi;
      int slo[3], shi[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double df = d0x * C.inv[k] + d0y * C.inv[3 + k] + d0z * C.inv[6 + k];
        slo[k] = C.reach[k] > 0.0 ? (int)ceil(-df - C.reach[k] - eps) : 0;
        shi[k] = C.reach[k] > 0.0 ? (int)floor(-df + C.reach[k] + eps) : 0;
      }
      for (int sx = slo[0]; sx <= shi[0]; ++sx)
        for (int sy = slo[1]; sy <= shi[1]; ++sy)
          for (int sz = slo[2]; sz <= shi[2]; ++sz) {
            const double dx = d0x + sx * C.a[0] + sy * C.a[3] + sz * C.a[6];
            const double dy = d0y + sx * C.a[1] + sy * C.a[4] + sz * C.a[7];
            const double dz = d0z + sx * C.a[2] + sy * C.a[5] + sz * C.a[8];
            if (dx * dx + dy * dy + dz * dz < rc2 && !(j == i && sx == 0 && sy == 0 && sz == 0)) {
              if (FILL) {
                if (out >= out_end) continue;
                src[out] = (int32_t)j;
                center[out] = (int32_t)i;
                edge_vec[3 * out + 0] = (float)dx;
                edge_vec[3 * out + 1] = (float)dy;
                edge_vec[3 * out + 2] = (float)dz;
                if (shifts) {
                  shifts[3 * out + 0] = sx;
                  shifts[3 * out + 1] = sy;
                  shifts[3 * out + 2] = sz;
                }
                ++out;
              } else {
                ++cnt;
              }
            }
          }
    }
  }
  if (!FILL) count[i] = cnt;
}

// ---- per-system reductions: per-atom fp64 values, then one block per segment sums them in a fixed order
// folded readout, one wave per atom (the arithmetic of snet_readout_energy); the fp64 atomic energy goes to e64
__global__ __launch_bounds__(256) void seg_readout_kernel(const float *__restrict__ x, int64_t n, int dim, const double *__restrict__ v,
                                                          double c, const int32_t *__restrict__ types, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, int n_scale, float *__restrict__ e_atom,
                                                          double *__restrict__ e64) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int64_t i = (int64_t)blockIdx.x * 4 + wave; i < n; i += (int64_t)gridDim.x * 4) {
    const float *row = x + i * dim;
    double d = 0.0;
    for (int k = lane; k < dim; k += 64) d += (double)row[k] * v[k];
    d = snet::wave_sum_d(d) + c;
    const int t = n_scale > 1 ? types[i] : 0;
    const double e = d * (double)scale[t] + (double)shift[t];
    if (lane == 0) {
      e_atom[i] = (float)e;
      e64[i] = e;
    }
  }
}

// e_atom = e * scale[t] + shift[t] (the arithmetic of snet_rescale_reduce)
__global__ __launch_bounds__(256) void seg_rescale_kernel(const float *__restrict__ e, const int32_t *__restrict__ types,
                                                          const float *__restrict__ scale, const float *__restrict__ shift, int n_scale,
                                                          int64_t n, float *__restrict__ e_atom, double *__restrict__ e64) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = n_scale > 1 ? types[i] : 0;
    const float val = e[i] * scale[t] + shift[t];
    e_atom[i] = val;
    e64[i] = (double)val;
  }
}

// forces and per-atom virial (the arithmetic of snet_edge_force); the per-atom virial also goes to v64 in fp64
__global__ __launch_bounds__(256) void seg_force_kernel(const float *__restrict__ g, const float *__restrict__ rv,
                                                        const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_ptr,
                                                        const int32_t *__restrict__ eperm, int64_t n_nodes, float *__restrict__ F,
                                                        float *__restrict__ vir_atom, double *__restrict__ v64) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += (int64_t)gridDim.x * blockDim.x) {
    float fx = 0.f, fy = 0.f, fz = 0.f;
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
      fx += g[3 * (int64_t)e + 0];
      fy += g[3 * (int64_t)e + 1];
      fz += g[3 * (int64_t)e + 2];
    }
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f, v5 = 0.f;
    for (int k = col_ptr[i]; k < col_ptr[i + 1]; ++k) {
      const int64_t e = eperm[k];
      const float gx = g[3 * e + 0], gy = g[3 * e + 1], gz = g[3 * e + 2];
      const float rx = rv[3 * e + 0], ry = rv[3 * e + 1], rz = rv[3 * e + 2];
      fx -= gx;
      fy -= gy;
      fz -= gz;
      v0 += rx * gx; v1 += ry * gy; v2 += rz * gz;
      v3 += rx * gy; v4 += ry * gz; v5 += rz * gx;
    }
    F[3 * i + 0] = fx;
    F[3 * i + 1] = fy;
    F[3 * i + 2] = fz;
    if (vir_atom) {
      vir_atom[6 * i + 0] = -v0; vir_atom[6 * i + 1] = -v1; vir_atom[6 * i + 2] = -v2;
      vir_atom[6 * i + 3] = -v3; vir_atom[6 * i + 4] = -v4; vir_atom[6 * i + 5] = -v5;
    }
    v64[6 * i + 0] = -(double)v0; v64[6 * i + 1] = -(double)v1; v64[6 * i + 2] = -(double)v2;
    v64[6 * i + 3] = -(double)v3; v64[6 * i + 4] = -(double)v4; v64[6 * i + 5] = -(double)v5;
  }
}

// out[b, c] = sum over the rows [seg_ptr[b], seg_ptr[b+1]) of val[row, c]: one block per segment, fixed order
template <int NC>
__global__ __launch_bounds__(256) void seg_sum_kernel(const double *__restrict__ val, const int32_t *__restrict__ seg_ptr, int64_t n,
                                                      double *__restrict__ out) {
  __shared__ double sm[4][NC];
  const int b = blockIdx.x;
  int64_t a0 = seg_ptr[b], a1 = seg_ptr[b + 1];
  a0 = a0 < 0 ? 0 : (a0 > n ? n : a0);
  a1 = a1 > n ? n : (a1 < a0 ? a0 : a1);
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  for (int64_t i = a0 + threadIdx.x; i < a1; i += blockDim.x)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] += val[NC * i + c];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const double t = snet::wave_sum_d(acc[c]);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    out[(int64_t)b * NC + c] = sm[0][c] + sm[1][c] + sm[2][c] + sm[3][c];
  }
}

inline unsigned grid_for(int64_t n, int per_block) {
  int64_t g = (n + per_block - 1) / per_block;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// per-segment sums of the fp64 rows in scratch, then their fixed-order total
void launch_seg_sums(const double *val, int nc, const int32_t *seg_ptr, int32_t n_seg, int64_t n, double *out_seg, double *out_total,
                     hipStream_t st) {
  if (nc == 1) seg_sum_kernel<1><<<(unsigned)n_seg, 256, 0, st>>>(val, seg_ptr, n, out_seg);
  else seg_sum_kernel<6><<<(unsigned)n_seg, 256, 0, st>>>(val, seg_ptr, n, out_seg);
  if (out_total) snet::launch_final_sum(out_seg, n_seg, nc, nc, out_total, st);
}

}  // namespace

extern "C" int snet_batch_nl_count(const double *pos, const int32_t *atom_ptr, int32_t n_sys, const double *cells, const int32_t *pbc,
                                   int64_t n_atoms, double cutoff, int32_t *count, void *stream) {
  SNET_REQUIRE(cutoff > 0 && n_sys >= 1 && n_atoms < (1ll << 31), "snet_batch_nl_count: bad cutoff / shape");
  if (n_atoms <= 0) return 0;
  SNET_REQUIRE(pos && atom_ptr && cells && pbc && count, "snet_batch_nl_count: null argument");
  batch_nl_kernel<false><<<(unsigned)((n_atoms + 127) / 128), 128, 0, static_cast<hipStream_t>(stream)>>>(
      pos, atom_ptr, n_sys, cells, pbc, n_atoms, cutoff, count, nullptr, nullptr, nullptr, nullptr, nullptr);
  SNET_CHECK_LAUNCH("snet_batch_nl_count");
  return 0;
}

extern "C" int snet_batch_nl_fill(const double *pos, const int32_t *atom_ptr, int32_t n_sys, const double *cells, const int32_t *pbc,
                                  int64_t n_atoms, double cutoff, const int32_t *row_ptr, int32_t *src, int32_t *center,
                                  float *edge_vec, int32_t *shifts, void *stream) {
  SNET_REQUIRE(cutoff > 0 && n_sys >= 1 && n_atoms < (1ll << 31), "snet_batch_nl_fill: bad cutoff / shape");
  if (n_atoms <= 0) return 0;
  // (the outputs of an edge-free batch are empty, null pointers: out_end bounds every write by the scanned counts)
  SNET_REQUIRE(pos && atom_ptr && cells && pbc && row_ptr, "snet_batch_nl_fill: null argument");
  batch_nl_kernel<true><<<(unsigned)((n_atoms + 127) / 128), 128, 0, static_cast<hipStream_t>(stream)>>>(
      pos, atom_ptr, n_sys, cells, pbc, n_atoms, cutoff, nullptr, row_ptr, src, center, edge_vec, shifts);
  SNET_CHECK_LAUNCH("snet_batch_nl_fill");
  return 0;
}

extern "C" int snet_readout_energy_seg(const float *x, int64_t n, int32_t dim, const double *v, double c, const int32_t *types,
                                       const float *scale, const float *shift, int32_t n_scale, const int32_t *seg_ptr, int32_t n_seg,
                                       float *e_atom, double *energy_seg, double *energy_total, void *stream) {
  SNET_REQUIRE(n_scale >= 1 && dim > 0, "snet_readout_energy_seg: n_scale >= 1 and dim > 0 required");
  SNET_REQUIRE(n_scale == 1 || types != nullptr, "snet_readout_energy_seg: species-wise scale needs types");
  SNET_REQUIRE(n_seg >= 1 && seg_ptr != nullptr && energy_seg != nullptr, "snet_readout_energy_seg: segments required");
  hipStream_t st = static_cast<hipStream_t>(stream);
  n = n < 0 ? 0 : n;
  double *e64 = snet::reduce_scratch(n, st);
  SNET_REQUIRE(e64 != nullptr, "snet_readout_energy_seg: scratch allocation failed");
  if (n > 0) seg_readout_kernel<<<grid_for(n, 4), 256, 0, st>>>(x, n, dim, v, c, types, scale, shift, n_scale, e_atom, e64);
  launch_seg_sums(e64, 1, seg_ptr, n_seg, n, energy_seg, energy_total, st);
  SNET_CHECK_LAUNCH("snet_readout_energy_seg");
  return 0;
}

extern "C" int snet_rescale_reduce_seg(const float *e_scaled, const int32_t *types, const float *scale, const float *shift,
                                       int32_t n_scale, int64_t n, const int32_t *seg_ptr, int32_t n_seg, float *e_atom,
                                       double *energy_seg, double *energy_total, void *stream) {
  SNET_REQUIRE(n_scale >= 1, "snet_rescale_reduce_seg: n_scale >= 1 required");
  SNET_REQUIRE(n_seg >= 1 && seg_ptr != nullptr && energy_seg != nullptr, "snet_rescale_reduce_seg: segments required");
  hipStream_t st = static_cast<hipStream_t>(stream);
  n = n < 0 ? 0 : n;
  double *e64 = snet::reduce_scratch(n, st);
  SNET_REQUIRE(e64 != nullptr, "snet_rescale_reduce_seg: scratch allocation failed");
  if (n > 0) seg_rescale_kernel<<<grid_for(n, 256), 256, 0, st>>>(e_scaled, types, scale, shift, n_scale, n, e_atom, e64);
  launch_seg_sums(e64, 1, seg_ptr, n_seg, n, energy_seg, energy_total, st);
  SNET_CHECK_LAUNCH("snet_rescale_reduce_seg");
  return 0;
}

extern "C" int snet_edge_force_seg(const float *g_vec, const float *edge_vec, const int32_t *row_ptr, const int32_t *col_ptr,
                                   const int32_t *eperm, int64_t n_nodes, int64_t n_edges, const int32_t *seg_ptr, int32_t n_seg,
                                   float *forces, float *virial_atom, double *virial_seg, double *virial_total, void *stream) {
  (void)n_edges;
  SNET_REQUIRE(n_seg >= 1 && seg_ptr != nullptr && virial_seg != nullptr, "snet_edge_force_seg: segments required");
  hipStream_t st = static_cast<hipStream_t>(stream);
  n_nodes = n_nodes < 0 ? 0 : n_nodes;
  double *v64 = snet::reduce_scratch(6 * n_nodes, st);
  SNET_REQUIRE(v64 != nullptr, "snet_edge_force_seg: scratch allocation failed");
  if (n_nodes > 0)
    seg_force_kernel<<<grid_for(n_nodes, 256), 256, 0, st>>>(g_vec, edge_vec, row_ptr, col_ptr, eperm, n_nodes, forces, virial_atom, v64);
  launch_seg_sums(v64, 6, seg_ptr, n_seg, n_nodes, virial_seg, virial_total, st);
  SNET_CHECK_LAUNCH("snet_edge_force_seg");
  return 0;
}
