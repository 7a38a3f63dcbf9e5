// First interaction layer from per-atom radial moments (snet_layer0_*, include/snet_hip.h).
//
// Layer 0's source features depend on the species alone (x[src(e)] = T[s(e), :]) and its paths are (0, l -> l) with unit
// diagonal coupling, so the message of edge e is  scale * Y_e[q] * T[s(e), u] * sum_k h2_e[k] W2[k, l(q) mul + u].
// The sum over a node's edges commutes with the W2 product: with the folded weights
//   B_l[(s, k), u] = W2[k, l mul + u] * T[s, u] * scale          (fp64 product, rounded once)
// the reverse pass is  Bm_i[q, s, k] = sum_u g_m_i[q, u] B_l(q)[(s, k), u],
//                      dE/dY_e[q] = sum_k h2_e[k] Bm_i[q, s(e), k],   dE/d|r_e| = sum_q Y_e[q] sum_k h2'_e[k] Bm_i[q, s(e), k]:
// one grouped GEMM per ATOM (snet_gemm_grouped, split-precision MFMA) and one memory-bound pass over the edges in fp32 FMAs instead of
// a 64 -> wn matrix product and the tensor-product bodies per EDGE.  No fp16 operand anywhere: no row bounds, no operand scales.
// (The forward pass has the mirror form -- moments M_i[q, s, k] = sum_e Y_e[q] h2_e[k], then M B_l -- and stays on the fused kernel:
// DESIGN 4k records why.)
#include <vector>

#include "snet_common.h"

struct snet_layer0_plan {
  int lmax, Q, S, mul;
  void *BT[4];  // device, snet_gemm_split_pack of B_l^T [mul, 64 S]
};

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int HID = 64;   // width of the radial network's last hidden layer (the only one the fused layers support)
constexpr int WAVES = 4;  // nodes per 256-thread workgroup, one wavefront each

__device__ __forceinline__ int edge_slot(const int32_t *__restrict__ src, const int32_t *__restrict__ types,
                                         const int32_t *__restrict__ slot, int e, int S) {
  const int s = slot[types[src[e]]];
  return s < 0 ? 0 : (s >= S ? S - 1 : s);   // (the host hands over slots in [0, S): the clamp only keeps a bad table in bounds)
}

// Reverse pass over the edges.  A wavefront takes a node; lanes are 16 edges x 4 quarters of k.  Every lane contracts its 16 entries
// of h2 / h2' with the node's Bm[q, s(e), :] rows (the 16 lanes of a quarter read the same addresses: one fetch), the four lanes of an
// edge are summed with two permlane swaps, and the first of them folds dE/dY with dY/dr and adds the radial term along r_e / |r_e| to
// its own g_vec row: plain read-modify-write, every edge belongs to exactly one node.
template <int LMAX>
__global__ __launch_bounds__(64 * WAVES) void layer0_bwd_edges(
    const float *__restrict__ Bm, const float *__restrict__ h2, const float *__restrict__ h2d, const int32_t *__restrict__ w_row,
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ src, const int32_t *__restrict__ types,
    const int32_t *__restrict__ slot, const float *__restrict__ sh, const float *__restrict__ dsh,
    const float *__restrict__ edge_vec, int64_t n_nodes, int S, float *__restrict__ g_vec) {
  constexpr int Q = (LMAX + 1) * (LMAX + 1);
  const int lane = threadIdx.x & 63;
  // (every XCD walks a contiguous range of nodes: the two directed edges of a pair sit in neighbouring rows and read the same h2 / h2' row)
  const int64_t node = (int64_t)snet::xcd_node(blockIdx.x, gridDim.x) * WAVES + (threadIdx.x >> 6);
  if (node >= n_nodes) return;   // (wave-uniform)
  const int j = lane & 15, g = lane >> 4;
  const int e0 = row_ptr[node], e1 = row_ptr[node + 1];
  const float *Bn = Bm + (size_t)node * Q * S * HID + g * 16;
  for (int eb = e0; eb < e1; eb += 16) {
    const bool valid = eb + j < e1;
    const int e = valid ? eb + j : e1 - 1;   // idle lanes repeat the last edge: every lane takes part in the swaps
    const size_t r = (size_t)(w_row ? w_row[e] : e) * HID + g * 16;
    const float *Bs = Bn + (size_t)(S == 1 ? 0 : edge_slot(src, types, slot, e, S)) * HID;   // (one slot: no species look-up)
    f32x4 a[4], d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = *reinterpret_cast<const f32x4 *>(h2 + r + 4 * i);
      d[i] = *reinterpret_cast<const f32x4 *>(h2d + r + 4 * i);
    }
    const float *Y = sh + (size_t)e * Q;
    float gy[Q], gr = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float *b = Bs + (size_t)q * S * HID;
      float t = 0.f, u = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 bv = *reinterpret_cast<const f32x4 *>(b + 4 * i);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          t = fmaf(a[i][c], bv[c], t);
          u = fmaf(d[i][c], bv[c], u);
        }
      }
      gy[q] = t;
      gr = fmaf(Y[q], u, gr);
    }
#pragma unroll
    for (int q = 1; q < Q; ++q) {   // (Y_0 is constant: no spherical gradient)
      gy[q] = snet::swap_add16(gy[q], gy[q]);
      gy[q] = snet::swap_add32(gy[q], gy[q]);
    }
    gr = snet::swap_add16(gr, gr);
    gr = snet::swap_add32(gr, gr);
    if (valid && g == 0) {
      float t0 = 0.f, t1 = 0.f, t2 = 0.f;
      const float *jd = dsh + (size_t)e * (3 * Q);
#pragma unroll
      for (int q = 1; q < Q; ++q) {
        t0 = fmaf(gy[q], jd[3 * q], t0);
        t1 = fmaf(gy[q], jd[3 * q + 1], t1);
        t2 = fmaf(gy[q], jd[3 * q + 2], t2);
      }
      const float *v = edge_vec + (size_t)e * 3;
      const float vx = v[0], vy = v[1], vz = v[2];
      const float ir = 1.f / sqrtf(vx * vx + vy * vy + vz * vz);
      float *o = g_vec + (size_t)e * 3;
      o[0] += t0 + gr * vx * ir;
      o[1] += t1 + gr * vy * ir;
      o[2] += t2 + gr * vz * ir;
    }
  }
}

bool upload_packed(const std::vector<float> &w, int K, int N, void **dev) {
  std::vector<unsigned char> packed((size_t)snet_gemm_split_size(K, N));
  if (snet_gemm_split_pack(w.data(), K, N, packed.data())) return false;
  if (hipMalloc(dev, packed.size()) != hipSuccess) return false;
  return hipMemcpy(*dev, packed.data(), packed.size(), hipMemcpyHostToDevice) == hipSuccess;
}

}  // namespace

extern "C" int snet_layer0_fold(const float *W2_host, int32_t wn, int32_t mul, const float *table_host, float scale, int32_t n_slots,
                                int32_t l, float *bt_host) {
  SNET_REQUIRE(W2_host != nullptr && table_host != nullptr && bt_host != nullptr && mul >= 1 && n_slots >= 1 && l >= 0 &&
                   (int64_t)(l + 1) * mul <= wn, "snet_layer0_fold: bad argument");
  const int KS = HID * n_slots;
  for (int s = 0; s < n_slots; ++s)
    for (int k = 0; k < HID; ++k)
      for (int u = 0; u < mul; ++u)
        bt_host[(size_t)u * KS + s * HID + k] =
            (float)((double)W2_host[(size_t)k * wn + l * mul + u] * (double)table_host[(size_t)s * mul + u] * (double)scale);
  return 0;
}

extern "C" int snet_layer0_plan_create(const snet_conv_plan *conv, const float *W2_host, const float *table_host, float scale,
                                       int32_t n_slots, snet_layer0_plan **out) {
  SNET_REQUIRE(conv != nullptr && W2_host != nullptr && table_host != nullptr && out != nullptr, "snet_layer0_plan_create: null argument");
  *out = nullptr;
  int32_t dx = 0, dout = 0, nsh = 0, wn = 0;
  if (int rc = snet_conv_plan_dims(conv, &dx, &dout, &nsh, &wn)) return rc;
  int lmax = 0;
  while ((lmax + 1) * (lmax + 1) < nsh) ++lmax;
  // scalar inputs of multiplicity dx, one path (0, l -> l) per l <= lmax: wn = (lmax + 1) dx columns, dout = nsh dx outputs
  SNET_REQUIRE((lmax + 1) * (lmax + 1) == nsh && lmax <= 3 && dx >= 16 && dx % 16 == 0 && dx <= 512 && wn == (lmax + 1) * dx &&
                   dout == nsh * dx,
               "snet_layer0_plan_create: not a scalar-input (0, l -> l) shape with lmax <= 3 and 16 | mul <= 512");
  SNET_REQUIRE(n_slots >= 1 && n_slots <= 4, "snet_layer0_plan_create: 1 .. 4 species slots");
  auto *p = new snet_layer0_plan{lmax, nsh, n_slots, dx, {nullptr, nullptr, nullptr, nullptr}};
  const int KS = HID * n_slots;
  std::vector<float> bt((size_t)KS * dx);
  bool ok = true;
  for (int l = 0; ok && l <= lmax; ++l)
    ok = snet_layer0_fold(W2_host, wn, dx, table_host, scale, n_slots, l, bt.data()) == 0 && upload_packed(bt, dx, KS, &p->BT[l]);
  if (!ok) {
    snet_layer0_plan_destroy(p);
    snet::set_error("snet_layer0_plan_create: packing / upload of the folded weights failed");
    return 1;
  }
  *out = p;
  return 0;
}

extern "C" void snet_layer0_plan_destroy(snet_layer0_plan *p) {
  if (p == nullptr) return;
  for (int l = 0; l < 4; ++l)
    if (p->BT[l]) (void)hipFree(p->BT[l]);
  delete p;
}

extern "C" int64_t snet_layer0_scratch_size(const snet_layer0_plan *p, int64_t n_nodes) {
  return p == nullptr || n_nodes < 0 ? -1 : n_nodes * p->Q * p->S * HID;
}

extern "C" int snet_layer0_conv_bwd(const snet_layer0_plan *p, const float *g_m, const float *h2, const float *h2d,
                                    const int32_t *w_row, const int32_t *row_ptr, const int32_t *src, const int32_t *types,
                                    const int32_t *species_slot, const float *sh, const float *dsh, const float *edge_vec,
                                    int64_t n_nodes, float *scratch, float *g_vec, void *stream) {
  SNET_REQUIRE(p != nullptr, "snet_layer0_conv_bwd: null plan");
  if (n_nodes <= 0) return 0;
  SNET_REQUIRE(g_m && h2 && h2d && row_ptr && src && types && species_slot && sh && dsh && edge_vec && scratch && g_vec,
               "snet_layer0_conv_bwd: null argument");
  SNET_REQUIRE((n_nodes + WAVES - 1) / WAVES < (1ll << 31), "snet_layer0_conv_bwd: too many rows");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int KS = HID * p->S;
  snet_gemm_desc descs[4];
  for (int l = 0; l <= p->lmax; ++l)   // Bm[node, q, (s, k)] = g_m[node, q, :] @ B_l^T
    descs[l] = snet_gemm_desc{nullptr, p->BT[l], (int64_t)l * l * p->mul, (int64_t)l * l * KS, 2 * l + 1, p->mul, KS, 0};
  if (int rc = snet_gemm_grouped(descs, p->lmax + 1, g_m, scratch, n_nodes, (int64_t)p->Q * p->mul, (int64_t)p->Q * KS, nullptr, stream))
    return rc;
  const dim3 grid((unsigned)((n_nodes + WAVES - 1) / WAVES)), block(64 * WAVES);
#define SNET_L0_BWD(LM)                                                                                                         \
  layer0_bwd_edges<LM><<<grid, block, 0, st>>>(scratch, h2, h2d, w_row, row_ptr, src, types, species_slot, sh, dsh, edge_vec, \
                                               n_nodes, p->S, g_vec)
  switch (p->lmax) {
    case 0: SNET_L0_BWD(0); break;
    case 1: SNET_L0_BWD(1); break;
    case 2: SNET_L0_BWD(2); break;
    default: SNET_L0_BWD(3); break;
  }
#undef SNET_L0_BWD
  SNET_CHECK_LAUNCH("snet_layer0_conv_bwd");
  return 0;
}
