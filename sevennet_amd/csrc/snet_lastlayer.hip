// Reverse pass of a scalar-output interaction layer (the last one) in ONE pass over the edges grouped by source
// (snet_lastlayer_*, include/snet_hip.h).
//
// Every path of such a layer is (l, l -> 0) with the diagonal coupling c_l, so the layer's share of the energy gradient is the
// bilinear form
//   B = scale sum_e sum_{l,u} g_m[dst(e)][l,u] w_e[l,u] c_l sum_a h[src(e)][l,u,a] Y_e[l,a],       w_e = h2_e W2.
// The fused kernels evaluate it twice: grouped by destination for dB/dr_e (g_vec; gathers the dx-float source row per edge) and,
// transposed, grouped by source for dB/dh (g_h; gathers the dmid-float g_m row per edge), each with its own W2 products.  Grouped by
// SOURCE, one wave keeps its node's h row on chip and both derivatives fall out of the same per-edge quantities:
//   t_e[l,u]       = scale c_l w_e[l,u] g_m[dst(e)][l,u]
//   g_h[j][l,u,a]  = sum_e t_e[l,u] Y_e[l,a]
//   dB/dY_e[l,a]   = sum_u t_e[l,u] h_j[l,u,a]
//   dB/d|r_e|      = sum_{l,u} scale c_l w'_e[l,u] g_m[dst(e)][l,u] sum_a h_j[l,u,a] Y_e[l,a],      w'_e = h2'_e W2
// (c_l rides on W2's columns: the plan takes them from the shape's transposed-product table, snet_conv_plan_transposed.)
//
// Mapping: a wave takes one source atom and walks its out-edges in tiles of 16.  w and w' tiles of 16 edges x 16 channels come from
// v_mfma_f32_16x16x32_f16 on two-term fp16 operands (snet_split.h): A = the tile's h2 / h2' rows, each with its own power-of-two tile
// scale, B = W2, split once on the host and resident in LDS for the whole workgroup (64 wn 4 bytes).  The accumulator puts a
// channel on lane & 15 and four edges (lane >> 4) 4 + i in its registers: the g_h accumulators of a channel live in that channel's
// lanes (the node's h row and the tile's Y in wave-private LDS), the g_m gather is one 64-byte row segment per edge and channel
// tile.  No operand of a matrix product depends on g_m: no row bounds.  Every sum runs in a fixed order; g_vec rows are added to
// with plain read-modify-write (a directed edge has one source), g_h rows -- dead ranges included -- are written once per node.
#include <cmath>
#include <cstring>
#include <vector>

#include "snet_split.h"

struct snet_lastlayer_plan {
  int lmax, nsh, dx, dmid, wn;
  int m[4];       // 16-channel tiles per l
  int x_off[4];   // offset of block l in the source row
  int n_dead, dead[16];
  int w2_exp;     // W2 is stored times 2^w2_exp
  void *image;    // device: fp16 hi / lo fragments of W2, [column tile][q][term][lane] x 16 bytes
};

namespace {

using snet::f32x4;
using snet::u32x4;
using snet::bf16x8;
using snet::SplitN;
constexpr int HID = 64;
constexpr int WAVES = 4;   // nodes in flight per 256-thread workgroup, one wavefront each

struct LastArgs {
  const float *h, *g_m, *sh, *dsh, *edge_vec, *h2, *h2d;
  const int32_t *col_ptr, *center_t, *w_row_t, *eperm;
  const u32x4 *image;
  float *g_h, *g_vec;
  int64_t row_a, row_b;
  float scale;
  int w2_exp, dx, dmid;
  int x_off[4];
  int n_dead, dead[16];
};

__device__ __forceinline__ float sum16(float v) {   // over the 16 lanes of a row; every lane gets the same bits
  v += snet::lane_xor<1>(v);
  v += snet::lane_xor<2>(v);
  v += snet::lane_xor<4>(v);
  v += snet::lane_xor<8>(v);
  return v;
}
// An empty statement the compiler cannot move a value's definition across.  Without these on the running sums hipcc gathers the
// matrix products of every tile first and spills their results (253 registers of scratch at SevenNet-0's shape; none with them).
template <class T>
__device__ __forceinline__ void pin(T &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ float pick4(const f32x4 v, int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }

// A run of MC channel tiles [C0, C0 + MC) of path (l, l -> 0) (M tiles; W2 columns / g_m entries from tile T0): first run of a path
// clears the path's dB/dY partials, the last one folds them.  hs = the node's block l in LDS ([a][channel]), acc = its g_h sums.
template <int L, int M, int T0, int C0, int MC>
struct PathRun {
  static constexpr int NA = 2 * L + 1;
  __device__ static __forceinline__ void run(const u32x4 *__restrict__ img, const float *__restrict__ yl, const float *__restrict__ hs,
                                             int lane, const SplitN<2> (&ha)[2], const SplitN<2> (&hd)[2], f32x4 (&G)[MC], float cu,
                                             float cd, float (&acc)[M][NA], f32x4 (&gy)[7], const float *__restrict__ jd, float &t0,
                                             float &t1, float &t2, f32x4 &gr) {
    f32x4 Y[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      Y[a] = *reinterpret_cast<const f32x4 *>(yl + (L * L + a) * 16);
      if constexpr (C0 == 0) gy[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      const int ct = C0 + k;
      f32x4 wv = f32x4{0.f, 0.f, 0.f, 0.f}, wd = wv;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        bf16x8 b[2];
        b[0] = snet::as_bf16x8(img[(((T0 + ct) * 2 + q) * 2 + 0) * 64 + lane]);
        b[1] = snet::as_bf16x8(img[(((T0 + ct) * 2 + q) * 2 + 1) * 64 + lane]);
        wv = snet::mfma16_split<2, true>(ha[q], b, wv);
        wd = snet::mfma16_split<2, true>(hd[q], b, wd);   // w' on the same W2 fragments
      }
      const f32x4 t = wv * (G[k] * cu), td = wd * (G[k] * cd);
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const float hv = hs[(a * M + ct) * 16];
        float v = acc[ct][a];
#pragma unroll
        for (int i = 0; i < 4; ++i) v = fmaf(t[i], Y[a][i], v);
        pin(v);
        acc[ct][a] = v;
        if constexpr (L > 0) {   // (Y_0 is constant: no spherical gradient)
          gy[a] = t * hv + gy[a];
          pin(gy[a]);
        }
        s = Y[a] * hv + s;
      }
      gr = td * s + gr;
      pin(gr);
      // (left alone, the scheduler issues the matrix products of every tile first and parks their results in scratch)
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (L > 0 && C0 + MC == M) {
      // dB/dY of the path: over the 16 channel lanes, then lane c of an edge group folds edge c & 3 with dY/dr
      const int i = lane & 3;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = sum16(gy[a][k]);
        const float v = pick4(r, i);
        const float *d = jd + 3 * (L * L + a);
        t0 = fmaf(v, d[0], t0);
        t1 = fmaf(v, d[1], t1);
        t2 = fmaf(v, d[2], t2);
        pin(t0);
        pin(t1);
        pin(t2);
      }
    }
  }
};

// g_h entries of one block: summed over the four edge groups, stored by the first
template <int M, int NA>
__device__ __forceinline__ void store_rows(float *__restrict__ p, int c, bool first, float (&acc)[M][NA]) {
#pragma unroll
  for (int ct = 0; ct < M; ++ct)
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      float v = acc[ct][a];
      v = snet::swap_add16(v, v);
      v = snet::swap_add32(v, v);
      acc[ct][a] = v;
    }
  if (first) {
#pragma unroll
    for (int ct = 0; ct < M; ++ct)
#pragma unroll
      for (int a = 0; a < NA; ++a) p[(a * M + ct) * 16 + c] = acc[ct][a];
  }
}

template <int M, int NA>
__device__ __forceinline__ void clear_rows(float (&acc)[M][NA]) {
#pragma unroll
  for (int ct = 0; ct < M; ++ct)
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[ct][a] = 0.f;
}

// g_m segments of MC channel tiles from column col on: one 64-byte segment per edge and tile over the 16 channel lanes
template <int MC>
__device__ __forceinline__ void gather_g(const float *(&gp)[4], const f32x4 okm, int col, f32x4 (&G)[MC]) {
#pragma unroll
  for (int k = 0; k < MC; ++k) {
    f32x4 x;
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = gp[i][col + 16 * k];
    G[k] = x * okm;
  }
}

// (keeps the loads and LDS reads that follow behind the ones in front: the gathers run one run of tiles ahead of their use, no further)
__device__ __forceinline__ void stage() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <int M0, int M1, int M2, int M3>
__global__ __launch_bounds__(64 * WAVES, 2) void lastlayer_bwd(const LastArgs A) {
  constexpr int LMAX = M3 > 0 ? 3 : (M2 > 0 ? 2 : (M1 > 0 ? 1 : 0)), NSH = (LMAX + 1) * (LMAX + 1);
  constexpr int NT = M0 + M1 + M2 + M3;   // column tiles of W2
  constexpr int X1 = M1 > 0 ? M1 : 1, X2 = M2 > 0 ? M2 : 1, X3 = M3 > 0 ? M3 : 1;
  constexpr int H1 = 16 * M0, H2 = H1 + 48 * M1, H3 = H2 + 80 * M2, HN = H3 + 112 * M3;   // live blocks of the source row, packed
  constexpr int A0 = M0 > 4 ? M0 / 2 : M0, B0 = M0 - A0, B0x = B0 > 0 ? B0 : 1;            // path 0 in two runs when it is long
  __shared__ u32x4 img[NT * 4 * 64];
  __shared__ __attribute__((aligned(16))) float s_y[WAVES][NSH * 16];
  __shared__ float s_h[WAVES][HN];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  for (int k = tid; k < NT * 4 * 64; k += 64 * WAVES) img[k] = A.image[k];
  __syncthreads();
  // a workgroup walks a contiguous run of node quads (every XCD a contiguous range of runs): the W2 image is loaded once per run
  const int64_t n_rows = A.row_b - A.row_a, n_quads = (n_rows + WAVES - 1) / WAVES;
  const int64_t per = (n_quads + gridDim.x - 1) / gridDim.x;
  const int64_t q0 = (int64_t)snet::xcd_node(blockIdx.x, gridDim.x) * per, q1 = q0 + per < n_quads ? q0 + per : n_quads;
  float *yw = s_y[wave], *hw = s_h[wave];
  const float *yl = yw + 4 * g, *hl = hw + c;
  for (int64_t quad = q0; quad < q1; ++quad) {
    const int64_t node = A.row_a + quad * WAVES + wave;
    if (node >= A.row_b) break;   // (wave-uniform; no workgroup barrier below)
    const float *hrow = A.h + (size_t)node * A.dx;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the previous node's reads are done)
    __builtin_amdgcn_wave_barrier();
    for (int k = lane; k < H1; k += 64) hw[k] = hrow[A.x_off[0] + k];
    if constexpr (M1 > 0) for (int k = lane; k < H2 - H1; k += 64) hw[H1 + k] = hrow[A.x_off[1] + k];
    if constexpr (M2 > 0) for (int k = lane; k < H3 - H2; k += 64) hw[H2 + k] = hrow[A.x_off[2] + k];
    if constexpr (M3 > 0) for (int k = lane; k < HN - H3; k += 64) hw[H3 + k] = hrow[A.x_off[3] + k];
    float a0[M0][1], a1[X1][3], a2[X2][5], a3[X3][7];
    clear_rows<M0, 1>(a0);
    clear_rows<X1, 3>(a1);
    clear_rows<X2, 5>(a2);
    clear_rows<X3, 7>(a3);
    const int p_begin = A.col_ptr[node], p_end = A.col_ptr[node + 1];
    for (int p0 = p_begin; p0 < p_end; p0 += 16) {
      const int cnt = min(16, p_end - p0);
      // ---- A operands: row c of the tile = edge p0 + c (idle rows repeat the last edge; their products are never used)
      const int pr = p0 + min(c, cnt - 1);
      const size_t wr = (size_t)A.w_row_t[pr] * HID + 8 * g;
      // ---- the lane's four edges (accumulator rows 4 g + i): destination rows of g_m
      const float *gp[4];
      f32x4 okm;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        okm[i] = 4 * g + i < cnt ? 1.f : 0.f;
        gp[i] = A.g_m + (size_t)A.center_t[p0 + min(4 * g + i, cnt - 1)] * A.dmid + c;
      }
      f32x4 Ga[A0], Gb[B0x], G1[X1], G2[X2], G3[X3];
      gather_g<A0>(gp, okm, 0, Ga);
      SplitN<2> ha[2], hd[2];
      float cu, cd;
      {
        float hv[2][8], dv[2][8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 x0 = *reinterpret_cast<const f32x4 *>(A.h2 + wr + 32 * q), x1 = *reinterpret_cast<const f32x4 *>(A.h2 + wr + 32 * q + 4);
          const f32x4 y0 = *reinterpret_cast<const f32x4 *>(A.h2d + wr + 32 * q), y1 = *reinterpret_cast<const f32x4 *>(A.h2d + wr + 32 * q + 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) { hv[q][i] = x0[i]; hv[q][4 + i] = x1[i]; dv[q][i] = y0[i]; dv[q][4 + i] = y1[i]; }
        }
        const int kh = min(60, snet::F16_TOP - snet::bound_exp(snet::wave_max(fmaxf(snet::max8(hv[0]), snet::max8(hv[1])))));
        const int kd = min(60, snet::F16_TOP - snet::bound_exp(snet::wave_max(fmaxf(snet::max8(dv[0]), snet::max8(dv[1])))));
        const float sh_ = snet::pow2f(kh), sd_ = snet::pow2f(kd);
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int i = 0; i < 8; ++i) { hv[q][i] *= sh_; dv[q][i] *= sd_; }
        ha[0] = snet::splitn8<2, true>(hv[0]);
        ha[1] = snet::splitn8<2, true>(hv[1]);
        hd[0] = snet::splitn8<2, true>(dv[0]);
        hd[1] = snet::splitn8<2, true>(dv[1]);
        cu = A.scale * snet::pow2f(-(kh + A.w2_exp));
        cd = A.scale * snet::pow2f(-(kd + A.w2_exp));
      }
      // ---- spherical harmonics of the tile in wave-private LDS, [component][edge]
      const int er = A.eperm[pr];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the previous tile's reads are done)
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = g; k < NSH; k += 4) yw[k * 16 + c] = A.sh[(size_t)er * NSH + k];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // lane c of an edge group finishes edge 4 g + (c & 3)
      const bool mine = c < 4 && 4 * g + c < cnt;
      const int em = A.eperm[p0 + min(4 * g + (c & 3), cnt - 1)];
      const float *jd = A.dsh + (size_t)em * (3 * NSH);
      float t0 = 0.f, t1 = 0.f, t2 = 0.f;
      f32x4 gr = f32x4{0.f, 0.f, 0.f, 0.f}, gy[7];
      // the W2 fragments do not depend on the tile: an offset the compiler cannot see through keeps their LDS reads inside the
      // tile loop (hoisted, the whole image would sit in registers)
      int lz = lane;
      asm volatile("" : "+v"(lz));
      // runs of channel tiles, the g_m segments of each gathered one run ahead of its use
      if constexpr (B0 > 0) gather_g<B0x>(gp, okm, 16 * A0, Gb);
      else if constexpr (M1 > 0) gather_g<X1>(gp, okm, 16 * M0, G1);
      stage();
      PathRun<0, M0, 0, 0, A0>::run(img, yl, hl, lz, ha, hd, Ga, cu, cd, a0, gy, jd, t0, t1, t2, gr);
      if constexpr (B0 > 0) {
        if constexpr (M1 > 0) gather_g<X1>(gp, okm, 16 * M0, G1);
        stage();
        PathRun<0, M0, 0, A0, B0x>::run(img, yl, hl, lz, ha, hd, Gb, cu, cd, a0, gy, jd, t0, t1, t2, gr);
      }
      if constexpr (M1 > 0) {
        if constexpr (M2 > 0) gather_g<X2>(gp, okm, 16 * (M0 + M1), G2);
        stage();
        PathRun<1, X1, M0, 0, X1>::run(img, yl, hl + H1, lz, ha, hd, G1, cu, cd, a1, gy, jd, t0, t1, t2, gr);
      }
      if constexpr (M2 > 0) {
        if constexpr (M3 > 0) gather_g<X3>(gp, okm, 16 * (M0 + M1 + M2), G3);
        stage();
        PathRun<2, X2, M0 + M1, 0, X2>::run(img, yl, hl + H2, lz, ha, hd, G2, cu, cd, a2, gy, jd, t0, t1, t2, gr);
      }
      if constexpr (M3 > 0) {
        stage();
        PathRun<3, X3, M0 + M1 + M2, 0, X3>::run(img, yl, hl + H3, lz, ha, hd, G3, cu, cd, a3, gy, jd, t0, t1, t2, gr);
      }
      f32x4 rr;
#pragma unroll
      for (int k = 0; k < 4; ++k) rr[k] = sum16(gr[k]);
      const float grm = pick4(rr, c & 3);
      if (mine) {
        const float *v = A.edge_vec + (size_t)em * 3;
        const float vx = v[0], vy = v[1], vz = v[2];
        const float ir = 1.f / sqrtf(vx * vx + vy * vy + vz * vz);
        float *o = A.g_vec + (size_t)em * 3;
        o[0] += t0 + grm * vx * ir;
        o[1] += t1 + grm * vy * ir;
        o[2] += t2 + grm * vz * ir;
      }
    }
    float *orow = A.g_h + (size_t)node * A.dx;
    store_rows<M0, 1>(orow + A.x_off[0], c, g == 0, a0);
    if constexpr (M1 > 0) store_rows<X1, 3>(orow + A.x_off[1], c, g == 0, a1);
    if constexpr (M2 > 0) store_rows<X2, 5>(orow + A.x_off[2], c, g == 0, a2);
    if constexpr (M3 > 0) store_rows<X3, 7>(orow + A.x_off[3], c, g == 0, a3);
    for (int d = 0; d < A.n_dead; ++d)   // source blocks no path reads: zero gradient
      for (int k = lane; k < A.dead[2 * d + 1]; k += 64) orow[A.dead[2 * d] + k] = 0.f;
  }
}

// fp16 bits of x, round to nearest even (subnormals kept: the lo terms of small entries are subnormal), and back
uint16_t f16_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const int e = (int)((u >> 23) & 0xffu) - 127;
  const uint32_t man = u & 0x7fffffu;
  if (e > 15) return (uint16_t)(sign | 0x7c00u);   // (never reached: entries are scaled below 2^14)
  if (e >= -14) {
    uint32_t hbits = ((uint32_t)(e + 15) << 10) | (man >> 13);
    const uint32_t rem = man & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (hbits & 1u))) ++hbits;
    return (uint16_t)(sign | hbits);
  }
  if (e >= -25) {
    const uint32_t m = man | 0x800000u;
    const int shift = -14 - e + 13;
    uint32_t hbits = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (hbits & 1u))) ++hbits;
    return (uint16_t)(sign | hbits);
  }
  return sign;
}
float f16_value(uint16_t b) {
  const int e = (b >> 10) & 0x1f, man = b & 0x3ff;
  const float v = e == 0 ? std::ldexp((float)man, -24) : std::ldexp((float)(man | 0x400), e - 25);
  return (b & 0x8000u) ? -v : v;
}

struct Shape { int m[4]; void (*kernel)(const LastArgs); };
const Shape SHAPES[] = {
    {{1, 1, 0, 0}, lastlayer_bwd<1, 1, 0, 0>},
    {{1, 1, 1, 0}, lastlayer_bwd<1, 1, 1, 0>},
    {{8, 4, 2, 0}, lastlayer_bwd<8, 4, 2, 0>},
    {{8, 4, 2, 2}, lastlayer_bwd<8, 4, 2, 2>},
};

const Shape *find_shape(const int (&m)[4]) {
  for (const Shape &s : SHAPES)
    if (s.m[0] == m[0] && s.m[1] == m[1] && s.m[2] == m[2] && s.m[3] == m[3]) return &s;
  return nullptr;
}

}  // namespace

extern "C" int snet_lastlayer_plan_create(const snet_conv_plan *conv, const float *W2_host, snet_lastlayer_plan **out) {
  SNET_REQUIRE(conv != nullptr && W2_host != nullptr && out != nullptr, "snet_lastlayer_plan_create: null argument");
  *out = nullptr;
  int32_t dx = 0, dout = 0, nsh = 0, wn = 0;
  if (int rc = snet_conv_plan_dims(conv, &dx, &dout, &nsh, &wn)) return rc;
  SNET_REQUIRE(wn > 0 && wn == dout && wn % 16 == 0 && wn <= 512, "snet_lastlayer_plan_create: not a scalar-output shape (wn = dout, 16 | wn <= 512)");
  char ttag[13];
  std::vector<float> cs((size_t)wn);
  int32_t dead[32], nd = 0;
  SNET_REQUIRE(snet_conv_plan_transposed(conv, ttag, cs.data(), dead, 16, &nd) == 0 && ttag[0] != 0 && nd <= 8,
               "snet_lastlayer_plan_create: the shape has no transposed scalar product");
  // one path (l, l -> 0) per l in l order: the column factors of the transposed product are c_l = 1 / sqrt(2 l + 1) on path l's columns
  snet_lastlayer_plan p{};
  int col = 0, l = 0;
  for (; l < 4 && col < wn; ++l) {
    const float cl = (float)(1.0 / std::sqrt(2.0 * l + 1.0));
    int n = 0;
    while (col + n < wn && std::fabs(cs[col + n] - cl) <= 1e-6f) ++n;
    SNET_REQUIRE(n > 0 && n % 16 == 0, "snet_lastlayer_plan_create: paths are not (l, l -> 0) in l order with 16 | mul");
    p.m[l] = n / 16;
    col += n;
  }
  SNET_REQUIRE(col == wn, "snet_lastlayer_plan_create: paths are not (l, l -> 0) in l order, l <= 3");
  p.lmax = l - 1;
  p.nsh = (p.lmax + 1) * (p.lmax + 1);
  SNET_REQUIRE(p.nsh == nsh, "snet_lastlayer_plan_create: spherical harmonics beyond the paths' l");
  SNET_REQUIRE(find_shape(p.m) != nullptr, "snet_lastlayer_plan_create: no kernel for these multiplicities");
  // source blocks in l order, skipping the ranges no path reads
  int off = 0, live = 0;
  auto skip_dead = [&] {
    for (bool again = true; again;) {
      again = false;
      for (int d = 0; d < nd; ++d)
        if (dead[2 * d] == off && dead[2 * d + 1] > 0) { off += dead[2 * d + 1]; again = true; }
    }
  };
  for (int k = 0; k <= p.lmax; ++k) {
    skip_dead();
    p.x_off[k] = off;
    off += (2 * k + 1) * 16 * p.m[k];
    live += (2 * k + 1) * 16 * p.m[k];
  }
  skip_dead();
  int dead_len = 0;
  for (int d = 0; d < nd; ++d) { p.dead[2 * d] = dead[2 * d]; p.dead[2 * d + 1] = dead[2 * d + 1]; dead_len += dead[2 * d + 1]; }
  p.n_dead = nd;
  SNET_REQUIRE(off == dx && live + dead_len == dx, "snet_lastlayer_plan_create: source row is not the paths' blocks in l order");
  p.dx = dx; p.dmid = dout; p.wn = wn;
  // W2 with c_l on its columns, times 2^w2_exp (largest entry below 2^14), as two fp16 terms in B-fragment order
  float wmax = 0.f;
  for (int k = 0; k < HID; ++k)
    for (int c = 0; c < wn; ++c) wmax = std::fmax(wmax, std::fabs(W2_host[(size_t)k * wn + c] * cs[c]));
  SNET_REQUIRE(std::isfinite(wmax), "snet_lastlayer_plan_create: W2 is not finite");
  int e = 0;
  if (wmax > 0.f) (void)std::frexp(wmax, &e);   // wmax < 2^e
  p.w2_exp = snet::F16_TOP - e;
  p.w2_exp = p.w2_exp > 40 ? 40 : (p.w2_exp < -40 ? -40 : p.w2_exp);
  const int nt = wn / 16;
  std::vector<uint16_t> image((size_t)nt * 4 * 64 * 8);
  for (int t = 0; t < nt; ++t)
    for (int q = 0; q < 2; ++q)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int k = 32 * q + 8 * (lane >> 4) + j, c = 16 * t + (lane & 15);
          const float x = std::ldexp(W2_host[(size_t)k * wn + c] * cs[c], p.w2_exp);
          const uint16_t hi = f16_bits(x);
          const uint16_t lo = f16_bits(x - f16_value(hi));
          image[((((size_t)t * 2 + q) * 2 + 0) * 64 + lane) * 8 + j] = hi;
          image[((((size_t)t * 2 + q) * 2 + 1) * 64 + lane) * 8 + j] = lo;
        }
  SNET_REQUIRE(hipMalloc(&p.image, image.size() * 2) == hipSuccess, "snet_lastlayer_plan_create: device allocation failed");
  if (hipMemcpy(p.image, image.data(), image.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p.image);
    snet::set_error("snet_lastlayer_plan_create: upload of the W2 image failed");
    return 1;
  }
  *out = new snet_lastlayer_plan(p);
  return 0;
}

extern "C" void snet_lastlayer_plan_destroy(snet_lastlayer_plan *p) {
  if (p == nullptr) return;
  if (p->image) (void)hipFree(p->image);
  delete p;
}

extern "C" int snet_lastlayer_conv_bwd(const snet_lastlayer_plan *p, const float *h, const float *g_m, const float *sh, const float *dsh,
                                       const float *edge_vec, const float *h2, const float *h2d, const int32_t *col_ptr,
                                       const int32_t *center_t, const int32_t *w_row_t, const int32_t *eperm, int64_t row_a,
                                       int64_t row_b, float scale, float *g_h, float *g_vec, void *stream) {
  SNET_REQUIRE(p != nullptr, "snet_lastlayer_conv_bwd: null plan");
  if (row_b <= row_a) return 0;
  SNET_REQUIRE(row_a >= 0 && h && g_m && sh && dsh && edge_vec && h2 && h2d && col_ptr && center_t && w_row_t && eperm && g_h && g_vec,
               "snet_lastlayer_conv_bwd: null argument");
  const Shape *s = find_shape(p->m);
  SNET_REQUIRE(s != nullptr, "snet_lastlayer_conv_bwd: no kernel for this plan");
  LastArgs a{};
  a.h = h; a.g_m = g_m; a.sh = sh; a.dsh = dsh; a.edge_vec = edge_vec; a.h2 = h2; a.h2d = h2d;
  a.col_ptr = col_ptr; a.center_t = center_t; a.w_row_t = w_row_t; a.eperm = eperm;
  a.image = static_cast<const u32x4 *>(p->image);
  a.g_h = g_h; a.g_vec = g_vec; a.row_a = row_a; a.row_b = row_b; a.scale = scale;
  a.w2_exp = p->w2_exp; a.dx = p->dx; a.dmid = p->dmid;
  for (int l = 0; l < 4; ++l) a.x_off[l] = p->x_off[l];
  a.n_dead = p->n_dead;
  for (int d = 0; d < 2 * p->n_dead; ++d) a.dead[d] = p->dead[d];
  const int64_t quads = (row_b - row_a + WAVES - 1) / WAVES;
  const unsigned grid = (unsigned)(quads < 2048 ? quads : 2048);
  s->kernel<<<dim3(grid), dim3(64 * WAVES), 0, static_cast<hipStream_t>(stream)>>>(a);
  SNET_CHECK_LAUNCH("snet_lastlayer_conv_bwd");
  return 0;
}
