/*
 * snet_hip.h -- C ABI of libsnet_hip.so, the MI355X (gfx950) force-engine kernels
 * for SevenNet's per-MD-step energy/force path.
 *
 * Boundary rules
 *   - extern "C", plain pointers and sizes only (no torch / ATen types);
 *   - every pointer argument is a DEVICE pointer unless the name ends in _host;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the legacy default stream); the caller owns all buffers;
 *   - return value: 0 = ok, nonzero = error, message via snet_last_error()
 *     (thread-local).  Style follows the reference's only existing C ABI,
 *     sevenn/pair_e3gnn/pair_d3_for_ase.cu:2034-2082 (opaque handle + int rc).
 *   - all floating point is fp32 (the reference is fp32-only:
 *     sevenn/main/sevenn.py:138-139), indices are int32.
 *
 * Feature layout: node features are `ir_mul` (for each irrep block, a
 * [2l+1][mul] slab; blocks concatenated) inside the engine.  The reference's
 * boundary layout `mul_ir` ([mul][2l+1]) is converted with snet_permute_cols().
 *
 * Each entry point cites the reference code it replaces.
 */
#ifndef SNET_HIP_H
#define SNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an exported signature or a file format changes incompatibly; every host checks snet_abi_version() against
 * the header it was built from (sevennet_amd/_lib.py, lammps/pair_*_hip.cpp).  History: 1 = rounds 1-3; 2 = round 4 (snet_nl_grid /
 * _bin / _count / _fill gained the open-axis arguments, .snet files moved to "SNETMDL4") and round 5 (pair_failed); 3 = round 6 (the
 * unwired two-fp16-term grouped GEMM snet_gemm_f16_size / _pack / snet_gemm_grouped_f16 left the library); 4 = snet_layer0_* (layer 0
 * from per-atom radial moments). */
#define SNET_ABI_VERSION 4

/* ---- housekeeping ------------------------------------------------------- */
int snet_abi_version(void);
const char *snet_last_error(void);
/* number of compiled tensor-product shapes; tag i (12 hex chars) */
int snet_conv_num_shapes(void);
const char *snet_conv_shape_tag(int i);

/* ---- a1: edge embedding -------------------------------------------------
 * replaces EdgeEmbedding.forward, sevenn/nn/edge_embedding.py:207-217
 * (BesselBasis :101-103, PolynomialCutoff :125-132, XPLORCutoff :150-160,
 *  SphericalEncoding :164-185 = e3nn SphericalHarmonics 'component').       */
typedef struct snet_edge_params {
  float cutoff;        /* rc */
  int32_t n_basis;     /* <= 16 */
  int32_t cutoff_kind; /* 0 poly_cut, 1 XPLOR */
  int32_t poly_p;      /* poly_cut p value */
  float cutoff_on;     /* XPLOR r_on */
  int32_t lmax;        /* <= 3 */
  int32_t normalize;   /* SH on unit vector (1) or raw vector (0, <0.10 checkpoints) */
} snet_edge_params;

/* Per-step input of an MD host: positions, not edge vectors.  edge_vec[e] = pos[src[e]] - pos[center[e]] + shift[e]
 * (fp64 positions [n_total,3] and per-edge periodic-image offsets shift[E,3] = S.cell, nullable = no images; the
 * subtraction runs in fp64, as in the reference's hosts: pair_e3gnn.cpp:160-175, train/dataload.py:62-70).  With the
 * topology resident, a step uploads 24 bytes per atom instead of 12 bytes per edge. */
int snet_edge_vectors(const double *pos, const int32_t *center, const int32_t *src, const double *shift, int64_t n_edges,
                      float *edge_vec, void *stream);
/* edge_vec[E,3] -> emb[E,n_basis], sh[E,nsh], nsh = (lmax+1)^2; coeffs_host[n_basis] = Bessel c_n
 * (HOST).  dsh (nullable) receives the Jacobian d sh[e,i] / d edge_vec[e,a] as [E,nsh,3]; the
 * tensor-product reverse kernel contracts with it so only 3 values per edge are reduced. */
int snet_edge_embed_fwd(const snet_edge_params *p_host, const float *coeffs_host, const float *edge_vec,
                        int64_t n_edges, float *emb, float *sh, float *dsh, void *stream);
/* g_vec[E,3] (+)= d/d edge_vec of <g_emb,emb> + <g_sh,sh>  (replaces autograd through a1).
 * g_sh may be NULL (spherical part already accumulated by snet_conv_bwd_edge_vec);
 * accumulate != 0 adds to g_vec instead of overwriting it. */
int snet_edge_embed_bwd(const snet_edge_params *p_host, const float *coeffs_host, const float *edge_vec,
                        int64_t n_edges, const float *g_emb, const float *g_sh, float *g_vec, int32_t accumulate,
                        void *stream);

/* ---- a3/a4/a2.1: dense channel mixing on MFMA (fp32 in / fp32 acc) --------
 * One call = one per-irrep block of e3nn o3.Linear (sevenn/nn/linear.py:94-100),
 * one species slice of the FCTP self-connection (self_connection.py:11-67), or
 * one layer of the radial FullyConnectedNet (convolution.py:93-95,121).
 *   C[node(n), m, :] (+)= A[node(n), m, :] @ B          n < n_nodes, m < d
 *   A row address = A + node*a_node_stride + a_off + m*K      (K contiguous)
 *   C row address = C + node*c_node_stride + c_off + m*N
 *   node(n) = row_idx ? row_idx[n] : n        (species-grouped rows for FCTP)
 * B is [K,N] row-major with the e3nn path normalisation already folded in.   */
int snet_gemm(const float *A, const float *B, float *C, int64_t n_nodes, int32_t d, int32_t K, int32_t N,
              int64_t a_node_stride, int64_t a_off, int64_t c_node_stride, int64_t c_off,
              const int32_t *row_idx, int32_t accumulate, void *stream);

/* All per-irrep GEMMs of ONE equivariant linear in a single launch (same A, C, node strides, row
 * list; blocks writing the same output block must not be grouped unless the later ones accumulate
 * into distinct rows -- the host keeps accumulating blocks in separate launches).             */
typedef struct snet_gemm_desc {
  const float *B;      /* device [K,N] row-major (exact fp32 MFMA), or NULL when B_split is given */
  const void *B_split; /* device copy of a snet_gemm_split_pack buffer: bf16 x 6 split-precision MFMA
                          (fp32-rounding-class error, ~2.5x the fp32 matrix-pipe rate); or NULL */
  int64_t a_off, c_off;
  int32_t d, K, N, accumulate;
} snet_gemm_desc;
#define SNET_MAX_GEMM_GROUP 8
int snet_gemm_grouped(const snet_gemm_desc *descs_host, int32_t n_desc, const float *A, float *C, int64_t n_nodes,
                      int64_t a_node_stride, int64_t c_node_stride, const int32_t *row_idx, void *stream);
/* Two-source grouped GEMM (split-packed weights only): every problem writes ONE output block from one or two operand pairs,
 *   C[node, c_off + m*N + :] = A0[node, a_off0 + m*K0 + :] B0  (+ A1[node, a_off1 + m*K1 + :] B1)  (+ table[types[node], same columns])
 * in one launch: the k loop runs through source 0's k steps and then source 1's, each source into its own accumulators, which are
 * added once at the single (non-accumulating) store.  It replaces a writing launch followed by an accumulating one over the same
 * rows (y = SI2(m) + sc(x), g_x = sc^T(g_y) + SI1^T(g_h)) and returns that pair's bits: the accumulating epilogue added the same
 * two numbers.  Each source has its own base pointer, node stride, offset and K; all
 * problems of a launch share C, its node stride, the row list and n_nodes.  `table` (with `types`, both device, or both NULL):
 * fp32 [n_types, c_node_stride], addressed like C; its row is added in the epilogue (layer 0's species-only self-connection).
 * With one source and no table the result is bit-identical to snet_gemm_grouped.  A source whose weights are fp32 (`B`) is
 * refused, alone or mixed with packed ones; n_nodes <= 0 returns 0.                                                          */
#define SNET_GEMM_MAX_SRC 2
typedef struct snet_gemm_src {
  const float *A;       /* device rows of this source */
  const float *B;       /* fp32 weights: not served here (must be NULL) */
  const void *B_split;  /* device copy of a snet_gemm_split_pack buffer of [K,N] */
  int64_t a_node_stride, a_off;
  int32_t K, reserved;
} snet_gemm_src;
typedef struct snet_gemm_multi_desc {
  snet_gemm_src src[SNET_GEMM_MAX_SRC];
  int64_t c_off;
  int32_t n_src, d, N, reserved;
} snet_gemm_multi_desc;
int snet_gemm_multi(const snet_gemm_multi_desc *descs_host, int32_t n_desc, float *C, int64_t n_nodes, int64_t c_node_stride,
                    const int32_t *row_idx, const float *table, const int32_t *types, void *stream);
/* weights [K,N] (HOST, fp32, normalisation folded) -> matrix-core B fragments, each value written as
 * a sum of three bf16 terms (HOST buffer of snet_gemm_split_size bytes; upload it and pass the device
 * copy as snet_gemm_desc.B_split).  All problems of one grouped launch must use the same kind. */
int64_t snet_gemm_split_size(int32_t K, int32_t N);
int snet_gemm_split_pack(const float *B_host, int32_t K, int32_t N, void *packed_host);
/* Fused radial MLP, e3nn FullyConnectedNet([nb,h1,h2,wn], act) (convolution.py:93-95,121):
 *   fwd  w[E,wn] = (act(act(emb W0) cst W1) cst) W2          W0[nb,h1] W1[h1,h2] W2[h2,wn]
 *   bwd  g_emb[E,nb] += d<g_w,w>/d emb
 * A plan holds device copies of the weights (HOST pointers in, row-major, 1/sqrt(fan_in) already
 * folded).  Hidden activations stay in registers (fwd) or are recomputed (bwd).
 *   mode 0: exact fp32 MFMA (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain)
 *   mode 1: bf16 x 6 split products on v_mfma_f32_32x32x16_bf16 (operands written as 3-term bf16
 *           sums, the six products of order <= 2 accumulated in fp32: fp32-rounding-class error at
 *           6/16 of the fp32 matrix-pipe time)
 * Only h1 = h2 = 64 and nb <= 32 are fused (rc 2 otherwise: use snet_gemm + snet_act_*). */
typedef struct snet_mlp_plan snet_mlp_plan;
int snet_radial_mlp_plan_create(int32_t nb, int32_t h1, int32_t h2, int32_t wn, const float *W0_host,
                                const float *W1_host, const float *W2_host, int32_t act, float cst, int32_t mode,
                                snet_mlp_plan **plan);
void snet_radial_mlp_plan_destroy(snet_mlp_plan *plan);
int snet_radial_mlp_fwd(const snet_mlp_plan *plan, const float *emb, int64_t n_edges, float *w_out, void *stream);
int snet_radial_mlp_bwd(const snet_mlp_plan *plan, const float *emb, const float *g_w, int64_t n_edges,
                        float *g_emb, void *stream);

/* a = act(z)*cst  /  g_z = g_a * cst * act'(z)   (act: 0 silu, 1 tanh);
 * radial-MLP hidden activations, normalize2mom constant `cst` */
int snet_act_fwd(const float *z, float *a, int64_t n, int32_t act, float cst, void *stream);
int snet_act_bwd(const float *z, const float *g_a, float *g_z, int64_t n, int32_t act, float cst, void *stream);

/* ---- a2.2-a2.5: fused gather -> uvu tensor product -> segmented reduce ----
 * replaces IrrepsConvolution.forward lines 131-135 / the `convolution_cls`
 * plug-in call of IrrepsScatterGatterFusedConvolution (convolution.py:270-278):
 *   out[i] = scale * sum_{e: dst(e)=i} TP_uvu(x[src(e)], sh[e]; w[e])
 * Edges must be sorted by destination (CSR row_ptr over the n_dst owned
 * nodes); x has n_src >= n_dst rows (ghost rows are gather sources only,
 * convolution.py:125-138).  A plan is a compiled specialisation looked up by
 * its shape tag (sevennet_amd.model_spec.ConvSpec.tag).                      */
typedef struct snet_conv_plan snet_conv_plan;
int snet_conv_plan_create(const char *tag, snet_conv_plan **plan);
void snet_conv_plan_destroy(snet_conv_plan *plan);
/* Shapes are compiled ahead of time (sevennet_amd/shapes.py) or ON DEMAND: a shape library is a small .so holding
 * the generated kernels of one or more shapes (python -m sevennet_amd.jit <irreps...>, sevennet_amd.jit.ensure_conv_shape,
 * which the Python plug-in and engine call themselves for an unknown shape -- the reference's accelerator back ends JIT
 * theirs the same way, convolution.py:237-247).  Loading it registers its shapes with this library. */
int snet_conv_register_library(const char *path);
int snet_conv_plan_dims(const snet_conv_plan *plan, int32_t *dx, int32_t *dout, int32_t *nsh, int32_t *wn);

/* w_row (nullable, int32[E]): row of w that edge e reads.  NULL = edge e reads row e (the reference's
 * layout, convolution.py:121).  The radial weights depend on |r| only, so the two directed edges of
 * one undirected pair carry the same w row; snet_edge_pairs builds the map that lets the radial MLP
 * run once per pair and w hold one row per pair.                                                   */
int snet_conv_fwd(const snet_conv_plan *plan, const float *x, const float *sh, const float *w, const int32_t *w_row,
                  const int32_t *row_ptr, const int32_t *src, int64_t n_dst, float scale, float *out,
                  void *stream);
/* ---- fused radial weights + tensor product: w[E,wn] and g_w[E,wn] never exist in memory ----------
 * The contract of the reference's own accelerator plug-ins (flash_helper.py:43, convolution.py:118-141:
 * no `weight` / `message` tensor survives) taken one step further: the radial MLP's LAST layer
 * w_e = h2_e @ W2 (64 -> weight_numel, the largest FLOP term of the model) runs on the matrix cores
 * inside the tensor-product kernels (v_mfma_f32_16x16x32_bf16 tiles whose accumulator layout is the
 * tensor product's operand layout), and the reverse kernel contracts the weight gradient with W2^T on
 * the fly.  What crosses HBM per edge is h2[64] in and g_h2[64] out instead of w[wn] and g_w[wn].
 *   h2[R,64]   hidden activations a2 of the MLP (snet_radial_mlp_hidden_fwd), R = edges or undirected
 *              pairs; edge e reads row w_row[e] (NULL: row e)
 *   terms      precision mode of the in-kernel products (both operands split into low-precision terms, fp32 accumulate):
 *              4 = f16x3 (default of both hosts): two fp16 terms per operand, hi*hi + hi*lo + lo*hi on
 *              v_mfma_f32_16x16x32_f16, operands scaled by powers of two (W2 per matrix at plan creation, h2 / g_w per
 *              16-edge tile in the kernel) -- 22 significand bits per operand: fp32-rounding class;
 *              3 = bf16x6 (three bf16 terms, six products: fp32-rounding class at twice the matrix-core work);
 *              2 = bf16x3 (two bf16 terms: ~2^-17 per product; whole-model force error at max|F| = 8 eV/A up to
 *              3.5e-4 eV/A, i.e. outside the 1e-4 bar -- kept for throughput comparisons);
 *              1 = plain bf16 (1e-2 relative)
 *   tile_ptr   int32[n_dst+1], exclusive scan of ceil(degree/16), and tile_node int32[n_tiles] (tile -> node), both
 *              from snet_edge_tiles: the reverse kernel gives each 16-edge tile of a node's CSR segment to one
 *              wavefront (tile_node capacity: n_dst + n_edges / 16 entries always suffice)
 * reverse outputs: g_xe[E,dx] (nullable; chunk order of snet_fused_plan_gxe_chunks; sum per source with
 * snet_segment_sum_rows_chunked), g_vec[E,3] ACCUMULATED (as
 * snet_conv_bwd_edge_vec), and exactly ONE of
 *   g_h2[E,64]  overwritten; feed to snet_radial_mlp_hidden_bwd, or
 *   g_emb[E,nb] ACCUMULATED: the kernel also reverses the MLP's two hidden layers per 16-edge tile (it reads
 *               emb[E,nb], the radial basis values per DIRECTED edge), so g_h2 never reaches memory either.
 *               Needs snet_fused_plan_has_mlp_tail(plan) != 0 (n_basis <= 16 and a multiple of 4).
 * x_rowmax[n_rows of x] / g_rowmax[n_dst]: upper bounds of max|x[row]| and max|g_out[node]| (snet_row_absmax, or
 *   snet_row_norm2 of the linear map's input that produced g_out); required for terms = 4, ignored (NULL) otherwise.
 * snet_conv_fused_available() != 0 iff the shape has these kernels (channel multiplicities % 16 == 0). */
#define SNET_FUSED_TERMS_DEFAULT 4
typedef struct snet_fused_plan snet_fused_plan;
int snet_radial_mlp_hidden_fwd(const snet_mlp_plan *plan, const float *emb, int64_t n_edges, float *h2, void *stream);
/* the hidden activations of n_layers (1 .. 8) interaction layers in ONE launch: the layers read the same edge embedding
 * (nn/edge_embedding.py:176-181 feeds every convolution's weight_nn, nn/convolution.py:124) and differ in weights only;
 * h2[l] <- what snet_radial_mlp_hidden_fwd(plans[l], ...) writes, bit for bit (it is the same kernel with one layer). */
int snet_radial_mlp_hidden_fwd_layers(const snet_mlp_plan *const *plans, int32_t n_layers, const float *emb, int64_t n_edges,
                                      float *const *h2, void *stream);
int snet_radial_mlp_hidden_bwd(const snet_mlp_plan *plan, const float *emb, const float *g_h2, int64_t n_edges,
                               float *g_emb, void *stream);
int snet_conv_fused_available(const snet_conv_plan *plan);
int snet_fused_plan_create(const snet_conv_plan *plan, const snet_mlp_plan *mlp, int32_t terms, snet_fused_plan **out);
void snet_fused_plan_destroy(snet_fused_plan *plan);
int snet_edge_tiles(const int32_t *row_ptr, int64_t n_dst, int32_t *tile_ptr, int32_t *tile_node, int64_t tile_capacity,
                    int64_t *n_tiles, void *stream);
/* Packed work list (reverse kernels whose snet_fused_plan_tile_mode() is 1 -- every shape whose registers hold a second
 * row's g_out entries; the lmax-3 shapes keep the per-row tiles of snet_edge_tiles, mode 0): a tile is a window of <= 16 CONSECUTIVE CSR edges of
 * the destination rows [node_begin, node_end) that touches at most two rows.  tile_e0[n_tiles + 1] (first edge of every
 * tile, then the end of the last) goes where the reverse kernel takes tile_ptr, tile_nodes[2 n_tiles] (row of the tile's
 * first / last edge) where it takes tile_node.  (node_end - node_begin) + n_edges / 16 tiles always suffice. */
int snet_edge_tiles_packed(const int32_t *row_ptr, int64_t node_begin, int64_t node_end, int32_t *tile_e0,
                           int32_t *tile_nodes, int64_t tile_capacity, int64_t *n_tiles, void *stream);
int snet_fused_plan_tile_mode(const snet_fused_plan *plan);
/* ---- merged g_xe stores -------------------------------------------------------------------------------------------------
 * A workgroup of the tangent-mode reverse kernel takes `window` consecutive tiles of its launch's list (a WINDOW, counted from the
 * start of the list), and neighbouring destination rows share sources: the g_xe rows of a window that have the same source are added
 * in LDS and written ONCE, into a compact buffer g_xe[n_rows, dx], which the segment sum then reads instead of one row per edge.
 *   snet_fused_plan_merge_window   tiles per window of this plan's merged-store kernel; 0: the shape has none (only the packed-tile
 *                                  class in tangent mode does) and the host keeps snet_conv_bwd_fused_tangent
 *   snet_gxe_merge_map             per graph, beside the tile list.  The list is tile_ptr / tile_node / n_tiles in the plan's tile
 *                                  mode (0: snet_edge_tiles, 1: snet_edge_tiles_packed), launched as the sub-lists [0, tile_cut) and
 *                                  [tile_cut, n_tiles) (tile_cut = 0: one launch): no window straddles the cut.  n_dst rows of row_ptr,
 *                                  sources in [0, n_src).  Outputs (device):
 *                                    merge_row[E]   row of the compact buffer the edge OWNS -- the first edge of its window, in edge
 *                                                   order, with its source -- or -1
 *                                    merge_next[E]  slot (16 x tile of the window + place in the tile) of the next edge of the window
 *                                                   with the same source, -1: none.  An owner's chain is summed in slot order, whatever
 *                                                   the multiplicity (several periodic images of one source in one row included)
 *                                    seg_ptr[n_src + 1], perm[n_rows <= E]  the merged rows of every source, as
 *                                                   snet_segment_sum_rows_chunked takes col_ptr / eperm
 *                                    *n_rows        merged rows in all
 *                                  It reads the index arrays back and synchronises the stream (topology only, once per graph).
 *   snet_gxe_merge_map_host        the same on host arrays, no device involved
 *   snet_conv_bwd_fused_tangent_merged  snet_conv_bwd_fused_tangent with g_xe[n_rows, dx] compact (required); g_vec bit for bit the
 *                                  same.  Rows keep the kernel's chunk order (snet_fused_plan_gxe_chunks). */
int snet_fused_plan_merge_window(const snet_fused_plan *plan);
int snet_gxe_merge_map(const int32_t *row_ptr, const int32_t *src, const int32_t *tile_ptr, const int32_t *tile_node, int64_t n_tiles,
                       int64_t tile_cut, int32_t tile_mode, int32_t window, int64_t n_dst, int64_t n_src, int64_t n_edges,
                       int32_t *merge_row, int32_t *merge_next, int32_t *seg_ptr, int32_t *perm, int64_t *n_rows, void *stream);
int snet_gxe_merge_map_host(const int32_t *row_ptr, const int32_t *src, const int32_t *tile_ptr, const int32_t *tile_node,
                            int64_t n_tiles, int64_t tile_cut, int32_t tile_mode, int32_t window, int64_t n_src, int64_t n_edges,
                            int32_t *merge_row, int32_t *merge_next, int32_t *seg_ptr, int32_t *perm, int64_t *n_rows);
int snet_conv_bwd_fused_tangent_merged(const snet_fused_plan *plan, const float *x, const float *sh, const float *dsh, const float *h2,
                                       const float *h2d, const int32_t *w_row, const int32_t *row_ptr, const int32_t *src,
                                       const int32_t *tile_ptr, const int32_t *tile_node, int64_t n_tiles, float scale,
                                       const float *g_out, float *g_xe, const int32_t *merge_row, const int32_t *merge_next,
                                       const float *edge_vec, float *g_vec, const float *x_rowmax, const float *g_rowmax, void *stream);
/* Scalar-output shapes (every path (l, l -> 0): the last interaction layer): the source-row gradient
 *   g_x[j] = sum over the edges e that have j as their source of  w_e * T * Y(e) * g_out[center(e)]
 * is itself a uvu convolution -- shape `tag` (x = the g_out row, out = g_x), radial weights W2 with column c scaled by
 * col_scale[c], run with snet_conv_fwd_fused over the edges grouped by SOURCE (row_ptr = col_ptr, src = center_t, w_row =
 * w_row_t, sh rows gathered by eperm; n_dst = n_total).  It gathers dout floats per edge where the per-edge path
 * (g_xe of snet_conv_bwd_fused + snet_segment_sum_rows_chunked) writes and re-reads dx floats.  Replaces nothing in the
 * reference (e3nn's autograd scatters g_x rows with index_add, sevenn/nn/convolution.py:130-136); exists because the
 * reverse kernel's g_xe stores are half of the last layer's time.
 * snet_conv_plan_transposed: tag[13] ("" when the shape has a non-scalar output), col_scale[wn] (nullable), dead[2 k] =
 * (offset, length) ranges of g_x the transposed product leaves unwritten (zero them).
 * snet_edges_by_source: center_t[e'] / w_row_t[e'] of the edge eperm[e'] (w_row NULL: w_row_t = eperm). */
int snet_conv_plan_transposed(const snet_conv_plan *plan, char *tag, float *col_scale, int32_t *dead, int32_t dead_capacity,
                              int32_t *n_dead);
int snet_edges_by_source(const int32_t *row_ptr, int64_t n_dst, const int32_t *eperm, const int32_t *w_row, int64_t n_edges,
                         int32_t *center_t, int32_t *w_row_t, void *stream);
int snet_conv_fwd_fused(const snet_fused_plan *plan, const float *x, const float *sh, const float *h2,
                        const int32_t *w_row, const int32_t *row_ptr, const int32_t *src, int64_t n_dst, float scale,
                        float *out, void *stream);
int snet_conv_bwd_fused(const snet_fused_plan *plan, const float *x, const float *sh, const float *dsh,
                        const float *h2, const int32_t *w_row, const int32_t *row_ptr, const int32_t *src,
                        const int32_t *tile_ptr, const int32_t *tile_node, int64_t n_tiles, float scale,
                        const float *g_out, float *g_xe, float *g_h2, const float *emb, float *g_emb, float *g_vec,
                        const float *x_rowmax, const float *g_rowmax, void *stream);
/* The same reverse pass for hosts that differentiate with respect to the harmonics THEMSELVES -- the reference's plug-in point
 * hands `edge_attr` to autograd (sevenn/nn/convolution.py:118-141, flash_helper.py:33-48): g_sh[E, nsh] is OVERWRITTEN with
 * dE/dY of every edge; no dsh / g_vec (the caller chains through its own spherical-harmonics module). */
int snet_conv_bwd_fused_sh(const snet_fused_plan *plan, const float *x, const float *sh, const float *h2, const int32_t *w_row,
                           const int32_t *row_ptr, const int32_t *src, const int32_t *tile_ptr, const int32_t *tile_node,
                           int64_t n_tiles, float scale, const float *g_out, float *g_xe, float *g_h2, const float *emb,
                           float *g_emb, float *g_sh, const float *x_rowmax, const float *g_rowmax, void *stream);
int snet_fused_plan_has_mlp_tail(const snet_fused_plan *plan);
/* ---- radial gradient by FORWARD TANGENT --------------------------------------------------------------------------------
 * The radial branch of an edge is a function of ONE scalar, |r_e|: emb(|r|) -> h2 -> w = h2 W2.  So all the reverse pass needs of
 * it is dE/d|r_e| = sum_k g_w[e,k] w'_e[k] with w'_e = h2'_p W2 and h2'_p = d h2_p / d|r| (one 64-float row per radial row and
 * layer).  w' is a second product on the W2 fragments the reverse kernel reads for w anyway, its contraction with the fresh g_w
 * tiles one multiply-add per register: the kernel then needs no operand split of g_w, no g_h2 = g_w W2^T products, no second W2
 * image in LDS and no hidden-layer tail, and nothing is left for snet_edge_embed_bwd to do.
 *   snet_edge_embed_tangent                  demb[n_rows, nb] = d emb / d|r| of row i's edge (edge_of_row[i]; NULL: edge i)
 *   snet_radial_mlp_hidden_fwd_layers_tangent  snet_radial_mlp_hidden_fwd_layers (h2[l] bit for bit) plus h2d[l][R,64] = d h2 / d|r|;
 *                                            every radial activation, any n_basis <= 32
 *   snet_conv_bwd_fused_tangent              snet_conv_bwd_fused without g_h2 / emb / g_emb: g_vec[E,3] ACCUMULATES the spherical part
 *                                            (as before) AND dE/d|r_e| r_e / |r_e|; g_xe as snet_conv_bwd_fused writes it, bit for bit.
 *                                            h2d rows are read like h2 rows (w_row); edge_vec[E,3] as snet_edge_embed_fwd took it. */
 /* snet_fused_plan_prefers_tangent() != 0: this shape's reverse pass is faster in tangent mode (every shape has both kernels; the
 * lmax-3 middle-layer shapes, which sit at the register limit, keep the reverse-mode one).  Both hosts follow it per layer. */
int snet_fused_plan_prefers_tangent(const snet_fused_plan *plan);
int snet_edge_embed_tangent(const snet_edge_params *p_host, const float *coeffs_host, const float *edge_vec,
                            const int32_t *edge_of_row, int64_t n_rows, float *demb, void *stream);
int snet_radial_mlp_hidden_fwd_layers_tangent(const snet_mlp_plan *const *plans, int32_t n_layers, const float *emb, const float *demb,
                                              int64_t n_rows, float *const *h2, float *const *h2d, void *stream);
int snet_conv_bwd_fused_tangent(const snet_fused_plan *plan, const float *x, const float *sh, const float *dsh, const float *h2,
                                const float *h2d, const int32_t *w_row, const int32_t *row_ptr, const int32_t *src,
                                const int32_t *tile_ptr, const int32_t *tile_node, int64_t n_tiles, float scale, const float *g_out,
                                float *g_xe, const float *edge_vec, float *g_vec, const float *x_rowmax, const float *g_rowmax,
                                void *stream);
/* ---- first interaction layer from per-atom radial moments --------------------------------------------------------------
 * Layer 0's source rows depend on the species alone, x[src(e)] = table[species(src(e))] (node embedding -> SI1, the species-only
 * tables of both hosts), its inputs are scalars and its paths (0, l -> l) with unit diagonal coupling.  Per edge the message is
 * scale Y_e[q] table[s,u] sum_k h2_e[k] W2[k, l(q) mul + u], and the sum over a node's edges commutes with the W2 product.  With
 *   B_l[(s,k), u] = W2[k, l mul + u] table[s, u] scale        (folded in fp64 at plan creation, rounded once)
 * reverse:  Bm_i[q,s,k] = sum_u g_out_i[q,u] B_l(q)[(s,k),u]       (one grouped split-precision GEMM), then per edge, in fp32 FMAs,
 *           dE/dY_e[q] = sum_k h2_e[k] Bm_i[q,slot(e),k] and dE/d|r_e| = sum_q Y_e[q] sum_k h2d_e[k] Bm_i[q,slot(e),k],
 *           both ACCUMULATED into g_vec[E,3] as snet_conv_bwd_fused_tangent does (dsh, r_e / |r_e|); no atomics.
 * The W2 product runs once per atom instead of once per edge, and nothing is an fp16 operand: no x_rowmax / g_rowmax.  (The forward
 * pass keeps snet_conv_fwd_fused: its moments form missed the accuracy bar)
 *   plan       conv = the layer's shape (refused unless dx = mul scalars, wn = (lmax + 1) mul, dout = nsh mul, 16 | mul <= 512,
 *              lmax <= 3: the CALLER vouches for the paths being (0, l -> l) in l order); W2_host[64, wn] and scale as the fused
 *              kernels take them; table_host[n_slots, mul], row s = the source row of the species in slot s; 1 <= n_slots <= 4
 *   species_slot  int32[n_species] (device): slot of each species in [0, n_slots); species of an edge = types[src[e]]
 *   h2 / h2d / w_row / row_ptr / src / sh / dsh / edge_vec: as snet_conv_bwd_fused_tangent; n_nodes destination rows
 *   scratch    snet_layer0_scratch_size(plan, n_nodes) = n_nodes nsh n_slots 64 floats (Bm), owned by the caller                */
typedef struct snet_layer0_plan snet_layer0_plan;
int snet_layer0_plan_create(const snet_conv_plan *conv, const float *W2_host, const float *table_host, float scale,
                            int32_t n_slots, snet_layer0_plan **plan);
void snet_layer0_plan_destroy(snet_layer0_plan *plan);
/* the fold itself, on the host (what the plan packs): bt_host[mul, 64 n_slots] = B_l^T, bt[u, s 64 + k] = W2[k, l mul + u] table[s, u] scale */
int snet_layer0_fold(const float *W2_host, int32_t wn, int32_t mul, const float *table_host, float scale, int32_t n_slots, int32_t l,
                     float *bt_host);
int64_t snet_layer0_scratch_size(const snet_layer0_plan *plan, int64_t n_nodes);
int snet_layer0_conv_bwd(const snet_layer0_plan *plan, const float *g_out, const float *h2, const float *h2d, const int32_t *w_row,
                         const int32_t *row_ptr, const int32_t *src, const int32_t *types, const int32_t *species_slot,
                         const float *sh, const float *dsh, const float *edge_vec, int64_t n_nodes, float *scratch, float *g_vec,
                         void *stream);
/* ---- scalar-output (last) interaction layer: the whole reverse pass in one source-grouped launch ------------------------------
 * Every path is (l, l -> 0) with the diagonal coupling c_l, so g_h (d/d source row) and g_vec (d/d r_e) are derivatives of one
 * bilinear form  B = scale sum_e sum_{l,u} g_out[center(e)][l,u] w_e[l,u] c_l sum_a x[src(e)][l,u,a] Y_e[l,a],  w_e = h2_e W2.
 * A wave takes one SOURCE row j, keeps x[j] on chip and walks j's out-edges (col_ptr / snet_edges_by_source) in tiles of 16:
 *   t_e = scale c_l w_e g_out[center(e)];  g_x[j][l,u,a] = sum_e t_e Y_e[l,a];  dB/dY_e[l,a] = sum_u t_e x[j][l,u,a];
 *   dB/d|r_e| = sum_{l,u} scale c_l w'_e g_out[center(e)] sum_a x[j][l,u,a] Y_e[l,a],  w'_e = h2d_e W2
 * -- one pair of W2 products per edge (two-term fp16 operands, fp32 accumulate) where snet_conv_bwd_fused_tangent +
 * snet_conv_fwd_fused of the transposed shape run two, no dx-float gather per edge, no operand that depends on g_out (hence no
 * x_rowmax / g_rowmax).  g_vec[eperm[e']] is ADDED to (plain read-modify-write: an edge has one source); g_x rows [row_a, row_b)
 * are WRITTEN whole, the dead ranges of snet_conv_plan_transposed as zeros.  Fixed summation order: two launches give the same bits,
 * and a call over [a, b) then [b, c) the bits of one over [a, c).
 *   plan     conv = the layer's shape: refused unless its transposed product exists, its column factors are 1 / sqrt(2 l + 1) in
 *            runs of multiples of 16 for l = 0, 1, .. <= 3 (one path (l, l -> 0) per l, in l order: the CALLER vouches for the diagonal
 *            coupling and for the x blocks following each other in l order around the dead ranges --
 *            sevennet_amd.model_spec.lastlayer_merged_eligible) and a kernel for these multiplicities is compiled in;
 *            W2_host[64, wn] as the fused kernels take it (the column factors are applied here)
 *   x, g_out, h2, h2d, sh[E,nsh], dsh[E,3 nsh], edge_vec[E,3]: as snet_conv_bwd_fused_tangent (sh / dsh / edge_vec / g_vec in the
 *            destination-grouped edge order); col_ptr[n_total + 1], center_t, w_row_t, eperm: as snet_conv_fwd_fused of the
 *            transposed shape takes them (col_ptr is NOT offset by row_a)                                                        */
typedef struct snet_lastlayer_plan snet_lastlayer_plan;
int snet_lastlayer_plan_create(const snet_conv_plan *conv, const float *W2_host, snet_lastlayer_plan **plan);
void snet_lastlayer_plan_destroy(snet_lastlayer_plan *plan);
int snet_lastlayer_conv_bwd(const snet_lastlayer_plan *plan, const float *x, const float *g_out, const float *sh, const float *dsh,
                            const float *edge_vec, const float *h2, const float *h2d, const int32_t *col_ptr,
                            const int32_t *center_t, const int32_t *w_row_t, const int32_t *eperm, int64_t row_a, int64_t row_b,
                            float scale, float *g_x, float *g_vec, void *stream);
/* g_xe[E,dx] of snet_conv_bwd_fused is an intermediate with its own row layout: the 16-channel chunks of a row are stored in
 * the order the kernel produces them ([x block][channel tile][component]: each (block, tile) writes one contiguous run per
 * edge instead of half cache lines).  chunk_pos[s] (dx / 16 entries, host) = position of standard chunk s in the row;
 * snet_segment_sum_rows_chunked (chunk_pos on the DEVICE) sums such rows per source atom and returns standard order. */
int snet_fused_plan_gxe_chunks(const snet_fused_plan *plan, int32_t *chunk_pos, int32_t capacity);
int snet_segment_sum_rows_chunked(const float *x, const int32_t *seg_ptr, const int32_t *perm, int64_t n_seg, int32_t dim,
                                  const int32_t *chunk_pos, float *out, void *stream);
/* out[r] = max_k |x[r,k]| for r < n_rows.  The f16x3 reverse kernel (terms = 4) scales its fp16 operand g_w per edge by a
 * power of two derived from a BOUND of |g_w| -- (sum |C|) max|g_out[node]| max|x[src]| max|Y_e| -- so that no entry can
 * overflow fp16 whatever the model's feature magnitudes are; the two row maxima come from this kernel. */
int snet_row_absmax(const float *x, int64_t n_rows, int32_t dim, float *out, void *stream);
/* the same for n (1 .. 8) matrices x[j][n_rows[j], dims[j]] -> out[j] in one launch (both hosts: the source-row bounds of all
 * interaction layers at the start of the reverse pass); matrices with n_rows[j] <= 0 are skipped */
int snet_row_absmax_multi(const float *const *x, const int64_t *n_rows, const int32_t *dims, float *const *out, int32_t n,
                          void *stream);
/* out[r] = mult * ||x[r,:]||_2.  With mult = the largest row norm of a linear map's matrix this bounds every entry of
 * the map's output row (Cauchy-Schwarz): both hosts bound g_out = SI2^T g_y this way from the 5x narrower g_y instead
 * of reading g_out[N, dmid] once more (g_rowmax of snet_conv_bwd_fused may be ANY upper bound of max|g_out[node]|). */
int snet_row_norm2(const float *x, int64_t n_rows, int32_t dim, float mult, float *out, void *stream);
/* per-edge gradients given g_out[n_dst,dout]: g_w[E,wn] (overwritten), g_sh[E,nsh] (ACCUMULATED,
 * so one buffer collects all layers) and, if g_xe != NULL, this edge's contribution to the gradient
 * of its source row, g_xe[E,dx] (overwritten; sum it per source node with snet_segment_sum_rows --
 * 1.9 KB/edge written once instead of the 12.5 KB/edge g_out gathers of snet_conv_bwd_node).    */
int snet_conv_bwd_edge(const snet_conv_plan *plan, const float *x, const float *sh, const float *w,
                       const int32_t *w_row, const int32_t *row_ptr, const int32_t *src, int64_t n_dst, float scale,
                       const float *g_out, float *g_w, float *g_xe, float *g_sh, void *stream);
/* same, but the spherical-harmonic gradient is contracted with dsh[E,nsh,3] (snet_edge_embed_fwd)
 * inside the kernel and ACCUMULATED into g_vec[E,3]: 3 instead of nsh values per edge cross the
 * wavefront reduction.  This is the variant the whole-model engine uses. */
int snet_conv_bwd_edge_vec(const snet_conv_plan *plan, const float *x, const float *sh, const float *dsh,
                           const float *w, const int32_t *w_row, const int32_t *row_ptr, const int32_t *src,
                           int64_t n_dst, float scale, const float *g_out, float *g_w, float *g_xe, float *g_vec,
                           void *stream);
/* source-node gradient g_x[n_src,dx] (overwritten) via the source-sorted edge
 * permutation: col_ptr[n_src+1], eperm[E] (edge ids grouped by source), dst[E].
 * Deterministic replacement of the scatter-add autograd performs for x[src]. */
int snet_conv_bwd_node(const snet_conv_plan *plan, const float *sh, const float *w, const int32_t *w_row,
                       const int32_t *col_ptr,
                       const int32_t *eperm, const int32_t *dst, int64_t n_src, float scale,
                       const float *g_out, float *g_x, void *stream);

/* out[s,:] = sum_{k in [seg_ptr[s], seg_ptr[s+1])} x[perm[k],:]  (deterministic segmented row sum;
 * with col_ptr/eperm it turns g_xe[E,dx] into g_x[n_src,dx], the reverse of the x[src] gather) */
int snet_segment_sum_rows(const float *x, const int32_t *seg_ptr, const int32_t *perm, int64_t n_seg, int32_t dim,
                          float *out, void *stream);

/* ---- a5: equivariant gate ------------------------------------------------
 * replaces EquivariantGate.forward, sevenn/nn/equivariant_gate.py:57-59     */
typedef struct snet_gate_seg {
  int32_t kind;     /* 0: scalars -> act(s)*cst ; 1: gated[m,u] * (act(gate[u])*cst) */
  int32_t in_off;   /* offset in the gate input row */
  int32_t out_off;  /* offset in the output row */
  int32_t mul;
  int32_t l;
  int32_t gate_off; /* kind 1: offset of this segment's gate scalars in the input row */
  int32_t act;      /* 0 silu, 1 tanh */
  float cst;        /* normalize2mom constant of act */
} snet_gate_seg;
#define SNET_MAX_GATE_SEGS 16
/* addend (nullable, [n_nodes, dim_in]): the self-connection term of SelfConnectionOutro
 * (self_connection.py:118-138); y += addend is applied in place before the gate, so y holds the gate
 * input that snet_gate_bwd needs. */
int snet_gate_fwd(float *y, const float *addend, float *out, int64_t n_nodes, int32_t dim_in, int32_t dim_out,
                  const snet_gate_seg *segs_host, int32_t n_segs, void *stream);
int snet_gate_bwd(const float *y, const float *g_out, float *g_y, int64_t n_nodes, int32_t dim_in,
                  int32_t dim_out, const snet_gate_seg *segs_host, int32_t n_segs, void *stream);
/* snet_gate_bwd that also returns row_norm[n] = norm_mult * ||g_y[n]||_2 (nullable), the bound snet_row_norm2 gives: the rows
 * are in registers anyway, one pass over g_y less per layer. */
int snet_gate_bwd_norm(const float *y, const float *g_out, float *g_y, int64_t n_nodes, int32_t dim_in, int32_t dim_out,
                       const snet_gate_seg *segs, int32_t n_segs, float norm_mult, float *row_norm, void *stream);

/* ---- a6: species embedding (one-hot @ W == table lookup) ------------------
 * replaces OnehotEmbedding + first IrrepsLinear, node_embedding.py:44-53,
 * model_build.py:505-521.  out[n,:] = table[types[n],:]                     */
int snet_embed_rows(const float *table, const int32_t *types, float *out, int64_t n_nodes, int32_t dim,
                    void *stream);

/* ---- a4.1 and friends: y += x ; column permutation (layout conversion) --- */
int snet_add_inplace(float *y, const float *x, int64_t n, void *stream);
/* y[r, :] += bias[:] for r < n_rows: the constant a multi-modal linear's one-hot inputs contribute for a
 * fixed fidelity channel (IrrepsLinear._patch_modal_to_data, sevenn/nn/linear.py:72-92) */
int snet_add_row_bias(float *y, const float *bias, int64_t n_rows, int32_t dim, void *stream);
int snet_permute_cols(const float *x, const int32_t *col_idx, float *out, int64_t n_rows, int32_t dim,
                      void *stream); /* out[r,c] = x[r,col_idx[c]] */

/* ---- a7/a8: per-species rescale + total energy ---------------------------
 * replaces (SpeciesWise)Rescale.forward scale.py:53-56,155-162 and AtomReduce
 * linear.py:127-141.  e_atom[n] = e[n]*scale[t]+shift[t] (n_scale==1: global);
 * *energy (device double) = sum over the first n_nodes rows (deterministic).  */
int snet_rescale_reduce(const float *e_scaled, const int32_t *types, const float *scale, const float *shift,
                        int32_t n_scale, int64_t n_nodes, float *e_atom, double *energy, void *stream);

/* out[i] = in[i] + delta over n int32 entries (tile pointers of a sub-list of the reverse kernels' tile list) */
int snet_i32_shift(const int32_t *in, int32_t delta, int32_t *out, int64_t n, void *stream);

/* Folded readout (a3 + a7 + a8 in one pass): the reference's two readout linears (reduce_input_to_hidden,
 * reduce_hidden_to_energy; sevenn/model_build.py, nn/linear.py:94-100) have no nonlinearity between them, so
 * a host may fold them to one vector v[dim] and constant c (fp64, at load time).  For the first n rows:
 * e_atom[i] = (x[i] . v + c) * scale[t] + shift[t] with the dot product and the rescale in fp64,
 * *energy (device double) = their deterministic fp64 sum.  v is a DEVICE pointer to doubles.  */
int snet_readout_energy(const float *x, int64_t n_nodes, int32_t dim, const double *v, double c, const int32_t *types,
                        const float *scale, const float *shift, int32_t n_scale, float *e_atom, double *energy,
                        void *stream);
/* its reverse: g_x[i, k] = scale[type_i] * v[k]  (dE/dx of the folded readout)  */
int snet_readout_grad(const double *v, int32_t dim, const int32_t *types, const float *scale, int32_t n_scale,
                      int64_t n_nodes, float *g_x, void *stream);

/* ---- a9/a11: forces and virial from dE/d edge_vec --------------------------
 * replaces ForceStressOutputFromEdge.forward force_output.py:189-228 and the
 * host loops of pair_e3gnn.cpp:210-270.  Over n_nodes rows (locals + ghosts):
 *   F[i]   = sum_{e: center(e)=i} g[e] - sum_{e: neighbor(e)=i} g[e]
 *   vir[i] = -sum_{e: neighbor(e)=i} (rx gx, ry gy, rz gz, rx gy, ry gz, rz gx)
 * in-edges via row_ptr (edges sorted by center), out-edges via col_ptr/eperm.
 * virial_atom may be NULL; virial_total[6] (device double) may be NULL.       */
int snet_edge_force(const float *g_vec, const float *edge_vec, const int32_t *row_ptr, const int32_t *col_ptr,
                    const int32_t *eperm, int64_t n_nodes, int64_t n_edges, float *forces, float *virial_atom,
                    double *virial_total, void *stream);

/* ---- batched evaluation: per-system fp64 reductions ------------------------
 * The atoms of B systems are contiguous segments seg_ptr[B+1] (device int32, seg_ptr[0] = 0, seg_ptr[B] = n_nodes) of
 * one graph whose edges never cross systems.  The variants below compute exactly what their single-total namesakes
 * compute per atom, keep the fp64 per-atom values and sum them per segment in a fixed order (AtomReduce per graph,
 * sevenn/nn/linear.py:127-141; the per-graph virial scatter of force_output.py:213-228):
 *   energy_seg[B] / virial_seg[B,6] (device double), and *_total (device double, may be NULL) = their fixed-order sum.
 * Deterministic: two runs give bit-identical results.  A segment may hold one atom without edges.  */
int snet_readout_energy_seg(const float *x, int64_t n_nodes, int32_t dim, const double *v, double c, const int32_t *types,
                            const float *scale, const float *shift, int32_t n_scale, const int32_t *seg_ptr, int32_t n_seg,
                            float *e_atom, double *energy_seg, double *energy_total, void *stream);
int snet_rescale_reduce_seg(const float *e_scaled, const int32_t *types, const float *scale, const float *shift,
                            int32_t n_scale, int64_t n_nodes, const int32_t *seg_ptr, int32_t n_seg, float *e_atom,
                            double *energy_seg, double *energy_total, void *stream);
int snet_edge_force_seg(const float *g_vec, const float *edge_vec, const int32_t *row_ptr, const int32_t *col_ptr,
                        const int32_t *eperm, int64_t n_nodes, int64_t n_edges, const int32_t *seg_ptr, int32_t n_seg,
                        float *forces, float *virial_atom, double *virial_seg, double *virial_total, void *stream);

/* ---- a12: halo pack / unpack ---------------------------------------------
 * replaces PairE3GNNParallel::pack_forward_comm_gnn / unpack_reverse_comm_gnn,
 * pair_e3gnn_parallel.cpp:747-911 (index_select / scatter / scatter-add).
 *   gather:      out[i,:]      = x[idx[i],:]
 *   scatter_add: y[idx[i],:]  += x[i,:]       (idx unique within one call)   */
int snet_gather_rows(const float *x, const int32_t *idx, float *out, int64_t n_idx, int32_t dim, void *stream);
int snet_scatter_add_rows(const float *x, const int32_t *idx, float *y, int64_t n_idx, int32_t dim,
                          void *stream);

/* ---- f1: neighbor list on the GPU ---------------------------------------------
 * replaces the host graph build unlabeled_atoms_to_graph / _graph_build_{ase,matscipy}
 * (sevenn/train/dataload.py:32-129) and yields the CSR-by-center edge layout directly.
 * cell_host[9] row-major lattice vectors (HOST), positions / wrapped positions fp64 (device).
 * pbc_host[3] (HOST, nullable = fully periodic): open axes are neither wrapped nor imaged; frac_range_host[6] (HOST,
 * required with an open axis) = lower (3) and upper (3) bound of the atoms' fractional coordinates, read for open axes.
 * A periodic cell may be thinner than the cutoff (it then meets itself through ceil(cutoff / height) images).
 * Sequence: snet_nl_grid (bins per axis) -> snet_nl_bin (wrapped positions, image index, bin id)
 * -> [caller sorts atoms by bin id: order[], bin_start[]] -> snet_nl_count -> [exclusive scan:
 * row_ptr] -> snet_nl_fill (src, center, edge_vec fp32, optional image shifts).              */
int snet_nl_grid(const double *cell_host, double cutoff, const int32_t *pbc_host, const double *frac_range_host,
                 int32_t *nbins_host);
int snet_nl_bin(const double *cell_host, double cutoff, const int32_t *pbc_host, const double *frac_range_host,
                const double *pos, int64_t n_atoms, double *wpos, int32_t *wrap, int32_t *cell_id, void *stream);
int snet_nl_count(const double *cell_host, double cutoff, const int32_t *pbc_host, const double *frac_range_host,
                  const double *wpos, const int32_t *cell_id, const int32_t *order, const int32_t *bin_start,
                  int64_t n_atoms, int32_t *count, void *stream);
int snet_nl_fill(const double *cell_host, double cutoff, const int32_t *pbc_host, const double *frac_range_host,
                 const double *wpos, const int32_t *wrap, const int32_t *cell_id, const int32_t *order,
                 const int32_t *bin_start, int64_t n_atoms, const int32_t *row_ptr, int32_t *src, int32_t *center,
                 float *edge_vec, int32_t *shifts, void *stream);

/* Batched neighbor list of B small systems (one count launch, one fill launch): atoms of system s are rows
 * [atom_ptr[s], atom_ptr[s+1]) of pos[n_atoms,3] (fp64); cells[B,9] (row-major lattice vectors, fp64) and pbc[B,3]
 * (int32) per system, all on the device.  Same conventions and CSR-by-center output as snet_nl_fill (every ordered pair
 * within the cutoff, no self edge, edge_vec = r_j - r_i + S.cell in fp64 stored as fp32, open axes neither wrapped nor
 * imaged, a zero cell row of an open axis padded); indices are global, shifts (may be NULL) relative to the given
 * positions.  One lane per center atom over the atoms of its own system: O(n_s^2) work per system.  A system whose cell is
 * singular after padding, or thinner than 1/64 of the cutoff along a periodic axis, gets no edges (the host routes it
 * elsewhere).  snet_batch_nl_count writes count[n_atoms]; the caller scans it into row_ptr for snet_batch_nl_fill.  */
int snet_batch_nl_count(const double *pos, const int32_t *atom_ptr, int32_t n_sys, const double *cells, const int32_t *pbc,
                        int64_t n_atoms, double cutoff, int32_t *count, void *stream);
int snet_batch_nl_fill(const double *pos, const int32_t *atom_ptr, int32_t n_sys, const double *cells, const int32_t *pbc,
                       int64_t n_atoms, double cutoff, const int32_t *row_ptr, int32_t *src, int32_t *center,
                       float *edge_vec, int32_t *shifts, void *stream);

/* ---- batched FIRE relaxation step (fixed cell, unit masses) -------------------------------------
 * One step of FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201 (2006), as ASE's optimizer states it) for n_sys systems in ONE
 * launch: the atoms of system s are rows [seg_ptr[s], seg_ptr[s+1]) (device int32, as Graph.seg_ptr) of pos / vel (fp64
 * [n_atoms,3], updated in place) and of forces (fp32 [n_atoms,3], as the engine returns them; forces_extra, fp64 [n_atoms,3] or
 * NULL, is added to them).  Per-system state on the device: dt, alpha (fp64 [n_sys]), n_pos, active, n_steps (int32 [n_sys]).
 * For every system with active == 1, in fp64 with F the summed forces:
 *   fm = max_i |F_i|; fmax_sys[s] = fm; if fm < fmax: active = 0 and nothing else changes (converged at these positions)
 *   P = sum F.v;  P > 0: v = (1 - alpha) v + alpha F / |F| |v|; if n_pos > n_min: dt = min(dt f_inc, dt_max), alpha *= f_alpha;
 *                        n_pos += 1
 *                 else:  v = 0, alpha = alpha_start, dt *= f_dec, n_pos = 0
 *   v += dt F;  dr = dt v, scaled to length max_step if longer (norm over the whole system);  pos += dr;  n_steps += 1
 * Systems with active == 0 are not touched.  *n_active (device int32) receives the number of systems still active.
 * dt_start is the value the caller initialised dt[] with (range-checked with the others, not read by the step).
 * One workgroup per system, fp64 sums in a fixed order: two runs give identical bits.  Calls on one device must follow
 * each other in stream order.  */
int snet_fire_step(double *pos, double *vel, const float *forces, const double *forces_extra, int64_t n_atoms,
                   const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                   int32_t *n_steps, double *fmax_sys, int32_t *n_active, double fmax, double dt_start, double dt_max,
                   int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha, double max_step, void *stream);
/* snet_fire_step_fixed: the same step with components held fixed.  hold (device int32 [n_atoms], not NULL): bit k (k = 0, 1, 2) of
 * hold[i] & 7 says that Cartesian component k of atom i is held, so 7 holds the whole atom (the name keeps it apart from the 0/1
 * `fixed` array of snet_neb_forces).  For a held component (i, k): its force is taken as 0 by selection, not by multiplication -- a
 * non-finite force there poisons nothing -- and that 0 is what enters every sum of the step (max |F_i|^2, F.v, |F|^2, |v|^2,
 * |dt v|^2); its velocity is taken as 0 whatever vel holds on entry and is stored as 0 by a step that moves; pos[3 i + k] is never
 * written.  So fmax_sys and convergence refer to the free components only, and a system whose components are all held is found
 * converged (fm = 0 < fmax) on the first launch with no step counted.  With hold all zero every output equals snet_fire_step's bit
 * for bit.  The arrival word is the one of snet_fire_step: calls of the two on one device follow each other in stream order.  */
int snet_fire_step_fixed(double *pos, double *vel, const float *forces, const double *forces_extra, int64_t n_atoms,
                         const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                         int32_t *n_steps, double *fmax_sys, int32_t *n_active, double fmax, double dt_start, double dt_max,
                         int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha, double max_step,
                         const int32_t *hold, void *stream);

/* ---- batched variable-cell FIRE relaxation step (unit masses) -----------------------------------
 * One step of FIRE over the atoms AND the cell of n_sys systems in ONE launch: the rule of ASE's UnitCellFilter (Tadmor et al.,
 * Phys. Rev. B 59, 235 (1999): atoms in the frame of a reference cell plus the deformation gradient) under the FIRE of
 * snet_fire_step.  Arrays as snet_fire_step, and per system: cell (fp64 [n_sys,9], row-major lattice vectors, updated in place),
 * cell0 (the reference cell, read only), vel_cell (fp64 [n_sys,9], updated in place), virial (fp64 [n_sys,6], the engine's
 * virial_per_system: order xx,yy,zz,xy,yz,zx, stress = -virial / volume; virial_extra, fp64 [n_sys,6] or NULL, is added to it),
 * status (int32 [n_sys]: the caller's 0 while running, 1 written when converged, 2 when the guard below fails).
 * For every system with active == 1 and n atoms, in fp64, with C the cell, C0 the reference cell and f the summed forces:
 *   F = (C0^-1 C)^T  (so C = C0 F^T);  V = |det C|;  W = the symmetric 3x3 of the summed virials - scalar_pressure V I
 *   cell force:  G = W F^-T;  if hydrostatic_strain: G = I tr(G)/3;  G *= M elementwise, M the symmetric 0/1 matrix of
 *                cell_mask_bits (bit k = Voigt flag k of xx,yy,zz,yz,xz,xy);  if constant_volume: G -= I tr(G)/3;  G /= n
 *   atom forces: g_i = f_i F  (row vector times matrix)
 *   The generalised coordinates are the n rows s_i = r_i F^-T followed by the three rows of n F, their velocities vel[n,3] and
 *   vel_cell[3,3], their forces g_i and the rows of G.  Over these n + 3 rows exactly the step of snet_fire_step:
 *     fm = largest row norm of the forces; fmax_sys[s] = fm; if fm < fmax: active = 0, status = 1, nothing else changes
 *     P, |g|, |v| over all rows -> the velocity mixing and the dt / alpha / n_pos bookkeeping;  v += dt g;  dq = dt v, scaled to
 *     length max_step if longer (norm over all rows)
 *   move:  s_i += dq_i;  F_new = F + dQ / n (dQ the cell rows of dq);  C_new = C0 F_new^T;  r_i = s_i F_new^T;  n_steps += 1
 *   guard, before anything but fmax_sys is written:  if the step length or an entry of F_new is not finite, det F_new <= 0, or a
 *   face-to-face height of C_new is below min_height (the batched neighbour kernels take heights down to cutoff / 64):
 *   active = 0, status = 2, and pos, cell, both velocities, dt, alpha, n_pos, n_steps keep their bits.
 * Systems with active == 0 are not touched.  *n_active (device int32) receives the number of systems still active.
 * One 256-thread workgroup per system, fp64 sums in a fixed order: two runs give identical bits.  Calls on one device must follow
 * each other in stream order (the arrival word is apart from snet_fire_step's).  */
int snet_fire_cell_step(double *pos, double *vel, double *cell, double *vel_cell, const double *cell0, const float *forces,
                        const double *forces_extra, const double *virial, const double *virial_extra, int64_t n_atoms,
                        const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                        int32_t *n_steps, int32_t *status, double *fmax_sys, int32_t *n_active, double fmax, double dt_start,
                        double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha, double max_step,
                        double scalar_pressure, int32_t cell_mask_bits, int32_t hydrostatic_strain, int32_t constant_volume,
                        double min_height, void *stream);
/* snet_fire_cell_step_fixed: the same step with whole atoms held.  hold as for snet_fire_step_fixed, read per atom: an atom with
 * hold[i] & 7 != 0 is held (a rule per component has no clean form under a sheared F; the Python driver refuses such masks).  Its
 * force counts as 0: g_i = 0 in every sum, by selection on g_i = f_i F (a non-finite force there poisons nothing, and a free atom's
 * g_i is formed exactly as without a mask); its reference-frame velocity is taken as 0 and stored as 0.  Its position still goes through r_i = (r_i F^-T) F_new^T: a held atom keeps its fractional
 * coordinates and moves with the cell, which is what ASE's UnitCellFilter does with FixAtoms.  The virial and the cell force are
 * untouched, and the n of G /= n and F_new = F + dQ / n stays the system's full atom count (ASE: len(atoms)).  With hold all zero
 * every output equals snet_fire_cell_step's bit for bit; the arrival word is the one of snet_fire_cell_step.  */
int snet_fire_cell_step_fixed(double *pos, double *vel, double *cell, double *vel_cell, const double *cell0, const float *forces,
                              const double *forces_extra, const double *virial, const double *virial_extra, int64_t n_atoms,
                              const int32_t *seg_ptr, int32_t n_sys, double *dt, double *alpha, int32_t *n_pos, int32_t *active,
                              int32_t *n_steps, int32_t *status, double *fmax_sys, int32_t *n_active, double fmax, double dt_start,
                              double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha,
                              double max_step, double scalar_pressure, int32_t cell_mask_bits, int32_t hydrostatic_strain,
                              int32_t constant_volume, double min_height, const int32_t *hold, void *stream);

/* ---- batched nudged-elastic-band forces ----------------------------------------------------------
 * The NEB forces of the moving images of n_bands bands in ONE launch: the improved tangent of Henkelman and Jonsson, J. Chem.
 * Phys. 113, 9978 (2000), and the climbing image of Henkelman, Uberuaga and Jonsson, J. Chem. Phys. 113, 9901 (2000).  The flat
 * arrays hold the INTERIOR images only: band b owns images [img_ptr[b], img_ptr[b+1]) (device int32 [n_bands+1]) of the n_img
 * moving images, image j owns rows [seg_ptr[j], seg_ptr[j+1]) (device int32 [n_img+1]) of pos (fp64 [n_atoms,3]), forces (fp32
 * [n_atoms,3]; forces_extra, fp64 [n_atoms,3] or NULL, is added in fp64), fixed (int32 [n_atoms] or NULL) and f_neb (fp64
 * [n_atoms,3], written); all images of a band have the same n_b atoms in the same order.  energy (fp64 [n_img]; energy_extra,
 * fp64 [n_img] or NULL, is added).  The two endpoints of band b are rows [end_ptr[b], end_ptr[b] + n_b) (initial) and the n_b
 * rows after them (final) of pos_end (fp64 [n_end,3]; end_ptr device int32 [n_bands+1]), their energies e_end[2 b], e_end[2 b + 1]
 * (fp64); the previous image of a band's first interior image is the initial endpoint, the next image of its last one the final
 * endpoint.  Per band: cells and inv_cells (fp64 [n_bands,9], row-major lattice vectors with the zero rows of open axes padded to
 * an invertible matrix, and its inverse), pbc (int32 [n_bands,3]), k (fp64 [n_bands], the spring constant), active and status
 * (int32 [n_bands]), imax (int32 [n_bands], written).
 * For every image i of a band with active == 1, in fp64, with R the positions, F the summed forces and E the summed energies:
 *   F of an atom with fixed != 0 is zero before anything else, and so is its f_neb
 *   mic(d):  s = d inv(cell);  s_k -= rint(s_k) on the periodic axes;  d = s cell  (row vectors; without a periodic axis d is
 *            left as it is).  This is the shortest image whenever the true displacement is shorter than half the smallest
 *            face-to-face height of the cell (|s_k| <= |d| / h_k): the documented domain, not checked.
 *   t+ = mic(R_next - R_i),  t- = mic(R_i - R_prev);  Ep, Ei, Em the energies of the next, this and the previous image
 *   Ep > Ei > Em: tau = t+;   Ep < Ei < Em: tau = t-;   otherwise, with dmax = max(|Ep - Ei|, |Em - Ei|) and dmin their min:
 *   tau = t+ dmax + t- dmin if Ep > Em, else tau = t+ dmin + t- dmax (exact ties land here);  tau is then normalised over all
 *   3 n_b components, a zero norm leaves tau = 0
 *   f_neb = F - (F.tau) tau + k (|t+| - |t-|) tau
 *   imax[b] = the interior image of highest energy (index within the band, lowest index on ties); with climb != 0 that image gets
 *   f_neb = F - 2 (F.tau) tau instead, and no spring
 * A band with active != 1 is skipped: its f_neb rows are written as zero, nothing else of it is touched.  If one of Ei, Ep, Em,
 * |t+|^2, |t-|^2, |tau|^2 (before normalisation) or F.tau of an image is not finite, status[b] = 2 and active[b] = 0 are written
 * (by every workgroup that finds it so) and that image's f_neb rows are zero: a snet_fire_step launch that follows leaves the
 * band where it was.  Images of unequal size within a band, or endpoint rows outside pos_end, give status[b] = 3 the same way.
 * One 256-thread workgroup per moving image, fp64 sums in a fixed order: two runs give identical bits.  With one segment per
 * band (the bands' row offsets as its seg_ptr) snet_fire_step on f_neb is the single FIRE that ASE runs over NEB(images).  */
int snet_neb_forces(const double *pos, const float *forces, const double *forces_extra, const double *energy,
                    const double *energy_extra, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_img, const int32_t *img_ptr,
                    int32_t n_bands, const double *pos_end, const int32_t *end_ptr, int64_t n_end, const double *e_end,
                    const double *cells, const double *inv_cells, const int32_t *pbc, const int32_t *fixed, const double *k,
                    int32_t climb, int32_t *active, int32_t *status, double *f_neb, int32_t *imax, void *stream);

/* ---- batched finite-difference Hessians (harmonic analysis) --------------------------------------
 * Central differences of forces, as ASE's Vibrations with direction='central'.  For system b let idx_b be the m_b atoms that are
 * displaced, delta the displacement in A, and F(a,i,q) the summed forces (the engine's fp32 forces widened, plus forces_extra in
 * fp64) on the atoms idx_b when coordinate i of atom a is moved by q delta.  With the row r = 3 (position of a in idx_b) + i:
 *   nfree = 2:  D[r,:] = (F(a,i,-1) - F(a,i,+1)) / (2 delta)
 *   nfree = 4:  D[r,:] = (((8 F(a,i,-1) - F(a,i,-2)) - 8 F(a,i,+1)) + F(a,i,+2)) / (12 delta)
 *   H  = (D + D^T) 0.5                              eV/A^2
 *   asymmetry = max |D - D^T|                       the noise floor of fp32 forces at this delta
 *   Hm[r,c] = H[r,c] (w_r w_c),  w = 1 / sqrt(mass in amu) of the row's / column's atom       (bitwise symmetric, like H)
 * and on the host (sevennet_amd/vib.py): lambda = the eigenvalues of Hm, ascending, in eV/(A^2 amu);
 *   h nu = hbar sqrt(ACC |lambda|) sign(lambda) with hbar = 0.6582119569 eV fs and ACC = 9.648533212e-3, so an imaginary mode is
 *   reported as a negative number; frequencies = h nu 8065.543937 cm^-1/eV; zpe = (1/2) sum of the positive h nu.
 * Every expression is evaluated in fp64 in the order written, no product contracted with a sum, so the results equal the numpy
 * restatement (tests/vib_ref.py) bit for bit.  One 256-thread workgroup per unit of work, no atomics: two runs give identical bits.
 *
 * snet_vib_displace writes the displaced copies.  pos0 (fp64 [n0,3]) holds the base positions, system b being rows
 * [seg_ptr0[b], seg_ptr0[b+1]) (int32 [n_sys+1]).  Copy j is described by desc[4 j ..] = (system, atom within the system, axis,
 * multiplier q in -2 .. 2) (int32 [n_copies,4]) and owns rows [copy_ptr[j], copy_ptr[j+1]) (int32 [n_copies+1]) of pos_out (fp64
 * [n_out,3]): they receive the system's rows with q delta added to the one component -- the product is rounded, then added; q = 0
 * is the undisplaced copy, bit for bit.  A descriptor that does not fit -- a system, atom, axis or multiplier out of range, base or
 * output rows outside their arrays, a copy span that differs from the system's atom count -- sets status[j] = 1 (int32
 * [n_copies], otherwise left as it is) and leaves its rows unwritten; it is refused before anything is read or written.
 *
 * snet_vib_rows turns the forces on the copies of ONE call into rows of D.  forces (fp32 [n_atoms,3]) and forces_extra (fp64
 * [n_atoms,3] or NULL) are those of the n_copies copies of the call, copy j being rows [seg_ptr[j], seg_ptr[j+1]).  Row group g
 * is group[3 g ..] = (first copy j0, system b, row r) (int32 [n_groups,3]): its nfree copies j0 .. j0 + nfree - 1 are adjacent, in
 * the order q = -1, +1 or q = -2, -1, +1, +2.  The selected atoms of system b are sel[sel_ptr[b] .. sel_ptr[b+1]) (int32, indices
 * within the system; sel_ptr int32 [n_sys+1], n_sel entries in all).  Row r of the [3 m_b, 3 m_b] block that starts at D[d_off[b]]
 * (d_off int64 [n_sys], D fp64 [d_size]) is WRITTEN, not accumulated: each row is written by one workgroup of one call, so the
 * result does not depend on how the rows are spread over calls.  A force that is not finite sets status[b] = 2 (int32 [n_sys]); a
 * group that does not fit (copies outside the call, copies of unequal size, a row or block outside D, a selected atom outside the
 * system) sets status[b] = 3 and writes nothing outside the arrays.
 *
 * snet_vib_finish, once after the last call, one workgroup per system: reads D and writes H, Hm (fp64 [d_size], the same blocks)
 * and asymmetry[b]; w (fp64 [n_sel]) holds 1 / sqrt(mass) of the selected atoms.  For a system with status[b] != 0 the three are
 * NaN.                                                                                                                        */
int snet_vib_displace(const double *pos0, int64_t n0, const int32_t *seg_ptr0, int32_t n_sys, const int32_t *desc,
                      const int32_t *copy_ptr, int32_t n_copies, double delta, double *pos_out, int64_t n_out, int32_t *status,
                      void *stream);
int snet_vib_rows(const float *forces, const double *forces_extra, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_copies,
                  const int32_t *group, int32_t n_groups, int32_t nfree, double delta, const int32_t *sel, const int32_t *sel_ptr,
                  int64_t n_sel, const int64_t *d_off, int32_t n_sys, double *D, int64_t d_size, int32_t *status, void *stream);
int snet_vib_finish(const double *D, const int64_t *d_off, const int32_t *sel_ptr, int64_t n_sel, const double *w, int32_t n_sys,
                    int64_t d_size, int32_t *status, double *H, double *Hm, double *asymmetry, void *stream);

/* ---- batched supercell phonons ---------------------------------------------------------------------
 * Finite-displacement phonons of fully periodic crystals.  System b is a primitive cell C_b (rows), its m_b atoms and repeats
 * (n1,n2,n3) >= 1.  The supercell lattice is S = diag(n) C; supercell atom j = c m + beta is home atom beta shifted by
 * (c1,c2,c3) C with c = (c1 n2 + c2) n3 + c3; the home cell is c = 0, so the home atoms are the first m_b of the N_b = m_b n1 n2 n3.
 *   Force constants: Phi[(alpha,i),(j,k)], a [3 m_b, 3 N_b] array, row r = 3 alpha + i, column 3 j + k: the central difference of
 *     the forces on ALL N_b atoms when home atom alpha moves along axis i -- the stencil of snet_vib_rows, in its operation order.
 *   Acoustic sum rule: asr_defect = max over (alpha,i,k) of |sum_j Phi[(alpha,i),(j,k)]|, taken before any correction; with
 *     `acoustic` set, Phi[(alpha,i),(alpha,k)] is replaced by -sum_{j != alpha} Phi[(alpha,i),(j,k)].  Both sums run in ascending j.
 *   Images of the pair (alpha, j): d0 = r_j - r_alpha; f_c = (d0_x Sinv[0][c] + d0_y Sinv[1][c]) + d0_z Sinv[2][c]; n0 = -rint(f);
 *     the candidates are n = n0 + (x,y,z), x,y,z in {-1,0,1}, with d_c = d0_c + ((n1 S[0][c] + n2 S[1][c]) + n3 S[2][c]) and
 *     |d| = sqrt((d_x^2 + d_y^2) + d_z^2); a candidate is kept when |d| <= min |d| + symprec, and the kept ones share the weight
 *     equally.  The 27 candidates hold every nearest image when S is Minkowski-reduced, which the driver checks on the host.
 *   Dynamical matrix at q_cart (rad/A): R(q)[(alpha,i),(beta,k)] = (w_alpha w_beta) sum_c Phi[(alpha,i),(c m + beta,k)] p(alpha, c m +
 *     beta), c ascending, with the pair's phase p = (sum over the kept d of exp(i q_cart . d)) / n_kept, summed in ascending (x,y,z),
 *     q . d = (q_x d_x + q_y d_y) + q_z d_z and w = 1 / sqrt(mass in amu); D(q) = (R + R^H) 0.5; hermiticity = max |R - R^H|.
 *     The phase is taken with the full vector d, so eigenvectors are in that convention (no extra factor exp(i q . r_beta)).
 * fp64 throughout, one 256-thread workgroup per unit of work, no atomics, every output element written by one thread and every
 * sum in the order written: two runs give identical bits.  The numpy restatement is tests/phonon_ref.py.
 *
 * Shared descriptors: m_ptr (int32 [n_sys+1]): the home atoms of system b are entries [m_ptr[b], m_ptr[b+1]) of the per-home-atom
 * arrays; sc_ptr (int32 [n_sys+1]): its supercell atoms are rows [sc_ptr[b], sc_ptr[b+1]) of pos (fp64 [n_atoms,3]); p_off (int64
 * [n_sys]): its block of Phi starts at phi[p_off[b]] (fp64 [p_size]); i_off (int64 [n_sys]): entry (alpha, j) of its image arrays
 * is i_off[b] + alpha N_b + j (img_base int32 [i_size,3], img_mask int32 [i_size]).  A descriptor that does not fit -- a range
 * outside its array, N_b no multiple of m_b, a block outside its buffer -- sets status[b] = 3 (int32 [n_sys]) and nothing of that
 * unit of work is read or written.
 *
 * snet_ph_rows is snet_vib_rows with rows over all atoms of the copy: forces / forces_extra / seg_ptr / group / nfree / delta as
 * there (group[3 g ..] = (first copy, system, row r in [0, 3 m_b)); every copy of the group must hold N_b atoms).  Row r of Phi is
 * WRITTEN, not accumulated.  A force that is not finite sets status[b] = 2.
 * snet_ph_finish, one workgroup per system: writes asr_defect[b] and phi_out (fp64 [p_size], the same blocks, not phi itself): phi
 * with the self terms corrected if `acoustic`, copied otherwise.  For a system with status[b] != 0 both are NaN throughout.
 * snet_ph_images, one workgroup per home atom (home_sys int32 [n_home]: the system of each): reads pos, S and S_inv (fp64
 * [n_sys,9] each, row-major; S_inv is the caller's, so that device and restatement wrap with the same bits) and writes img_base =
 * n0 and img_mask, where bit 9 (x+1) + 3 (y+1) + (z+1) marks a kept candidate.  A pair whose f is not finite keeps no image and
 * sets status[b] = 3.
 * snet_ph_dynmat: q-point g of the launch (q_cart fp64 [n_q,3]) belongs to system q_sys[g] (int32 [n_q]) and is number
 * g - q_ptr[b] of its q_ptr[b+1] - q_ptr[b] points (q_ptr int32 [n_sys+1]); its [3 m_b, 3 m_b] complex blocks of R and D (fp64
 * [d_size,2]: real, imaginary) start at complex element d_off[b] + (g - q_ptr[b]) 9 m_b^2 (d_off int64 [n_sys]), its hermiticity is
 * hermiticity[g] (fp64 [n_q]).  w (fp64 [n_home]) holds 1 / sqrt(mass) of the home atoms, max_m the largest m_b (<= 65535).  Two
 * launches: one workgroup per (q, alpha) computes each pair's phase once, stages the phases in LDS (1024 at a time) and reuses
 * them for the pair's nine entries; then one workgroup per q writes D and the hermiticity.  D equals D^H bit for bit.  Values
 * that are not finite (the Phi of a failed system) pass through: R and D are NaN there and so is the hermiticity.              */
int snet_ph_rows(const float *forces, const double *forces_extra, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_copies,
                 const int32_t *group, int32_t n_groups, int32_t nfree, double delta, const int32_t *m_ptr, const int32_t *sc_ptr,
                 const int64_t *p_off, int32_t n_sys, double *phi, int64_t p_size, int32_t *status, void *stream);
int snet_ph_finish(const double *phi, const int64_t *p_off, const int32_t *m_ptr, const int32_t *sc_ptr, int32_t n_sys, int64_t p_size,
                   int32_t acoustic, int32_t *status, double *phi_out, double *asr_defect, void *stream);
int snet_ph_images(const double *pos, int64_t n_atoms, const int32_t *sc_ptr, const int32_t *m_ptr, const int32_t *home_sys,
                   int32_t n_home, const double *S, const double *S_inv, const int64_t *i_off, int32_t n_sys, double symprec,
                   int32_t *img_base, int32_t *img_mask, int64_t i_size, int32_t *status, void *stream);
int snet_ph_dynmat(const double *phi, const int64_t *p_off, int64_t p_size, const double *pos, int64_t n_atoms, const int32_t *sc_ptr,
                   const int32_t *m_ptr, const double *w, int32_t n_home, const double *S, const int32_t *img_base,
                   const int32_t *img_mask, const int64_t *i_off, int64_t i_size, const double *q_cart, const int32_t *q_sys,
                   const int32_t *q_ptr, int32_t n_q, const int64_t *d_off, int32_t n_sys, int32_t max_m, int32_t *status, double *R,
                   double *D, int64_t d_size, double *hermiticity, void *stream);

/* ---- batched elastic tensors from strained copies ---------------------------------------------------
 * Second-order elastic constants of fully periodic crystals by central differences of the stress over homogeneously strained
 * copies.  Voigt index j = 0 .. 5 in ASE order (xx, yy, zz, yz, xz, xy), rows are vectors, delta is the strain step.
 *   Strain patterns: E_j = e_a e_a^T for j < 3 (a = j); E_j = (e_a e_b^T + e_b e_a^T) / 2 for the shears, (a,b) = (1,2), (0,2),
 *     (0,1) for j = 3, 4, 5, so that a shear step delta is the engineering strain gamma = delta.
 *   Copy (b, j, q): F = I + (q delta) E_j with s = q delta rounded first (as snet_vib_displace rounds its shift) and h = s 0.5.
 *     A row x of the positions or of the cell becomes x F:  j < 3:  x_a <- x_a + s x_a;  shear:  x_a <- x_a + h x_b and
 *     x_b <- x_b + h x_a, both from the unstrained x; the other components are copied.  q = 0 is the unstrained copy, bit for bit.
 *     q runs over the stencil of snet_vib_rows (-1, +1 for nfree 2; -2, -1, +1, +2 for nfree 4): 6 nfree + 1 copies per system.
 *   Stress of a copy: sigma_i = -((virial + virial_extra)[p_i] / V'), p = (0, 1, 2, 4, 5, 3) taking the engine's order
 *     (xx,yy,zz,xy,yz,zx) to ASE Voigt, V' = |det(cell F)| of that copy (computed by the caller on the host, in fp64).
 *   S[i,j] = d sigma_i / d epsilon_j and L[j, 3 a + k] = d F_ak / d epsilon_j (the internal-strain tensor Lambda at fixed scaled
 *     coordinates; F the engine's fp32 forces widened, plus forces_extra in fp64) by the same stencil, with f_q the value at q:
 *       nfree = 2:  (f_+1 - f_-1) / (2 delta)
 *       nfree = 4:  (((8 f_+1 - f_+2) - 8 f_-1) + f_-2) / (12 delta)
 *   C = (S + S^T) 0.5 (bitwise symmetric), asymmetry = max |S - S^T|.  Under a residual stress sigma_0 of the unstrained cell S is
 *     legitimately asymmetric by terms of the order of sigma_0; C is the elastic tensor where that stress is about zero.
 *   Relaxed ions (on the host, sevennet_amd/elastic.py): with Phi the Gamma Hessian [3n,3n] of the unstrained structure
 *     (snet_vib_*), T the three normalised uniform translations, P = I - T T^T and kappa the mean diagonal of Phi,
 *     Phi+ = (P Phi P + kappa T T^T)^-1 - T T^T / kappa and S_rel = S - L Phi+ L^T / V, symmetrised as above.
 * Every expression is evaluated in fp64 in the order written, no product contracted with a sum, so the results equal the numpy
 * restatement (tests/elastic_ref.py) bit for bit.  One 256-thread workgroup per unit of work, no atomics, every output element
 * written by one thread: two runs give identical bits.
 *
 * snet_el_strain writes the strained copies.  pos0 / seg_ptr0 / copy_ptr / pos_out / status as snet_vib_displace; copy c is
 * desc[3 c ..] = (system, j, q) (int32 [n_copies,3]).  A descriptor that does not fit -- a system out of range, j outside 0 .. 5,
 * |q| > 2, base or output rows outside their arrays, a copy span that differs from the system's atom count -- sets status[c] = 1
 * (otherwise left as it is) and leaves its rows unwritten; it is refused before anything is read or written.
 *
 * snet_el_rows turns the results of the copies of ONE call into columns of S and rows of L.  virial and virial_extra (fp64
 * [n_copies,6], the latter or NULL), volume (fp64 [n_copies]), forces (fp32 [n_atoms,3]) and forces_extra (fp64 [n_atoms,3] or NULL)
 * are those of the call's copies, copy c being rows [seg_ptr[c], seg_ptr[c+1]).  Group g is group[3 g ..] = (first copy c0, system b,
 * column j) (int32 [n_groups,3]): its nfree copies c0 .. c0 + nfree - 1 are adjacent, in the order of the stencil.  System b has
 * atom_ptr[b+1] - atom_ptr[b] atoms (int32 [n_sys+1], n_base in all); its S is the row-major [6,6] block at S[36 b] (fp64
 * [36 n_sys]), its L the row-major [6, 3 n_b] block at L[18 atom_ptr[b]] (fp64 [18 n_base]).  Column j of S and row j of L are
 * WRITTEN, not accumulated, each element once.  A virial, volume or force that is not finite, or a volume that is not positive,
 * sets status[b] = 2 (int32 [n_sys]); a group that does not fit (copies outside the call or of another size than the system, j
 * outside 0 .. 5, atoms outside n_base) sets status[b] = 3 and writes nothing else.
 *
 * snet_el_finish, once after the last call, one workgroup per system: reads S and writes C (fp64 [36 n_sys]) and asymmetry[b];
 * both are NaN for a system with status[b] != 0.                                                                              */
int snet_el_strain(const double *pos0, int64_t n0, const int32_t *seg_ptr0, int32_t n_sys, const int32_t *desc,
                   const int32_t *copy_ptr, int32_t n_copies, double delta, double *pos_out, int64_t n_out, int32_t *status,
                   void *stream);
int snet_el_rows(const double *virial, const double *virial_extra, const double *volume, const float *forces,
                 const double *forces_extra, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_copies, const int32_t *group,
                 int32_t n_groups, int32_t nfree, double delta, const int32_t *atom_ptr, int64_t n_base, int32_t n_sys, double *S,
                 double *L, int32_t *status, void *stream);
int snet_el_finish(const double *S, int32_t n_sys, const int32_t *status, double *C, double *asymmetry, void *stream);

/* ---- batched NVE / Langevin MD step (fixed cell) -------------------------------------------------
 * One launch per MD step for n_sys systems; units eV, A, fs, amu, with ACC = 9.648533212e-3 (1 eV / (A amu) in A / fs^2).  The
 * atoms of system s are rows [seg_ptr[s], seg_ptr[s+1]) (device int32) of pos / vel (fp64 [n_atoms,3], updated in place), of
 * forces (fp32 [n_atoms,3], as the engine returns them; forces_extra, fp64 [n_atoms,3] or NULL, is added to them in fp64) and of
 * mass (fp64 [n_atoms], amu).  Per system on the device: sys_id (int32, the caller's index of the system: read by the noise
 * stream only), kT (fp64, eV), step_index (int32, in/out), e_kin (fp64, out).  The step is BAOAB (Leimkuhler, Matthews 2013; the
 * rule of TorchSim's nvt_langevin), folded around the force call so that one launch finishes step k and begins step k + 1.  With
 * F the summed forces at the current positions, for every system:
 *   if phase & 1 (FINISH):  v += (dt/2) ACC F / m
 *   e_kin[s] = sum_i (1/2) m_i |v_i|^2 / ACC                       (always)
 *   if phase & 2 (START):   v += (dt/2) ACC F / m
 *                           c2 == 0:  x += dt v                                                          (NVE)
 *                           else:     x += (dt/2) v;  v = c1 v + c2 sqrt(kT[s] ACC / m) xi;  x += (dt/2) v
 *                           step_index[s] += 1
 * c1 = exp(-gamma dt) and c2 = sqrt(1 - c1^2) are the caller's (computed once on the host in fp64).  phase 0 writes e_kin only.
 * xi: three standard normals per atom from Philox4x32-10 (Random123 constants: multipliers 0xD2511F53, 0xCD9E8D57, key increments
 * 0x9E3779B9, 0xBB67AE85) with key (seed & 0xffffffff, seed >> 32) and counter (a, sys_id[s], step_index[s], tag): a = the atom's
 * index within its system, step_index[s] before the increment, tag 0 for this thermostat and 1 for snet_mdb_init_velocities.  The
 * four output words w_k give u_k = (w_k + 0.5) 2^-32 and xi_x = sqrt(-2 ln u0) cos(2 pi u1), xi_y = sqrt(-2 ln u0) sin(2 pi u1),
 * xi_z = sqrt(-2 ln u2) cos(2 pi u3).  An atom's noise depends on (seed, system id, atom, step) only: not on the batch, the slot
 * or the launch grid.  With c2 == 0 no random number is generated.
 * One 256-thread workgroup per system, fp64 sums in a fixed order, no atomics: two runs give identical bits, and a system's
 * results do not depend on the other systems of the launch.
 *
 * snet_mdb_init_velocities: v_i = sqrt(kT[s] ACC / m_i) xi_i with the same generator (tag 1, step word 0).  remove_com != 0 and
 * more than one atom: the centre-of-mass velocity sum m v / sum m is subtracted and the velocities are scaled so that the kinetic
 * energy is (1/2) (3 n_s - 3) kT[s] exactly; remove_com != 0 and one atom: zero velocity.                                      */
int snet_mdb_step(double *pos, double *vel, const float *forces, const double *forces_extra, const double *mass, int64_t n_atoms,
                  const int32_t *seg_ptr, const int32_t *sys_id, int32_t n_sys, const double *kT, int32_t *step_index,
                  double *e_kin, double dt, double c1, double c2, uint64_t seed, int32_t phase, void *stream);
int snet_mdb_init_velocities(double *vel, const double *mass, int64_t n_atoms, const int32_t *seg_ptr, const int32_t *sys_id,
                             int32_t n_sys, const double *kT, uint64_t seed, int32_t remove_com, void *stream);
/* snet_mdb_step_fixed: the same step with components held fixed (hold as for snet_fire_step_fixed, not NULL).  A held component
 * (i, k) gets no kick, no drift and no thermostat noise: pos[3 i + k] is not written, vel[3 i + k] is stored as 0 (by every phase
 * that stores velocities) and the component contributes 0 to e_kin.  The noise counters do not depend on the mask -- a free
 * component draws exactly what it draws without one -- and every update of the step is component-wise, so the free components
 * equal snet_mdb_step's on the same inputs bit for bit.  snet_mdb_npt_step has no masked form.
 *
 * snet_mdb_init_velocities_fixed: held components are 0.  A system with no held component is treated exactly as by
 * snet_mdb_init_velocities, bit for bit.  For a system with at least one: the centre-of-mass shift is skipped (the held atoms
 * anchor the frame), and with remove_com != 0 the velocities are scaled so that the kinetic energy is (1/2) dof kT[s] exactly,
 * dof = 3 n_s - (held components); with dof = 0 all velocities are 0 (no 0/0).                                                  */
int snet_mdb_step_fixed(double *pos, double *vel, const float *forces, const double *forces_extra, const double *mass, int64_t n_atoms,
                        const int32_t *seg_ptr, const int32_t *sys_id, int32_t n_sys, const double *kT, int32_t *step_index,
                        double *e_kin, double dt, double c1, double c2, uint64_t seed, int32_t phase, const int32_t *hold, void *stream);
int snet_mdb_init_velocities_fixed(double *vel, const double *mass, int64_t n_atoms, const int32_t *seg_ptr, const int32_t *sys_id,
                                   int32_t n_sys, const double *kT, uint64_t seed, int32_t remove_com, const int32_t *hold,
                                   void *stream);

/* ---- batched isotropic NPT MD step (the cell moves on the device) --------------------------------
 * snet_mdb_step with the stochastic cell rescaling of Bernetti and Bussi, J. Chem. Phys. 153, 114107 (2020), isotropic form: a
 * barostat of first order in the cell, one normal deviate per system and step, no barostat momentum.  Arrays, units, phase bits
 * and the thermostat's noise as snet_mdb_step, and per system: cell (fp64 [n_sys,9], row-major lattice vectors, updated in
 * place), virial (fp64 [n_sys,6], the engine's virial_per_system: order xx,yy,zz,xy,yz,zx, stress = -virial / volume;
 * virial_extra, fp64 [n_sys,6] or NULL, is added to it), p0 (fp64, the external pressure, eV/A^3), beta_over_tau (fp64, the
 * isothermal compressibility over the barostat's relaxation time, A^3/(eV fs)), volume and pressure (fp64, out), active (int32,
 * in/out: 1 while the system runs) and status (int32: the caller's 0, 2 written when the guard below fails).  With F and W the
 * summed forces and virials at the current positions and cell, for every system with active == 1:
 *   1. if phase & 1 (FINISH):  v += (dt/2) ACC F / m
 *   2. K = sum_i (1/2) m_i |v_i|^2 / ACC;  V = |det cell|;  P = (2 K + W_xx + W_yy + W_zz) / (3 V)
 *      e_kin[s] = K, volume[s] = V, pressure[s] = P                                       (always, in every phase)
 *   3. if phase & 2 (START):   v += (dt/2) ACC F / m, then the barostat step S:
 *        de = -beta_over_tau[s] (p0[s] - P) dt + sqrt(2 kT[s] beta_over_tau[s] dt / V) xi_s
 *        mu = exp(de / 3);  x <- mu x;  v <- v / mu;  cell <- mu cell
 *   4. then, still under START, the A-O-A part of snet_mdb_step:  c2 == 0:  x += dt v
 *        else:  x += (dt/2) v;  v = c1 v + c2 sqrt(kT[s] ACC / m) xi;  x += (dt/2) v;           step_index[s] += 1
 * S sits after both kicks with the forces of step k and before the next force evaluation: every kick uses forces at the positions
 * and the cell they were evaluated at, and P is synchronous at step k.  xi_s is the first normal of the generator of
 * snet_mdb_step under the counter (0, sys_id[s], step_index[s], tag 2): the same barostat noise alone as in a batch.  With
 * kT == 0 or beta_over_tau == 0 the noise term is zero and no random number is generated for it; with beta_over_tau == 0 mu is
 * exactly 1 and pos, vel, e_kin and step_index are those of snet_mdb_step bit for bit.
 * Guard: nothing of a system but e_kin, volume and pressure is written before its next cell has passed.  If de or an entry of
 * the new cell is not finite (a NaN virial), |de| > max_log_volume_step, or a face-to-face height of the new cell is below
 * min_height (the batched neighbour kernels take heights down to cutoff / 64): active = 0, status = 2, and pos, vel, cell and
 * step_index keep their bits -- the finishing kick of this launch is not stored either.  A system with active == 0 is taken at
 * phase 0 in every later launch: its e_kin (of the velocities as they are), volume and pressure are written, nothing else.
 * One 256-thread workgroup per system, fp64 sums in a fixed order, no atomics: two runs give identical bits, and a system's
 * results do not depend on the other systems of the launch.                                                                   */
int snet_mdb_npt_step(double *pos, double *vel, double *cell, const float *forces, const double *forces_extra, const double *virial,
                      const double *virial_extra, const double *mass, int64_t n_atoms, const int32_t *seg_ptr,
                      const int32_t *sys_id, int32_t n_sys, const double *kT, const double *p0, const double *beta_over_tau,
                      int32_t *step_index, double *e_kin, double *volume, double *pressure, int32_t *active, int32_t *status,
                      double dt, double c1, double c2, uint64_t seed, int32_t phase, double max_log_volume_step, double min_height,
                      void *stream);

/* ---- MD observables accumulated on the device -----------------------------------------------------
 * What an MD driver samples while positions and velocities stay on the device (sevennet_amd.observe): pair counts of the radial
 * distribution function, and mean-square displacement and velocity autocorrelation against a ring of origin frames.  One launch
 * each per sample for n_sys systems; the atoms of system b are rows [seg_ptr[b], seg_ptr[b+1]) (device int32) of pos / vel (fp64
 * [n_atoms,3]), mass (fp64 [n_atoms]) and kind (int32 [n_atoms]: the atom's kind, 0 .. kinds_b - 1, numbered within its system).
 * All arithmetic is fp64 and no product is contracted with the sum that follows it.
 *
 * snet_obs_rdf adds, for every system b, to counts[off_b + (ka kinds_b + kb) bins + bin] (uint64) the number of ordered triples
 * (i of kind ka, j of kind kb, lattice shift n) with (i != j or n != 0) whose distance falls into `bin`:
 *   d = x_j - x_i;  f = d cell_b^-1;  f_k -= rint(f_k) on periodic axes;  d = f cell_b          (positions need not be wrapped)
 *   for n_k in [-reach_k, reach_k] on periodic axes (0 on open ones):  r = |d + n cell_b|,  q = r / dr,  counted if q < bins in
 *   bin (int) q,  r = sqrt((x x + y y) + z z).
 * cell (fp64 [n_sys,9], row-major lattice vectors; rows of open axes only have to keep the cell invertible where another axis
 * is periodic, and a cell without a periodic axis is not read).  sys_desc (int32 [n_sys,8]) = (kinds_b, off_b, pbc bits (bit k:
 * axis k is periodic), reach_x, reach_y, reach_z, 0, 0): reach_k = floor(r_max / height_k + 0.5), r_max = bins dr, is the
 * caller's, and with |f_k| <= 1/2 after the reduction no image within r_max lies beyond it.  tile (int32 [n_tiles,3]) = (system,
 * first row within the system, rows): one 256-thread workgroup per tile takes the pairs (i in the tile, j in the system), counts
 * into a uint32 histogram of kinds_b^2 bins words in LDS and adds its non-zero words to `counts` with one integer atomicAdd each
 * -- integers only, so the result does not depend on the order of anything.  kinds_max (<= 8, kinds_max^2 bins <= 8192: the LDS
 * histogram) and reach_max (<= 4) bound what the descriptors may say; a system or tile whose descriptor exceeds them, or points
 * outside the system's rows or outside counts[0 .. n_counts), counts nothing.
 *
 * snet_obs_correlate: the ring holds `ring` = ceil(lags / origin_every) origin frames, ring_pos / ring_vel (fp64 [ring,n_atoms,3]);
 * origin number q is sample q origin_every and sits in slot q % ring.  The CALLER stores the frame of a sample that is an origin
 * into its slot (a device-to-device copy on the same stream) before this launch.  For sample number `sample`, grid (system, slot):
 * the workgroup of a slot whose origin q has lag = sample - q origin_every < lags adds, for every kind of the system,
 *   msd_sum [(kind_ptr[b] + kind) lags + lag] += sum_i |d_i|^2,            d_i = (x_i - X) - (x_i(origin) - X(origin))
 *   vacf_sum[(kind_ptr[b] + kind) lags + lag] += sum_i (v_i - V) . (v_i(origin) - V(origin))
 * over the system's atoms of that kind, in the fixed order of one workgroup's sum (kind_ptr int32 [n_sys+1], n_kinds rows of `lags`
 * in msd_sum / vacf_sum, at most 8 kinds per system).  remove_com != 0: X and V are the mass-weighted centres sum m x / sum m of
 * each frame; a system with a held component (hold, int32 [n_atoms] as for snet_mdb_step_fixed, or NULL) is anchored and not
 * corrected, like snet_mdb_init_velocities_fixed, and a system of one free atom adds 0.  remove_com == 0: X = V = 0.  The live
 * origins of a sample have distinct lags, so no two workgroups of a launch write one slot, and launches are ordered by the
 * stream: a system's sums do not depend on the batch it is in.  How often lag l was added to is a matter of the schedule
 * alone (sevennet_amd.observe.origin_counts).                                                                                  */
int snet_obs_rdf(const double *pos, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_sys, const int32_t *kind, const double *cell,
                 const int32_t *sys_desc, const int32_t *tile, int32_t n_tiles, double dr, int32_t bins, int32_t kinds_max,
                 int32_t reach_max, uint64_t *counts, int64_t n_counts, void *stream);
int snet_obs_correlate(const double *pos, const double *vel, const double *ring_pos, const double *ring_vel, const double *mass,
                       const int32_t *hold, int64_t n_atoms, const int32_t *seg_ptr, int32_t n_sys, const int32_t *kind,
                       const int32_t *kind_ptr, int64_t n_kinds, int32_t sample, int32_t origin_every, int32_t ring, int32_t lags,
                       int32_t remove_com, double *msd_sum, double *vacf_sum, void *stream);

/* ---- whole-model sequencer ------------------------------------------------------------------
 * replaces, for a native (C++) host, `model.forward(input_dict)` + `torch::autograd::grad(...)` of
 * the LAMMPS pair styles (sevenn/pair_e3gnn/pair_e3gnn.cpp:200-207, pair_e3gnn_parallel.cpp:424-503)
 * and the TorchScript archive they load (`torch::jit::load`, pair_e3gnn.cpp:356).  The model comes
 * from a `.snet` file written by sevennet_amd.model_file.write_model_file (the analogue of
 * `sevenn get_model`, sevenn/scripts/deploy.py:16-76).  One evaluation runs the op sequence above on
 * the caller's stream out of a grow-only device arena owned by the model: no per-step allocation
 * once the largest system has been seen.                                                        */
typedef struct snet_model snet_model;
int snet_model_load(const char *path, snet_model **model);
int snet_model_load_memory(const void *blob, int64_t n_bytes, snet_model **model);
void snet_model_destroy(snet_model *model);
/* cutoff, species count, number of interaction layers and (comm_dims[t], t < max_layers) the row
 * width of the ghost exchange before layer t -- what pair_e3gnn_parallel.cpp:571-660 reads from the
 * archive's extra files ("cutoff", "comm_size", ...).  Any output pointer may be NULL. */
int snet_model_info(const snet_model *model, float *cutoff, int32_t *n_species, int32_t *n_layers,
                    int32_t *comm_dims, int32_t max_layers);
/* value of one metadata key of the model file into value[capacity] (NUL-terminated); keys as in the
 * reference's deployed model (pair_e3gnn.cpp:321-330): chemical_symbols_to_index, cutoff, num_species,
 * model_type, version, dtype.  rc 3: no such key. */
int snet_model_meta(const snet_model *model, const char *key, char *value, int32_t capacity);
/* Ghost exchange hooks (pair_e3gnn_parallel.cpp:369,435; comm_brick.cpp:1057-1123):
 *   forward(user, x[n_total,dim], ...)  fill rows n_local.. with their owners' rows
 *   reverse(user, gx[n_total,dim], ...) add rows n_local.. into their owners' rows
 * x is a DEVICE pointer, work must be ordered on `stream`; return non-zero to abort the evaluation.
 * Needed iff an evaluation has n_total > n_local.  fold_forces != 0: the engine also calls `reverse`
 * on forces[n_total,3] (and virial_atom) so ghost rows end up in their owners; 0: ghost rows are
 * left to the host (LAMMPS folds them itself with reverse_comm when newton_pair is on). */
typedef int (*snet_halo_fn)(void *user, float *x, int64_t n_total, int64_t n_local, int32_t dim, void *stream);
/* Topology cache: with it on, snet_model_eval keeps what depends on the edge list only (tile list of the reverse kernels --
 * its construction reads a count back, i.e. synchronises the stream --, the edges grouped by source, per-species row lists)
 * across evaluations for as long as the caller passes the SAME device index arrays (row_ptr, src, eperm, w_row; same counts)
 * and has not called snet_model_topology_changed.  A caller that rewrites those arrays in place must call it.  Off by default.
 * Models of more than 4 species also keep the set of species that occur among the n_total atoms (layer 0's species slots,
 * snet_layer0_*) under the same rule, keyed by the `types` device array: a caller that rewrites `types` in place must call
 * snet_model_topology_changed as well.  With the cache off such a model reads `types` back on every evaluation (one n_total-sized
 * copy and one stream synchronisation per step); models of at most 4 species never do.
 * snet_model_eval_syncs: stream synchronisations issued inside snet_model_eval since the model was loaded (diagnostic). */
/* Bricks of a spatial decomposition that number their local atoms INTERIOR FIRST (rows [0, n_interior) have no ghost source;
 * sevennet_amd.parallel.BrickGraph.n_interior) let the sequencer run the interior rows of the fused convolutions while the
 * ghost exchange of the layer is in flight (library halo installed with snet_model_set_rccl_halo; second stream inside the
 * model).  0 (default) = no split.  Applies to the following evaluations until set again.                              */
int snet_model_set_interior(snet_model *model, int64_t n_interior);
int snet_model_set_topology_cache(snet_model *model, int32_t enable);
/* layer 0's reverse pass through snet_layer0_conv_bwd (enable != 0; the default unless SNET_LAYER0_MOMENTS=0 is in the environment at
 * load time) or through the fused kernel (0), where the model is eligible at all: its file carries the metadata key layer0_moments=1
 * and the shape passes snet_layer0_plan_create.  Applies to the following evaluations.  For A/B runs and tests. */
int snet_model_set_layer0_moments(snet_model *model, int32_t enable);
/* the last layer's reverse pass through snet_lastlayer_conv_bwd (enable != 0; the default unless SNET_LAST_LAYER_MERGED=0 is in the
 * environment at load time) or through snet_conv_bwd_fused_tangent + the transposed convolution (0), where the model is eligible:
 * its file carries the metadata key last_layer_merged=1 and the shape passes snet_lastlayer_plan_create.  Applies to the following
 * evaluations.  For A/B runs and tests. */
int snet_model_set_last_layer_merged(snet_model *model, int32_t enable);
/* the middle layers' g_xe rows merged inside the reverse kernel (snet_conv_bwd_fused_tangent_merged over snet_gxe_merge_map;
 * enable != 0, the default unless SNET_GXE_MERGE=0 is in the environment at load time) or one row per edge (0).  Taken where the
 * topology cache is on (the map is kept with the tile list), the layer's shape has the kernel and the graph's merged rows are at most
 * 0.8 of its edges (an atom order without locality merges nothing).  Applies to the following evaluations.  For A/B runs and tests. */
int snet_model_set_gxe_merge(snet_model *model, int32_t enable);
int snet_model_topology_changed(snet_model *model);
int64_t snet_model_eval_syncs(const snet_model *model);
int snet_model_set_halo(snet_model *model, snet_halo_fn forward, snet_halo_fn reverse, void *user,
                        int32_t fold_forces);
/* ---- a12, native: the ghost exchange itself, on RCCL (xGMI point-to-point), no host staging --------------
 * What a C++ host (LAMMPS pair style, any MD driver) installs instead of writing its own hooks; replaces the
 * reference's PairE3GNNParallel::{pack,unpack}_{forward,reverse}_comm_gnn (pair_e3gnn_parallel.cpp:747-911) and the
 * float overloads of CommBrick::forward_comm / reverse_comm (comm_brick.cpp:1057-1123): six sequential blocking
 * MPI swaps (with ghost-of-ghost forwarding and optional host staging, :806-809) become ONE ncclGroup of
 * send / recv pairs per call -- every peer concurrently, each over its own xGMI link, on the caller's stream.
 *   snet_rccl_unique_id / snet_rccl_comm_create   one communicator per process group: rank 0 makes the 128-byte id,
 *       the host broadcasts it (MPI_Bcast, torch.distributed ...), every rank creates its communicator
 *   snet_halo_create   the exchange plan of one decomposition: send_counts[world] rows go to each peer, taken from
 *       local rows send_idx (HOST int32, concatenated in peer order); recv_counts[world] ghost rows arrive from
 *       each peer and land contiguously, in peer order, behind the local rows -- or, with recv_perm (HOST
 *       int32[n_ghost], nullable), the k-th row of that peer-ordered stream is the host's ghost row recv_perm[k]
 *       (hosts that number their ghost nodes in their own order, e.g. a LAMMPS pair style)
 *   snet_halo_forward / snet_halo_reverse   have the snet_halo_fn signature (user = the snet_halo*): forward fills
 *       ghost rows, reverse adds ghost rows into their owners (received rows are summed per target row in fixed
 *       peer order: deterministic).  snet_model_set_rccl_halo installs both on a model.
 * RCCL is bound with dlopen at first use: libsnet_hip.so has no link-time dependency on it.                        */
typedef struct snet_halo snet_halo;
int snet_rccl_unique_id(void *id128);
int snet_rccl_comm_create(const void *id128, int32_t world, int32_t rank, void **comm);
void snet_rccl_comm_destroy(void *comm);
/* snet_rccl_available: 1 if librccl.so can be bound in this process -- local and non-collective, so that ranks can agree on the
 * transport BEFORE entering the collective snet_rccl_comm_create.  snet_rccl_comm_info: the size and this process's rank as RCCL
 * itself reports them (ncclCommCount / ncclCommUserRank): a host's start-up check that the communicator spans the ranks it
 * thinks it does. */
int snet_rccl_available(void);
int snet_rccl_comm_info(void *comm, int32_t *world_out, int32_t *rank_out);
int snet_rccl_allreduce_sum_f64(void *comm, double *dev_values, int64_t n, void *stream);
int snet_halo_create(void *comm, int32_t world, int32_t rank, const int32_t *send_counts, const int32_t *send_idx_host,
                     const int32_t *recv_counts, const int32_t *recv_perm_host, snet_halo **out);
void snet_halo_destroy(snet_halo *halo);
int64_t snet_halo_ghost_rows(const snet_halo *halo);
int64_t snet_halo_send_rows(const snet_halo *halo);
int snet_halo_forward(void *halo, float *x, int64_t n_total, int64_t n_local, int32_t dim, void *stream);
int snet_halo_reverse(void *halo, float *gx, int64_t n_total, int64_t n_local, int32_t dim, void *stream);
/* snet_halo_reverse in two halves, for hosts that overlap the exchange with work that still WRITES the local rows
 * (interior / boundary split of the convolution): _exchange reads the ghost rows gx[n_local ..] only and stages what the peers
 * return inside the halo; _accumulate adds the staged rows into gx[.. n_local].  One exchange may be staged at a time.   */
int snet_halo_reverse_exchange(void *halo, const float *gx, int64_t n_total, int64_t n_local, int32_t dim, void *stream);
int snet_halo_reverse_accumulate(void *halo, float *gx, int32_t dim, void *stream);
int snet_model_set_rccl_halo(snet_model *model, snet_halo *halo, int32_t fold_forces);
/* In-process stand-in for the RCCL communicator -- TEST infrastructure for one GPU: W host threads play W ranks; a
 * send posts {device pointer, ready event}, the matching receive copies device to device on the receiver's stream
 * and acknowledges with an event the sender's stream waits on (ncclSend / ncclRecv inside one ncclGroup: FIFO per
 * ordered pair, the group end blocks until the peers arrived).  A communicator made by snet_loopback_comm_create is
 * accepted wherever one from snet_rccl_comm_create is (snet_halo_create ...; not the all-reduce) and is destroyed with
 * snet_rccl_comm_destroy; everything above the transport is the code the RCCL path runs.                          */
int snet_loopback_hub_create(int32_t world, void **hub);
void snet_loopback_hub_abort(void *hub);
void snet_loopback_hub_destroy(void *hub);
int snet_loopback_comm_create(void *hub, int32_t rank, void **comm);

/* One energy/force evaluation.  Device inputs: types[n_total] species index, row_ptr[n_local+1] /
 * src[E] edges sorted by center (CSR), col_ptr[n_total+1] / eperm[E] the same edges grouped by source,
 * edge_vec[E,3] = r_src - r_center.  types_host[n_local] (HOST, may be NULL for models without a
 * per-species self-connection).  w_row[E] / pair_edge[n_pairs] (snet_edge_pairs; both NULL and
 * n_pairs 0 = one radial-weight row per directed edge).  Device outputs, each nullable: energy (double), e_atom[n_local],
 * dE_dr[E,3], forces[n_total,3] (ghost rows folded into owners when halo hooks are set),
 * virial[6] (double, xx yy zz xy yz zx = -sum r (x) dE/dr), virial_atom[n_total,6].             */
int snet_model_eval(snet_model *model, int64_t n_total, int64_t n_local, int64_t n_edges, const int32_t *types,
                    const int32_t *types_host, const int32_t *row_ptr, const int32_t *src, const int32_t *col_ptr,
                    const int32_t *eperm, const float *edge_vec, const int32_t *w_row, const int32_t *pair_edge,
                    int64_t n_pairs, double *energy, float *e_atom, float *dE_dr, float *forces, double *virial,
                    float *virial_atom, void *stream);

/* ---- undirected pairs: one radial-weight row per pair --------------------------------------------
 * The radial MLP's input (Bessel x cutoff of |r|, edge_embedding.py:101-160) is the same for the two
 * directed edges i->j and j->i, so w[e] == w[rev(e)].  Given the center-sorted edge list of
 * n_local owned atoms, this finds each edge's reverse (same atom pair, opposite vector within
 * 2e-5) and numbers the undirected pairs: w_row[e] in [0, n_pairs) is the row edge e reads,
 * pair_edge[p] is one edge of pair p (whose embedding row feeds the MLP).  Edges whose source is a
 * ghost (row on another rank) form singleton pairs.  Evaluate the radial MLP on the n_pairs gathered
 * embedding rows and pass w_row to the snet_conv_* calls: half the MLP work and half the w bytes for
 * a bulk cell, identical results.  Device in/out; *n_pairs on the HOST (the call synchronises). */
int snet_edge_pairs(const int32_t *row_ptr, const int32_t *src, const float *edge_vec, int64_t n_local,
                    int64_t n_edges, int32_t *w_row, int32_t *pair_edge, int64_t *n_pairs, void *stream);

/* ---- MD host: LAMMPS-style neighbor list in, forces accumulated out --------------------------
 * replaces the body of PairE3GNN::compute (sevenn/pair_e3gnn/pair_e3gnn.cpp:74-289) and the graph
 * build + force epilogue of PairE3GNNParallel::compute (pair_e3gnn_parallel.cpp:194-306,459-506).
 * All arrays are HOST pointers exactly as a pair style holds them:
 *   inum, ilist[inum], numneigh[nall] (indexed by atom), firstneigh[nall] (rows of a FULL list,
 *   entries may carry special-bond bits), x[nall,3] = &atom->x[0][0], type[nall] (1-based),
 *   tag[nall] (tag_bytes 4 or 8), type_map[ntypes+1] = the pair style's `map` (type -> species).
 * ghost_mode 0 (pair e3gnn): a neighbor is aliased to the local atom with the same tag, others are
 *   dropped (tag_map, :102,147-149) -- one process holding the whole periodic cell.
 * ghost_mode 1 (pair e3gnn/parallel): every ghost identity is a graph node after the inum locals
 *   (tag_to_graph_idx, pair_e3gnn_parallel.cpp:262-287); set the model's halo hooks first (with
 *   fold_forces 0: ghost forces are added to f[ghost] for LAMMPS' reverse_comm).  node_to_atom_out
 *   (nullable, capacity nall) receives node -> atom index BEFORE the model runs, for those hooks.
 * The neighbor filter (r^2 < cutoff^2 in fp64, edge_vec = x[j]-x[i] rounded to fp32), the CSR /
 * source grouping, the model and the force / virial reduction all run on `stream`; results are
 * ADDED to f[nall,3], *eng, virial[6] (LAMMPS order xx yy zz xy xz yz), eatom[nall], vatom[nall,6]
 * as ev_tally-free pair styles do.  Blocking: returns after the results are on the host.        */
typedef struct snet_md_host snet_md_host;
int snet_md_create(snet_model *model, snet_md_host **host);
/* node -> atom index exactly as snet_md_compute will number the graph nodes for these arrays (capacity nall);
 * lets a pair style lay out its ghost exchange (snet_halo_create) when the neighbor list was rebuilt */
int snet_md_nodes(int32_t inum, const int32_t *ilist, int32_t nall, const void *tag, int32_t tag_bytes,
                  int32_t ghost_mode, int32_t *node_to_atom_out, int64_t *n_nodes_out);
void snet_md_destroy(snet_md_host *host);
/* One-shot hint: the NEXT snet_md_compute call gets the same neighbor list as the previous one (LAMMPS `neighbor->ago > 0`:
 * same inum / ilist / numneigh / firstneigh / nall / tags / types) -- the flattened list, node maps and species uploaded then
 * are reused, only the positions travel (the edge set inside the cutoff is still re-derived from them every step).       */
int snet_md_list_unchanged(snet_md_host *host);
int snet_md_compute(snet_md_host *host, int32_t inum, const int32_t *ilist, const int32_t *numneigh,
                    const int32_t *const *firstneigh, int32_t nall, const double *x, const int32_t *type,
                    const void *tag, int32_t tag_bytes, const int32_t *type_map, int32_t ntypes, int32_t ghost_mode,
                    int32_t eflag_atom, int32_t vflag, int32_t vflag_atom, double *f, double *eng, double *virial,
                    double *eatom, double *vatom, int32_t *node_to_atom_out, int64_t *n_nodes_out,
                    int64_t *n_edges_out, void *stream);

/* ---- DFT-D3 dispersion -----------------------------------------------------------------------------
 * What the reference's CUDA library behind sevenn.calculator.D3Calculator computes (pair_d3_for_ase.cu), as own HIP
 * kernels (csrc/snet_d3.hip: one workgroup per atom over its (neighbour, lattice translation) row, fp64, deterministic
 * reductions), behind the same call sequence as the reference's C-ABI (pair_d3_for_ase.cu:2034-2082):
 *   pair_init          -> snet_d3_create            pair_run_coeff     -> snet_d3_set_tables (published tables, from the
 *   pair_set_atom      -> snet_d3_set_atoms                               blob sevennet_amd/data/d3_params.npz) + set_atoms
 *   pair_set_domain    -> snet_d3_set_cell          pair_run_compute   -> snet_d3_compute
 *   pair_run_settings  -> snet_d3_settings          pair_get_energy / _force / _stress -> snet_d3_energy / _forces / _stress
 *   pair_fin           -> snet_d3_destroy
 * Units at the boundary: A, eV, eV/A, eV/A^3; cutoffs in bohr^2 like the reference (vdw 9000, cn 1600).
 *   snet_d3_set_tables  r0ab[94*94] (A), c6ab[n_c6*5] (C6, Z_i + 100 ref_i, Z_j + 100 ref_j, CN_i, CN_j), r2r4[94], rcov[94]
 *   snet_d3_settings    damping 0 = damp_zero, 1 = damp_bj; func5 = (s6, rs6, s18, rs18, alp) of the functional
 *   snet_d3_set_cell    cell[9]: lattice vectors as rows (any orientation: no LAMMPS-style rotation needed), pbc[3]
 *   snet_d3_stress      [9] = dE/d(strain) / volume, row-major symmetric (ASE sign convention)
 * Batches: snet_d3_compute_batch evaluates n_sys systems -- atoms [atom_ptr[s], atom_ptr[s+1]) of the flat arrays, cell
 * cells[9 s ..] (rows = lattice vectors, A; molecules need a box, as for snet_d3_compute), pbc[3 s ..] -- in one set of
 * three launches, with the tables and settings of the handle (snet_d3_set_atoms / _set_cell are not used).  Every system's
 * results equal those of snet_d3_compute on it bit for bit.  Outputs are caller-owned host buffers: energy[n_sys] (eV),
 * forces[3 N] (eV/A), stress[9 n_sys] (as snet_d3_stress, per system), cn[N].  Errors name the system ("system 3: ...");
 * at most 2^31 - 1 atoms in total.  Synchronises `stream` before it returns.
 * Device-resident evaluation (the D3 term of the batched drivers): snet_d3_plan does ONCE per set of systems the host work that
 * depends on species and topology only (dense type index, per-atom rcov / r2r4, the r0 and reference-C6 slices, atom ranges) and
 * fixes a translation CAPACITY per system and list: the count of lattice translations with every periodic axis' repetition
 * count one larger than for the plan's cell (cells_move != 0), exactly that of the plan's cell (cells_move == 0), 27 for a system
 * with box_rule[s] != 0 (the molecule box of sevenn/calculator.py:533-548, formed from the positions of each call, pbc all
 * true).  All device memory is allocated there; a plan whose translation storage would exceed 2^27 doubles is refused.  A handle
 * holds one plan; planning again replaces it.  Synchronises `stream`.
 * snet_d3_compute_device evaluates the planned systems at DEVICE positions[N,3] (A) and DEVICE cells[n_sys,9] (A; NULL: the
 * plan's) into device outputs: energy[n_sys] (eV), forces[N,3] (eV/A), virial[n_sys,6] in the engine's convention (order
 * xx,yy,zz,xy,yz,zx, stress = -virial / volume: what snet_fire_cell_step takes as virial_extra), and, each nullable, cn[N],
 * volume[n_sys] (A^3), status[n_sys].  Six launches on `stream`, no host read, no synchronisation, no allocation; the work is
 * bounded by the plan's capacities whatever the cells hold.  status 1: the system's cell is not finite, |det| <= 1e-12 bohr^3, or
 * a translation list would exceed its capacity -- its energy, forces and virial are NaN, every other system is unaffected.
 * Energy, forces and cn equal snet_d3_compute_batch on the same inputs bit for bit.                                        */
typedef struct snet_d3 snet_d3;
int snet_d3_create(snet_d3 **out);
void snet_d3_destroy(snet_d3 *d3);
int snet_d3_set_tables(snet_d3 *d3, const double *r0ab, const double *c6ab, int64_t n_c6, const double *r2r4, const double *rcov);
int snet_d3_settings(snet_d3 *d3, double vdw_cutoff_au2, double cn_cutoff_au2, int32_t damping, const double *func5);
int snet_d3_set_atoms(snet_d3 *d3, int32_t n, const int32_t *atomic_numbers, const double *positions);
int snet_d3_set_cell(snet_d3 *d3, const double *cell9, const int32_t *pbc3);
int snet_d3_compute(snet_d3 *d3, void *stream);
int snet_d3_compute_batch(snet_d3 *d3, int32_t n_sys, const int64_t *atom_ptr /*[n_sys+1]*/, const int32_t *atomic_numbers /*[N]*/,
                          const double *positions /*[N*3], A*/, const double *cells /*[n_sys*9], A*/, const int32_t *pbc /*[n_sys*3]*/,
                          double *energy /*[n_sys], eV*/, double *forces /*[N*3], eV/A*/, double *stress /*[n_sys*9], eV/A^3*/,
                          double *cn /*[N]*/, void *stream);
int snet_d3_plan(snet_d3 *d3, int32_t n_sys, const int64_t *atom_ptr /*[n_sys+1]*/, const int32_t *atomic_numbers /*[N]*/,
                 const double *cells /*[n_sys*9], A*/, const int32_t *pbc /*[n_sys*3]*/, const int32_t *box_rule /*[n_sys]*/,
                 int32_t cells_move, void *stream);
int snet_d3_compute_device(snet_d3 *d3, const double *positions /*[N*3], A, device*/, const double *cells /*[n_sys*9], A, device*/,
                           double *energy /*[n_sys]*/, double *forces /*[N*3]*/, double *virial /*[n_sys*6]*/, double *cn /*[N]*/,
                           double *volume /*[n_sys]*/, int32_t *status /*[n_sys]*/, void *stream);
double snet_d3_energy(const snet_d3 *d3);
const double *snet_d3_forces(const snet_d3 *d3);
const double *snet_d3_stress(const snet_d3 *d3);
const double *snet_d3_coordination_numbers(const snet_d3 *d3);

#ifdef __cplusplus
}
#endif
#endif /* SNET_HIP_H */
