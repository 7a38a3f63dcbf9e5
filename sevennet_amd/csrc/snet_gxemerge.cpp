// Merge map of the merged-store reverse kernel (generated convftm_<tag>.hip): which g_xe rows of a workgroup's window
// of tiles are added together before they leave the chip, where the sums go, and the segment lists of the compact buffer.
// Topology only: built once per graph beside the tile list, on the host (one pass over the edges), from copies of the index arrays.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "snet_common.h"
#include "snet_hip.h"

namespace {
// edge range of tile t: mode 1 packed tiles (tile_ptr = tile_e0[n_tiles + 1]), mode 0 16-edge pieces of one row (tile_ptr[row] = first
// tile of the row, tile_node[t] = its row)
inline void tile_range(int mode, const int32_t *row_ptr, const int32_t *tile_ptr, const int32_t *tile_node, int64_t t, int64_t &e0, int64_t &cnt) {
  if (mode == 1) {
    e0 = tile_ptr[t];
    cnt = tile_ptr[t + 1] - e0;
    return;
  }
  const int32_t node = tile_node[t];
  e0 = row_ptr[node] + 16 * (t - tile_ptr[node]);
  const int64_t left = row_ptr[node + 1] - e0;
  cnt = left < 16 ? left : 16;
}
}  // namespace

extern "C" int snet_gxe_merge_map_host(const int32_t *row_ptr, const int32_t *src, const int32_t *tile_ptr, const int32_t *tile_node,
                                       int64_t n_tiles, int64_t tile_cut, int32_t tile_mode, int32_t window, int64_t n_src,
                                       int64_t n_edges, int32_t *merge_row, int32_t *merge_next, int32_t *seg_ptr, int32_t *perm,
                                       int64_t *n_rows) {
  const char *who = "snet_gxe_merge_map";
  SNET_REQUIRE(merge_row && merge_next && seg_ptr && n_rows, std::string(who) + ": null output");
  SNET_REQUIRE(window >= 1 && window <= 16, std::string(who) + ": window must be 1 .. 16 tiles");
  SNET_REQUIRE(tile_mode == 0 || tile_mode == 1, std::string(who) + ": tile_mode must be 0 or 1");
  SNET_REQUIRE(n_tiles >= 0 && tile_cut >= 0 && tile_cut <= n_tiles && n_src >= 0 && n_edges >= 0 && n_edges < (1ll << 31),
               std::string(who) + ": bad sizes");
  SNET_REQUIRE(n_tiles == 0 || (row_ptr && src && tile_ptr && tile_node), std::string(who) + ": null input");
  SNET_REQUIRE(n_edges == 0 || perm != nullptr, std::string(who) + ": null output");
  for (int64_t e = 0; e < n_edges; ++e) merge_row[e] = merge_next[e] = -1;
  // per window: a small open-addressing table source -> slot of the last edge seen with it (<= 256 slots per window)
  constexpr int H = 1024;
  int32_t key[H], last[H], used[16 * 16];
  for (int i = 0; i < H; ++i) key[i] = -1;
  int32_t slot_edge[16 * 16];
  int64_t rows = 0;
  const int64_t range[3] = {0, tile_cut, n_tiles};   // windows count from the start of each sub-list: none straddles the cut
  for (int part = 0; part < 2; ++part) {
    for (int64_t w0 = range[part]; w0 < range[part + 1]; w0 += window) {
      const int64_t w1 = w0 + window < range[part + 1] ? w0 + window : range[part + 1];
      int n_used = 0;
      for (int64_t t = w0; t < w1; ++t) {
        int64_t e0, cnt;
        tile_range(tile_mode, row_ptr, tile_ptr, tile_node, t, e0, cnt);
        SNET_REQUIRE(cnt >= 0 && cnt <= 16 && e0 >= 0 && e0 + cnt <= n_edges, std::string(who) + ": tile out of range");
        for (int64_t q = 0; q < cnt; ++q) {
          const int32_t e = (int32_t)(e0 + q), s = src[e], slot = (int32_t)(16 * (t - w0) + q);
          SNET_REQUIRE(s >= 0 && s < n_src, std::string(who) + ": source out of range");
          slot_edge[slot] = e;
          unsigned h = ((unsigned)s * 2654435761u) >> 22;   // 10 bits
          while (key[h] >= 0 && key[h] != s) h = (h + 1) & (H - 1);
          if (key[h] < 0) {   // first edge of the window with this source: the owner of a new row
            key[h] = s;
            used[n_used++] = (int32_t)h;
            SNET_REQUIRE(rows < (1ll << 31) - 1, std::string(who) + ": too many rows");
            merge_row[e] = (int32_t)rows++;
          } else {
            merge_next[slot_edge[last[h]]] = slot;
          }
          last[h] = slot;
        }
      }
      for (int i = 0; i < n_used; ++i) key[used[i]] = -1;
    }
  }
  *n_rows = rows;
  // segment lists of the merged rows per source, as snet_segment_sum_rows(_chunked) takes them: rows of one source in edge order
  for (int64_t s = 0; s <= n_src; ++s) seg_ptr[s] = 0;
  for (int64_t e = 0; e < n_edges; ++e)
    if (merge_row[e] >= 0) ++seg_ptr[src[e] + 1];
  for (int64_t s = 0; s < n_src; ++s) seg_ptr[s + 1] += seg_ptr[s];
  std::vector<int32_t> fill(seg_ptr, seg_ptr + n_src);
  for (int64_t e = 0; e < n_edges; ++e)
    if (merge_row[e] >= 0) perm[fill[src[e]]++] = merge_row[e];
  return 0;
}

extern "C" int snet_gxe_merge_map(const int32_t *row_ptr, const int32_t *src, const int32_t *tile_ptr, const int32_t *tile_node,
                                  int64_t n_tiles, int64_t tile_cut, int32_t tile_mode, int32_t window, int64_t n_dst, int64_t n_src,
                                  int64_t n_edges, int32_t *merge_row, int32_t *merge_next, int32_t *seg_ptr, int32_t *perm,
                                  int64_t *n_rows, void *stream) {
  const char *who = "snet_gxe_merge_map";
  SNET_REQUIRE(n_rows != nullptr && seg_ptr != nullptr, std::string(who) + ": null output");
  SNET_REQUIRE(n_tiles >= 0 && n_dst >= 0 && n_src >= 0 && n_edges >= 0, std::string(who) + ": bad sizes");
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (mode 1: the edge ranges come from tile_e0 alone -- neither the tiles' row pairs nor row_ptr are read back)
  const size_t n_tp = tile_mode == 1 ? (size_t)n_tiles + 1 : (size_t)n_dst + 1, n_tn = tile_mode == 1 ? 1 : (size_t)n_tiles;
  std::vector<int32_t> h_rp(tile_mode == 1 ? 1 : (size_t)n_dst + 1), h_src((size_t)n_edges), h_tp(n_tp), h_tn(n_tn);
  std::vector<int32_t> h_row((size_t)n_edges), h_next((size_t)n_edges), h_seg((size_t)n_src + 1), h_perm((size_t)n_edges);
  auto down = [&](std::vector<int32_t> &h, const int32_t *d) {
    return h.empty() || n_tiles == 0 || hipMemcpyAsync(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
  };
  SNET_REQUIRE((tile_mode == 1 || (down(h_rp, row_ptr) && down(h_tn, tile_node))) && down(h_src, src) && down(h_tp, tile_ptr) &&
                   hipStreamSynchronize(st) == hipSuccess,
               std::string(who) + ": readback failed");
  if (int rc = snet_gxe_merge_map_host(h_rp.data(), h_src.data(), h_tp.data(), h_tn.data(), n_tiles, tile_cut, tile_mode, window, n_src, n_edges,
                                       h_row.data(), h_next.data(), h_seg.data(), h_perm.data(), n_rows))
    return rc;
  auto up = [&](const std::vector<int32_t> &h, int32_t *d, size_t n) {
    return n == 0 || hipMemcpyAsync(d, h.data(), n * 4, hipMemcpyHostToDevice, st) == hipSuccess;
  };
  SNET_REQUIRE(up(h_row, merge_row, h_row.size()) && up(h_next, merge_next, h_next.size()) && up(h_seg, seg_ptr, h_seg.size()) &&
                   up(h_perm, perm, (size_t)*n_rows) && hipStreamSynchronize(st) == hipSuccess,
               std::string(who) + ": upload failed");
  return 0;
}
