"""Shared by tests/test_gxe_merge_cpu.py and tests/test_gxe_merge_gpu.py: small graphs as CSR lists sorted by centre, their packed
tile lists (tests/helpers.packed_tiles_expected), a numpy restatement of the merge map (snet_gxe_merge_map, include/snet_hip.h) and
the native map on host arrays (snet_gxe_merge_map_host).  Nothing here touches a GPU."""
import ctypes as C

import numpy as np

from helpers import packed_tiles_expected


def diamond_graph(reps, cutoff=5.0, sigma=0.05, seed=2):
    """(row_ptr[n + 1], src[E], edge_vec[E, 3]) of a periodic diamond cell, edges sorted by centre (stable: the list's own order
    inside a row)"""
    from sevennet_amd.neighbor import diamond_cubic, neighbor_list
    pos, cell = diamond_cubic(5.431, reps, sigma, seed)
    ei, vec, _ = neighbor_list(pos, cell, [True] * 3, cutoff)
    order = np.argsort(ei[0], kind='stable')
    deg = np.bincount(ei[0], minlength=len(pos))
    row_ptr = np.zeros(len(pos) + 1, np.int32)
    row_ptr[1:] = np.cumsum(deg)
    return row_ptr, ei[1][order].astype(np.int32), vec[order].astype(np.float32)


def tile_lists(row_ptr, n_local, cut=0):
    """packed tiles of rows [0, cut) and [cut, n_local) as ONE list -> (tile_e0[n + 1], tile_nodes[2 n], n, k): what both hosts build"""
    e0a, na = packed_tiles_expected(row_ptr, 0, cut) if cut else ([int(row_ptr[0])], [])
    e0b, nb = packed_tiles_expected(row_ptr, cut, n_local)
    k = len(e0a) - 1
    e0 = e0a[:k] + e0b
    return np.asarray(e0, np.int32), np.asarray(na + nb, np.int32), len(e0) - 1, k


def per_row_tiles(row_ptr, n_local):
    """mode-0 tiles (snet_edge_tiles): 16-edge pieces of one row -> (tile_ptr[n_local + 1], tile_node[n], n)"""
    deg = np.diff(np.asarray(row_ptr[:n_local + 1], np.int64))
    cnt = (deg + 15) // 16
    tp = np.zeros(n_local + 1, np.int32)
    tp[1:] = np.cumsum(cnt)
    return tp, np.repeat(np.arange(n_local, dtype=np.int32), cnt), int(tp[-1])


def tile_edges(mode, row_ptr, tile_ptr, tile_node, t):
    if mode == 1:
        return int(tile_ptr[t]), int(tile_ptr[t + 1] - tile_ptr[t])
    node = int(tile_node[t])
    e0 = int(row_ptr[node]) + 16 * (t - int(tile_ptr[node]))
    return e0, min(16, int(row_ptr[node + 1]) - e0)


def merge_expected(mode, row_ptr, src, tile_ptr, tile_node, n_tiles, cut, window, n_src):
    """numpy restatement: windows of `window` tiles counted from the start of [0, cut) and of [cut, n_tiles); inside a window the
    first edge (in edge order) of every source owns a new row, numbered in that order; every edge points to the slot of the next
    edge of its window with its source.  Segment lists: the owners of every source, in edge order."""
    E = len(src)
    row, nxt = np.full(E, -1, np.int32), np.full(E, -1, np.int32)
    owner = np.full(E, -1, np.int64)
    n = 0
    for lo, hi in ((0, cut), (cut, n_tiles)):
        for w0 in range(lo, hi, window):
            first, last = {}, {}
            for t in range(w0, min(w0 + window, hi)):
                e0, cnt = tile_edges(mode, row_ptr, tile_ptr, tile_node, t)
                for q in range(cnt):
                    e, s, slot = e0 + q, int(src[e0 + q]), 16 * (t - w0) + q
                    if s not in first:
                        first[s] = e
                        row[e] = n
                        n += 1
                    else:
                        nxt[last[s]] = slot
                    last[s] = e
                    owner[e] = first[s]
    owners = np.nonzero(row >= 0)[0]
    by_src = owners[np.argsort(src[owners], kind='stable')]
    seg = np.zeros(n_src + 1, np.int32)
    seg[1:] = np.cumsum(np.bincount(src[owners], minlength=n_src))
    return dict(row=row, next=nxt, owner=owner, seg=seg, perm=row[by_src].astype(np.int32), n_rows=n)


def native_map(lib, mode, row_ptr, src, tile_ptr, tile_node, n_tiles, cut, window, n_src):
    """snet_gxe_merge_map_host on numpy arrays -> the same dict as merge_expected (without `owner`)"""
    from sevennet_amd import _lib
    E = len(src)
    arrs = [np.ascontiguousarray(a, np.int32) for a in (row_ptr, src, tile_ptr, tile_node)]
    row, nxt, perm = (np.full(max(E, 1), -7, np.int32) for _ in range(3))
    seg = np.full(n_src + 1, -7, np.int32)
    n = C.c_int64(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _lib.check(lib.snet_gxe_merge_map_host(*[p(a) for a in arrs], n_tiles, cut, mode, window, n_src, E, p(row), p(nxt), p(seg), p(perm),
                                           C.byref(n)), 'snet_gxe_merge_map_host')
    return dict(row=row[:E], next=nxt[:E], seg=seg, perm=perm[:n.value], n_rows=int(n.value))
