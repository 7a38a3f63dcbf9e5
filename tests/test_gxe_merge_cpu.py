"""CPU: the merge map of the merged-store reverse kernel (snet_gxe_merge_map_host, include/snet_hip.h) against the numpy
restatement of tests/gxe_merge.py, on graphs where sources are shared across centres, inside one centre (periodic images), not at
all, and on the degenerate lists."""
import numpy as np
import pytest

import gxe_merge as gm


def _lib():
    from sevennet_amd import _lib
    return _lib.load()


def _case(name):
    """-> (mode, row_ptr, src, tile_ptr, tile_node, n_tiles, cut, window, n_src)"""
    if name in ('cell64', 'cell64_w8', 'cell64_last_window', 'cell64_brick'):
        rp, src, _ = gm.diamond_graph((2, 2, 2))
        n = len(rp) - 1
        cut = 40 if name == 'cell64_brick' else 0   # rows [0, 40) interior, [40, 64) boundary: two sub-lists
        tp, tn, nt, k = gm.tile_lists(rp, n, cut)
        window = 8 if name == 'cell64_w8' else 4
        if name == 'cell64_last_window':
            window = next(w for w in (4, 3, 5) if nt % w)   # the last window has fewer tiles
        return 1, rp, src, tp, tn, nt, k, window, n
    if name == 'cell8':   # 8 atoms, cutoff 5 A > a / 2: a source reaches one centre through several images
        rp, src, _ = gm.diamond_graph((1, 1, 1))
        n = len(rp) - 1
        assert max(np.bincount(src[rp[i]:rp[i + 1]]).max() for i in range(n)) > 1
        tp, tn, nt, k = gm.tile_lists(rp, n)
        return 1, rp, src, tp, tn, nt, k, 4, n
    if name == 'no_shared':   # every edge its own source: merged rows == edges
        deg = np.array([3, 16, 17, 5, 0, 40])
        rp = np.zeros(len(deg) + 1, np.int32)
        rp[1:] = np.cumsum(deg)
        src = np.arange(rp[-1], dtype=np.int32)[::-1].copy()
        tp, tn, nt, k = gm.tile_lists(rp, len(deg))
        return 1, rp, src, tp, tn, nt, k, 4, int(rp[-1])
    if name == 'empty':
        return 1, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32), 0, 0, 4, 5
    if name in ('gaps_short_tiles', 'per_row_tiles'):   # rows without edges, tiles shorter than 16, ghost sources (>= n_local)
        rng = np.random.default_rng(5)
        deg = np.array([0, 0, 2, 0, 1, 19, 0, 3, 3, 0, 33, 1, 0])
        rp = np.zeros(len(deg) + 1, np.int32)
        rp[1:] = np.cumsum(deg)
        src = rng.integers(0, len(deg) + 3, rp[-1]).astype(np.int32)
        if name == 'per_row_tiles':
            tp, tn, nt = gm.per_row_tiles(rp, len(deg))
            return 0, rp, src, tp, tn, nt, 0, 4, len(deg) + 3
        tp, tn, nt, k = gm.tile_lists(rp, len(deg))
        assert (np.diff(tp) < 16).any()
        return 1, rp, src, tp, tn, nt, k, 4, len(deg) + 3
    raise KeyError(name)


CASES = ['cell64', 'cell64_w8', 'cell64_last_window', 'cell64_brick', 'cell8', 'no_shared', 'empty', 'gaps_short_tiles', 'per_row_tiles']


@pytest.mark.parametrize('name', CASES)
def test_merge_map_matches_the_restatement(name):
    mode, rp, src, tp, tn, nt, cut, window, n_src = c = _case(name)
    want = gm.merge_expected(*c)
    got = gm.native_map(_lib(), *c)
    E = len(src)
    assert got['n_rows'] == want['n_rows']                      # merged row count equals the numpy count
    for k in ('row', 'next', 'seg', 'perm'):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # the properties themselves, from the native arrays alone
    row, nxt = got['row'], got['next']
    owner = np.full(E, -1, np.int64)
    for lo, hi in ((0, cut), (cut, nt)):
        for w0 in range(lo, hi, window):
            slots = {}
            for t in range(w0, min(w0 + window, hi)):
                e0, cnt = gm.tile_edges(mode, rp, tp, tn, t)
                for q in range(cnt):
                    slots[16 * (t - w0) + q] = e0 + q
            for slot in sorted(slots):          # walk every owner's chain: slot order, same source, every edge reached once
                e = slots[slot]
                if row[e] < 0:
                    continue
                owner[e], at = e, e
                while nxt[at] >= 0:
                    assert nxt[at] > max(s for s, ee in slots.items() if ee == at)
                    at = slots[int(nxt[at])]
                    assert owner[at] == -1 and src[at] == src[e] and row[at] == -1
                    owner[at] = e
    assert (owner >= 0).all()                                    # every edge maps to exactly one owner ...
    assert (src[owner] == src).all() and (owner <= np.arange(E)).all()   # ... with its source, first in edge order
    np.testing.assert_array_equal(owner, want['owner'])
    n = got['n_rows']
    assert sorted(row[row >= 0]) == list(range(n))
    assert sorted(got['perm']) == list(range(n))                 # the segment lists cover every merged row exactly once
    row_src = np.empty(n, np.int64)
    row_src[row[row >= 0]] = src[row >= 0]
    for s in range(n_src):
        assert (row_src[got['perm'][got['seg'][s]:got['seg'][s + 1]]] == s).all()
    assert got['seg'][0] == 0 and got['seg'][-1] == n
    if name == 'no_shared':
        assert n == E
    if name == 'cell64':
        assert n < 0.8 * E                                       # sources ARE shared across neighbouring centres
    if name == 'cell64_brick':
        # no window straddles the cut: no chain links an interior edge and a boundary edge
        e_cut = int(tp[cut])
        assert ((owner < e_cut) == (np.arange(E) < e_cut)).all()


def test_arguments_are_checked():
    lib = _lib()
    c = list(_case('cell8'))
    for pos, bad in ((7, 0), (7, 17), (0, 2), (6, c[5] + 1)):   # window, window, tile mode, cut past the end
        d = list(c)
        d[pos] = bad
        with pytest.raises(RuntimeError):
            gm.native_map(lib, *d)
    d = list(c)
    d[2] = c[2].copy()
    d[2][3] = c[8] + 5   # a source outside [0, n_src)
    with pytest.raises(RuntimeError):
        gm.native_map(lib, *d)
