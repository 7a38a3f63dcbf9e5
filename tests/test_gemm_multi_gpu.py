"""GPU: snet_gemm_multi, the two-source grouped GEMM (C = A0 B0 + A1 B1 (+ table[types]), written once), at op level.

Reference: the fp64 numpy product.  Yardstick: the write-then-accumulate pair of snet_gemm_grouped launches it replaces, on the
same inputs (source 1 written, source 0 accumulated onto it -- the forward order sc, then SI2): the two-source launch's largest
error may be at most RATIO = 1.5 times the pair's (the project's bar for a change of arithmetic), launch by launch.
Both errors are printed.  The kernel keeps one accumulator set per source and adds them at the store, which is the sum the
accumulating epilogue formed: beyond the bar, the two-source result is asserted to BE the pair's, bit for bit.  (A first version
ran one accumulator set through both sources; its figures, 1.35 .. 1.8 times the pair's error at K = 224 + 128, are in DESIGN 4m.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from stream_order import run_ab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RATIO = 1.5
NS = (32, 64, 96, 224)          # 96 and 224 end in a partial column block (of 64- / 128-wide blocks)
NODES = (1, 37, 129)            # below a wave's 32 rows, a ragged tile, just across the 128-row workgroup boundary
K_PAIRS = [(20, 8), (224, 128), (64, 32), (10, 6), (64, None)]   # (20, 8): both end in a partial k step; (10, 6): no 16-byte loads


def _lib():
    from sevennet_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pack(L, lib, B):
    Bh = np.ascontiguousarray(B, np.float32)
    K, N = Bh.shape
    buf = np.empty(int(lib.snet_gemm_split_size(K, N)), np.uint8)
    L.check(lib.snet_gemm_split_pack(C.c_void_p(Bh.ctypes.data), K, N, C.c_void_p(buf.ctypes.data)))
    return torch.from_numpy(buf).to(DEV)


class _Src:
    """one source: rows A[n_total, stride] holding the (d, K) block at a non-zero 16-byte-aligned offset, weights B[K, N]"""

    def __init__(self, L, lib, rng, n_total, d, K, N, off, pad, scale=None):
        self.d, self.K, self.N, self.off = d, K, N, off
        self.stride = off + d * K + pad
        a = rng.standard_normal((n_total, self.stride)).astype(np.float32)
        if scale is not None:
            a *= scale[:, None].astype(np.float32)
        self.a_host = a
        self.b_host = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
        self.A = torch.from_numpy(a).to(DEV)
        self.packed = _pack(L, lib, self.b_host)

    def product(self, nodes):
        """fp64 [len(nodes), d * N]"""
        blk = self.a_host[nodes, self.off:self.off + self.d * self.K].astype(np.float64).reshape(len(nodes), self.d, self.K)
        return np.einsum('nmk,kj->nmj', blk, self.b_host.astype(np.float64)).reshape(len(nodes), self.d * self.N)


def _multi(L, lib, probs, Cm, n, rows=None, table=None, types=None, stream=None):
    """probs: [(c_off, d, N, [_Src, ...])]"""
    arr = (L.GemmMultiDesc * len(probs))()
    for p, (c_off, d, N, srcs) in zip(arr, probs):
        p.c_off, p.n_src, p.d, p.N = c_off, len(srcs), d, N
        for s, src in zip(p.src, srcs):
            s.A, s.B_split, s.a_node_stride, s.a_off, s.K = src.A.data_ptr(), src.packed.data_ptr(), src.stride, src.off, src.K
    return lib.snet_gemm_multi(arr, len(probs), _p(Cm), n, Cm.shape[1], _p(rows), _p(table), _p(types), stream)


def _grouped(L, lib, items, Cm, n, rows=None):
    """items: [(c_off, _Src, accumulate)] -- they share A and its stride"""
    descs = (L.GemmDesc * len(items))(*[L.GemmDesc(None, s.packed.data_ptr(), s.off, c_off, s.d, s.K, s.N, int(acc))
                                        for c_off, s, acc in items])
    L.check(lib.snet_gemm_grouped(descs, len(items), _p(items[0][1].A), _p(Cm), n, items[0][1].stride, Cm.shape[1], _p(rows), None))


def _pair(L, lib, c_off, s0, s1, Cm, n, rows=None):
    """what the two-source launch replaces: source 1 written, source 0 accumulated onto it"""
    _grouped(L, lib, [(c_off, s1, 0)], Cm, n, rows)
    _grouped(L, lib, [(c_off, s0, 1)], Cm, n, rows)


@pytest.mark.parametrize('d', [1, 3, 5])
@pytest.mark.parametrize('kpair', K_PAIRS, ids=lambda k: f'K{k[0]}+{k[1]}')
def test_two_source_vs_fp64_and_vs_the_accumulating_pair(d, kpair):
    L, lib = _lib()
    rng = np.random.default_rng(100 * d + kpair[0])
    K0, K1 = kpair
    worst_new = worst_old = 0.0
    for N in NS:
        for n in NODES:
            s0 = _Src(L, lib, rng, n, d, K0, N, off=8, pad=4)                       # like m at its own stride
            s1 = _Src(L, lib, rng, n, d, K1, N, off=12, pad=8) if K1 else None      # like x: another stride and offset
            c_off, c_stride = 4, 4 + d * N + 12
            fill = torch.from_numpy(rng.standard_normal((n, c_stride)).astype(np.float32)).to(DEV)
            Cn, Co = fill.clone(), fill.clone()
            L.check(_multi(L, lib, [(c_off, d, N, [s0] + ([s1] if s1 else []))], Cn, n), 'snet_gemm_multi')
            if s1 is None:
                _grouped(L, lib, [(c_off, s0, 0)], Co, n)
            else:
                _pair(L, lib, c_off, s0, s1, Co, n)
            torch.cuda.synchronize()
            nodes = np.arange(n)
            ref = s0.product(nodes) + (s1.product(nodes) if s1 else 0.0)
            blk = slice(c_off, c_off + d * N)
            e_new = np.abs(Cn[:, blk].double().cpu().numpy() - ref).max()
            e_old = np.abs(Co[:, blk].double().cpu().numpy() - ref).max()
            print(f'd={d} K={kpair} N={N} n={n}: max|err| two-source {e_new:.3e}, pair {e_old:.3e}, max|ref| {np.abs(ref).max():.3f}')
            worst_new, worst_old = max(worst_new, e_new), max(worst_old, e_old)
            assert e_new <= RATIO * e_old, (d, kpair, N, n)
            assert torch.equal(Cn, Co), (d, kpair, N, n)      # one source: the grouped kernel's bits; two: the pair's
            # columns outside the block are bit-unchanged
            assert torch.equal(Cn[:, :c_off], fill[:, :c_off]) and torch.equal(Cn[:, c_off + d * N:], fill[:, c_off + d * N:])
    print(f'd={d} K={kpair}: largest error two-source {worst_new:.3e}, pair {worst_old:.3e}, ratio {worst_new / worst_old:.3f}')
    assert worst_old > 0 and worst_new <= RATIO * worst_old


def _three_block_case(L, lib, rng, n_total, two=True, scale=None):
    """the node-linear layout: blocks d = 1, 3, 5 with N = 96, 64, 32 covering all 448 columns of C; source 0 rows at stride 3136-like
    (here 8 + d K + 4 per block source), source 1 at another"""
    probs, c_off = [], 0
    for d, N, K0, K1 in ((1, 96, 224, 128), (3, 64, 64, 32), (5, 32, 20, 8)):
        s0 = _Src(L, lib, rng, n_total, d, K0, N, off=8, pad=4, scale=scale)
        s1 = _Src(L, lib, rng, n_total, d, K1, N, off=12, pad=8, scale=scale)
        probs.append((c_off, d, N, [s0, s1] if two else [s0]))
        c_off += d * N
    return probs, c_off


def _ref(probs, nodes, second=None):
    out = []
    for k, (c_off, d, N, srcs) in enumerate(probs):
        r = srcs[0].product(nodes)
        if len(srcs) > 1:
            r = r + (second[k] if second is not None else srcs[1]).product(nodes)
        out.append(r)
    return np.concatenate(out, 1)


def test_permuted_row_list_over_a_subset():
    L, lib = _lib()
    rng = np.random.default_rng(7)
    n_total, n = 129, 37
    probs, dim = _three_block_case(L, lib, rng, n_total)
    rows_h = rng.permutation(n_total)[:n].astype(np.int32)
    rows = torch.from_numpy(rows_h).to(DEV)
    fill = torch.from_numpy(rng.standard_normal((n_total, dim)).astype(np.float32)).to(DEV)
    Cn, Co = fill.clone(), fill.clone()
    L.check(_multi(L, lib, probs, Cn, n, rows=rows), 'snet_gemm_multi')
    for c_off, d, N, (s0, s1) in probs:
        _pair(L, lib, c_off, s0, s1, Co, n, rows)
    torch.cuda.synchronize()
    ref = _ref(probs, rows_h)
    e_new = np.abs(Cn[rows.long()].double().cpu().numpy() - ref).max()
    e_old = np.abs(Co[rows.long()].double().cpu().numpy() - ref).max()
    print(f'row list: max|err| two-source {e_new:.3e}, pair {e_old:.3e}')
    assert e_new <= RATIO * e_old and torch.equal(Cn, Co)
    off = np.setdiff1d(np.arange(n_total), rows_h)
    assert torch.equal(Cn[off], fill[off])          # rows outside the list: bit-unchanged


def test_two_species_lists_write_every_row_once():
    """per-species source-1 weights (the FCTP self-connection) with shared source-0 weights, one launch per list"""
    L, lib = _lib()
    rng = np.random.default_rng(8)
    n_total = 129
    probs, dim = _three_block_case(L, lib, rng, n_total)
    other = []      # species 1: same rows of source 1, other weights
    for c_off, d, N, (s0, s1) in probs:
        o = _Src.__new__(_Src)
        o.__dict__.update(s1.__dict__)
        o.b_host = (rng.standard_normal((s1.K, N)) / np.sqrt(s1.K)).astype(np.float32)
        o.packed = _pack(L, lib, o.b_host)
        other.append(o)
    probs1 = [(c_off, d, N, [s0, o]) for (c_off, d, N, (s0, _)), o in zip(probs, other)]
    perm = rng.permutation(n_total).astype(np.int32)
    lists = [perm[:50], perm[50:]]
    Cn = torch.full((n_total, dim), float('nan'), device=DEV)
    Co = torch.full((n_total, dim), float('nan'), device=DEV)
    for rows_h, pr in zip(lists, (probs, probs1)):
        rows = torch.from_numpy(rows_h).to(DEV)
        L.check(_multi(L, lib, pr, Cn, len(rows_h), rows=rows), 'snet_gemm_multi')
        for c_off, d, N, (s0, s1) in pr:
            _pair(L, lib, c_off, s0, s1, Co, len(rows_h), rows)
    torch.cuda.synchronize()
    assert not torch.isnan(Cn).any()                # together the lists write every row
    ref = np.empty((n_total, dim))
    ref[lists[0]] = _ref(probs, lists[0])
    ref[lists[1]] = _ref(probs1, lists[1])
    e_new = np.abs(Cn.double().cpu().numpy() - ref).max()
    e_old = np.abs(Co.double().cpu().numpy() - ref).max()
    print(f'two species lists: max|err| two-source {e_new:.3e}, pair {e_old:.3e}')
    assert e_new <= RATIO * e_old and torch.equal(Cn, Co)


@pytest.mark.parametrize('n', NODES)
def test_table_row_equals_embed_rows_plus_accumulating_gemm(n):
    L, lib = _lib()
    rng = np.random.default_rng(9 + n)
    probs, dim = _three_block_case(L, lib, rng, n, two=False)
    table = torch.from_numpy(rng.standard_normal((3, dim)).astype(np.float32)).to(DEV)
    types = torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)).to(DEV)
    Cn = torch.full((n, dim), float('nan'), device=DEV)
    Co = torch.full((n, dim), float('nan'), device=DEV)
    L.check(_multi(L, lib, probs, Cn, n, table=table, types=types), 'snet_gemm_multi')
    L.check(lib.snet_embed_rows(_p(table), _p(types), _p(Co), n, dim, None), 'snet_embed_rows')
    for c_off, d, N, (s0,) in probs:
        _grouped(L, lib, [(c_off, s0, 1)], Co, n)
    torch.cuda.synchronize()
    assert torch.equal(Cn, Co)
    # two sources and the table: the plain two-source result plus the row, one fp32 rounding
    probs2, _ = _three_block_case(L, lib, rng, n)
    Cp, Ct = torch.empty(n, dim, device=DEV), torch.empty(n, dim, device=DEV)
    L.check(_multi(L, lib, probs2, Cp, n), 'snet_gemm_multi')
    L.check(_multi(L, lib, probs2, Ct, n, table=table, types=types), 'snet_gemm_multi')
    torch.cuda.synchronize()
    assert torch.equal(Ct, Cp + table[types.long()])


def test_rows_of_mixed_magnitude_hold_the_bound_relative_to_their_own_row():
    L, lib = _lib()
    rng = np.random.default_rng(10)
    n = 129
    scale = 10.0 ** np.linspace(-20, 5, n)
    rng.shuffle(scale)
    probs, dim = _three_block_case(L, lib, rng, n, scale=scale)
    Cn, Co = torch.empty(n, dim, device=DEV), torch.empty(n, dim, device=DEV)
    L.check(_multi(L, lib, probs, Cn, n), 'snet_gemm_multi')
    for c_off, d, N, (s0, s1) in probs:
        _pair(L, lib, c_off, s0, s1, Co, n)
    torch.cuda.synchronize()
    assert torch.isfinite(Cn).all()
    ref = _ref(probs, np.arange(n))
    e_new = (np.abs(Cn.double().cpu().numpy() - ref) / scale[:, None]).max()
    e_old = (np.abs(Co.double().cpu().numpy() - ref) / scale[:, None]).max()
    print(f'rows scaled 1e-20 .. 1e5: max|err| / row scale two-source {e_new:.3e}, pair {e_old:.3e}')
    assert e_new <= RATIO * e_old and torch.equal(Cn, Co)


def test_empty_and_refused_launches():
    L, lib = _lib()
    rng = np.random.default_rng(11)
    probs, dim = _three_block_case(L, lib, rng, 5)
    Cm = torch.zeros(5, dim, device=DEV)
    arr = (L.GemmMultiDesc * 1)()
    assert lib.snet_gemm_multi(arr, 1, None, 0, dim, None, None, None, None) == 0        # n_nodes = 0: before any pointer check
    assert _multi(L, lib, probs, Cm, 0) == 0
    assert _multi(L, lib, probs, Cm, 5) == 0
    # mixed packed / fp32 weights
    arr = (L.GemmMultiDesc * 1)()
    c_off, d, N, (s0, s1) = probs[0]
    p = arr[0]
    p.c_off, p.n_src, p.d, p.N = c_off, 2, d, N
    for s, src in zip(p.src, (s0, s1)):
        s.A, s.B_split, s.a_node_stride, s.a_off, s.K = src.A.data_ptr(), src.packed.data_ptr(), src.stride, src.off, src.K
    assert lib.snet_gemm_multi(arr, 1, _p(Cm), 5, dim, None, None, None, None) == 0
    w32 = torch.from_numpy(s1.b_host).to(DEV)
    p.src[1].B_split, p.src[1].B = None, w32.data_ptr()
    assert lib.snet_gemm_multi(arr, 1, _p(Cm), 5, dim, None, None, None, None) != 0 and b'mix' in lib.snet_last_error()
    p.src[0].B_split, p.src[0].B = None, w32.data_ptr()                                    # fp32 only: not served either
    assert lib.snet_gemm_multi(arr, 1, _p(Cm), 5, dim, None, None, None, None) != 0
    # more than two sources, more than 8 problems, a table without types
    p.src[0].B_split, p.src[0].B, p.src[1].B_split, p.src[1].B = s0.packed.data_ptr(), None, s1.packed.data_ptr(), None
    p.n_src = 3
    assert lib.snet_gemm_multi(arr, 1, _p(Cm), 5, dim, None, None, None, None) != 0
    p.n_src = 2
    nine = (L.GemmMultiDesc * 9)(*[arr[0]] * 9)
    assert lib.snet_gemm_multi(nine, 9, _p(Cm), 5, dim, None, None, None, None) != 0
    assert lib.snet_gemm_multi(arr, 1, _p(Cm), 5, dim, None, _p(Cm), None, None) != 0
    torch.cuda.synchronize()


def test_on_a_delayed_non_default_stream():
    """the stream contract (tests/stream_order.py): both sources late behind a delay on a fresh stream"""
    L, lib = _lib()
    rng = np.random.default_rng(12)
    n = 301
    probs, dim = _three_block_case(L, lib, rng, n)
    table = torch.from_numpy(rng.standard_normal((3, dim)).astype(np.float32)).to(DEV)
    types = torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)).to(DEV)
    late = []
    for k, (_, _, _, srcs) in enumerate(probs):
        for e, s in enumerate(srcs):
            b = (s.A.double() * 1.1 + 0.01).float()
            late.append((s.A, s.A.clone(), b))
    out = torch.empty(n, dim, device=DEV)
    torch.cuda.synchronize()

    def call():
        L.check(_multi(L, lib, probs, out, n, table=table, types=types, stream=L.stream()), 'snet_gemm_multi')
    run_ab('snet_gemm_multi', late, call, [out])
