"""fp64 restatement of the one-launch reverse pass of a scalar-output layer (snet_lastlayer_conv_bwd, include/snet_hip.h),
the hand-built graphs it is tested on and the mixed-magnitude factors, on the CPU.  Nothing here comes from a GPU kernel:
tests/test_lastlayer_cpu.py checks the restatement against autograd through the oracle's tensor product (tests/fused_range.py),
tests/test_lastlayer_gpu.py checks the kernel against the restatement."""
import math

import numpy as np
import torch

# out-degrees every graph must contain: the boundaries of the 16-edge tiles (and of one / two / three / four tiles)
DEGREES = (0, 1, 15, 16, 17, 32, 33, 49)


def path_table(spec):
    """(l, mul, weight column = g_out column, source-row offset) of every path (l, l -> 0)"""
    x_off = spec.irreps_x.offsets()
    return [(p.l1, p.mul, p.w_off, x_off[p.i_x]) for p in spec.paths]


def lastlayer_reference(spec, x, g_out, sh, dsh, edge_vec, h2, h2d, W2, w_row, row_ptr, src, scale):
    """g_x[n_total, dx] and g_vec[E, 3] of  B = scale sum_e sum_{l,u} g_out[dst(e)][l,u] w_e[l,u] c_l sum_a x[src(e)][l,u,a] Y_e[l,a]
    with w_e = h2_e W2, c_l = 1 / sqrt(2 l + 1), |r_e| entering through h2 (h2d = d h2 / d|r|) and Y_e through dsh = dY / dr.
    Edges are sorted by destination (row_ptr); everything is evaluated in fp64 from the formulas, no autograd."""
    f64 = torch.float64
    N, E, nsh, NT = row_ptr.numel() - 1, src.numel(), sh.shape[1], x.shape[0]
    node = torch.repeat_interleave(torch.arange(N), (row_ptr[1:] - row_ptr[:-1]).long())
    rows = torch.arange(E) if w_row is None else w_row.long()
    x, g_out, sh, W2 = x.to(f64), g_out.to(f64), sh.to(f64), W2.to(f64)
    w, wd = h2.to(f64)[rows] @ W2, h2d.to(f64)[rows] @ W2
    g_x = torch.zeros(NT, x.shape[1], dtype=f64)
    dY = torch.zeros(E, nsh, dtype=f64)
    g_rad = torch.zeros(E, dtype=f64)
    for l, mul, col, xo in path_table(spec):
        na, cl = 2 * l + 1, 1.0 / math.sqrt(2 * l + 1)
        X = x[src.long(), xo:xo + na * mul].reshape(E, na, mul)
        Y = sh[:, l * l:l * l + na]
        G = g_out[node, col:col + mul]
        t = scale * cl * w[:, col:col + mul] * G
        g_x[:, xo:xo + na * mul].index_add_(0, src.long(), (t[:, None, :] * Y[:, :, None]).reshape(E, na * mul))
        dY[:, l * l:l * l + na] = torch.einsum('eu,eau->ea', t, X)
        g_rad += scale * cl * (wd[:, col:col + mul] * G * torch.einsum('eau,ea->eu', X, Y)).sum(1)
    ev = edge_vec.to(f64)
    g_vec = torch.einsum('ei,eia->ea', dY[:, 1:], dsh.to(f64).reshape(E, nsh, 3)[:, 1:]) + g_rad[:, None] * ev / ev.norm(dim=1, keepdim=True)
    return g_x, g_vec


def hand_graph(n_local, n_ghost, seed, ghost_degrees=()):
    """A directed edge list built by hand: sources 0 .. 7 have the out-degrees DEGREES, the other local sources 2 .. 6, the ghost
    sources `ghost_degrees`; destinations are drawn at random among the local atoms (multi-edges allowed: they are distinct
    directed edges).  Returns the destination-sorted CSR (row_ptr, src), the source grouping (col_ptr over n_total rows, eperm,
    center_t) and unit-scale edge vectors."""
    rng = np.random.default_rng(seed)
    NT = n_local + n_ghost
    deg = np.concatenate([np.array(DEGREES), rng.integers(2, 7, n_local - len(DEGREES)), np.array(ghost_degrees, dtype=np.int64)])
    assert len(deg) == NT
    s = np.repeat(np.arange(NT), deg)
    d = rng.integers(0, n_local, len(s))
    order = np.lexsort((rng.permutation(len(s)), d))      # by destination, sources scrambled inside a row
    s, d = s[order], d[order]
    E = len(s)
    row_ptr = np.zeros(n_local + 1, np.int64)
    np.add.at(row_ptr, d + 1, 1)
    row_ptr = np.cumsum(row_ptr)
    eperm = np.argsort(s, kind='stable')
    col_ptr = np.zeros(NT + 1, np.int64)
    np.add.at(col_ptr, s + 1, 1)
    col_ptr = np.cumsum(col_ptr)
    vec = rng.normal(0, 1, (E, 3))
    vec *= (rng.uniform(1.5, 4.5, E) / np.linalg.norm(vec, axis=1))[:, None]
    out_deg = np.diff(col_ptr)
    assert set(DEGREES) <= set(out_deg.tolist())
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    return dict(N=n_local, NT=NT, E=E, row_ptr=i32(row_ptr), src=i32(s), col_ptr=i32(col_ptr), eperm=i32(eperm), center_t=i32(d[eperm]),
                edge_vec=np.ascontiguousarray(vec, dtype=np.float32))


def random_inputs(spec, g, seed, pairs=True):
    """unit-scale rows for `hand_graph` g: x[NT, dx], g_out[N, dmid], h2 / h2d[R, 64] (several edges share a radial row when `pairs`),
    W2[64, wn] at the radial network's scale"""
    rng = np.random.default_rng(seed)
    E = g['E']
    R = E // 2 + 3 if pairs else E
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return dict(x=f32(rng.normal(0, 1, (g['NT'], spec.irreps_x.dim))), g_out=f32(rng.normal(0, 1, (g['N'], spec.irreps_out.dim))),
                h2=f32(rng.normal(0, 1, (R, 64))), h2d=f32(rng.normal(0, 1, (R, 64))),
                W2=f32(rng.normal(0, 1, (64, spec.weight_numel)) / 8.0),
                w_row=np.ascontiguousarray(rng.integers(0, R, E), dtype=np.int32) if pairs else None)


def mixed_factors(g, R):
    """power-of-two factors in the manner of tests/fused_range.py: g_out rows spanning 2^+-20, h2 / h2' rows by their own tables
    (so that the rows of one 16-edge tile differ by many binades) and one all-zero h2 row"""
    from fused_range import RD_TAB, R_TAB
    tab = lambda t, n: np.array(t, dtype=np.float64)[np.arange(n) % len(t)]  # noqa: E731
    fg = 2.0 ** tab((0, 20, -20, 7, -13, 0, 20, -20), g['N'])
    fh, fhd = 2.0 ** tab(R_TAB, R), 2.0 ** tab(RD_TAB, R)
    fh[1] = 0.0
    return fg.astype(np.float32), fh.astype(np.float32), fhd.astype(np.float32)


def meta_of(blob: bytes) -> dict:
    """key -> value of the metadata block that ends a .snet file"""
    p = blob.rfind(b'chemical_symbols_to_index=')
    assert p >= 4 and int.from_bytes(blob[p - 4:p], 'little') == len(blob) - p
    return dict(line.split('=', 1) for line in blob[p:].decode().splitlines())


def without_meta_key(blob: bytes, key: str) -> bytes:
    """the same .snet file with one metadata key removed (what a file written before the key existed looks like)"""
    p = blob.rfind(b'chemical_symbols_to_index=')
    text = b''.join(line for line in blob[p:].splitlines(keepends=True) if not line.startswith(key.encode() + b'='))
    return blob[:p - 4] + len(text).to_bytes(4, 'little') + text
