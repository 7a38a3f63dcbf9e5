"""Mixed-magnitude inputs for the fp16-operand (terms = 4) fused tensor-product kernels, on the CPU: the power-of-two factor tables,
the classification of the reverse kernels' 16-edge tiles, the per-edge error bound, and the fp64 reference of the fused operation
(oracle.model.tp_uvu + autograd; nothing here comes from a GPU kernel).  Used by tests/test_fused_range_cpu.py and
tests/test_fused_range_gpu.py."""
import torch

from helpers import packed_tiles_expected

# exponents of the power-of-two factors, by destination node (g_out), source row (x) and radial row (h2; h2' in the tangent kernel)
P_TAB = (0, 0, 12, 12, -20, -20, 0, 12, -20)
Q_TAB = (0, -15, 10)
R_TAB = (0, -12, 6)
RD_TAB = (0, 9, -14)
WINDOW = 12     # an edge whose own exponent is at most this far below its tile's largest is bounded at its OWN magnitude
TOL = 2e-5      # what test_conv_fused_matches_separate_kernels grants terms = 4, as a fraction of the unit-scale maximum
CST = 1.6791767923989418   # normalize2mom constant of silu


def _tab(table, n):
    return torch.tensor(table, dtype=torch.long)[torch.arange(n) % len(table)]


def axis_exponents(c, axes):
    """exponent per destination node / source row / radial row (h2 and h2') of `_fused_case` c; axes: subset of 'pqr'"""
    z = lambda n: torch.zeros(n, dtype=torch.long)  # noqa: E731
    return dict(p=_tab(P_TAB, c['N']) if 'p' in axes else z(c['N']), q=_tab(Q_TAB, c['NT']) if 'q' in axes else z(c['NT']),
                r=_tab(R_TAB, c['R']) if 'r' in axes else z(c['R']), rd=_tab(RD_TAB, c['R']) if 'r' in axes else z(c['R']))


def edge_maps(c):
    """(destination node, source row, radial row) of every edge"""
    deg = (c['row_ptr'][1:] - c['row_ptr'][:-1]).long()
    node = torch.repeat_interleave(torch.arange(c['N']), deg)
    rows = torch.arange(c['E']) if c['w_row'] is None else c['w_row'].long()
    return node, c['src'].long(), rows


def work_list(row_ptr, N, mode):
    """(e0[nt + 1], nodes[nt, 2]) of the reverse kernels' tile list: mode 1 = packed windows over <= 2 rows
    (snet_edge_tiles_packed), mode 0 = 16-edge pieces of one row (snet_edge_tiles)"""
    if mode == 1:
        e0, nodes = packed_tiles_expected(row_ptr, 0, N)
        return torch.tensor(e0, dtype=torch.long), torch.tensor(nodes, dtype=torch.long).view(-1, 2)
    rp = [int(v) for v in row_ptr]
    e0, nodes = [], []
    for n in range(N):
        for e in range(rp[n], rp[n + 1], 16):
            e0.append(e)
            nodes.append((n, n))
    return torch.tensor(e0 + [rp[N]], dtype=torch.long), torch.tensor(nodes, dtype=torch.long).view(-1, 2)


def tile_of_edge(e0):
    E = int(e0[-1])
    return torch.searchsorted(e0, torch.arange(E), right=True) - 1


def tile_classes(nodes, p):
    """per tile: 0 = one row, 1 = two rows with the same exponent p, 2 = two rows with different p; and the exponent gap"""
    a, b = nodes[:, 0], nodes[:, 1]
    gap = (p[a] - p[b]).abs()
    cls = torch.where(a == b, 0, torch.where(gap == 0, 1, 2))
    return cls, gap


def bound_exponent(own, tile, n_tiles):
    """the exponent k of the bound tol * S * 2^k of every edge: its own, where the tile's largest is within WINDOW of it (the
    documented window of the tile scale covers the edge); the tile's largest otherwise"""
    top = torch.full((n_tiles,), -(1 << 40), dtype=torch.long).scatter_reduce(0, tile, own, 'amax')[tile]
    return torch.where(top - own <= WINDOW, own, top)


def row_exponent(own, node, N):
    """forward rows: the largest exponent among the row's own edges (0 for a row without edges)"""
    top = torch.full((N,), -(1 << 40), dtype=torch.long).scatter_reduce(0, node, own, 'amax')
    return torch.where(top < -(1 << 39), torch.zeros_like(top), top)


def hidden_layers(emb, demb, W0, W1):
    """fp64 (h2, h2') of the radial MLP's two silu layers (tests/test_tangent_cpu.py)"""
    from test_tangent_cpu import tangent_reference
    return tangent_reference(emb.double(), demb.double(), W0.double(), W1.double(), 'silu')


def hidden_backward(emb_e, W0, W1, g_h2):
    """g_emb[E, nb] = (d h2 / d emb)^T g_h2 per directed edge, fp64 autograd through the two hidden layers"""
    e = emb_e.double().clone().requires_grad_(True)
    a1 = torch.nn.functional.silu(e @ W0.double()) * CST
    a2 = torch.nn.functional.silu(a1 @ W1.double()) * CST
    (g,) = torch.autograd.grad(a2, e, g_h2.double())
    return g


def fused_reference(spec, x, sh, dsh, h2, W2, w_row, row_ptr, src, scale, g_out, h2d=None):
    """fp64 reference of the fused operation on engine (ir_mul) rows: w = h2[w_row] W2 -> uvu tensor product -> segment sum, and its
    gradients by autograd.  Returns out[N, dout], the per-edge messages msg[E, dout] (out = their sum per destination row),
    g_xe[E, dx], g_h2[E, 64] = g_w W2^T, the spherical part of g_vec[E, 3] = dE/dY . dsh (Y_0 is constant: its Jacobian row is not
    read) and, given h2' rows, the radial scalar g_rad[E] = sum_k g_w[e, k] (h2' W2)[k] -- and what else tests/conv_shapes.conv_reference
    returns: it is that function, which takes any ConvSpec of the catalogue."""
    from conv_shapes import conv_reference
    return conv_reference(spec, x, sh, dsh, w_row, row_ptr, src, scale, g_out, h2=h2, W2=W2, h2d=h2d)


def scaled_reference(ref, c, fg, fx, fh, fhd):
    """the reference for g_out[n] * fg[n], x[s] * fx[s], h2[r] * fh[r], h2'[r] * fhd[r] from the unit-scale one.  Every output is
    linear in each of these rows, and the factors are powers of two (or zero), so in fp64 this equals `fused_reference` of the scaled
    inputs up to its own rounding (tests/test_fused_range_cpu.py checks that)."""
    node, src, rows = edge_maps(c)
    g, x, h, hd = fg.double()[node], fx.double()[src], fh.double()[rows], fhd.double()[rows]
    out = torch.zeros_like(ref['out']).index_add_(0, node, ref['msg'] * (x * h)[:, None])
    return dict(out=out, g_xe=ref['g_xe'] * (g * h)[:, None], g_h2=ref['g_h2'] * (g * x)[:, None],
                g_vec=ref['g_vec'] * (g * x * h)[:, None], g_rad=ref['g_rad'] * (g * x * hd))
