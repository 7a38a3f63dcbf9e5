"""GPU: the fp16-operand (terms = 4, the engine default) fused tensor-product kernels on inputs of mixed magnitude.

snet_conv_fwd_fused, snet_conv_bwd_fused (g_h2 output and hidden-layer tail) and snet_conv_bwd_fused_tangent scale every fp16
operand by ONE power of two per 16-edge tile, derived from bounds (x_max[src] g_max[node] max|Y| KC |scale| for g_w; the largest
entry for h2 and h2').  Here g_out rows, source rows and radial rows carry power-of-two factors that differ INSIDE tiles
(tests/fused_range.py; tests/test_fused_range_cpu.py shows that they do), and every output is held, per edge, to
    |kernel - fp64| <= 2e-5 * S * 2^k
with S the largest reference entry of that output at unit scale and k the edge's own exponent where its tile's largest exponent is
within 12 of it, the tile's largest otherwise.  The fp64 reference is fused_range.fused_reference (oracle tensor product + autograd
on the CPU).  Where no fp16 operand mixes two exponents the results must moreover scale bit for bit."""
import ctypes as C
import functools

import pytest
import torch

import fused_range as fr
from test_ops_gpu import _fused_case, _lib, _p, _work_list

pytestmark = pytest.mark.gpu
SCALE = 0.25
SHAPES = {'7net0_mid': ('sevennet_0', 1, True), '7net0_first': ('sevennet_0', 0, False), 'l3i5_mid': ('sevennet_l3i5', 1, True)}
ZERO_NODE, ZERO_SRC = 8, 3   # a 70-edge row (whole tiles with a zero bound) and a source row, zeroed in the 'zero' case


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs and unit-scale fp64 reference of one shape, computed once and shared (never modified) by all its cases"""
    model, layer, pairs = SHAPES[shape]
    c = _fused_case(model, layer, 40 + layer, pairs)
    g = torch.Generator().manual_seed(7)
    c['demb'] = torch.randn(c['R'], c['nb'], generator=g)   # d emb / d|r| of every radial row
    h2, h2d = fr.hidden_layers(c['emb'], c['demb'], c['W0'], c['W1'])
    c['h2'], c['h2d'] = h2.float(), h2d.float()    # inputs of the kernels: the reference takes the fp32 values as given
    c['vec'] = torch.randn(c['E'], 3, generator=g)
    ref = fr.fused_reference(c['spec'], c['x'], c['sh'], c['dsh'], c['h2'], c['W2'], c['w_row'], c['row_ptr'], c['src'], SCALE,
                             c['g_out'], c['h2d'])
    return c, ref


class _Kernels:
    """plans of one shape at terms = 4, the work list in the plan's format, and one run of all four kernels"""

    def __init__(self, c):
        self.L, self.lib = _lib()
        L, lib, self.c, self.dev = self.L, self.lib, c, 'cuda:0'
        fp = lambda t: t.numpy().ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        self.mlp, self.plan, self.fplan = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(lib.snet_radial_mlp_plan_create(c['nb'], 64, 64, c['wn'], fp(c['W0']), fp(c['W1']), fp(c['W2']), 0, fr.CST, 1, C.byref(self.mlp)))
        L.check(lib.snet_conv_plan_create(c['spec'].tag.encode(), C.byref(self.plan)))
        assert lib.snet_conv_fused_available(self.plan) == 1
        L.check(lib.snet_fused_plan_create(self.plan, self.mlp, 4, C.byref(self.fplan)))
        assert lib.snet_fused_plan_has_mlp_tail(self.fplan) == 1
        self.mode = lib.snet_fused_plan_tile_mode(self.fplan)
        dev = self.dev
        self.rp, self.sr = c['row_ptr'].to(dev), c['src'].to(dev)
        self.wr = None if c['w_row'] is None else c['w_row'].to(dev)
        self.sh, self.dsh, self.vec = c['sh'].to(dev), c['dsh'].to(dev), c['vec'].to(dev)
        self.dsh0 = torch.zeros_like(self.dsh)
        self.axis = torch.tensor([2.0, 0.0, 0.0]).repeat(c['E'], 1).to(dev)   # |r| = 2 exactly: g_vec[:, 0] is the radial scalar itself
        emb_e = c['emb'] if c['w_row'] is None else c['emb'][c['w_row'].long()]
        self.emb_e = emb_e.contiguous().to(dev)
        self.tile_ptr, self.tile_node, self.n_tiles = _work_list(L, lib, self.fplan, self.rp, c['row_ptr'], c['N'], c['E'], dev)
        cp = (C.c_int32 * (c['dx'] // 16))()
        L.check(lib.snet_fused_plan_gxe_chunks(self.fplan, cp, c['dx'] // 16))
        self.col = (torch.tensor(list(cp), dtype=torch.long)[:, None] * 16 + torch.arange(16)[None, :]).reshape(-1)

    def tiles(self):
        """(first edge of every tile + end, the tile's two rows) read back from the device lists"""
        c, nt = self.c, self.n_tiles.value
        tp, tn = self.tile_ptr.cpu().long(), self.tile_node.cpu().long()
        if self.mode == 1:
            return tp[:nt + 1], tn[:2 * nt].view(-1, 2)
        node = tn[:nt]
        e0 = c['row_ptr'].long()[node] + 16 * (torch.arange(nt) - tp[node])
        return torch.cat([e0, c['row_ptr'].long()[-1:]]), torch.stack([node, node], 1)

    def run(self, x, h2, h2d, g_out, gx, tail):
        """all outputs (CPU, g_xe in standard column order).  Outputs the kernels overwrite start as NaN, accumulated ones as 0."""
        L, lib, c, dev = self.L, self.lib, self.c, self.dev
        N, E, NT, dx = c['N'], c['E'], c['NT'], c['dx']
        x, h2, h2d, g_out = (t.contiguous().to(dev) for t in (x, h2, h2d, g_out))
        nan = lambda *s: torch.full(s, float('nan'), device=dev)  # noqa: E731
        zero = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
        x_max, g_max = nan(NT), nan(N)
        L.check(lib.snet_row_absmax(_p(x), NT, dx, _p(x_max), None))
        L.check(lib.snet_row_absmax(_p(g_out), N, c['dout'], _p(g_max), None))
        o = dict(out=nan(N, c['dout']), g_h2=nan(E, 64), g_vec=zero(E, 3), t_g_vec=zero(E, 3), t_rad=zero(E, 3))
        if gx:
            o.update(g_xe=nan(E, dx), t_g_xe=nan(E, dx))
        L.check(lib.snet_conv_fwd_fused(self.fplan, _p(x), _p(self.sh), _p(h2), _p(self.wr), _p(self.rp), _p(self.sr), N, SCALE, _p(o['out']), None))
        lists = (_p(self.tile_ptr), _p(self.tile_node), self.n_tiles.value, SCALE, _p(g_out))
        head = (self.fplan, _p(x), _p(self.sh))
        L.check(lib.snet_conv_bwd_fused(*head, _p(self.dsh), _p(h2), _p(self.wr), _p(self.rp), _p(self.sr), *lists, _p(o.get('g_xe')),
                                        _p(o['g_h2']), None, None, _p(o['g_vec']), _p(x_max), _p(g_max), None))
        if tail:
            o.update(tail_g_emb=zero(E, c['nb']), tail_g_vec=zero(E, 3))
            if gx:
                o['tail_g_xe'] = nan(E, dx)
            L.check(lib.snet_conv_bwd_fused(*head, _p(self.dsh), _p(h2), _p(self.wr), _p(self.rp), _p(self.sr), *lists, _p(o.get('tail_g_xe')),
                                            None, _p(self.emb_e), _p(o['tail_g_emb']), _p(o['tail_g_vec']), _p(x_max), _p(g_max), None))
        L.check(lib.snet_conv_bwd_fused_tangent(*head, _p(self.dsh), _p(h2), _p(h2d), _p(self.wr), _p(self.rp), _p(self.sr), *lists,
                                                _p(o.get('t_g_xe')), _p(self.vec), _p(o['t_g_vec']), _p(x_max), _p(g_max), None))
        # the radial scalar alone: a zero Jacobian leaves the spherical part at exactly 0, and along (2, 0, 0) the unit vector is exact
        L.check(lib.snet_conv_bwd_fused_tangent(*head, _p(self.dsh0), _p(h2), _p(h2d), _p(self.wr), _p(self.rp), _p(self.sr), *lists,
                                                None, _p(self.axis), _p(o['t_rad']), _p(x_max), _p(g_max), None))
        torch.cuda.synchronize()
        assert torch.equal(x_max, x.abs().amax(1)) and torch.equal(g_max, g_out.abs().amax(1))
        o = {k: v.cpu() for k, v in o.items()}
        for k in [k for k in o if k.endswith('g_xe')]:
            o[k] = o[k][:, self.col].contiguous()
        assert o['t_rad'][:, 1:].abs().max().item() == 0.0
        o['t_rad'] = o['t_rad'][:, 0].contiguous()
        return o

    def close(self):
        self.lib.snet_fused_plan_destroy(self.fplan)
        self.lib.snet_conv_plan_destroy(self.plan)
        self.lib.snet_radial_mlp_plan_destroy(self.mlp)


# output -> (reference key, which exponents its magnitude carries: p g_out row, q source row, r h2 row, d h2' row)
DEPENDS = {'out': ('out', 'qr'), 'g_xe': ('g_xe', 'pr'), 'g_h2': ('g_h2', 'pq'), 'g_vec': ('g_vec', 'pqr'),
           'tail_g_xe': ('g_xe', 'pr'), 'tail_g_emb': ('g_emb', 'pq'), 'tail_g_vec': ('g_vec', 'pqr'),
           't_g_xe': ('g_xe', 'pr'), 't_rad': ('g_rad', 'pqd')}


def _bounds(c, ex, S, e0, names):
    """the rule, once: output name -> bound array (per edge; per row for the forward output), and the exponent arrays behind it"""
    node, src, rows = fr.edge_maps(c)
    per_axis = dict(p=ex['p'][node], q=ex['q'][src], r=ex['r'][rows], d=ex['rd'][rows])
    tile, nt = fr.tile_of_edge(e0), e0.numel() - 1
    bound, expo = {}, {}
    for name in names:
        if name == 't_g_vec':   # spherical part + radial scalar along a unit vector: the two errors add (below)
            continue
        key, axes = DEPENDS[name]
        own = sum(per_axis[a] for a in axes)
        k = fr.row_exponent(own, node, c['N']) if name == 'out' else fr.bound_exponent(own, tile, nt)
        expo[name] = (own, k)
        bound[name] = fr.TOL * S[key] * 2.0 ** k.double()
    if 't_g_vec' in names:
        bound['t_g_vec'] = bound['g_vec'] + bound['t_rad']
        expo['t_g_vec'] = expo['g_vec']
    return bound, expo


def _worst(name, got, want, bound, expo, c, ex, e0, nodes):
    """worst error as a multiple of its bound, and a message that names the edge, its tile, the tile's rows and their exponents"""
    err = (got.double() - want).abs().reshape(got.shape[0], -1).amax(1)
    ratio = err / bound
    i = int(ratio.argmax())
    if name == 'out':
        return float(ratio[i]), f'{name}: row {i} (largest edge exponent {int(expo[name][1][i])}): error {float(err[i]):.3e} = {float(ratio[i]):.3g} x bound'
    t = int(fr.tile_of_edge(e0)[i])
    a, b = int(nodes[t, 0]), int(nodes[t, 1])
    own, k = expo[name]
    return float(ratio[i]), (f'{name}: edge {i} (own exponent {int(own[i])}, bound exponent {int(k[i])}) in tile {t} = edges [{int(e0[t])}, {int(e0[t + 1])}) of '
                             f'rows {a}, {b} (g_out exponents {int(ex["p"][a])}, {int(ex["p"][b])}): error {float(err[i]):.3e} = {float(ratio[i]):.3g} x bound')


@pytest.mark.parametrize('axes', ['p', 'q', 'r', 'pqr', 'zero'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_fused_kernels_mixed_magnitudes(shape, axes):
    """finite outputs, per-tile accuracy against fp64, and (axes = 'p') exact power-of-two covariance with the unit-scale run.
    The 'zero' case has an all-zero g_out row of 70 edges (tiles whose bound is 0: the kg <= 60 clamp) and an all-zero source row.
    With radial-row factors (axes with 'r') the hidden-layer tail is left out: it recomputes h2 from the embedding."""
    c, ref1 = _case(shape)
    gx, tail = SHAPES[shape][1] != 0, 'r' not in axes
    ex = fr.axis_exponents(c, '' if axes == 'zero' else axes)
    fg, fx, fh, fhd = (2.0 ** ex[k].double() for k in ('p', 'q', 'r', 'rd'))
    if axes == 'zero':
        fg[ZERO_NODE], fx[ZERO_SRC] = 0.0, 0.0
    ref = fr.scaled_reference(ref1, c, fg, fx, fh, fhd)
    S = {k: ref1[k].abs().max().item() for k in ('out', 'g_xe', 'g_h2', 'g_vec', 'g_rad')}
    node, src, rows = fr.edge_maps(c)
    unit = c['vec'].double() / c['vec'].double().norm(dim=1, keepdim=True)
    if tail:
        ref['g_emb'] = fr.hidden_backward(c['emb'] if c['w_row'] is None else c['emb'][rows], c['W0'], c['W1'], ref['g_h2'])
        S['g_emb'] = fr.hidden_backward(c['emb'] if c['w_row'] is None else c['emb'][rows], c['W0'], c['W1'], ref1['g_h2']).abs().max().item()
    ref['t_g_vec'] = ref['g_vec'] + ref['g_rad'][:, None] * unit
    K = _Kernels(c)
    try:
        e0, nodes = K.tiles()
        cls, gap = fr.tile_classes(nodes, fr.axis_exponents(c, 'p')['p'])
        if K.mode == 1:   # the packed list really has all three tile classes and every gap (else the checks below would be vacuous)
            assert min(int((cls == k).sum()) for k in range(3)) > 0 and set(gap[cls == 2].tolist()) == {12, 20, 32}
        else:
            assert bool((cls == 0).all())
        f32 = lambda t, f: (t * f.float()[:, None]).contiguous()  # noqa: E731
        got = K.run(f32(c['x'], fx), f32(c['h2'], fh), f32(c['h2d'], fhd), f32(c['g_out'], fg), gx, tail)
        names = [n for n in got]
        # (a) finiteness
        for n in names:
            assert bool(torch.isfinite(got[n]).all()), (n, 'not finite')
        if axes == 'zero':
            dead = (node == ZERO_NODE)
            for n in names:
                if n != 'out' and 'p' in (DEPENDS[n][1] if n in DEPENDS else 'p'):
                    assert got[n][dead].abs().max().item() == 0.0, n
            assert got['out'][ZERO_NODE].abs().max().item() > 0.0
        # (b) accuracy per tile
        bound, expo = _bounds(c, ex, S, e0, names)
        lines, bad = [], []
        for n in names:
            key = 't_g_vec' if n == 't_g_vec' else DEPENDS[n][0]
            r, msg = _worst(n, got[n], ref[key], bound[n].reshape(-1), expo, c, ex, e0, nodes)
            lines.append(f'{shape} {axes} {msg}')
            if not r <= 1.0:
                bad.append(msg)
        print('\n'.join(lines))
        assert not bad, bad
        # (d) the radial scalar dE/d|r| of the tangent kernel against the one the tail kernel's g_emb gives (g_emb . emb', contracted
        # here in fp64), each against the fp64 value of what it was given: new error <= 1.5 x old error, per tile class
        if tail:
            de = c['demb'].double()[rows]
            old = ((got['tail_g_emb'].double() * de).sum(1) - (ref['g_emb'] * de).sum(1)).abs()
            new = (got['t_rad'].double() - ref['g_rad']).abs()
            ecls = cls[fr.tile_of_edge(e0)]
            for k, cname in enumerate(('single-row tiles', 'two-row tiles, same p', 'two-row tiles, different p')):
                if bool((ecls == k).any()):
                    o_, n_ = old[ecls == k].max().item(), new[ecls == k].max().item()
                    print(f'{shape} {axes} radial scalar, {cname}: tail {o_:.3e}, tangent {n_:.3e}')
                    assert n_ <= 1.5 * o_, (cname, n_, o_)
        # the tail and tangent instantiations agree with the g_h2 one on what they share (last-bit differences between two
        # instantiations of one source are allowed, as in test_conv_fused_matches_separate_kernels)
        if tail:
            assert torch.equal(got['tail_g_vec'], got['g_vec'])
            if gx:
                assert torch.equal(got['tail_g_xe'], got['g_xe'])
        # (c) covariance: g_out[n] * 2^p[n] multiplies the results by exactly 2^p -- everywhere for the fp32 bodies on parked
        # g_out 2^kg (g_xe, spherical g_vec), and wherever the tile's fp16 operand g_w carries ONE factor (single-row tiles, two-row
        # tiles whose rows share p) for g_h2, the tail's g_emb and the tangent kernel's radial scalar.  Same kernel, same binary.
        if axes == 'p':
            one = K.run(c['x'], c['h2'], c['h2d'], c['g_out'], gx, tail)
            f = fg[node].float()
            uniform = (cls != 2)[fr.tile_of_edge(e0)]
            assert bool(uniform.any()) and (K.mode == 0 or bool((~uniform).any()))
            assert torch.equal(got['out'], one['out'])
            held = []
            for n in names:
                if n == 'out':
                    continue
                sel = torch.ones_like(uniform) if n in ('g_xe', 'g_vec', 'tail_g_xe', 'tail_g_vec', 't_g_xe') else uniform
                a, b = got[n][sel], (one[n] * (f if one[n].dim() == 1 else f[:, None]))[sel]
                ok = torch.equal(a, b)
                held.append(ok)
                ndiff = int((a != b).reshape(a.shape[0], -1).any(1).sum())
                print(f'{shape} covariance {n}: {"exact" if ok else f"{ndiff} of {a.shape[0]} edges differ"} on {int(sel.sum())} edges')
            assert all(held), [n for n, ok in zip([n for n in names if n != 'out'], held) if not ok]
    finally:
        K.close()
