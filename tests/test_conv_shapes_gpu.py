"""GPU: EVERY tensor-product kernel the build ships against the fp64 tensor product, at the kernel's own interface.

One parameter per ConvSpec.tag of sevennet_amd.shapes.aot_conv_specs() -- computed from the catalogue, so a shape added to it is
swept without anyone adding it here (tests/test_conv_shapes_cpu.py pins that).  The case (tests/conv_shapes.shape_case): destination
degrees 0, 1, 2, 15, 16, 17, 33, 65, 0 (149 edges), 3 ghost source rows, with and without a scrambled pair map of the radial rows.
The reference (tests/conv_shapes.conv_reference) is the oracle's tensor product + autograd in fp64; it handles the pruned shape
(MF-ompa layer 3: 34 of 68 paths, output columns no path writes), which the helpers before it did not.

Bars (the project's own): separate fp32 kernels 3e-5 x max(1, largest reference entry) (test_conv_plugin_vs_oracle_autograd); fused
kernels at terms 4 and 3 fused_range.TOL = 2e-5 x max(floor, largest reference entry), floor 1 = the scale of g_out
(test_conv_fused_matches_separate_kernels).  Every shape holds these plain bars, the ones that had never been held to them
included (worst: 0.09 x bar, g_h2 of MF-ompa layer 3 at terms 3); no shape needed the fp32-class rule (error <= 1.5 x the error of
the reference evaluated in fp32 torch), so it is not implemented here.  The worst measured errors are in profiles/conv_shape_errors.txt (the lines this module prints)."""
import ctypes as C

import pytest
import torch

import conv_shapes as cs
import fused_range as fr
from test_ops_gpu import _lib, _p, _work_list

pytestmark = pytest.mark.gpu

_CAT = cs.catalogue()
TAGS = list(_CAT)
FUSABLE = [t for t in TAGS if cs.fusable(_CAT[t])]
PRUNED = [t for t in TAGS if cs.unwritten_ranges(_CAT[t])]     # shapes with output columns that no path writes


def _transposed():
    """last-layer tag -> tag of its transposed product, for the shapes whose transposed product the build ships"""
    from sevennet_amd.model_spec import transposed_scalar_conv
    out = {}
    for t, spec in _CAT.items():
        tr = transposed_scalar_conv(spec)
        if tr is not None and cs.fusable(spec) and tr[0].tag in _CAT:
            out[t] = tr[0].tag
    return out


TRANSPOSED = _transposed()
DEV = 'cuda:0'


class _Report:
    """collects error / bar of every output of one parameter, prints one line per kernel run, asserts once at the end"""

    def __init__(self, tag):
        self.tag, self.bad, self.line = tag, [], []

    def check(self, name, got, ref, tol, mask=None):
        ok, ratio = cs.judge(got.cpu(), ref, tol, 1.0, mask)
        self.line.append(f'{name} {ratio:.3f}')
        if not ok:
            self.bad.append((self.where, name, ratio))

    def exact(self, name, a, b):
        ok = torch.equal(a, b)
        self.line.append(f'{name} {"bit-equal" if ok else "DIFFERS"}')
        if not ok:
            self.bad.append((self.where, name, 'not bit-equal'))

    def begin(self, where):
        self.where, self.line = where, []

    def end(self):
        print(f'conv_shape {self.tag} {self.where}: ' + ', '.join(self.line))


def _dev(c):
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items() if k != 'spec'}
    node = torch.repeat_interleave(torch.arange(c['N']), (c['row_ptr'][1:] - c['row_ptr'][:-1]).long())
    order = torch.argsort(c['src'].long(), stable=True)
    col_ptr = torch.zeros(c['NT'] + 1, dtype=torch.int32)
    col_ptr[1:] = torch.cumsum(torch.bincount(c['src'].long(), minlength=c['NT']), 0).to(torch.int32)
    d.update(dst=node.to(torch.int32).to(DEV), eperm=order.to(torch.int32).to(DEV), col_ptr=col_ptr.to(DEV))
    return d


def _nan(*s):
    return torch.full(s, float('nan'), device=DEV)


def _junk(c, d):
    """g_out with finite junk (+-1e3) in the columns that no path writes"""
    g = d['g_out'].clone()
    dead = (~c['written']).to(DEV)
    sign = torch.where(torch.arange(c['dout'], device=DEV) % 2 == 0, 1e3, -1e3)
    g[:, dead] = sign[dead]
    return g


def _separate(L, lib, plan, c, d, g_out):
    """one run of the five separate entry points; overwritten outputs start as NaN, accumulated ones (g_sh, g_vec) at 0.5"""
    N, NT, E, dx, dout, nsh, wn = (c[k] for k in ('N', 'NT', 'E', 'dx', 'dout', 'nsh', 'wn'))
    o = dict(out=_nan(N, dout), g_w=_nan(E, wn), g_xe=_nan(E, dx), g_sh=torch.full((E, nsh), 0.5, device=DEV),
             v_g_w=_nan(E, wn), v_g_xe=_nan(E, dx), g_vec=torch.full((E, 3), 0.5, device=DEV), g_x=_nan(NT, dx), s_g_x=_nan(NT, dx))
    x, sh, dsh, w, wr, rp, sr = (d[k] for k in ('x', 'sh', 'dsh', 'w', 'w_row', 'row_ptr', 'src'))
    L.check(lib.snet_conv_fwd(plan, _p(x), _p(sh), _p(w), _p(wr), _p(rp), _p(sr), N, cs.SCALE, _p(o['out']), None))
    L.check(lib.snet_conv_bwd_edge(plan, _p(x), _p(sh), _p(w), _p(wr), _p(rp), _p(sr), N, cs.SCALE, _p(g_out), _p(o['g_w']), _p(o['g_xe']),
                                   _p(o['g_sh']), None))
    L.check(lib.snet_conv_bwd_edge_vec(plan, _p(x), _p(sh), _p(dsh), _p(w), _p(wr), _p(rp), _p(sr), N, cs.SCALE, _p(g_out), _p(o['v_g_w']),
                                       _p(o['v_g_xe']), _p(o['g_vec']), None))
    L.check(lib.snet_conv_bwd_node(plan, _p(sh), _p(w), _p(wr), _p(d['col_ptr']), _p(d['eperm']), _p(d['dst']), NT, cs.SCALE, _p(g_out),
                                   _p(o['g_x']), None))
    L.check(lib.snet_segment_sum_rows(_p(o['g_xe']), _p(d['col_ptr']), _p(d['eperm']), NT, dx, _p(o['s_g_x']), None))
    torch.cuda.synchronize()
    o['g_sh'] -= 0.5
    o['g_vec'] -= 0.5
    return o


@pytest.mark.parametrize('tag', TAGS)
def test_separate_kernels_vs_fp64(tag):
    """snet_conv_fwd, snet_conv_bwd_edge, snet_conv_bwd_edge_vec, snet_conv_bwd_node and snet_segment_sum_rows of one shape, with
    and without pair-shared weight rows.  Nothing is asserted about the columns of `out` that no path writes (the engine zeroes
    them itself); on a shape that has such columns, junk in g_out there must not change one bit of any gradient."""
    L, lib = _lib()
    spec = _CAT[tag]
    plan = C.c_void_p()
    L.check(lib.snet_conv_plan_create(tag.encode(), C.byref(plan)))
    dims = [C.c_int32() for _ in range(4)]
    L.check(lib.snet_conv_plan_dims(plan, *[C.byref(v) for v in dims]))
    assert [v.value for v in dims] == [spec.irreps_x.dim, spec.irreps_out.dim, spec.irreps_sh.dim, spec.weight_numel]
    assert (lib.snet_conv_fused_available(plan) != 0) == (tag in FUSABLE)
    rep = _Report(tag)
    try:
        for pairs in (False, True):
            c, ref, _ = cs.tag_case(tag, pairs)
            d = _dev(c)
            o = _separate(L, lib, plan, c, d, d['g_out'])
            rep.begin('separate' + (' w_row' if pairs else ''))
            rep.check('out', o['out'], ref['out'], cs.TOL_SEPARATE, c['written'])
            for name, key in (('g_w', 'g_w'), ('g_xe', 'g_xe'), ('g_sh', 'g_sh'), ('vec.g_w', 'g_w'), ('vec.g_xe', 'g_xe'), ('g_vec', 'g_vec'),
                              ('node.g_x', 'g_x'), ('segsum.g_x', 'g_x')):
                got = o[{'vec.g_w': 'v_g_w', 'vec.g_xe': 'v_g_xe', 'node.g_x': 'g_x', 'segsum.g_x': 's_g_x'}.get(name, name)]
                rep.check(name, got, ref[key], cs.TOL_SEPARATE)
            rep.end()
            if tag in PRUNED:
                o2 = _separate(L, lib, plan, c, d, _junk(c, d))
                rep.begin('separate' + (' w_row' if pairs else '') + ', junk in the unwritten g_out columns')
                for k in ('g_w', 'g_xe', 'g_sh', 'v_g_w', 'v_g_xe', 'g_vec', 'g_x', 's_g_x'):
                    rep.exact(k, o2[k], o[k])
                rep.end()
    finally:
        lib.snet_conv_plan_destroy(plan)
    assert not rep.bad, rep.bad


class _Fused:
    """radial plan (nb = 8, silu, mode 1) and fused plan of one shape at one precision mode"""

    def __init__(self, L, lib, tag, c, W2, terms):
        self.L, self.lib = L, lib
        fp = lambda t: t.numpy().ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        self.mlp, self.plan, self.fplan = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(lib.snet_radial_mlp_plan_create(c['nb'], 64, 64, W2.shape[1], fp(c['W0']), fp(c['W1']), fp(W2), 0, cs.CST, 1, C.byref(self.mlp)))
        L.check(lib.snet_conv_plan_create(tag.encode(), C.byref(self.plan)))
        assert lib.snet_conv_fused_available(self.plan) != 0
        L.check(lib.snet_fused_plan_create(self.plan, self.mlp, terms, C.byref(self.fplan)))

    def close(self):
        self.lib.snet_fused_plan_destroy(self.fplan)
        self.lib.snet_conv_plan_destroy(self.plan)
        self.lib.snet_radial_mlp_plan_destroy(self.mlp)


def _fused_reverse(L, lib, K, c, d, g_out, g_max, x_max, lists, gx=True):
    """one run of every fused reverse entry point.  Overwritten outputs start as NaN, accumulated ones at 0.5."""
    N, E, dx, nsh, nb = c['N'], c['E'], c['dx'], c['nsh'], c['nb']
    half = lambda *s: torch.full(s, 0.5, device=DEV)  # noqa: E731
    o = dict(g_h2=_nan(E, 64), g_vec=half(E, 3), tail_g_emb=half(E, nb), tail_g_vec=half(E, 3), sh_g_sh=_nan(E, nsh), sh_g_h2=_nan(E, 64),
             t_g_vec=half(E, 3), t_rad=half(E, 3))
    if gx:
        o.update(g_xe=_nan(E, dx), tail_g_xe=_nan(E, dx), sh_g_xe=_nan(E, dx), t_g_xe=_nan(E, dx))
    x, sh, dsh, h2, h2d, wr, rp, sr = (d[k] for k in ('x', 'sh', 'dsh', 'h2', 'h2d', 'w_row', 'row_ptr', 'src'))
    tail = (*lists, cs.SCALE, _p(g_out))
    bounds = (_p(x_max), _p(g_max), None)
    L.check(lib.snet_conv_bwd_fused(K.fplan, _p(x), _p(sh), _p(dsh), _p(h2), _p(wr), _p(rp), _p(sr), *tail, _p(o.get('g_xe')), _p(o['g_h2']),
                                    None, None, _p(o['g_vec']), *bounds))
    L.check(lib.snet_conv_bwd_fused(K.fplan, _p(x), _p(sh), _p(dsh), _p(h2), _p(wr), _p(rp), _p(sr), *tail, _p(o.get('tail_g_xe')), None,
                                    _p(d['emb_e']), _p(o['tail_g_emb']), _p(o['tail_g_vec']), *bounds))
    L.check(lib.snet_conv_bwd_fused_sh(K.fplan, _p(x), _p(sh), _p(h2), _p(wr), _p(rp), _p(sr), *tail, _p(o.get('sh_g_xe')), _p(o['sh_g_h2']),
                                       None, None, _p(o['sh_g_sh']), *bounds))
    L.check(lib.snet_conv_bwd_fused_tangent(K.fplan, _p(x), _p(sh), _p(dsh), _p(h2), _p(h2d), _p(wr), _p(rp), _p(sr), *tail,
                                            _p(o.get('t_g_xe')), _p(d['vec']), _p(o['t_g_vec']), *bounds))
    # the radial scalar alone: a zero Jacobian leaves the spherical part at exactly 0; along (2, 0, 0) the unit vector is exact
    L.check(lib.snet_conv_bwd_fused_tangent(K.fplan, _p(x), _p(sh), _p(d['dsh0']), _p(h2), _p(h2d), _p(wr), _p(rp), _p(sr), *tail,
                                            None, _p(d['axis']), _p(o['t_rad']), *bounds))
    torch.cuda.synchronize()
    for k in ('g_vec', 'tail_g_emb', 'tail_g_vec', 't_g_vec', 't_rad'):
        o[k] -= 0.5
    return o


@pytest.mark.parametrize('tag', FUSABLE)
def test_fused_kernels_vs_fp64(tag):
    """snet_conv_fwd_fused, snet_conv_bwd_fused (g_h2 output and hidden-layer tail), snet_conv_bwd_fused_sh and
    snet_conv_bwd_fused_tangent of one shape at terms 4 and 3, with and without pair-shared radial rows, the chunk order of g_xe and
    snet_segment_sum_rows_chunked.  The same rules about unwritten output columns as for the separate kernels."""
    L, lib = _lib()
    spec = _CAT[tag]
    layer0 = all(l == 0 for _, l, _ in spec.irreps_x) and len(spec.irreps_x) == 1 and tag not in TRANSPOSED.values()
    rep = _Report(tag)
    for pairs in (False, True):
        c, _, ref = cs.tag_case(tag, pairs)
        d = _dev(c)
        N, NT, E, dx, dout = c['N'], c['NT'], c['E'], c['dx'], c['dout']
        rows = torch.arange(E) if c['w_row'] is None else c['w_row'].long()
        emb_e = c['emb'][rows].contiguous()
        d.update(emb_e=emb_e.to(DEV), dsh0=torch.zeros_like(d['dsh']), axis=torch.tensor([2.0, 0.0, 0.0]).repeat(E, 1).to(DEV))
        unit = c['vec'].double() / c['vec'].double().norm(dim=1, keepdim=True)
        want = dict(ref, g_emb=fr.hidden_backward(emb_e, c['W0'], c['W1'], ref['g_h2']), t_g_vec=ref['g_vec'] + ref['g_rad'][:, None] * unit)
        for terms in (4, 3):
            K = _Fused(L, lib, tag, c, c['W2'], terms)
            try:
                assert lib.snet_fused_plan_has_mlp_tail(K.fplan) == 1
                tile_ptr, tile_node, n_tiles = _work_list(L, lib, K.fplan, d['row_ptr'], c['row_ptr'], N, E, DEV)
                lists = (_p(tile_ptr), _p(tile_node), n_tiles.value)
                x_max, g_max = _nan(NT), _nan(N)
                L.check(lib.snet_row_absmax(_p(d['x']), NT, dx, _p(x_max), None))
                L.check(lib.snet_row_absmax(_p(d['g_out']), N, dout, _p(g_max), None))
                out = _nan(N, dout)
                L.check(lib.snet_conv_fwd_fused(K.fplan, _p(d['x']), _p(d['sh']), _p(d['h2']), _p(d['w_row']), _p(d['row_ptr']), _p(d['src']), N,
                                                cs.SCALE, _p(out), None))
                o = _fused_reverse(L, lib, K, c, d, d['g_out'], g_max, x_max, lists)
                assert torch.equal(x_max, d['x'].abs().amax(1)) and torch.equal(g_max, d['g_out'].abs().amax(1))
                # g_xe rows keep the kernel's own order of 16-channel chunks: undo it; the chunked segment sum must return the
                # standard-order sums bit for bit
                cp = (C.c_int32 * (dx // 16))()
                L.check(lib.snet_fused_plan_gxe_chunks(K.fplan, cp, dx // 16))
                cpos = torch.tensor(list(cp), dtype=torch.long)
                assert sorted(cpos.tolist()) == list(range(dx // 16))
                col = (cpos[:, None] * 16 + torch.arange(16)[None, :]).reshape(-1).to(DEV)
                raw = o['g_xe']
                for k in ('g_xe', 'tail_g_xe', 'sh_g_xe', 't_g_xe'):
                    o[k] = o[k][:, col].contiguous()
                s_std, s_chk = _nan(NT, dx), _nan(NT, dx)
                L.check(lib.snet_segment_sum_rows(_p(o['g_xe']), _p(d['col_ptr']), _p(d['eperm']), NT, dx, _p(s_std), None))
                L.check(lib.snet_segment_sum_rows_chunked(_p(raw), _p(d['col_ptr']), _p(d['eperm']), NT, dx,
                                                          _p(torch.tensor(list(cp), dtype=torch.int32, device=DEV)), _p(s_chk), None))
                torch.cuda.synchronize()
                rep.begin(f'fused terms {terms}' + (' w_row' if pairs else ''))
                rep.check('out', out, want['out'], cs.TOL_FUSED, c['written'])
                for name, key in (('g_xe', 'g_xe'), ('g_h2', 'g_h2'), ('g_vec', 'g_vec'), ('tail.g_emb', 'g_emb'), ('tail.g_xe', 'g_xe'),
                                  ('tail.g_vec', 'g_vec'), ('sh.g_sh', 'g_sh'), ('sh.g_xe', 'g_xe'), ('sh.g_h2', 'g_h2'),
                                  ('tangent.g_vec', 't_g_vec'), ('segsum.g_x', 'g_x')):
                    got = s_std if name == 'segsum.g_x' else o[name.replace('tangent.', 't_').replace('.', '_')]
                    rep.check(name, got, want[key], cs.TOL_FUSED)
                assert o['t_rad'][:, 1:].abs().max().item() == 0.0
                rep.check('tangent.g_rad', o['t_rad'][:, 0], want['g_rad'], cs.TOL_FUSED)
                rep.exact('tangent.g_xe == g_xe', o['t_g_xe'], o['g_xe'])
                rep.exact('chunked segment sum == standard', s_chk, s_std)
                rep.end()
                if layer0:   # first layer: the source rows depend on the species alone, g_xe = NULL
                    o0 = _fused_reverse(L, lib, K, c, d, d['g_out'], g_max, x_max, lists, gx=False)
                    rep.begin(f'fused terms {terms}' + (' w_row' if pairs else '') + ', g_xe = NULL')
                    for name, key in (('g_h2', 'g_h2'), ('g_vec', 'g_vec'), ('tail_g_emb', 'g_emb'), ('tail_g_vec', 'g_vec'), ('sh_g_sh', 'g_sh'),
                                      ('sh_g_h2', 'g_h2'), ('t_g_vec', 't_g_vec')):
                        rep.check(name, o0[name], want[key], cs.TOL_FUSED)
                    rep.end()
                if tag in PRUNED:   # same g_rowmax as before: junk in the unwritten columns must not reach one bit of any gradient
                    o2 = _fused_reverse(L, lib, K, c, d, _junk(c, d), g_max, x_max, lists)
                    rep.begin(f'fused terms {terms}' + (' w_row' if pairs else '') + ', junk in the unwritten g_out columns')
                    for k in ('g_xe', 'tail_g_xe', 'sh_g_xe', 't_g_xe'):
                        o2[k] = o2[k][:, col].contiguous()
                    for k in ('g_xe', 'g_h2', 'g_vec', 'tail_g_xe', 'tail_g_emb', 'tail_g_vec', 'sh_g_sh', 'sh_g_xe', 'sh_g_h2', 't_g_xe', 't_g_vec',
                              't_rad'):
                        rep.exact(k, o2[k], o[k])
                    rep.end()
            finally:
                K.close()
    assert not rep.bad, rep.bad


@pytest.mark.parametrize('tag', list(TRANSPOSED))
def test_transposed_plan_reproduces_the_source_row_gradient(tag):
    """the last layers' source-row gradient as a FORWARD convolution of the transposed shape snet_conv_plan_transposed names: edges
    grouped by source (snet_edges_by_source), W2 columns scaled by col_scale, sh rows gathered by eperm -> the parent shape's fp64
    g_x, at terms 4 and 3.  Nothing is asserted on the dead ranges it reports."""
    L, lib = _lib()
    spec = _CAT[tag]
    plan = C.c_void_p()
    L.check(lib.snet_conv_plan_create(tag.encode(), C.byref(plan)))
    name, col = C.create_string_buffer(13), torch.zeros(spec.weight_numel)
    dead, nd = (C.c_int32 * 32)(), C.c_int32()
    L.check(lib.snet_conv_plan_transposed(plan, name, C.c_void_p(col.data_ptr()), C.cast(dead, C.c_void_p), 32, C.byref(nd)))
    lib.snet_conv_plan_destroy(plan)
    assert name.value.decode() == TRANSPOSED[tag]
    live = torch.ones(spec.irreps_x.dim, dtype=torch.bool)
    for i in range(nd.value):
        live[dead[2 * i]:dead[2 * i] + dead[2 * i + 1]] = False
    rep = _Report(tag)
    for pairs in (False, True):
        c, _, ref = cs.tag_case(tag, pairs)
        d = _dev(c)
        N, NT, E = c['N'], c['NT'], c['E']
        center_t, w_row_t = torch.full((E,), -1, dtype=torch.int32, device=DEV), torch.full((E,), -1, dtype=torch.int32, device=DEV)
        L.check(lib.snet_edges_by_source(_p(d['row_ptr']), N, _p(d['eperm']), _p(d['w_row']), E, _p(center_t), _p(w_row_t), None))
        torch.cuda.synchronize()
        ep = d['eperm'].long()
        assert torch.equal(center_t, d['dst'][ep]) and torch.equal(w_row_t, d['eperm'] if c['w_row'] is None else d['w_row'][ep])
        sh_t = d['sh'][ep].contiguous()
        for terms in (4, 3):
            K = _Fused(L, lib, TRANSPOSED[tag], c, (c['W2'] * col[None, :]).contiguous(), terms)
            try:
                g_x = _nan(NT, c['dx'])
                L.check(lib.snet_conv_fwd_fused(K.fplan, _p(d['g_out']), _p(sh_t), _p(d['h2']), _p(w_row_t), _p(d['col_ptr']), _p(center_t), NT,
                                                cs.SCALE, _p(g_x), None))
                torch.cuda.synchronize()
                rep.begin(f'transposed {TRANSPOSED[tag]} terms {terms}' + (' w_row' if pairs else ''))
                rep.check('g_x', g_x, ref['g_x'], cs.TOL_FUSED, live)
                rep.end()
            finally:
                K.close()
    assert not rep.bad, rep.bad
