"""GPU: the merged-store instantiation of the tangent-mode reverse kernel (snet_conv_bwd_fused_tangent_merged over
snet_gxe_merge_map) against today's kernel (snet_conv_bwd_fused_tangent) and the fp64 restatement
(fused_range.fused_reference), on the 64-atom diamond cell of smoke() -- neighbouring centres share sources there -- at the two
16-channel last-layer shapes (lmax 1 and 2: per-row tiles, one sub-step per block) and at the SevenNet-0 middle-layer shape (packed
tiles), with unit and mixed-magnitude inputs; and the whole model, both hosts, with the switch on and off."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fused_range as fr
import gxe_merge as gm
from test_ops_gpu import _lib, _p

pytestmark = pytest.mark.gpu
SCALE = 0.25
DEV = 'cuda:0'
CUT_ROW = 40   # rows [0, 40) / [40, 64): the two sub-lists of the split launches


def _spec(shape):
    from sevennet_amd.model_spec import build_model_spec, sevennet_0_config
    from sevennet_amd.shapes import lastlayer_test_configs
    if shape.startswith('7net0_mid'):
        return build_model_spec(sevennet_0_config()).layers[1].conv
    return build_model_spec(lastlayer_test_configs()[{'l1': 'last16_l1', 'l2': 'last16_l2'}[shape]]).layers[-1].conv


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs on the 64-atom cell (drawn as test_ops_gpu._fused_case draws them) and their unit-scale fp64 reference, computed once
    and shared, never modified"""
    spec = _spec(shape)
    rp, src, vec = gm.diamond_graph((2, 2, 2), seed=0)
    N, E = len(rp) - 1, len(src)
    nb, wn, dx, dout, nsh = 8, spec.weight_numel, spec.irreps_x.dim, spec.irreps_out.dim, spec.irreps_sh.dim
    g = torch.Generator().manual_seed(11)
    R, w_row = E, None
    if shape.endswith('_pairs'):   # several edges share one radial row, in scrambled order (as _fused_case's `pairs`)
        R = E // 2 + 3
        w_row = torch.randint(0, R, (E,), generator=g).to(torch.int32)
    c = dict(spec=spec, nb=nb, wn=wn, dx=dx, dout=dout, nsh=nsh, N=N, NT=N, E=E, R=R, w_row=w_row,
             row_ptr=torch.from_numpy(rp), src=torch.from_numpy(src), vec=torch.from_numpy(vec),
             x=torch.randn(N, dx, generator=g), sh=torch.randn(E, nsh, generator=g), dsh=torch.randn(E, nsh * 3, generator=g),
             emb=torch.randn(R, nb, generator=g), demb=torch.randn(R, nb, generator=g), g_out=torch.randn(N, dout, generator=g),
             W0=(torch.randn(nb, 64, generator=g) / nb ** 0.5).contiguous(), W1=(torch.randn(64, 64, generator=g) / 8).contiguous(),
             W2=(torch.randn(64, wn, generator=g) / 8).contiguous())
    h2, h2d = fr.hidden_layers(c['emb'], c['demb'], c['W0'], c['W1'])
    c['h2'], c['h2d'] = h2.float().contiguous(), h2d.float().contiguous()
    ref = fr.fused_reference(spec, c['x'], c['sh'], c['dsh'], c['h2'], c['W2'], c['w_row'], c['row_ptr'], c['src'], SCALE, c['g_out'], c['h2d'])
    return c, ref


class _Kernels:
    """plans of one shape at terms = 4 (the engine default), the tile list in the plan's format -- whole and cut at CUT_ROW -- and the
    merge maps of both"""

    def __init__(self, c):
        self.L, self.lib = L, lib = _lib()
        self.c = c
        fp = lambda t: t.numpy().ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        self.mlp, self.plan, self.fplan = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(lib.snet_radial_mlp_plan_create(c['nb'], 64, 64, c['wn'], fp(c['W0']), fp(c['W1']), fp(c['W2']), 0, fr.CST, 1, C.byref(self.mlp)))
        L.check(lib.snet_conv_plan_create(c['spec'].tag.encode(), C.byref(self.plan)))
        L.check(lib.snet_fused_plan_create(self.plan, self.mlp, 4, C.byref(self.fplan)))
        self.mode = lib.snet_fused_plan_tile_mode(self.fplan)
        self.window = lib.snet_fused_plan_merge_window(self.fplan)
        assert self.window in (2, 4, 8), 'this shape has no merged-store kernel'
        N, E = c['N'], c['E']
        self.rp, self.sr = c['row_ptr'].to(DEV), c['src'].to(DEV)
        self.sh, self.dsh, self.vec = c['sh'].to(DEV), c['dsh'].to(DEV), c['vec'].to(DEV)
        self.wr = None if c['w_row'] is None else c['w_row'].to(DEV)
        order = torch.sort(c['src'].long(), stable=True).indices
        self.eperm = order.to(torch.int32).to(DEV)
        col = torch.zeros(N + 1, dtype=torch.int32)
        col[1:] = torch.cumsum(torch.bincount(c['src'].long(), minlength=N), 0)
        self.col_ptr = col.to(DEV)
        nch = c['dx'] // 16
        cp = (C.c_int32 * nch)()
        L.check(lib.snet_fused_plan_gxe_chunks(self.fplan, cp, nch))
        self.chunks = torch.tensor(list(cp), dtype=torch.int32, device=DEV)
        # tile lists: [whole], [cut at CUT_ROW] -> (tile_ptr, tile_node, n_tiles, k, launches [(tp, tn, n)])
        self.lists = [self._tiles(0), self._tiles(CUT_ROW)]
        self.maps = [self._map(*lst[:4]) for lst in self.lists]

    def _tiles(self, cut):
        L, lib, c = self.L, self.lib, self.c
        N, E = c['N'], c['E']
        n = C.c_int64()
        if self.mode == 1:
            cap = N + E // 16 + 2
            tp = torch.full((cap + 1,), -1, dtype=torch.int32, device=DEV)
            tn = torch.full((2 * cap,), -1, dtype=torch.int32, device=DEV)
            k = 0
            if cut:
                L.check(lib.snet_edge_tiles_packed(_p(self.rp), 0, cut, _p(tp), _p(tn), cap, C.byref(n), None))
                k = n.value
            L.check(lib.snet_edge_tiles_packed(_p(self.rp), cut, N, C.c_void_p(tp.data_ptr() + 4 * k), C.c_void_p(tn.data_ptr() + 8 * k), cap - k,
                                               C.byref(n), None))
            nt = k + n.value
            parts = [(tp, tn, nt)] if not cut else [(tp, tn, k), (tp[k:], tn[2 * k:], nt - k)]
            return tp, tn, nt, k, parts
        tp = torch.empty(N + 1, dtype=torch.int32, device=DEV)
        cap = N + E // 16 + 1
        tn = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
        L.check(lib.snet_edge_tiles(_p(self.rp), N, _p(tp), _p(tn), cap, C.byref(n), None))
        nt = n.value
        k = int(tp[cut].item()) if cut else 0
        parts = [(tp, tn, nt)] if not cut else [(tp, tn, k), ((tp - k).contiguous(), tn[k:], nt - k)]   # (as Graph.tiles_split re-bases them)
        return tp, tn, nt, k, parts

    def _map(self, tp, tn, nt, k):
        """the device builder, checked against the host builder on the same lists (tests/test_gxe_merge_cpu.py pins that one)"""
        L, lib, c = self.L, self.lib, self.c
        N, E = c['N'], c['E']
        mr, mn, pm = (torch.full((E,), -9, dtype=torch.int32, device=DEV) for _ in range(3))
        sp = torch.full((N + 1,), -9, dtype=torch.int32, device=DEV)
        n = C.c_int64()
        L.check(lib.snet_gxe_merge_map(_p(self.rp), _p(self.sr), _p(tp), _p(tn), nt, k, self.mode, self.window, N, N, E, _p(mr), _p(mn), _p(sp),
                                       _p(pm), C.byref(n), None))
        want = gm.native_map(lib, self.mode, c['row_ptr'].numpy(), c['src'].numpy(), tp.cpu().numpy(), tn.cpu().numpy(), nt, k, self.window, N)
        assert n.value == want['n_rows'] < E
        for got, key in ((mr, 'row'), (mn, 'next'), (sp, 'seg'), (pm[:n.value], 'perm')):
            np.testing.assert_array_equal(got.cpu().numpy(), want[key], err_msg=key)
        return mr, mn, sp, pm, n.value

    def run(self, x, h2, h2d, g_out, which, merged):
        """(g_xe rows as written, g_x[N, dx] after the segment sum, g_vec[E, 3]) of one pass over tile list `which` (0 whole, 1 split)"""
        L, lib, c = self.L, self.lib, self.c
        N, E, dx = c['N'], c['E'], c['dx']
        x_max, g_max = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
        L.check(lib.snet_row_absmax(_p(x), N, dx, _p(x_max), None))
        L.check(lib.snet_row_absmax(_p(g_out), N, c['dout'], _p(g_max), None))
        mr, mn, sp, pm, n_rows = self.maps[which]
        g_xe = torch.full((n_rows if merged else E, dx), float('nan'), device=DEV)
        g_vec, g_x = torch.zeros(E, 3, device=DEV), torch.full((N, dx), float('nan'), device=DEV)
        for tp, tn, nt in self.lists[which][4]:
            head = (self.fplan, _p(x), _p(self.sh), _p(self.dsh), _p(h2), _p(h2d), _p(self.wr), _p(self.rp), _p(self.sr), _p(tp), _p(tn), nt, SCALE,
                    _p(g_out), _p(g_xe))
            tail = (_p(self.vec), _p(g_vec), _p(x_max), _p(g_max), None)
            if merged:
                L.check(lib.snet_conv_bwd_fused_tangent_merged(*head, _p(mr), _p(mn), *tail))
            else:
                L.check(lib.snet_conv_bwd_fused_tangent(*head, *tail))
        L.check(lib.snet_segment_sum_rows_chunked(_p(g_xe), _p(sp if merged else self.col_ptr), _p(pm if merged else self.eperm), N, dx,
                                                  _p(self.chunks), _p(g_x), None))
        torch.cuda.synchronize()
        return g_xe.cpu(), g_x.cpu(), g_vec.cpu()

    def close(self):
        self.lib.snet_fused_plan_destroy(self.fplan)
        self.lib.snet_conv_plan_destroy(self.plan)
        self.lib.snet_radial_mlp_plan_destroy(self.mlp)


@pytest.mark.parametrize('inputs', ['unit', 'mixed'])
@pytest.mark.parametrize('shape', ['l1', 'l2', '7net0_mid', '7net0_mid_pairs'])
def test_merged_kernel_against_todays_and_fp64(shape, inputs):
    """g_vec bit-identical to today's kernel; g_x after the segment sum against fp64: merged error <= 1.5 x today's error on the same
    inputs (the project's bar; both printed); two launches give the same bits; the launches over [a, b) then [b, c) give today's
    g_vec bits for the split step and hold the same error bar."""
    c, ref1 = _case(shape)
    ex = fr.axis_exponents(c, 'pqr' if inputs == 'mixed' else '')
    fg, fx, fh, fhd = (2.0 ** ex[k].double() for k in ('p', 'q', 'r', 'rd'))
    ref = fr.scaled_reference(ref1, c, fg, fx, fh, fhd)
    gx_ref = torch.zeros(c['N'], c['dx'], dtype=torch.float64).index_add_(0, c['src'].long(), ref['g_xe'])
    f32 = lambda t, f: (t * f.float()[:, None]).contiguous().to(DEV)  # noqa: E731
    args = (f32(c['x'], fx), f32(c['h2'], fh), f32(c['h2d'], fhd), f32(c['g_out'], fg))
    K = _Kernels(c)
    try:
        assert K.mode == (1 if shape.startswith('7net0_mid') else 0)
        for which, name in ((0, 'one launch'), (1, f'launches [0, k) + [k, n), rows cut at {CUT_ROW}')):
            n_rows = K.maps[which][4]
            _, gx_t, gv_t = K.run(*args, which, merged=False)
            xe_m, gx_m, gv_m = K.run(*args, which, merged=True)
            xe_2, gx_2, gv_2 = K.run(*args, which, merged=True)
            assert bool(torch.isfinite(xe_m).all()) and bool(torch.isfinite(gx_m).all())
            assert torch.equal(gv_m, gv_t), 'g_vec differs from the tangent-mode kernel'
            assert torch.equal(xe_m, xe_2) and torch.equal(gx_m, gx_2) and torch.equal(gv_m, gv_2), 'two launches differ'
            err_t = (gx_t.double() - gx_ref).abs().max().item()
            err_m = (gx_m.double() - gx_ref).abs().max().item()
            print(f'{shape} {inputs} {name}: {n_rows} merged rows of {c["E"]} edges (window {K.window}); max|g_x - fp64| today '
                  f'{err_t:.3e}, merged {err_m:.3e} (max|g_x| {gx_ref.abs().max().item():.3e})')
            assert err_m <= 1.5 * err_t, (err_m, err_t)
    finally:
        K.close()


@functools.lru_cache(maxsize=None)
def _model_case():
    from oracle.model import OracleModel
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.neighbor import diamond_cubic, neighbor_list
    from sevennet_amd.synthetic import random_state_dict
    cfg = sevennet_0_config()
    sd = random_state_dict(cfg, seed=0)
    pos, cell = diamond_cubic(5.431, (2, 2, 2), 0.05, 0)
    ei, ev, _ = neighbor_list(pos, cell, [True] * 3, cfg['cutoff'])
    types = np.zeros(len(pos), np.int64)
    ref = OracleModel(cfg, sd, dtype=torch.float64).forward(types, ei, ev)
    return cfg, sd, types, ei, ev, ref['forces'].numpy()


def test_whole_model_both_hosts():
    """smoke()'s cell: the Python host and the native host bit-identical with the switch on; energy and atomic energies bit-identical
    to the switch-off path (the forward pass does not change); max|dF| against fp64 printed beside the switch-off figure"""
    from sevennet_amd.engine import HipForceEngine, build_graph
    from sevennet_amd.native_model import NativeModel
    cfg, sd, types, ei, ev, f_ref = _model_case()
    g = build_graph(types, ei, ev, device=DEV)
    eng = HipForceEngine(cfg, sd, device=DEV)
    assert [L.merge_window for L in eng.layers] == [0, 4, 4, 4, 0]
    assert all(eng._gxe_merge(L, g) is not None for L in eng.layers[1:4]), 'the cell does not take the merged path'
    on = eng.compute(g)
    nat = NativeModel(cfg, sd, device=DEV).compute(g)
    off = HipForceEngine(cfg, sd, device=DEV, merge_gxe=False).compute(build_graph(types, ei, ev, device=DEV))
    nat_off = NativeModel(cfg, sd, device=DEV, merge_gxe=False).compute(g)
    torch.cuda.synchronize()
    for k in ('energy', 'atomic_energy', 'forces', 'dE_dr', 'virial'):
        assert torch.equal(on[k], nat[k]), f'{k}: the two hosts differ with the switch on'
        assert torch.equal(off[k], nat_off[k]), f'{k}: the two hosts differ with the switch off'
    assert torch.equal(on['energy'], off['energy']) and torch.equal(on['atomic_energy'], off['atomic_energy'])
    assert not torch.equal(on['forces'], off['forces'])   # (the switch does something: the source-row sums are taken in another order)
    d_on = float(np.abs(on['forces'].cpu().numpy() - f_ref).max())
    d_off = float(np.abs(off['forces'].cpu().numpy() - f_ref).max())
    print(f'whole model, 64 atoms: max|dF| vs fp64 merged {d_on:.3e}, one row per edge {d_off:.3e} eV/A (max|F| {np.abs(f_ref).max():.3e})')
