"""GPU: the radial gradient by forward tangent -- snet_edge_embed_tangent, snet_radial_mlp_hidden_fwd_layers_tangent and the tangent
mode of the fused reverse kernels (snet_conv_bwd_fused_tangent) -- against the fp64 restatement of tests/test_tangent_cpu.py and
against the reverse-mode path they replace (in-kernel hidden-layer tail -> g_emb -> snet_edge_embed_bwd)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from test_ops_gpu import _fused_case, _lib, _p, _work_list
from test_tangent_cpu import embedding_and_tangent, tangent_reference

pytestmark = pytest.mark.gpu
ACT_NAME = {0: 'silu', 1: 'tanh', 2: 'relu', 3: 'abs', 4: 'ssp', 5: 'sigmoid', 6: 'elu'}
RC, NB = 5.0, 8


def _edge_params(L, kind=0, lmax=2, nb=NB):
    P = L.EdgeParams(RC, nb, kind, 6, 4.2 if kind else 0.0, lmax, 1)
    coeffs = [(k + 1) * math.pi / RC for k in range(nb)]
    return P, (C.c_float * nb)(*coeffs), torch.tensor(coeffs, dtype=torch.float64)


def _vectors(n, seed):
    """n vectors with lengths over (0.7, cutoff), a few of them within 1e-2 .. 1e-4 of the cutoff"""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    r = torch.rand(n, generator=g, dtype=torch.float64) * (RC - 0.8) + 0.7
    r[:3] = torch.tensor([RC - 1e-2, RC - 1e-3, RC - 1e-4], dtype=torch.float64)[:min(3, n)]
    return (d / d.norm(dim=1, keepdim=True) * r[:, None]).float()


@pytest.mark.parametrize('nb,acts,E,kind', [(8, (0, 0, 0, 0, 0), 1000, 0), (8, (0, 1, 4), 333, 1), (6, (2, 3, 5, 6), 130, 0), (8, (0,), 5, 0)])
def test_hidden_layers_tangent_vs_fp64(nb, acts, E, kind):
    """h2 of the tangent launch == snet_radial_mlp_hidden_fwd_layers bit for bit; emb' and h2' against fp64, bounded the way
    test_ops_gpu.py bounds h2 itself (3e-6 of max(1, largest entry): fp32 rounding class of bf16 x6 products and hardware exp2 / rcp)."""
    from sevennet_amd.model_spec import ACT_CST
    L, lib = _lib()
    dev = 'cuda:0'
    rng = np.random.default_rng(nb * 100 + E)
    P, cf, coeffs = _edge_params(L, kind, 2, nb)
    vec = _vectors(E, E).to(dev)
    nsh = 9
    emb, sh = torch.empty(E, nb, device=dev), torch.empty(E, nsh, device=dev)
    demb = torch.full((E, nb), float('nan'), device=dev)
    L.check(lib.snet_edge_embed_fwd(C.byref(P), cf, _p(vec), E, _p(emb), _p(sh), None, None))
    L.check(lib.snet_edge_embed_tangent(C.byref(P), cf, _p(vec), None, E, _p(demb), None))
    r64 = vec.double().cpu().norm(dim=1)
    emb64, demb64 = embedding_and_tangent(r64, coeffs, RC, 'poly_cut' if kind == 0 else 'XPLOR', 6, 4.2)
    torch.cuda.synchronize()
    # the basis derivative: fp32 sin / cos of arguments up to 8 pi, |r| itself rounded to fp32 (the forward embedding's class)
    assert (emb.cpu().double() - emb64).abs().max() < 2e-6 * max(1.0, emb64.abs().max().item())
    err_d = (demb.cpu().double() - demb64).abs().max().item()
    print(f'emb\' vs fp64: {err_d:.3e} (largest entry {demb64.abs().max().item():.3g})')
    assert err_d < 2e-6 * max(1.0, demb64.abs().max().item())
    plans, Ws = [], []
    fp = lambda t: t.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    for a in acts:
        W0 = (rng.normal(0, 1, (nb, 64)) / np.sqrt(nb)).astype(np.float32)
        W1 = (rng.normal(0, 1, (64, 64)) / 8).astype(np.float32)
        W2 = (rng.normal(0, 1, (64, 32)) / 8).astype(np.float32)
        mlp = C.c_void_p()
        L.check(lib.snet_radial_mlp_plan_create(nb, 64, 64, 32, fp(W0), fp(W1), fp(W2), a, ACT_CST[ACT_NAME[a]], 1, C.byref(mlp)))
        plans.append(mlp)
        Ws.append((W0, W1))
    n = len(acts)
    plain = [torch.full((E, 64), float('nan'), device=dev) for _ in acts]
    h2 = [torch.full((E, 64), float('nan'), device=dev) for _ in acts]
    h2d = [torch.full((E, 64), float('nan'), device=dev) for _ in acts]
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    L.check(lib.snet_radial_mlp_hidden_fwd_layers((C.c_void_p * n)(*plans), n, _p(emb), E, ptrs(plain), None))
    L.check(lib.snet_radial_mlp_hidden_fwd_layers_tangent((C.c_void_p * n)(*plans), n, _p(emb), _p(demb), E, ptrs(h2), ptrs(h2d), None))
    torch.cuda.synchronize()
    e_in, d_in = emb.cpu().double(), demb.cpu().double()   # (the fp32 rows the launch read, as the h2 test does)
    for a, (W0, W1), o, v, d in zip(acts, Ws, plain, h2, h2d):
        assert torch.equal(o, v)
        ref, ref_d = tangent_reference(e_in, d_in, torch.from_numpy(W0).double(), torch.from_numpy(W1).double(), ACT_NAME[a])
        err, err_t = (v.cpu().double() - ref).abs().max().item(), (d.cpu().double() - ref_d).abs().max().item()
        print(f'act {ACT_NAME[a]}: h2 vs fp64 {err:.3e} (max {ref.abs().max().item():.3g}), h2\' vs fp64 {err_t:.3e} (max {ref_d.abs().max().item():.3g})')
        assert err < 3e-6 * max(1.0, ref.abs().max().item()), (a, err)
        assert err_t < 3e-6 * max(1.0, ref_d.abs().max().item()), (a, err_t)
    with pytest.raises(RuntimeError, match='1 .. 8 layers'):
        L.check(lib.snet_radial_mlp_hidden_fwd_layers_tangent((C.c_void_p * n)(*plans), 0, _p(emb), _p(demb), E, ptrs(h2), ptrs(h2d), None))
    # an edge-free graph hands over empty tensors (null data pointers): nothing is launched
    nul = (C.c_void_p * n)()
    L.check(lib.snet_radial_mlp_hidden_fwd_layers_tangent((C.c_void_p * n)(*plans), n, None, None, 0, nul, nul, None))
    L.check(lib.snet_edge_embed_tangent(C.byref(P), cf, None, None, 0, None, None))
    for p in plans:
        lib.snet_radial_mlp_plan_destroy(p)


@pytest.mark.parametrize('model,layer,pairs,gx', [('sevennet_0', 1, True, True), ('sevennet_0', 0, False, False),
                                                  ('sevennet_l3i5', 1, True, True), ('sevennet_0', 4, False, False)])
def test_tangent_kernel_vs_tail_kernel(model, layer, pairs, gx):
    """g_vec of snet_conv_bwd_fused_tangent against g_vec of the tail-mode kernel + snet_edge_embed_bwd, engine default precision
    (fp16 terms).  Both are measured against fp64: the spherical part and g_w of the separate fp32 kernels (snet_conv_bwd_edge_vec,
    as test_conv_fused_matches_separate_kernels takes its fp64 references) with the radial scalar dE/d|r| = sum_k g_w w' contracted in
    fp64 from the fp64 tangent of the radial MLP.  The project's fp32-class rule: new error <= 1.5 x old error, on the whole g_vec and
    on the radial scalar alone (the part that changed; the spherical part's error is common to both)."""
    L, lib = _lib()
    dev = 'cuda:0'
    c = _fused_case(model, layer, 70 + layer, pairs)
    spec, nb, wn, dx, dout, nsh, N, E, R, NT = (c[k] for k in ('spec', 'nb', 'wn', 'dx', 'dout', 'nsh', 'N', 'E', 'R', 'NT'))
    lmax = int(round(math.sqrt(nsh))) - 1
    P, cf, coeffs = _edge_params(L, 0, lmax)
    # geometry: one vector per radial row; a directed edge carries +- its row's vector (the two edges of a pair: same |r| bit for bit)
    pvec = _vectors(R, 7 + layer)
    if pairs:
        sgn = (torch.randint(0, 2, (E,), generator=torch.Generator().manual_seed(3)) * 2 - 1).float()
        vec = (pvec[c['w_row'].long()] * sgn[:, None]).contiguous()
    else:
        vec = pvec.clone()
    pvec, vec = pvec.to(dev), vec.to(dev)
    emb_r, sh_r = torch.empty(R, nb, device=dev), torch.empty(R, nsh, device=dev)
    emb_e, sh, dsh = torch.empty(E, nb, device=dev), torch.empty(E, nsh, device=dev), torch.empty(E, 3 * nsh, device=dev)
    demb = torch.empty(R, nb, device=dev)
    L.check(lib.snet_edge_embed_fwd(C.byref(P), cf, _p(pvec), R, _p(emb_r), _p(sh_r), None, None))
    L.check(lib.snet_edge_embed_fwd(C.byref(P), cf, _p(vec), E, _p(emb_e), _p(sh), _p(dsh), None))
    L.check(lib.snet_edge_embed_tangent(C.byref(P), cf, _p(pvec), None, R, _p(demb), None))
    fp = lambda t: t.numpy().ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    mlp, plan, fplan = C.c_void_p(), C.c_void_p(), C.c_void_p()
    cst = 1.6791767923989418
    L.check(lib.snet_radial_mlp_plan_create(nb, 64, 64, wn, fp(c['W0']), fp(c['W1']), fp(c['W2']), 0, cst, 1, C.byref(mlp)))
    L.check(lib.snet_conv_plan_create(spec.tag.encode(), C.byref(plan)))
    L.check(lib.snet_fused_plan_create(plan, mlp, 4, C.byref(fplan)))
    rp, sr = c['row_ptr'].to(dev), c['src'].to(dev)
    wr = None if c['w_row'] is None else c['w_row'].to(dev)
    x, g_out = c['x'].to(dev), c['g_out'].to(dev)
    scale = 0.25
    # ---- fp64 reference: separate fp32 kernels for g_w and the spherical part, the radial contraction in fp64
    w_ref, g_w = torch.empty(R, wn, device=dev), torch.empty(E, wn, device=dev)
    g_sph_ref = torch.zeros(E, 3, device=dev)
    L.check(lib.snet_radial_mlp_fwd(mlp, _p(emb_r), R, _p(w_ref), None))
    L.check(lib.snet_conv_bwd_edge_vec(plan, _p(x), _p(sh), _p(dsh), _p(w_ref), _p(wr), _p(rp), _p(sr), N, scale, _p(g_out), _p(g_w),
                                       None, _p(g_sph_ref), None))
    r64 = pvec.double().cpu().norm(dim=1)
    emb64, demb64 = embedding_and_tangent(r64, coeffs, RC, 'poly_cut', 6)
    _, h2d64 = tangent_reference(emb64, demb64, c['W0'].double(), c['W1'].double(), 'silu')
    wd64 = h2d64 @ c['W2'].double()
    rows = torch.arange(E) if wr is None else c['w_row'].long()
    torch.cuda.synchronize()
    gr64 = (g_w.double().cpu() * wd64[rows]).sum(1)
    v64 = vec.double().cpu()
    unit = v64 / v64.norm(dim=1, keepdim=True)
    g_vec64 = g_sph_ref.double().cpu() + gr64[:, None] * unit
    # ---- both kernels
    h2, h2d = torch.empty(R, 64, device=dev), torch.empty(R, 64, device=dev)
    L.check(lib.snet_radial_mlp_hidden_fwd_layers_tangent((C.c_void_p * 1)(mlp), 1, _p(emb_r), _p(demb), R, (C.c_void_p * 1)(h2.data_ptr()),
                                                          (C.c_void_p * 1)(h2d.data_ptr()), None))
    tile_ptr, tile_node, n_tiles = _work_list(L, lib, fplan, rp, c['row_ptr'], N, E, dev)
    if lib.snet_fused_plan_tile_mode(fplan) == 1:   # packed work list: this case has tiles that span two rows
        tn = tile_node.cpu()[:2 * n_tiles.value].view(-1, 2)
        assert (tn[:, 0] != tn[:, 1]).any()
    x_max, g_max = torch.empty(NT, device=dev), torch.empty(N, device=dev)
    L.check(lib.snet_row_absmax(_p(x), NT, dx, _p(x_max), None))
    L.check(lib.snet_row_absmax(_p(g_out), N, dout, _p(g_max), None))
    assert lib.snet_fused_plan_has_mlp_tail(fplan) == 1
    g_xe_o = torch.full((E, dx), float('nan'), device=dev) if gx else None
    g_xe_n = torch.full((E, dx), float('nan'), device=dev) if gx else None
    g_emb, g_old, g_new = torch.zeros(E, nb, device=dev), torch.zeros(E, 3, device=dev), torch.zeros(E, 3, device=dev)
    L.check(lib.snet_conv_bwd_fused(fplan, _p(x), _p(sh), _p(dsh), _p(h2), _p(wr), _p(rp), _p(sr), _p(tile_ptr), _p(tile_node),
                                    n_tiles.value, scale, _p(g_out), _p(g_xe_o), None, _p(emb_e), _p(g_emb), _p(g_old), _p(x_max), _p(g_max), None))
    torch.cuda.synchronize()
    g_sph_old = g_old.clone()
    L.check(lib.snet_edge_embed_bwd(C.byref(P), cf, _p(vec), E, _p(g_emb), None, _p(g_old), 1, None))
    L.check(lib.snet_conv_bwd_fused_tangent(fplan, _p(x), _p(sh), _p(dsh), _p(h2), _p(h2d), _p(wr), _p(rp), _p(sr), _p(tile_ptr),
                                            _p(tile_node), n_tiles.value, scale, _p(g_out), _p(g_xe_n), _p(vec), _p(g_new), _p(x_max),
                                            _p(g_max), None))
    with pytest.raises(RuntimeError, match='h2d'):
        L.check(lib.snet_conv_bwd_fused_tangent(fplan, _p(x), _p(sh), _p(dsh), _p(h2), None, _p(wr), _p(rp), _p(sr), _p(tile_ptr),
                                                _p(tile_node), n_tiles.value, scale, _p(g_out), _p(g_xe_n), _p(vec), _p(g_new), _p(x_max),
                                                _p(g_max), None))
    # no tiles (an edge-free graph): nothing is launched, nothing is read
    L.check(lib.snet_conv_bwd_fused_tangent(fplan, None, None, None, None, None, None, _p(rp), None, None, None, 0, scale, None, None, None,
                                            None, _p(x_max), _p(g_max), None))
    torch.cuda.synchronize()
    assert not torch.isnan(g_new).any() and not torch.isnan(g_old).any()
    if gx:   # the source-row gradient does not depend on the mode (two instantiations of one source: equal up to the last bit)
        assert not torch.isnan(g_xe_n).any()
        assert (g_xe_n - g_xe_o).abs().max().item() <= 1e-6 * g_xe_o.abs().max().item()
    old_e = (g_old.double().cpu() - g_vec64).abs().max().item()
    new_e = (g_new.double().cpu() - g_vec64).abs().max().item()
    # the radial scalar alone: what each path added along the unit vector on top of ITS OWN kernel's spherical part
    sph_new = g_sph_old.double().cpu()   # (the spherical part is the same arithmetic in both modes)
    rad_old = ((g_old.double().cpu() - g_sph_old.double().cpu()) * unit).sum(1)
    rad_new = ((g_new.double().cpu() - sph_new) * unit).sum(1)
    old_r, new_r = (rad_old - gr64).abs().max().item(), (rad_new - gr64).abs().max().item()
    print(f'{model} layer {layer}: max|g_vec| {g_vec64.abs().max().item():.3g}, max|dE/dr| {gr64.abs().max().item():.3g} | g_vec error vs fp64 '
          f'old {old_e:.3e} new {new_e:.3e} | radial scalar old {old_r:.3e} new {new_r:.3e}')
    assert new_e <= 1.5 * old_e, (new_e, old_e)
    assert new_r <= 1.5 * old_r, (new_r, old_r)
    lib.snet_fused_plan_destroy(fplan)
    lib.snet_conv_plan_destroy(plan)
    lib.snet_radial_mlp_plan_destroy(mlp)


def test_engine_tangent_equals_reverse_mode():
    """whole model, both hosts: the tangent path (default) against the reverse-mode path (tangent=False) and the fp64 oracle, on a cell
    with and one without edges.  Energies are bit-identical (the forward pass does not change); forces obey the fp32-class rule."""
    from oracle.model import OracleModel
    from sevennet_amd.engine import HipForceEngine, build_graph
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.native_model import NativeModel
    from sevennet_amd.neighbor import diamond_cubic, neighbor_list
    from sevennet_amd.synthetic import random_state_dict
    cfg = sevennet_0_config()
    sd = random_state_dict(cfg, seed=0)
    pos, cell = diamond_cubic(5.431, (2, 2, 2), 0.05, 0)
    ei, ev, _ = neighbor_list(pos, cell, [True] * 3, cfg['cutoff'])
    types = np.zeros(len(pos), np.int64)
    ref1 = OracleModel(cfg, sd, dtype=torch.float64).forward(types, ei, ev)
    sd = dict(sd)   # MD-scale forces (max |F| = 8 eV/A), as smoke() does
    sd['rescale_atomic_energy.scale'] = (np.asarray(sd['rescale_atomic_energy.scale'], np.float64) * 8.0 / float(ref1['forces'].abs().max())).astype(np.float32)
    ref = OracleModel(cfg, sd, dtype=torch.float64).forward(types, ei, ev)
    g = build_graph(types, ei, ev, device='cuda:0')
    new = HipForceEngine(cfg, sd, device='cuda:0').compute(g)
    old = HipForceEngine(cfg, sd, device='cuda:0', tangent=False).compute(g)
    nat = NativeModel(cfg, sd, device='cuda:0').compute(g)
    torch.cuda.synchronize()
    assert torch.equal(new['energy'], old['energy']) and torch.equal(new['atomic_energy'], old['atomic_energy'])
    assert torch.equal(new['forces'], nat['forces']) and torch.equal(new['dE_dr'], nat['dE_dr']) and torch.equal(new['virial'], nat['virial'])
    f_ref = ref['forces'].numpy()
    d_new, d_old = np.abs(new['forces'].cpu().numpy() - f_ref).max(), np.abs(old['forces'].cpu().numpy() - f_ref).max()
    print(f'forces vs fp64 at max|F| = {np.abs(f_ref).max():.3g} eV/A: reverse mode {d_old:.3e}, tangent {d_new:.3e}; '
          f'max |F_new - F_old| {(new["forces"] - old["forces"]).abs().max().item():.3e}')
    assert d_new <= 1.5 * d_old and d_new < 1e-4
    # isolated atoms: no edges anywhere in the reverse pass
    g0 = build_graph(np.zeros(3, np.int64), np.zeros((2, 0), np.int64), np.zeros((0, 3)), device='cuda:0')
    out0 = HipForceEngine(cfg, sd, device='cuda:0').compute(g0)
    torch.cuda.synchronize()
    assert out0['forces'].abs().max().item() == 0.0 and out0['dE_dr'].shape[0] == 0
