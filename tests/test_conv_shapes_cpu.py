"""CPU: what the catalogue sweep of the tensor-product kernels (tests/test_conv_shapes_gpu.py) rests on -- the generalised fp64
reference (tests/conv_shapes.py) equals the one it replaces wherever that one worked, equals the UNPRUNED oracle product on the one
shape it did not work on (MF-ompa's third layer, 34 of 68 paths), the sweep's parameter list is the build's own catalogue, and the
bars of the sweep fail on a kernel that is wrong in one path by one part in a thousand."""
import functools

import numpy as np
import pytest
import torch

import conv_shapes as cs

PRUNED_TAG = '0431c055196e'    # MF-ompa layer 3: irreps_mid keeps the 68 blocks of the reference, 34 paths write
KEYS = ('out', 'msg', 'g_xe', 'g_h2', 'g_vec', 'g_rad')


def _old_mid_index(spec):
    """tests/test_ops_gpu._mid_index as it was before tests/conv_shapes.py: the path's RANK among the paths (frozen copy)"""
    order = sorted(range(len(spec.paths)), key=lambda q: (spec.paths[q].out_off, spec.paths[q].out_ch))
    idx = [0] * len(spec.paths)
    for k, q in enumerate(order):
        idx[q] = k
    return idx


def _old_fused_reference(spec, x, sh, dsh, h2, W2, w_row, row_ptr, src, scale, g_out, h2d=None):
    """tests/fused_range.fused_reference as it was before tests/conv_shapes.py (frozen copy)"""
    from oracle.e3 import Irreps as OIrreps
    from oracle.model import tp_uvu
    from sevennet_amd.irreps import irmul_to_mulir_index, mulir_to_irmul_index
    f64 = torch.float64
    N, E, nsh = row_ptr.numel() - 1, src.numel(), sh.shape[1]
    node = torch.repeat_interleave(torch.arange(N), (row_ptr[1:] - row_ptr[:-1]).long())
    rows = torch.arange(E) if w_row is None else w_row.long()
    from_x = torch.as_tensor(irmul_to_mulir_index(spec.irreps_x))
    to_o = torch.as_tensor(mulir_to_irmul_index(spec.irreps_out))
    xe = x.to(f64)[src.long()].clone().requires_grad_(True)
    she = sh.to(f64).clone().requires_grad_(True)
    h2e = h2.to(f64)[rows].clone().requires_grad_(True)
    W2 = W2.to(f64)
    w = h2e @ W2
    w.retain_grad()
    ins = [(p.i_x, p.i_sh, k) for p, k in zip(spec.paths, _old_mid_index(spec))]
    msg = tp_uvu(xe[:, from_x], she, w, OIrreps(str(spec.irreps_x)), OIrreps(str(spec.irreps_sh)), OIrreps(str(spec.irreps_mid)),
                 ins)[:, to_o] * scale
    out = torch.zeros(N, msg.shape[1], dtype=f64).index_add_(0, node, msg)
    (out * g_out.to(f64)).sum().backward()
    res = dict(out=out.detach(), msg=msg.detach(), g_xe=xe.grad, g_h2=h2e.grad,
               g_vec=torch.einsum('ei,eia->ea', she.grad[:, 1:], dsh.to(f64).reshape(E, nsh, 3)[:, 1:]))
    if h2d is not None:
        res['g_rad'] = (w.grad * (h2d.to(f64)[rows] @ W2)).sum(1)
    return res


@functools.lru_cache(maxsize=None)
def _case(tag):
    """the sweep's case with pair-shared radial rows and its two fp64 references, once per tag"""
    return cs.tag_case(tag, True)


def _close(a, b):
    return (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()


def test_sweep_is_the_catalogue():
    """the GPU parametrisation is aot_conv_specs() itself: 31 tags today, 15 of them fusable (every multiplicity a multiple of 16,
    which is codegen_fused's own rule), every layer of every aot_configs() model and every transposed last-layer shape among them"""
    import test_conv_shapes_gpu as gpu
    from sevennet_amd import codegen_fused
    from sevennet_amd.model_spec import build_model_spec, transposed_scalar_conv
    from sevennet_amd.shapes import aot_configs
    cat = cs.catalogue()
    assert gpu.TAGS == list(cat) and len(gpu.TAGS) == 31 and len(set(gpu.TAGS)) == 31
    fus = [t for t in cat if cs.fusable(cat[t])]
    assert gpu.FUSABLE == fus and fus == [t for t in cat if codegen_fused.fusable(cat[t])]
    assert fus == ['63d146a1b3d9', 'ecc5d202727d', '22d6a77ad5ac', '005c575f8ec2', '0b99ee053764', 'c611da7b78ef', '1cad2f51cbd0',
                   '8e687c31f582', '10d3029db455', '568ada5bb7a7', '707b9944ff82', '2d3e65aea6f3', PRUNED_TAG, '502c5bba8e99',
                   '31149129d833']
    transposed = []
    for cfg in aot_configs().values():
        for ls in build_model_spec(cfg).layers:
            assert ls.conv.tag in cat
            tr = transposed_scalar_conv(ls.conv)
            if tr is not None and cs.fusable(ls.conv):
                assert tr[0].tag in cat
                transposed.append((ls.conv.tag, tr[0].tag))
    assert sorted(t for _, t in transposed) == sorted(['0b99ee053764', '10d3029db455', '31149129d833'])
    assert gpu.TRANSPOSED == dict(transposed)
    assert gpu.PRUNED == [t for t in cat if len(cat[t].paths) < len(cat[t].irreps_mid)] == [PRUNED_TAG]
    # the case itself: 149 edges, rows without edges at both ends, 3 ghost rows, 77 radial rows for 149 edges
    c = _case('0b99ee053764')[0]
    assert (c['E'], c['N'], c['NT'], c['R']) == (149, 9, 12, 149 // 2 + 3) and int(c['src'].max()) >= c['N']
    assert len(set(c['w_row'].tolist())) < c['E'] and c['w_row'].tolist() != sorted(c['w_row'].tolist())


@pytest.mark.parametrize('tag', [t for t in cs.catalogue() if t != PRUNED_TAG])
def test_new_reference_equals_the_old_one(tag):
    """wherever the rank-based helper worked (every shape but the pruned one), the out_off / out_ch-based one returns the same
    numbers: every output of the old fused_reference to 1e-12 of its maximum, and fused_range.fused_reference is now the new one"""
    import fused_range as fr
    c, _, new = _case(tag)
    a = cs.case_args(c)
    args = (c['spec'], a['x'], a['sh'], a['dsh'], c['h2'], c['W2'], a['w_row'], a['row_ptr'], a['src'], a['scale'], a['g_out'], c['h2d'])
    old = _old_fused_reference(*args)
    assert _old_mid_index(c['spec']) == cs.mid_index(c['spec']) or cs.unwritten_ranges(c['spec'])
    for k in KEYS:
        assert old[k].shape == new[k].shape and old[k].abs().max().item() > 0 and _close(new[k], old[k]), k
    thin = fr.fused_reference(*args)
    assert all(torch.equal(thin[k], new[k]) for k in KEYS)
    # the quantities the old helper did not return, from the ones it did
    assert _close(new['g_x'], torch.zeros_like(new['g_x']).index_add_(0, c['src'].long(), old['g_xe']))
    assert _close(new['g_h2'], new['g_w'] @ c['W2'].double().T)
    assert new['g_sh'].shape == (c['E'], c['nsh']) and new['g_w'].shape == (c['E'], c['wn'])
    g_vec = torch.einsum('ei,eia->ea', new['g_sh'][:, 1:], c['dsh'].double().reshape(c['E'], c['nsh'], 3)[:, 1:])
    assert torch.equal(g_vec, new['g_vec'])


def test_old_helper_fails_on_the_pruned_shape():
    """why the op-level tests stopped at MF-ompa layer 2: the rank-based index pairs the 34 paths with the first 34 of 68 blocks"""
    spec = cs.catalogue()[PRUNED_TAG]
    assert len(spec.paths) == 34 and len(spec.irreps_mid) == 68
    assert _old_mid_index(spec) != cs.mid_index(spec)
    assert cs.unwritten_ranges(spec)[0][0] == 0      # the first output block (0o) is filled by no path


def test_pruned_reference_equals_the_unpruned_oracle_product():
    """MF-ompa layer 3, the largest kernel of the build and the only pruned one: the reference on the 34-path spec against the
    oracle product of all 68 paths (build_model_spec(_prune_unread_paths=False)) with full weights whose kept columns (w_cols) are
    the test's -- equal to 1e-12 on every column SI2 reads, on g_xe, g_sh, g_vec, g_h2, g_rad and on the kept columns of g_w"""
    from sevennet_amd.model_spec import build_model_spec, sevennet_mf_ompa_config
    layer = build_model_spec(sevennet_mf_ompa_config()).layers[3]
    full = build_model_spec(dict(sevennet_mf_ompa_config(), _prune_unread_paths=False)).layers[3].conv
    c, _, ref = _case(PRUNED_TAG)
    spec = c['spec']
    assert layer.conv.tag == PRUNED_TAG and len(full.paths) == 68 and len(spec.paths) == 34
    assert full.irreps_out == spec.irreps_out and str(full.irreps_mid) == str(spec.irreps_mid)
    cols = torch.as_tensor(np.asarray(layer.w_cols))
    assert cols.numel() == spec.weight_numel and full.weight_numel == 2 * spec.weight_numel
    read = torch.zeros(spec.irreps_out.dim, dtype=torch.bool)    # the columns SI2 reads, from SI2's own blocks
    for b in layer.si2.blocks:
        read[b.in_off:b.in_off + (2 * b.l + 1) * b.mul_in] = True
    assert torch.equal(read, cs.written_mask(spec)) and int(read.sum()) < read.numel()
    assert cs.unwritten_ranges(spec) == ref['unwritten'] and all(not read[b:e].any() for b, e in ref['unwritten'])
    assert sum(e - b for b, e in ref['unwritten']) == int((~read).sum())
    assert c['g_out'][:, ~read].abs().max().item() == 0.0 and c['g_out'][:, read].abs().min().item() > 0.0
    g = torch.Generator().manual_seed(3)
    W2_full = (torch.randn(64, full.weight_numel, generator=g) / 8)
    W2_full[:, cols] = c['W2']
    want = cs.conv_reference(full, h2=c['h2'], W2=W2_full, h2d=c['h2d'], **cs.case_args(c))
    assert not want['unwritten'] and want['out'][:, ~read].abs().max().item() > 0.1    # the unpruned product does fill them
    assert ref['out'][:, ~read].abs().max().item() == 0.0
    assert _close(ref['out'][:, read], want['out'][:, read]) and _close(ref['msg'][:, read], want['msg'][:, read])
    for k in ('g_xe', 'g_x', 'g_sh', 'g_vec', 'g_h2', 'g_rad'):
        assert ref[k].abs().max().item() > 0 and _close(ref[k], want[k]), k
    assert _close(ref['g_w'], want['g_w'][:, cols])


@functools.lru_cache(maxsize=None)
def _fp32_as_kernel(tag, path=-1, factor=1.0):
    """the reference in fp32 torch standing in for a kernel; with `path`, a kernel whose path carries a coupling constant that is
    wrong by `factor`: its output block, its share of g_xe and its g_w block are all off by that factor"""
    c = _case(tag)[0]
    m = torch.ones(c['wn'])
    if path >= 0:
        p = c['spec'].paths[path]
        m[p.w_off:p.w_off + p.mul] = factor
    res = cs.conv_reference(c['spec'], w=c['w'] * m, dtype=torch.float32, **cs.case_args(c))
    res['g_w'] = res['g_w'] * m
    return res


@pytest.mark.parametrize('tag', list(cs.catalogue()))
def test_bars_pass_on_the_fp32_reference(tag):
    """the comparison of the sweep, fed the fp32 torch evaluation as the kernel: inside both bars on every output of every shape"""
    c, ref, _ = _case(tag)
    k32 = _fp32_as_kernel(tag)
    for tol in (cs.TOL_SEPARATE, cs.TOL_FUSED):
        for name in ('out', 'g_xe', 'g_w', 'g_sh', 'g_vec', 'g_x'):
            ok, ratio = cs.judge(k32[name], ref[name], tol, mask=c['written'] if name == 'out' else None)
            assert ok and ratio < 1.0, (name, tol, ratio)


@pytest.mark.parametrize('mutation', [1.0 + 1e-3, -1.0])
@pytest.mark.parametrize('tag', ['22d6a77ad5ac', PRUNED_TAG, '0b99ee053764'])    # SevenNet-0 middle, MF-ompa layer 3, SevenNet-0 transposed
def test_bars_fail_on_one_wrong_path(tag, mutation):
    """... and outside them on out, g_xe and g_w when one path is wrong by 1e-3, or has the wrong sign: whichever path it is"""
    from sevennet_amd.model_spec import build_model_spec, sevennet_0_config
    c, ref, _ = _case(tag)
    if tag == '22d6a77ad5ac':
        assert build_model_spec(sevennet_0_config()).layers[1].conv.tag == tag
    for path in sorted({0, len(c['spec'].paths) // 2, len(c['spec'].paths) - 1}):
        bad = _fp32_as_kernel(tag, path, mutation)
        for name in ('out', 'g_xe', 'g_w'):
            ok, ratio = cs.judge(bad[name], ref[name], cs.TOL_SEPARATE, mask=c['written'] if name == 'out' else None)
            assert not ok and ratio > 1.0, (path, name, ratio)
