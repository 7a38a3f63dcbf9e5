"""CPU: the eligibility predicate of the last layer's one-launch reverse pass (model_spec.lastlayer_merged_eligible), the fp64
restatement of its algebra (tests/lastlayer_ref.py) against autograd through the oracle's tensor product, and the model-file key."""
import numpy as np
import pytest
import torch

from fused_range import fused_reference
from lastlayer_ref import hand_graph, lastlayer_reference, meta_of, random_inputs, without_meta_key


def _last(cfg):
    from sevennet_amd.model_spec import build_model_spec
    return build_model_spec(cfg).layers[-1]


def test_eligibility_predicate():
    from sevennet_amd.model_spec import (LASTLAYER_LDS_BUDGET, build_model_spec, lastlayer_merged_eligible, sevennet_0_config,
                                         sevennet_l3i5_config, sevennet_mf_ompa_config)
    from sevennet_amd.shapes import lastlayer_test_configs, mini_sevennet_0_config
    tags = []
    for cfg in (sevennet_0_config(), sevennet_l3i5_config(), sevennet_mf_ompa_config()):
        layers = build_model_spec(cfg).layers
        assert lastlayer_merged_eligible(layers[-1].conv, layers[-1].mlp_dims)                 # the three shipped last layers
        tags.append(layers[-1].conv.tag)
        assert not lastlayer_merged_eligible(layers[2].conv, layers[2].mlp_dims)               # a middle layer: non-scalar outputs
        assert not lastlayer_merged_eligible(layers[0].conv, layers[0].mlp_dims)               # paths (0, l -> l): outputs of every l
        assert not lastlayer_merged_eligible(layers[-1].conv, [8, 32, 32, layers[-1].conv.weight_numel])   # another radial network
        wn = layers[-1].conv.weight_numel
        assert 64 * wn * 4 <= LASTLAYER_LDS_BUDGET                                              # the W2 image fits beside a second workgroup's
    assert tags == ['005c575f8ec2', '8e687c31f582', '502c5bba8e99']
    for cfg in lastlayer_test_configs().values():
        ls = _last(cfg)
        assert lastlayer_merged_eligible(ls.conv, ls.mlp_dims)
    mini = _last(mini_sevennet_0_config())                                                      # 8 and 4 channels: no 16-channel tiles
    assert not lastlayer_merged_eligible(mini.conv, mini.mlp_dims)


@pytest.mark.parametrize('name', ['last16_l1', 'last16_l2', 'last16_o3_dead', 'sevennet_0'])
def test_restatement_matches_autograd(name):
    """g_x and g_vec of the restatement against autograd through oracle.model.tp_uvu (tests/fused_range.fused_reference): the per-edge
    source-row gradients summed per source, and the spherical part plus the radial scalar along r / |r|"""
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.shapes import lastlayer_test_configs
    spec = _last(sevennet_0_config() if name == 'sevennet_0' else lastlayer_test_configs()[name]).conv
    g = hand_graph(40, 4, seed=3, ghost_degrees=(0, 5, 16, 20))
    c = random_inputs(spec, g, seed=5)
    rng = np.random.default_rng(7)
    nsh = spec.irreps_sh.dim
    t = torch.from_numpy
    sh, dsh = t(rng.normal(0, 1, (g['E'], nsh))), t(rng.normal(0, 1, (g['E'], 3 * nsh)))
    args = dict(x=t(c['x']), sh=sh, dsh=dsh, h2=t(c['h2']), W2=t(c['W2']), w_row=t(c['w_row']), row_ptr=t(g['row_ptr']), src=t(g['src']),
                scale=0.05, g_out=t(c['g_out']), h2d=t(c['h2d']))
    ref = fused_reference(spec, **args)
    ev = t(g['edge_vec']).double()
    gx_auto = torch.zeros(g['NT'], spec.irreps_x.dim, dtype=torch.float64).index_add_(0, t(g['src']).long(), ref['g_xe'])
    gv_auto = ref['g_vec'] + ref['g_rad'][:, None] * ev / ev.norm(dim=1, keepdim=True)
    g_x, g_vec = lastlayer_reference(spec, args['x'], args['g_out'], sh, dsh, t(g['edge_vec']), args['h2'], args['h2d'], args['W2'],
                                     args['w_row'], args['row_ptr'], args['src'], 0.05)
    assert gx_auto.abs().max() > 0.1 and gv_auto.abs().max() > 0.1
    assert (g_x - gx_auto).abs().max() <= 1e-12 * gx_auto.abs().max()
    assert (g_vec - gv_auto).abs().max() <= 1e-12 * gv_auto.abs().max()
    dead = [i for i in range(len(spec.irreps_x)) if not any(p.i_x == i for p in spec.paths)]
    assert bool(dead) == (name == 'last16_o3_dead')
    for i in dead:                                                                              # a block no path reads: zero gradient
        o, (m, l, _) = spec.irreps_x.offsets()[i], spec.irreps_x[i]
        assert (g_x[:, o:o + m * (2 * l + 1)] == 0).all() and (gx_auto[:, o:o + m * (2 * l + 1)] == 0).all()


def test_model_file_key_round_trips(tmp_path):
    from sevennet_amd.model_file import write_model_file
    from sevennet_amd.shapes import lastlayer_test_configs, mini_sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    for cfg, want in ((lastlayer_test_configs()['last16_l2'], '1'), (mini_sevennet_0_config(), '0')):
        path = tmp_path / f'm{want}.snet'
        write_model_file(str(path), cfg, random_state_dict(cfg, seed=1))
        blob = path.read_bytes()
        meta = meta_of(blob)
        assert meta['last_layer_merged'] == want and 'layer0_moments' in meta
        old = without_meta_key(blob, 'last_layer_merged')
        assert 'last_layer_merged' not in meta_of(old) and meta_of(old)['layer0_moments'] == meta['layer0_moments']
        assert len(old) == len(blob) - len(f'last_layer_merged={want}\n')
