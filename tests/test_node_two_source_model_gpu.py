"""GPU: the whole model with the node linears on the two-source launches (y = SI2(m) + sc(x) and g_x = sc^T(g_y) + SI1^T(g_h)
written once): the Python host and the native sequencer stay bit-identical, and energies and forces stay in the fp32
class against the fp64 oracle -- at most 1.5 times the error the fp32 PyTorch oracle makes on the same cell, measured here."""
import numpy as np
import pytest
import torch

from helpers import synthetic_system
from test_engine_gpu import _fp32_class, _md_scale_state

pytestmark = pytest.mark.gpu

CASES = {
    # mini SevenNet-0 (linear self-connection: one launch, no row list) on a 64-atom rattled cell, one species and two
    'mini_one_species': ('mini', 1),
    'mini_two_species': ('mini', 2),
    # per-species self-connection (FCTP): one launch per species row list
    'unit_nequip_four_species': ('unit', 4),
}


@pytest.mark.parametrize('case', list(CASES))
def test_hosts_bit_identical_and_fp32_class(case):
    from sevennet_amd.engine import HipForceEngine, build_graph
    from sevennet_amd.native_model import NativeModel
    from sevennet_amd.shapes import mini_sevennet_0_config, unit_test_config
    from sevennet_amd.synthetic import random_state_dict
    kind, n_species = CASES[case]
    cfg = mini_sevennet_0_config() if kind == 'mini' else unit_test_config()
    cutoff = float(cfg['cutoff'])
    types, pos, cell, ei, ev = synthetic_system((2, 2, 2), sigma=0.06, seed=21, cutoff=cutoff, n_species=n_species)
    assert len(types) == 64 and len(set(types.tolist())) == n_species
    sd, ref = _md_scale_state(cfg, random_state_dict(cfg, seed=5), types, ei, ev)
    eng = HipForceEngine(cfg, sd, device='cuda:0')
    # the launches under test are the ones that run
    assert all(L.fwd2.ok for L in eng.layers if L.sc is not None) and all(L.rev2.ok for L in eng.layers[1:] if L.sc is not None)
    assert any(L.sc is not None for L in eng.layers[1:])
    g = build_graph(types, ei, ev, device='cuda:0', num_species=eng.spec.num_species)
    out = eng.compute(g, want_atomic_virial=True)
    nat = NativeModel(cfg, sd).compute(g, want_atomic_virial=True)
    torch.cuda.synchronize()
    for k in ('energy', 'atomic_energy', 'dE_dr', 'forces', 'virial'):
        assert torch.equal(out[k], nat[k]), k
    r32 = ref['fp32']
    for k, floor in (('energy', 1e-5), ('atomic_energy', 2e-5), ('forces', 2e-6)):
        shape = (1,) if k == 'energy' else ref[k].shape
        err, err32 = _fp32_class(out[k], ref[k].reshape(shape), r32[k].reshape(shape), floor, k)
        print(f'{case}: {k} error vs fp64 {err:.3e}, fp32 oracle {err32:.3e}')
