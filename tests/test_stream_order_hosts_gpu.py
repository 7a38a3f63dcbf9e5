"""GPU: the stream contract of the hosts and the drivers (tests/stream_order.py has the method; test_stream_order_ops_gpu.py the
positive control that shows the harness catching a launch on the wrong stream).

Hosts on an already-evaluated Graph -- HipForceEngine.compute (fused kernels; unfused, where the engine's own side stream runs
beside a non-default main stream; a batch with per-system reductions), NativeModel.compute, D3Engine.compute_device -- take their
floating-point input late, behind a delay on a fresh non-default stream, and must return the default stream's bits; none of them
synchronises, so the delay must still be running when they return.  BatchForces builds its neighbour list from late device
positions and reads the edge count back: B is A plus a rattle that keeps the edge set (checked on the CPU, no pair within
0.01 A of the cutoff).  The drivers take host arrays: the whole call runs inside the delayed stream against the whole call on
the default stream, every returned array bit for bit.

Systems: the 64-atom cell of helpers.synthetic_system((2, 2, 2)) and the three small cells of test_relax_gpu.  Every path
here is bit-repeatable on the default stream (the project's "two runs are identical" tests claim it per path; asserted again per
case)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import synthetic_system
from stream_order import run_ab, run_whole, same_edge_set
from test_batch_gpu import Z, _batch, _calc
from test_relax_gpu import D3_CUT, _args, _cells

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OUTS = ('energy', 'atomic_energy', 'dE_dr', 'forces', 'virial', 'atomic_virial')


@functools.lru_cache(maxsize=None)
def _host_case(case):
    """engine, native sequencer (None for the batch) and an already-evaluated graph"""
    from sevennet_amd.engine import HipForceEngine, build_graph
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.native_model import NativeModel
    from sevennet_amd.shapes import mini_sevennet_0_config, unit_test_config
    from sevennet_amd.synthetic import random_state_dict
    if case == 'batch':
        calc, _, _ = _calc(mini_sevennet_0_config(), compute_atomic_virial=True)
        eng, nat, g = calc.model, None, _batch(calc, _cells())
        assert g.seg_ptr is not None
    else:
        cfg, nsp, rc, fused = (sevennet_0_config(), 1, 5.0, True) if case == 'sevennet_0' else (unit_test_config(), 4, 4.0, False)
        sd = random_state_dict(cfg, seed=0)
        types, _, _, ei, ev = synthetic_system((2, 2, 2), sigma=0.05, seed=0, cutoff=rc, n_species=nsp)
        eng, nat = HipForceEngine(cfg, sd, device=DEV), NativeModel(cfg, sd, device=DEV)
        g = build_graph(types, ei, ev, device=DEV, num_species=eng.spec.num_species)
        assert any(L.fused_fwd or L.fused_bwd for L in eng.layers) == fused
        if not fused:   # the unfused path is the one with the engine's own side stream
            assert eng.overlap and g.n_edges <= eng.OVERLAP_MAX_EDGES and all(L.fused_mlp for L in eng.layers)
    for host in (eng, nat):
        if host is not None:
            host.compute(g, want_atomic_virial=True)      # tile lists, species sets, plans and arenas exist from here on
    torch.cuda.synchronize()
    return SimpleNamespace(eng=eng, nat=nat, g=g)


def _late_edge_vec(g):
    """B = 0.97 A: every length shrinks (nothing crosses the cutoff), and the two directions of a pair stay opposite and equally
    long, as the shared radial rows assume"""
    a = g.edge_vec.clone()
    return (g.edge_vec, a, (a * 0.97).contiguous())


def _outputs(out, batch):
    keys = OUTS + (('energy_per_system', 'virial_per_system') if batch else ())
    return [out[k] for k in keys]


# (the native sequencer takes one structure per call: no batch row for it)
@pytest.mark.parametrize('case,host', [('sevennet_0', 'engine'), ('unit', 'engine'), ('batch', 'engine'), ('sevennet_0', 'native'),
                                       ('unit', 'native')])
def test_compute_with_late_edge_vectors(case, host):
    """energy, atomic energies, dE/dr, forces, virial and atomic virial (the batch: per-system energies and virials too) with
    g.edge_vec late; then the same host once more on the default stream; the native sequencer also against the engine"""
    c = _host_case(case)
    model = c.eng if host == 'engine' else c.nat
    late = [_late_edge_vec(c.g)]
    call = lambda: _outputs(model.compute(c.g, want_atomic_virial=True), case == 'batch')   # noqa: E731
    ref, got = run_ab(f'{type(model).__name__}.compute[{case}]', late, call)
    # the same host once more on the default stream: the default-stream bits again
    c.g.edge_vec.copy_(late[0][2])
    torch.cuda.synchronize()
    again = call()
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(again, ref)):
        assert torch.equal(x, y), k
    if host == 'native':    # ... and bit-identical to the engine there, as today
        eng = _outputs(c.eng.compute(c.g, want_atomic_virial=True), False)
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(got, eng)):
            assert torch.equal(x, y), OUTS[k]
    c.g.edge_vec.copy_(late[0][1])
    torch.cuda.synchronize()


def _rattled(systems, sigma, seed):
    rng = np.random.default_rng(seed)
    return [p + rng.normal(0.0, sigma, p.shape) for p in (s[1] for s in systems)]


def test_d3_compute_device_with_late_positions():
    """D3Engine.compute_device after plan(): late device positions.  The D3 kernels loop over every atom and every planned
    lattice translation -- no neighbour list, and no buffer whose size depends on the positions -- so the rattle needs no
    edge-set check here; the translation tables depend on the (fixed) cells alone.  This relies on all three systems being fully
    periodic: a molecule's box, and with it its translation list, would be formed from the positions of each call."""
    from sevennet_amd.d3 import D3Engine
    eng = D3Engine('damp_bj', 'pbe', D3_CUT['vdw_cutoff'], D3_CUT['cn_cutoff'])
    systems = _cells()
    z, pos, cells, pbcs = _args(systems)
    plan = eng.plan(np.concatenate(z), [len(p) for p in pos], cells, pbcs)
    a = torch.as_tensor(np.concatenate(pos)).to(DEV)
    b = torch.as_tensor(np.concatenate(_rattled(systems, 0.002, 5))).to(DEV)
    torch.cuda.synchronize()
    buf = a.clone()

    def call():
        eng.compute_device(plan, buf)       # (writes the plan's own output tensors)
    ref, _ = run_ab('D3Engine.compute_device', [(buf, a, b)], call, outs=[plan.energy, plan.forces, plan.virial, plan.cn])
    assert plan.status.tolist() == [0] * len(systems) and float(ref[1].abs().max()) > 1e-4


@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd)


def test_batch_forces_with_late_positions(model):
    """the force call of the batched drivers: neighbour list from late device positions, one edge-count readback (exempt from the
    pending assertion).  B keeps A's edge set."""
    from sevennet_amd.batch import BatchForces, validate_batch_inputs
    systems = _cells()
    rc = model.calc.cutoff
    pos_b = _rattled(systems, 0.002, 7)
    for s, pb in zip(systems, pos_b):
        assert same_edge_set(s[1], pb, s[2], s[3], rc), 'the rattle changes the edge set or a pair sits within 0.01 A of the cutoff'
    types, _, n_at, cells, pbcs = validate_batch_inputs([s[0] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
                                                        np.array([s[3] for s in systems]), rc, model.calc.model.spec.num_species)
    forces = BatchForces(model.calc.model, types, n_at, cells, pbcs, rc, None)
    a = torch.as_tensor(np.concatenate([s[1] for s in systems])).to(DEV)
    b = torch.as_tensor(np.concatenate(pos_b)).to(DEV)
    buf = a.clone()

    def call():
        g, out, _, _ = forces(buf)
        return [out['forces'], out['energy_per_system'], out['virial_per_system'], out['atomic_energy'], g.edge_vec]
    run_ab('BatchForces', [(buf, a, b)], call, reads_back=True)


# ------------------------------------------------------------------------------------------------ the drivers, whole calls
def _numbers(systems):
    return [np.array(Z)[s[0]] for s in systems]


def _md_args(systems):
    from test_md_batch_gpu import MASS_OF
    z, pos, cells, pbcs = _args(systems)
    return z, pos, [MASS_OF[s[0]] for s in systems], cells, pbcs


def _other(systems, seed=9):
    """the systems with rattled positions: what the disturbing call of run_whole evaluates"""
    return [(s[0], p) + tuple(s[2:]) for s, p in zip(systems, _rattled(systems, 0.01, seed))]


def test_compute_many(model):
    systems = _cells()
    run_whole('compute_many', lambda: model.calc.compute_many(*_args(systems)), lambda: model.calc.compute_many(*_args(_other(systems))))


def test_d3_calculator_compute_many():
    from sevennet_amd.d3 import D3Calculator
    d3 = D3Calculator(**D3_CUT)
    systems = _cells()
    run_whole('D3Calculator.compute_many', lambda: d3.compute_many(*_args(systems)), lambda: d3.compute_many(*_args(_other(systems))))


def test_md_many_langevin(model):
    systems = _cells()
    run = lambda sy: model.calc.md_many(*_md_args(sy), 1.0, 20, seed=3, temperature=350.0, friction=0.01)   # noqa: E731
    res = run_whole('md_many', lambda: run(systems), lambda: run(_other(systems)))
    assert all(not np.array_equal(r['positions'], s[1]) for r, s in zip(res, systems))


def test_md_many_pressure(model):
    systems = _cells()
    run = lambda sy: model.calc.md_many(*_md_args(sy), 1.0, 10, seed=5, temperature=300.0, friction=0.01, pressure=0.01,   # noqa: E731
                                        compressibility=50.0, barostat_time=100.0)
    res = run_whole('md_many(pressure)', lambda: run(systems), lambda: run(_other(systems)))
    assert all(not np.array_equal(r['cell'], s[2]) for r, s in zip(res, systems))


def test_relax_many_fixed_cell(model):
    systems = _cells()
    run = lambda sy: model.calc.relax_many(*_args(sy), fmax=1e-4, steps=10)   # noqa: E731
    res = run_whole('relax_many', lambda: run(systems), lambda: run(_other(systems)))
    assert all(r['n_steps'] == 10 for r in res)


def test_neb_many(model):
    from test_neb_gpu import K_MODEL, _neb_args, model_bands
    bands = model_bands()
    rng = np.random.default_rng(9)
    other = [(b[0], b[1] + rng.normal(0.0, 0.01, b[1].shape)) + tuple(b[2:]) for b in bands]
    run = lambda bs: model.calc.neb_many(*_neb_args(bs), fmax=1e-4, steps=5, k=K_MODEL)   # noqa: E731
    res = run_whole('neb_many', lambda: run(bands), lambda: run(other))
    assert all(r['n_steps'] == 5 for r in res)


def test_vibrations_many(model):
    """nfree = 2 on the five-atom molecule of the batch tests"""
    from test_vib_gpu import DELTA, _vib_args, model_systems
    systems = model_systems()[1:2]
    assert len(systems[0][1]) == 5
    other = [(s[0], p) + tuple(s[2:]) for s, p in zip(systems, _rattled(systems, 0.01, 9))]
    run = lambda sy: model.calc.vibrations_many(*_vib_args(sy), delta=DELTA, nfree=2, indices=[s[4] for s in sy])   # noqa: E731
    run_whole('vibrations_many', lambda: run(systems), lambda: run(other))


def test_torchsim_model_forward(model):
    from sevennet_amd.torchsim import SevenNetModel
    systems = _cells()
    ts = SevenNetModel((model.cfg, model.sd), device=DEV)
    dev = torch.device(DEV)
    n = [len(s[0]) for s in systems]
    state = lambda sy: SimpleNamespace(positions=torch.as_tensor(np.concatenate([s[1] for s in sy]), device=dev),   # noqa: E731
                            row_vector_cell=torch.as_tensor(np.stack([s[2] for s in systems]), device=dev),
                            pbc=torch.as_tensor(np.array([s[3] for s in systems]), device=dev),
                            atomic_numbers=torch.as_tensor(np.concatenate(_numbers(systems)), device=dev),
                            system_idx=torch.repeat_interleave(torch.arange(len(n), device=dev), torch.as_tensor(n, device=dev)))
    here, other = state(systems), state(_other(systems))
    torch.cuda.synchronize()
    res = run_whole('SevenNetModel.forward', lambda: ts.forward(here), lambda: ts.forward(other))
    assert set(res) >= {'energy', 'forces', 'stress'}
