#!/usr/bin/env python3
"""Bit identity of the native whole-model sequencer (csrc/snet_model.cpp, through NativeModel) between two trees of this package:
a refactor of its host code against its parent commit.  Built like tools/driver_identity.py.

    python tools/model_identity.py TREE OUT.pkl             run the cases below with the package of TREE, pickle the results
    python tools/model_identity.py --compare A.pkl B.pkl [--report FILE]    A is the reference
    python tools/model_identity.py --single TREE            one evaluation of the mini and of the unit model (under rocprofv3
                                                            --kernel-trace: the launch order of a tree)
    python tools/model_identity.py --call-time TREE         wall time per call of 200 cache-hit evaluations, 64-atom mini model

Each tree runs in a process of its own, on the libsnet_hip.so built in it.  Every case is a list of NativeModel.compute(g,
want_atomic_virial=True) calls; recorded after every call: all output tensors and eval_syncs().  Random weights, synthetic diamond
cells (tests/helpers.py synthetic_system).  Cases: the six CASES of tests/test_native_model_gpu.py ((2,2,2) cell, a (1,1,1) cell out of
the same arena, back); the mini SevenNet-0 shape with layer0_moments / last_layer_merged in all four combinations and with
SNET_FUSED_TERMS 2 and 3; sevennet_0_config(num_species=2) -- packed tiles -- on the (2,2,2) cell twice, the (2,2,3) cell, and back
(cache hit, miss, rebuild); a graph without the pair map (share_pairs=False); the isolated atom; SNET_NO_OVERLAP=1; two bricks of
the (4,4,3) cell (SevenNet-0 shape) and of the (4,4,4) cell (mini) of tests/test_engine_gpu.py, one host thread each, ghost rows
through Python callbacks, through the library's loopback halo (interior / boundary split) and the same with
SNET_NO_HALO_SPLIT=1.  Compared: every tensor by shape, dtype and bytes, every counter by ==."""
import argparse
import contextlib
import json
import os
import pickle
import sys
import threading
import time

import numpy as np


@contextlib.contextmanager
def environment(**kw):
    """os.environ with `kw` set (the sequencer reads SNET_NO_OVERLAP / SNET_FUSED_TERMS when a model is loaded, SNET_NO_HALO_SPLIT
    in every evaluation)"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def use_tree(tree):
    sys.path.insert(0, os.path.abspath(tree))
    sys.path.insert(0, os.path.join(os.path.abspath(tree), 'tests'))
    import sevennet_amd
    from sevennet_amd import _lib
    assert os.path.abspath(sevennet_amd.__file__).startswith(os.path.abspath(tree) + os.sep), sevennet_amd.__file__
    assert os.path.abspath(_lib.LIB_PATH).startswith(os.path.abspath(tree) + os.sep), _lib.LIB_PATH


def graph(n_rep, sigma, seed, cutoff, nsp, **kw):
    from helpers import synthetic_system
    from sevennet_amd.engine import build_graph
    types, _, _, ei, ev = synthetic_system(n_rep, sigma=sigma, seed=seed, cutoff=cutoff, n_species=nsp)
    return build_graph(types, ei, ev, device='cuda:0', num_species=nsp, **kw)


def calls(nat, graphs):
    """[(outputs, eval_syncs)] of nat.compute on every graph in turn"""
    import torch
    out = []
    for g in graphs:
        o = nat.compute(g, want_atomic_virial=True)
        torch.cuda.synchronize()
        out.append(({k: v.cpu().numpy() for k, v in o.items()}, nat.eval_syncs()))
    return out


def brick_cases(record, model):
    import torch
    from helpers import synthetic_system
    from sevennet_amd.engine import build_graph
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.native_model import NativeModel
    from sevennet_amd.parallel import LoopbackHub, NativeHalo, build_brick_graph
    from sevennet_amd.shapes import mini_sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    world = 2
    if model == 'sevennet_0':   # test_interior_boundary_split_of_the_fused_convolutions
        cfg = sevennet_0_config(num_species=2)
        sd = random_state_dict(cfg, seed=4)
        types, pos, cell, ei, ev = synthetic_system((4, 4, 3), sigma=0.06, seed=8, cutoff=5.0, n_species=2)
    else:                       # test_bricks_through_the_native_halo_equal_single_graph
        cfg = mini_sevennet_0_config()
        sd = random_state_dict(cfg, seed=9)
        types, pos, cell, ei, ev = synthetic_system((4, 4, 4), sigma=0.06, seed=4, cutoff=5.0, n_species=2)
    bricks = [build_brick_graph(pos, cell, types, 5.0, world, r, neighbors=(ei, ev)) for r in range(world)]
    assert any(0 < b.n_interior < b.n_local for b in bricks)

    class CallbackHalo:   # the same exchange behind Python callbacks: the sequencer then cannot split
        def __init__(self, h):
            self.forward, self.reverse = h.forward, h.reverse

    for name, wrap, env in (('python callbacks', CallbackHalo, {}), ('library halo, split', lambda h: h, {}),
                            ('library halo, SNET_NO_HALO_SPLIT=1', lambda h: h, {'SNET_NO_HALO_SPLIT': '1'})):
        hub = LoopbackHub(world)
        halos = [NativeHalo(hub.comm(r), bricks[r].send_lists, bricks[r].recv_counts) for r in range(world)]
        models = [NativeModel(cfg, sd) for _ in range(world)]
        results, errors = [None] * world, []

        def rank(r):
            try:
                with torch.cuda.stream(torch.cuda.Stream(device='cuda:0')):
                    b = bricks[r]
                    g = build_graph(b.types, b.edge_index, b.edge_vec, n_local=b.n_local, n_interior=b.n_interior, device='cuda:0')
                    models[r].set_halo(wrap(halos[r]))
                    results[r] = calls(models[r], [g, g])
            except Exception as e:  # noqa: BLE001
                errors.append((r, e))
                hub.abort()

        with environment(**env):
            threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
            for t in threads:
                t.start()
            for t in threads:
                t.join(300)
        assert not errors, errors
        for r in range(world):
            record[f'two bricks of {model}, {name}, rank {r}'] = results[r]


def run(tree, out_path):
    use_tree(tree)
    from sevennet_amd.model_spec import sevennet_0_config
    from sevennet_amd.native_model import NativeModel
    from sevennet_amd.shapes import mini_sevennet_0_config, unit_test_config
    from sevennet_amd.synthetic import random_state_dict
    from test_native_model_gpu import CASES
    record = {}
    for name, c in CASES.items():
        cfg = unit_test_config(**c['over']) if c['cfg'] == 'unit' else mini_sevennet_0_config()
        g, g2 = graph((2, 2, 2), 0.08, 11, c['cutoff'], c['nsp']), graph((1, 1, 1), 0.05, 2, c['cutoff'], c['nsp'])
        record[f'CASES[{name}]: (2,2,2), (1,1,1), (2,2,2)'] = calls(NativeModel(cfg, random_state_dict(cfg, seed=7)), [g, g2, g])
    mini, unit = mini_sevennet_0_config(), unit_test_config()
    sd_mini, sd_unit = random_state_dict(mini, seed=7), random_state_dict(unit, seed=7)
    g_mini, g_unit = graph((2, 2, 2), 0.08, 11, 5.0, 2), graph((2, 2, 2), 0.08, 11, 4.0, 4)
    for l0 in (True, False):
        for ll in (True, False):
            record[f'mini, layer0_moments={l0}, last_layer_merged={ll}'] = \
                calls(NativeModel(mini, sd_mini, layer0_moments=l0, last_layer_merged=ll), [g_mini, g_mini])
    for terms in ('2', '3'):
        with environment(SNET_FUSED_TERMS=terms):
            nat = NativeModel(mini, sd_mini)
        record[f'mini, SNET_FUSED_TERMS={terms}'] = calls(nat, [g_mini, g_mini])
    s0 = sevennet_0_config(num_species=2)
    a, b = graph((2, 2, 2), 0.05, 1, 5.0, 2), graph((2, 2, 3), 0.05, 2, 5.0, 2)
    record['sevennet_0(num_species=2): (2,2,2) twice, (2,2,3), (2,2,2)'] = calls(NativeModel(s0, random_state_dict(s0, seed=2)), [a, a, b, a])
    record['mini, share_pairs=False'] = calls(NativeModel(mini, sd_mini), [graph((2, 2, 2), 0.08, 11, 5.0, 2, share_pairs=False)] * 2)
    from sevennet_amd.engine import build_graph
    iso = build_graph(np.array([2]), np.zeros((2, 0), np.int64), np.zeros((0, 3)), device='cuda:0', num_species=4)
    record['unit, isolated atom'] = calls(NativeModel(unit, sd_unit), [iso, g_unit, iso])
    with environment(SNET_NO_OVERLAP='1'):
        nat = NativeModel(unit, sd_unit)
    record['unit, SNET_NO_OVERLAP=1'] = calls(nat, [g_unit, g_unit])
    brick_cases(record, 'sevennet_0')
    brick_cases(record, 'mini')
    for key, v in record.items():
        print(key, '-> eval_syncs', [s for _, s in v], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'wb') as f:
        pickle.dump(record, f)


def single(tree):
    use_tree(tree)
    import torch
    from sevennet_amd.native_model import NativeModel
    from sevennet_amd.shapes import mini_sevennet_0_config, unit_test_config
    from sevennet_amd.synthetic import random_state_dict
    for cfg, cutoff, nsp in ((mini_sevennet_0_config(), 5.0, 2), (unit_test_config(), 4.0, 4)):
        NativeModel(cfg, random_state_dict(cfg, seed=7)).compute(graph((2, 2, 2), 0.08, 11, cutoff, nsp), want_atomic_virial=True)
        torch.cuda.synchronize()


def call_time(tree, n_calls=200):
    use_tree(tree)
    import torch
    from sevennet_amd.native_model import NativeModel
    from sevennet_amd.shapes import mini_sevennet_0_config
    from sevennet_amd.synthetic import random_state_dict
    cfg = mini_sevennet_0_config()
    nat, g = NativeModel(cfg, random_state_dict(cfg, seed=7)), graph((2, 2, 2), 0.08, 11, 5.0, 2)
    assert g.n_local == 64
    for _ in range(20):
        nat.compute(g)
    torch.cuda.synchronize()
    s0, t0 = nat.eval_syncs(), time.perf_counter()
    for _ in range(n_calls):
        nat.compute(g)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert nat.eval_syncs() == s0   # cache hits: no synchronisation inside the calls
    print(json.dumps({'tree': os.path.abspath(tree), 'atoms': g.n_local, 'calls': n_calls, 'us_per_call': round(1e6 * dt / n_calls, 2)}), flush=True)


def differences(a, b, where):
    """the places where b is not a, bit for bit"""
    if type(a) is not type(b):
        return [f'{where}: {type(a).__name__} against {type(b).__name__}']
    if isinstance(a, dict):
        out = [] if list(a) == list(b) else [f'{where}: keys {list(a)} against {list(b)}']
        return out + [d for k in a if k in b for d in differences(a[k], b[k], f'{where}[{k!r}]')]
    if isinstance(a, (list, tuple)):
        out = [] if len(a) == len(b) else [f'{where}: length {len(a)} against {len(b)}']
        return out + [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f'{where}[{i}]')]
    if isinstance(a, np.ndarray):
        same = a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
        return [] if same else [f'{where}: arrays {a.shape} {a.dtype} against {b.shape} {b.dtype} differ']
    return [] if a == b else [f'{where}: {a!r} against {b!r}']


def compare(ref_path, new_path, report):
    with open(ref_path, 'rb') as f:
        ref = pickle.load(f)
    with open(new_path, 'rb') as f:
        new = pickle.load(f)
    lines, bad = [], list(differences(list(ref), list(new), 'the cases'))
    for key, want in ref.items():
        lines.append(key)
        lines.append(f'    {len(want)} calls, eval_syncs after each {[s for _, s in want]}, tensors '
                     f'{ {k: v.shape for k, v in want[0][0].items()} }')
        diff = differences(want, new.get(key), key)
        bad += diff
        lines += [f'    DIFFERS {d}' for d in diff] or ['    -> identical']
    lines.append(f'ALL {len(ref)} CASES IDENTICAL (every tensor byte for byte, eval_syncs after every call)' if not bad else f'{len(bad)} DIFFERENCES')
    print('\n'.join(lines))
    if report:
        with open(report, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('paths', nargs='+', help='TREE OUT.pkl; with --compare: REFERENCE.pkl NEW.pkl; with --single / --call-time: TREE')
    ap.add_argument('--compare', action='store_true')
    ap.add_argument('--single', action='store_true')
    ap.add_argument('--call-time', action='store_true')
    ap.add_argument('--report')
    a = ap.parse_args()
    if a.single or a.call_time:
        sys.exit((single if a.single else call_time)(*a.paths))
    sys.exit(compare(a.paths[0], a.paths[1], a.report) if a.compare else run(*a.paths))


if __name__ == '__main__':
    main()
