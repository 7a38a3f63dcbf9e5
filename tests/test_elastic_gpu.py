"""GPU: batched elastic tensors -- the three kernels against their fp64 restatement (elastic_ref), the loop on an analytic pair
potential, and the driver and the public surfaces on the mini SevenNet-0 model against elastic_ref driven by the fp64 oracle at
the same strained copies: the 2-atom primitive diamond cell with a displaced atom, the rattled triclinic two-species cell of the
batch tests and the perfect 8-atom cubic diamond cell."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import elastic_ref
from helpers import oracle_model
from test_batch_gpu import Z, _calc, _systems
from test_relax_gpu import D3_CUT, DEV, _Atoms

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
DELTA = 0.005


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


# ------------------------------------------------------------------------------------------------ the kernels
KERNEL_N = [1, 5, 300]   # 300: more atoms than threads
B = len(KERNEL_N)


def _kernel_case(nfree):
    """every copy of three systems in one call, with random fp32 forces, fp64 extra forces, fp64 virials and extra virials"""
    from sevennet_amd.elastic import plan_elastic
    rng = np.random.default_rng(21)
    n = np.array(KERNEL_N)
    cells = rng.normal(0.0, 0.6, (B, 3, 3)) + 5.0 * np.eye(3)
    plan = plan_elastic(n, cells, DELTA, nfree, 10 ** 7)
    assert len(plan.calls) == 1
    call = plan.calls[0]
    copy_ptr = np.concatenate([[0], np.cumsum(n[call.desc[:, 0]])])
    N, c = int(copy_ptr[-1]), len(call.ids)
    return SimpleNamespace(nfree=nfree, plan=plan, call=call, n=n, cells=cells, pos0=[rng.uniform(-3.0, 9.0, (k, 3)) for k in KERNEL_N],
                           copy_ptr=copy_ptr, N=N, f32=rng.normal(0.0, 1.0, (N, 3)).astype(np.float32), fx=rng.normal(0.0, 1e-2, (N, 3)),
                           virial=rng.normal(0.0, 5.0, (c, 6)), vx=rng.normal(0.0, 0.1, (c, 6)), volume=plan.slot_volumes[call.ids].copy())


def _strain(case, desc=None):
    from sevennet_amd.elastic import el_strain
    desc = case.call.desc if desc is None else desc
    pos = torch.full((case.N, 3), 123.0, dtype=torch.float64, device=DEV)
    status = torch.zeros(len(desc), dtype=torch.int32, device=DEV)
    el_strain(_t(np.concatenate(case.pos0), torch.float64), _t(np.concatenate([[0], np.cumsum(case.n)]), torch.int32),
              _t(desc, torch.int32), _t(case.copy_ptr, torch.int32), DELTA, pos, status)
    torch.cuda.synchronize()
    return pos.cpu().numpy(), status.cpu().numpy()


def _reduce(case, f32=None, virial=None, volume=None, groups=None):
    """snet_el_rows + snet_el_finish on the case's inputs -> (S [B,6,6], L per system, C, asymmetry, status); every output is
    pre-filled with a sentinel: rows are written, not accumulated, so it must go"""
    from sevennet_amd.elastic import el_finish, el_rows
    f64, i32 = torch.float64, torch.int32
    a_ptr = np.concatenate([[0], np.cumsum(case.n)])
    S = torch.full((36 * B,), 7.0, dtype=f64, device=DEV)
    L = torch.full((18 * int(a_ptr[-1]),), 7.0, dtype=f64, device=DEV)
    status = torch.zeros(B, dtype=i32, device=DEV)
    el_rows(_t(case.virial if virial is None else virial, f64), _t(case.vx, f64), _t(case.volume if volume is None else volume, f64),
            _t(case.f32 if f32 is None else f32, torch.float32), _t(case.fx, f64), _t(case.copy_ptr, i32),
            _t(case.call.groups if groups is None else groups, i32), case.nfree, DELTA, _t(a_ptr, i32), S, L, status)
    C, asym = torch.full_like(S, 7.0), torch.full((B,), 7.0, dtype=f64, device=DEV)
    el_finish(S, status, C, asym)
    torch.cuda.synchronize()
    L_h = L.cpu().numpy()
    return (S.cpu().numpy().reshape(B, 6, 6), [L_h[18 * a_ptr[b]:18 * a_ptr[b + 1]].reshape(6, 3 * case.n[b]) for b in range(B)],
            C.cpu().numpy().reshape(B, 6, 6), asym.cpu().numpy(), status.cpu().numpy())


def _restated(case):
    """elastic_ref on the bits the kernels see -> per system (S, its scale, L, its scale, C, asymmetry)"""
    F = case.f32.astype(np.float64) + case.fx
    out = []
    for b in range(B):
        S, s_scale = np.zeros((6, 6)), np.zeros((6, 6))
        L, l_scale = np.zeros((6, 3 * case.n[b])), np.zeros((6, 3 * case.n[b]))
        for c0, gb, j in case.call.groups:
            if gb != b:
                continue
            sig = [elastic_ref.stress_of(case.virial[c0 + w], case.vx[c0 + w], case.volume[c0 + w]) for w in range(case.nfree)]
            f = [F[case.copy_ptr[c0 + w]:case.copy_ptr[c0 + w + 1]].reshape(-1) for w in range(case.nfree)]
            S[:, j], s_scale[:, j] = elastic_ref.difference(sig, case.nfree, DELTA), elastic_ref.scale(sig, case.nfree, DELTA)
            L[j], l_scale[j] = elastic_ref.difference(f, case.nfree, DELTA), elastic_ref.scale(f, case.nfree, DELTA)
        out.append((S, s_scale, L, l_scale) + elastic_ref.finish(S))
    return out


@pytest.mark.parametrize('nfree', [2, 4])
def test_kernels_equal_the_restatement(nfree):
    """pos_out bit for bit; every element of S and L within 8 x 2^-53 x sum_w |weight_w x_w| / delta.  An element of S takes at
    most seven roundings (the extra virial added, the division by the volume, three sums, the product 12 delta and the division
    by it; the products by 8 and the negation are exact), one of L six (no division by a volume): 8 covers both.  C bitwise
    symmetric and within the bound of S, the asymmetry equal to the restatement's."""
    case = _kernel_case(nfree)
    pos, status = _strain(case)
    assert not status.any()
    want = np.concatenate([elastic_ref.strained(case.pos0[b], j, q, DELTA) for b, j, q in case.call.desc.tolist()])
    assert np.array_equal(pos, want)
    for c, (b, j, q) in enumerate(case.call.desc.tolist()):   # the unstrained copies are the base rows themselves, the others are not
        assert np.array_equal(pos[case.copy_ptr[c]:case.copy_ptr[c + 1]], case.pos0[b]) == (q == 0)
    S, L, C, asym, status = _reduce(case)
    assert not status.any()
    for b, (S_ref, s_scale, L_ref, l_scale, C_ref, asym_ref) in enumerate(_restated(case)):
        s_tol, l_tol = 8 * EPS * s_scale, 8 * EPS * l_scale
        print(f'nfree {nfree}, system {b} (n {KERNEL_N[b]}): max |dS| {np.abs(S[b] - S_ref).max():.3e} (smallest bound {s_tol.min():.3e}), '
              f'max |dL| {np.abs(L[b] - L_ref).max():.3e} (smallest bound {l_tol.min():.3e}), asymmetry {asym[b]:.6e} (restatement {asym_ref:.6e})')
        assert (np.abs(S[b] - S_ref) <= s_tol).all() and (np.abs(L[b] - L_ref) <= l_tol).all()
        assert (np.abs(C[b] - C_ref) <= np.maximum(s_tol, s_tol.T)).all()
        assert np.array_equal(C[b], C[b].T) and np.array_equal(C[b], (S[b] + S[b].T) * 0.5)
        assert asym[b] == asym_ref


def test_a_descriptor_that_does_not_fit_is_refused_and_its_rows_are_left_alone():
    case = _kernel_case(2)
    ref, _ = _strain(case)
    desc = case.call.desc.copy()
    first = {b: int(np.nonzero(desc[:, 0] == b)[0][0]) for b in range(B)}
    wrong_system, wrong_j, wrong_q, wrong_span = first[0], first[1] + 1, first[1] + 4, first[2] + 3
    desc[wrong_system, 0] = B
    desc[wrong_j, 1] = 6
    desc[wrong_q, 2] = 3
    desc[wrong_span, 0] = 1          # a 300-row copy described as a copy of the 5-atom system
    pos, status = _strain(case, desc=desc)
    bad = [wrong_system, wrong_j, wrong_q, wrong_span]
    assert np.nonzero(status)[0].tolist() == sorted(bad) and set(status[bad].tolist()) == {1}
    for c in range(len(desc)):
        rows = slice(case.copy_ptr[c], case.copy_ptr[c + 1])
        assert (pos[rows] == 123.0).all() if c in bad else np.array_equal(pos[rows], ref[rows])
    # the rows kernel: a group whose copies are of another size than its system, and a column outside 0 .. 5
    S0, L0, C0, asym0, _ = _reduce(case)
    groups = case.call.groups.copy()
    g1 = int(np.nonzero(groups[:, 1] == 1)[0][2])
    groups[g1, 1] = 2                # copies of the 5-atom system handed to the 300-atom system
    S, L, C, asym, status = _reduce(case, groups=groups)
    assert status.tolist() == [0, 0, 3] and np.isnan(C[2]).all() and np.isnan(asym[2])
    assert np.array_equal(C[0], C0[0]) and asym[0] == asym0[0] and np.array_equal(L[0], L0[0])
    assert np.array_equal(S[1][:, groups[g1, 2]], np.full(6, 7.0))   # the refused group wrote nothing: its own column keeps the sentinel
    groups = case.call.groups.copy()
    groups[g1, 2] = 6
    assert _reduce(case, groups=groups)[4].tolist() == [0, 3, 0]


def test_an_input_that_is_not_finite_fails_its_system_alone():
    case = _kernel_case(2)
    S0, L0, C0, asym0, _ = _reduce(case)
    c0 = int(case.call.groups[np.nonzero(case.call.groups[:, 1] == 1)[0][3], 0])   # a strained copy of system 1
    virial = case.virial.copy()
    virial[c0, 4] = np.nan
    f32 = case.f32.copy()
    f32[case.copy_ptr[c0] + 2, 1] = np.inf
    volume = case.volume.copy()
    volume[c0] = 0.0
    for kw in (dict(virial=virial), dict(f32=f32), dict(volume=volume)):
        S, L, C, asym, status = _reduce(case, **kw)
        assert status.tolist() == [0, 2, 0], kw.keys()
        assert np.isnan(C[1]).all() and np.isnan(asym[1])
        for b in (0, 2):
            assert np.array_equal(S[b], S0[b]) and np.array_equal(L[b], L0[b]) and np.array_equal(C[b], C0[b]) and asym[b] == asym0[b]


# ------------------------------------------------------------------------------------------------ the loop, analytic potential
def _pair_eval(pot, pos, cell):
    """elastic_ref.PairPotential in fp64 torch on the device, one copy at a time -> (forces [n,3], virial [6] in the engine's order)"""
    img = _t(pot.images(cell), torch.float64)
    d = pos[None, :, None, :] + img[None, None, :, :] - pos[:, None, None, :]
    r = torch.sqrt((d * d).sum(-1))
    keep = (r > 1e-9) & (r < pot.rc)
    rs = torch.where(keep, r, torch.ones_like(r))
    m = 1.0 - torch.exp(-pot.a * (rs - pot.r0))
    u = 1.0 - (rs / pot.rc) ** 2
    de = (2.0 * pot.D * m * pot.a * (1.0 - m)) * u ** 4 + (pot.D * (m * m - 1.0)) * 4.0 * u ** 3 * (-2.0 * rs / pot.rc ** 2)
    g = (torch.where(keep, de, torch.zeros_like(de)) / rs)[..., None] * d
    w = -0.5 * torch.einsum('ijma,ijmb->ab', g, d)
    return g.sum((1, 2)), torch.stack([w[0, 0], w[1, 1], w[2, 2], w[0, 1], w[1, 2], w[2, 0]])


class _PairForces:
    """The pair potential behind the call interface of batch.BatchForces over the slots of an elastic plan: the engine's fp32
    forces and fp64 virial are zero, the potential's forces go through the extra slot and its virial through `virial_extra`.
    Each copy is evaluated on its own, in its slot's strained cell, so its results do not depend on what else is in the call."""

    def __init__(self, plan, n):
        self.plan, self.n, self.pot = plan, np.asarray(n, np.int64), elastic_ref.PairPotential()
        self.engine = SimpleNamespace(dev=torch.device(DEV))
        self.n_force_calls = 0
        self.virial_extra = None

    def __call__(self, pos, ids=None, **kw):
        ids = np.asarray(ids, np.int64)
        seg = np.concatenate([[0], np.cumsum(self.n[self.plan.slot_system[ids]])])
        res = [_pair_eval(self.pot, pos[int(seg[c]):int(seg[c + 1])], self.plan.slot_cells[s]) for c, s in enumerate(ids)]
        self.n_force_calls += 1
        self.virial_extra = torch.stack([r[1] for r in res]).contiguous()
        g = SimpleNamespace(seg_ptr=_t(seg, torch.int32), seg_ptr_host=seg)
        out = dict(forces=torch.zeros(len(pos), 3, dtype=torch.float32, device=pos.device),
                   virial_per_system=torch.zeros(len(ids), 6, dtype=torch.float64, device=pos.device))
        return g, out, torch.cat([r[0] for r in res]).contiguous(), None


def _pair_systems():
    rng = np.random.default_rng(8)
    cells = [np.array([[4.1, 0.0, 0.0], [0.7, 3.8, 0.0], [0.4, -0.5, 4.4]]), 4.3 * np.eye(3) + rng.normal(0.0, 0.2, (3, 3)),
             np.array([[5.0, 0.3, 0.0], [0.0, 4.6, 0.2], [0.1, 0.0, 4.8]])]
    frac = [np.array([[0.2, 0.3, 0.25]]), rng.uniform(0.05, 0.95, (3, 3)), rng.uniform(0.05, 0.95, (5, 3))]
    return [1, 3, 5], [f @ c for f, c in zip(frac, cells)], cells


def _pair_loop(which, nfree, budget):
    from sevennet_amd.elastic import elastic_loop, plan_elastic
    n, pos, cells = ([a[b] for b in which] for a in _pair_systems())
    plan = plan_elastic(n, np.stack(cells), DELTA, nfree, budget)
    return elastic_loop(_PairForces(plan, n), plan, np.concatenate(pos), n) + (plan,)


@pytest.mark.parametrize('nfree', [2, 4])
def test_loop_equals_the_restatement_on_a_pair_potential_whatever_the_packing(nfree):
    """elastic_ref driven by the same potential at the same copies: the strained positions and cells have the same bits, so the
    potential's results do too, and S and L are within the bound of test_kernels_equal_the_restatement"""
    n, pos, cells = _pair_systems()
    S, L, C, asym, status, info, plan = _pair_loop([0, 1, 2], nfree, 10 ** 6)
    assert len(plan.calls) == 1 and status.tolist() == [0, 0, 0]
    pot = elastic_ref.PairPotential()
    for b in range(3):
        def fn(p, c):
            f, w = _pair_eval(pot, _t(p, torch.float64), c)
            return f.cpu().numpy(), elastic_ref.stress_of(w.cpu().numpy(), None, abs(np.linalg.det(c)))
        S_ref, L_ref = elastic_ref.stress_strain(fn, pos[b], cells[b], DELTA, nfree)
        smax = max(np.abs(fn(elastic_ref.strained(pos[b], j, q, DELTA), elastic_ref.strained(cells[b], j, q, DELTA))[1]).max()
                   for j in range(6) for q in (-2, 2))
        lmax = np.abs(L_ref).max() * 2 * DELTA + np.abs(fn(pos[b], cells[b])[0]).max()
        c_w = {2: 1.0, 4: 1.5}[nfree]
        s_tol, l_tol = 8 * EPS * c_w * smax / DELTA, 8 * EPS * c_w * lmax / DELTA
        C_ref, asym_ref = elastic_ref.finish(S_ref)
        print(f'nfree {nfree}, system {b}: max |dS| {np.abs(S[b] - S_ref).max():.3e} (bound {s_tol:.3e}), max |dL| {np.abs(L[b] - L_ref).max():.3e} '
              f'(bound {l_tol:.3e}), max |S| {np.abs(S_ref).max():.3e}, asymmetry {asym[b]:.3e}')
        assert np.abs(S[b] - S_ref).max() <= s_tol and np.abs(L[b] - L_ref).max() <= l_tol
        assert np.abs(C[b] - C_ref).max() <= s_tol and abs(asym[b] - asym_ref) <= 2 * s_tol and np.array_equal(C[b], C[b].T)
        # against the numpy form of the potential, whose sums run in another order: at most 1e4 pair terms of the order 1 each,
        # so 1e4 x 2^-53 = 1e-12 per stress or force, times 1.5 / delta
        S_np, L_np = elastic_ref.stress_strain(pot.eval_fn(), pos[b], cells[b], DELTA, nfree)
        assert np.abs(S[b] - S_np).max() <= 1e-9 and np.abs(L[b] - L_np).max() <= 1e-9
    copies = 3 * (6 * nfree + 1)
    assert info == dict(n_force_calls=1, copies_evaluated=copies, launches=3)
    # one item per call: the same bits
    S1, L1, C1, asym1, _, info1, plan1 = _pair_loop([0, 1, 2], nfree, 1)
    assert len(plan1.calls) == 3 * 7 and all(len(c.groups) + len(c.base) == 1 for c in plan1.calls)
    assert info1 == dict(n_force_calls=21, copies_evaluated=copies, launches=21 + 18 + 1)
    # a budget between the two
    S2, L2, C2, asym2, _, info2, plan2 = _pair_loop([0, 1, 2], nfree, 9 * nfree)
    assert 1 < len(plan2.calls) < 21 and info2['n_force_calls'] == len(plan2.calls) and info2['copies_evaluated'] == copies
    for x, y in ((S1, S), (S2, S), (C1, C), (C2, C), (asym1, asym), (asym2, asym)):
        assert np.array_equal(x, y)
    for b in range(3):
        assert np.array_equal(L1[b], L[b]) and np.array_equal(L2[b], L[b])
    # a system alone: the same bits as inside the batch
    Sa, La, Ca, asyma, _, infoa, _ = _pair_loop([1], nfree, 10 ** 6)
    assert np.array_equal(Sa[0], S[1]) and np.array_equal(La[0], L[1]) and np.array_equal(Ca[0], C[1]) and asyma[0] == asym[1]
    assert infoa['copies_evaluated'] == 6 * nfree + 1


# ------------------------------------------------------------------------------------------------ the driver on a model
F_TOL = 1e-4     # the force tolerance of test_batch_gpu.test_batch_against_the_fp64_oracle for this engine (eV/A)
# The engine-versus-oracle stress tolerance: four times the worst |sigma_engine - sigma_oracle| over the copies of these tests
# (test_stress_tolerance_covers_the_copies measures it: S_TOL_MEASURED eV/A^3 on an MI355X); the factor 4 covers the spread between
# boxes and the order of summation.
S_TOL_MEASURED = 3.706e-08
S_TOL = 4 * S_TOL_MEASURED
C_W = {2: 1.0, 4: 1.5}   # the sums of the stencil's |weights|


def model_systems():
    """[(types, positions, cell, pbc)]: the 2-atom primitive diamond cell with its displaced atom, the rattled triclinic
    two-species 8-atom cell, the perfect 8-atom cubic diamond cell"""
    from sevennet_amd.neighbor import diamond_cubic
    sys2 = _systems(2)
    pos, cell = diamond_cubic(5.431, (1, 1, 1))
    return [sys2[2], sys2[1], (np.zeros(8, np.int64), pos, cell, [True] * 3)]


def _args(systems):
    return ([np.array(Z)[s[0]] for s in systems], [s[1] for s in systems], np.stack([s[2] for s in systems]),
            np.array([s[3] for s in systems]))


@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd, orc=oracle_model(cfg, sd), cache={})


def _oracle_eval(model, types):
    """eval_fn of elastic_ref on the fp64 oracle (forces, ASE-Voigt stress from its `virial`), memoised by the inputs' bits: the
    copies of nfree 2 are among those of nfree 4, and several tests read them"""
    from sevennet_amd.neighbor import neighbor_list

    def fn(pos, cell):
        key = (types.tobytes(), np.asarray(pos).tobytes(), np.asarray(cell).tobytes())
        if key not in model.cache:
            ei, ev, _ = neighbor_list(pos, cell, [True] * 3, model.calc.cutoff)
            out = model.orc.forward(types, ei, ev)
            model.cache[key] = (out['forces'].detach().numpy().copy(),
                                elastic_ref.stress_of(out['virial'].detach().numpy().astype(np.float64).reshape(6), None, abs(np.linalg.det(cell))))
        return model.cache[key]
    return fn


@pytest.fixture(scope='module')
def runs(model):
    """elastic_many for both nfree, once"""
    systems = model_systems()
    out = {}
    for nfree in (2, 4):
        res = model.calc.elastic_many(*_args(systems), delta=DELTA, nfree=nfree)
        out[nfree] = (res, dict(model.calc.elastic_info))
    return systems, out


def test_stress_tolerance_covers_the_copies(model):
    """the measurement behind S_TOL: the engine's stresses (compute_many) against the oracle's on every copy the driver tests
    evaluate (three systems, six patterns, q = -2 .. 2)"""
    systems = model_systems()
    worst, biggest = 0.0, 0.0
    for b, (types, pos, cell, pbc) in enumerate(systems):
        copies = [(j, q) for j in range(6) for q in (-2, -1, 1, 2)] + [(0, 0)]
        p = [elastic_ref.strained(pos, j, q, DELTA) for j, q in copies]
        c = [elastic_ref.strained(cell, j, q, DELTA) for j, q in copies]
        got = model.calc.compute_many([np.array(Z)[types]] * len(copies), p, np.stack(c), np.ones((len(copies), 3), bool))
        fn = _oracle_eval(model, np.asarray(types, np.int64))
        err = max(np.abs(r['stress'] - fn(x, y)[1]).max() for r, x, y in zip(got, p, c))
        f_err = max(np.abs(r['forces'] - fn(x, y)[0]).max() for r, x, y in zip(got, p, c))
        biggest = max(biggest, max(np.abs(r['stress']).max() for r in got))
        print(f'system {b}: max |sigma_engine - sigma_oracle| {err:.3e} eV/A^3, max |F_engine - F_oracle| {f_err:.3e} eV/A over {len(copies)} copies')
        worst = max(worst, err)
    print(f'worst {worst:.3e} eV/A^3 (S_TOL {S_TOL}), largest |sigma| {biggest:.3e}')
    assert worst <= S_TOL


@pytest.mark.parametrize('nfree', [2, 4])
def test_tensors_against_the_fp64_oracle(model, runs, nfree):
    """|S - S_oracle| <= c S_TOL / delta and |L - L_oracle| <= c F_TOL / delta, c = 1 (nfree 2) or 1.5 (nfree 4): the sums of the
    stencil weights times the engine's stress and force tolerances"""
    systems, out = runs
    res, info = out[nfree]
    c = C_W[nfree]
    assert info == dict(n_force_calls=1, copies_evaluated=3 * (6 * nfree + 1), launches=3)   # everything fits one call
    for b, (types, pos, cell, pbc) in enumerate(systems):
        fn = _oracle_eval(model, np.asarray(types, np.int64))
        S_ref, L_ref = elastic_ref.stress_strain(fn, pos, cell, DELTA, nfree)
        C_ref, asym_ref = elastic_ref.finish(S_ref)
        r = res[b]
        n = len(types)
        L = r['internal_strain'].transpose(2, 0, 1).reshape(6, 3 * n)
        s_err, l_err = np.abs(r['stress_strain'] - S_ref).max(), np.abs(L - L_ref).max()
        print(f'nfree {nfree}, system {b} (n {n}): max |dS| {s_err:.3e} eV/A^3 (bound {c * S_TOL / DELTA:.3e}), max |dL| {l_err:.3e} eV/A '
              f'(bound {c * F_TOL / DELTA:.3e}), max |S| {np.abs(S_ref).max():.3e}, max |L| {np.abs(L_ref).max():.3e}, asymmetry '
              f'{r["asymmetry"]:.3e} (oracle {asym_ref:.3e}), |sigma_0| {np.abs(r["stress"]).max():.3e}, fmax {r["fmax"]:.3e}')
        assert r['status'] == 'ok'
        assert s_err <= c * S_TOL / DELTA and l_err <= c * F_TOL / DELTA
        assert np.array_equal(r['elastic_tensor'], r['elastic_tensor'].T)
        assert np.array_equal(r['elastic_tensor'], (r['stress_strain'] + r['stress_strain'].T) * 0.5)
        assert r['asymmetry'] == np.abs(r['stress_strain'] - r['stress_strain'].T).max()
        assert r['internal_strain'].shape == (n, 3, 6) and r['fmax'] == np.abs(r['forces']).max()
        m = elastic_ref.moduli(r['elastic_tensor'])
        assert np.allclose(list(r['bulk_modulus'].values()), m['bulk'], rtol=1e-12, atol=0)
        assert np.allclose(list(r['shear_modulus'].values()), m['shear'], rtol=1e-12, atol=0)
        assert r['stable'] == bool((np.linalg.eigvalsh(r['elastic_tensor']) > 0).all())
    # the perfect cubic cell: three independent constants, and internal strain in the shear columns only
    C = res[2]['elastic_tensor']
    tol = 2 * c * S_TOL / DELTA
    c11, c12, c44 = C[0, 0], C[0, 1], C[3, 3]
    print(f'cubic cell: C11 {c11:.5f}, C12 {c12:.5f}, C44 {c44:.5f} eV/A^3; tolerance {tol:.3e}')
    assert max(abs(C[1, 1] - c11), abs(C[2, 2] - c11), abs(C[0, 2] - c12), abs(C[1, 2] - c12), abs(C[4, 4] - c44), abs(C[5, 5] - c44)) <= tol
    off = C.copy()
    off[:3, :3] = 0.0
    off[np.arange(3, 6), np.arange(3, 6)] = 0.0
    assert np.abs(off).max() <= tol
    lam = res[2]['internal_strain']
    assert np.abs(lam[:, :, :3]).max() <= c * F_TOL / DELTA and np.abs(lam[:, :, 3:]).max() > c * F_TOL / DELTA


# ------------------------------------------------------------------------------------------------ relaxed ions
RELAX_FMAX = (2e-4, 2e-3)   # eV/A, per system: see `relaxed`
MIN_DISTANCE = 1.0          # A


def _closest_pair(pos, cell):
    from sevennet_amd.neighbor import neighbor_list
    return float(np.linalg.norm(neighbor_list(pos, cell, [True] * 3, 5.0)[1], axis=1).min())


@pytest.fixture(scope='module')
def relaxed(model):
    """The first two systems with their ions relaxed at fixed cells, and elastic_many(relax_ions=True) on them.

    The 2-atom cell is relaxed to 2e-4 eV/A.  The rattled 8-atom cell is relaxed to 2e-3 eV/A only (81 steps, closest pair 1.74 A):
    the random-weight model has no core repulsion, and below 1e-3 eV/A FIRE walks that cell into a state where three pairs of atoms
    sit on top of each other (263 steps and more, closest pair 4e-6 A, energy 0.089 instead of 0.66 eV).  There the unit vector of an
    edge amplifies fp32 rounding by 1 / r = 2.5e5 and the engine's forces are up to 2e-3 eV/A off the oracle's, equal and opposite
    within each merged pair, while its energy still has the oracle's derivative: a geometry outside the engine's force tolerance,
    and no crystal.  The comparison below holds at any positions; the test asserts the closest pair stays above MIN_DISTANCE."""
    systems = model_systems()[:2]
    rel = [model.calc.relax_many(*_args([s]), fmax=f, steps=2000)[0] for s, f in zip(systems, RELAX_FMAX)]
    systems = [(s[0], r['positions'], s[2], s[3]) for s, r in zip(systems, rel)]
    res = model.calc.elastic_many(*_args(systems), delta=DELTA, nfree=2, relax_ions=True)
    return systems, rel, res, dict(model.calc.elastic_info)


@pytest.mark.parametrize('b', [0, 1])
def test_relaxed_ions_against_the_oracle_by_the_same_formula(model, relaxed, b):
    """elastic_ref (oracle forces and stresses, the same copies, the same formula), in two steps that hold for any structure and
    one that needs a stiff one.
      1. What enters the formula is within the engine's tolerances of the oracle's: |dS| <= S_TOL / delta, |dL| <= F_TOL / delta,
         |dPhi| <= F_TOL / ion_delta (nfree 2), elementwise; hence the eigenvalues of Phi off the translations within 3n F_TOL /
         ion_delta of the oracle's (Weyl, with 3n max |dPhi| above the spectral norm).
      2. The driver applies the formula exactly: where the status is 'ok', elastic_ref.relaxed on the S, L and Phi it returns gives
         its S_rel but for fp64 rounding (an inverse of condition number below 1e4 here: 1e-9 of the correction is ample), and the
         smallest eigenvalue is above the Hessian's asymmetry; where it is 'singular', that eigenvalue is at or below it, the
         relaxed tensor is NaN and the clamped one is not.
      3. End to end.  S_rel = S - L Phi+ L^T / V; with M = Phi+ L^T (the oracle's) the first-order error of entry (i,j) is at most
             S_TOL / delta + (F_TOL / delta) (|M|_1i + |M|_1j) / V + (F_TOL / ion_delta) |M|_1i |M|_1j / V
         with |M|_1i the sum of |M| over column i.  Higher orders come through (1 - x)^-1 with x = 3n |dPhi| max |Phi+|, a factor
         of at most 1.25 where x <= 0.2.  That holds for the 2-atom cell (asserted); where a structure has a mode softer than what
         the force tolerance resolves at this ion_delta no such bound exists, and steps 1 and 2 are what is asserted."""
    systems, rel, res, info = relaxed
    ion_delta = 0.01
    n_at = [len(s[0]) for s in systems]
    assert info['copies_evaluated'] == sum(13 + 6 * n + 1 for n in n_at)
    types, pos, cell, pbc = systems[b]
    closest = _closest_pair(pos, cell)
    fn = _oracle_eval(model, np.asarray(types, np.int64))
    ref = elastic_ref.elastic(fn, pos, cell, DELTA, 2, relax_ions=True, ion_delta=ion_delta)
    r, V, n = res[b], abs(np.linalg.det(cell)), len(types)
    L = r['internal_strain'].transpose(2, 0, 1).reshape(6, 3 * n)
    plus = elastic_ref.pseudo_inverse(ref['hessian'])
    q = np.linalg.svd(np.eye(3 * n) - elastic_ref.translations(n) @ elastic_ref.translations(n).T)[0][:, :3 * n - 3]
    lam_ref = np.linalg.eigvalsh(q.T @ ref['hessian'] @ q)
    M1 = np.abs(plus @ ref['L'].T).sum(0)
    x = 3 * n * (F_TOL / ion_delta) * np.abs(plus).max()
    tol = 1.25 * (S_TOL / DELTA + (F_TOL / DELTA) * (M1[:, None] + M1[None, :]) / V + (F_TOL / ion_delta) * np.outer(M1, M1) / V)
    err = np.abs(r['stress_strain'] - ref['stress_strain'])
    print(f'system {b}: status {r["status"]}, closest pair {closest:.3f} A, max |dS_rel| {err.max():.3e} (bounds {tol.min():.3e} .. {tol.max():.3e}, x {x:.3e}), '
          f'max |dS| {np.abs(r["stress_strain_clamped"] - ref["stress_strain_clamped"]).max():.3e} (bound {S_TOL / DELTA:.3e}), max |dL| '
          f'{np.abs(L - ref["L"]).max():.3e} (bound {F_TOL / DELTA:.1e}), max |dPhi| {np.abs(r["hessian"] - ref["hessian"]).max():.3e} (bound '
          f'{F_TOL / ion_delta:.1e}), max |d lambda| {np.abs(r["ion_eigenvalues"] - lam_ref).max():.3e}, smallest ion eigenvalue '
          f'{r["ion_eigenvalues"][0]:.3e} (oracle {lam_ref[0]:.3e}), hessian asymmetry {r["hessian_asymmetry"]:.3e}, fmax {r["fmax"]:.3e}, relaxed in '
          f'{rel[b]["n_steps"]} steps')
    assert rel[b]['converged'] and closest > MIN_DISTANCE
    assert np.abs(r['stress_strain_clamped'] - ref['stress_strain_clamped']).max() <= S_TOL / DELTA
    assert np.abs(L - ref['L']).max() <= F_TOL / DELTA and np.abs(r['hessian'] - ref['hessian']).max() <= F_TOL / ion_delta
    assert len(r['ion_eigenvalues']) == 3 * n - 3 and np.abs(r['ion_eigenvalues'] - lam_ref).max() <= 3 * n * F_TOL / ion_delta
    assert np.isfinite(r['elastic_tensor_clamped']).all()
    if r['status'] == 'ok':
        again = elastic_ref.relaxed(r['stress_strain_clamped'], L, r['hessian'], V)
        corr = np.abs(again - r['stress_strain_clamped']).max()
        print(f'  the formula applied again: {np.abs(again - r["stress_strain"]).max():.3e} (correction {corr:.3e})')
        assert np.abs(again - r['stress_strain']).max() <= 1e-9 * corr
        assert r['ion_eigenvalues'][0] > r['hessian_asymmetry']
        assert np.array_equal(r['elastic_tensor'], r['elastic_tensor'].T)
        assert np.array_equal(r['elastic_tensor'], (r['stress_strain'] + r['stress_strain'].T) * 0.5)
        if x <= 0.2:
            assert (err <= tol).all()
    else:
        assert r['status'] == 'singular' and r['ion_eigenvalues'][0] <= r['hessian_asymmetry']
        assert np.isnan(r['elastic_tensor']).all() and np.isnan(r['stress_strain']).all() and not r['stable']
    if b == 0:
        assert r['status'] == 'ok' and x <= 0.2


BF_DELTA, BF_ION_DELTA, BF_FMAX = 3e-4, 1e-3, 2e-5


def test_relaxed_ions_against_brute_force_relaxation(model):
    """the 2-atom cell: its 12 strained copies relaxed in one relax_many batch and the central differences of their stresses.
    Bound: S_TOL / delta for the stresses, and max |L^T Phi+| fmax_reached / (V delta) for the ions' distance from equilibrium
    (a residual force f displaces the ions by Phi+ f, which changes sigma by L^T Phi+ f / V, in a difference over 2 delta with
    weights 1/2).

    The steps are small here, for a reason that lies in the structure and not in the method.  In diamond at a = 5.431 A the third
    neighbour shell sits at 4.5030 A, 0.003 A outside the radius 4.5 A at which the model's XPLOR envelope starts to switch, and
    the second derivative of that envelope jumps there.  A second derivative of the energy (an elastic constant, a force
    constant) is then one-sided, and steps that carry the shell across the radius give central differences that average the two
    sides: the formula and the brute-force route average them differently and disagree by an amount that does not go down with
    delta (measured on an MI355X: 2.7e-3, 2.6e-3, 2.4e-3 eV/A^3 on C44 at delta = 5e-3, 2.5e-3, 1.25e-3, where the correction itself
    is 1.4e-2).  delta 4.5 A < 0.003 A and ion_delta < 0.003 A keep every copy on one side."""
    types, pos, cell, pbc = model_systems()[0]
    z = np.array(Z)[types]
    assert BF_DELTA * 4.503 < 0.003 and BF_ION_DELTA < 0.003
    base = model.calc.relax_many([z], [pos], cell[None], np.ones((1, 3), bool), fmax=BF_FMAX, steps=2000)[0]
    pos = base['positions']
    r = model.calc.elastic_many([z], [pos], cell[None], np.ones((1, 3), bool), delta=BF_DELTA, nfree=2, relax_ions=True,
                                ion_delta=BF_ION_DELTA)[0]
    copies = [(j, q) for j in range(6) for q in (-1, 1)]
    p = [elastic_ref.strained(pos, j, q, BF_DELTA) for j, q in copies]
    c = np.stack([elastic_ref.strained(cell, j, q, BF_DELTA) for j, q in copies])
    out = model.calc.relax_many([z] * 12, p, c, np.ones((12, 3), bool), fmax=BF_FMAX, steps=2000)
    fmax = max(np.abs(o['forces']).max() for o in out)
    S_bf = np.stack([elastic_ref.difference([out[2 * j]['stress'], out[2 * j + 1]['stress']], 2, BF_DELTA) for j in range(6)], 1)
    V = abs(np.linalg.det(cell))
    L = r['internal_strain'].transpose(2, 0, 1).reshape(6, 6)
    gain = np.abs(L @ elastic_ref.pseudo_inverse(r['hessian'])).max()
    t_stress, t_ions = S_TOL / BF_DELTA, gain * fmax / (V * BF_DELTA)
    err = np.abs(r['stress_strain'] - S_bf).max()
    corr = np.abs(r['elastic_tensor'] - r['elastic_tensor_clamped']).max()
    print(f'2-atom cell: max |S_rel - brute force| {err:.3e} eV/A^3 (bound {t_stress + t_ions:.3e} = {t_stress:.3e} stresses + {t_ions:.3e} ions, '
          f'fmax reached {fmax:.3e}, base {np.abs(base["forces"]).max():.3e}); correction {corr:.3e}; all converged '
          f'{all(o["converged"] for o in out)} in at most {max(o["n_steps"] for o in out)} steps; status {r["status"]}')
    assert r['status'] == 'ok' and base['converged'] and all(o['converged'] for o in out)
    assert err <= t_stress + t_ions
    assert corr > t_stress + t_ions   # the correction is seen to be in


# ------------------------------------------------------------------------------------------------ surfaces
class _ReadOnlyAtoms(_Atoms):
    def set_positions(self, pos):
        raise AssertionError('elastic_many_atoms writes nothing back')


def test_surfaces_and_validation(model, runs):
    systems, out = runs
    res, _ = out[2]
    args = _args(systems)
    many = model.calc.compute_many(*args)
    extra = {'stress_strain', 'elastic_tensor', 'asymmetry', 'internal_strain', 'fmax', 'compliance', 'bulk_modulus', 'shear_modulus',
             'youngs_modulus', 'poisson_ratio', 'stable', 'status'}
    for r, one in zip(res, many):   # the batch-versus-single tolerances of test_vib_gpu
        assert set(r) == set(one) | extra
        assert abs(r['energy'] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6 and r['free_energy'] == r['energy']
        assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max())
        assert np.abs(r['energies'] - one['energies']).max() <= 1e-6 * max(1.0, np.abs(one['energies']).max())
        assert r['num_edges'] == one['num_edges']
        assert np.allclose(r['stress'], one['stress'], rtol=0, atol=1e-5 * max(1e-3, np.abs(one['stress']).max()))
        assert set(r['bulk_modulus']) == set(r['shear_modulus']) == {'voigt', 'reuss', 'hill'}
    again = model.calc.elastic_many(*args, delta=DELTA, nfree=2)
    for x, y in zip(res, again):
        for key in ('stress_strain', 'elastic_tensor', 'internal_strain', 'compliance', 'forces', 'stress'):
            assert np.array_equal(x[key], y[key]), key
        assert x['asymmetry'] == y['asymmetry'] and x['energy'] == y['energy'] and x['bulk_modulus'] == y['bulk_modulus']
    fresh = _args(model_systems())
    assert all(np.array_equal(a, b) for a, b in zip(args[1], fresh[1])) and np.array_equal(args[2], fresh[2])   # the caller's arrays
    atoms = [_ReadOnlyAtoms(z, p, c, pb) for z, p, c, pb in zip(*args)]
    got = model.calc.elastic_many_atoms(atoms, delta=DELTA, nfree=2)
    for x, y in zip(res, got):
        assert np.array_equal(x['stress_strain'], y['stress_strain']) and np.array_equal(x['internal_strain'], y['internal_strain'])
    # a small budget: several calls; each run is within S_TOL / delta of the oracle's S, so the two are within twice that
    small = model.calc.elastic_many(*args, delta=DELTA, nfree=2, max_atoms_per_call=20)
    assert model.calc.elastic_info['n_force_calls'] > 1 and model.calc.elastic_info['copies_evaluated'] == 39
    for x, y in zip(res, small):
        assert np.abs(x['stress_strain'] - y['stress_strain']).max() <= 2 * S_TOL / DELTA
    mol, slab = _systems(2)[4], _systems(2)[3]
    for bad, name in ((mol, 'molecule'), (slab, 'slab')):
        with pytest.raises(ValueError, match='system 1: an elastic tensor needs a fully periodic system'):
            model.calc.elastic_many(*_args([systems[0], bad]))
    with pytest.raises(ValueError, match='nfree'):
        model.calc.elastic_many(*args, nfree=3)
    with pytest.raises(ValueError, match='delta'):
        model.calc.elastic_many(*args, delta=0.0)


def test_d3_share_on_the_device_term_and_the_host_term_is_refused(model, runs):
    """S(model + D3) - S(model) is the central difference of the D3 stresses alone but for fp64 rounding: the model's virials are
    the same bits in both runs (the same copies in the same slots), and each of the two matrices is within 8 x 2^-53 x sum_w
    |weight_w sigma_w| / delta of the exact combination of its stresses (test_kernels_equal_the_restatement); the restatement's own
    S adds as much again, and the D3 term's virial against D3Calculator's stress (other sums, a division by the volume) another
    such share: 40 x 2^-53 x max |sigma| / delta with sigma the summed stresses.  The same for L with the forces."""
    from sevennet_amd.d3 import D3Calculator, SevenNetD3Calculator
    systems, out = runs
    plain, _ = out[2]
    calc = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    args = _args(systems)
    with pytest.raises(ValueError, match="d3_term='host'"):
        calc.elastic_many(*args, d3_term='host')
    both = calc.elastic_many(*args, d3_term='device', delta=DELTA, nfree=2)
    assert calc.elastic_info == dict(n_force_calls=1, copies_evaluated=39, launches=3)
    d3 = D3Calculator(**D3_CUT)
    for b, (h, p) in enumerate(zip(both, plain)):
        z, pos, cell, pbc = args[0][b], args[1][b], args[2][b], args[3][b]
        alone = d3.compute(z, pos, cell, pbc)
        assert h['status'] == 'ok' and abs(h['energy'] - (p['energy'] + alone['energy'])) <= 1e-12 * abs(h['energy'])
        assert np.abs(h['stress'] - (p['stress'] + alone['stress'])).max() <= 1e-12 * max(1.0, np.abs(h['stress']).max())

        def fn(q, c):
            r = d3.compute(z, q, c, pbc)
            return r['forces'], r['stress']
        S_ref, L_ref = elastic_ref.stress_strain(fn, pos, cell, DELTA, 2)
        n = len(z)
        share = h['stress_strain'] - p['stress_strain']
        l_share = (h['internal_strain'] - p['internal_strain']).transpose(2, 0, 1).reshape(6, 3 * n)
        smax = np.abs(h['stress']).max() + np.abs(h['stress_strain']).max() * 2 * DELTA   # (stresses at the strained copies)
        fmax = np.abs(h['forces']).max() + np.abs(h['internal_strain']).max() * 2 * DELTA
        err, tol, l_err, l_tol = np.abs(share - S_ref).max(), 40 * EPS * smax / DELTA, np.abs(l_share - L_ref).max(), 40 * EPS * fmax / DELTA
        print(f'system {b}: max |S(model + D3) - S(model) - S(D3)| {err:.3e} (bound {tol:.3e}), max |S(D3)| {np.abs(S_ref).max():.3e}; '
              f'the same for L {l_err:.3e} (bound {l_tol:.3e}), max |L(D3)| {np.abs(L_ref).max():.3e}')
        assert err <= tol and l_err <= l_tol
        assert np.abs(S_ref).max() > 0 and not np.array_equal(h['stress_strain'], p['stress_strain'])   # the D3 share is in
