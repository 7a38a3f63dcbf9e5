"""GPU: batched supercell phonons -- the four kernels against their fp64 restatement (phonon_ref) on random data, the loop on a
diatomic chain whose dispersion is known in closed form, and the driver and the public surfaces on a model: a rattled two-species
two-atom cell with repeats (2,1,1) and (1,2,3) in one batch, against phonon_ref driven by the fp64 oracle at the same displacements."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import phonon_ref
import vib_ref
from helpers import oracle_model
from test_batch_gpu import Z, _calc
from test_relax_gpu import D3_CUT, DEV, _oracle
from test_vib_gpu import F_TOL, MASS, _MassAtoms, _QuadraticForces

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
DELTA = 0.01
SYMPREC = 1e-5


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


# ------------------------------------------------------------------------------------------------ the kernels
A = 3.9
FCC = np.array([[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]]) * A
TRI_S = np.array([[6.0, 0.3, 0.2], [0.4, 5.8, -0.3], [-0.2, 0.5, 6.2]])    # a reduced triclinic supercell, (3,1,2) of the cell below
# (m, repeats, primitive cell): N = 1, 4, 18, 40 and 300 (more atoms than threads)
KERNEL_SYSTEMS = [(1, (1, 1, 1), np.eye(3) * A), (2, (2, 1, 1), np.diag([3.1, 6.5, 6.9])), (3, (3, 1, 2), TRI_S / np.array([3.0, 1.0, 2.0])[:, None]),
                  (5, (2, 2, 2), FCC), (3, (5, 5, 4), np.eye(3) * 3.0)]
KERNEL_NQ = [1, 2, 3, 2, 2]
B = len(KERNEL_SYSTEMS)


def _layout():
    m = np.array([s[0] for s in KERNEL_SYSTEMS], np.int64)
    N = np.array([s[0] * int(np.prod(s[1])) for s in KERNEL_SYSTEMS], np.int64)
    assert N.tolist() == [1, 4, 18, 40, 300]
    i32, i64 = torch.int32, torch.int64
    p_off, i_off = np.concatenate([[0], np.cumsum(9 * m * N)]), np.concatenate([[0], np.cumsum(m * N)])
    return SimpleNamespace(m=m, N=N, p_off=p_off, i_off=i_off, m_ptr=_t(np.concatenate([[0], np.cumsum(m)]), i32),
                           sc_ptr=_t(np.concatenate([[0], np.cumsum(N)]), i32), off_d=_t(p_off[:-1], i64), ioff_d=_t(i_off[:-1], i64),
                           home_sys=_t(np.repeat(np.arange(B), m), i32))


def _structures(rattle):
    """supercell positions and lattices of the five systems: a random basis repeated exactly (rattle 0: atoms half a supercell apart
    have two or more equally near images) or every supercell atom moved by `rattle` (no ties)"""
    from sevennet_amd.phonon import is_reduced
    rng = np.random.default_rng(21)
    pos, S = [], []
    for m, reps, C in KERNEL_SYSTEMS:
        p, s = phonon_ref.supercell(rng.uniform(0.0, 1.0, (m, 3)) @ C, C, reps)
        assert is_reduced(s)
        pos.append(p + (rng.normal(0.0, rattle, p.shape) if rattle else 0.0))
        S.append(s)
    return pos, S


def _kernel_case(nfree):
    """every copy of the five systems in one call, with random fp32 forces and fp64 extra forces on them"""
    from sevennet_amd.vib import plan_copies
    rng = np.random.default_rng(12)
    lay = _layout()
    plan = plan_copies(lay.N, [np.arange(k) for k in lay.m], nfree, 10 ** 7)
    assert len(plan.calls) == 1
    call = plan.calls[0]
    copy_ptr = np.concatenate([[0], np.cumsum(lay.N[call.desc[:, 0]])])
    n_all = int(copy_ptr[-1])
    return SimpleNamespace(nfree=nfree, lay=lay, call=call, copy_ptr=copy_ptr, f32=rng.normal(0.0, 1.0, (n_all, 3)).astype(np.float32),
                           fx=rng.normal(0.0, 1e-2, (n_all, 3)), masses=[rng.uniform(1.0, 60.0, k) for k in lay.m])


def _rows_and_finish(case, acoustic=True, f32=None, groups=None, p_off=None):
    """snet_ph_rows + snet_ph_finish -> (Phi as written by the rows, Phi after the sum rule: per system [3m,3N]; asr_defect; status)"""
    from sevennet_amd.phonon import ph_finish, ph_rows
    lay = case.lay
    f64, i32 = torch.float64, torch.int32
    phi = torch.full((int(lay.p_off[-1]),), 7.0, dtype=f64, device=DEV)   # (rows are written, not accumulated: the 7.0 must go)
    status = torch.zeros(B, dtype=i32, device=DEV)
    ph_rows(_t(case.f32 if f32 is None else f32, torch.float32), _t(case.fx, f64), _t(case.copy_ptr, i32),
            _t(case.call.groups if groups is None else groups, i32), case.nfree, DELTA, lay.m_ptr, lay.sc_ptr, lay.off_d, phi, status)
    out, asr = torch.full_like(phi, -5.0), torch.full((B,), -5.0, dtype=f64, device=DEV)
    ph_finish(phi, lay.off_d if p_off is None else _t(p_off, torch.int64), lay.m_ptr, lay.sc_ptr, acoustic, status, out, asr)
    torch.cuda.synchronize()
    cut = lambda a: [a.cpu().numpy()[lay.p_off[b]:lay.p_off[b + 1]].reshape(3 * lay.m[b], 3 * lay.N[b]) for b in range(B)]   # noqa: E731
    return cut(phi), cut(out), asr.cpu().numpy(), status.cpu().numpy()


def _restated_rows(case):
    """vib_ref.row on the bits the kernel sees: fp32 forces widened plus the fp64 ones -> per system (Phi, scale)"""
    F = case.f32.astype(np.float64) + case.fx
    lay = case.lay
    out = [(np.zeros((3 * lay.m[b], 3 * lay.N[b])), np.zeros((3 * lay.m[b], 3 * lay.N[b]))) for b in range(B)]
    for j0, b, r in case.call.groups:
        rows = [F[case.copy_ptr[j0 + w]:case.copy_ptr[j0 + w + 1]].reshape(-1) for w in range(case.nfree)]
        out[b][0][r] = vib_ref.row(rows, case.nfree, DELTA)
        out[b][1][r] = sum(wt * np.abs(f) for wt, f in zip(vib_ref.WEIGHTS[case.nfree], rows)) / DELTA
    return out


@pytest.mark.parametrize('nfree', [2, 4])
def test_rows_and_sum_rule_equal_the_restatement(nfree):
    """every element of Phi within 8 x 2^-53 x sum_w |weight_w F_w| / delta (the bound test_vib_gpu derives: at most 8 roundings),
    written over the prefilled buffer; asr_defect and the corrected self terms within the rounding of an N-term ordered sum, N x
    2^-53 x sum_j |Phi|; everything but the self terms copied bit for bit; without `acoustic` the whole of Phi is"""
    case = _kernel_case(nfree)
    raw, fixed, asr, status = _rows_and_finish(case)
    _, plain, asr_plain, _ = _rows_and_finish(case, acoustic=False)
    assert not status.any()
    for b, (want, scale) in enumerate(_restated_rows(case)):
        m, N = int(case.lay.m[b]), int(case.lay.N[b])
        tol = 8 * EPS * scale
        assert (np.abs(raw[b] - want) <= tol).all()
        asr_ref, fixed_ref = phonon_ref.sum_rule(raw[b], m, True)
        col_abs = np.abs(raw[b].reshape(m, 3, N, 3)).sum(2)          # sum_j |Phi[(a,i),(j,k)]|
        sum_tol = N * EPS * col_abs
        d_self = np.array([[np.abs(fixed[b].reshape(m, 3, N, 3)[a, :, a, :] - fixed_ref.reshape(m, 3, N, 3)[a, :, a, :])] for a in range(m)]).reshape(m, 3, 3)
        print(f'nfree {nfree}, system {b} (m {m}, N {N}): max |dPhi| {np.abs(raw[b] - want).max():.3e} (smallest bound {tol.min():.3e}), '
              f'|d asr_defect| {abs(asr[b] - asr_ref):.3e} and max |d self term| {d_self.max():.3e} (bounds from {sum_tol.min():.3e}), '
              f'asr_defect {asr[b]:.6e}')
        assert abs(asr[b] - asr_ref) <= sum_tol.max() and (d_self <= sum_tol).all()
        other = np.ones((m, N), bool)
        other[np.arange(m), np.arange(m)] = False
        sel = np.broadcast_to(other[:, None, :, None], (m, 3, N, 3)).reshape(3 * m, 3 * N)
        assert np.array_equal(fixed[b][sel], raw[b][sel])
        assert np.array_equal(plain[b], raw[b]) and asr_plain[b] == asr[b]
        if N > 1:
            assert np.abs(fixed[b].reshape(m, 3, N, 3).sum(2)).max() <= 2 * sum_tol.max()   # the rule holds afterwards


def test_a_force_that_is_not_finite_fails_its_system_alone():
    case = _kernel_case(2)
    _, good, asr0, _ = _rows_and_finish(case)
    f32 = case.f32.copy()
    j0 = int(case.call.groups[np.nonzero(case.call.groups[:, 1] == 2)[0][4], 0])   # a displaced copy of system 2
    f32[case.copy_ptr[j0] + 11, 1] = np.inf
    _, out, asr, status = _rows_and_finish(case, f32=f32)
    assert status.tolist() == [0, 0, 2, 0, 0]
    assert np.isnan(out[2]).all() and np.isnan(asr[2])
    for b in (0, 1, 3, 4):
        assert np.array_equal(out[b], good[b]) and asr[b] == asr0[b]


def _images(pos, S, lay, i_off=None, symprec=SYMPREC):
    from sevennet_amd.phonon import ph_images
    f64, i32 = torch.float64, torch.int32
    n_pairs = int(lay.i_off[-1])
    base = torch.full((n_pairs, 3), -77, dtype=i32, device=DEV)
    mask = torch.full((n_pairs,), -77, dtype=i32, device=DEV)
    status = torch.zeros(B, dtype=i32, device=DEV)
    S_d = _t(np.stack(S).reshape(B, 9), f64)
    Si_d = _t(np.stack([np.linalg.inv(s) for s in S]).reshape(B, 9), f64)
    pos_d = _t(np.concatenate(pos), f64)
    ph_images(pos_d, lay.sc_ptr, lay.m_ptr, lay.home_sys, S_d, Si_d, lay.ioff_d if i_off is None else _t(i_off, torch.int64), symprec, base,
              mask, status)
    torch.cuda.synchronize()
    return SimpleNamespace(base=base, mask=mask, status=status.cpu().numpy(), S_d=S_d, pos_d=pos_d)


def _image_sets(img, lay, b):
    sl = slice(lay.i_off[b], lay.i_off[b + 1])
    return phonon_ref.mask_to_translations(img.base.cpu().numpy()[sl].reshape(lay.m[b], lay.N[b], 3),
                                           img.mask.cpu().numpy()[sl].reshape(lay.m[b], lay.N[b]))


@pytest.fixture(scope='module')
def brute():
    """the brute-force image sets of the five systems, perfect and rattled, once"""
    out = {}
    lay = _layout()
    for rattle in (0.0, 0.05):
        pos, S = _structures(rattle)
        sets = [phonon_ref.images_brute(pos[b], S[b], int(lay.m[b]), SYMPREC) for b in range(B)]
        # the restatement decides every candidate safely: none within 1e-9 A of the threshold min + symprec
        assert min(s[1] for s in sets) > 1e-9
        out[rattle] = (pos, S, [s[0] for s in sets])
    return out


@pytest.mark.parametrize('rattle', [0.0, 0.05])
def test_image_sets_equal_the_brute_force_sets(brute, rattle):
    pos, S, sets = brute[rattle]
    lay = _layout()
    img = _images(pos, S, lay)
    assert not img.status.any()
    sizes = []
    for b in range(B):
        got = _image_sets(img, lay, b)
        assert {k: sorted(v) for k, v in got.items()} == sets[b], b
        sizes.append(max(len(v) for v in got.values()))
    print(f'rattle {rattle}: most images kept per pair and system {sizes}')
    if rattle == 0.0:
        assert sizes[0] == 1 and sizes[1] == 2 and min(sizes[1:]) >= 2   # every even repeat puts an atom half a supercell away
    else:
        assert sizes == [1] * B


def _dynmat(case, phi, img, q_cart, d_off=None, q_sys=None):
    from sevennet_amd.phonon import ph_dynmat
    lay = case.lay
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    n_q = np.array(KERNEL_NQ, np.int64)
    blocks = np.concatenate([[0], np.cumsum(n_q * 9 * lay.m * lay.m)])
    R = torch.full((int(blocks[-1]), 2), -3.0, dtype=f64, device=DEV)
    D, herm = torch.full_like(R, -3.0), torch.full((int(n_q.sum()),), -3.0, dtype=f64, device=DEV)
    status = torch.zeros(B, dtype=i32, device=DEV)
    w = np.concatenate([1.0 / np.sqrt(ms) for ms in case.masses])
    ph_dynmat(phi, lay.off_d, img.pos_d, lay.sc_ptr, lay.m_ptr, _t(w, f64), img.S_d, img.base, img.mask, lay.ioff_d, _t(np.concatenate(q_cart), f64),
              _t(np.repeat(np.arange(B), n_q) if q_sys is None else q_sys, i32), _t(np.concatenate([[0], np.cumsum(n_q)]), i32),
              _t(blocks[:-1] if d_off is None else d_off, i64), int(lay.m.max()), status, R, D, herm)
    torch.cuda.synchronize()

    def cut(a):
        a = a.cpu().numpy()
        return [(a[blocks[b]:blocks[b + 1], 0] + 1j * a[blocks[b]:blocks[b + 1], 1]).reshape(n_q[b], 3 * lay.m[b], 3 * lay.m[b]) for b in range(B)]
    q0 = np.concatenate([[0], np.cumsum(n_q)])
    return cut(R), cut(D), [herm.cpu().numpy()[q0[b]:q0[b + 1]] for b in range(B)], status.cpu().numpy()


def _q_points():
    rng = np.random.default_rng(33)
    q = [rng.uniform(-0.5, 0.5, (k, 3)) for k in KERNEL_NQ]
    q[1][0] = 0.0                   # Gamma
    q[3][1] = [0.5, 0.0, 0.5]       # a zone-boundary point
    return q


@pytest.mark.parametrize('rattle', [0.0, 0.05])
def test_dynamical_matrices_equal_the_restatement(brute, rattle):
    """R and D within 2^-53 x (8 + 4 max |q . d|) x sum_c |Phi| w_alpha w_beta per element: the roundings of the products and of
    the ordered sum, and the phase argument (an error of 2^-53 |q . d| in the argument moves sin and cos by as much); D equals D^H bit
    for bit; the hermiticity within the two elements' bounds plus the rounding of the modulus"""
    pos, S, sets = brute[rattle]
    case = _kernel_case(2)
    lay = case.lay
    _, fixed, _, _ = _rows_and_finish(case)
    phi = _t(np.concatenate([f.reshape(-1) for f in fixed]), torch.float64)
    img = _images(pos, S, lay)
    q_frac = _q_points()
    q_cart = [phonon_ref.q_cartesian(q_frac[b], KERNEL_SYSTEMS[b][2]) for b in range(B)]
    R, D, herm, status = _dynmat(case, phi, img, q_cart)
    assert not status.any()
    for b in range(B):
        m = int(lay.m[b])
        for k, q in enumerate(q_cart[b]):
            R_ref, D_ref, herm_ref, scale, arg_max = phonon_ref.dynmat(fixed[b], pos[b], S[b], m, case.masses[b], sets[b], q)
            tol = EPS * (8 + 4 * arg_max) * scale
            dR, dD = np.abs(R[b][k] - R_ref), np.abs(D[b][k] - D_ref)
            print(f'rattle {rattle}, system {b} (m {m}, N {lay.N[b]}), q {k}: max |dR| {dR.max():.3e}, max |dD| {dD.max():.3e} (bounds from '
                  f'{tol.min():.3e} to {tol.max():.3e}, max |q.d| {arg_max:.2f}), hermiticity {herm[b][k]:.6e} (restatement {herm_ref:.6e})')
            assert (dR <= tol).all() and (dD <= np.maximum(tol, tol.T)).all()
            assert np.array_equal(D[b][k], D[b][k].conj().T)
            assert abs(herm[b][k] - herm_ref) <= 2 * tol.max() + 4 * EPS * herm_ref
    assert np.abs(R[1][0].imag).max() == 0.0   # Gamma: every phase is 1


def test_descriptors_that_do_not_fit_are_refused_and_the_outputs_left_alone(brute):
    pos, S, sets = brute[0.05]
    case = _kernel_case(2)
    lay = case.lay
    raw0, fixed0, asr0, _ = _rows_and_finish(case)
    # rows: a row index one past the last of system 1; finish: a block of system 3 that ends outside the buffer
    groups = case.call.groups.copy()
    g = int(np.nonzero((groups[:, 1] == 1) & (groups[:, 2] == 0))[0][0])
    groups[g, 2] = 3 * lay.m[1]
    p_off = lay.p_off[:-1].copy()
    p_off[3] = lay.p_off[-1] - 9 * lay.m[3] * lay.N[3] + 1
    raw, fixed, asr, status = _rows_and_finish(case, groups=groups, p_off=p_off)
    assert status.tolist() == [0, 3, 0, 3, 0]
    assert (raw[1][0] == 7.0).all() and np.array_equal(raw[1][1:], raw0[1][1:])
    assert (fixed[3] == -5.0).all() and np.isnan(asr[3]) and np.isnan(fixed[1]).all()
    for b in (0, 2, 4):
        assert np.array_equal(fixed[b], fixed0[b]) and asr[b] == asr0[b]
    # images: the pairs of system 2 placed past the end of the arrays
    good = _images(pos, S, lay)
    i_off = lay.i_off[:-1].copy()
    i_off[2] = lay.i_off[-1] - lay.m[2] * lay.N[2] + 1
    img = _images(pos, S, lay, i_off=i_off)
    assert img.status.tolist() == [0, 0, 3, 0, 0]
    sl = slice(lay.i_off[2], lay.i_off[3])
    assert (img.mask.cpu().numpy()[sl] == -77).all() and (img.base.cpu().numpy()[sl] == -77).all()
    keep = np.ones(int(lay.i_off[-1]), bool)
    keep[sl] = False
    assert np.array_equal(img.mask.cpu().numpy()[keep], good.mask.cpu().numpy()[keep])
    # dynmat: the blocks of system 4 placed so that the last one ends outside R and D; a q-point given to a system that does not own it
    phi = _t(np.concatenate([f.reshape(-1) for f in fixed0]), torch.float64)
    q_cart = [phonon_ref.q_cartesian(q, KERNEL_SYSTEMS[b][2]) for b, q in enumerate(_q_points())]
    R0, D0, herm0, status = _dynmat(case, phi, good, q_cart)
    assert not status.any()
    n_q = np.array(KERNEL_NQ, np.int64)
    blocks = np.concatenate([[0], np.cumsum(n_q * 9 * lay.m * lay.m)])
    d_off = blocks[:-1].copy()
    d_off[4] += 1
    q_sys = np.repeat(np.arange(B), n_q)
    q_sys[1] = 2                                       # the first q-point of system 1 claimed for system 2
    R, D, herm, status = _dynmat(case, phi, good, q_cart, d_off=d_off, q_sys=q_sys)
    assert status.tolist() == [0, 0, 3, 0, 3]
    assert (R[4] == -3.0 - 3.0j).all() and (D[4] == -3.0 - 3.0j).all() and (herm[4] == -3.0).all()
    assert (R[1][0] == -3.0 - 3.0j).all() and (D[1][0] == -3.0 - 3.0j).all() and herm[1][0] == -3.0
    assert np.array_equal(R[1][1], R0[1][1]) and np.array_equal(D[1][1], D0[1][1])
    for b in (0, 2, 3):
        assert np.array_equal(R[b], R0[b]) and np.array_equal(D[b], D0[b]) and np.array_equal(herm[b], herm0[b])


# ------------------------------------------------------------------------------------------------ the loop, analytic potential
CHAIN_N = [2, 3, 4]
CHAIN_Q = [0.0, 0.13, 0.37, 0.5]


def _chain_loop(budget, nfree=2, acoustic=True, max_q_per_call=4096):
    """the chains (n,1,1), n = 2, 3, 4, in one batch: their springs as fp64 matrix-vector products on the device (the stand-in of
    test_vib_gpu behind the call interface of batch.BatchForces)"""
    from sevennet_amd.phonon import phonon_loop
    from sevennet_amd.vib import plan_copies
    pos, cell, masses = phonon_ref.chain_cell()
    sc = [phonon_ref.supercell(pos, cell, (n, 1, 1)) for n in CHAIN_N]
    N = np.array([len(s[0]) for s in sc])
    plan = plan_copies(N, [np.arange(2)] * 3, nfree, budget)
    forces = _QuadraticForces(plan.slot_system, [phonon_ref.chain_hessian(n) for n in CHAIN_N], [s[0] for s in sc])
    q_cart = [phonon_ref.q_cartesian([[q, 0.0, 0.0] for q in CHAIN_Q], cell)] * 3
    out = phonon_loop(forces, plan, np.concatenate([s[0] for s in sc]), N, [2, 2, 2], [masses] * 3, np.stack([s[1] for s in sc]), q_cart,
                      delta=DELTA, acoustic=acoustic, max_q_per_call=max_q_per_call)
    return out, plan


@pytest.mark.parametrize('nfree', [2, 4])
def test_loop_meets_the_closed_form_of_the_chain_whatever_the_packing(nfree):
    """the potential is harmonic, so the central differences are exact up to rounding over delta: eigenvalues within 1e-9 of the
    largest (2^-53 |F| / delta is of the order 1e-14 here); Phi bit for bit the same from one call, from one item per call and from
    a budget between the two, and from D(q) launches of one q-point each"""
    (phi, asr, D, herm, status, info), plan = _chain_loop(10 ** 6, nfree)
    assert len(plan.calls) == 1 and status.tolist() == [0, 0, 0]
    for b, n in enumerate(CHAIN_N):
        assert phi[b].shape == (2, 2 * n, 3, 3) and D[b].shape == (4, 6, 6)
        K_home = phonon_ref.chain_hessian(n)[:6].reshape(2, 3, 2 * n, 3).transpose(0, 2, 1, 3)
        worst = 0.0
        for k, q in enumerate(CHAIN_Q):
            lam = np.linalg.eigvalsh(D[b][k])
            want = np.sort(np.concatenate([np.zeros(4), phonon_ref.chain_closed_form(q)]))
            worst = max(worst, np.abs(lam - want).max() / want.max())
            assert np.abs(lam - want).max() <= 1e-9 * want.max()
        print(f'nfree {nfree}, n {n}: max |d lambda| / max lambda {worst:.3e} (bound 1e-9), max |Phi - K| {np.abs(phi[b] - K_home).max():.3e}, '
              f'asr_defect {asr[b]:.3e}, hermiticity {herm[b].max():.3e}')
        assert np.abs(phi[b] - K_home).max() <= 1e-9 * np.abs(K_home).max()
    copies = 3 * (nfree * 6 + 1)
    assert info == dict(n_force_calls=1, copies_evaluated=copies, launches=5, q_evaluated=12)
    (phi1, asr1, D1, herm1, _, info1), plan1 = _chain_loop(1, nfree, max_q_per_call=1)
    assert len(plan1.calls) == 3 * 7 and info1['n_force_calls'] == 21 and info1['launches'] == 21 + 18 + 2 + 12
    (phi2, _, D2, _, _, info2), plan2 = _chain_loop(40, nfree, max_q_per_call=5)
    assert 1 < len(plan2.calls) < 21 and info2['launches'] == len(plan2.calls) + sum(1 for c in plan2.calls if len(c.groups)) + 2 + 3
    for b in range(3):
        assert np.array_equal(phi1[b], phi[b]) and np.array_equal(phi2[b], phi[b]) and asr1[b] == asr[b]
        assert np.array_equal(D1[b], D[b]) and np.array_equal(D2[b], D[b]) and np.array_equal(herm1[b], herm[b])


# ------------------------------------------------------------------------------------------------ the driver on a model
CELL = np.array([[2.8, 0.0, 0.0], [0.2, 5.5, 0.0], [0.1, 0.3, 8.1]])
REPEATS = [(2, 1, 1), (1, 2, 3)]
Q_PATH = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.21, -0.4, 0.33], [0.0, 0.5, 1.0 / 3.0]])
MESH = (2, 1, 2)
TEMPS = [0.0, 300.0]


def model_systems():
    """[(types, positions, cell)]: the same rattled two-species two-atom cell twice (it gets two different supercells)"""
    rng = np.random.default_rng(5)
    pos = np.array([[0.0, 0.0, 0.0], [1.4, 2.7, 4.0]]) + rng.normal(0.0, 0.08, (2, 3))
    return [(np.array([0, 1]), pos.copy(), CELL.copy()) for _ in REPEATS]


def _ph_args(systems):
    numbers = [np.array(Z)[s[0]] for s in systems]
    return (numbers, [s[1] for s in systems], [np.array([MASS[z] for z in zs]) for zs in numbers], np.stack([s[2] for s in systems]),
            [True] * 3)


@pytest.fixture(scope='module')
def model():
    from sevennet_amd.shapes import mini_sevennet_0_config
    calc, cfg, sd = _calc(mini_sevennet_0_config())
    return SimpleNamespace(calc=calc, cfg=cfg, sd=sd, orc=oracle_model(cfg, sd))


@pytest.fixture(scope='module')
def runs(model):
    """phonons_many for both nfree, once: without the sum-rule correction (what the oracle bounds speak about) and, for nfree 2, with"""
    systems = model_systems()
    out = {}
    for nfree, acoustic in ((2, False), (4, False), (2, True)):
        res = model.calc.phonons_many(*_ph_args(systems), REPEATS, qpoints=Q_PATH, mesh=MESH, temperatures=TEMPS, delta=DELTA, nfree=nfree,
                                      acoustic=acoustic, want_modes=True, dos_bins=30)
        out[(nfree, acoustic)] = (res, dict(model.calc.phonon_info))
    return systems, out


@pytest.mark.parametrize('nfree', [2, 4])
def test_force_constants_and_spectra_against_the_fp64_oracle(model, runs, nfree):
    """|dPhi| <= c f_tol / delta, c = 1 (nfree 2) or 1.5 (nfree 4): the sums of the stencil weights times the engine's force
    tolerance, for the finite differences as they are (acoustic=False: a corrected self term is a sum of N - 1 of them);
    |dD| <= n_cells c f_tol / delta w_alpha w_beta (a sum over the cells, phases of modulus <= 1); |d lambda| <= ||dD||_F (Weyl, the
    Frobenius norm above the spectral norm).  Eigenvalues, not frequencies: the square root is unbounded near zero."""
    systems, out = runs
    res, info = out[(nfree, False)]
    c = {2: 1.0, 4: 1.5}[nfree]
    args = _ph_args(systems)
    n_mesh = int(np.prod(MESH))
    assert info == dict(n_force_calls=1, copies_evaluated=2 * (nfree * 6 + 1), launches=5, q_evaluated=2 * (len(Q_PATH) + n_mesh))
    for b, (types, pos, cell) in enumerate(systems):
        n_cells = int(np.prod(REPEATS[b]))
        types_sc = np.tile(types, n_cells)
        r = res[b]
        ref = phonon_ref.phonons(lambda p: _oracle(model, types_sc, p, r['supercell_cell'], [True] * 3)[1], pos, cell, args[2][b], REPEATS[b],
                                 Q_PATH, DELTA, nfree, acoustic=False)
        assert np.array_equal(r['supercell_positions'], ref['pos_sc']) and np.array_equal(r['supercell_cell'], ref['S'])
        phi_ref = ref['Phi'].reshape(2, 3, 2 * n_cells, 3).transpose(0, 2, 1, 3)
        err, tol = np.abs(r['force_constants'] - phi_ref).max(), c * F_TOL / DELTA
        w = np.repeat(1.0 / np.sqrt(args[2][b]), 3)
        ww = w[:, None] * w[None, :]
        assert r['status'] == 'ok' and err <= tol
        assert abs(r['asr_defect'] - ref['asr_defect']) <= 2 * n_cells * tol
        worst_d = worst_l = 0.0
        images = phonon_ref.images_brute(ref['pos_sc'], ref['S'], 2)[0]
        for k in range(len(Q_PATH)):
            R, D, _, _, _ = phonon_ref.dynmat(r['force_constants'].transpose(0, 2, 1, 3).reshape(6, -1), ref['pos_sc'], ref['S'], 2, args[2][b],
                                              images, phonon_ref.q_cartesian(Q_PATH[k], cell))
            lam, vec = np.linalg.eigh(D)
            dD = np.abs(D - ref['D'][k])
            d_lam = np.abs(r['eigenvalues'][k] - ref['eigenvalues'][k]).max()
            worst_d, worst_l = max(worst_d, (dD / ww).max()), max(worst_l, d_lam)
            assert (dD <= n_cells * tol * ww).all()
            assert d_lam <= np.linalg.norm(D - ref['D'][k]) + 1e-12 * np.abs(lam).max()
            # the driver's own D(q), seen through its eigen-decomposition: that of the restatement on the driver's Phi
            assert np.abs(r['eigenvalues'][k] - lam).max() <= 1e-12 * np.abs(lam).max()
            M = r['modes'][k].reshape(6, 6)
            assert np.abs(M.conj() @ M.T - np.eye(6)).max() <= 1e-12
            assert np.abs(D @ M[5] - r['eigenvalues'][k, 5] * M[5]).max() <= 1e-10 * np.abs(lam).max()
        print(f'nfree {nfree}, system {b} (repeats {REPEATS[b]}): max |dPhi| {err:.3e} eV/A^2 (bound {tol:.3e}), max |dD| / (w w) {worst_d:.3e} '
              f'(bound {n_cells * tol:.3e}), max |d lambda| {worst_l:.3e}, asr_defect {r["asr_defect"]:.3e} (oracle {ref["asr_defect"]:.3e}), '
              f'max |Phi| {np.abs(phi_ref).max():.3e}, hermiticity {r["hermiticity"].max():.3e}')
        e = phonon_ref.energies_of(r['eigenvalues'])
        assert np.array_equal(r['energies'], e) and np.array_equal(r['frequencies'], e * vib_ref.INV_CM)
        assert np.all(np.diff(r['eigenvalues'], axis=1) >= 0)


def test_commensurate_q_points_give_the_spectrum_of_the_explicit_supercell(model, runs):
    """vibrations_many on the explicit supercell, all atoms displaced, against phonons_many on the primitive cell at the n1 n2 n3
    commensurate q-points, acoustic=False.  With exact forces the finite-difference matrix H of the supercell is block-circulant
    (displacing atom beta of cell c is the translate of displacing it in the home cell), exp(i q . n S) = 1 at a commensurate q
    whichever images are kept, and the Fourier transform over the cells is unitary: the mass-weighted sym(H) has the spectrum of
    the blocks D(q).  vibrations_many diagonalises W sym(H + E_v) W and phonons_many the blocks herm(R(q) + R_E(q)) with
    R_E(q) = W sum_c E_p exp(..) W, where every element of E_v and E_p is below t = c f_tol / delta (the Hessian test above and of
    test_vib_gpu).  By Weyl each spectrum is within the spectral norm of its perturbation, bounded by the Frobenius norm: 3N t
    w_max^2 for the [3N,3N] matrix, and 3m (n_cells t) w_max^2 = 3N t w_max^2 for a block whose elements sum n_cells terms.  The two
    sorted spectra therefore differ by at most 2 x 3N t w_max^2, the bound from twice the force tolerance."""
    from sevennet_amd.phonon import build_supercell
    systems, _ = runs
    numbers, positions, masses, cells, pbcs = _ph_args(systems)
    q_comm = [np.array([[i / r[0], j / r[1], k / r[2]] for i in range(r[0]) for j in range(r[1]) for k in range(r[2])]) for r in REPEATS]
    ph = model.calc.phonons_many(numbers, positions, masses, cells, pbcs, REPEATS, qpoints=q_comm, delta=DELTA, nfree=2, acoustic=False)
    sc = [build_supercell(numbers[b], positions[b], cells[b], REPEATS[b]) for b in range(2)]
    vib = model.calc.vibrations_many([s[0] for s in sc], [s[1] for s in sc], [np.tile(masses[b], len(sc[b][0]) // 2) for b in range(2)],
                                     np.stack([s[2] for s in sc]), pbcs, delta=DELTA, nfree=2)
    for b in range(2):
        N = len(sc[b][0])
        got, want = np.sort(ph[b]['eigenvalues'].reshape(-1)), vib[b]['eigenvalues']
        tol = 2 * 3 * N * (F_TOL / DELTA) / masses[b].min()
        print(f'system {b} (repeats {REPEATS[b]}, N {N}): max |d lambda| {np.abs(got - want).max():.3e} (bound {tol:.3e}), largest '
              f'eigenvalue {np.abs(want).max():.3e}')
        assert got.shape == want.shape == (3 * N,) and np.abs(got - want).max() <= tol
        assert 'dos' not in ph[b] and ph[b]['qpoints'].shape == (N // 2, 3)


def test_surfaces(model, runs):
    systems, out = runs
    res, _ = out[(2, True)]
    raw, _ = out[(2, False)]
    args = _ph_args(systems)
    n_mesh = int(np.prod(MESH))
    keys = {'free_energy', 'energy', 'atomic_energies', 'forces', 'stress', 'num_edges', 'supercell', 'supercell_positions', 'supercell_cell',
            'force_constants', 'asr_defect', 'qpoints', 'energies', 'frequencies', 'eigenvalues', 'hermiticity', 'modes', 'mesh', 'dos_energies',
            'dos', 'thermo', 'status'}
    for b, r in enumerate(res):
        n_cells = int(np.prod(REPEATS[b]))
        N = 2 * n_cells
        assert set(r) == keys and r['status'] == 'ok' and r['supercell'].tolist() == list(REPEATS[b]) and r['mesh'] == MESH
        assert r['force_constants'].shape == (2, N, 3, 3) and r['supercell_positions'].shape == (N, 3) and r['forces'].shape == (N, 3)
        assert r['atomic_energies'].shape == (N,) and r['energies'].shape == r['frequencies'].shape == r['eigenvalues'].shape == (4, 6)
        assert r['hermiticity'].shape == (4,) and r['modes'].shape == (4, 6, 2, 3) and np.iscomplexobj(r['modes'])
        assert np.array_equal(r['qpoints'], Q_PATH) and r['dos'].shape == r['dos_energies'].shape == (30,)
        width = r['dos_energies'][1] - r['dos_energies'][0]
        assert abs((r['dos'] * width).sum() - 6.0) <= 1e-9
        th = r['thermo']
        assert set(th) == {'temperatures', 'free_energy', 'entropy', 'heat_capacity', 'zpe', 'n_imaginary', 'n_skipped'}
        assert th['temperatures'].tolist() == TEMPS and th['free_energy'][0] == th['zpe'] and th['entropy'][0] == 0.0
        assert th['n_imaginary'] + th['n_skipped'] <= 6 * n_mesh and th['n_skipped'] >= 0
        # the sum rule: every element but the self terms is the raw run's, the self terms close the sums (ordered sums of N terms)
        fc, fc_raw = r['force_constants'], raw[b]['force_constants']
        other = np.ones((2, N), bool)
        other[np.arange(2), np.arange(2)] = False
        assert np.array_equal(fc[other], fc_raw[other]) and r['asr_defect'] == raw[b]['asr_defect']
        assert np.abs(fc.sum(1)).max() <= 2 * N * EPS * np.abs(fc).sum(1).max()
        assert np.array_equal(r['forces'], raw[b]['forces']) and r['energy'] == raw[b]['energy']
    # the undisplaced supercell is compute_many's (the batch-versus-single tolerances of test_batch_gpu)
    many = model.calc.compute_many([np.tile(args[0][b], int(np.prod(REPEATS[b]))) for b in range(2)], [r['supercell_positions'] for r in res],
                                   np.stack([r['supercell_cell'] for r in res]), [True] * 3)
    for r, one in zip(res, many):
        assert abs(r['energy'] - one['energy']) <= 1e-6 * abs(one['energy']) + 1e-6 and r['free_energy'] == r['energy']
        assert np.abs(r['forces'] - one['forces']).max() <= 2e-5 * max(1.0, np.abs(one['forces']).max())
        assert r['num_edges'] == one['num_edges']
    # the atoms surface: the same bits; the caller's arrays are as they were
    atoms = [_MassAtoms(z, p, c, [True] * 3, ms) for z, p, ms, c in zip(args[0], args[1], args[2], args[3])]
    got = model.calc.phonons_many_atoms(atoms, REPEATS, qpoints=Q_PATH, mesh=MESH, temperatures=TEMPS, delta=DELTA, nfree=2, want_modes=True,
                                        dos_bins=30)
    for x, y in zip(res, got):
        for key in ('force_constants', 'eigenvalues', 'energies', 'dos', 'hermiticity', 'forces'):
            assert np.array_equal(x[key], y[key]), key
        assert np.array_equal(x['thermo']['free_energy'], y['thermo']['free_energy'])
    assert np.array_equal(args[1][0], model_systems()[0][1]) and np.array_equal(args[3][0], CELL)
    # a system alone against the same system inside the batch: each force of either run is within 2e-5 max(1, |F|) of the
    # single-structure one (test_batch_gpu), two of them over 2 delta -- the bound of test_vib_gpu for a small budget
    # (the finite differences themselves, acoustic=False: a corrected self term sums N - 1 of them)
    kw = dict(qpoints=Q_PATH, delta=DELTA, nfree=2, acoustic=False)
    alone = model.calc.phonons_many(args[0][1:], args[1][1:], args[2][1:], args[3][1:], [True] * 3, REPEATS[1], **kw)
    assert model.calc.phonon_info['copies_evaluated'] == 13 and 'dos' not in alone[0] and 'modes' not in alone[0]
    assert np.abs(alone[0]['force_constants'] - raw[1]['force_constants']).max() <= 4e-5 * max(1.0, 2.0 * np.abs(raw[1]['forces']).max()) / DELTA
    small = model.calc.phonons_many(*args, REPEATS, max_atoms_per_call=30, max_q_per_call=3, **kw)
    assert model.calc.phonon_info['n_force_calls'] > 1 and model.calc.phonon_info['q_evaluated'] == 8
    for x, y in zip(raw, small):
        assert np.abs(x['force_constants'] - y['force_constants']).max() <= 4e-5 * max(1.0, 2.0 * np.abs(x['forces']).max()) / DELTA
    sheared = args[3].copy()
    sheared[1, 2] += 2.0 * sheared[1, 0]
    with pytest.raises(ValueError, match='system 1: the supercell .* is not reduced'):
        model.calc.phonons_many(args[0], args[1], args[2], sheared, [True] * 3, REPEATS, qpoints=Q_PATH)
    with pytest.raises(ValueError, match='pass `qpoints`, `mesh` or both'):
        model.calc.phonons_many(*args, REPEATS)
    with pytest.raises(ValueError, match='fully periodic'):
        model.calc.phonons_many(*args[:4], [True, True, False], REPEATS, qpoints=Q_PATH)


def test_d3_sum_on_the_host_term_and_on_the_device_term(model, runs):
    """the device term's forces are the host term's bit for bit at fixed cells (test_d3_device_gpu) and the rows kernel adds them in
    a fixed order, so the force constants and all that follows are equal bit for bit; the D3 share is in"""
    from sevennet_amd.d3 import SevenNetD3Calculator
    systems, out = runs
    plain, _ = out[(2, True)]
    calc = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    args = _ph_args(systems)
    kw = dict(qpoints=Q_PATH, delta=DELTA, nfree=2)
    host = calc.phonons_many(*args, REPEATS, d3_term='host', **kw)
    info = dict(calc.phonon_info)
    dev = calc.phonons_many(*args, REPEATS, d3_term='device', **kw)
    assert calc.phonon_info == info and info['n_force_calls'] == 1
    for h, d, p in zip(host, dev, plain):
        assert np.isfinite(h['force_constants']).all() and h['status'] == d['status'] == 'ok'
        assert np.array_equal(h['force_constants'], d['force_constants']) and np.array_equal(h['eigenvalues'], d['eigenvalues'])
        assert h['energy'] == d['energy'] and np.array_equal(h['forces'], d['forces'])
        assert not np.array_equal(h['force_constants'], p['force_constants']) and h['energy'] != p['energy']
