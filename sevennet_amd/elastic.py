"""Batched second-order elastic tensors: the strained copies of many crystals written, evaluated and reduced on the device.

The rule is central differences of the stress over homogeneously strained copies; it is written out in include/snet_hip.h
("batched elastic tensors from strained copies") and restated in fp64 numpy in tests/elastic_ref.py.  System b has six strain
patterns (Voigt j = 0 .. 5 in ASE order xx, yy, zz, yz, xz, xy; a shear step is the engineering strain), nfree copies per pattern
and one unstrained copy: 6 nfree + 1 evaluations.  `plan_elastic` gives every copy (b, j, q) a slot of its own -- the strained
cells and volumes of the slots are computed once on the host, in fp64, by the expression the kernel applies to the positions, and
are what the force call and a D3 term are built with -- and packs the copies into calls of at most `max_atoms_per_call` atoms with
`fd.plan_copies`.  Per call one `snet_el_strain` launch writes the copies from the base positions (uploaded once), one batched
evaluation (sevennet_amd.batch) gives their virials and forces and one `snet_el_rows` launch writes the columns of the raw
stress-strain matrix S = d sigma / d epsilon and the rows of the internal-strain tensor L = d F / d epsilon they determine.  Each is
written by one workgroup of one call, so nothing is accumulated across calls and the result does not depend on the packing.
After the last call one `snet_el_finish` launch forms C = (S + S^T) / 2 and the asymmetry max |S - S^T|, and one transfer brings
everything to the host.  The relaxed-ion correction (the Gamma Hessian by `vib.vib_loop`, a pseudo-inverse and two products) and
the polycrystal averages run in numpy there: the matrices are tiny against the force calls.

Under a residual stress sigma_0 of the unstrained cell S is legitimately asymmetric by terms of the order of sigma_0, and C is the
elastic tensor where that stress is about zero: the unstrained copy's `stress` is returned beside it.  The relaxed-ion formula
presumes that the unstrained structure is at force equilibrium: `fmax` is returned, nothing is refused.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .batch import BatchForces, _as_host, device_positions, to_device, validate_batch_inputs
from .fd import STENCIL, BaseCopies, call_info, check_extra, check_refused, copy_calls, plan_copies, refused_count, write_copies
from .vib import vib_loop

GPA = 160.21766208   # GPa per eV/A^3
ELASTIC_STATUS_NAMES = ('ok', 'failed', 'singular')
SHEAR_AXES = {3: (1, 2), 4: (0, 2), 5: (0, 1)}   # the pair of axes a shear pattern couples


# ------------------------------------------------------------------------------------------------ validation, plan
def validate_elastic_inputs(n_atoms, cells, pbcs, delta, nfree, max_atoms_per_call, ion_delta=0.01) -> None:
    """The arguments of `elastic_batch` that `validate_batch_inputs` does not see, on the host (ValueError names the system):
    n_atoms [B], cells [B,3,3], pbcs [B,3] as validate_batch_inputs returns them; every system periodic along all three axes with a
    cell volume above zero; delta (the strain step) and ion_delta (A) finite and positive; nfree 2 or 4."""
    n_atoms = np.asarray(n_atoms, np.int64).reshape(-1)
    B = len(n_atoms)
    cells, pbcs = np.asarray(cells, np.float64).reshape(B, 3, 3), np.asarray(pbcs, bool).reshape(B, 3)
    for name, val, unit in (('delta', delta, 'strain step'), ('ion_delta', ion_delta, 'displacement in A')):
        try:
            ok = bool(np.isfinite(val)) and val > 0 and not isinstance(val, bool)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f'{name} = {val!r}: a finite positive {unit} is required')
    if isinstance(nfree, bool) or nfree not in (2, 4):
        raise ValueError(f'nfree = {nfree!r}: 2 (two strained copies per pattern) or 4 is required')
    if isinstance(max_atoms_per_call, bool) or not isinstance(max_atoms_per_call, (int, np.integer)) or max_atoms_per_call < 1:
        raise ValueError(f'max_atoms_per_call = {max_atoms_per_call!r}: an integer >= 1 is required')
    for b in range(B):
        if not pbcs[b].all():
            raise ValueError(f'system {b}: an elastic tensor needs a fully periodic system, got pbc = {pbcs[b].tolist()}')
        if not np.isfinite(cells[b]).all() or not abs(np.linalg.det(cells[b])) > 0.0:
            raise ValueError(f'system {b}: the cell is singular or not finite')


def strain_rows(x, j: int, q: int, delta: float) -> np.ndarray:
    """rows x [..., 3] (positions, or the cell's lattice vectors) times F = I + (q delta) E_j, by the expression of snet_el_strain:
    the same bits as the device's"""
    x = np.asarray(x, np.float64)
    out = x.copy()
    if q == 0:
        return out
    s = float(q) * delta
    if j < 3:
        out[..., j] = x[..., j] + s * x[..., j]
    else:
        a, b = SHEAR_AXES[j]
        h = s * 0.5
        out[..., a] = x[..., a] + h * x[..., b]
        out[..., b] = x[..., b] + h * x[..., a]
    return out


def plan_elastic(n_atoms, cells, delta: float, nfree: int, max_atoms_per_call: int) -> SimpleNamespace:
    """The strained copies of B systems packed into calls by `fd.plan_copies` with six row groups per system (a pure function
    of its arguments).  Every copy has a slot of its own, because its cell is its own: slot (6 nfree + 1) b + nfree j + w holds
    copy (b, j, STENCIL[nfree][w]) and slot (6 nfree + 1) b + 6 nfree the unstrained copy.
    -> plan with `slot_system` int64 [S], `slot_desc` int32 [S,3] (system, j, q), `slot_cells` fp64 [S,3,3] (cell F),
    `slot_volumes` fp64 [S], `delta`, `nfree` and `calls` as plan_copies, except that `ids` are these slots, `desc` is int32 [c,3]
    (system, j, q) and `groups` int32 [g,3] holds (first copy within the call, system, j)."""
    n = np.asarray(n_atoms, np.int64).reshape(-1)
    B = len(n)
    cells = np.asarray(cells, np.float64).reshape(B, 3, 3)
    per = 6 * nfree + 1
    plan = plan_copies(n, None, nfree, int(max_atoms_per_call), n_groups=[6] * B)
    slot_desc = np.zeros((B * per, 3), np.int32)
    for b in range(B):
        for j in range(6):
            for w, q in enumerate(STENCIL[nfree]):
                slot_desc[per * b + nfree * j + w] = (b, j, q)
        slot_desc[per * b + 6 * nfree] = (b, 0, 0)
    slot_cells = np.stack([strain_rows(cells[b], j, q, delta) for b, j, q in slot_desc.tolist()])
    calls = []
    for call in plan.calls:
        desc = np.ascontiguousarray(call.desc[:, [0, 1, 3]])
        w_of = {q: w for w, q in enumerate(STENCIL[nfree])}
        ids = np.array([per * b + (6 * nfree if q == 0 else nfree * j + w_of[q]) for b, j, q in desc.tolist()], np.int64)
        calls.append(SimpleNamespace(ids=ids, desc=desc, groups=call.groups, base=call.base, n_atoms=call.n_atoms))
    return SimpleNamespace(slot_system=np.repeat(np.arange(B), per), slot_desc=slot_desc, slot_cells=slot_cells,
                           slot_volumes=np.abs(np.linalg.det(slot_cells)), delta=float(delta), nfree=nfree, calls=calls)


# ------------------------------------------------------------------------------------------------ launches
def el_strain(pos0, seg_ptr0, desc, copy_ptr, delta, pos_out, status) -> None:
    """one `snet_el_strain` launch on the current stream (fd.write_copies; desc int32 [c,3])"""
    write_copies('snet_el_strain', 3, pos0, seg_ptr0, desc, copy_ptr, delta, pos_out, status)


def el_rows(virial: torch.Tensor, virial_extra: Optional[torch.Tensor], volume: torch.Tensor, forces: torch.Tensor,
            forces_extra: Optional[torch.Tensor], seg_ptr: torch.Tensor, group: torch.Tensor, nfree: int, delta: float,
            atom_ptr: torch.Tensor, S: torch.Tensor, L: torch.Tensor, status: torch.Tensor) -> None:
    """one `snet_el_rows` launch on the current stream (forces fp32; virial / virial_extra / volume / forces_extra / S / L fp64; the
    rest int32)"""
    N, n_copies, n_groups = int(forces.shape[0]), int(seg_ptr.numel()) - 1, int(group.shape[0])
    n_sys, n_base = int(atom_ptr.numel()) - 1, int(L.numel()) // 18
    f64, i32 = torch.float64, torch.int32
    want = [(virial, f64, (n_copies, 6)), (volume, f64, (n_copies,)), (forces, torch.float32, (N, 3)), (seg_ptr, i32, (n_copies + 1,)),
            (group, i32, (n_groups, 3)), (atom_ptr, i32, (n_sys + 1,)), (S, f64, (36 * n_sys,)), (L, f64, (18 * n_base,)),
            (status, i32, (n_sys,))]
    if virial_extra is not None:
        want.append((virial_extra, f64, (n_copies, 6)))
    if forces_extra is not None:
        want.append((forces_extra, f64, (N, 3)))
    _lib.check_device_tensors('el_rows', S, want)
    P = _lib.ptr
    with torch.cuda.device(S.device):
        _lib.check(_lib.load().snet_el_rows(P(virial), P(virial_extra), P(volume), P(forces), P(forces_extra), N, P(seg_ptr), n_copies,
                                            P(group), n_groups, int(nfree), float(delta), P(atom_ptr), n_base, n_sys, P(S), P(L),
                                            P(status), _lib.stream()), 'snet_el_rows')


def el_finish(S: torch.Tensor, status: torch.Tensor, C: torch.Tensor, asymmetry: torch.Tensor) -> None:
    """one `snet_el_finish` launch on the current stream (S / C / asymmetry fp64, status int32)"""
    n_sys = int(status.numel())
    f64 = torch.float64
    _lib.check_device_tensors('el_finish', S, [(S, f64, (36 * n_sys,)), (status, torch.int32, (n_sys,)), (C, f64, (36 * n_sys,)),
                                               (asymmetry, f64, (n_sys,))])
    P = _lib.ptr
    with torch.cuda.device(S.device):
        _lib.check(_lib.load().snet_el_finish(P(S), n_sys, P(status), P(C), P(asymmetry), _lib.stream()), 'snet_el_finish')


# ------------------------------------------------------------------------------------------------ the loop
def elastic_loop(forces, plan, positions, n_atoms, *, keeper: Optional[Callable] = None, want_atomic_virial: bool = False):
    """The calls of a plan (`plan_elastic`).  forces: a BatchForces over the slots of `plan` (plan.slot_system, plan.slot_cells), or
    any object with its call interface (relax.fire_cell_loop documents it); the virial of its `extra`, if any, is read from
    `forces.virial_extra` after each call.  positions: the flat base positions [sum n_b, 3]; n_atoms [B].  Per call one
    `snet_el_strain`, one force call (fd.copy_calls: keeper(call, graph, output, extra forces), if given, is called after each
    force call -- the driver keeps the unstrained copies' results with it -- and want_atomic_virial asks the calls that hold such
    a copy for the per-atom virial) and one `snet_el_rows`, nothing read back.  Then one `snet_el_finish` and one transfer.
    -> (S [B,6,6] raw d sigma_i / d epsilon_j in eV/A^3, L: per system [6,3 n_b] in eV/A, C [B,6,6], asymmetry [B], status [B] (0
    ok, 2 a non-finite virial or force or a volume that is not positive, 3 a layout the kernels refused), info)"""
    dev = forces.engine.dev
    n = np.asarray(n_atoms, np.int64).reshape(-1)
    B, nfree, delta = len(n), plan.nfree, plan.delta
    a_ptr = np.concatenate([[0], np.cumsum(n)])
    f64, i32 = torch.float64, torch.int32
    with torch.cuda.device(dev):
        pos0 = device_positions(positions, dev).contiguous()
        seg0 = to_device(a_ptr, i32, dev)
        S = torch.zeros(36 * B, dtype=f64, device=dev)
        L = torch.zeros(18 * int(a_ptr[-1]), dtype=f64, device=dev)
        status = torch.zeros(B, dtype=i32, device=dev)
        refused = []
        for call, g, out, fx in copy_calls(forces, plan.calls, pos0, seg0, n, el_strain, delta, refused, want_atomic_virial, keeper):
            if len(call.groups):
                el_rows(out['virial_per_system'], getattr(forces, 'virial_extra', None), to_device(plan.slot_volumes[call.ids], f64, dev),
                        out['forces'], fx, g.seg_ptr, to_device(call.groups, i32, dev), nfree, delta, seg0, S, L, status)
        C, asym = torch.empty_like(S), torch.empty(B, dtype=f64, device=dev)
        el_finish(S, status, C, asym)
        flat = torch.cat([S, C, asym, L, status.to(f64), refused_count(refused)]).cpu().numpy()   # the one transfer
    check_refused(flat[-1], el_strain)
    l0 = 73 * B
    L_h = [flat[l0 + 18 * a_ptr[b]:l0 + 18 * a_ptr[b + 1]].reshape(6, 3 * int(n[b])).copy() for b in range(B)]
    return (flat[:36 * B].reshape(B, 6, 6).copy(), L_h, flat[36 * B:72 * B].reshape(B, 6, 6).copy(), flat[72 * B:73 * B].copy(),
            flat[l0 + 18 * int(a_ptr[-1]):l0 + 18 * int(a_ptr[-1]) + B].astype(np.int64), call_info(forces, plan.calls, 1))


# ------------------------------------------------------------------------------------------------ host: relaxed ions, moduli
def translations(n: int) -> np.ndarray:
    """T [3n,3]: the three normalised uniform translations of n atoms"""
    T = np.zeros((3 * n, 3))
    for k in range(3):
        T[k::3, k] = 1.0 / np.sqrt(n)
    return T


def ion_pseudo_inverse(phi: np.ndarray, floor: float = 0.0) -> Tuple[Optional[np.ndarray], np.ndarray]:
    """Phi+ = (P Phi P + kappa T T^T)^-1 - T T^T / kappa of a Gamma Hessian Phi [3n,3n], with T the uniform translations, P = I - T T^T
    and kappa the mean diagonal of Phi: the inverse of Phi on the complement of T, zero on T.  -> (Phi+, the eigenvalues of P Phi P
    on that complement, ascending); Phi+ is None where the smallest of them is at or below `floor` (the noise of Phi), or kappa is
    not positive.  One atom has no internal coordinate: Phi+ = 0."""
    n3 = phi.shape[0]
    T = translations(n3 // 3)
    TT = T @ T.T
    P = np.eye(n3) - TT
    A = P @ phi @ P
    A = (A + A.T) * 0.5
    if n3 == 3:
        return np.zeros((3, 3)), np.zeros(0)
    q = np.linalg.svd(P)[0][:, :n3 - 3]   # an orthonormal basis of the complement of T (P has the singular values 1 and 0)
    lam = np.linalg.eigvalsh(q.T @ A @ q)
    kappa = float(np.mean(np.diag(phi)))
    if not (np.isfinite(lam).all() and kappa > 0 and lam[0] > floor):
        return None, lam
    return np.linalg.inv(A + kappa * TT) - TT / kappa, lam


def relaxed_stress_strain(S: np.ndarray, L: np.ndarray, phi_plus: np.ndarray, volume: float) -> np.ndarray:
    """S_rel = S - L Phi+ L^T / V: the raw stress-strain matrix with the ions following the strain (S [6,6], L [6,3n])"""
    return S - (L @ phi_plus @ L.T) / volume


def symmetrise(S: np.ndarray) -> Tuple[np.ndarray, float]:
    """(C = (S + S^T) 0.5, max |S - S^T|): what snet_el_finish computes, for a matrix formed on the host"""
    return (S + S.T) * 0.5, float(np.abs(S - S.T).max())


def moduli(C: np.ndarray) -> Dict[str, Any]:
    """compliance, the Voigt / Reuss / Hill bulk and shear moduli, Young's modulus and Poisson's ratio (from the Hill values) of an
    elastic tensor C [6,6] (the units of C), and `stable`: every eigenvalue of C positive (Born).  NaN where C is not finite or
    cannot be inverted."""
    nan = float('nan')
    vrh = lambda v, r: dict(voigt=v, reuss=r, hill=0.5 * (v + r))   # noqa: E731
    bad = dict(compliance=np.full((6, 6), np.nan), bulk_modulus=vrh(nan, nan), shear_modulus=vrh(nan, nan), youngs_modulus=nan,
               poisson_ratio=nan, stable=False)
    if not np.isfinite(C).all():
        return bad
    stable = bool((np.linalg.eigvalsh(C) > 0).all())
    try:
        s = np.linalg.inv(C)
    except np.linalg.LinAlgError:
        return bad
    k_v = ((C[0, 0] + C[1, 1] + C[2, 2]) + 2.0 * (C[0, 1] + C[0, 2] + C[1, 2])) / 9.0
    g_v = ((C[0, 0] + C[1, 1] + C[2, 2]) - (C[0, 1] + C[0, 2] + C[1, 2]) + 3.0 * (C[3, 3] + C[4, 4] + C[5, 5])) / 15.0
    k_r = 1.0 / ((s[0, 0] + s[1, 1] + s[2, 2]) + 2.0 * (s[0, 1] + s[0, 2] + s[1, 2]))
    g_r = 15.0 / (4.0 * (s[0, 0] + s[1, 1] + s[2, 2]) - 4.0 * (s[0, 1] + s[0, 2] + s[1, 2]) + 3.0 * (s[3, 3] + s[4, 4] + s[5, 5]))
    K, G = vrh(float(k_v), float(k_r)), vrh(float(g_v), float(g_r))
    k, g = K['hill'], G['hill']
    return dict(compliance=s, bulk_modulus=K, shear_modulus=G, youngs_modulus=9.0 * k * g / (3.0 * k + g),
                poisson_ratio=(3.0 * k - 2.0 * g) / (2.0 * (3.0 * k + g)), stable=stable)


# ------------------------------------------------------------------------------------------------ the driver
def elastic_batch(engine, types, positions, cells, pbcs, *, cutoff: float, delta: float = 0.005, nfree: int = 2,
                  relax_ions: bool = False, ion_delta: float = 0.01, masses=None, extra: Optional[Callable] = None,
                  make_extra: Optional[Callable] = None, max_atoms_per_call: int = 32768, n_atoms=None,
                  want_atomic_virial: bool = False) -> Tuple[List[Dict[str, Any]], Dict[str, int]]:
    """Second-order elastic tensors of B crystals at once.

    engine: a HipForceEngine; types / positions / cells / pbcs / n_atoms as batch.build_batch_graph takes them (pbc all true).
    delta: the strain step (a shear step is the engineering strain); nfree: 2 or 4 strained copies per pattern;
    max_atoms_per_call as vib.vibrations_batch.  relax_ions: also the relaxed-ion tensor, from the Gamma Hessian of all atoms
    by `vib.vib_loop` with the displacement ion_delta (A) and the same nfree; masses are not needed (the Hessian is not
    mass-weighted) and are accepted for symmetry with the other drivers.  extra: as batch.BatchForces, called over the slots of
    `plan_elastic` (it must return a virial, the third element, to take part in the stresses; not with relax_ions, whose Hessian
    has slots of its own); make_extra(slot_system, slot_cells) -> extra builds such a term once the slots and their (strained)
    cells are known, and is called once more for the Hessian's slots with relax_ions.  The caller's arrays are not modified.

    Returns (results, info).  results[b]: the keys of SevenNetCalculator.compute_many for the unstrained structure (the model's
    values; an `extra` term is not in them) -- its `stress` tells how far C can be read as the elastic tensor, see the module's
    text -- plus `stress_strain` [6,6] (raw d sigma_i / d epsilon_j, eV/A^3, ASE Voigt order, engineering shear), `elastic_tensor`
    [6,6] (its symmetric part), `asymmetry` (max |S - S^T|), `internal_strain` [n,3,6] (d F_ak / d epsilon_j at fixed scaled
    coordinates, eV/A), `fmax` (the largest force component of the unstrained structure, `extra` included), `compliance`,
    `bulk_modulus` and `shear_modulus` (dicts with `voigt`, `reuss`, `hill`), `youngs_modulus` and `poisson_ratio` (from the Hill
    values), `stable` (every eigenvalue of the tensor positive) and `status`: 'ok', 'failed' (a non-finite virial or force: what
    follows from it is NaN) or 'singular'.  With relax_ions `elastic_tensor` and what follows from it are the relaxed-ion ones
    and there are also `elastic_tensor_clamped`, `stress_strain_clamped`, `hessian` [3n,3n] (eV/A^2), `hessian_asymmetry` and
    `ion_eigenvalues` (of the Hessian on the complement of the uniform translations, ascending); where the smallest of them is at
    or below `hessian_asymmetry`, the noise of the Hessian, the relaxed tensor is NaN and the status 'singular'.  Multiply by
    GPA for GPa.  info: `n_force_calls`, `copies_evaluated` and `launches` (of the kernels), the Hessian's included.  Invalid
    input raises ValueError before any device work."""
    types, positions, n_at, cells, pbcs = validate_batch_inputs(types, positions, cells, pbcs, cutoff, engine.spec.num_species, n_atoms)
    validate_elastic_inputs(n_at, cells, pbcs, delta, nfree, max_atoms_per_call, ion_delta)
    check_extra(extra, make_extra)
    if extra is not None and relax_ions:
        raise ValueError('relax_ions evaluates a second set of copies (the Hessian\'s): pass `make_extra`, which is called for each set')
    B = len(n_at)
    a_ptr = np.concatenate([[0], np.cumsum(n_at)])
    positions = _as_host(positions, np.float64).reshape(-1, 3)
    plan = plan_elastic(n_at, cells, delta, nfree, int(max_atoms_per_call))
    slot = plan.slot_system
    if make_extra is not None:
        extra = make_extra(slot, plan.slot_cells)
    slot_types = lambda s: np.concatenate([types[a_ptr[b]:a_ptr[b + 1]] for b in s])   # noqa: E731
    forces = BatchForces(engine, slot_types(slot), n_at[slot], plan.slot_cells, pbcs[slot], cutoff, extra)
    base = BaseCopies(want_atomic_virial, keep_extra=True)
    S, L, C, asym, status, info = elastic_loop(forces, plan, positions, n_at, keeper=base, want_atomic_virial=want_atomic_virial)
    hess = None
    if relax_ions:
        selected = [np.arange(int(k), dtype=np.int64) for k in n_at]
        vplan = plan_copies(n_at, selected, nfree, int(max_atoms_per_call))
        vslot = vplan.slot_system
        vextra = make_extra(vslot, cells[vslot]) if make_extra is not None else None
        vforces = BatchForces(engine, slot_types(vslot), n_at[vslot], cells[vslot], pbcs[vslot], cutoff, vextra)
        H, _, h_asym, h_status, h_info = vib_loop(vforces, vplan, positions, n_at, selected, [np.ones(int(k)) for k in n_at],
                                                   delta=ion_delta)
        hess = (H, h_asym, h_status)
        info = {k: info[k] + h_info[k] for k in info}
    results = base.results(n_at, cells)
    for res in results:   # (fmax: of the unstrained structure, the extra forces included)
        fx = res.pop('forces_extra', None)
        res['fmax'] = float(np.abs(res['forces'] if fx is None else res['forces'] + fx).max())
    volumes = np.abs(np.linalg.det(cells))
    for b in range(B):
        res = results[b]
        code = 0 if status[b] == 0 else 1
        tensor, raw, a = C[b], S[b], float(asym[b])
        if code:
            raw, L[b] = np.full((6, 6), np.nan), np.full_like(L[b], np.nan)
        if relax_ions:
            H, h_asym, h_status = hess
            res.update(elastic_tensor_clamped=tensor, stress_strain_clamped=raw, hessian=H[b], hessian_asymmetry=float(h_asym[b]))
            phi_plus, lam = (None, np.full(max(3 * int(n_at[b]) - 3, 0), np.nan)) if code or h_status[b] != 0 else \
                ion_pseudo_inverse(H[b], float(h_asym[b]))
            res['ion_eigenvalues'] = lam
            if phi_plus is None:
                code = code or (1 if h_status[b] != 0 else 2)
                raw, tensor, a = np.full((6, 6), np.nan), np.full((6, 6), np.nan), float('nan')
            else:
                raw = relaxed_stress_strain(raw, L[b], phi_plus, float(volumes[b]))
                tensor, a = symmetrise(raw)
        res.update(stress_strain=raw, elastic_tensor=tensor, asymmetry=a,
                   internal_strain=np.ascontiguousarray(L[b].reshape(6, int(n_at[b]), 3).transpose(1, 2, 0)),
                   status=ELASTIC_STATUS_NAMES[code])
        res.update(moduli(tensor))
    return results, info
