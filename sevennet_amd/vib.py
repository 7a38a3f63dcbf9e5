"""Batched harmonic analysis: the finite-difference Hessians of many structures, their displaced copies written, evaluated and
reduced on the device.

The rule is central differences of forces, as ASE's `Vibrations` with direction='central'; it is written out in
include/snet_hip.h (snet_vib_displace / snet_vib_rows / snet_vib_finish) and restated in fp64 numpy in tests/vib_ref.py.  For
system b with m_b displaced atoms there are nfree * 3 m_b displaced copies and one undisplaced copy.  `plan_copies` packs the
copies of all systems into calls of at most `max_atoms_per_call` atoms; per call one `snet_vib_displace` launch writes the
copies from the base positions (uploaded once), one batched evaluation (sevennet_amd.batch) gives their forces and one
`snet_vib_rows` launch writes the rows of the difference matrix D they determine.  Each row is written by one workgroup of one
call, so nothing is accumulated across calls and the result does not depend on the packing.  After the last call one
`snet_vib_finish` launch forms H = (D + D^T) / 2, the mass-weighted Hm and the asymmetry max |D - D^T|, one transfer brings them
to the host, and numpy.linalg.eigh runs per system there: the matrices are tiny against the force calls.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .batch import BatchForces, _as_host, device_positions, to_device, validate_batch_inputs
from .fd import (STENCIL, BaseCopies, call_info, check_extra, check_refused, copy_calls, plan_copies,   # noqa: F401
                 refused_count, write_copies)
from .md import ACC

HBAR = 0.6582119569        # eV fs
INV_CM = 8065.543937       # cm^-1 per eV
VIB_STATUS_NAMES = ('ok', 'failed')


# ------------------------------------------------------------------------------------------------ validation, plan
def validate_vib_inputs(n_atoms, masses, indices, delta, nfree, max_atoms_per_call) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """The arguments of `vibrations_batch` that `validate_batch_inputs` does not see, on the host (ValueError names the system):
    n_atoms [B]; masses: per-system arrays [n_b] in amu, or one flat array [sum n_b]; indices: None, or per system None (all
    atoms), a bool mask [n_b] or a list of unique atom indices.  -> (masses per system fp64, selected atoms per system int64)"""
    n_atoms = np.asarray(n_atoms, np.int64).reshape(-1)
    B = len(n_atoms)
    try:
        delta_ok = bool(np.isfinite(delta)) and delta > 0
    except TypeError:
        delta_ok = False
    if not delta_ok:
        raise ValueError(f'delta = {delta!r}: a finite positive displacement in A is required')
    if isinstance(nfree, bool) or nfree not in (2, 4):
        raise ValueError(f'nfree = {nfree!r}: 2 (two displacements per coordinate) or 4 is required')
    if isinstance(max_atoms_per_call, bool) or not isinstance(max_atoms_per_call, (int, np.integer)) or max_atoms_per_call < 1:
        raise ValueError(f'max_atoms_per_call = {max_atoms_per_call!r}: an integer >= 1 is required')
    if isinstance(masses, (list, tuple)) and len(masses) == B and not np.isscalar(masses[0]):
        masses = [_as_host(m, np.float64).reshape(-1) for m in masses]
    else:
        flat = _as_host(masses, np.float64).reshape(-1)
        if len(flat) != int(n_atoms.sum()):
            raise ValueError(f'{len(flat)} masses but {int(n_atoms.sum())} atoms in {B} systems')
        masses = np.split(flat, np.cumsum(n_atoms)[:-1])
    for b, m in enumerate(masses):
        if len(m) != n_atoms[b]:
            raise ValueError(f'system {b}: {len(m)} masses but {int(n_atoms[b])} atoms')
        if not (np.isfinite(m) & (m > 0)).all():
            raise ValueError(f'system {b}: masses must be finite and positive (amu), got {m[~(np.isfinite(m) & (m > 0))][0]}')
    if indices is None:
        indices = [None] * B
    if not isinstance(indices, (list, tuple)) or len(indices) != B:
        raise ValueError(f'indices: None, or one entry per system ({B}), is required')
    selected = []
    for b, idx in enumerate(indices):
        n = int(n_atoms[b])
        if idx is None:
            selected.append(np.arange(n, dtype=np.int64))
            continue
        idx = np.asarray(idx)
        if idx.dtype == bool:
            if idx.shape != (n,):
                raise ValueError(f'system {b}: an index mask of shape ({n},) is required, got {idx.shape}')
            idx = np.nonzero(idx)[0]
        elif idx.size and (not np.issubdtype(idx.dtype, np.integer) or idx.ndim != 1):
            raise ValueError(f'system {b}: the displaced atoms are given as None, a bool mask or a list of atom indices')
        idx = idx.astype(np.int64).reshape(-1)
        if idx.size == 0:
            raise ValueError(f'system {b}: no atom is selected')
        if ((idx < 0) | (idx >= n)).any():
            raise ValueError(f'system {b}: atom index {int(idx[(idx < 0) | (idx >= n)][0])} is out of range (the system has {n} atoms)')
        if len(np.unique(idx)) != len(idx):
            raise ValueError(f'system {b}: an atom index is given more than once')
        selected.append(idx)
    return masses, selected


# ------------------------------------------------------------------------------------------------ launches
def vib_displace(pos0, seg_ptr0, desc, copy_ptr, delta, pos_out, status) -> None:
    """one `snet_vib_displace` launch on the current stream (fd.write_copies; desc int32 [c,4])"""
    write_copies('snet_vib_displace', 4, pos0, seg_ptr0, desc, copy_ptr, delta, pos_out, status)


def vib_rows(forces: torch.Tensor, forces_extra: Optional[torch.Tensor], seg_ptr: torch.Tensor, group: torch.Tensor, nfree: int,
             delta: float, sel: torch.Tensor, sel_ptr: torch.Tensor, d_off: torch.Tensor, D: torch.Tensor, status: torch.Tensor) -> None:
    """one `snet_vib_rows` launch on the current stream (forces fp32, forces_extra / D fp64, d_off int64, the rest int32)"""
    N, n_copies, n_groups = int(forces.shape[0]), int(seg_ptr.numel()) - 1, int(group.shape[0])
    n_sel, n_sys, d_size = int(sel.numel()), int(sel_ptr.numel()) - 1, int(D.numel())
    f64, i32 = torch.float64, torch.int32
    want = [(forces, torch.float32, (N, 3)), (seg_ptr, i32, (n_copies + 1,)), (group, i32, (n_groups, 3)), (sel, i32, (n_sel,)),
            (sel_ptr, i32, (n_sys + 1,)), (d_off, torch.int64, (n_sys,)), (D, f64, (d_size,)), (status, i32, (n_sys,))]
    if forces_extra is not None:
        want.append((forces_extra, f64, (N, 3)))
    _lib.check_device_tensors('vib_rows', D, want)
    P = _lib.ptr
    with torch.cuda.device(D.device):
        _lib.check(_lib.load().snet_vib_rows(P(forces), P(forces_extra), N, P(seg_ptr), n_copies, P(group), n_groups, int(nfree),
                                             float(delta), P(sel), P(sel_ptr), n_sel, P(d_off), n_sys, P(D), d_size, P(status),
                                             _lib.stream()), 'snet_vib_rows')


def vib_finish(D: torch.Tensor, d_off: torch.Tensor, sel_ptr: torch.Tensor, w: torch.Tensor, status: torch.Tensor, H: torch.Tensor,
               Hm: torch.Tensor, asymmetry: torch.Tensor) -> None:
    """one `snet_vib_finish` launch on the current stream (D / w / H / Hm / asymmetry fp64, d_off int64, the rest int32)"""
    n_sel, n_sys, d_size = int(w.numel()), int(sel_ptr.numel()) - 1, int(D.numel())
    f64, i32 = torch.float64, torch.int32
    _lib.check_device_tensors('vib_finish', D, [(D, f64, (d_size,)), (d_off, torch.int64, (n_sys,)), (sel_ptr, i32, (n_sys + 1,)),
                                                (w, f64, (n_sel,)), (status, i32, (n_sys,)), (H, f64, (d_size,)), (Hm, f64, (d_size,)),
                                                (asymmetry, f64, (n_sys,))])
    P = _lib.ptr
    with torch.cuda.device(D.device):
        _lib.check(_lib.load().snet_vib_finish(P(D), P(d_off), P(sel_ptr), n_sel, P(w), n_sys, d_size, P(status), P(H), P(Hm),
                                               P(asymmetry), _lib.stream()), 'snet_vib_finish')


# ------------------------------------------------------------------------------------------------ the loop
def vib_loop(forces, plan, positions, n_atoms, selected, masses, *, delta: float, keeper: Optional[Callable] = None,
             want_atomic_virial: bool = False):
    """The calls of a plan.  forces: a BatchForces over the copy slots of `plan` (plan.slot_system), or any object with its call
    interface (relax.fire_cell_loop documents it); positions: the flat base positions [sum n_b, 3]; n_atoms [B], selected and
    masses per system as `validate_vib_inputs` returns them.  Per call one `snet_vib_displace`, one force call (fd.copy_calls:
    keeper(call, graph, output, extra forces), if given, is called after each force call -- the driver keeps the undisplaced
    copies' results with it -- and want_atomic_virial asks the calls that hold such a copy for the per-atom virial) and one
    `snet_vib_rows`, nothing read back.  Then one `snet_vib_finish` and one transfer.
    -> (hessian, mass-weighted hessian: lists of [3 m_b, 3 m_b] fp64 arrays; asymmetry [B]; status [B] (0 ok, 2 a non-finite
    force, 3 a layout the kernels refused); info)"""
    dev = forces.engine.dev
    n = np.asarray(n_atoms, np.int64).reshape(-1)
    B, nfree = len(n), plan.nfree
    m = np.array([len(s) for s in selected], np.int64)
    d_off = np.concatenate([[0], np.cumsum(9 * m * m)])
    f64, i32 = torch.float64, torch.int32
    with torch.cuda.device(dev):
        pos0 = device_positions(positions, dev).contiguous()
        seg0 = to_device(np.concatenate([[0], np.cumsum(n)]), i32, dev)
        sel_d, sel_ptr = to_device(np.concatenate(selected), i32, dev), to_device(np.concatenate([[0], np.cumsum(m)]), i32, dev)
        w_d = to_device(np.concatenate([1.0 / np.sqrt(np.asarray(ms, np.float64)[s]) for ms, s in zip(masses, selected)]), f64, dev)
        off_d = to_device(d_off[:-1], torch.int64, dev)
        D = torch.zeros(int(d_off[-1]), dtype=f64, device=dev)
        status = torch.zeros(B, dtype=i32, device=dev)
        refused = []
        for call, g, out, fx in copy_calls(forces, plan.calls, pos0, seg0, n, vib_displace, delta, refused, want_atomic_virial, keeper):
            if len(call.groups):
                vib_rows(out['forces'], fx, g.seg_ptr, to_device(call.groups, i32, dev), nfree, delta, sel_d, sel_ptr, off_d, D, status)
        H, Hm, asym = torch.empty_like(D), torch.empty_like(D), torch.empty(B, dtype=f64, device=dev)
        vib_finish(D, off_d, sel_ptr, w_d, status, H, Hm, asym)
        flat = torch.cat([H, Hm, asym, status.to(f64), refused_count(refused)]).cpu().numpy()   # the one transfer
    check_refused(flat[-1], vib_displace)
    size = int(d_off[-1])
    cut = lambda a: [a[d_off[b]:d_off[b + 1]].reshape(3 * m[b], 3 * m[b]).copy() for b in range(B)]   # noqa: E731
    return (cut(flat[:size]), cut(flat[size:2 * size]), flat[2 * size:2 * size + B].copy(),
            flat[2 * size + B:2 * size + 2 * B].astype(np.int64), call_info(forces, plan.calls, 1))


# ------------------------------------------------------------------------------------------------ host: spectrum
def spectrum(hm: np.ndarray) -> Dict[str, Any]:
    """eigenvalues (ascending, eV/(A^2 amu)), modes [3m, m, 3] (row k: the eigenvector of eigenvalues[k]), energies h nu (eV) and
    frequencies (cm^-1), both signed -- an imaginary mode is a negative number -- and the zero-point energy (eV, half the sum of
    the positive h nu) of a mass-weighted Hessian [3m,3m]; NaN throughout where it is not finite"""
    k = hm.shape[0]
    if not np.isfinite(hm).all():
        nan = np.full(k, np.nan)
        return dict(eigenvalues=nan, modes=np.full((k, k // 3, 3), np.nan), energies=nan.copy(), frequencies=nan.copy(), zpe=float('nan'))
    lam, vec = np.linalg.eigh(hm)
    e = HBAR * np.sqrt(ACC * np.abs(lam)) * np.sign(lam)
    return dict(eigenvalues=lam, modes=np.ascontiguousarray(vec.T).reshape(k, k // 3, 3), energies=e, frequencies=e * INV_CM,
                zpe=float(0.5 * e[e > 0].sum()))


def harmonic_prefactor(energies_min, energies_saddle) -> float:
    """The Vineyard prefactor prod nu_min / prod' nu_saddle in THz (harmonic transition-state theory: rate = prefactor
    exp(-barrier / kT)) from the signed mode energies h nu (eV) of `vibrations_many` at a minimum and at the saddle of a hop,
    over the positive modes of each.  The minimum must have exactly one positive mode more than the saddle (the hop's
    direction, imaginary at the saddle): ValueError otherwise."""
    lo, hi = np.asarray(energies_min, np.float64).reshape(-1), np.asarray(energies_saddle, np.float64).reshape(-1)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError('harmonic_prefactor: the mode energies must be finite')
    p_min, p_sad = lo[lo > 0], hi[hi > 0]
    if len(p_min) != len(p_sad) + 1:
        raise ValueError(f'harmonic_prefactor: {len(p_min)} positive modes at the minimum and {len(p_sad)} at the saddle, but the '
                         'minimum must have exactly one more than the saddle')
    to_thz = 1e3 / (2.0 * np.pi * HBAR)   # nu = h nu / (2 pi hbar) in 1/fs, times 1e3
    return float(np.exp(np.log(p_min * to_thz).sum() - np.log(p_sad * to_thz).sum()))


# ------------------------------------------------------------------------------------------------ the driver
def vibrations_batch(engine, types, positions, masses, cells, pbcs, *, cutoff: float, delta: float = 0.01, nfree: int = 2,
                     indices=None, max_atoms_per_call: int = 32768, extra: Optional[Callable] = None,
                     make_extra: Optional[Callable] = None, n_atoms=None,
                     want_atomic_virial: bool = False) -> Tuple[List[Dict[str, Any]], Dict[str, int]]:
    """Finite-difference Hessians and harmonic spectra of B structures at once.

    engine: a HipForceEngine; types / positions / cells / pbcs / n_atoms as batch.build_batch_graph takes them; masses in amu,
    per system or flat.  delta: the displacement in A; nfree: 2 or 4 displacements per coordinate; indices: None, or per system
    None (all atoms), a bool mask or a list of the atoms that are displaced -- the Hessian is the [3m,3m] block of those atoms,
    the others are held fixed.  max_atoms_per_call: the most atoms the copies of one force call may hold.  The default, 32 768,
    is a third of the 97 336-atom cell the engine is benchmarked on, so its memory need is known to fit: it is a cap, not a
    tuned value.  extra: as batch.BatchForces, called over the COPY SLOTS (`plan_copies`: slot s is a copy of system
    plan.slot_system[s]); make_extra(slot_system) -> extra builds such a term once the slots are known.  The caller's arrays
    are not modified.

    Returns (results, info).  results[b]: the keys of SevenNetCalculator.compute_many for the undisplaced copy (the model's
    values; an `extra` term is not in them), which show whether the structure is at a stationary point -- except that the
    per-atom energies are `atomic_energies` here, because `energies` are the modes' -- plus `indices` [m],
    `hessian` [3m,3m] (eV/A^2), `asymmetry` (max |D - D^T| of the unsymmetrised differences: the noise floor of fp32 forces at
    this delta), `eigenvalues` [3m] of the mass-weighted Hessian (ascending, eV/(A^2 amu)), `modes` [3m,m,3] (row k belongs to
    eigenvalues[k]), `energies` (h nu in eV) and `frequencies` (cm^-1), both signed so that an imaginary mode is a negative
    number, `zpe` (eV) and `status`: 'ok' or 'failed' (a non-finite force: the Hessian and what follows from it are NaN).
    info: `n_force_calls`, `copies_evaluated` (the sum of nfree 3 m_b + 1) and `launches` (of the three kernels).  Invalid input
    raises ValueError before any device work."""
    types, positions, n_at, cells, pbcs = validate_batch_inputs(types, positions, cells, pbcs, cutoff, engine.spec.num_species, n_atoms)
    masses, selected = validate_vib_inputs(n_at, masses, indices, delta, nfree, max_atoms_per_call)
    check_extra(extra, make_extra)
    B = len(n_at)
    plan = plan_copies(n_at, selected, nfree, int(max_atoms_per_call))
    slot = plan.slot_system
    a_ptr = np.concatenate([[0], np.cumsum(n_at)])
    if make_extra is not None:
        extra = make_extra(slot)
    forces = BatchForces(engine, np.concatenate([types[a_ptr[b]:a_ptr[b + 1]] for b in slot]), n_at[slot], cells[slot], pbcs[slot],
                         cutoff, extra)
    base = BaseCopies(want_atomic_virial)
    H, Hm, asym, status, info = vib_loop(forces, plan, positions, n_at, selected, masses, delta=delta, keeper=base,
                                         want_atomic_virial=want_atomic_virial)
    base = base.results(n_at, cells, 'atomic_energies')
    results = []
    for b in range(B):
        res = base[b]
        ok = status[b] == 0
        res.update(indices=selected[b].copy(), hessian=H[b], asymmetry=float(asym[b]), status=VIB_STATUS_NAMES[0 if ok else 1])
        res.update(spectrum(Hm[b]))
        results.append(res)
    return results, info
