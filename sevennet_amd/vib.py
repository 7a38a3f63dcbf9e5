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

from types import SimpleNamespace
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .batch import BatchForces, _as_host, validate_batch_inputs, virial_to_stress
from .md import ACC

HBAR = 0.6582119569        # eV fs
INV_CM = 8065.543937       # cm^-1 per eV
VIB_STATUS_NAMES = ('ok', 'failed')
STENCIL = {2: (-1, 1), 4: (-2, -1, 1, 2)}   # the multipliers q of a row group, in the order of its copies


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


def plan_copies(n_atoms, selected: Optional[Sequence[np.ndarray]], nfree: int, max_atoms_per_call: int,
                n_groups: Optional[Sequence[int]] = None) -> SimpleNamespace:
    """The copies of B systems packed into calls (a pure function of its arguments).  n_atoms [B]; selected[b]: the displaced
    atoms of system b (indices within the system).  System b has 3 m_b ROW GROUPS -- the nfree copies of one (atom a, axis i), in
    the order of STENCIL[nfree] -- and one undisplaced copy.  Row groups are never split; a call holds at most
    `max_atoms_per_call` atoms unless it holds a single item (one row group, or one undisplaced copy: a system larger than the
    budget still runs); every (system, atom, axis, q) is planned exactly once.

    The force call sees COPY SLOTS as its systems: system b owns nfree g_b + 1 of them (g_b row groups and the undisplaced copy),
    with g_b = ceil(3 m_b / K) for the smallest number of calls K whose slots all fit the budget at once, so that slot counts are
    proportional to the systems' work, the systems finish together and all but the last calls use the same slots (a term planned
    per slot layout, d3.D3DeviceTerm, is then planned once and again where the layout thins out).  Where not even one row group
    per system fits, g_b = 1 and a call takes the systems that fit, in order.

    -> plan with `slot_system` int64 [S] (the system of each slot), `n_groups` [B] and `calls`: a list of namespaces with `ids`
    int64 [c] (the slots of the call's copies, ascending), `desc` int32 [c,4] (system, atom, axis, q per copy), `groups` int32
    [g,3] (first copy within the call, system, row r = 3 (position of a in selected[b]) + i) and `base` (pairs (copy within the
    call, system) of the undisplaced copies).

    n_groups [B]: the number of row groups of each system where they are not the coordinates of selected atoms (the six strain
    patterns of elastic.py).  `selected` is then not read, row r of system b is an index 0 .. n_groups[b] - 1 of the caller's, and
    the descriptor of its copies is (system, r, 0, q)."""
    n = np.asarray(n_atoms, np.int64).reshape(-1)
    B = len(n)
    qs = STENCIL[nfree]
    G = np.array([3 * len(s) for s in selected], np.int64) if n_groups is None else np.array(n_groups, np.int64).reshape(-1)
    budget = int(max_atoms_per_call)
    g = np.ones(B, np.int64)
    lo, hi = 1, int(G.max())   # the smallest K whose slots fit (the slots' atom count does not grow with K)
    fits = lambda K: int((n * (nfree * -(-G // K) + 1)).sum()) <= budget   # noqa: E731
    if fits(hi):
        while lo < hi:
            mid = (lo + hi) // 2
            if fits(mid):
                hi = mid
            else:
                lo = mid + 1
        g = -(-G // lo)
    slot0 = np.concatenate([[0], np.cumsum(nfree * g + 1)])
    slot_system = np.repeat(np.arange(B), nfree * g + 1)
    pending, next_row, base_done = G.copy(), np.zeros(B, np.int64), np.zeros(B, bool)
    calls = []
    while (pending > 0).any() or not base_done.all():
        ids, desc, groups, base = [], [], [], []
        used = n_items = 0
        for b in range(B):
            if pending[b] > 0:
                t = int(min(g[b], pending[b], (budget - used) // (nfree * n[b])))
                if t <= 0 and n_items == 0:
                    t = 1
                for k in range(max(t, 0)):
                    r = int(next_row[b]) + k
                    groups.append((len(desc), b, r))
                    for w, q in enumerate(qs):
                        ids.append(slot0[b] + nfree * k + w)
                        desc.append((b, int(selected[b][r // 3]), r % 3, q) if n_groups is None else (b, r, 0, q))
                if t > 0:
                    used += t * nfree * int(n[b])
                    n_items += t
                    pending[b] -= t
                    next_row[b] += t
            if pending[b] == 0 and not base_done[b] and (used + n[b] <= budget or n_items == 0):
                base.append((len(desc), b))
                ids.append(slot0[b] + nfree * g[b])
                desc.append((b, 0, 0, 0))
                used += int(n[b])
                n_items += 1
                base_done[b] = True
        calls.append(SimpleNamespace(ids=np.asarray(ids, np.int64), desc=np.asarray(desc, np.int32).reshape(-1, 4),
                                     groups=np.asarray(groups, np.int32).reshape(-1, 3), base=base, n_atoms=used))
    return SimpleNamespace(slot_system=slot_system, n_groups=G, calls=calls, nfree=nfree)


# ------------------------------------------------------------------------------------------------ launches
def vib_displace(pos0: torch.Tensor, seg_ptr0: torch.Tensor, desc: torch.Tensor, copy_ptr: torch.Tensor, delta: float,
                 pos_out: torch.Tensor, status: torch.Tensor) -> None:
    """one `snet_vib_displace` launch on the current stream (dtypes as the C ABI: pos0 / pos_out fp64, the rest int32)"""
    n0, n_sys, n_copies, n_out = int(pos0.shape[0]), int(seg_ptr0.numel()) - 1, int(desc.shape[0]), int(pos_out.shape[0])
    f64, i32 = torch.float64, torch.int32
    _lib.check_device_tensors('vib_displace', pos0, [(pos0, f64, (n0, 3)), (seg_ptr0, i32, (n_sys + 1,)), (desc, i32, (n_copies, 4)),
                                                      (copy_ptr, i32, (n_copies + 1,)), (pos_out, f64, (n_out, 3)),
                                                      (status, i32, (n_copies,))])
    P = _lib.ptr
    with torch.cuda.device(pos0.device):
        _lib.check(_lib.load().snet_vib_displace(P(pos0), n0, P(seg_ptr0), n_sys, P(desc), P(copy_ptr), n_copies, float(delta),
                                                 P(pos_out), n_out, P(status), _lib.stream()), 'snet_vib_displace')


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
def vib_loop(forces, plan, positions, n_atoms, selected, masses, *, delta: float, on_call: Optional[Callable] = None,
             want_atomic_virial: bool = False):
    """The calls of a plan.  forces: a BatchForces over the copy slots of `plan` (plan.slot_system), or any object with its call
    interface (relax.fire_cell_loop documents it); positions: the flat base positions [sum n_b, 3]; n_atoms [B], selected and
    masses per system as `validate_vib_inputs` returns them.  Per call one `snet_vib_displace`, one force call and one
    `snet_vib_rows`, nothing read back; on_call(call, graph, output), if given, is called after each force call (the driver
    keeps the undisplaced copies' results with it; want_atomic_virial asks the calls that hold such a copy for the per-atom
    virial).  Then one `snet_vib_finish` and one transfer.
    -> (hessian, mass-weighted hessian: lists of [3 m_b, 3 m_b] fp64 arrays; asymmetry [B]; status [B] (0 ok, 2 a non-finite
    force, 3 a layout the kernels refused); info)"""
    dev = forces.engine.dev
    n = np.asarray(n_atoms, np.int64).reshape(-1)
    B, nfree = len(n), plan.nfree
    m = np.array([len(s) for s in selected], np.int64)
    d_off = np.concatenate([[0], np.cumsum(9 * m * m)])
    f64, i32 = torch.float64, torch.int32

    def up(a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a)).to(dev, dtype)

    with torch.cuda.device(dev):
        pos0 = (positions.to(dev, f64) if isinstance(positions, torch.Tensor)
                else torch.as_tensor(np.ascontiguousarray(positions, np.float64)).to(dev)).reshape(-1, 3).contiguous()
        seg0 = up(np.concatenate([[0], np.cumsum(n)]), i32)
        sel_d, sel_ptr = up(np.concatenate(selected), i32), up(np.concatenate([[0], np.cumsum(m)]), i32)
        w_d = up(np.concatenate([1.0 / np.sqrt(np.asarray(ms, np.float64)[s]) for ms, s in zip(masses, selected)]), f64)
        off_d = up(d_off[:-1], torch.int64)
        D = torch.zeros(int(d_off[-1]), dtype=f64, device=dev)
        status = torch.zeros(B, dtype=i32, device=dev)
        refused = []
        for call in plan.calls:
            copy_ptr = np.concatenate([[0], np.cumsum(n[call.desc[:, 0]])])
            pos = torch.empty(int(copy_ptr[-1]), 3, dtype=f64, device=dev)
            st = torch.zeros(len(call.ids), dtype=i32, device=dev)
            vib_displace(pos0, seg0, up(call.desc, i32), up(copy_ptr, i32), delta, pos, st)
            refused.append(st)
            g, out, fx, _ = forces(pos, call.ids, want_atomic_virial=want_atomic_virial and bool(call.base))
            if on_call is not None:
                on_call(call, g, out)
            if len(call.groups):
                vib_rows(out['forces'], fx, g.seg_ptr, up(call.groups, i32), nfree, delta, sel_d, sel_ptr, off_d, D, status)
        H, Hm, asym = torch.empty_like(D), torch.empty_like(D), torch.empty(B, dtype=f64, device=dev)
        vib_finish(D, off_d, sel_ptr, w_d, status, H, Hm, asym)
        flat = torch.cat([H, Hm, asym, status.to(f64), torch.cat(refused).sum().to(f64).reshape(1)]).cpu().numpy()   # the one transfer
    if flat[-1] != 0:
        raise RuntimeError(f'snet_vib_displace refused {int(flat[-1])} copies of the plan: its descriptors do not fit the systems')
    size = int(d_off[-1])
    cut = lambda a: [a[d_off[b]:d_off[b + 1]].reshape(3 * m[b], 3 * m[b]).copy() for b in range(B)]   # noqa: E731
    n_rows_calls = sum(1 for c in plan.calls if len(c.groups))
    info = dict(n_force_calls=forces.n_force_calls, copies_evaluated=int(sum(len(c.ids) for c in plan.calls)),
                launches=len(plan.calls) + n_rows_calls + 1)
    return (cut(flat[:size]), cut(flat[size:2 * size]), flat[2 * size:2 * size + B].copy(),
            flat[2 * size + B:2 * size + 2 * B].astype(np.int64), info)


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
    if extra is not None and make_extra is not None:
        raise ValueError('pass `extra` or `make_extra`, not both')
    B = len(n_at)
    plan = plan_copies(n_at, selected, nfree, int(max_atoms_per_call))
    slot = plan.slot_system
    a_ptr = np.concatenate([[0], np.cumsum(n_at)])
    if make_extra is not None:
        extra = make_extra(slot)
    forces = BatchForces(engine, np.concatenate([types[a_ptr[b]:a_ptr[b + 1]] for b in slot]), n_at[slot], cells[slot], pbcs[slot],
                         cutoff, extra)
    kept = []   # per call with undisplaced copies: (systems, device tensors of their results)

    def keep_base(call, g, out):
        if not call.base:
            return
        dev = out['forces'].device
        sp = g.seg_ptr_host
        copies = np.array([j for j, _ in call.base], np.int64)
        rows = torch.as_tensor(np.concatenate([np.arange(sp[j], sp[j + 1]) for j in copies])).to(dev)
        j_d = torch.as_tensor(copies).to(dev)
        rp = g.row_ptr.long()
        took = dict(energy=out['energy_per_system'][j_d].clone(), virial=out['virial_per_system'][j_d].clone(),
                    forces=out['forces'][rows].clone(), energies=out['atomic_energy'][rows].clone(),
                    n_edges=rp[torch.as_tensor(sp[copies + 1]).to(dev)] - rp[torch.as_tensor(sp[copies]).to(dev)])
        if want_atomic_virial:
            took['stresses'] = out['atomic_virial'][rows].clone()
        kept.append(([b for _, b in call.base], took))

    H, Hm, asym, status, info = vib_loop(forces, plan, positions, n_at, selected, masses, delta=delta, on_call=keep_base,
                                         want_atomic_virial=want_atomic_virial)
    base: List[Optional[Dict[str, Any]]] = [None] * B
    for systems, took in kept:
        host = {k: v.cpu().numpy() for k, v in took.items()}
        stress = virial_to_stress(host['virial'], cells[systems])
        r0 = 0
        for k, b in enumerate(systems):
            r1 = r0 + int(n_at[b])
            res = {'free_energy': float(host['energy'][k]), 'energy': float(host['energy'][k]),
                   'atomic_energies': host['energies'][r0:r1].astype(np.float64), 'forces': host['forces'][r0:r1].astype(np.float64),
                   'stress': stress[k], 'num_edges': int(host['n_edges'][k])}
            if want_atomic_virial:
                res['stresses'] = host['stresses'][r0:r1]
            base[b] = res
            r0 = r1
    results = []
    for b in range(B):
        res = dict(base[b])
        ok = status[b] == 0
        res.update(indices=selected[b].copy(), hessian=H[b], asymmetry=float(asym[b]), status=VIB_STATUS_NAMES[0 if ok else 1])
        res.update(spectrum(Hm[b]))
        results.append(res)
    return results, info
