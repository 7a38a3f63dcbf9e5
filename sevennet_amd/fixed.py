"""Atoms and Cartesian components held fixed in `relax_many` and `md_many`: the one parser of `fixed_list`, and what the drivers
derive from its masks.

A mask is the `hold` array of the `*_fixed` step kernels (include/snet_hip.h, snet_fire_step_fixed): int32 [N], bit k (k = 0, 1,
2) of a word says that Cartesian component k of that atom is held, so 7 holds the whole atom.  `neb_many` keeps its own
`fixed_list` of whole atoms (neb._check_bands), which ends in the 0/1 `fixed` array of snet_neb_forces."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

WHOLE_ATOM = 7


def _system_mask(f, n: int, b: int) -> np.ndarray:
    """one entry of fixed_list -> int32 [n]; ValueError names the system"""
    if f is None:
        return np.zeros(n, np.int32)
    f = f.detach().cpu().numpy() if hasattr(f, 'detach') else np.asarray(f)   # (a torch tensor, or anything numpy reads)
    if f.dtype == object:
        raise ValueError(f'system {b}: fixed atoms are given as a bool mask of shape ({n},) or ({n}, 3) or a list of atom indices, '
                         'got an array of objects')
    if f.dtype == bool:
        if f.shape == (n,):
            return np.where(f, WHOLE_ATOM, 0).astype(np.int32)
        if f.shape == (n, 3):
            return (f.astype(np.int32) << np.arange(3, dtype=np.int32)).sum(1).astype(np.int32)
        raise ValueError(f'system {b}: a fixed mask of shape ({n},) (whole atoms) or ({n}, 3) (components) is required, got {f.shape}')
    if f.size and (not np.issubdtype(f.dtype, np.integer) or f.ndim != 1):
        raise ValueError(f'system {b}: fixed atoms are given as a bool mask of shape ({n},) or ({n}, 3) or a list of atom indices')
    f = f.astype(np.int64).reshape(-1)
    bad = (f < 0) | (f >= n)
    if bad.any():
        raise ValueError(f'system {b}: fixed atom index {int(f[bad][0])} is out of range (the system has {n} atoms)')
    mask = np.zeros(n, np.int32)
    mask[f] = WHOLE_ATOM
    return mask


def hold_masks(fixed_list, n_atoms) -> Optional[np.ndarray]:
    """fixed_list (None, or per system: None, a bool mask [n] of whole atoms, a bool mask [n,3] of components, or an integer index
    list of whole atoms) for systems of n_atoms [B] atoms -> the `hold` array int32 [N] of the step kernels, or None when nothing
    is held (the drivers then take the path without a mask).  A wrong length, a wrong shape, an index out of range or an object
    dtype raises ValueError naming the system."""
    if fixed_list is None:
        return None
    n_atoms = np.asarray(n_atoms, np.int64).reshape(-1)
    if not isinstance(fixed_list, (list, tuple)):
        raise ValueError(f'fixed_list: a list with one entry per system ({len(n_atoms)}) is required, got {type(fixed_list).__name__}')
    if len(fixed_list) != len(n_atoms):
        raise ValueError(f'fixed_list has {len(fixed_list)} entries but there are {len(n_atoms)} systems')
    parts = [_system_mask(f, int(n), b) for b, (f, n) in enumerate(zip(fixed_list, n_atoms))]
    hold = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    return hold if hold.any() else None


def held_components(hold: np.ndarray) -> np.ndarray:
    """hold int32 [N] -> bool [N,3]: component k of atom i is held"""
    return ((np.asarray(hold, np.int32)[:, None] >> np.arange(3, dtype=np.int32)) & 1).astype(bool)


def check_whole_atoms(hold: np.ndarray, n_atoms) -> None:
    """ValueError naming the first system whose mask holds some but not all components of an atom (what relax_cell refuses)"""
    partial = (hold & WHOLE_ATOM != 0) & (hold & WHOLE_ATOM != WHOLE_ATOM)
    if partial.any():
        a_ptr = np.concatenate([[0], np.cumsum(np.asarray(n_atoms, np.int64))])
        i = int(np.nonzero(partial)[0][0])
        b = int(np.searchsorted(a_ptr, i, side='right') - 1)
        raise ValueError(f'system {b}: relax_cell holds whole atoms only, and atom {i - int(a_ptr[b])} has some of its components '
                         'held: the rule of a held atom under a moving cell (fixed fractional coordinates, as ASE\'s UnitCellFilter '
                         'with FixAtoms) has no clean per-component form under a sheared deformation gradient')


def attach_fixed(results: List[dict], hold: np.ndarray, seg_ptr_host) -> List[dict]:
    """`fixed` (bool [n,3]) into each system's results dict"""
    comp = held_components(hold)
    for b, res in enumerate(results):
        res['fixed'] = comp[int(seg_ptr_host[b]):int(seg_ptr_host[b + 1])].copy()
    return results


def constraints_fixed_list(atoms_list) -> Optional[list]:
    """the `fixed_list` of ASE-like objects, from their `constraints` (read through `todict()`, ASE's own serialisation):
    {'name': 'FixAtoms', 'kwargs': {'indices': ...}} holds whole atoms, {'name': 'FixCartesian', 'kwargs': {'a': ..., 'mask': ...}}
    the components of atoms `a` whose mask entry is true; several constraints on one object add up.  None when no object has a
    constraint.  Any other constraint raises ValueError naming it: dropping it silently would relax or integrate another system
    than the one the caller described."""
    out, any_held = [], False
    for b, atoms in enumerate(atoms_list):
        cons = getattr(atoms, 'constraints', None)
        if cons is None:
            cons = []
        elif not isinstance(cons, (list, tuple)):
            cons = [cons]
        if len(cons) == 0:
            out.append(None)
            continue
        n = len(np.asarray(atoms.get_atomic_numbers()).reshape(-1))
        mask = np.zeros((n, 3), bool)
        for c in cons:
            d = c.todict() if hasattr(c, 'todict') else None
            name = d.get('name') if isinstance(d, dict) else None
            kwargs = d.get('kwargs', {}) if isinstance(d, dict) else {}
            if name == 'FixAtoms':
                idx, comp = kwargs.get('indices'), np.ones(3, bool)
            elif name == 'FixCartesian':
                idx, comp = kwargs.get('a'), np.asarray(kwargs.get('mask', (True, True, True)))
            else:
                raise ValueError(f'system {b}: constraint {name or type(c).__name__!r} is not supported (FixAtoms and FixCartesian are); '
                                 'remove it, or pass fixed_list= to say which components are held')
            idx = np.asarray(idx)
            if idx.dtype == bool and idx.shape == (n,):
                idx = np.nonzero(idx)[0]
            idx = idx.reshape(-1)
            if idx.size and not np.issubdtype(idx.dtype, np.integer):
                raise ValueError(f'system {b}: constraint {name}: atom indices are required, got dtype {idx.dtype}')
            idx = idx.astype(np.int64)
            if ((idx < -n) | (idx >= n)).any():
                raise ValueError(f'system {b}: constraint {name}: atom index {int(idx[(idx < -n) | (idx >= n)][0])} is out of range '
                                 f'(the system has {n} atoms)')
            if comp.dtype == object or comp.shape not in ((3,), (len(idx), 3)):
                raise ValueError(f'system {b}: constraint {name}: a mask of three flags is required, got shape {comp.shape}')
            np.logical_or.at(mask, idx, np.broadcast_to(comp.astype(bool), (len(idx), 3)))   # (an index may come twice)
        out.append(mask)
        any_held = any_held or bool(mask.any())
    return out if any_held else None
