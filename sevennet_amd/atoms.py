"""The ASE-facing side of the calculators, once: the `Calculator` base (ASE's, or a stand-in where ASE is absent), the
arguments of the batched surfaces read from ASE-like objects, and the `*_atoms` adapters over them."""
from __future__ import annotations

from typing import Any, Dict, List

import numpy as np

from .fixed import constraints_fixed_list

try:  # ASE is optional: without it the calculators are plain objects that expose compute() and the batched surfaces
    from ase.calculators.calculator import Calculator, all_changes
    HAVE_ASE = True
except ImportError:  # pragma: no cover - depends on the environment
    HAVE_ASE = False
    all_changes = ['positions', 'numbers', 'cell', 'pbc']

    class Calculator:  # minimal stand-in with the attributes the calculators use
        def __init__(self, **kwargs):
            self.results: Dict[str, Any] = {}
            self.atoms = None

        def calculate(self, atoms=None, properties=None, system_changes=None):
            self.atoms = atoms


def atoms_args(atoms_list):
    """(numbers_list, positions_list, cells[B,3,3], pbcs[B,3]) of ASE-like objects (get_atomic_numbers / get_positions /
    get_cell / get_pbc)"""
    atoms_list = list(atoms_list)
    return ([a.get_atomic_numbers() for a in atoms_list], [a.get_positions() for a in atoms_list],
            np.array([np.array(a.get_cell(), np.float64).reshape(3, 3) for a in atoms_list]).reshape(-1, 3, 3),
            np.array([np.asarray(a.get_pbc(), bool).reshape(3) for a in atoms_list]).reshape(-1, 3))


def atoms_velocities(atoms_list, kw: dict) -> dict:
    """the keyword arguments of md_many for ASE-like objects: `velocities` from get_velocities() when the caller passed none
    and every object has some (an object without the method, or one that returns None, has none).  Objects of the ase package
    itself are refused unless the caller passes `velocities` (ValueError): their unit is not A/fs."""
    if kw.get('velocities') is not None:
        return kw
    for b, a in enumerate(atoms_list):   # ASE's velocity unit is A / (10.18 fs): read as A/fs it would be wrong tenfold, silently
        if type(a).__module__.split('.')[0] == 'ase':
            raise ValueError(f'system {b} is an ase object, whose velocities are in ASE units, not A/fs: pass velocities= in A/fs '
                             '(get_velocities() * ase.units.fs) explicitly, and divide what is written back by ase.units.fs')
    vels = [a.get_velocities() if hasattr(a, 'get_velocities') else None for a in atoms_list]
    if any(v is None for v in vels):
        return kw
    return dict(kw, velocities=[np.asarray(v, np.float64) for v in vels])


def atoms_fixed(atoms_list, kw: dict) -> dict:
    """the keyword arguments of relax_many / md_many for ASE-like objects: `fixed_list` from the objects' `constraints` (FixAtoms,
    FixCartesian; fixed.constraints_fixed_list) when the caller passed none and some object holds something.  Objects without
    constraints leave kw as it is; a constraint of another kind raises ValueError."""
    if kw.get('fixed_list') is not None:
        return kw
    fixed_list = constraints_fixed_list(atoms_list)
    return kw if fixed_list is None else dict(kw, fixed_list=fixed_list)


class ManyAtomsMixin:
    """`calculate_many`, `relax_many_atoms`, `neb_many_atoms`, `vibrations_many_atoms`, `phonons_many_atoms`, `elastic_many_atoms` and
    `md_many_atoms` over ASE-like objects, for a class that has `compute_many`, `relax_many`, `neb_many`, `vibrations_many`,
    `phonons_many`, `elastic_many` and `md_many` (a class without the latter six inherits adapters that fail where they are called)"""

    def calculate_many(self, atoms_list) -> List[Dict[str, Any]]:
        """`compute_many` over ASE-like objects (anything with get_atomic_numbers / get_positions / get_cell / get_pbc)"""
        return self.compute_many(*atoms_args(atoms_list))

    def relax_many_atoms(self, atoms_list, fmax: float = 0.05, steps: int = 500, **kw) -> List[Dict[str, Any]]:
        """`relax_many` over ASE-like objects (get_atomic_numbers / get_positions / get_cell / get_pbc / set_positions): the
        relaxed positions are written back with `set_positions`; with relax_cell=True the relaxed cell first, with
        `set_cell(cell, scale_atoms=False)`.  Without a `fixed_list` of the caller's the objects' `constraints` are read:
        FixAtoms and FixCartesian become the `fixed_list` of `relax_many`, any other constraint raises ValueError (it is not
        dropped: the object would end up in a state no calculation produced)."""
        atoms_list = list(atoms_list)
        kw = atoms_fixed(atoms_list, kw)
        results = self.relax_many(*atoms_args(atoms_list), fmax=fmax, steps=steps, **kw)
        for a, r in zip(atoms_list, results):
            if kw.get('relax_cell'):
                a.set_cell(r['cell'], scale_atoms=False)
            a.set_positions(r['positions'])
        return results

    def neb_many_atoms(self, bands, fmax: float = 0.05, steps: int = 500, **kw) -> List[Dict[str, Any]]:
        """`neb_many` over ASE-like objects: bands[b] is the list of a band's images (get_atomic_numbers / get_positions /
        get_cell / get_pbc / set_positions), at least three.  Numbers, cell and pbc come from the band's first object; the
        positions of the interior images are written back with `set_positions`, the endpoints are left untouched."""
        bands = [list(band) for band in bands]
        if any(len(band) == 0 for band in bands):
            raise ValueError(f'band {[len(band) for band in bands].index(0)}: no images')
        numbers, _, cells, pbcs = atoms_args([band[0] for band in bands])
        results = self.neb_many(numbers, [np.stack([np.asarray(a.get_positions(), np.float64) for a in band]) for band in bands],
                                cells, pbcs, fmax=fmax, steps=steps, **kw)
        for band, r in zip(bands, results):
            for a, image in zip(band[1:-1], r['images'][1:-1]):
                a.set_positions(image['positions'])
        return results

    def vibrations_many_atoms(self, atoms_list, **kw) -> List[Dict[str, Any]]:
        """`vibrations_many` over ASE-like objects (get_atomic_numbers / get_positions / get_masses / get_cell / get_pbc);
        nothing is written back to them"""
        atoms_list = list(atoms_list)
        numbers, positions, cells, pbcs = atoms_args(atoms_list)
        return self.vibrations_many(numbers, positions, [a.get_masses() for a in atoms_list], cells, pbcs, **kw)

    def phonons_many_atoms(self, atoms_list, supercells, **kw) -> List[Dict[str, Any]]:
        """`phonons_many` over ASE-like objects holding the primitive cells (get_atomic_numbers / get_positions / get_masses /
        get_cell / get_pbc); nothing is written back to them"""
        atoms_list = list(atoms_list)
        numbers, positions, cells, pbcs = atoms_args(atoms_list)
        return self.phonons_many(numbers, positions, [a.get_masses() for a in atoms_list], cells, pbcs, supercells, **kw)

    def elastic_many_atoms(self, atoms_list, **kw) -> List[Dict[str, Any]]:
        """`elastic_many` over ASE-like objects (get_atomic_numbers / get_positions / get_cell / get_pbc); nothing is written
        back to them"""
        return self.elastic_many(*atoms_args(atoms_list), **kw)

    def md_many_atoms(self, atoms_list, dt: float, steps: int, **kw) -> List[Dict[str, Any]]:
        """`md_many` over ASE-like objects (get_atomic_numbers / get_positions / get_masses / get_cell / get_pbc, and
        get_velocities where the object has velocities): positions and velocities are written back with `set_positions` /
        `set_velocities`; with `pressure=` (constant-pressure MD) the cell first, with `set_cell(cell, scale_atoms=False)`.
        Velocities at this surface are in A/fs, read and written as they are.  ASE's own time unit is
        A sqrt(amu / eV) = 10.1805 fs, so the velocities of a real ase.Atoms are in A / (10.1805 fs): multiply
        get_velocities() by ase.units.fs (0.0982269) on the way in and divide by it on the way out, or pass
        `velocities=` in A/fs yourself (it takes precedence over the objects').  Because the mistake would be silent, objects of
        the ase package are refused (ValueError) unless `velocities=` is passed.  Without a `fixed_list` of the caller's the
        objects' `constraints` are read as in `relax_many_atoms`."""
        atoms_list = list(atoms_list)
        kw = atoms_fixed(atoms_list, kw)
        numbers, positions, cells, pbcs = atoms_args(atoms_list)
        results = self.md_many(numbers, positions, [a.get_masses() for a in atoms_list], cells, pbcs, dt, steps,
                               **atoms_velocities(atoms_list, kw))
        for a, r in zip(atoms_list, results):
            if kw.get('pressure') is not None:
                a.set_cell(r['cell'], scale_atoms=False)
            a.set_positions(r['positions'])
            a.set_velocities(r['velocities'])
        return results
