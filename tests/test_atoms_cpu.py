"""CPU: the ASE-like adapters (sevennet_amd.atoms) over a host class that records what it is called with."""
import numpy as np
import pytest

from sevennet_amd.atoms import ManyAtomsMixin, atoms_args


class _Atoms:
    def __init__(self, z, pos, cell, pbc, masses, vel=None):
        self.z, self.pos, self.cell, self.pbc, self.masses, self.vel = z, np.array(pos, float), cell, pbc, masses, vel

    def get_atomic_numbers(self):
        return np.asarray(self.z)

    def get_positions(self):
        return self.pos.copy()

    def get_cell(self):
        return np.asarray(self.cell, float)

    def get_pbc(self):
        return np.asarray(self.pbc, bool)

    def get_masses(self):
        return np.asarray(self.masses, float)

    def get_velocities(self):
        return self.vel

    def set_positions(self, pos):
        self.pos = np.array(pos, float)

    def set_velocities(self, vel):
        self.vel = np.array(vel, float)


class _Host(ManyAtomsMixin):
    """records the arguments of the three batched surfaces and returns canned dicts: system b moves to b + 1, velocity -b"""

    def __init__(self):
        self.calls = []

    def _canned(self, positions):
        return [{'energy': float(b), 'positions': np.full(np.shape(p), b + 1.0), 'velocities': np.full(np.shape(p), -float(b))}
                for b, p in enumerate(positions)]

    def compute_many(self, numbers, positions, cells, pbcs):
        self.calls.append(('compute_many', (numbers, positions, cells, pbcs), {}))
        return self._canned(positions)

    def relax_many(self, numbers, positions, cells, pbcs, **kw):
        self.calls.append(('relax_many', (numbers, positions, cells, pbcs), kw))
        return self._canned(positions)

    def md_many(self, numbers, positions, masses, cells, pbcs, dt, steps, **kw):
        self.calls.append(('md_many', (numbers, positions, masses, cells, pbcs, dt, steps), kw))
        return self._canned(positions)


def _atoms(with_velocities=True):
    v = (lambda n: np.full((n, 3), 0.01 * n)) if with_velocities else (lambda n: None)
    return [_Atoms([14, 8], [[0.0, 0, 0], [1.2, 0, 0]], np.eye(3) * 6.0, [True] * 3, [28.0855, 15.999], v(2)),
            _Atoms([1], [[0.1, 0.2, 0.3]], np.zeros((3, 3)), [False] * 3, [1.008], v(1)),
            _Atoms([8, 1, 1], np.arange(9.0).reshape(3, 3), np.diag([5.0, 5.0, 9.0]), [True, True, False], [15.999, 1.008, 1.008], v(3))]


def _same_args(got, want):
    assert len(got) == len(want)
    for g, w in zip(got[:2], want[:2]):
        assert len(g) == len(w) and all(np.array_equal(x, y) for x, y in zip(g, w))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


def test_atoms_args_shapes_and_dtypes():
    atoms = _atoms()
    for B in (3, 1):
        numbers, positions, cells, pbcs = atoms_args(iter(atoms[:B]))
        assert cells.shape == (B, 3, 3) and cells.dtype == np.float64 and pbcs.shape == (B, 3) and pbcs.dtype == bool
        assert [n.tolist() for n in numbers] == [a.z for a in atoms[:B]]
        assert all(np.array_equal(p, a.pos) for p, a in zip(positions, atoms))
    assert np.array_equal(cells[0], np.eye(3) * 6.0) and atoms_args(atoms)[3].tolist()[2] == [True, True, False]


def test_calculate_many_passes_the_atoms_args_through():
    host, atoms = _Host(), _atoms()
    res = host.calculate_many(atoms)
    (name, args, kw), = host.calls
    assert name == 'compute_many' and kw == {} and [r['energy'] for r in res] == [0.0, 1.0, 2.0]
    _same_args(args, atoms_args(atoms))


def test_relax_many_atoms_writes_each_systems_positions_back():
    host, atoms = _Host(), _atoms()
    before = atoms_args(atoms)
    res = host.relax_many_atoms(iter(atoms), fmax=0.01, steps=7, repack_below=0.25)
    (name, args, kw), = host.calls
    assert name == 'relax_many' and kw == dict(fmax=0.01, steps=7, repack_below=0.25)
    _same_args(args, before)
    assert isinstance(res, list) and len(res) == 3
    for b, a in enumerate(atoms):
        assert np.array_equal(a.pos, np.full((len(a.z), 3), b + 1.0)) and res[b]['positions'] is not a.pos


def test_md_many_atoms_passes_masses_and_velocities_and_writes_both_back():
    host, atoms = _Host(), _atoms()
    before, vel = atoms_args(atoms), [a.vel.copy() for a in atoms]
    res = host.md_many_atoms(atoms, 0.5, 4, temperature=300.0)
    (name, args, kw), = host.calls
    assert name == 'md_many' and args[5:] == (0.5, 4) and set(kw) == {'temperature', 'velocities'} and kw['temperature'] == 300.0
    _same_args(args[:2] + args[3:5], before)
    assert all(np.array_equal(m, a.masses) for m, a in zip(args[2], atoms)) and len(args[2]) == 3
    assert all(np.array_equal(v, w) and v.dtype == np.float64 for v, w in zip(kw['velocities'], vel))
    for b, a in enumerate(atoms):
        assert np.array_equal(a.pos, np.full((len(a.z), 3), b + 1.0)) and np.array_equal(a.vel, np.full((len(a.z), 3), -float(b)))
    assert len(res) == 3
    # one object without velocities: none are passed; the caller's own take precedence
    host, atoms = _Host(), _atoms()
    atoms[1].vel = None
    host.md_many_atoms(atoms, 0.5, 4, temperature=300.0)
    assert 'velocities' not in host.calls[0][2]
    given = [np.zeros((2, 3)), np.zeros((1, 3)), np.zeros((3, 3))]
    host.md_many_atoms(_atoms(), 0.5, 4, velocities=given)
    assert host.calls[1][2]['velocities'] is given


def test_md_many_atoms_refuses_ase_objects_without_explicit_velocities():
    FromAse = type('Atoms', (_Atoms,), {'__module__': 'ase.atoms'})
    atoms = _atoms()
    atoms[2] = FromAse(atoms[2].z, atoms[2].pos, atoms[2].cell, atoms[2].pbc, atoms[2].masses, atoms[2].vel)
    host = _Host()
    with pytest.raises(ValueError, match='system 2 is an ase object'):
        host.md_many_atoms(atoms, 0.5, 4, temperature=300.0)
    assert host.calls == []
    host.md_many_atoms(atoms, 0.5, 4, velocities=[np.zeros((2, 3)), np.zeros((1, 3)), np.zeros((3, 3))])
    assert host.calls[0][0] == 'md_many' and np.array_equal(atoms[2].vel, np.full((3, 3), -2.0))
