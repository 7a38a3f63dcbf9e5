"""DFT-D3 dispersion for the ASE-level surface.

Mirrors sevenn.calculator.D3Calculator / SevenNetD3Calculator (sevenn/calculator.py:236-314, 387-618): same
constructor arguments (damping_type 'damp_bj' | 'damp_zero', functional_name, vdw_cutoff / cn_cutoff in bohr^2), same
result keys, units and signs -- over libsnet_hip.so's own HIP kernels (csrc/snet_d3.hip, C-ABI snet_d3_*).  The
published D3 tables travel as a data blob (sevennet_amd/data/d3_params.npz, written by oracle/tools/make_d3_params.py).
There is no CPU path: the reference needs CUDA for this term, this one needs a ROCm GPU."""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, List, NamedTuple

import numpy as np

from . import _lib
from .atoms import HAVE_ASE, Calculator, ManyAtomsMixin, all_changes
from .batch import _as_host, _normalize, system_of

AU_TO_ANG = 0.52917726
_BLOB = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'd3_params.npz')
_DAMPING = {'damp_zero': 0, 'damp_bj': 1}


def _dp(a):
    return C.c_void_p(a.ctypes.data)


def molecule_box(positions, cell, pbc, rthr: float, cnthr: float):
    """(cell [3,3], pbc [3]) that D3 evaluates: a cell that sums to zero becomes an orthogonal periodic box larger than the
    longest cutoff, extent + sqrt(max(rthr, cnthr)) bohr + 1 A (sevenn/calculator.py:533-548); any other cell is kept"""
    positions = np.asarray(positions, np.float64).reshape(-1, 3)
    cell = np.array(cell, np.float64).reshape(3, 3)
    pbc = np.asarray(pbc, bool).reshape(3)
    if cell.sum() == 0:
        max_cutoff = np.sqrt(max(rthr, cnthr)) * AU_TO_ANG
        cell = np.eye(3) * (positions.max(0) - positions.min(0) + max_cutoff + 1.0)
        pbc = np.array([True, True, True])
    return cell, pbc


class D3Batch(NamedTuple):
    """flat host inputs of snet_d3_compute_batch: system s owns atoms [atom_ptr[s], atom_ptr[s+1])"""
    atom_ptr: np.ndarray    # int64 [B+1]
    numbers: np.ndarray     # int32 [N]
    positions: np.ndarray   # float64 [N,3], A
    cells: np.ndarray       # float64 [B,3,3], A, after the molecule box
    pbcs: np.ndarray        # int32 [B,3], after the molecule box


def prepare_d3_batch(numbers, positions, cells, pbcs, rthr: float, cnthr: float, n_atoms=None) -> D3Batch:
    """Host-side preparation of a D3 batch, with no device work.  numbers / positions: per-system sequences, or flat
    arrays together with n_atoms[B] (the shape rules of SevenNetCalculator.compute_many); cells[B,3,3] (rows = lattice
    vectors), pbcs[B,3] or one [3].  Applies `molecule_box` per system.  Raises ValueError on an empty batch or system,
    mismatched lengths, Z outside 1..94 and a cell that is singular after the box rule."""
    numbers, positions, n_at, cells, pbcs = _normalize(numbers, positions, cells, pbcs, n_atoms)
    numbers = _as_host(numbers, np.int64).reshape(-1)
    positions = np.ascontiguousarray(_as_host(positions, np.float64).reshape(-1, 3))
    atom_ptr = np.concatenate([[0], np.cumsum(n_at)]).astype(np.int64)
    if atom_ptr[-1] > 2 ** 31 - 1:
        raise ValueError(f'{int(atom_ptr[-1])} atoms: at most 2^31 - 1 in one D3 batch')
    bad = (numbers < 1) | (numbers > 94)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f'system {system_of(atom_ptr, i)}: Z = {int(numbers[i])} has no D3 parameters (Z = 1 .. 94)')
    B = len(n_at)
    cells_out, pbcs_out = np.empty((B, 3, 3)), np.empty((B, 3), np.int32)
    for b in range(B):
        cell, pbc = molecule_box(positions[atom_ptr[b]:atom_ptr[b + 1]], cells[b], pbcs[b], rthr, cnthr)
        if not abs(np.linalg.det(cell / AU_TO_ANG)) > 1e-12:   # the bound of snet_d3_compute (bohr^3)
            raise ValueError(f'system {b}: singular cell {cell.tolist()} (pbc {pbc.tolist()})')
        cells_out[b], pbcs_out[b] = cell, pbc
    return D3Batch(atom_ptr, np.ascontiguousarray(numbers, np.int32), positions, cells_out, pbcs_out)


class D3Plan(NamedTuple):
    """a plan of `D3Engine.plan` and the device tensors `D3Engine.compute_device` writes (overwritten by each call)"""
    atom_ptr: np.ndarray    # int64 [B+1], host
    cells_move: bool        # capacities leave room for one more repetition along every periodic axis
    energy: Any             # fp64 [B], eV
    forces: Any             # fp64 [N,3], eV/A
    virial: Any             # fp64 [B,6], the engine's convention (`stress_to_virial`)
    cn: Any                 # fp64 [N]
    volume: Any             # fp64 [B], A^3 (of the molecule box where that rule applies)
    status: Any             # int32 [B]: 1 = cell not finite, singular, or more lattice translations than the plan has room for


def stress_to_virial(stress, volume):
    """[..., 6] virial in the engine's convention -- order xx,yy,zz,xy,yz,zx, stress = -virial / volume: what
    `relax.fire_cell_step` adds to the model's `virial_per_system` -- from the D3 stress [..., 3, 3] (dE/d strain / volume,
    eV/A^3) and the volume(s) (A^3)"""
    s = np.asarray(stress, np.float64)
    six = np.stack([s[..., 0, 0], s[..., 1, 1], s[..., 2, 2], s[..., 0, 1], s[..., 1, 2], s[..., 2, 0]], axis=-1)
    return -six * np.asarray(volume, np.float64)[..., None]


class D3Engine:
    """thin handle over snet_d3_*: compute(numbers, positions, cell, pbc) -> energy, forces, stress (3x3, dE/d strain / V)"""

    def __init__(self, damping_type: str = 'damp_bj', functional_name: str = 'pbe', vdw_cutoff: float = 9000.0,
                 cn_cutoff: float = 1600.0, blob: str = _BLOB):
        self.damp_name, self.func_name = damping_type.lower(), functional_name.lower()
        if self.damp_name not in _DAMPING:
            raise ValueError('Error: Invalid damping type.')      # sevenn/calculator.py:424-425
        import torch
        if not torch.cuda.is_available():
            raise NotImplementedError('CPU + D3 is not implemented yet')     # :415-416
        z = np.load(blob)
        names = z[self.damp_name + '_names'].tolist()
        if self.func_name not in names:
            raise ValueError(f'Functional name unknown: {functional_name!r} for {self.damp_name} (known: {names})')
        func = np.ascontiguousarray(z[self.damp_name + '_params'][names.index(self.func_name)], np.float64)
        self.rthr, self.cnthr = float(vdw_cutoff), float(cn_cutoff)
        self.lib = _lib.load()
        self.handle = C.c_void_p()
        _lib.check(self.lib.snet_d3_create(C.byref(self.handle)), 'snet_d3_create')
        tabs = [np.ascontiguousarray(z[k], np.float64) for k in ('r0ab', 'c6ab', 'r2r4', 'rcov')]
        _lib.check(self.lib.snet_d3_set_tables(self.handle, _dp(tabs[0]), _dp(tabs[1]), tabs[1].shape[0], _dp(tabs[2]), _dp(tabs[3])),
                   'snet_d3_set_tables')
        _lib.check(self.lib.snet_d3_settings(self.handle, self.rthr, self.cnthr, _DAMPING[self.damp_name], _dp(func)), 'snet_d3_settings')

    def compute(self, numbers, positions, cell, pbc) -> Dict[str, Any]:
        import torch
        numbers = np.ascontiguousarray(numbers, np.int32)
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        cell, pbc = molecule_box(positions, cell, pbc, self.rthr, self.cnthr)
        n = len(numbers)
        _lib.check(self.lib.snet_d3_set_atoms(self.handle, n, _dp(numbers), _dp(positions)), 'snet_d3_set_atoms')
        cell_c = np.ascontiguousarray(cell)
        pbc_c = np.ascontiguousarray(pbc.astype(np.int32))
        _lib.check(self.lib.snet_d3_set_cell(self.handle, _dp(cell_c), _dp(pbc_c)), 'snet_d3_set_cell')
        _lib.check(self.lib.snet_d3_compute(self.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'snet_d3_compute')
        f = np.ctypeslib.as_array(self.lib.snet_d3_forces(self.handle), shape=(n, 3)).copy()
        s = np.ctypeslib.as_array(self.lib.snet_d3_stress(self.handle), shape=(3, 3)).copy()
        cn = np.ctypeslib.as_array(self.lib.snet_d3_coordination_numbers(self.handle), shape=(n,)).copy()
        return dict(energy=float(self.lib.snet_d3_energy(self.handle)), forces=f, stress=s, cn=cn)

    def compute_many(self, numbers_list, positions_list, cells, pbcs, n_atoms=None) -> List[Dict[str, Any]]:
        """`compute` for B systems in one snet_d3_compute_batch call (three kernel launches, one readback): one dict per
        system, in the given order, equal bit for bit to `compute` on that system.  Inputs as `prepare_d3_batch`."""
        import torch
        bt = prepare_d3_batch(numbers_list, positions_list, cells, pbcs, self.rthr, self.cnthr, n_atoms=n_atoms)
        B, N = len(bt.atom_ptr) - 1, len(bt.numbers)
        energy, forces, stress, cn = np.empty(B), np.empty((N, 3)), np.empty((B, 3, 3)), np.empty(N)
        _lib.check(self.lib.snet_d3_compute_batch(self.handle, B, _dp(bt.atom_ptr), _dp(bt.numbers), _dp(bt.positions),
                                                  _dp(bt.cells), _dp(bt.pbcs), _dp(energy), _dp(forces), _dp(stress), _dp(cn),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'snet_d3_compute_batch')
        ap = bt.atom_ptr
        return [dict(energy=float(energy[b]), forces=forces[ap[b]:ap[b + 1]], stress=stress[b], cn=cn[ap[b]:ap[b + 1]])
                for b in range(B)]

    def plan(self, numbers, n_atoms, cells, pbcs, cells_move: bool = False, device=None) -> 'D3Plan':
        """snet_d3_plan for B systems: numbers flat [N], n_atoms [B], cells [B,3,3] (A) and pbcs [B,3] (or one [3]) as the caller
        has them -- a cell that sums to zero marks a molecule, whose box `compute_device` forms from the positions of each call.
        Everything that depends on species and topology alone is prepared and uploaded here, once, and the capacity of each
        system's translation lists is fixed: exact for its cell, or, with cells_move, with every periodic axis' repetition count
        one larger.  -> the plan with its output tensors on `device` (default: the current GPU).  The engine holds ONE plan:
        planning again makes the earlier plan unusable.  ValueError on an empty batch or system, Z outside 1..94 and a singular
        cell."""
        import torch
        n_atoms = _as_host(n_atoms, np.int64).reshape(-1)
        numbers = np.ascontiguousarray(_as_host(numbers, np.int64).reshape(-1))
        B = len(n_atoms)
        if B == 0 or (n_atoms <= 0).any() or int(n_atoms.sum()) != len(numbers):
            raise ValueError(f'n_atoms {n_atoms.tolist()} (all positive) must sum to the {len(numbers)} atomic numbers')
        atom_ptr = np.concatenate([[0], np.cumsum(n_atoms)]).astype(np.int64)
        if atom_ptr[-1] > 2 ** 31 - 1:
            raise ValueError(f'{int(atom_ptr[-1])} atoms: at most 2^31 - 1 in one D3 batch')
        bad = (numbers < 1) | (numbers > 94)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise ValueError(f'system {system_of(atom_ptr, i)}: Z = {int(numbers[i])} has no D3 parameters (Z = 1 .. 94)')
        cells = np.ascontiguousarray(_as_host(cells, np.float64).reshape(B, 3, 3))
        pbcs = np.ascontiguousarray(np.broadcast_to(_as_host(pbcs, bool).reshape(-1, 3), (B, 3)).astype(np.int32))
        box = np.ascontiguousarray((cells.reshape(B, 9).sum(1) == 0).astype(np.int32))   # the rule of `molecule_box`
        for b in np.nonzero(box == 0)[0]:
            if not abs(np.linalg.det(cells[b] / AU_TO_ANG)) > 1e-12:
                raise ValueError(f'system {b}: singular cell {cells[b].tolist()} (pbc {pbcs[b].astype(bool).tolist()})')
        z32 = np.ascontiguousarray(numbers, np.int32)
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(dev):
            _lib.check(self.lib.snet_d3_plan(self.handle, B, _dp(atom_ptr), _dp(z32), _dp(cells), _dp(pbcs), _dp(box),
                                             int(bool(cells_move)), _lib.stream()), 'snet_d3_plan')
            f64, N = torch.float64, int(atom_ptr[-1])
            self._plan = D3Plan(atom_ptr, bool(cells_move), torch.empty(B, dtype=f64, device=dev), torch.empty(N, 3, dtype=f64, device=dev),
                                torch.empty(B, 6, dtype=f64, device=dev), torch.empty(N, dtype=f64, device=dev),
                                torch.empty(B, dtype=f64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
        return self._plan

    def compute_device(self, plan: 'D3Plan', positions, cells_dev=None) -> 'D3Plan':
        """snet_d3_compute_device on the current stream: the planned systems at `positions` (fp64 [N,3] on the plan's device,
        A) and, where given, `cells_dev` (fp64 [B,9] on the device, A; None: the plan's cells) into the plan's output tensors,
        which the next call overwrites.  Six launches; nothing is read back, nothing synchronises, nothing is allocated.
        Energy, forces and cn equal `compute_many` on the same inputs bit for bit; a system with status 1 (see `D3Plan`) holds
        NaN."""
        import torch
        if plan is not getattr(self, '_plan', None):
            raise ValueError('this plan has been replaced: a D3Engine holds one plan at a time (plan again)')
        B, N = len(plan.atom_ptr) - 1, int(plan.atom_ptr[-1])
        want = [(positions, torch.float64, (N, 3))] + ([] if cells_dev is None else [(cells_dev, torch.float64, (B, 9))])
        _lib.check_device_tensors('D3Engine.compute_device', plan.forces, want)
        P = _lib.ptr
        with torch.cuda.device(plan.forces.device):
            _lib.check(self.lib.snet_d3_compute_device(self.handle, P(positions), P(cells_dev), P(plan.energy), P(plan.forces),
                                                       P(plan.virial), P(plan.cn), P(plan.volume), P(plan.status), _lib.stream()),
                       'snet_d3_compute_device')
        return plan

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.lib.snet_d3_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class D3Term:
    """The D3 forces and energies as the `extra` of a batched driver (batch.BatchForces): one `D3Engine.compute_many` per
    call over the systems `ids` at the driver's positions.  numbers flat [N], n_atoms [B]; cells [B,3,3] and pbcs [B,3] (or one
    [3]) as the caller gave them -- the molecule box is applied by `compute_many`, from the positions of each call.  The batch is
    prepared on the host, so each call copies the positions down and the forces up.  `last`: the per-system results of the
    last call."""

    def __init__(self, d3_engine: D3Engine, numbers, n_atoms, cells, pbcs):
        self.engine = d3_engine
        self.numbers, self.n_atoms = _as_host(numbers, np.int64).reshape(-1), _as_host(n_atoms, np.int64).reshape(-1)
        B = len(self.n_atoms)
        self.a_ptr = np.concatenate([[0], np.cumsum(self.n_atoms)])
        self.cells = _as_host(cells, np.float64).reshape(B, 3, 3)
        self.pbcs = np.broadcast_to(_as_host(pbcs, bool).reshape(-1, 3), (B, 3))
        self.last: List[Dict[str, Any]] = []

    def __call__(self, pos, seg_ptr, ids):
        import torch
        z = np.concatenate([self.numbers[self.a_ptr[b]:self.a_ptr[b + 1]] for b in ids])
        self.last = self.engine.compute_many(z, pos.cpu().numpy(), self.cells[ids], self.pbcs[ids], n_atoms=self.n_atoms[ids])
        return (torch.as_tensor(np.concatenate([r['forces'] for r in self.last])).to(pos.device),
                torch.as_tensor(np.array([r['energy'] for r in self.last])).to(pos.device))


class D3DeviceTerm:
    """`D3Term` with the state on the device: the `extra` of a batched driver that reads the driver's positions (and, under a
    moving cell, its cells) where they are and returns (forces [N,3], energies [b], virial [b,6]) as device tensors -- one
    `D3Engine.compute_device` per call, no copy in either direction.  Built from the arguments of `D3Term`.  The engine is
    planned (`D3Engine.plan`) on the first call and again whenever `ids` changes (a repack of the batch); the returned tensors
    are the plan's, overwritten by the next call.  `provides_virial` marks the third element for batch.BatchForces, which then
    passes `cells_dev`; `status`: int32 [b] on the device, 1 for a system the last call could not evaluate (its forces,
    energy and virial are NaN, see `D3Plan`)."""

    provides_virial = True

    def __init__(self, d3_engine: D3Engine, numbers, n_atoms, cells, pbcs):
        self.engine = d3_engine
        self.numbers, self.n_atoms = _as_host(numbers, np.int64).reshape(-1), _as_host(n_atoms, np.int64).reshape(-1)
        B = len(self.n_atoms)
        self.a_ptr = np.concatenate([[0], np.cumsum(self.n_atoms)])
        self.cells = _as_host(cells, np.float64).reshape(B, 3, 3)
        self.pbcs = np.broadcast_to(_as_host(pbcs, bool).reshape(-1, 3), (B, 3))
        self._ids = self._plan = None
        self.n_plans = 0

    @property
    def status(self):
        return None if self._plan is None else self._plan.status

    def __call__(self, pos, seg_ptr, ids, cells_dev=None):
        ids = np.asarray(ids, np.int64)
        moving = cells_dev is not None
        if (self._plan is None or self._plan is not getattr(self.engine, '_plan', None) or self._plan.cells_move != moving
                or not np.array_equal(ids, self._ids)):
            z = np.concatenate([self.numbers[self.a_ptr[b]:self.a_ptr[b + 1]] for b in ids])
            self._plan = self.engine.plan(z, self.n_atoms[ids], self.cells[ids], self.pbcs[ids], cells_move=moving, device=pos.device)
            self._ids = ids.copy()
            self.n_plans += 1
        p = self.engine.compute_device(self._plan, pos, cells_dev)
        return p.forces, p.energy, p.virial


class D3Calculator(ManyAtomsMixin, Calculator):
    """ASE calculator for the D3 van der Waals correction (sevenn/calculator.py:387-618).
    implemented_properties and result conventions as the reference: free_energy = energy (eV), forces (eV/A),
    stress in ASE Voigt order xx, yy, zz, yz, xz, xy (eV/A^3)."""

    implemented_properties = ['free_energy', 'energy', 'forces', 'stress']

    def __init__(self, damping_type: str = 'damp_bj', functional_name: str = 'pbe', vdw_cutoff: float = 9000,
                 cn_cutoff: float = 1600, **kwargs) -> None:
        super().__init__(**kwargs)
        self.engine = D3Engine(damping_type, functional_name, vdw_cutoff, cn_cutoff)
        self.rthr, self.cnthr = self.engine.rthr, self.engine.cnthr
        self.damp_name, self.func_name = self.engine.damp_name, self.engine.func_name

    @staticmethod
    def _results(r) -> Dict[str, Any]:
        s = r['stress']
        return {'free_energy': r['energy'], 'energy': r['energy'], 'forces': r['forces'],
                'stress': np.array([s[0, 0], s[1, 1], s[2, 2], s[1, 2], s[0, 2], s[0, 1]])}

    def compute(self, numbers, positions, cell, pbc) -> Dict[str, Any]:
        return self._results(self.engine.compute(numbers, positions, cell, pbc))

    def compute_many(self, numbers_list, positions_list, cells, pbcs, n_atoms=None) -> List[Dict[str, Any]]:
        """`compute` for B systems in one D3Engine.compute_many call: one dict per system, in the given order"""
        return [self._results(r) for r in self.engine.compute_many(numbers_list, positions_list, cells, pbcs, n_atoms=n_atoms)]

    def calculate(self, atoms=None, properties=None, system_changes=all_changes):
        Calculator.calculate(self, atoms, properties, system_changes)
        if atoms is None:
            raise ValueError('No atoms to evaluate')
        if atoms.get_cell().sum() == 0:
            print('Warning: D3Calculator requires a cell.\nWarning: An orthogonal cell large enough is generated.')
        self.results = self.compute(atoms.get_atomic_numbers(), atoms.get_positions(), np.array(atoms.get_cell()), atoms.get_pbc())


def _d3_pair(model, file_type, device, modal, enable_cueq, enable_flash, enable_oeq, sevennet_config, damping_type,
             functional_name, vdw_cutoff, cn_cutoff, kwargs):
    import warnings
    from .calculator import SevenNetCalculator
    if kwargs.get('compute_atomic_virial', False):
        warnings.warn('D3Calculator does not support per-atom stress. Atomic stress from SevenNetD3Calculator will not '
                      'include D3 contributions.')
    d3_kwargs = {k: v for k, v in kwargs.items() if k != 'compute_atomic_virial'}
    d3_calc = D3Calculator(damping_type=damping_type, functional_name=functional_name, vdw_cutoff=vdw_cutoff,
                           cn_cutoff=cn_cutoff, **d3_kwargs)
    sevennet_calc = SevenNetCalculator(model=model, file_type=file_type, device=device, modal=modal, enable_cueq=enable_cueq,
                                       enable_flash=enable_flash, enable_oeq=enable_oeq, sevennet_config=sevennet_config, **kwargs)
    return sevennet_calc, d3_calc


if HAVE_ASE:
    from ase.calculators.mixing import SumCalculator as _SumBase
else:
    _SumBase = object


class SevenNetD3Calculator(ManyAtomsMixin, _SumBase):
    """SevenNet + D3 (sevenn/calculator.py:236-314: a SumCalculator subclass holding the two).  With ASE present this is an
    ase.calculators.mixing.SumCalculator subclass like the reference's; without it, `compute(numbers, positions, cell, pbc)`
    returns the summed results."""

    def __init__(self, model='7net-0', file_type: str = 'checkpoint', device='auto', modal=None, enable_cueq=False,
                 enable_flash=False, enable_oeq=False, sevennet_config=None, damping_type: str = 'damp_bj',
                 functional_name: str = 'pbe', vdw_cutoff: float = 9000, cn_cutoff: float = 1600, **kwargs):
        pair = _d3_pair(model, file_type, device, modal, enable_cueq, enable_flash, enable_oeq, sevennet_config, damping_type,
                        functional_name, vdw_cutoff, cn_cutoff, kwargs)
        if HAVE_ASE:
            super().__init__(list(pair))
        else:
            self.calcs = list(pair)
        self.relax_info = None   # counters of the last relax_many call
        self.md_info = None      # counters of the last md_many call
        self.neb_info = None     # counters of the last neb_many call
        self.vib_info = None     # counters of the last vibrations_many call
        self.phonon_info = None  # counters of the last phonons_many call
        self.elastic_info = None  # counters of the last elastic_many call

    @staticmethod
    def _sum(a, b) -> Dict[str, Any]:
        out = dict(a)
        for k in ('free_energy', 'energy', 'forces', 'stress'):
            out[k] = a[k] + b[k]
        return out

    def compute(self, numbers, positions, cell, pbc) -> Dict[str, Any]:
        a, b = (c.compute(numbers, positions, cell, pbc) for c in self.calcs)
        return self._sum(a, b)

    def compute_many(self, numbers_list, positions_list, cells, pbcs) -> List[Dict[str, Any]]:
        """`compute` for B structures: one SevenNetCalculator.compute_many and one D3Calculator.compute_many call, summed
        per system as `compute` sums them (cells[B,3,3], pbcs[B,3] or one [3])"""
        numbers_list, positions_list = list(numbers_list), list(positions_list)
        a, b = (c.compute_many(numbers_list, positions_list, cells, pbcs) for c in self.calcs)
        return [self._sum(x, y) for x, y in zip(a, b)]

    def _d3_term(self, numbers_list, positions_list, cells, pbcs, d3_term: str = 'host'):
        """the D3 side of a batched driver, validated on the host (Z range, cells after the box rule): a `D3Term`, or with
        d3_term = 'device' a `D3DeviceTerm`"""
        d3 = self.calcs[1]
        if len(numbers_list) != len(positions_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(positions_list)} position arrays')
        bt = prepare_d3_batch(numbers_list, positions_list, cells, pbcs, d3.rthr, d3.cnthr)
        return (D3DeviceTerm if d3_term == 'device' else D3Term)(d3.engine, bt.numbers, np.diff(bt.atom_ptr), cells, pbcs)

    @staticmethod
    def _check_d3_term(d3_term) -> None:
        if d3_term not in ('host', 'device'):
            raise ValueError(f"d3_term = {d3_term!r}: 'host' (the D3 batch is prepared on the host each step) or 'device' (the D3 "
                             'term stays on the device) is required')

    def relax_many(self, numbers_list, positions_list, cells, pbcs, fmax: float = 0.05, steps: int = 500, d3_term: str = 'host',
                   **kw) -> List[Dict[str, Any]]:
        """`SevenNetCalculator.relax_many` on the sum of the model's and the D3 forces (sevennet_amd.relax): one dict per
        system with the keys of `compute` plus `positions`, `converged` and `n_steps` (with relax_cell: `cell` and `status`); the
        results are `compute_many` at the returned positions (and cells), the counters are kept as `self.relax_info`.
        d3_term = 'host' (the default): `D3Engine.compute_many` prepares its batch on the host, so this path copies the
        positions down and the D3 forces up once per step (the model's forces and the optimizer state stay on the device).
        Fixed cells only: relax_cell=True raises ValueError, because the host term reaches the optimizer through the `extra`
        contract, which carries no virial.
        d3_term = 'device': the D3 term is a `D3DeviceTerm` -- planned once (and at each repack), evaluated from the driver's
        device positions, nothing copied per step.  It hands the optimizer a virial too, so relax_cell=True relaxes the cells
        under model + D3 (systems periodic along all three axes, at most batch.BATCH_MAX_ATOMS atoms, as for the model alone).
        The plan leaves each system's lattice sums room for one more repetition per axis than its starting cell needs; a cell
        that shrinks beyond that makes the D3 virial NaN, which the step kernel refuses: the system comes back as it was
        before that step with status 'cell_failed'.
        fixed_list (SevenNetCalculator.relax_many) goes through with either d3_term: the masked step ignores the model's and the
        D3 forces alike on held components, and the summed `forces` of the results stay the true ones."""
        self._check_d3_term(d3_term)
        if kw.get('relax_cell') and d3_term == 'host':
            raise ValueError("relax_cell is not available with d3_term='host': that D3 term reaches the optimizer through the `extra` "
                             "contract, which carries forces and energies but no virial, so its cell force is unknown (pass "
                             "d3_term='device', whose term carries one)")
        snet, d3 = self.calcs
        numbers_list, positions_list = list(numbers_list), list(positions_list)
        term = self._d3_term(numbers_list, positions_list, cells, pbcs, d3_term)
        results = snet.relax_many(numbers_list, positions_list, cells, pbcs, fmax=fmax, steps=steps, extra=term, **kw)
        self.relax_info = snet.relax_info
        final_cells = np.stack([r['cell'] for r in results]) if kw.get('relax_cell') else cells
        at_final = d3.compute_many(numbers_list, [r['positions'] for r in results], final_cells, pbcs)
        return [self._sum(a, b) for a, b in zip(results, at_final)]

    def neb_many(self, numbers_list, images_list, cells, pbcs, fmax: float = 0.05, steps: int = 500, d3_term: str = 'host',
                 **kw) -> List[Dict[str, Any]]:
        """`SevenNetCalculator.neb_many` on the sum of the model's and the D3 forces and energies (sevennet_amd.neb): one dict
        per band as there, the image dicts with the summed keys of `compute` at the returned positions; the tangents, `neb_fmax`,
        `imax` and the barriers are those of model + D3.  The counters are kept as `self.neb_info`.  d3_term as in `relax_many`:
        'host' prepares the D3 batch of all moving images on the host each step, 'device' keeps the term on the device; both
        hand the band their energies."""
        self._check_d3_term(d3_term)
        snet, d3 = self.calcs
        numbers_list, images_list = list(numbers_list), [np.asarray(im, np.float64) for im in images_list]
        if len(numbers_list) != len(images_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(images_list)} bands')
        for b, im in enumerate(images_list):
            if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 3 or im.shape[1] != len(np.asarray(numbers_list[b]).reshape(-1)):
                raise ValueError(f'band {b}: images of shape [M >= 3, {len(np.asarray(numbers_list[b]).reshape(-1))}, 3] are required, '
                                 f'got {im.shape}')
        # the flattened list of all images, band after band: what the `extra` of neb_batch is called over
        band_of = np.repeat(np.arange(len(images_list)), [im.shape[0] for im in images_list])
        cells_img = np.asarray(cells, np.float64).reshape(-1, 3, 3)[band_of]
        pbcs_img = np.broadcast_to(np.asarray(pbcs, bool).reshape(-1, 3), (len(images_list), 3))[band_of]
        flat_numbers = [np.asarray(numbers_list[b]).reshape(-1) for b in band_of]
        term = self._d3_term(flat_numbers, [x for im in images_list for x in im], cells_img, pbcs_img, d3_term)
        results = snet.neb_many(numbers_list, images_list, cells, pbcs, fmax=fmax, steps=steps, extra=term, **kw)
        self.neb_info = snet.neb_info
        at_final = d3.compute_many(flat_numbers, [x['positions'] for r in results for x in r['images']], cells_img, pbcs_img)
        it = iter(at_final)
        for r in results:
            r['images'] = [self._sum(a, next(it)) for a in r['images']]
        return results

    def vibrations_many(self, numbers_list, positions_list, masses_list, cells, pbcs, d3_term: str = 'host', **kw) -> List[Dict[str, Any]]:
        """`SevenNetCalculator.vibrations_many` on the sum of the model's and the D3 forces (sevennet_amd.vib): the Hessians and
        spectra are those of model + D3, the keys of `compute` for the undisplaced structures are the summed ones.  The
        counters are kept as `self.vib_info`.  d3_term as in `relax_many`: 'host' prepares the D3 batch of each call's copies
        on the host, 'device' keeps the term on the device, planned once per layout of the copy slots (fd.plan_copies)."""
        self._check_d3_term(d3_term)
        snet, d3 = self.calcs
        numbers_list, positions_list = list(numbers_list), [np.asarray(p, np.float64) for p in positions_list]
        if len(numbers_list) != len(positions_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(positions_list)} position arrays')
        B = len(numbers_list)
        cells_b = np.asarray(cells, np.float64).reshape(-1, 3, 3)
        pbcs_b = np.broadcast_to(np.asarray(pbcs, bool).reshape(-1, 3), (B, 3))

        def make_extra(slot_system):   # the D3 term over the copy slots: slot s holds a copy of system slot_system[s]
            return self._d3_term([numbers_list[b] for b in slot_system], [positions_list[b] for b in slot_system],
                                 cells_b[slot_system], pbcs_b[slot_system], d3_term)

        results = snet.vibrations_many(numbers_list, positions_list, masses_list, cells, pbcs, make_extra=make_extra, **kw)
        self.vib_info = snet.vib_info
        at_base = d3.compute_many(numbers_list, positions_list, cells, pbcs)
        return [self._sum(a, b) for a, b in zip(results, at_base)]

    def phonons_many(self, numbers_list, positions_list, masses_list, cells, pbcs, supercells, d3_term: str = 'host',
                     **kw) -> List[Dict[str, Any]]:
        """`SevenNetCalculator.phonons_many` on the sum of the model's and the D3 forces (sevennet_amd.phonon): the force constants
        and everything that follows from them are those of model + D3, the keys of `compute` for the undisplaced supercells are
        the summed ones.  The counters are kept as `self.phonon_info`.  d3_term as in `vibrations_many`: the term is built over
        the copy slots of the supercells (make_extra)."""
        from .phonon import build_supercell
        self._check_d3_term(d3_term)
        snet, d3 = self.calcs
        numbers_list, positions_list = list(numbers_list), [np.asarray(p, np.float64) for p in positions_list]
        if len(numbers_list) != len(positions_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(positions_list)} position arrays')
        built = {}   # the supercells as the driver builds them, made when it asks for the term: its validation has passed by then

        def make_extra(slot_system):   # the D3 term over the copy slots: slot s holds a copy of the supercell of system slot_system[s]
            B = len(numbers_list)
            cells_b = np.asarray(cells, np.float64).reshape(-1, 3, 3)
            reps = np.asarray(supercells, np.int64)
            reps = np.tile(reps, (B, 1)) if reps.ndim == 1 else reps
            sc = [build_supercell(numbers_list[b], positions_list[b], cells_b[b], reps[b]) for b in range(B)]
            built.update(numbers=[s[0] for s in sc], positions=[s[1] for s in sc], cells=np.stack([s[2] for s in sc]))
            return self._d3_term([built['numbers'][b] for b in slot_system], [built['positions'][b] for b in slot_system],
                                 built['cells'][slot_system], np.ones((len(slot_system), 3), bool), d3_term)

        results = snet.phonons_many(numbers_list, positions_list, masses_list, cells, pbcs, supercells, make_extra=make_extra, **kw)
        self.phonon_info = snet.phonon_info
        at_base = d3.compute_many(built['numbers'], built['positions'], built['cells'], np.ones((len(numbers_list), 3), bool))
        return [self._sum(a, b) for a, b in zip(results, at_base)]

    def elastic_many(self, numbers_list, positions_list, cells, pbcs, d3_term: str = 'device', **kw) -> List[Dict[str, Any]]:
        """`SevenNetCalculator.elastic_many` on the sum of the model's and the D3 stresses and forces (sevennet_amd.elastic): the
        tensors are those of model + D3, the keys of `compute` for the unstrained structures are the summed ones.  The counters
        are kept as `self.elastic_info`.  Only d3_term = 'device' is available: its `D3DeviceTerm`, built over the copy slots with
        their strained cells (make_extra), carries the virial the stresses need; d3_term = 'host' raises ValueError, as under
        relax_cell=True in `relax_many`."""
        self._check_d3_term(d3_term)
        if d3_term == 'host':
            raise ValueError("elastic_many is not available with d3_term='host': that D3 term reaches the driver through the `extra` "
                             "contract, which carries forces and energies but no virial, so its stress is unknown (pass "
                             "d3_term='device', whose term carries one)")
        snet, d3 = self.calcs
        numbers_list, positions_list = list(numbers_list), [np.asarray(p, np.float64) for p in positions_list]
        if len(numbers_list) != len(positions_list):
            raise ValueError(f'{len(numbers_list)} atomic-number arrays but {len(positions_list)} position arrays')
        pbcs_b = np.broadcast_to(np.asarray(pbcs, bool).reshape(-1, 3), (len(numbers_list), 3))

        def make_extra(slot_system, slot_cells):   # the D3 term over the copy slots: slot s holds a copy of system slot_system[s] in slot_cells[s]
            return self._d3_term([numbers_list[b] for b in slot_system], [positions_list[b] for b in slot_system], slot_cells,
                                 pbcs_b[slot_system], d3_term)

        results = snet.elastic_many(numbers_list, positions_list, cells, pbcs, make_extra=make_extra, **kw)
        self.elastic_info = snet.elastic_info
        at_base = d3.compute_many(numbers_list, positions_list, cells, pbcs)
        return [self._sum(a, b) for a, b in zip(results, at_base)]

    def md_many(self, numbers_list, positions_list, masses_list, cells, pbcs, dt: float, steps: int, d3_term: str = 'host',
                **kw) -> List[Dict[str, Any]]:
        """`SevenNetCalculator.md_many` on the sum of the model's and the D3 forces (sevennet_amd.md): one dict per system
        with the summed keys of `compute` at the returned positions plus `positions`, `velocities`, `e_pot` (D3 energy
        included), `e_kin`, `temperature` (and `trajectory`); the counters are kept as `self.md_info`.  d3_term as in
        `relax_many`: with 'host' the D3 batch is prepared on the host (this path copies the positions down and the D3 forces
        up once per step), with 'device' the D3 term stays on the device and the D3 share of the results is one
        `compute_many` at the returned positions.
        pressure= (constant-pressure MD, SevenNetCalculator.md_many) needs d3_term='device', whose term carries a virial: the D3
        virial then enters the barostat's pressure, and the D3 share of the results is evaluated at the returned cells.  With
        'host' it raises ValueError.
        fixed_list (SevenNetCalculator.md_many) goes through with either d3_term: held components feel neither the model's nor the
        D3 forces.  observe (SevenNetCalculator.md_many) goes through with either d3_term too: the dicts gain `observables`."""
        self._check_d3_term(d3_term)
        npt = kw.get('pressure') is not None
        if npt and d3_term == 'host':
            raise ValueError("pressure is not available with d3_term='host': that D3 term reaches the integrator through the `extra` "
                             "contract, which carries forces and energies but no virial, so its share of the pressure is unknown "
                             "(pass d3_term='device', whose term carries one)")
        snet, d3 = self.calcs
        numbers_list, positions_list = list(numbers_list), list(positions_list)
        term = self._d3_term(numbers_list, positions_list, cells, pbcs, d3_term)
        results = snet.md_many(numbers_list, positions_list, masses_list, cells, pbcs, dt, steps, extra=term, **kw)
        self.md_info = snet.md_info
        if d3_term == 'device':
            final_cells = np.stack([r['cell'] for r in results]) if npt else cells
            return [self._sum(a, b) for a, b in zip(results, d3.compute_many(numbers_list, [r['positions'] for r in results],
                                                                             final_cells, pbcs))]
        # the model's results and the D3 results of the last step's evaluations, both at the returned positions
        return [self._sum(a, D3Calculator._results(b)) for a, b in zip(results, term.last)]
