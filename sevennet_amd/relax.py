"""Batched geometry relaxation with FIRE, at fixed cells or with the cells relaxed too, positions (and cells) on the device
from the first step to the last.

`relax_batch` relaxes B structures at once: per step one batched neighbor build (sevennet_amd.batch), one engine call and one
`snet_fire_step` launch (csrc/snet_relax.hip: one workgroup per system, fp64, fixed summation order).  Positions, velocities
and the per-system optimizer state (dt, alpha, n_pos, active, n_steps) are device tensors; the only thing the optimizer reads
back per step is the number of systems still active.  A system whose largest atomic force is below `fmax` stops moving in the
same launch that finds it so, and when enough systems have finished the batch is rebuilt from the active ones only (the
"repack"), so the engine stops paying for structures that converged long ago.

FIRE: Bitzek, Koskinen, Gaehler, Moseler, Gumbsch, Phys. Rev. Lett. 97, 170201 (2006), as ASE's optimizer states it, with unit
masses; the step rule is written out in include/snet_hip.h (snet_fire_step) and restated in fp64 numpy in tests/relax_ref.py.

`relax_batch(..., relax_cell=True)` relaxes the cells with the atoms (`fire_cell_loop`): the rule of ASE's UnitCellFilter
(Tadmor, Smith, Bernstein, Kaxiras, Phys. Rev. B 59, 235 (1999)) under the same FIRE, one `snet_fire_cell_step` launch
(csrc/snet_relax_cell.hip) per step on the engine's per-system virial; the neighbor kernels read the moving cells from the
device tensor the step kernel writes, so no cell comes back to the host inside the loop.  The rule is written out in
include/snet_hip.h (snet_fire_cell_step) and restated in fp64 numpy in tests/cellrelax_ref.py.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .batch import _MAX_IMAGE_REACH, BatchForces, batch_results, classify_systems, device_positions, validate_batch_inputs
from .fixed import attach_fixed, check_whole_atoms, hold_masks

STATUS_NAMES = ('steps', 'converged', 'cell_failed')   # by the status word of snet_fire_cell_step (0: still running at the step cap)
FIRE_DEFAULTS = dict(dt_start=0.1, dt_max=1.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, max_step=0.2)


def check_fire_params(fmax: float, steps: int, repack_below: float, fire: dict) -> dict:
    """FIRE_DEFAULTS overridden by `fire`, range-checked (ValueError) together with fmax, steps and repack_below"""
    unknown = sorted(set(fire) - set(FIRE_DEFAULTS))
    if unknown:
        raise ValueError(f'unknown FIRE parameter {unknown[0]!r} (known: {sorted(FIRE_DEFAULTS)})')
    p = dict(FIRE_DEFAULTS, **fire)
    if not fmax >= 0:
        raise ValueError(f'fmax = {fmax}: the force threshold cannot be negative')
    if int(steps) != steps or steps < 0:
        raise ValueError(f'steps = {steps}: a non-negative integer is required')
    if not 0 <= repack_below <= 1:
        raise ValueError(f'repack_below = {repack_below}: a fraction in [0, 1] is required (0 switches repacking off)')
    if int(p['n_min']) != p['n_min'] or p['n_min'] < 0:
        raise ValueError(f'n_min = {p["n_min"]}: a non-negative integer is required')
    ok = {'dt_start': p['dt_start'] > 0, 'dt_max': p['dt_max'] >= p['dt_start'], 'f_inc': p['f_inc'] >= 1,
          'f_dec': 0 < p['f_dec'] < 1, 'alpha_start': 0 < p['alpha_start'] <= 1, 'f_alpha': 0 < p['f_alpha'] <= 1,
          'max_step': p['max_step'] > 0}
    for k, good in ok.items():
        if not good:   # (a NaN fails every comparison)
            raise ValueError(f'FIRE parameter {k} = {p[k]} is out of range (dt_max >= dt_start > 0, f_inc >= 1, 0 < f_dec < 1, '
                             '0 < alpha_start <= 1, 0 < f_alpha <= 1, max_step > 0)')
    p['n_min'] = int(p['n_min'])
    return p


def check_cell_params(scalar_pressure: float, cell_mask, hydrostatic_strain: bool, constant_volume: bool) -> dict:
    """the cell arguments of `relax_batch`, range-checked (ValueError): -> dict(scalar_pressure, cell_mask_bits (bit k = flag k of
    the six Voigt flags xx,yy,zz,yz,xz,xy), hydrostatic_strain, constant_volume)"""
    try:
        pressure = float(scalar_pressure)
    except (TypeError, ValueError):
        pressure = float('nan')
    if not np.isfinite(pressure):
        raise ValueError(f'scalar_pressure = {scalar_pressure!r}: a finite pressure in eV/A^3 is required')
    mask = np.ones(6) if cell_mask is None else np.asarray(cell_mask)
    if mask.shape != (6,) or mask.dtype == object or not np.isin(mask, (0, 1)).all():
        raise ValueError(f'cell_mask = {cell_mask!r}: six 0/1 flags in Voigt order xx,yy,zz,yz,xz,xy are required')
    if hydrostatic_strain and constant_volume:
        raise ValueError('hydrostatic_strain and constant_volume together leave the cell nothing to do: give one of them')
    return dict(scalar_pressure=pressure, cell_mask_bits=sum(int(m) << k for k, m in enumerate(mask)),
                hydrostatic_strain=bool(hydrostatic_strain), constant_volume=bool(constant_volume))


def check_cell_relax_systems(n_atoms, cells, pbcs, cutoff: float) -> None:
    """the systems a variable-cell relaxation takes: fully periodic ones of the batched neighbor kernel (batch.classify_systems
    kind 0 at the caller's cells); ValueError names the first that is not"""
    kind = classify_systems(np.asarray(n_atoms, np.int64), cells, pbcs, cutoff)
    for b in range(len(kind)):
        if not np.asarray(pbcs[b], bool).all():
            raise ValueError(f'system {b}: relax_cell needs a cell periodic along all three axes (pbc {np.asarray(pbcs[b]).tolist()})')
        if kind[b] != 0:
            why = 'more atoms than the batched neighbor kernel takes' if kind[b] == 1 else 'a periodic height below cutoff / 64'
            raise ValueError(f'system {b}: relax_cell reads the cells on the device, which the batched neighbor kernel alone does, '
                             f'and this system has {why}')


class RepackBook:
    """Host bookkeeping of a shrinking batch: which of the caller's systems are in the current batch (in their original
    relative order), and the final positions, step counts and flags (with a moving cell: cells and status words too) of those
    that have left it."""

    def __init__(self, n_atoms):
        self.n_atoms = np.asarray(n_atoms, np.int64)
        self.B = len(self.n_atoms)
        self.ids = np.arange(self.B)               # current batch slot -> caller's system
        self.positions: List[Any] = [None] * self.B
        self.n_steps = np.zeros(self.B, np.int64)
        self.converged = np.zeros(self.B, bool)
        self.cells: List[Any] = [None] * self.B    # variable-cell runs only
        self.status = np.zeros(self.B, np.int64)   # variable-cell runs only
        self.n_repacks = 0

    def seg_ptr(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.n_atoms[self.ids])]).astype(np.int64)

    @staticmethod
    def wants_repack(n_active: int, n_current: int, repack_below: float) -> bool:
        """some system has finished since the batch was last built, some are left, and at most repack_below of it is active"""
        return 0 < n_active < n_current and n_active <= repack_below * n_current

    def store(self, pos, active: np.ndarray, n_steps: np.ndarray, only_finished: bool, cells=None, status=None) -> None:
        """keep the results of the current batch's systems (`pos`: their flat positions, sliceable): the finished ones, or all.
        cells [b,9] and status [b] (both or neither): a variable-cell run, where converged means status 1"""
        sp = self.seg_ptr()
        for k, b in enumerate(self.ids):
            if only_finished and active[k]:
                continue
            self.positions[b] = pos[int(sp[k]):int(sp[k + 1])]
            self.n_steps[b] = int(n_steps[k])
            self.converged[b] = not active[k]
            if status is not None:
                self.cells[b] = cells[k]
                self.status[b] = int(status[k])
                self.converged[b] = int(status[k]) == 1

    def repack(self, pos, active: np.ndarray, n_steps: np.ndarray, cells=None, status=None) -> Tuple[np.ndarray, np.ndarray]:
        """store the finished systems and drop them: -> (slots kept, atom rows kept), both in the old batch's numbering"""
        self.store(pos, active, n_steps, only_finished=True, cells=cells, status=status)
        sp = self.seg_ptr()
        keep = np.nonzero(np.asarray(active) != 0)[0]
        rows = np.concatenate([np.arange(sp[k], sp[k + 1]) for k in keep]) if len(keep) else np.zeros(0, np.int64)
        self.ids = self.ids[keep]
        self.n_repacks += 1
        return keep, rows


def fire_step(pos: torch.Tensor, vel: torch.Tensor, forces: torch.Tensor, seg_ptr: torch.Tensor, dt: torch.Tensor,
              alpha: torch.Tensor, n_pos: torch.Tensor, active: torch.Tensor, n_steps: torch.Tensor, fmax_sys: torch.Tensor,
              n_active: torch.Tensor, fmax: float, params: dict, forces_extra: Optional[torch.Tensor] = None,
              hold: Optional[torch.Tensor] = None) -> None:
    """one `snet_fire_step` launch on the current stream; every tensor on the device, updated in place (dtypes as the C ABI:
    pos / vel / dt / alpha / fmax_sys fp64, forces fp32, forces_extra fp64, the rest int32).  hold (int32 [N], bit k of a word:
    component k of that atom is held; fixed.hold_masks): the launch is `snet_fire_step_fixed`."""
    N, B = int(pos.shape[0]), int(seg_ptr.numel()) - 1
    want = [(pos, torch.float64, (N, 3)), (vel, torch.float64, (N, 3)), (forces, torch.float32, (N, 3)), (seg_ptr, torch.int32, (B + 1,)),
            (dt, torch.float64, (B,)), (alpha, torch.float64, (B,)), (n_pos, torch.int32, (B,)), (active, torch.int32, (B,)),
            (n_steps, torch.int32, (B,)), (fmax_sys, torch.float64, (B,)), (n_active, torch.int32, (1,))]
    if forces_extra is not None:
        want.append((forces_extra, torch.float64, (N, 3)))
    if hold is not None:
        want.append((hold, torch.int32, (N,)))
    _lib.check_device_tensors('fire_step', pos, want)
    P = _lib.ptr
    args = (P(pos), P(vel), P(forces), P(forces_extra), N, P(seg_ptr), B, P(dt), P(alpha), P(n_pos), P(active), P(n_steps),
            P(fmax_sys), P(n_active), float(fmax), params['dt_start'], params['dt_max'], params['n_min'], params['f_inc'],
            params['f_dec'], params['alpha_start'], params['f_alpha'], params['max_step'])
    with torch.cuda.device(pos.device):
        if hold is None:
            _lib.check(_lib.load().snet_fire_step(*args, _lib.stream()), 'snet_fire_step')
        else:
            _lib.check(_lib.load().snet_fire_step_fixed(*args, P(hold), _lib.stream()), 'snet_fire_step_fixed')


def fire_loop(forces: BatchForces, positions, *, fmax: float, steps: int, repack_below: float, params: dict,
              hold: Optional[np.ndarray] = None):
    """The relaxation loop over the force call `forces` (a BatchForces on validated inputs; `check_fire_params`): -> (positions
    fp64 [N,3] on the device in the caller's order, n_steps [B], converged [B], info).  hold (int32 [N] on the host,
    fixed.hold_masks, or None): the components held fixed; the mask goes to the device once and is regathered at a repack."""
    dev = forces.engine.dev
    book = RepackBook(forces.n_atoms)
    B = book.B
    with torch.cuda.device(dev):
        pos = device_positions(positions, dev).clone()
        vel = torch.zeros_like(pos)
        hold = None if hold is None else torch.as_tensor(np.ascontiguousarray(hold, np.int32)).to(dev)
        dt = torch.full((B,), float(params['dt_start']), dtype=torch.float64, device=dev)
        alpha = torch.full((B,), float(params['alpha_start']), dtype=torch.float64, device=dev)
        n_pos = torch.zeros(B, dtype=torch.int32, device=dev)
        active = torch.ones(B, dtype=torch.int32, device=dev)
        n_steps = torch.zeros(B, dtype=torch.int32, device=dev)
        fmax_sys = torch.zeros(B, dtype=torch.float64, device=dev)
        n_active = torch.zeros(1, dtype=torch.int32, device=dev)
        fire_launches = 0
        for _ in range(int(steps)):
            g, out, fx = forces(pos, book.ids)[:3]   # (FIRE has no use for the extra energies)
            fire_step(pos, vel, out['forces'], g.seg_ptr, dt, alpha, n_pos, active, n_steps, fmax_sys, n_active, fmax, params, fx,
                      hold)
            fire_launches += 1
            left = int(n_active.item())   # the one readback of the step
            if left == 0:
                break
            if book.wants_repack(left, len(book.ids), repack_below):
                act_h, st_h = torch.stack([active, n_steps]).cpu().numpy()
                keep, rows = book.repack(pos, act_h, st_h)
                rows_d, keep_d = torch.as_tensor(rows).to(dev), torch.as_tensor(keep).to(dev)
                pos, vel = pos[rows_d], vel[rows_d]   # (gathers copy: the stored slices keep the old buffer)
                hold = None if hold is None else hold[rows_d]
                dt, alpha, n_pos, active, n_steps, fmax_sys = (t[keep_d] for t in (dt, alpha, n_pos, active, n_steps, fmax_sys))
        act_h, st_h = torch.stack([active, n_steps]).cpu().numpy()
        book.store(pos, act_h, st_h, only_finished=False)
        final = torch.cat(book.positions)
    info = dict(n_force_calls=forces.n_force_calls, n_repacks=book.n_repacks, system_steps_evaluated=forces.system_steps_evaluated,
                fire_launches=fire_launches)
    return final, book.n_steps.copy(), book.converged.copy(), info


def fire_cell_step(pos: torch.Tensor, vel: torch.Tensor, cell: torch.Tensor, vel_cell: torch.Tensor, cell0: torch.Tensor,
                   forces: torch.Tensor, virial: torch.Tensor, seg_ptr: torch.Tensor, dt: torch.Tensor, alpha: torch.Tensor,
                   n_pos: torch.Tensor, active: torch.Tensor, n_steps: torch.Tensor, status: torch.Tensor, fmax_sys: torch.Tensor,
                   n_active: torch.Tensor, fmax: float, params: dict, cell_params: dict, min_height: float,
                   forces_extra: Optional[torch.Tensor] = None, virial_extra: Optional[torch.Tensor] = None,
                   hold: Optional[torch.Tensor] = None) -> None:
    """one `snet_fire_cell_step` launch on the current stream; every tensor on the device, updated in place (dtypes as the C
    ABI: pos / vel / cell / vel_cell / cell0 / virial / virial_extra / forces_extra / dt / alpha / fmax_sys fp64, forces fp32, the
    rest int32).  params: `check_fire_params`; cell_params: `check_cell_params`.  hold (int32 [N], a nonzero word: that atom is
    held; fixed.hold_masks): the launch is `snet_fire_cell_step_fixed`."""
    N, B = int(pos.shape[0]), int(seg_ptr.numel()) - 1
    f64, i32 = torch.float64, torch.int32
    want = [(pos, f64, (N, 3)), (vel, f64, (N, 3)), (cell, f64, (B, 9)), (vel_cell, f64, (B, 9)), (cell0, f64, (B, 9)),
            (forces, torch.float32, (N, 3)), (virial, f64, (B, 6)), (seg_ptr, i32, (B + 1,)), (dt, f64, (B,)), (alpha, f64, (B,)),
            (n_pos, i32, (B,)), (active, i32, (B,)), (n_steps, i32, (B,)), (status, i32, (B,)), (fmax_sys, f64, (B,)),
            (n_active, i32, (1,))]
    if forces_extra is not None:
        want.append((forces_extra, f64, (N, 3)))
    if virial_extra is not None:
        want.append((virial_extra, f64, (B, 6)))
    if hold is not None:
        want.append((hold, i32, (N,)))
    _lib.check_device_tensors('fire_cell_step', pos, want)
    P = _lib.ptr
    args = (P(pos), P(vel), P(cell), P(vel_cell), P(cell0), P(forces), P(forces_extra), P(virial), P(virial_extra), N, P(seg_ptr), B,
            P(dt), P(alpha), P(n_pos), P(active), P(n_steps), P(status), P(fmax_sys), P(n_active), float(fmax), params['dt_start'],
            params['dt_max'], params['n_min'], params['f_inc'], params['f_dec'], params['alpha_start'], params['f_alpha'],
            params['max_step'], cell_params['scalar_pressure'], cell_params['cell_mask_bits'], int(cell_params['hydrostatic_strain']),
            int(cell_params['constant_volume']), float(min_height))
    with torch.cuda.device(pos.device):
        if hold is None:
            _lib.check(_lib.load().snet_fire_cell_step(*args, _lib.stream()), 'snet_fire_cell_step')
        else:
            _lib.check(_lib.load().snet_fire_cell_step_fixed(*args, P(hold), _lib.stream()), 'snet_fire_cell_step_fixed')


def fire_cell_loop(forces, positions, cells, *, fmax: float, steps: int, repack_below: float, params: dict, cell_params: dict,
                   min_height: float, hold: Optional[np.ndarray] = None):
    """The variable-cell relaxation loop.  forces: a BatchForces, or any object with its call interface (pos, ids, cells_dev=) ->
    (graph with seg_ptr, output with `forces` fp32 [N,3] and `virial_per_system` fp64 [b,6], extra forces or None, ...), its
    counters (n_force_calls, system_steps_evaluated), `n_atoms` and `engine.dev`, and optionally `virial_extra` (fp64 [b,6] on the
    device or None: the virial that goes with the extra forces, added to the model's in the step kernel).  cells [B,3,3]: the caller's, which stay the
    reference cells.  Per step: one graph build from the device cells, one engine call, one `snet_fire_cell_step`, one readback
    (n_active).  -> (positions fp64 [N,3] and cells fp64 [B,9] on the device in the caller's order, n_steps [B], status [B] (0
    step cap, 1 converged, 2 the kernel's guard refused the next cell), info).  hold (int32 [N] on the host, whole atoms:
    `fixed.check_whole_atoms`, or None): the atoms that keep their fractional coordinates; regathered at a repack."""
    dev = forces.engine.dev
    book = RepackBook(forces.n_atoms)
    B = book.B
    with torch.cuda.device(dev):
        pos = device_positions(positions, dev).clone()
        cell0 = torch.as_tensor(np.ascontiguousarray(np.asarray(cells, np.float64).reshape(B, 9))).to(dev)
        cell = cell0.clone()
        vel, vel_cell = torch.zeros_like(pos), torch.zeros_like(cell)
        hold = None if hold is None else torch.as_tensor(np.ascontiguousarray(hold, np.int32)).to(dev)
        dt = torch.full((B,), float(params['dt_start']), dtype=torch.float64, device=dev)
        alpha = torch.full((B,), float(params['alpha_start']), dtype=torch.float64, device=dev)
        n_pos = torch.zeros(B, dtype=torch.int32, device=dev)
        active = torch.ones(B, dtype=torch.int32, device=dev)
        n_steps = torch.zeros(B, dtype=torch.int32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        fmax_sys = torch.zeros(B, dtype=torch.float64, device=dev)
        n_active = torch.zeros(1, dtype=torch.int32, device=dev)
        fire_launches = 0
        for _ in range(int(steps)):
            g, out, fx = forces(pos, book.ids, cells_dev=cell)[:3]
            fire_cell_step(pos, vel, cell, vel_cell, cell0, out['forces'], out['virial_per_system'], g.seg_ptr, dt, alpha, n_pos,
                           active, n_steps, status, fmax_sys, n_active, fmax, params, cell_params, min_height, fx,
                           getattr(forces, 'virial_extra', None), hold)
            fire_launches += 1
            left = int(n_active.item())   # the one readback of the step
            if left == 0:
                break
            if book.wants_repack(left, len(book.ids), repack_below):
                act_h, st_h, status_h = torch.stack([active, n_steps, status]).cpu().numpy()
                keep, rows = book.repack(pos, act_h, st_h, cells=cell, status=status_h)
                rows_d, keep_d = torch.as_tensor(rows).to(dev), torch.as_tensor(keep).to(dev)
                pos, vel = pos[rows_d], vel[rows_d]   # (gathers copy: the stored slices keep the old buffers)
                hold = None if hold is None else hold[rows_d]
                cell, cell0, vel_cell, dt, alpha, n_pos, active, n_steps, status, fmax_sys = (
                    t[keep_d] for t in (cell, cell0, vel_cell, dt, alpha, n_pos, active, n_steps, status, fmax_sys))
        act_h, st_h, status_h = torch.stack([active, n_steps, status]).cpu().numpy()
        book.store(pos, act_h, st_h, only_finished=False, cells=cell, status=status_h)
        final, final_cells = torch.cat(book.positions), torch.stack(book.cells)
    info = dict(n_force_calls=forces.n_force_calls, n_repacks=book.n_repacks, system_steps_evaluated=forces.system_steps_evaluated,
                fire_launches=fire_launches)
    return final, final_cells, book.n_steps.copy(), book.status.copy(), info


def relax_batch(engine, types, positions, cells, pbcs, *, cutoff: float, fmax: float = 0.05, steps: int = 500,
                repack_below: float = 0.5, extra: Optional[Callable] = None, n_atoms=None, want_atomic_virial: bool = False,
                relax_cell: bool = False, scalar_pressure: float = 0.0, cell_mask=None, hydrostatic_strain: bool = False,
                constant_volume: bool = False, fixed_list=None, **fire) -> Tuple[List[Dict[str, Any]], Dict[str, int]]:
    """Relax B structures with FIRE until every atom's force is below `fmax` (eV/A) or `steps` steps are done; at fixed cells,
    or with relax_cell the cells too.

    engine: a HipForceEngine.  types / positions / cells / pbcs (and n_atoms for flat arrays) as `build_batch_graph`; the
    caller's arrays are not modified.  repack_below: when at most this fraction of the current batch is still active (and a
    system has finished since the batch was built) the batch is rebuilt from the active systems; 0 never repacks.
    extra: optional callable with the contract of `batch.BatchForces` (positions fp64 [N,3] on the device, seg_ptr int64
    [b+1] on the host, ids int64 [b]: the caller's index of each system of the current batch) -> forces [N,3], or (forces,
    energy_per_system [b]), added to the model's each step (FIRE has no use for the energies).  fire: FIRE_DEFAULTS overrides.

    Returns (results, info).  results[b]: the dict of SevenNetCalculator.compute_many from ONE batched evaluation of all B
    systems at their final positions, plus `positions` [n,3] fp64, `converged` and `n_steps` (the moves made).  A system is
    converged when the step kernel found its largest atomic force below fmax at the positions returned; one that reaches the
    step cap is returned with converged = False.  info: n_force_calls (engine calls, the final evaluation included),
    fire_launches (= loop iterations), system_steps_evaluated (systems in the batch, summed over the loop's engine calls),
    n_repacks.  Invalid input raises ValueError before any device work.

    relax_cell: relax the cells with the atoms, by the rule of ASE's UnitCellFilter (include/snet_hip.h, snet_fire_cell_step):
    the caller's cells are the reference cells, `fmax` bounds the atoms' forces in the reference frame (eV/A) and the rows of
    the cell force (virial - scalar_pressure V) F^-T / n alike.  scalar_pressure: the external pressure in eV/A^3; cell_mask:
    six 0/1 Voigt flags (xx,yy,zz,yz,xz,xy) of the strain components that may change (default: all); hydrostatic_strain: the
    cell changes by a uniform scaling only; constant_volume: the trace of the cell force is projected out.  Every system must
    be periodic along all three axes and one of the batched neighbor kernel (at most batch.BATCH_MAX_ATOMS atoms, no height
    below cutoff / 64); a plain `extra` is refused, because its contract carries forces and energies but no virial -- one marked
    `provides_virial = True` (d3.D3DeviceTerm; batch.BatchForces) is taken, and its virial enters the cell force.  A NaN in
    that virial fails the step kernel's guard like any other non-finite step ('cell_failed' below).  The results gain
    `cell` [3,3] fp64 (energy, forces and stress are those at the returned positions AND cell) and `status`: 'converged',
    'steps' (the step cap) or 'cell_failed' (the step kernel refused a next cell that was not finite, inverted, or flatter than
    cutoff / 64: the system is returned as it was before that step); `converged` is True for the first only.

    fixed_list: the atoms and Cartesian components that do not move (slabs, adsorbates on a frozen substrate, defects in a frozen
    matrix, selective dynamics): per system None, a bool mask [n] or an integer index list of whole atoms, or a bool mask [n,3]
    of components (fixed.hold_masks).  The step kernel (snet_fire_step_fixed) takes the force and the velocity of a held component
    as 0 and never writes its position, so the returned `positions` carry the caller's bits there; `converged` then refers to the
    free components only (a system with nothing free is converged at once, n_steps 0), while `forces` stay the model's true forces
    at the returned positions, on held atoms too.  With relax_cell whole atoms only (a mask that holds some but not all components
    of an atom raises ValueError): a held atom keeps its fractional coordinates and moves with the cell, as under ASE's
    UnitCellFilter with FixAtoms.  When something is held the results gain `fixed`, a bool array [n,3]; with fixed_list None, or
    masks that hold nothing, the call is the one without the argument: the same launches, the same dicts."""
    params = check_fire_params(fmax, steps, repack_below, fire)
    cell_params = check_cell_params(scalar_pressure, cell_mask, hydrostatic_strain, constant_volume)
    if relax_cell and extra is not None and not getattr(extra, 'provides_virial', False):
        raise ValueError('relax_cell with extra: the contract of `extra` carries forces and energies but no virial, so the cell '
                         'force of the extra term is unknown (an extra marked `provides_virial = True` returns one; for D3 that is '
                         "d3.D3DeviceTerm, SevenNetD3Calculator.relax_many(d3_term='device'))")
    types, positions, n_at, cells, pbcs = validate_batch_inputs(types, positions, cells, pbcs, cutoff, engine.spec.num_species,
                                                                n_atoms=n_atoms)
    hold = hold_masks(fixed_list, n_at)
    if relax_cell:
        if hold is not None:
            check_whole_atoms(hold, n_at)
        check_cell_relax_systems(n_at, cells, pbcs, cutoff)
        forces = BatchForces(engine, types, n_at, cells, pbcs, cutoff, extra)
        final, final_cells, n_steps, status, info = fire_cell_loop(
            forces, positions, cells, fmax=fmax, steps=steps, repack_below=repack_below, params=params, cell_params=cell_params,
            min_height=cutoff / _MAX_IMAGE_REACH, hold=hold)
        g, out, _, _ = forces(final, want_atomic_virial=want_atomic_virial, with_extra=False, cells_dev=final_cells)
        info['n_force_calls'] = forces.n_force_calls
        cells_h = final_cells.cpu().numpy().reshape(-1, 3, 3)
        results = attach_relaxed(batch_results(g, out, cells_h, want_atomic_virial), final, g.seg_ptr_host, n_steps, status == 1)
        for b, res in enumerate(results):
            res['cell'] = cells_h[b].copy()
            res['status'] = STATUS_NAMES[int(status[b])]
        return (results if hold is None else attach_fixed(results, hold, g.seg_ptr_host)), info
    forces = BatchForces(engine, types, n_at, cells, pbcs, cutoff, extra)
    final, n_steps, converged, info = fire_loop(forces, positions, fmax=fmax, steps=steps, repack_below=repack_below, params=params,
                                                hold=hold)
    g, out, _, _ = forces(final, want_atomic_virial=want_atomic_virial, with_extra=False)
    info['n_force_calls'] = forces.n_force_calls
    results = attach_relaxed(batch_results(g, out, cells, want_atomic_virial), final, g.seg_ptr_host, n_steps, converged)
    return (results if hold is None else attach_fixed(results, hold, g.seg_ptr_host)), info


def attach_relaxed(results: List[Dict[str, Any]], final: torch.Tensor, seg_ptr_host, n_steps, converged) -> List[Dict[str, Any]]:
    """`positions`, `converged` and `n_steps` into each system's results dict"""
    pos_h = final.cpu().numpy()
    for b, res in enumerate(results):
        res['positions'] = pos_h[int(seg_ptr_host[b]):int(seg_ptr_host[b + 1])].copy()
        res['converged'] = bool(converged[b])
        res['n_steps'] = int(n_steps[b])
    return results
