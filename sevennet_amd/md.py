"""Batched NVE / Langevin molecular dynamics at fixed cells, and isotropic NPT: the state on the device from the first step to the
last.

`md_batch` integrates B structures at once: per step one batched neighbor build (sevennet_amd.batch), one engine call and one
`snet_mdb_step` launch (csrc/snet_mdstep.hip: one workgroup per system, fp64, fixed summation order).  Positions, velocities,
the per-system step counters, the energy logs and the trajectory frames are device tensors; the integrator reads nothing back
while it runs, and everything comes to the host once, after the loop.  What still synchronises per step is the batched
neighbor build, which reads the edge total to size its arrays (a skinned list kept over several steps would remove it; that is
not done here).

The integrator is BAOAB (Leimkuhler, Matthews, Appl. Math. Res. Express 2013, 34; TorchSim's `nvt_langevin` states the same
rule), folded around the force call so that one launch finishes step k and begins step k + 1; with friction 0 it is velocity
Verlet.  The noise is Philox4x32-10 counted by (atom within its system, system id, step): a system's trajectory does not
depend on the batch it runs in.  The rule is written out in include/snet_hip.h (snet_mdb_step) and restated in fp64 numpy in
tests/md_ref.py.  Units: eV, A, fs, amu, K.

With a `pressure`, `md_batch` runs isotropic NPT (`md_npt_loop`): one `snet_mdb_npt_step` launch (csrc/snet_mdnpt.hip) per step
adds the stochastic cell rescaling of Bernetti and Bussi (J. Chem. Phys. 153, 114107 (2020)) between the kicks and the drift, on
the engine's per-system virial; the cells stay on the device, where the batched neighbor kernels read them.  That rule is
written out in include/snet_hip.h (snet_mdb_npt_step) and restated in tests/md_npt_ref.py.

With an `observe` (sevennet_amd.observe.Observe), the fixed-cell loop samples (x_k, v_k) every few steps into accumulators of the
radial distribution function, the mean-square displacement and the velocity autocorrelation on the device (snet_obs_rdf,
snet_obs_correlate), and the results gain `observables`."""
from __future__ import annotations

import math
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .batch import _MAX_IMAGE_REACH, BatchForces, _as_host, batch_results, system_of, validate_batch_inputs
from .fixed import attach_fixed, held_components, hold_masks
from .observe import Accumulator, Observe, attach_observables, observe_plan as make_observe_plan
from .relax import check_cell_relax_systems

ACC = 9.648533212e-3    # eV / (A amu) in A / fs^2
KB = 8.617333262e-5     # eV / K
FINISH, START = 1, 2    # snet_mdb_step phase bits
NPT_STATUS_NAMES = ('ok', None, 'cell_failed')   # by the status word of snet_mdb_npt_step (2: its guard refused a next cell)


def langevin_coefficients(friction: float, dt: float) -> Tuple[float, float]:
    """(c1, c2) = (exp(-gamma dt), sqrt(1 - c1^2)) in fp64 on the host: what snet_mdb_step is given (friction 0: (1, 0), NVE)"""
    c1 = math.exp(-float(friction) * float(dt))
    return c1, math.sqrt(1.0 - c1 * c1)


def _per_atom(x, n_at: np.ndarray, width: int, what: str) -> np.ndarray:
    """per-system sequences or one flat array -> fp64 [N] (width 0) or [N, width]; ValueError names the system"""
    N = int(n_at.sum())
    shape = (N,) if width == 0 else (N, width)
    if isinstance(x, (list, tuple)) and len(x) and not np.isscalar(x[0]) and not (isinstance(x[0], torch.Tensor) and x[0].ndim == 0):
        if len(x) != len(n_at):
            raise ValueError(f'{len(n_at)} systems but {len(x)} {what} arrays')
        parts = []
        for b, p in enumerate(x):
            p = _as_host(p, np.float64)
            want = (int(n_at[b]),) if width == 0 else (int(n_at[b]), width)
            if p.shape != want:
                raise ValueError(f'system {b}: {what} of shape {p.shape}, {want} expected ({int(n_at[b])} atoms)')
            parts.append(p)
        return np.concatenate(parts)
    x = _as_host(x, np.float64)
    if x.shape != shape:
        raise ValueError(f'{what} of shape {x.shape}: per-system arrays, or one flat array of shape {shape}, expected')
    return x.copy()


def validate_md_inputs(masses, n_at: np.ndarray, dt, steps, temperature, friction, velocities, seed, log_every, traj_every,
                       system_ids=None):
    """Host checks of everything md_batch takes beyond the batch inputs (`validate_batch_inputs`) -> (mass fp64 [N], velocities fp64 [N,3] or None, kT
    fp64 [B] in eV, system ids int32 [B]).  ValueError names the system."""
    B = len(n_at)
    a_ptr = np.concatenate([[0], np.cumsum(n_at)])
    if not (isinstance(dt, (int, float, np.floating, np.integer)) and dt > 0 and math.isfinite(dt)):
        raise ValueError(f'dt = {dt}: a positive time step (fs) is required')
    for name, v, low in (('steps', steps, 0), ('log_every', log_every, 1), ('traj_every', traj_every, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or v < low:
            raise ValueError(f'{name} = {v}: an integer >= {low} is required')
    real = (int, float, np.floating, np.integer)
    if isinstance(friction, bool) or not isinstance(friction, real) or not (friction >= 0 and math.isfinite(friction)):
        raise ValueError(f'friction = {friction!r}: a friction (1/fs) >= 0 is required')
    if friction > 0 and langevin_coefficients(friction, dt)[1] == 0.0:   # exp(-gamma dt) rounds to 1: the kernel would run NVE
        raise ValueError(f'friction = {friction} with dt = {dt}: friction * dt is below fp64 resolution, the thermostat would '
                         'do nothing (pass friction = 0 for NVE)')
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f'seed = {seed!r}: an integer in [0, 2^64) is required')
    if temperature is None:
        if velocities is None:
            raise ValueError('neither velocities nor temperature given: pass start velocities, or a temperature to draw them at')
        if friction > 0:
            raise ValueError(f'friction = {friction} needs a temperature: the thermostat has nothing to aim at')
        kT = np.zeros(B)
    else:
        T = _as_host(temperature, np.float64)
        if T.ndim == 0:
            T = np.full(B, float(T))
        if T.shape != (B,):
            raise ValueError(f'temperature of shape {T.shape}: a scalar or one value per system ({B}) is required')
        bad = ~((T >= 0) & np.isfinite(T))
        if bad.any():
            b = int(np.nonzero(bad)[0][0])
            raise ValueError(f'system {b}: temperature = {T[b]} K, a finite temperature >= 0 is required')
        kT = KB * T
    mass = _per_atom(masses, n_at, 0, 'masses')   # (as many as atoms)
    bad = ~((mass > 0) & np.isfinite(mass))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f'system {system_of(a_ptr, i)}: mass = {mass[i]} amu, finite masses > 0 are required')
    vel = None
    if velocities is not None:
        vel = _per_atom(velocities, n_at, 3, 'velocities')
        fin = np.isfinite(vel).all(1)
        if not fin.all():
            raise ValueError(f'system {system_of(a_ptr, int(np.nonzero(~fin)[0][0]))}: non-finite velocity')
    if system_ids is None:
        ids = np.arange(B, dtype=np.int64)
    else:
        ids = _as_host(system_ids, np.int64).reshape(-1)
        if len(ids) != B or (ids < 0).any() or (ids >= 2 ** 31).any():
            raise ValueError(f'system_ids: {B} integers in [0, 2^31) are required')
    return mass, vel, kT, ids.astype(np.int32)


def md_step(pos: torch.Tensor, vel: torch.Tensor, forces: torch.Tensor, mass: torch.Tensor, seg_ptr: torch.Tensor,
            sys_id: torch.Tensor, kT: torch.Tensor, step_index: torch.Tensor, e_kin: torch.Tensor, dt: float, c1: float, c2: float,
            seed: int, phase: int, forces_extra: Optional[torch.Tensor] = None, hold: Optional[torch.Tensor] = None) -> None:
    """one `snet_mdb_step` launch on the current stream; every tensor on the device, updated in place (dtypes as the C ABI:
    pos / vel / mass / kT / e_kin fp64, forces fp32, forces_extra fp64, seg_ptr / sys_id / step_index int32).  hold (int32 [N],
    bit k of a word: component k of that atom is held; fixed.hold_masks): the launch is `snet_mdb_step_fixed`."""
    N, B = int(pos.shape[0]), int(seg_ptr.numel()) - 1
    want = [(pos, torch.float64, (N, 3)), (vel, torch.float64, (N, 3)), (forces, torch.float32, (N, 3)), (mass, torch.float64, (N,)),
            (seg_ptr, torch.int32, (B + 1,)), (sys_id, torch.int32, (B,)), (kT, torch.float64, (B,)), (step_index, torch.int32, (B,)),
            (e_kin, torch.float64, (B,))]
    if forces_extra is not None:
        want.append((forces_extra, torch.float64, (N, 3)))
    if hold is not None:
        want.append((hold, torch.int32, (N,)))
    _lib.check_device_tensors('md_step', pos, want)
    P = _lib.ptr
    args = (P(pos), P(vel), P(forces), P(forces_extra), P(mass), N, P(seg_ptr), P(sys_id), B, P(kT), P(step_index), P(e_kin),
            float(dt), float(c1), float(c2), int(seed), int(phase))
    with torch.cuda.device(pos.device):
        if hold is None:
            _lib.check(_lib.load().snet_mdb_step(*args, _lib.stream()), 'snet_mdb_step')
        else:
            _lib.check(_lib.load().snet_mdb_step_fixed(*args, P(hold), _lib.stream()), 'snet_mdb_step_fixed')


def init_velocities(vel: torch.Tensor, mass: torch.Tensor, seg_ptr: torch.Tensor, sys_id: torch.Tensor, kT: torch.Tensor,
                    seed: int, remove_com: bool = True, hold: Optional[torch.Tensor] = None) -> None:
    """one `snet_mdb_init_velocities` launch on the current stream: Maxwell-Boltzmann velocities at kT (eV) into vel.  hold (int32
    [N], as `md_step`): the launch is `snet_mdb_init_velocities_fixed` -- held components are 0, and a system with some is not
    shifted to its centre of mass but scaled (remove_com) to a kinetic energy of (3 n - held components) kT / 2."""
    N, B = int(vel.shape[0]), int(seg_ptr.numel()) - 1
    want = [(vel, torch.float64, (N, 3)), (mass, torch.float64, (N,)), (seg_ptr, torch.int32, (B + 1,)), (sys_id, torch.int32, (B,)),
            (kT, torch.float64, (B,))]
    if hold is not None:
        want.append((hold, torch.int32, (N,)))
    _lib.check_device_tensors('init_velocities', vel, want)
    P = _lib.ptr
    args = (P(vel), P(mass), N, P(seg_ptr), P(sys_id), B, P(kT), int(seed), int(bool(remove_com)))
    with torch.cuda.device(vel.device):
        if hold is None:
            _lib.check(_lib.load().snet_mdb_init_velocities(*args, _lib.stream()), 'snet_mdb_init_velocities')
        else:
            _lib.check(_lib.load().snet_mdb_init_velocities_fixed(*args, P(hold), _lib.stream()), 'snet_mdb_init_velocities_fixed')


def _per_system(x, B: int, what: str, unit: str) -> np.ndarray:
    """a scalar or one value per system -> fp64 [B]; ValueError where it is neither"""
    try:
        a = _as_host(x, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'{what} = {x!r}: a scalar or one value per system ({unit}) is required') from None
    if a.ndim == 0:
        a = np.full(B, float(a))
    if a.shape != (B,):
        raise ValueError(f'{what} of shape {a.shape}: a scalar or one value per system ({B}) is required')
    return a.copy()


def validate_npt_inputs(n_at: np.ndarray, cells: np.ndarray, pbcs: np.ndarray, cutoff: float, pressure, compressibility,
                        barostat_time, max_log_volume_step, extra=None):
    """Host checks of what the barostat of md_batch adds to `validate_md_inputs` -> (pressure fp64 [B] in eV/A^3,
    compressibility / barostat_time fp64 [B] in A^3/(eV fs)).  ValueError names the system."""
    B = len(n_at)
    if compressibility is None:
        raise ValueError('pressure given without compressibility: the barostat needs the isothermal compressibility (A^3/eV) '
                         'that sets its coupling')
    p0 = _per_system(pressure, B, 'pressure', 'eV/A^3')
    bad = ~np.isfinite(p0)
    if bad.any():
        b = int(np.nonzero(bad)[0][0])
        raise ValueError(f'system {b}: pressure = {p0[b]} eV/A^3, a finite pressure is required')
    beta = _per_system(compressibility, B, 'compressibility', 'A^3/eV')
    bad = ~((beta > 0) & np.isfinite(beta))
    if bad.any():
        b = int(np.nonzero(bad)[0][0])
        raise ValueError(f'system {b}: compressibility = {beta[b]} A^3/eV, a finite compressibility > 0 is required')
    real = (int, float, np.floating, np.integer)
    for name, v in (('barostat_time', barostat_time), ('max_log_volume_step', max_log_volume_step)):
        if isinstance(v, bool) or not isinstance(v, real) or not (v > 0 and math.isfinite(v)):
            raise ValueError(f'{name} = {v!r}: a finite value > 0 is required')
    if extra is not None and not getattr(extra, 'provides_virial', False):
        raise ValueError('pressure with extra: the contract of `extra` carries forces and energies but no virial, so the '
                         'pressure of the extra term is unknown (an extra marked `provides_virial = True` returns one; for D3 that is '
                         "d3.D3DeviceTerm, SevenNetD3Calculator.md_many(d3_term='device'))")
    try:
        check_cell_relax_systems(n_at, cells, pbcs, cutoff)
    except ValueError as e:   # (the same restrictions, named for this driver)
        raise ValueError(str(e).replace('relax_cell', 'md with a pressure')) from None
    return p0, beta / float(barostat_time)


def md_npt_step(pos: torch.Tensor, vel: torch.Tensor, cell: torch.Tensor, forces: torch.Tensor, virial: torch.Tensor,
                mass: torch.Tensor, seg_ptr: torch.Tensor, sys_id: torch.Tensor, kT: torch.Tensor, p0: torch.Tensor,
                beta_over_tau: torch.Tensor, step_index: torch.Tensor, e_kin: torch.Tensor, volume: torch.Tensor,
                pressure: torch.Tensor, active: torch.Tensor, status: torch.Tensor, dt: float, c1: float, c2: float, seed: int,
                phase: int, max_log_volume_step: float, min_height: float, forces_extra: Optional[torch.Tensor] = None,
                virial_extra: Optional[torch.Tensor] = None) -> None:
    """one `snet_mdb_npt_step` launch on the current stream; every tensor on the device, updated in place (dtypes as the C ABI:
    as `md_step`, and cell [B,9] / virial [B,6] / virial_extra [B,6] / p0 / beta_over_tau / volume / pressure fp64, active /
    status int32)"""
    N, B = int(pos.shape[0]), int(seg_ptr.numel()) - 1
    f64, i32 = torch.float64, torch.int32
    want = [(pos, f64, (N, 3)), (vel, f64, (N, 3)), (cell, f64, (B, 9)), (forces, torch.float32, (N, 3)), (virial, f64, (B, 6)),
            (mass, f64, (N,)), (seg_ptr, i32, (B + 1,)), (sys_id, i32, (B,)), (kT, f64, (B,)), (p0, f64, (B,)),
            (beta_over_tau, f64, (B,)), (step_index, i32, (B,)), (e_kin, f64, (B,)), (volume, f64, (B,)), (pressure, f64, (B,)),
            (active, i32, (B,)), (status, i32, (B,))]
    if forces_extra is not None:
        want.append((forces_extra, f64, (N, 3)))
    if virial_extra is not None:
        want.append((virial_extra, f64, (B, 6)))
    _lib.check_device_tensors('md_npt_step', pos, want)
    P = _lib.ptr
    with torch.cuda.device(pos.device):
        _lib.check(_lib.load().snet_mdb_npt_step(
            P(pos), P(vel), P(cell), P(forces), P(forces_extra), P(virial), P(virial_extra), P(mass), N, P(seg_ptr), P(sys_id), B,
            P(kT), P(p0), P(beta_over_tau), P(step_index), P(e_kin), P(volume), P(pressure), P(active), P(status), float(dt),
            float(c1), float(c2), int(seed), int(phase), float(max_log_volume_step), float(min_height), _lib.stream()),
            'snet_mdb_npt_step')


def md_loop(forces: BatchForces, positions, mass: np.ndarray, vel0: Optional[np.ndarray], kT: np.ndarray, ids: np.ndarray, *,
            dt: float, steps: int, friction: float, seed: int, log_every: int, traj_every: int, remove_com: bool,
            want_atomic_virial: bool, hold: Optional[np.ndarray] = None, observe_plan: Optional[dict] = None):
    """The MD loop over the force call `forces` (a BatchForces on validated inputs; `validate_md_inputs`) -> (graph and engine
    output of the last force call, dict of device tensors: pos, vel [N,3], e_pot, e_kin [samples,B], traj [frames,N,3] or None,
    step_index [B]; info).  hold (int32 [N] on the host, fixed.hold_masks, or None): the components held fixed; the held
    components of vel0 are taken as 0.  observe_plan (observe.observe_plan, or None): (x_k, v_k) is sampled at every step k that is a
    multiple of its `every` -- that step's launch is split into its FINISH half, the observe launches and its START half, which is
    the same arithmetic because the kernel stores exact fp64 in between -- and the state gains `observe`, the Accumulator."""
    dev = forces.engine.dev
    n_atoms = forces.n_atoms
    B, steps, log_every, traj_every = len(n_atoms), int(steps), int(log_every), int(traj_every)
    c1, c2 = langevin_coefficients(friction, dt)
    up = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a, dtype)).to(dev)  # noqa: E731
    with torch.cuda.device(dev):
        pos = (positions.to(dev, torch.float64) if isinstance(positions, torch.Tensor)
               else up(positions, np.float64)).reshape(-1, 3).clone()
        N = int(pos.shape[0])
        m_d, kT_d, id_d, seg = up(mass, np.float64), up(kT, np.float64), up(ids, np.int32), up(forces.a_ptr, np.int32)
        hold_d = None if hold is None else up(hold, np.int32)
        if vel0 is None:
            vel = torch.empty_like(pos)
            init_velocities(vel, m_d, seg, id_d, kT_d, seed, remove_com, hold_d)
        else:
            vel = up(vel0 if hold is None else np.where(held_components(hold), 0.0, vel0), np.float64)
        step_index = torch.zeros(B, dtype=torch.int32, device=dev)
        e_kin = torch.zeros(B, dtype=torch.float64, device=dev)
        e_pot_log = torch.zeros(steps // log_every + 1, B, dtype=torch.float64, device=dev)
        e_kin_log = torch.zeros_like(e_pot_log)
        traj = torch.zeros(steps // traj_every + 1, N, 3, dtype=torch.float64, device=dev) if traj_every > 0 else None
        observer = None if observe_plan is None else Accumulator(observe_plan, m_d, seg, hold_d, dev)
        n_launches = 0
        g = out = None
        for k in range(steps + 1):
            last = k == steps
            g, out, fx, ex = forces(pos, want_atomic_virial=want_atomic_virial and last)
            if traj is not None and k % traj_every == 0:
                traj[k // traj_every].copy_(pos)   # x_k: the launch below moves on to x_{k+1}
            phase = (FINISH if k > 0 else 0) | (0 if last else START)
            # a sampled step: (x_k, v_k) stands between the finishing kick and the drift -- `vel` holds v_k after a FINISH launch
            # (step 0: as it is), `pos` holds x_k until a START launch
            sampled = observer is not None and k % observer.obs.every == 0
            halves = ([p for p in (FINISH, START) if phase & p] or [0]) if sampled else [phase]
            if sampled and not phase & FINISH:
                observer.sample(pos, vel)
            for half in halves:
                md_step(pos, vel, out['forces'], m_d, seg, id_d, kT_d, step_index, e_kin, dt, c1, c2, seed, half, fx, hold_d)
                n_launches += 1
                if sampled and half == FINISH:
                    observer.sample(pos, vel)
            if k % log_every == 0:   # e_kin is the kinetic energy of v_k, the potential energy that of x_k
                j = k // log_every
                e_pot_log[j].copy_(out['energy_per_system'] if ex is None else out['energy_per_system'] + ex)
                e_kin_log[j].copy_(e_kin)
    info = dict(n_force_calls=forces.n_force_calls, md_launches=n_launches, system_steps_evaluated=forces.system_steps_evaluated)
    if observer is not None:
        info['observe_samples'] = observer.n_samples
    return g, out, dict(pos=pos, vel=vel, e_pot=e_pot_log, e_kin=e_kin_log, traj=traj, step_index=step_index, observe=observer), info


def md_npt_loop(forces: BatchForces, positions, cells, mass: np.ndarray, vel0: Optional[np.ndarray], kT: np.ndarray, ids: np.ndarray,
                p0: np.ndarray, beta_over_tau: np.ndarray, *, dt: float, steps: int, friction: float, seed: int, log_every: int,
                traj_every: int, remove_com: bool, want_atomic_virial: bool, max_log_volume_step: float, min_height: float):
    """`md_loop` at constant pressure: the force call reads the cells from the device (`cells_dev`), and one `snet_mdb_npt_step`
    launch per step takes the engine's `virial_per_system` and `forces.virial_extra`.  cells [B,3,3]: the caller's, where the
    run starts.  -> as `md_loop`, the state also with cell [B,9], volume and pressure [samples,B] and active / status [B]; nothing
    is read back while the loop runs"""
    dev = forces.engine.dev
    n_atoms = forces.n_atoms
    B, steps, log_every, traj_every = len(n_atoms), int(steps), int(log_every), int(traj_every)
    c1, c2 = langevin_coefficients(friction, dt)
    up = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a, dtype)).to(dev)  # noqa: E731
    with torch.cuda.device(dev):
        pos = (positions.to(dev, torch.float64) if isinstance(positions, torch.Tensor)
               else up(positions, np.float64)).reshape(-1, 3).clone()
        N = int(pos.shape[0])
        cell = up(np.asarray(cells, np.float64).reshape(B, 9), np.float64)
        m_d, kT_d, id_d, seg = up(mass, np.float64), up(kT, np.float64), up(ids, np.int32), up(forces.a_ptr, np.int32)
        p0_d, bt_d = up(p0, np.float64), up(beta_over_tau, np.float64)
        if vel0 is None:
            vel = torch.empty_like(pos)
            init_velocities(vel, m_d, seg, id_d, kT_d, seed, remove_com)
        else:
            vel = up(vel0, np.float64)
        step_index = torch.zeros(B, dtype=torch.int32, device=dev)
        active = torch.ones(B, dtype=torch.int32, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)
        e_kin, volume, pressure = (torch.zeros(B, dtype=torch.float64, device=dev) for _ in range(3))
        e_pot_log = torch.zeros(steps // log_every + 1, B, dtype=torch.float64, device=dev)
        e_kin_log, volume_log, pressure_log = (torch.zeros_like(e_pot_log) for _ in range(3))
        traj = torch.zeros(steps // traj_every + 1, N, 3, dtype=torch.float64, device=dev) if traj_every > 0 else None
        g = out = None
        for k in range(steps + 1):
            last = k == steps
            g, out, fx, ex = forces(pos, want_atomic_virial=want_atomic_virial and last, cells_dev=cell)
            if traj is not None and k % traj_every == 0:
                traj[k // traj_every].copy_(pos)
            md_npt_step(pos, vel, cell, out['forces'], out['virial_per_system'], m_d, seg, id_d, kT_d, p0_d, bt_d, step_index, e_kin,
                        volume, pressure, active, status, dt, c1, c2, seed, (FINISH if k > 0 else 0) | (0 if last else START),
                        max_log_volume_step, min_height, fx, forces.virial_extra)
            if k % log_every == 0:   # kinetic energy, volume and pressure of step k: v_k, and the cell the forces were evaluated at
                j = k // log_every
                e_pot_log[j].copy_(out['energy_per_system'] if ex is None else out['energy_per_system'] + ex)
                e_kin_log[j].copy_(e_kin)
                volume_log[j].copy_(volume)
                pressure_log[j].copy_(pressure)
    info = dict(n_force_calls=forces.n_force_calls, md_launches=steps + 1, system_steps_evaluated=forces.system_steps_evaluated)
    state = dict(pos=pos, vel=vel, cell=cell, e_pot=e_pot_log, e_kin=e_kin_log, volume=volume_log, pressure=pressure_log, traj=traj,
                 step_index=step_index, active=active, status=status)
    return g, out, state, info


def attach_md(results: List[Dict[str, Any]], state: dict, seg_ptr_host, n_atoms, hold: Optional[np.ndarray] = None) -> List[Dict[str, Any]]:
    """`positions`, `velocities`, `e_pot`, `e_kin`, `temperature` (and `trajectory`) into each system's results dict: the one
    transfer to the host.  hold (int32 [N], fixed.hold_masks): a system with held components has 3 n - (held components) degrees
    of freedom in `temperature`, and 0.0 K where none is left"""
    n_held = None if hold is None else held_components(hold).sum(1)
    pos_h, vel_h = state['pos'].cpu().numpy(), state['vel'].cpu().numpy()
    e_pot, e_kin = state['e_pot'].cpu().numpy(), state['e_kin'].cpu().numpy()
    traj = None if state['traj'] is None else state['traj'].cpu().numpy()
    for b, res in enumerate(results):
        a0, a1 = int(seg_ptr_host[b]), int(seg_ptr_host[b + 1])
        res['positions'], res['velocities'] = pos_h[a0:a1].copy(), vel_h[a0:a1].copy()
        res['e_pot'], res['e_kin'] = e_pot[:, b].copy(), e_kin[:, b].copy()
        res['temperature'] = 2.0 * res['e_kin'] / (3.0 * int(n_atoms[b]) * KB)
        held = 0 if n_held is None else int(n_held[a0:a1].sum())
        if held:
            dof = 3 * int(n_atoms[b]) - held
            res['temperature'] = 2.0 * res['e_kin'] / (dof * KB) if dof else np.zeros_like(res['e_kin'])
        if traj is not None:
            res['trajectory'] = traj[:, a0:a1].copy()
    return results


def attach_npt(results: List[Dict[str, Any]], state: dict, cells_host: np.ndarray) -> List[Dict[str, Any]]:
    """`cell`, `volume`, `pressure` and `status` of a constant-pressure run into each system's results dict"""
    volume, pressure = state['volume'].cpu().numpy(), state['pressure'].cpu().numpy()
    status = state['status'].cpu().numpy()
    for b, res in enumerate(results):
        res['cell'] = cells_host[b].copy()
        res['volume'], res['pressure'] = volume[:, b].copy(), pressure[:, b].copy()
        res['status'] = NPT_STATUS_NAMES[int(status[b])]
    return results


def md_batch(engine, types, positions, masses, cells, pbcs, *, cutoff: float, dt: float, steps: int, temperature=None,
             friction: float = 0.0, velocities=None, seed: int = 0, log_every: int = 1, traj_every: int = 0, remove_com: bool = True,
             extra: Optional[Callable] = None, n_atoms=None, want_atomic_virial: bool = False,
             system_ids=None, pressure=None, compressibility=None, barostat_time: float = 1000.0,
             max_log_volume_step: float = 0.1, fixed_list=None,
             observe: Optional[Observe] = None) -> Tuple[List[Dict[str, Any]], Dict[str, int]]:
    """`steps` MD steps of `dt` fs for B structures: NVE (friction 0) or Langevin at `temperature` at fixed cells, or with
    `pressure` isotropic NPT, the cells moving on the device.

    engine: a HipForceEngine.  types / positions / cells / pbcs (and n_atoms for flat arrays) as `build_batch_graph`; masses (amu)
    and velocities (A/fs) per system or flat like the positions; the caller's arrays are not modified.  temperature (K): a
    scalar or one value per system; friction: gamma in 1/fs (> 0 needs a temperature).  velocities None: drawn at
    `temperature` on the device (`remove_com`: each system's centre of mass at rest, kinetic energy (3 n - 3) kT / 2
    exactly).  seed: of the noise (thermostat and draw); two runs with one seed give identical bits.  system_ids: the id each
    system's noise is counted under, default 0..B-1 -- a system run alone under the id it had in a batch sees the same noise.
    extra: optional callable with the contract of `batch.BatchForces` (positions fp64 [N,3] on the device, seg_ptr int64 [B+1]
    on the host, ids int64 [B]: the index of each system in this call) -> forces [N,3], or (forces, energy_per_system [B]),
    added to the model's each step (the energies go into the potential-energy log).  An extra that also returns a virial
    (`provides_virial = True`, d3.D3DeviceTerm) is taken as well; at fixed cells its virial is not used.

    Schedule: F0 = f(x0), one launch that starts step 1; then per step Fk = f(xk) and one launch that finishes step k and
    starts step k + 1 (the last one only finishes).  steps = 0: one force call, one launch that moves nothing.

    Returns (results, info).  results[b]: the dict of SevenNetCalculator.compute_many from the LAST engine call, which is at
    the returned positions, plus `positions` and `velocities` [n,3] fp64, `e_pot`, `e_kin` (eV) and `temperature`
    (2 e_kin / (3 n KB), K) over the logged steps -- sample j belongs to step j log_every -- and `trajectory` [frames,n,3]
    (step j traj_every) when traj_every > 0.  info: n_force_calls == md_launches == steps + 1, system_steps_evaluated ==
    B (steps + 1).  Invalid input raises ValueError before any device work.

    pressure (eV/A^3, a scalar or one value per system; None: fixed cells, the path above bit for bit): constant-pressure MD by
    stochastic cell rescaling (Bernetti, Bussi, J. Chem. Phys. 153, 114107 (2020), isotropic; include/snet_hip.h,
    snet_mdb_npt_step): each step scales cell, positions and inverse velocities by exp(de / 3), de = -(compressibility /
    barostat_time) (pressure - P) dt + sqrt(2 kT compressibility dt / (V barostat_time)) xi, P = (2 e_kin + tr virial) / (3 V)
    the instantaneous pressure at that step.  compressibility (A^3/eV, > 0, required; a scalar or one value per system): the
    isothermal compressibility the coupling is scaled by -- an estimate is enough, it sets the relaxation time only;
    barostat_time (fs).  Without a temperature (kT = 0) the noise term vanishes and the cell relaxes deterministically.  Every
    system must be periodic along all three axes and one of the batched neighbor kernel (at most batch.BATCH_MAX_ATOMS atoms,
    no height below cutoff / 64); a plain `extra` is refused, one marked `provides_virial = True` adds its virial to P.  The
    results gain `cell` [3,3] fp64 (energy, forces and stress are those at the returned positions AND cell), `volume` (A^3) and
    `pressure` (eV/A^3) over the logged steps, and `status`: 'ok', or 'cell_failed' where the step kernel refused a next cell
    (de not finite -- a NaN virial --, |de| > max_log_volume_step, or a height below cutoff / 64): that system is returned as it
    was before that step and stays in the batch, measured and not moved.

    fixed_list: the atoms and Cartesian components that do not move: per system None, a bool mask [n] or an integer index list of
    whole atoms, or a bool mask [n,3] of components (fixed.hold_masks).  The step kernel (snet_mdb_step_fixed) gives a held
    component no kick, no drift and no thermostat noise: its position keeps the caller's bits, its velocity is 0 and it adds
    nothing to `e_kin`; the free components see the arithmetic and the noise they see without a mask.  Held components of
    caller-supplied `velocities` are set to 0 (as ASE's set_momenta does under a constraint).  Drawn velocities: a system with
    held components is not shifted to its centre of mass -- the held atoms anchor the frame -- and with remove_com its kinetic
    energy is dof kT / 2 exactly, dof = 3 n - (held components), which is also the dof of its `temperature` (0.0 K where dof = 0);
    a system with nothing held keeps 3 n.  `forces` stay the model's true forces, on held atoms too.  Together with `pressure`
    fixed_list raises ValueError: constant-pressure MD with frozen atoms is not a defined ensemble here.  When something is held
    the results gain `fixed`, a bool array [n,3]; with fixed_list None, or masks that hold nothing, the call is the one without
    the argument: the same launches, the same dicts.

    observe (observe.Observe; None: nothing is sampled, the launches and dicts above): the radial distribution function, the
    mean-square displacement and the velocity autocorrelation function accumulated on the device (sevennet_amd.observe;
    snet_obs_rdf, snet_obs_correlate).  (x_k, v_k) is sampled at every step k that is a multiple of observe.every, v_k after the
    finishing half kick: steps // every + 1 samples.  The launch of a sampled step is issued in its two halves around the
    observe launches (`info['md_launches']` counts them, `info['observe_samples']` the samples); positions, velocities, `e_pot`,
    `e_kin` and `trajectory` keep the bits of the run without `observe`.  Each dict gains `observables`
    (observe.attach_observables).  Together with `pressure` it raises ValueError: displacements under a rescaled cell are not
    defined here, and the constant-pressure RDF is not provided."""
    types, positions, n_at, cells, pbcs = validate_batch_inputs(types, positions, cells, pbcs, cutoff, engine.spec.num_species,
                                                                n_atoms=n_atoms)
    mass, vel0, kT, ids = validate_md_inputs(masses, n_at, dt, steps, temperature, friction, velocities, seed, log_every, traj_every,
                                             system_ids)
    hold = hold_masks(fixed_list, n_at)
    if observe is not None and pressure is not None:
        raise ValueError('observe with pressure: the mean-square displacement under a rescaled cell is not defined here, and the '
                         'constant-pressure RDF is not provided; run at fixed cells, or without observe')
    plan = None if observe is None else make_observe_plan(observe, types, n_at, cells, pbcs)
    if pressure is not None:
        if fixed_list is not None:
            raise ValueError('fixed_list with pressure: constant-pressure MD with atoms held fixed is not a defined ensemble here '
                             '(the barostat rescales every position); run at fixed cells, or without fixed_list')
        p0, beta_over_tau = validate_npt_inputs(n_at, cells, pbcs, cutoff, pressure, compressibility, barostat_time,
                                                max_log_volume_step, extra)
        forces = BatchForces(engine, types, n_at, cells, pbcs, cutoff, extra)
        g, out, state, info = md_npt_loop(forces, positions, cells, mass, vel0, kT, ids, p0, beta_over_tau, dt=dt, steps=steps,
                                          friction=friction, seed=seed, log_every=log_every, traj_every=traj_every,
                                          remove_com=remove_com, want_atomic_virial=want_atomic_virial,
                                          max_log_volume_step=max_log_volume_step, min_height=cutoff / _MAX_IMAGE_REACH)
        cells_h = state['cell'].cpu().numpy().reshape(-1, 3, 3)
        results = attach_md(batch_results(g, out, cells_h, want_atomic_virial), state, g.seg_ptr_host, n_at)
        return attach_npt(results, state, cells_h), info
    forces = BatchForces(engine, types, n_at, cells, pbcs, cutoff, extra)
    g, out, state, info = md_loop(forces, positions, mass, vel0, kT, ids, dt=dt, steps=steps, friction=friction, seed=seed,
                                  log_every=log_every, traj_every=traj_every, remove_com=remove_com,
                                  want_atomic_virial=want_atomic_virial, hold=hold, observe_plan=plan)
    results = attach_md(batch_results(g, out, cells, want_atomic_virial), state, g.seg_ptr_host, n_at, hold)
    if plan is not None:
        attach_observables(results, plan, state['observe'].to_host(), dt)
    return (results if hold is None else attach_fixed(results, hold, g.seg_ptr_host)), info
