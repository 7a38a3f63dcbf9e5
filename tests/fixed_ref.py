"""fp64 numpy restatements of the masked step kernels (the `*_fixed` rules of include/snet_hip.h), built on the restatements of
the unmasked ones: relax_ref, cellrelax_ref and md_ref do the step on masked inputs, and this module says what a mask changes.

hold: int [n], bit k (k = 0, 1, 2) of a word says that Cartesian component k of that atom is held.  A held component enters a
step with force 0 and velocity 0 -- by selection, so that a NaN there goes nowhere -- and leaves it with the position it came
with.  Nothing here modifies its input."""
import numpy as np

import cellrelax_ref
import md_ref
import relax_ref


def components(hold):
    """hold [n] -> bool [n,3]"""
    return ((np.asarray(hold, np.int64).reshape(-1, 1) >> np.arange(3)) & 1).astype(bool)


def _free(held, x):
    return np.where(held, 0.0, np.asarray(x, np.float64).reshape(-1, 3))


def fire_step(state, forces, hold, fmax, **fire):
    """relax_ref.fire_step on (velocities with held components zeroed, forces with held components 0), held positions restored.
    A step that moves nothing (an inactive system, or one found converged) leaves the velocity array as it was."""
    held = components(hold)
    s, what = relax_ref.fire_step(dict(state, vel=_free(held, state['vel'])), _free(held, forces), fmax, **fire)
    s['pos'] = np.where(held, state['pos'], s['pos'])
    if s['n_steps'] == state['n_steps']:
        s['vel'] = state['vel'].copy()
    return s, what


def fire_relax(pos, force_fn, hold, fmax, steps, **fire):
    """relax one system under a mask: force_fn(pos) -> forces.  -> (final state, list of `what` per force evaluation)"""
    s = relax_ref.fire_init(pos, **fire)
    log = []
    for _ in range(steps):
        s, what = fire_step(s, force_fn(s['pos']), hold, fmax, **fire)
        log.append(what)
        if s['active'] != 1:
            break
    return s, log


def cell_fire_step(state, forces, virial, hold, fmax, min_h=0.0, forces_extra=None, virial_extra=None, opts=None, **fire):
    """cellrelax_ref.cell_fire_step with whole atoms held (a nonzero word): their Cartesian forces and reference-frame velocities
    enter as 0.  Their positions are NOT restored: with g = 0 and v = 0 the step leaves their coordinates in the reference frame
    alone and r = s F_new^T carries them with the cell."""
    held = np.repeat((np.asarray(hold, np.int64).reshape(-1, 1) & 7) != 0, 3, axis=1)
    fx = None if forces_extra is None else _free(held, forces_extra)
    s, what = cellrelax_ref.cell_fire_step(dict(state, vel=_free(held, state['vel'])), _free(held, forces), virial, fmax, min_h, fx,
                                           virial_extra, opts=opts, **fire)
    if s['n_steps'] == state['n_steps']:
        s['vel'] = state['vel'].copy()
    return s, what


def md_step(state, forces, hold, mass, kT, dt, c1, c2, seed, sys_id, phase):
    """md_ref.md_step on the same masked inputs, then held positions restored and held velocities zeroed (the thermostat's noise
    on a held component goes nowhere).  The finishing kick leaves a held v at 0, so e_kin needs no correction.  Phase 0 stores
    nothing: the velocity array stays as it was."""
    held = components(hold)
    s, e_kin = md_ref.md_step(dict(state, vel=_free(held, state['vel'])), _free(held, forces), mass, kT, dt, c1, c2, seed, sys_id, phase)
    s['pos'] = np.where(held, state['pos'], s['pos'])
    s['vel'] = state['vel'].copy() if phase == 0 else np.where(held, 0.0, s['vel'])
    return s, e_kin


def init_velocities(mass, hold, kT, seed, sys_id, remove_com=True):
    """the velocity draw under a mask: a system with nothing held is md_ref.init_velocities; otherwise held components are 0, the
    centre of mass is left alone, and with remove_com the kinetic energy is dof kT / 2, dof = 3 n - (held components) -- all
    zeros where dof = 0"""
    held = components(hold)
    if not held.any():
        return md_ref.init_velocities(mass, kT, seed, sys_id, remove_com)
    m = np.asarray(mass, np.float64).reshape(-1, 1)
    n = len(m)
    v = np.where(held, 0.0, np.sqrt(kT * md_ref.ACC / m) * md_ref.normals(seed, sys_id, n, 0, md_ref.STREAM_INIT))
    if remove_com:
        dof = 3 * n - int(held.sum())
        e_now = 0.5 * (m * v * v).sum() / md_ref.ACC
        v = v * (np.sqrt(0.5 * dof * kT / e_now) if e_now > 0 else 0.0)
    return v


def md_run(pos, force_fn, hold, mass, dt, steps, vel, temperature=None, friction=0.0, seed=0, sys_id=0):
    """md_ref.md_run under a mask, from given velocities (their held components are taken as 0)"""
    kT = 0.0 if temperature is None else md_ref.KB * float(temperature)
    c1, c2 = md_ref.langevin_coefficients(friction, dt)
    s = md_ref.md_init(pos, np.where(components(hold), 0.0, vel))
    e_pot, e_kin, traj = [], [], []
    for k in range(steps + 1):
        e, f = force_fn(s['pos'])
        traj.append(s['pos'].copy())
        s, ek = md_step(s, f, hold, mass, kT, dt, c1, c2, seed, sys_id, (md_ref.FINISH if k > 0 else 0) | (md_ref.START if k < steps else 0))
        e_pot.append(float(e))
        e_kin.append(ek)
    return dict(pos=s['pos'], vel=s['vel'], e_pot=np.asarray(e_pot), e_kin=np.asarray(e_kin), traj=np.asarray(traj), step=s['step'])
