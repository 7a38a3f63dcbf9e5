"""fp64 numpy restatement of one variable-cell FIRE step (the rule of include/snet_hip.h, snet_fire_cell_step): the reference
for the kernel.  One function per step of the rule, then the step and a loop, in the style of relax_ref.

State of one system: dict(pos [n,3], vel [n,3], cell [3,3], cell0 [3,3], vel_cell [3,3], dt, alpha, n_pos, active, n_steps,
status).  `cell_fire_step` returns the next state and what the step did (fm, P, branch, clipped, guard, F_new); it never modifies its input."""
import numpy as np

from relax_ref import FIRE

CELL = dict(scalar_pressure=0.0, cell_mask=(1, 1, 1, 1, 1, 1), hydrostatic_strain=False, constant_volume=False)
_VOIGT = np.array([[0, 5, 4], [5, 1, 3], [4, 3, 2]])   # xx,yy,zz,yz,xz,xy


def deformation(cell, cell0):
    """F = (C0^-1 C)^T, so that C = C0 F^T"""
    return (np.linalg.inv(cell0) @ cell).T


def virial_matrix(w6):
    """the symmetric 3x3 of a virial in the engine's order xx,yy,zz,xy,yz,zx"""
    w = np.asarray(w6, np.float64)
    return np.array([[w[0], w[3], w[5]], [w[3], w[1], w[4]], [w[5], w[4], w[2]]])


def mask_matrix(cell_mask):
    """the symmetric 0/1 matrix of six Voigt flags xx,yy,zz,yz,xz,xy"""
    return np.asarray(cell_mask, np.float64)[_VOIGT]


def cell_force(virial, F, volume, n, scalar_pressure=0.0, cell_mask=(1, 1, 1, 1, 1, 1), hydrostatic_strain=False,
               constant_volume=False, virial_extra=None):
    """the force on the rows of n F: (W - p V I) F^-T, projected, over n"""
    W = virial_matrix(virial)
    if virial_extra is not None:
        W = W + virial_matrix(virial_extra)
    W = W - scalar_pressure * volume * np.eye(3)
    G = W @ np.linalg.inv(F).T
    if hydrostatic_strain:
        G = np.eye(3) * (np.trace(G) / 3.0)
    G = G * mask_matrix(cell_mask)
    if constant_volume:
        G = G - np.eye(3) * (np.trace(G) / 3.0)
    return G / n


def atom_forces(forces, F):
    """g_i = f_i F: the forces on the atoms' coordinates in the reference frame"""
    return np.asarray(forces, np.float64).reshape(-1, 3) @ F


def generalised(state, forces, virial, forces_extra=None, virial_extra=None, **cell):
    """-> (F, coordinates [n+3,3], velocities [n+3,3], forces [n+3,3]) of a state"""
    c = dict(CELL, **cell)
    n = len(state['pos'])
    F = deformation(state['cell'], state['cell0'])
    f = np.asarray(forces, np.float64).reshape(-1, 3)
    if forces_extra is not None:
        f = f + np.asarray(forces_extra, np.float64).reshape(-1, 3)
    G = cell_force(virial, F, abs(np.linalg.det(state['cell'])), n, virial_extra=virial_extra, **c)
    q = np.concatenate([state['pos'] @ np.linalg.inv(F).T, n * F])
    return F, q, np.concatenate([state['vel'], state['vel_cell']]), np.concatenate([atom_forces(f, F), G])


def min_height(cell):
    """the smallest face-to-face height of a cell"""
    return float((1.0 / np.linalg.norm(np.linalg.inv(cell), axis=0)).min())


def guard_passes(F_new, cell0, min_h):
    """the new deformation gradient is finite and not inverted, and the new cell no flatter than min_h"""
    if not np.isfinite(F_new).all() or not np.linalg.det(F_new) > 0:
        return False
    return min_height(cell0 @ F_new.T) >= min_h


def cell_fire_init(pos, cell, cell0=None, **fire):
    p = dict(FIRE, **fire)
    pos = np.array(pos, np.float64).reshape(-1, 3)
    cell = np.array(cell, np.float64).reshape(3, 3)
    return dict(pos=pos, vel=np.zeros_like(pos), cell=cell, cell0=cell.copy() if cell0 is None else np.array(cell0, np.float64),
                vel_cell=np.zeros((3, 3)), dt=float(p['dt_start']), alpha=float(p['alpha_start']), n_pos=0, active=1, n_steps=0, status=0)


def cell_fire_step(state, forces, virial, fmax, min_h=0.0, forces_extra=None, virial_extra=None, opts=None, **fire):
    """one step of one system with the forces and the virial at state['pos'] / state['cell'] -> (next state, what happened);
    opts: overrides of CELL"""
    p = dict(FIRE, **fire)
    s = dict(state, **{k: state[k].copy() for k in ('pos', 'vel', 'cell', 'cell0', 'vel_cell')})
    what = dict(fm=None, P=None, cos=None, branch=None, clipped=False, guard=False, F_new=None)
    if s['active'] != 1:
        return s, what
    n = len(s['pos'])
    F, q, v, g = generalised(s, forces, virial, forces_extra, virial_extra, **(opts or {}))
    fm = float(np.sqrt((g * g).sum(1).max()))
    what['fm'] = fm
    if fm < fmax:
        s['active'], s['status'] = 0, 1
        return s, what
    dt, alpha, n_pos = s['dt'], s['alpha'], s['n_pos']
    P = float((g * v).sum())
    ng, nv = np.sqrt((g * g).sum()), np.sqrt((v * v).sum())
    what['P'], what['cos'] = P, (P / (ng * nv) if ng * nv > 0 else 0.0)
    if P > 0:
        v = (1 - alpha) * v + alpha * g / ng * nv
        if n_pos > p['n_min']:
            dt = min(dt * p['f_inc'], p['dt_max'])
            alpha = alpha * p['f_alpha']
        n_pos += 1
        what['branch'] = 'downhill'
    else:
        v = np.zeros_like(v)
        alpha = p['alpha_start']
        dt = dt * p['f_dec']
        n_pos = 0
        what['branch'] = 'uphill'
    v = v + dt * g
    dq = dt * v
    nd = np.sqrt((dq * dq).sum())
    if nd > p['max_step']:
        dq = dq * (p['max_step'] / nd)
        what['clipped'] = True
    F_new = what['F_new'] = F + dq[n:] / n
    if not np.isfinite(nd) or not guard_passes(F_new, s['cell0'], min_h):
        s['active'], s['status'] = 0, 2
        what['guard'], what['branch'], what['clipped'] = True, None, False
        return s, what
    s['pos'] = (q[:n] + dq[:n]) @ F_new.T
    s['cell'] = s['cell0'] @ F_new.T
    s['vel'], s['vel_cell'] = v[:n], v[n:]
    s['dt'], s['alpha'], s['n_pos'] = dt, alpha, n_pos
    s['n_steps'] += 1
    return s, what


def cell_fire_relax(pos, cell, force_fn, fmax, steps, min_h=0.0, opts=None, **fire):
    """relax one system: force_fn(pos, cell) -> (forces, virial[6]).  -> (final state, list of `what` per evaluation)"""
    s = cell_fire_init(pos, cell, **fire)
    log = []
    for _ in range(steps):
        f, w = force_fn(s['pos'], s['cell'])
        s, what = cell_fire_step(s, f, w, fmax, min_h, opts=opts, **fire)
        log.append(what)
        if s['active'] != 1:
            break
    return s, log


# ---- an analytic energy with a known minimum, for driving the loop without a model
HARMONIC = dict(k=2.0, kappa=0.004)


def harmonic_crystal(pos, cell, x0, metric0, k=HARMONIC['k'], kappa=HARMONIC['kappa']):
    """E = k/2 sum_i |r_i - x0_i C|^2 + kappa/4 |C C^T - metric0|^2 (Frobenius): atoms tied to the lattice sites of fractional
    coordinates x0, the cell tied to a metric tensor.  Rotation-invariant (r -> r R, C -> C R changes neither term), so its
    virial is symmetric, and zero exactly where r_i = x0_i C and C C^T = metric0.  numpy arrays or torch tensors (fp64) ->
    (energy, forces [n,3], virial 3x3 = -dE/d(strain) at fixed fractional coordinates)"""
    d = pos - x0 @ cell
    dm = cell @ cell.T - metric0
    energy = 0.5 * k * (d * d).sum() + 0.25 * kappa * (dm * dm).sum()
    return energy, -k * d, -k * (d.T @ d) - kappa * (cell.T @ dm @ cell)


def virial6(W):
    """the engine's order xx,yy,zz,xy,yz,zx of a symmetric 3x3"""
    return [W[0, 0], W[1, 1], W[2, 2], W[0, 1], W[1, 2], W[2, 0]]
