"""fp64 numpy restatement of one FIRE step (the rule of include/snet_hip.h, snet_fire_step): the reference for the kernel.

State of one system: dict(pos [n,3], vel [n,3], dt, alpha, n_pos, active, n_steps).  `fire_step` returns the next state and
what the step did (fm, P, branch, clipped); it never modifies its input."""
import numpy as np

FIRE = dict(dt_start=0.1, dt_max=1.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, max_step=0.2)


def fire_init(pos, **fire):
    p = dict(FIRE, **fire)
    pos = np.array(pos, np.float64).reshape(-1, 3)
    return dict(pos=pos, vel=np.zeros_like(pos), dt=float(p['dt_start']), alpha=float(p['alpha_start']), n_pos=0, active=1, n_steps=0)


def fire_step(state, forces, fmax, **fire):
    """one step of one system with the forces at state['pos'] (any float dtype, used in fp64) -> (next state, what happened)"""
    p = dict(FIRE, **fire)
    s = dict(state, pos=state['pos'].copy(), vel=state['vel'].copy())
    what = dict(fm=None, P=None, cos=None, branch=None, clipped=False)
    if s['active'] != 1:
        return s, what
    f = np.asarray(forces, np.float64).reshape(-1, 3)
    v = s['vel']
    fm = float(np.sqrt((f * f).sum(1).max()))
    what['fm'] = fm
    if fm < fmax:
        s['active'] = 0
        return s, what
    P = float((f * v).sum())
    nf, nv = np.sqrt((f * f).sum()), np.sqrt((v * v).sum())
    what['P'], what['cos'] = P, (P / (nf * nv) if nf * nv > 0 else 0.0)
    if P > 0:
        v = (1 - s['alpha']) * v + s['alpha'] * f / nf * nv
        if s['n_pos'] > p['n_min']:
            s['dt'] = min(s['dt'] * p['f_inc'], p['dt_max'])
            s['alpha'] = s['alpha'] * p['f_alpha']
        s['n_pos'] += 1
        what['branch'] = 'downhill'
    else:
        v = np.zeros_like(v)
        s['alpha'] = p['alpha_start']
        s['dt'] = s['dt'] * p['f_dec']
        s['n_pos'] = 0
        what['branch'] = 'uphill'
    v = v + s['dt'] * f
    dr = s['dt'] * v
    n = np.sqrt((dr * dr).sum())
    if n > p['max_step']:
        dr = dr * (p['max_step'] / n)
        what['clipped'] = True
    s['pos'] = s['pos'] + dr
    s['vel'] = v
    s['n_steps'] += 1
    return s, what


def fire_relax(pos, force_fn, fmax, steps, **fire):
    """relax one system: force_fn(pos) -> forces.  -> (final state, list of `what` per force evaluation, list of dt per move)"""
    s = fire_init(pos, **fire)
    log, dts = [], []
    for _ in range(steps):
        s, what = fire_step(s, force_fn(s['pos']), fmax, **fire)
        log.append(what)
        if s['active'] != 1:
            break
        dts.append(s['dt'])
    return s, log, dts
