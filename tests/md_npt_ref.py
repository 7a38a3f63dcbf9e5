"""fp64 numpy restatement of the batched NPT MD step (the rule of include/snet_hip.h, snet_mdb_npt_step): the reference for the
kernel.

BAOAB folded around the force call (md_ref.md_step) with the isotropic stochastic cell rescaling of Bernetti and Bussi, J. Chem.
Phys. 153, 114107 (2020), after both kicks and before the drift.  Units eV, A, fs, amu.  State of one system: dict(pos [n,3],
vel [n,3], cell [3,3], step, active, status).  `npt_step` returns the next state, the kinetic energy, the volume and the
pressure; it never modifies its input."""
import numpy as np

import md_ref
from md_ref import ACC, FINISH, KB, START, STREAM_THERMOSTAT

STREAM_BAROSTAT = 2


def npt_init(pos, cell, vel=None, step=0):
    s = md_ref.md_init(pos, vel, step)
    s.update(cell=np.array(cell, np.float64).reshape(3, 3), active=1, status=0)
    return s


def min_height(cell):
    """the smallest face-to-face height of the cell (row vectors)"""
    vol = abs(np.linalg.det(cell))
    return min(vol / np.linalg.norm(np.cross(cell[(i + 1) % 3], cell[(i + 2) % 3])) for i in range(3))


def pressure_of(e_kin, virial, volume):
    """(2 K + tr W) / (3 V) for the engine's virial (order xx,yy,zz,xy,yz,zx; stress = -W / V)"""
    w = np.asarray(virial, np.float64).reshape(-1)
    return (2.0 * e_kin + (w[0] + w[1] + w[2])) / (3.0 * volume)


def barostat_noise(seed, sys_id, step):
    """xi_s: the first normal of atom word 0 under the barostat's stream tag"""
    return float(md_ref.normals(seed, sys_id, 1, step, STREAM_BAROSTAT)[0, 0])


def npt_step(state, forces, virial, mass, kT, p0, beta_over_tau, dt, c1, c2, seed, sys_id, phase, max_log_volume_step, min_height_bound):
    """one launch's worth for one system, with the forces and the virial [6] at state['pos'] and state['cell'] (the forces
    ignored when phase is 0) -> (next state, e_kin, volume, pressure).  A system with active == 0 is taken at phase 0."""
    s = dict(state, pos=state['pos'].copy(), vel=state['vel'].copy(), cell=state['cell'].copy())
    if not s['active']:
        phase = 0
    m = np.asarray(mass, np.float64).reshape(-1, 1)
    x, v, cell = s['pos'], s['vel'], s['cell']
    with np.errstate(all='ignore'):
        kick = 0.0 if phase == 0 else (0.5 * dt) * ACC * np.asarray(forces, np.float64).reshape(-1, 3) / m
        if phase & FINISH:
            v = v + kick
        e_kin = float(0.5 * (m * v * v).sum() / ACC)
        volume = float(abs(np.linalg.det(cell)))
        pressure = float(pressure_of(e_kin, virial, volume))
        if phase & START:
            v = v + kick
            de = -beta_over_tau * (p0 - pressure) * dt
            amp = np.sqrt(2.0 * kT * beta_over_tau * dt / volume)
            if amp != 0.0:
                de = de + amp * barostat_noise(seed, sys_id, s['step'])
            mu = np.exp(de / 3.0)
            new_cell = mu * cell
            ok = bool(np.isfinite(de) and abs(de) <= max_log_volume_step and np.isfinite(new_cell).all()
                      and min_height(new_cell) >= min_height_bound)
            if not ok:   # refused: nothing of the state moves, the finishing kick included
                s['active'], s['status'] = 0, 2
                return s, e_kin, volume, pressure
            x, v, cell = mu * x, v / mu, new_cell
            if c2 == 0:
                x = x + dt * v
            else:
                x = x + (0.5 * dt) * v
                v = c1 * v + c2 * np.sqrt(kT * ACC / m) * md_ref.normals(seed, sys_id, len(x), s['step'], STREAM_THERMOSTAT)
                x = x + (0.5 * dt) * v
            s['step'] += 1
    s['pos'], s['vel'], s['cell'] = x, v, cell
    return s, e_kin, volume, pressure


def npt_run(pos, cell, force_fn, mass, dt, steps, p0, beta_over_tau, vel=None, temperature=None, friction=0.0, seed=0, sys_id=0,
            remove_com=True, max_log_volume_step=0.1, min_height_bound=0.0):
    """`steps` steps of one system: force_fn(pos, cell) -> (e_pot, forces, virial [6]).  The schedule of md_ref.md_run -> dict(pos,
    vel, cell, e_pot, e_kin, volume, pressure [steps + 1], traj [steps + 1, n, 3], cells [steps + 1, 3, 3], step, status)"""
    kT = 0.0 if temperature is None else KB * float(temperature)
    if vel is None:
        vel = md_ref.init_velocities(mass, kT, seed, sys_id, remove_com)
    c1, c2 = md_ref.langevin_coefficients(friction, dt)
    s = npt_init(pos, cell, vel)
    log = dict(e_pot=[], e_kin=[], volume=[], pressure=[], traj=[], cells=[])
    for k in range(steps + 1):
        e, f, w = force_fn(s['pos'], s['cell'])
        log['traj'].append(s['pos'].copy())
        log['cells'].append(s['cell'].copy())
        s, ek, vol, pr = npt_step(s, f, w, mass, kT, p0, beta_over_tau, dt, c1, c2, seed, sys_id,
                                  (FINISH if k > 0 else 0) | (START if k < steps else 0), max_log_volume_step, min_height_bound)
        for key, val in (('e_pot', float(e)), ('e_kin', ek), ('volume', vol), ('pressure', pr)):
            log[key].append(val)
    out = {k: np.asarray(v) for k, v in log.items()}
    out.update(pos=s['pos'], vel=s['vel'], cell=s['cell'], step=s['step'], status=s['status'])
    return out


def normals_many(seed, sys_ids, n, steps, stream_tag):
    """md_ref.normals for many systems at once: atoms 0..n-1 of the systems `sys_ids` [B], each at its own step [B] -> [B,n,3]"""
    seed, B = int(seed), len(sys_ids)
    ctr = np.zeros((B, n, 4), np.uint64)
    ctr[..., 0] = np.arange(n)
    ctr[..., 1] = np.asarray(sys_ids, np.uint64)[:, None]
    ctr[..., 2] = np.asarray(steps, np.uint64)[:, None]
    ctr[..., 3] = int(stream_tag)
    u = (md_ref.philox4x32(ctr, [seed & 0xffffffff, seed >> 32]).astype(np.float64) + 0.5) * 2.0 ** -32
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    return np.stack([r0 * np.cos(2.0 * np.pi * u[..., 1]), r0 * np.sin(2.0 * np.pi * u[..., 1]), r1 * np.cos(2.0 * np.pi * u[..., 3])], -1)


def free_gas_run(pos, vel, cells, mass, kT, p0, beta_over_tau, dt, c1, c2, seed, sys_ids, steps, max_log_volume_step, min_height_bound):
    """`npt_step` for B systems of n atoms each without forces or virial, all at once: pos / vel [B,n,3], cells [B,3,3], mass [n],
    the schedule of npt_run -> (pos, vel, cells, volume [steps + 1, B], e_kin [steps + 1, B]).  The same operations in the same
    order as npt_step (tests/test_md_npt_cpu.py holds the two against each other); a step the guard would refuse raises."""
    x, v, cell = (np.array(a, np.float64) for a in (pos, vel, cells))
    B, n = x.shape[:2]
    m = np.asarray(mass, np.float64).reshape(1, n, 1)
    sys_ids, step = np.asarray(sys_ids), np.zeros(B, np.int64)
    vol_log, ek_log = np.zeros((steps + 1, B)), np.zeros((steps + 1, B))
    for k in range(steps + 1):
        e_kin = 0.5 * (m * v * v).sum((1, 2)) / ACC   # (zero forces: the kicks add 0.0)
        volume = np.abs(np.linalg.det(cell))
        pressure = (2.0 * e_kin + 0.0) / (3.0 * volume)
        vol_log[k], ek_log[k] = volume, e_kin
        if k == steps:
            break
        de = -beta_over_tau * (p0 - pressure) * dt
        amp = np.sqrt(2.0 * kT * beta_over_tau * dt / volume)
        if amp.any():
            de = de + amp * normals_many(seed, sys_ids, 1, step, STREAM_BAROSTAT)[:, 0, 0]
        mu = np.exp(de / 3.0)
        cell = mu[:, None, None] * cell
        if not (np.isfinite(de).all() and (np.abs(de) <= max_log_volume_step).all()
                and np.isfinite(cell).all() and (min_height_bound <= 0 or all(min_height(c) >= min_height_bound for c in cell))):
            raise RuntimeError(f'step {k}: the guard would refuse a cell (largest |de| {np.abs(de).max():.3g})')
        x, v = mu[:, None, None] * x, v / mu[:, None, None]
        if c2 == 0:
            x = x + dt * v
        else:
            x = x + (0.5 * dt) * v
            v = c1 * v + c2 * np.sqrt(kT * ACC / m) * normals_many(seed, sys_ids, n, step, STREAM_THERMOSTAT)
            x = x + (0.5 * dt) * v
        step = step + 1
    return x, v, cell, vol_log, ek_log
