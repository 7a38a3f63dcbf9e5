"""fp64 numpy restatement of the batched MD step (the rule of include/snet_hip.h, snet_mdb_step): the reference for the kernel.

BAOAB folded around the force call, units eV, A, fs, amu; the noise is Philox4x32-10 (Random123 constants) through Box-Muller.
State of one system: dict(pos [n,3], vel [n,3], step).  `md_step` returns the next state and the kinetic energy; it never
modifies its input."""
import numpy as np

ACC = 9.648533212e-3    # eV / (A amu) in A / fs^2
KB = 8.617333262e-5     # eV / K
PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
STREAM_THERMOSTAT, STREAM_INIT = 0, 1
FINISH, START = 1, 2


def philox4x32(counter, key, rounds=10):
    """Philox4x32 of counter [..., 4] under key [..., 2] (broadcast against each other): -> uint32 [..., 4]"""
    c = np.asarray(counter, np.uint64) & np.uint64(0xffffffff)
    k = np.asarray(key, np.uint64) & np.uint64(0xffffffff)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    mask = np.uint64(0xffffffff)
    for r in range(rounds):
        if r > 0:
            k0 = (k0 + np.uint64(PHILOX_W[0])) & mask
            k1 = (k1 + np.uint64(PHILOX_W[1])) & mask
        p0 = np.uint64(PHILOX_M[0]) * c0      # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(PHILOX_M[1]) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def normals(seed, sys_id, n, step, stream_tag):
    """the three standard normals of atoms 0..n-1 of system `sys_id` at step `step`: fp64 [n,3]"""
    seed = int(seed)
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(n), int(sys_id), int(step), int(stream_tag)
    w = philox4x32(ctr, [seed & 0xffffffff, seed >> 32])
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(2.0 * np.pi * u[:, 1]), r0 * np.sin(2.0 * np.pi * u[:, 1]), r1 * np.cos(2.0 * np.pi * u[:, 3])], 1)


def langevin_coefficients(friction, dt):
    """(c1, c2) = (exp(-gamma dt), sqrt(1 - c1^2)); gamma = 0 gives (1, 0): NVE"""
    c1 = float(np.exp(-float(friction) * float(dt)))
    return c1, float(np.sqrt(1.0 - c1 * c1))


def kinetic_energy(mass, vel):
    return float(0.5 * (np.asarray(mass, np.float64)[:, None] * vel ** 2).sum() / ACC)


def md_init(pos, vel=None, step=0):
    pos = np.array(pos, np.float64).reshape(-1, 3)
    return dict(pos=pos, vel=np.zeros_like(pos) if vel is None else np.array(vel, np.float64).reshape(-1, 3), step=int(step))


def md_step(state, forces, mass, kT, dt, c1, c2, seed, sys_id, phase):
    """one launch's worth for one system, with the forces at state['pos'] (any float dtype, used in fp64; ignored when phase is
    0) -> (next state, e_kin)"""
    s = dict(state, pos=state['pos'].copy(), vel=state['vel'].copy())
    m = np.asarray(mass, np.float64).reshape(-1, 1)
    x, v = s['pos'], s['vel']
    kick = 0.0 if phase == 0 else (0.5 * dt) * ACC * np.asarray(forces, np.float64).reshape(-1, 3) / m
    if phase & FINISH:
        v = v + kick
    e_kin = float(0.5 * (m * v * v).sum() / ACC)
    if phase & START:
        v = v + kick
        if c2 == 0:
            x = x + dt * v
        else:
            x = x + (0.5 * dt) * v
            v = c1 * v + c2 * np.sqrt(kT * ACC / m) * normals(seed, sys_id, len(x), s['step'], STREAM_THERMOSTAT)
            x = x + (0.5 * dt) * v
        s['step'] += 1
    s['pos'], s['vel'] = x, v
    return s, e_kin


def init_velocities(mass, kT, seed, sys_id, remove_com=True):
    """Maxwell-Boltzmann velocities [n,3] at kT (eV); remove_com: centre of mass at rest and KE = (3 n - 3) kT / 2 exactly (one
    atom: zero)"""
    m = np.asarray(mass, np.float64).reshape(-1, 1)
    n = len(m)
    if remove_com and n == 1:
        return np.zeros((1, 3))
    v = np.sqrt(kT * ACC / m) * normals(seed, sys_id, n, 0, STREAM_INIT)
    if remove_com:
        v = v - (m * v).sum(0) / m.sum()
        e_now = 0.5 * (m * v * v).sum() / ACC
        v = v * (np.sqrt(0.5 * (3 * n - 3) * kT / e_now) if e_now > 0 else 0.0)
    return v


def md_run(pos, force_fn, mass, dt, steps, vel=None, temperature=None, friction=0.0, seed=0, sys_id=0, remove_com=True):
    """`steps` steps of one system: force_fn(pos) -> (e_pot, forces).  F0 = f(x0), launch START, then per step Fk = f(xk) and
    launch FINISH (+ START while steps remain) -> dict(pos, vel, e_pot[steps + 1], e_kin[steps + 1], traj[steps + 1, n, 3])"""
    kT = 0.0 if temperature is None else KB * float(temperature)
    if vel is None:
        vel = init_velocities(mass, kT, seed, sys_id, remove_com)
    c1, c2 = langevin_coefficients(friction, dt)
    s = md_init(pos, vel)
    e_pot, e_kin, traj = [], [], []
    for k in range(steps + 1):
        e, f = force_fn(s['pos'])
        traj.append(s['pos'].copy())
        s, ek = md_step(s, f, mass, kT, dt, c1, c2, seed, sys_id, (FINISH if k > 0 else 0) | (START if k < steps else 0))
        e_pot.append(float(e))
        e_kin.append(ek)
    return dict(pos=s['pos'], vel=s['vel'], e_pot=np.asarray(e_pot), e_kin=np.asarray(e_kin), traj=np.asarray(traj), step=s['step'])
