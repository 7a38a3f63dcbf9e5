"""fp64 numpy restatement of the nudged-elastic-band forces (the rule of include/snet_hip.h, snet_neb_forces: improved tangent,
springs along the tangent, climbing image) and the band FIRE loop on top of relax_ref.fire_step: the reference for the kernel
and for sevennet_amd.neb.  A band is an array [M, n, 3] of M images (both endpoints included) of the same n atoms."""
import numpy as np

import relax_ref


def pad_cell(cell, pbc):
    """the cell with the zero rows of open axes replaced by a unit vector along that axis, so that it can be inverted"""
    cell = np.array(cell, np.float64).reshape(3, 3)
    for k in range(3):
        if not pbc[k] and np.linalg.norm(cell[k]) < 1e-12:
            cell[k] = 0.0
            cell[k, k] = 1.0
    return cell


def mic(d, cell, pbc, inv=None):
    """minimum-image form of the displacements d [..., 3]: s = d inv(cell), s_k -= rint(s_k) on the periodic axes, d = s cell.
    The shortest image whenever |d| is below half the smallest cell height.  Without a periodic axis d is returned as it is."""
    pbc = np.asarray(pbc, bool).reshape(3)
    d = np.asarray(d, np.float64)
    if not pbc.any():
        return d.copy()
    cell = pad_cell(cell, pbc)
    inv = np.linalg.inv(cell) if inv is None else np.asarray(inv, np.float64).reshape(3, 3)
    s = d @ inv
    s[..., pbc] -= np.rint(s[..., pbc])
    return s @ cell


def tangent(tp, tm, Ep, Ei, Em):
    """(tau normalised over all components, branch name, margin: the smallest |energy difference| the branch decision rests on)"""
    if Ep > Ei > Em:
        tau, branch, margin = tp.copy(), 'rising', min(Ep - Ei, Ei - Em)
    elif Ep < Ei < Em:
        tau, branch, margin = tm.copy(), 'falling', min(Ei - Ep, Em - Ei)
    else:
        dp, dm = abs(Ep - Ei), abs(Em - Ei)
        dmax, dmin = max(dp, dm), min(dp, dm)
        kind = 'maximum' if (Ei >= Ep and Ei >= Em) else 'minimum'
        if Ep > Em:
            tau, branch = tp * dmax + tm * dmin, kind + '_up'
        else:
            tau, branch = tp * dmin + tm * dmax, kind + ('_tie' if Ep == Em else '_down')
        margin = min(dp, dm, abs(Ep - Em))
    norm = np.sqrt((tau * tau).sum())
    if norm > 0:
        tau = tau / norm
    else:
        tau, branch = np.zeros_like(tau), 'zero'
    return tau, branch, margin


def neb_forces(images, forces, energies, cell, pbc, k, climb=False, fixed=None, inv=None):
    """images [M,n,3] and energies [M] with both endpoints; forces [M,n,3] (the endpoints' rows are not read) or [M-2,n,3]
    (the interior images').  -> (f_neb [M-2,n,3], imax: the interior image of highest energy counted from the first interior
    image, lowest index on ties, info: per interior image dict(branch, margin, f_tau, tp, tm))"""
    images = np.asarray(images, np.float64)
    M, n = images.shape[:2]
    E = np.asarray(energies, np.float64).reshape(M)
    F = np.array(forces, np.float64)
    if F.shape[0] == M:
        F = F[1:-1]
    F = F.reshape(M - 2, n, 3).copy()
    fix = np.zeros(n, bool)
    if fixed is not None:   # a bool mask [n] or a list of atom indices
        fixed = np.asarray(fixed)
        fix[fixed.astype(np.int64) if fixed.dtype != bool else fixed] = True
    F[:, fix] = 0.0
    imax = int(np.argmax(E[1:-1]))   # (argmax: the first of equal maxima)
    out, info = np.zeros_like(F), []
    for i in range(1, M - 1):
        tp = mic(images[i + 1] - images[i], cell, pbc, inv)
        tm = mic(images[i] - images[i - 1], cell, pbc, inv)
        tau, branch, margin = tangent(tp, tm, E[i + 1], E[i], E[i - 1])
        f_tau = float((F[i - 1] * tau).sum())
        ntp, ntm = np.sqrt((tp * tp).sum()), np.sqrt((tm * tm).sum())
        if climb and i - 1 == imax:
            f = F[i - 1] - 2.0 * f_tau * tau
        else:
            f = F[i - 1] - f_tau * tau + k * (ntp - ntm) * tau
        f[fix] = 0.0
        out[i - 1] = f
        info.append(dict(branch=branch, margin=float(margin), f_tau=f_tau, tp=float(ntp), tm=float(ntm)))
    return out, imax, info


def interior_gap(energies):
    """how far the highest interior energy is above the second highest (the margin of the climbing image's choice); inf for
    a band of one interior image"""
    e = np.sort(np.asarray(energies, np.float64)[1:-1])
    return float(e[-1] - e[-2]) if len(e) > 1 else float('inf')


def neb_relax(images, energy_forces, cell, pbc, fmax, steps, k=0.1, climb=False, fixed=None, **fire):
    """relax the interior images of one band as ONE FIRE system (what ASE's FIRE(NEB(images)) does): energy_forces(pos [n,3])
    -> (energy, forces [n,3]).  -> dict(images [M,n,3], energies [M] and forces [M,n,3] of the LAST evaluation (at the images
    before the last move; the endpoints' forces are zero), n_steps, converged, imax, log (per evaluation: the FIRE step's `what`
    plus the tangent info of every image and `gap`), dts (dt per move))"""
    images = np.array(images, np.float64)
    M, n = images.shape[:2]
    e_end = [energy_forces(images[0])[0], energy_forces(images[-1])[0]]
    s = relax_ref.fire_init(images[1:-1].reshape(-1, 3), **fire)
    log, dts = [], []
    E, F, imax = np.array([e_end[0]] + [np.nan] * (M - 2) + [e_end[1]]), np.zeros_like(images), -1
    for _ in range(steps):
        cur = images.copy()
        cur[1:-1] = s['pos'].reshape(M - 2, n, 3)
        for i in range(1, M - 1):
            E[i], F[i] = energy_forces(cur[i])
        f_neb, imax, info = neb_forces(cur, F, E, cell, pbc, k, climb, fixed)
        s, what = relax_ref.fire_step(s, f_neb.reshape(-1, 3), fmax, **fire)
        log.append(dict(what, images=info, gap=interior_gap(E)))
        if s['active'] != 1:
            break
        dts.append(s['dt'])
    final = images.copy()
    final[1:-1] = s['pos'].reshape(M - 2, n, 3)
    return dict(images=final, energies=E.copy(), forces=F.copy(), n_steps=s['n_steps'], converged=s['active'] != 1, imax=imax,
                log=log, dts=dts)


# ---- the analytic two-well potential of the tests ----------------------------------------------------------------------------
SADDLE_A = 0.6


def saddle_potential(pos):
    """per-atom V = (x^2 - 1)^2 + 2 (y - a (1 - x^2))^2 + 2 z^2, a = 0.6: minima at (+-1, 0, 0) with V = 0, a saddle at (0, a, 0)
    with V = 1 whose smallest |curvature| is 4.  pos [n,3] -> (energy summed over the atoms, forces [n,3])"""
    pos = np.asarray(pos, np.float64)
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    u = y - SADDLE_A * (1.0 - x * x)
    e = ((x * x - 1.0) ** 2 + 2.0 * u * u + 2.0 * z * z).sum()
    g = np.stack([4.0 * x * (x * x - 1.0) + 4.0 * u * (2.0 * SADDLE_A * x), 4.0 * u, 4.0 * z], axis=1)
    return float(e), -g


def saddle_band(n, m, seed=0, sigma=0.02):
    """[m + 2, n, 3]: n atoms in the left well, atom 0 hops to the right one; m interior images on the straight line plus
    N(0, sigma) noise on every coordinate of the interior images"""
    a = np.tile([-1.0, 0.0, 0.0], (n, 1))
    b = a.copy()
    b[0, 0] = 1.0
    t = np.linspace(0.0, 1.0, m + 2)[:, None, None]
    band = a[None] + t * (b - a)[None]
    band[1:-1] += np.random.default_rng(seed).normal(0.0, sigma, (m, n, 3))
    return band
