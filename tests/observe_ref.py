"""fp64 numpy restatement of the MD observables (include/snet_hip.h: snet_obs_rdf, snet_obs_correlate), written without the
kernels' loop structure: the RDF wraps every atom into the cell by `floor` and goes by brute force over all images one cell
further than the kernel's reach; the correlations loop over (origin, lag) with whole trajectories in memory, no ring."""
import itertools

import numpy as np


def padded_cell(cell, pbc):
    """the cell with the zero rows of open axes replaced by unit vectors (the axis is not reduced: its length does not matter)"""
    cell, pbc = np.array(cell, np.float64).reshape(3, 3), np.asarray(pbc, bool).reshape(3)
    for k in range(3):
        if not pbc[k] and np.linalg.norm(cell[k]) < 1e-12:
            cell[k] = 0.0
            cell[k, k] = 1.0
    return cell


def heights(cell):
    """face-to-face heights of a cell: |det| / |a_j x a_k|"""
    vol = abs(np.linalg.det(cell))
    return np.array([vol / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3])) for k in range(3)])


def rdf_counts(pos, kind, n_kinds, cell, pbc, r_max, bins):
    """-> (counts int64 [S,S,bins], margin): counts[ka,kb,bin] = ordered triples (i of kind ka, j of kind kb, shift n), (i != j or
    n != 0), with int(|x_j - x_i + n cell| / dr) == bin < bins; margin = the smallest distance of any pair with r < r_max + dr to a
    bin edge k dr, k = 0 .. bins (inf where there is no such pair)"""
    pos, kind, pbc = np.asarray(pos, np.float64), np.asarray(kind), np.asarray(pbc, bool).reshape(3)
    n, dr = len(pos), r_max / bins
    counts = np.zeros((n_kinds, n_kinds, bins), np.int64)
    margin = np.inf
    reach = [0, 0, 0]
    if pbc.any():
        cell = padded_cell(cell, pbc)
        frac = pos @ np.linalg.inv(cell)
        frac[:, pbc] -= np.floor(frac[:, pbc])
        pos = frac @ cell
        h = heights(cell)
        reach = [int(np.floor(r_max / h[k] + 0.5)) + 1 if pbc[k] else 0 for k in range(3)]
    else:
        cell = np.zeros((3, 3))
    d = pos[None, :, :] - pos[:, None, :]   # d[i, j] = x_j - x_i
    pair_kind = (kind[:, None] * n_kinds + kind[None, :]).ravel()
    for shift in itertools.product(*(range(-m, m + 1) for m in reach)):
        r = np.linalg.norm(d + np.asarray(shift, np.float64) @ cell, axis=2)
        keep = np.ones((n, n), bool)
        if not any(shift):
            keep[np.arange(n), np.arange(n)] = False
        r, pk = r.ravel()[keep.ravel()], pair_kind[keep.ravel()]
        near = r < r_max + dr
        if near.any():
            q = r[near] / dr
            k = np.minimum(np.rint(q), bins)
            margin = min(margin, float(np.abs(r[near] - k * dr).min()))
        b = (r / dr).astype(np.int64)
        ok = (r / dr) < bins
        np.add.at(counts.reshape(-1), pk[ok] * bins + b[ok], 1)
    return counts, margin


def mass_centre(x, mass):
    """[T,3]: sum m x / sum m of every frame of x [T,n,3]"""
    return (mass[None, :, None] * x).sum(1) / mass.sum()


def correlate(pos, vel, mass, kind, n_kinds, lags, origin_every, remove_com=True, anchored=False):
    """pos, vel [T,n,3]: -> (msd_sum [S,lags], vacf_sum [S,lags], n_origins int64 [lags]), the sums over origins so = 0, origin_every,
    .. and lags l < lags with so + l < T of sum_i |d_i|^2 and sum_i v_i(so + l) . v_i(so) per kind.  remove_com: both relative to
    the frame's mass-weighted centre; not for an anchored system (one with held components), and one free atom gives 0."""
    pos, vel, mass, kind = (np.asarray(a) for a in (pos, vel, mass, kind))
    T, n = pos.shape[:2]
    msd, vacf, n_or = np.zeros((n_kinds, lags)), np.zeros((n_kinds, lags)), np.zeros(lags, np.int64)
    if remove_com and not anchored:
        if n == 1:
            pos, vel = np.zeros_like(pos), np.zeros_like(vel)
        else:
            pos = pos - mass_centre(pos, mass)[:, None, :]
            vel = vel - mass_centre(vel, mass)[:, None, :]
    for so in range(0, T, origin_every):
        for l in range(lags):
            s = so + l
            if s >= T:
                break
            n_or[l] += 1
            d2 = ((pos[s] - pos[so]) ** 2).sum(1)
            vv = (vel[s] * vel[so]).sum(1)
            for k in range(n_kinds):
                msd[k, l] += d2[kind == k].sum()
                vacf[k, l] += vv[kind == k].sum()
    return msd, vacf, n_or


def local_kinds(types):
    """(species present ascending, kind of each atom within them)"""
    present = np.unique(types)
    return present, np.searchsorted(present, types)
