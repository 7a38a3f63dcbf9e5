"""TEST HELPER (numpy only, nothing from sevennet_amd): the all-element D3 cases of test_d3_elements_cpu.py and
test_d3_elements_gpu.py.

  all_element_cell    94 atoms, one of each Z = 1 .. 94, in a triclinic cell: DILUTE (every pair's Gaussian C6 average is
                      well defined) and DENSE (most pairs take the nearest-reference fallback of d3_c6, reference :833-837)
  c6_den              the denominator of the C6 average per ordered atom pair, from the blob's c6ab rows: which branch a pair takes
  dimer_closed_form   the D3 energy and coordination numbers of an isolated two-atom molecule, written out
  coordination_numbers  CN of a cell in numpy, for the preconditions
  pairs_inside        the (i, j, image) triples within a cutoff: what a finite difference must not change
  oracle_result       oracle.d3.d3 on a named case, computed once per process

Units as csrc/snet_d3.hip: bohr / hartree inside, A / eV outside."""
import functools
import os

import numpy as np

AU_TO_ANG = 0.52917726
AU_TO_EV = 27.21138505
BLOB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sevennet_amd', 'data', 'd3_params.npz')

CELL = np.array([[13.5, 0.6, 0.0], [0.4, 13.0, 0.7], [0.3, 0.5, 11.2]])
GRID = (5, 5, 4)
JITTER = 0.06
VDW_CUT, CN_CUT = 1600.0, 900.0          # bohr^2
SCALE = dict(DILUTE=1.6, DENSE=1.0)
# DENSE: of seeds 1 .. 60, 22 and 32 meet both conditions of test_d3_elements_cpu.py that depend on the draw (no pair's den near
# 1e-99; every element's last reference carries weight in some case); 22 keeps den further from the threshold
SEED = dict(DILUTE=11, DENSE=22)
TTT, TTF, FFF = (True, True, True), (True, True, False), (False, False, False)

# the cases of test_d3_elements_gpu.py part (a): (cell, pbc, damping, functional)
CASES = [('DILUTE', TTT, 'damp_bj', 'pbe'), ('DILUTE', TTT, 'damp_zero', 'pbe'), ('DENSE', TTT, 'damp_bj', 'pbe'),
         ('DENSE', TTT, 'damp_zero', 'pbe'), ('DENSE', TTF, 'damp_bj', 'pbe'), ('DENSE', FFF, 'damp_zero', 'b2-plyp'),
         ('DENSE', TTT, 'damp_bj', 'b3-lyp')]

ONE_REF = (2, 10, 18, 36, 54, 58, 86)     # He Ne Ar Kr Xe Ce Rn: one reference coordination number
FIVE_REF = (5, 6, 14, 32, 50, 82)         # B C Si Ge Sn Pb: five (both checked against the blob in test_d3_elements_cpu.py)


def all_element_cell(scale, seed):
    """-> Z [94] (a shuffle of 1 .. 94), positions [94,3] (A), cell [3,3] (A): the first 94 sites of a 5 x 5 x 4 grid with a
    fractional jitter of +-0.06, in CELL * scale"""
    rng = np.random.default_rng(seed)
    Z = rng.permutation(np.arange(1, 95))
    sites = np.stack(np.meshgrid(*[np.arange(g) for g in GRID], indexing='ij'), -1).reshape(-1, 3)[:94]
    frac = (sites + 0.5) / np.array(GRID) + rng.uniform(-JITTER, JITTER, (94, 3))
    cell = CELL * scale
    return Z, frac @ cell, cell


@functools.lru_cache(maxsize=None)
def named_cell(name):
    return all_element_cell(SCALE[name], SEED[name])


@functools.lru_cache(maxsize=None)
def tables():
    """the blob, with the c6ab rows spread into c6 / cn_a / cn_b [95,95,5,5] (c6 = 0: no such reference pair) and mxc [95].
    Row: C6, Z_i + 100 ref_i, Z_j + 100 ref_j, CN_i, CN_j; Z <= 94, so Z = code mod 100 and ref = code div 100."""
    z = np.load(BLOB)
    t = z['c6ab']
    ci, cj = t[:, 1].astype(np.int64), t[:, 2].astype(np.int64)
    zi, ri, zj, rj = ci % 100, ci // 100, cj % 100, cj // 100
    c6, cna, cnb = (np.zeros((95, 95, 5, 5)) for _ in range(3))
    c6[zi, zj, ri, rj], cna[zi, zj, ri, rj], cnb[zi, zj, ri, rj] = t[:, 0], t[:, 3], t[:, 4]
    c6[zj, zi, rj, ri], cna[zj, zi, rj, ri], cnb[zj, zi, rj, ri] = t[:, 0], t[:, 4], t[:, 3]
    mxc = np.zeros(95, np.int64)
    np.maximum.at(mxc, zi, ri + 1)
    np.maximum.at(mxc, zj, rj + 1)
    func = {d: dict(zip(z[d + '_names'].tolist(), z[d + '_params'])) for d in ('damp_zero', 'damp_bj')}
    return dict(c6=c6, cna=cna, cnb=cnb, mxc=mxc, r0ab=z['r0ab'], r2r4=z['r2r4'], rcov=z['rcov'], func=func)


def _weights(zi, zj, cni, cnj):
    """Gaussian weights [..., 5, 5] of the pairs' reference grids (0 outside the mxc_i x mxc_j box and where c6 = 0) and the
    reference C6 values"""
    T = tables()
    c6 = T['c6'][zi, zj]
    a = np.arange(5)
    box = (a[:, None] < T['mxc'][zi][..., None, None]) & (a[None, :] < T['mxc'][zj][..., None, None])
    rr = (T['cna'][zi, zj] - np.asarray(cni)[..., None, None]) ** 2 + (T['cnb'][zi, zj] - np.asarray(cnj)[..., None, None]) ** 2
    return np.where(box & (c6 > 0), np.exp(-4.0 * rr), 0.0), c6


def c6_den(Z, cn):
    """[n,n]: den = sum exp(-4 ((CN_i - a)^2 + (CN_j - b)^2)) over the reference grid of the ordered pair (i, j); the pair takes
    the fallback of d3_c6 where den <= 1e-99"""
    Z, cn = np.asarray(Z, np.int64), np.asarray(cn, np.float64)
    w, _ = _weights(Z[:, None], Z[None, :], cn[:, None], cn[None, :])
    return w.sum((-1, -2))


def dimer_closed_form(zi, zj, r, damping, functional):
    """isolated two-atom molecules zi-zj at distance r (A), vectorised -> energy (eV), CN_i, CN_j"""
    T = tables()
    zi, zj = np.asarray(zi, np.int64), np.asarray(zj, np.int64)
    r = np.asarray(r, np.float64) / AU_TO_ANG
    s6, rs6, s18, rs18, alp = T['func'][damping][functional]
    cn = 1.0 / (1.0 + np.exp(-16.0 * ((T['rcov'][zi - 1] + T['rcov'][zj - 1]) / r - 1.0)))
    w, c6ref = _weights(zi, zj, cn, cn)
    den = w.sum((-1, -2))
    assert (den > 1e-99).all()    # CN < 1: no dimer is anywhere near the fallback
    c6 = (w * c6ref).sum((-1, -2)) / den
    r42 = T['r2r4'][zi - 1] * T['r2r4'][zj - 1]
    if damping == 'damp_bj':
        R0 = rs6 * np.sqrt(3.0 * r42) + rs18
        phi = s6 / (r ** 6 + R0 ** 6) + 3.0 * s18 * r42 / (r ** 8 + R0 ** 8)
    else:
        r0 = T['r0ab'][zi - 1, zj - 1] / AU_TO_ANG
        f6 = 1.0 / (1.0 + 6.0 * (rs6 * r0 / r) ** alp)
        f8 = 1.0 / (1.0 + 6.0 * (rs18 * r0 / r) ** (alp + 2.0))
        phi = s6 * f6 / r ** 6 + 3.0 * s18 * r42 * f8 / r ** 8
    return -c6 * phi * AU_TO_EV, cn, cn


def dimer_force(zi, zj, r, damping, functional, h):
    """-dE/dr (eV/A) of the closed form by a central difference of step h (A)"""
    return -(dimer_closed_form(zi, zj, r + h, damping, functional)[0] - dimer_closed_form(zi, zj, r - h, damping, functional)[0]) / (2 * h)


def dimer_sample():
    """40 element pairs with a distance each (2.0 .. 4.5 A): every one-reference and every five-reference element, the lightest
    and the heaviest, like and unlike"""
    rng = np.random.default_rng(5)
    pairs = [(2, 2), (10, 86), (58, 6), (94, 94), (1, 1), (1, 94), (6, 6), (79, 8)]
    pairs += [(z, int(rng.integers(1, 95))) for z in ONE_REF + FIVE_REF]
    pairs += [(int(rng.integers(1, 95)), z) for z in ONE_REF + FIVE_REF]
    pairs += [(z, z) for z in (18, 36, 54, 82)] + [(int(a), int(b)) for a, b in rng.integers(1, 95, (2, 2))]
    zi, zj = np.array(pairs).T
    return zi, zj, rng.uniform(2.0, 4.5, len(pairs))


def all_pairs():
    """all 4 465 unordered element pairs zi <= zj with a distance (2.0 .. 4.5 A) and a unit direction each"""
    zi, zj = np.triu_indices(94)
    rng = np.random.default_rng(9)
    u = rng.normal(size=(len(zi), 3))
    return zi + 1, zj + 1, rng.uniform(2.0, 4.5, len(zi)), u / np.linalg.norm(u, axis=1, keepdims=True)


def pairs_inside(positions, cell, pbc, r2_cut):
    """the set of (i, j, n1, n2, n3) with |x_j - x_i + n.cell|^2 <= r2_cut (bohr^2), self pairs excluded.  Positions are taken as
    they are (the cells above keep every atom inside); the images reach one repetition further than the oracle's"""
    from oracle.d3 import translations
    a = np.asarray(cell, np.float64) / AU_TO_ANG
    x = np.asarray(positions, np.float64) / AU_TO_ANG
    _, g = translations(a, pbc, r2_cut)
    reach = np.abs(g).max(0) + np.asarray(pbc, np.int64)
    g = np.stack(np.meshgrid(*[np.arange(-m, m + 1) for m in reach], indexing='ij'), -1).reshape(-1, 3)
    out = set()
    for n in g:
        d = x[None, :, :] - x[:, None, :] + n @ a
        i, j = np.nonzero((d * d).sum(-1) <= r2_cut)
        keep = (i != j) | n.any()
        out.update((int(p), int(q), int(n[0]), int(n[1]), int(n[2])) for p, q in zip(i[keep], j[keep]))
    return out


def coordination_numbers(Z, positions, cell, pbc):
    """CN [n] within CN_CUT, in numpy (the oracle's cn costs a whole evaluation; test_d3_elements_cpu.py compares the two)"""
    from oracle.d3 import translations
    a = np.asarray(cell, np.float64) / AU_TO_ANG
    x = np.asarray(positions, np.float64) / AU_TO_ANG
    rc = tables()['rcov'][np.asarray(Z) - 1]
    tau, g = translations(a, pbc, CN_CUT)
    cn = np.zeros(len(x))
    for t, n in zip(tau, g):
        d = x[None, :, :] - x[:, None, :] + t
        r2 = (d * d).sum(-1)
        ok = r2 <= CN_CUT
        if not n.any():
            ok &= ~np.eye(len(x), dtype=bool)
        r = np.sqrt(np.where(ok, r2, 1.0))
        cn += np.where(ok, 1.0 / (1.0 + np.exp(-16.0 * ((rc[:, None] + rc[None, :]) / r - 1.0))), 0.0).sum(1)
    return cn


@functools.lru_cache(maxsize=None)
def oracle_result(name, pbc, damping='damp_bj', functional='pbe'):
    """oracle.d3.d3 on the named cell at VDW_CUT / CN_CUT, once per process"""
    from oracle.d3 import d3
    Z, pos, cell = named_cell(name)
    return d3(Z, pos, cell, list(pbc), damping=damping, functional=functional, vdw_cutoff=VDW_CUT, cn_cutoff=CN_CUT)


# ---- finite differences.  Steps and defects are established by test_d3_elements_cpu.py against the oracle (it prints and bounds
# them); test_d3_elements_gpu.py takes its bars from them.
# DILUTE, collective displacement FD_STEP * fd_direction() (A): no (i, j, image) enters or leaves either cutoff between -h and +h,
# so the central difference of the oracle's energy against -sum F.d is left with its truncation error: 1.23e-9 (Becke-Johnson) and
# 1.79e-9 (zero damping) relative measured; 9.7e-9 and 1.5e-8 at three times the step.
FD_SEED, FD_STEP, FD_DEFECT = 3, 1e-5, 2e-9
# dimers: |central difference of the closed form in r - the oracle's force| / (|F| + |E| / r) over dimer_sample(): 6.7e-10 (BJ) and
# 5.1e-10 (zero damping) measured, falling as h^2 (a hundred times as much at h = 1e-4).  The scale is not |F| alone: the damped energy is flat
# at short range and zero damping has a turning point, so F passes through zero where the truncation error, h^2 E''' / 6, does not.
DIMER_FD_STEP, DIMER_FD_DEFECT = 1e-5, 7e-10


def fd_direction():
    return np.random.default_rng(FD_SEED).uniform(-1.0, 1.0, (94, 3))
