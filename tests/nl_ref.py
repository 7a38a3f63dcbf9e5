"""Test helper: a brute-force neighbor list and the table of adversarial cells every graph builder is pinned to.

`brute_force_list` restates only the reference's convention (sevenn/train/dataload.py:32-129, ASE 'ijDS'): every ordered
pair (i, j) and integer image S with |r_j - r_i + S.cell|^2 < rc^2, no (i == j, S == 0), open axes not imaged, a zero cell
row of an open axis padded along that axis.  Plain numpy in fp64 on the CALLER's positions: nothing is wrapped, binned or put
in a tree, and nothing is imported from sevennet_amd -- it shares no structure with the four builders it judges.

`adversarial_cases` is the case table shared by the CPU and GPU tests (tests/test_nl_ref_cpu.py,
tests/test_neighbor_adversarial_gpu.py).  Every case uses the cutoff RC so that all of them fit one heterogeneous batch; all
seeds are fixed, and the table is chosen so that the reference finds no borderline pair in any case (asserted on the CPU).
"""
import itertools
from typing import NamedTuple

import numpy as np

RC = 5.0
BORDERLINE_REL = 1e-9   # pairs with |d^2 - rc^2| <= 1e-9 rc^2: membership depends on the order of fp64 operations


def _padded(cell, pbc, rc):
    cell = np.array(cell, np.float64).reshape(3, 3)
    for k in range(3):
        if not pbc[k] and np.linalg.norm(cell[k]) < 1e-12:
            cell[k] = 0.0
            cell[k, k] = 5.0 * rc   # any length: an open axis is never imaged
    return cell


def image_range(pos, cell, pbc, rc):
    """per axis, the largest |S_k| enumerated: ceil(rc / h_k + max_ij |frac_i - frac_j|_k) on periodic axes (inside the cutoff
    sphere the fractional coordinate of r_j - r_i + S.cell along k is at most rc / h_k in magnitude), 0 on open ones"""
    inv = np.linalg.inv(cell)
    frac = pos @ inv
    reach = rc * np.linalg.norm(inv, axis=0)                # rc / h_k: column k of inv has length 1 / h_k
    spread = frac.max(0) - frac.min(0) if len(pos) else np.zeros(3)
    return [int(np.ceil(reach[k] + spread[k])) if pbc[k] else 0 for k in range(3)]


def brute_force_list(pos, cell, pbc, rc, chunk=1 << 21):
    """-> (edge_index[2,E] int64, edge_vec[E,3] fp64, shifts[E,3] int64, borderline[K,5] int64 rows (i, j, S))
    sorted by (i, j, S); edge_vec = (r_j - r_i) + S.cell.  `borderline` lists the pairs (listed or not) within 1e-9 rc^2 of
    the cutoff."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    pbc = np.asarray(pbc, bool).reshape(3)
    n = len(pos)
    if n == 0:
        return np.zeros((2, 0), np.int64), np.zeros((0, 3)), np.zeros((0, 3), np.int64), np.zeros((0, 5), np.int64)
    cell = _padded(cell, pbc, rc)
    R = image_range(pos, cell, pbc, rc)
    S_all = np.array(list(itertools.product(*[range(-r, r + 1) for r in R])), np.int64).reshape(-1, 3)
    ii, jj = [a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing='ij')]
    d0 = pos[jj] - pos[ii]                                   # [n^2, 3]
    rc2 = rc * rc
    rows, vecs, border = [], [], []
    step = max(1, chunk // (n * n))
    for s0 in range(0, len(S_all), step):
        S = S_all[s0:s0 + step]
        d = d0[None, :, :] + (S.astype(np.float64) @ cell)[:, None, :]          # [s, n^2, 3]
        d2 = (d * d).sum(-1)
        self_edge = (ii == jj)[None, :] & (S == 0).all(1)[:, None]
        si, pi = np.nonzero((d2 < rc2) & ~self_edge)
        rows.append(np.concatenate([ii[pi, None], jj[pi, None], S[si]], 1))
        vecs.append(d[si, pi])
        si, pi = np.nonzero((np.abs(d2 - rc2) <= BORDERLINE_REL * rc2) & ~self_edge)
        border.append(np.concatenate([ii[pi, None], jj[pi, None], S[si]], 1))
    rows, vecs, border = np.concatenate(rows), np.concatenate(vecs), np.concatenate(border)
    order = np.lexsort(rows.T[::-1])
    rows, vecs = rows[order], vecs[order]
    return rows[:, :2].T.copy(), vecs, rows[:, 2:].copy(), border[np.lexsort(border.T[::-1])]


# ---------------------------------------------------------------------------------------------------------- the case table
class Case(NamedTuple):
    name: str
    types: np.ndarray   # species indices in {0, 1}
    pos: np.ndarray     # [n,3] fp64, A
    cell: np.ndarray    # [3,3] rows = lattice vectors
    pbc: tuple
    must_list: tuple = ()      # ordered pairs (i, j) that must appear (with some S)
    must_not_list: tuple = ()  # ordered pairs that must not appear with any S


_DIAMOND = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0],
                     [.25, .25, .25], [.25, .75, .75], [.75, .25, .75], [.75, .75, .25]])
SHEAR = np.array([[1, 0, 0], [3, 1, 0], [-2, 4, 1]])   # unimodular: the same lattice, a strongly sheared cell
TRI = np.array([[5.4, 0.0, 0.0], [1.0, 5.2, 0.0], [0.5, 0.8, 5.6]])


def _diamond(lengths, reps, sigma, seed):
    """rattled diamond sites in the orthogonal cell diag(lengths): (Cartesian positions, cell)"""
    reps = np.asarray(reps)
    g = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing='ij'), -1).reshape(-1, 3)
    frac = (g[:, None, :] + _DIAMOND[None]).reshape(-1, 3) / reps
    cell = np.diag(np.asarray(lengths, np.float64))
    rng = np.random.default_rng(seed)
    return frac @ cell + rng.normal(0.0, sigma, frac.shape), cell


def _types(n, seed):
    return np.random.default_rng(1000 + seed).integers(0, 2, n)


def _height(cell, k):
    return 1.0 / np.linalg.norm(np.linalg.inv(cell)[:, k])


# NOT in the table (it has borderline pairs by construction): one atom at the origin of an orthogonal cell of height rc / 2.  Every
# product and sum any builder forms is exact in fp64, so the second image is at exactly rc in every order of operations and the
# strict inequality of the convention decides: images +-1 are listed, +-2 are not.
EXACT_CUTOFF_CASE = Case('exact_cutoff', np.zeros(1, np.int64), np.zeros((1, 3)), np.diag([RC / 2, 4 * RC, 4 * RC]), (True,) * 3)


def adversarial_cases():
    P3 = (True, True, True)
    out = []

    def add(name, pos, cell, pbc, seed, **kw):
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        out.append(Case(name, _types(len(pos), seed), pos, np.array(cell, np.float64).reshape(3, 3), tuple(pbc), **kw))

    a = 5.431
    # strong shear: the 32-atom crystal of diag(2a, 2a, a) described by the cell SHEAR . diag (rc / h = 13 along the first axis);
    # the atoms keep their Cartesian places and lie mostly outside the new cell
    pos, diag = _diamond((2 * a, 2 * a, a), (2, 2, 1), 0.06, 1)
    add('shear', pos, SHEAR @ diag, P3, 1)
    # the same crystal in left-handed cells (negative determinant): two rows swapped
    add('shear_left_handed', pos, (SHEAR @ diag)[[1, 0, 2]], P3, 1)
    add('cubic_left_handed', pos, diag[[0, 2, 1]], P3, 1)
    # every atom moved by its own lattice combination in [-3, 3]^3, triclinic cell; then one axis by +-1000
    rng = np.random.default_rng(2)
    cell2 = TRI * [[2], [1], [1]]
    base = (np.concatenate([_DIAMOND, _DIAMOND + [1, 0, 0]]) / [2, 1, 1]) @ cell2 + rng.normal(0, 0.08, (16, 3))
    add('lattice_jumps', base + rng.integers(-3, 4, (16, 3)) @ cell2, cell2, P3, 2)
    base8 = _DIAMOND @ TRI + rng.normal(0, 0.08, (8, 3))
    jump = np.stack([rng.choice([-1000, 1000], 8), rng.integers(-1, 2, 8), rng.integers(-1, 2, 8)], 1)
    add('lattice_jumps_1000', base8 + jump @ TRI, TRI, P3, 3)
    add('lattice_jumps_1000_last_axis', base8 + jump[:, ::-1] @ TRI, TRI, P3, 3)
    # atoms exactly on cell faces: fractional 0 and -1e-17 (f - floor(f) gives 1.0), orthogonal, triclinic and thin cells
    f = np.array([[0, 0, 0], [-1e-17, .5, .5], [.5, -1e-17, 0], [.5, .5, -1e-17], [-1e-17, -1e-17, -1e-17], [.25, 0, .75],
                  [0, .31, -1e-17], [.77, .13, .42]])
    add('on_faces_orthogonal', f @ np.diag([7.0, 6.5, 8.0]), np.diag([7.0, 6.5, 8.0]), P3, 4)
    add('on_faces_triclinic', f @ TRI, TRI, P3, 4)
    thin = np.array([[RC / 2.37, 0, 0], [0.4, 6.1, 0], [0.3, -0.5, RC / 1.43]])
    add('on_faces_thin', f @ thin, thin, P3, 4)
    # diamond 3x3x3 (216 atoms), first face distance rc (k -+ 1e-3): the cell list switches its bin count / search range there
    for k in (1, 2, 3):
        for tag, eps in (('below', -1e-3), ('above', 1e-3)):
            pos, cell = _diamond((RC * (k + eps), 2.2 * RC, 2.4 * RC), (3, 3, 3), 0.05, 10 + k)
            add(f'face_{k}rc_{tag}', pos, cell, P3, 10 + k)
    # rc / h = 63.5 and 64.5 along the first axis: both sides of the routing boundary (device lists / host list)
    for tag, reach in (('63p5', 63.5), ('64p5', 64.5)):
        cell = np.array([[1.0, 0, 0], [0.3, 12.0, 0], [0.2, 0.5, 12.5]])
        cell[0] *= (RC / reach) / _height(cell, 0)
        add(f'reach_{tag}', np.array([[0.01, 1.0, 2.0], [0.05, 4.1, 3.3], [-0.02, 9.5, 7.0]]), cell, P3, 20)
    # slab and wire in skewed cells whose OPEN rows are not zero (and not along a Cartesian axis); atoms far outside along them
    rng = np.random.default_rng(5)
    slab = np.array([[6.0, 0, 0], [2.0, 5.5, 0], [1.5, -1.0, 9.0]])
    add('slab_skewed', rng.uniform(-0.5, 1.5, (24, 3)) @ slab * [1, 1, 0.8] + [0, 0, -3.0], slab, (True, True, False), 5)
    wire = np.array([[8.0, 1.0, 0.5], [0.7, 4.2, 0.3], [0.4, -0.9, 7.0]])
    add('wire_skewed', rng.uniform(-1.0, 2.0, (20, 3)) @ wire * [0.6, 1, 0.6], wire, (False, True, False), 6)
    add('slab_zero_row', rng.uniform(0, 1, (20, 3)) @ np.diag([6.0, 7.0, 9.0]) + [30.0, -40.0, 5.0],
        [[6.0, 0, 0], [1.0, 7.0, 0], [0, 0, 0]], (True, True, False), 7)
    # one atom in a periodic cell thinner than the cutoff: self images only
    add('single_atom_thin', [[0.3, -7.2, 11.0]], [[2.0, 0, 0], [0.6, 3.1, 0], [-0.4, 0.7, 1.7]], P3, 8)
    add('molecule', [[0.0, 0.0, 0.0], [1.1, 0.0, 0.0], [-0.4, 1.0, 0.0], [0.2, -0.5, 1.0], [2.3, 0.4, -0.6], [6.9, 0.4, -0.6]],
        np.zeros((3, 3)), (False,) * 3, 9)
    add('isolated_atom', [[0.3, -0.2, 0.1]], np.zeros((3, 3)), (False,) * 3, 9)
    # constructed pairs at rc (1 - 1e-6) (atoms 2m, 2m+1 with m even: listed) and rc (1 + 1e-6) (m odd: not listed), 20 A apart,
    # in an open box, and through the faces of a periodic cell
    rng = np.random.default_rng(11)
    u = rng.normal(size=(8, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    centre = np.array([[20.0 * m, 3.0 * (m % 3), -2.0 * m] for m in range(8)])
    scale = np.array([RC * (1 - 1e-6) if m % 2 == 0 else RC * (1 + 1e-6) for m in range(8)])
    pairs = np.stack([centre, centre + u * scale[:, None]], 1).reshape(16, 3)
    yes = tuple((2 * m + s, 2 * m + 1 - s) for m in range(0, 8, 2) for s in (0, 1))
    no = tuple((2 * m + s, 2 * m + 1 - s) for m in range(1, 8, 2) for s in (0, 1))
    add('cutoff_pairs_open', pairs, np.zeros((3, 3)), (False,) * 3, 11, must_list=yes, must_not_list=no)
    L = 3.0 * RC
    box = np.array([[L, 0, 0], [0.2 * L, L, 0], [0.1 * L, -0.3 * L, L]])
    c4 = np.array([[0.05, 0.1, 0.1], [0.1, 0.02, 0.6], [0.6, 0.5, 0.03], [0.55, 0.97, 0.5]]) @ box
    ax = np.array([0, 1, 2, 1])                       # pair m reaches its partner through the face of axis ax[m]
    sign = np.array([-1.0, -1.0, -1.0, 1.0])
    partner = np.empty((4, 3))
    for m in range(4):
        n_hat = np.linalg.inv(box)[:, ax[m]]
        n_hat = n_hat / np.linalg.norm(n_hat)          # normal of that face
        partner[m] = c4[m] + sign[m] * n_hat * scale[m] - sign[m] * box[ax[m]]   # its image S = sign e_ax is at n_hat * scale
    add('cutoff_pairs_periodic', np.stack([c4, partner], 1).reshape(8, 3), box, P3, 12,
        must_list=tuple(p for p in yes if max(p) < 8), must_not_list=tuple(p for p in no if max(p) < 8))
    return out
