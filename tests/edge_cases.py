"""Test helper: the case table the edge kernels (snet_edge_embed_fwd / _bwd / _tangent, the generated harmonics, snet_edge_force /
snet_edge_force_seg) are pinned to -- edges as crystals and close contacts produce them, not random ones.

  lattice   every non-zero integer vector of {-2..2}^3 at two lattice constants: axes, face and body diagonals, every sign pattern,
            -v beside every v, whole shells of one |r|, components exactly 0 or equal in magnitude
  radial    lengths at the ends of the range along the polar axis of the harmonics and along one generic direction: close
            contacts, r_on and its fp32 neighbours, the cutoff approached by halving the distance to it down to one fp32 ulp, and
            r == r_c itself (an fp64 r < r_c of a graph builder can round to r_c in fp32; nothing lies beyond it)
  sizes     1, 255, 256, 257 edges: partial and full 256-thread blocks
  params    every lmax x normalize x cutoff kind, the ends of the n_basis range, the other poly_p, another cutoff
  force     300 atoms in 7 systems with an empty segment, an atom without edges, in-only and out-only atoms, degrees 0..70

numpy only: shared by tests/test_edge_geometry_cpu.py (the table's own properties, on any machine) and
tests/test_edge_geometry_gpu.py (the kernels)."""
import itertools
import math
from typing import NamedTuple

import numpy as np

RC, R_ON = 5.0, 4.5
LATTICE_SCALES = (0.37, 1.3575)
RADIAL_DIRECTIONS = ((0.0, 1.0, 0.0), (0.36, -0.48, 0.8))   # the polar axis of the harmonics; a generic unit vector
SIZES = (1, 255, 256, 257)


class Params(NamedTuple):
    lmax: int
    normalize: int
    kind: int          # 0 = polynomial cutoff, 1 = XPLOR
    n_basis: int = 8
    poly_p: int = 6
    rc: float = RC
    r_on: float = R_ON

    @property
    def id(self):
        return (f'l{self.lmax}-n{self.normalize}-{"xplor" if self.kind else "poly"}-nb{self.n_basis}-p{self.poly_p}'
                f'-rc{self.rc:g}')

    @property
    def nsh(self):
        return (self.lmax + 1) ** 2

    def coeffs(self):
        """n pi / r_c in fp32, as the reference's BesselBasis stores them"""
        return np.array([n * math.pi / self.rc for n in range(1, self.n_basis + 1)], np.float32)


def params_table():
    t = [Params(lmax, nz, kind) for lmax in range(4) for nz in (0, 1) for kind in (0, 1)]
    for kind in (0, 1):
        t += [Params(2, 1, kind, n_basis=1), Params(2, 1, kind, n_basis=16), Params(2, 1, kind, poly_p=5)]
    t.append(Params(2, 1, 1, rc=6.0, r_on=5.5))
    return t


def lattice_integers():
    """[124, 3] int64: {-2..2}^3 without the origin, lexicographic"""
    return np.array([v for v in itertools.product(range(-2, 3), repeat=3) if any(v)], np.int64)


def lattice_edges():
    """[248, 3] fp32: the integer vectors at both lattice constants (the product is formed in fp64 and rounded once)"""
    ints = lattice_integers().astype(np.float64)
    return np.concatenate([(ints * s).astype(np.float32) for s in LATTICE_SCALES])


def lattice_partner():
    """[248] int64: the index of -v for every lattice edge v"""
    n = len(lattice_integers())
    return np.concatenate([np.arange(n)[::-1] + k * n for k in range(len(LATTICE_SCALES))])


def radial_lengths(rc=RC, r_on=R_ON):
    """[27] fp32 lengths, none beyond rc"""
    on = np.float32(r_on)
    near = [np.float32(rc * (1.0 - 2.0 ** -k)) for k in range(4, 24)]
    return np.array([0.3, 0.4, 1.0, np.nextafter(on, np.float32(0)), on, np.nextafter(on, np.float32(2 * rc))] + near + [rc],
                    np.float32)


def radial_edges(rc=RC, r_on=R_ON):
    """[54, 3] fp32: every radial length along both directions.  Along the polar axis |v| is the listed fp32 length exactly;
    along the generic direction the three components round separately, so |v| in fp64 lies within one fp32 rounding of it."""
    r = radial_lengths(rc, r_on).astype(np.float64)
    return np.concatenate([(r[:, None] * np.array(d, np.float64)[None, :]).astype(np.float32) for d in RADIAL_DIRECTIONS])


def sized_edges(n):
    """the first n lattice edges; the table holds 248, so 255..257 run round it again"""
    lat = lattice_edges()
    return lat[np.arange(n) % len(lat)]


def length_fp32(vec):
    """|v| the way the kernels form it: fp32 products, summed left to right, fp32 square root (no contraction: an FMA changes the
    last bit at most, and both signs of v give the same bits either way)"""
    v = np.asarray(vec, np.float32)
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def edge_of_row_map(n_edges, seed=5):
    """int32 row -> edge map that permutes, repeats and omits: a shuffle of the even edges (the odd ones appear nowhere) followed
    by edge 0 five times and the last even edge twice"""
    rng = np.random.default_rng(seed)
    even = np.arange(0, n_edges, 2)
    return np.concatenate([rng.permutation(even), np.zeros(5, np.int64), np.full(2, even[-1])]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the force graph
FORCE_SEG = (0, 40, 40, 41, 100, 180, 250, 300)     # 7 systems: 40 atoms, none, one atom without edges, 59, 80, 70, 50
R_SCALE = (1.0, 1e2, 1e4)                            # |r_x| ~ 1, |r_y| ~ 1e2, |r_z| ~ 1e4
G_SCALE = (1.0, 1e6, 1e12)                           # |g_x| ~ 1, |g_y| ~ 1e6, |g_z| ~ 1e12
# -> the Voigt slots xx, yy, zz, xy, yz, zx ~ 1, 1e8, 1e16, 1e6, 1e14, 1e4: a swapped, dropped or doubled slot is off by ~100x


def force_graph(seed=11):
    """edges sorted by centre (row_ptr), the source-sorted permutation (col_ptr, eperm), as the engine's build_graph hands them to
    snet_edge_force; every edge stays inside its system.  Per system with >= 2 atoms: the first atom is nobody's centre (out-edges
    only), the second nobody's source (in-edges only); in-degrees are drawn from 0..12, and system 0 carries the degrees 69 and 70
    (more than its 40 atoms: parallel edges, as periodic images make them)."""
    rng = np.random.default_rng(seed)
    seg = np.array(FORCE_SEG, np.int64)
    n = int(seg[-1])
    deg = np.zeros(n, np.int64)
    for b in range(len(seg) - 1):
        a0, a1 = seg[b], seg[b + 1]
        if a1 - a0 >= 2:
            deg[a0 + 1:a1] = rng.integers(0, 13, a1 - a0 - 1)
            deg[a0] = 0
    deg[2], deg[3], deg[4] = 70, 69, 0
    center = np.repeat(np.arange(n), deg)
    system = np.searchsorted(seg, center, side='right') - 1
    lo, hi = seg[system], seg[system + 1]
    src = lo + rng.integers(0, 1 << 30, len(center)) % (hi - lo - 1)       # any atom of the system but its second ...
    src = np.where(src >= lo + 1, src + 1, src)
    row_ptr = np.zeros(n + 1, np.int64)
    row_ptr[1:] = np.cumsum(deg)
    col_ptr = np.zeros(n + 1, np.int64)
    col_ptr[1:] = np.cumsum(np.bincount(src, minlength=n))
    eperm = np.argsort(src, kind='stable')
    E = len(center)
    rij = (rng.standard_normal((E, 3)) * np.array(R_SCALE)).astype(np.float32)
    g = (rng.standard_normal((E, 3)) * np.array(G_SCALE)).astype(np.float32)
    return dict(n=n, E=E, seg_ptr=seg.astype(np.int32), center=center, src=src, row_ptr=row_ptr.astype(np.int32),
                col_ptr=col_ptr.astype(np.int32), eperm=eperm.astype(np.int32), rij=rij, g=g)
