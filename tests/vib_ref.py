"""The rule of sevennet_amd.vib in fp64 numpy, written out independently of the kernels (include/snet_hip.h, "batched
finite-difference Hessians"): central differences of forces as ASE's Vibrations with direction='central', the symmetrised and
mass-weighted Hessian, and the signed harmonic spectrum.  Every expression is evaluated in the order the header states, so
that the device results can be compared bit for bit where the inputs have the same bits."""
import numpy as np

HBAR = 0.6582119569      # eV fs
ACC = 9.648533212e-3     # eV / (A amu) in A / fs^2 (sevennet_amd.md.ACC)
INV_CM = 8065.543937     # cm^-1 per eV
STENCIL = {2: (-1, 1), 4: (-2, -1, 1, 2)}
# |weight| of each copy's force in a row of D, in the order of STENCIL, as multiples of 1 / delta
WEIGHTS = {2: (0.5, 0.5), 4: (1.0 / 12.0, 8.0 / 12.0, 8.0 / 12.0, 1.0 / 12.0)}


def displaced(pos, atom, axis, q, delta):
    """a copy of pos [n,3] with q delta added to one component: the product is rounded, then added; q = 0 is pos itself"""
    out = np.array(pos, np.float64, copy=True)
    if q != 0:
        out[atom, axis] = out[atom, axis] + float(q) * delta
    return out


def row(F, nfree, delta):
    """one row of D from the forces F[w] (each [3m]) on the selected atoms at the copies of STENCIL[nfree]"""
    if nfree == 2:
        return (F[0] - F[1]) / (2.0 * delta)
    return (((8.0 * F[1] - F[0]) - 8.0 * F[2]) + F[3]) / (12.0 * delta)


def difference_matrix(force_fn, pos, idx, delta, nfree, with_scale=False):
    """D [3m,3m]: row 3 k + i from the forces on the atoms idx with coordinate i of atom idx[k] displaced.  force_fn(pos [n,3])
    -> forces [n,3] fp64.  with_scale: also sum_w |weight_w F_w| / delta per element (what a rounding bound scales with)."""
    idx = np.asarray(idx, np.int64)
    m = len(idx)
    D, scale = np.zeros((3 * m, 3 * m)), np.zeros((3 * m, 3 * m))
    for k, a in enumerate(idx):
        for i in range(3):
            F = [np.asarray(force_fn(displaced(pos, a, i, q, delta)), np.float64)[idx].reshape(-1) for q in STENCIL[nfree]]
            D[3 * k + i] = row(F, nfree, delta)
            scale[3 * k + i] = sum(w * np.abs(f) for w, f in zip(WEIGHTS[nfree], F)) / delta
    return (D, scale) if with_scale else D


def finish(D, masses_selected):
    """(H, Hm, asymmetry) of a difference matrix: H = (D + D^T) 0.5, Hm[r,c] = H[r,c] (w_r w_c) with w = 1 / sqrt(mass) of the
    row's / column's atom, asymmetry = max |D - D^T|"""
    w = np.repeat(1.0 / np.sqrt(np.asarray(masses_selected, np.float64)), 3)
    H = (D + D.T) * 0.5
    return H, H * (w[:, None] * w[None, :]), float(np.abs(D - D.T).max())


def spectrum(Hm):
    """eigenvalues (ascending), modes [3m,m,3], signed energies h nu (eV), signed frequencies (cm^-1), zpe (eV)"""
    lam, vec = np.linalg.eigh(Hm)
    e = HBAR * np.sqrt(ACC * np.abs(lam)) * np.sign(lam)
    k = len(lam)
    return dict(eigenvalues=lam, modes=vec.T.reshape(k, k // 3, 3), energies=e, frequencies=e * INV_CM, zpe=float(0.5 * e[e > 0].sum()))


def vibrations(force_fn, pos, masses, idx, delta=0.01, nfree=2):
    """the whole analysis of one structure: hessian, asymmetry and the spectrum"""
    idx = np.arange(len(pos)) if idx is None else np.asarray(idx, np.int64)
    D = difference_matrix(force_fn, pos, idx, delta, nfree)
    H, Hm, asym = finish(D, np.asarray(masses, np.float64)[idx])
    return dict(D=D, hessian=H, hessian_mw=Hm, asymmetry=asym, **spectrum(Hm))


def quadratic(K, x0=None):
    """force_fn of E = (1/2) (x - x0)^T K (x - x0) over the flattened coordinates: central differences are exact on it"""
    K = np.asarray(K, np.float64)
    x0 = np.zeros(K.shape[0]) if x0 is None else np.asarray(x0, np.float64).reshape(-1)
    return lambda pos: -(K @ (np.asarray(pos, np.float64).reshape(-1) - x0)).reshape(-1, 3)


def random_spd_like(rng, n3, scale=1.0):
    """a random symmetric matrix [n3,n3] (not necessarily positive)"""
    A = rng.normal(0.0, scale, (n3, n3))
    return (A + A.T) * 0.5
