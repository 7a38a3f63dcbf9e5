"""The rule of sevennet_amd.phonon in fp64 numpy, written out independently of the kernels (include/snet_hip.h, "batched supercell
phonons"): the supercell, the rows of the force constants, the acoustic sum rule, the nearest images, R(q) and D(q), and the
harmonic thermodynamics.  Sums run in the order the header states.  The images are found here by brute force over the translations
{-3..3}^3, without wrapping the pair first: an independent route to the sets the device finds among 27 candidates around the wrapped
pair (`images_27` restates that route too, for the CPU tests of the rule itself)."""
import itertools
import math

import numpy as np

import vib_ref

KB = 8.617333262e-5      # eV / K (sevennet_amd.md.KB)
SPAN = 3


# ------------------------------------------------------------------------------------------------ supercell, rows, sum rule
def supercell(pos, cell, repeats):
    """-> (positions [N,3], S [3,3]): atom c m + beta is atom beta shifted by (c1,c2,c3) cell, c = (c1 n2 + c2) n3 + c3"""
    pos, cell = np.asarray(pos, np.float64), np.asarray(cell, np.float64)
    n1, n2, n3 = (int(x) for x in repeats)
    out = []
    for c1 in range(n1):
        for c2 in range(n2):
            for c3 in range(n3):
                out.append(pos + np.array([c1, c2, c3], np.float64) @ cell)
    return np.concatenate(out), np.array([n1, n2, n3], np.float64)[:, None] * cell


def force_constants(force_fn, pos_sc, m, delta, nfree, with_scale=False):
    """Phi [3m,3N]: row 3 alpha + i from the forces on all atoms with coordinate i of home atom alpha displaced (the stencil of
    vib_ref.row).  with_scale: also sum_w |weight_w F_w| / delta per element."""
    N = len(pos_sc)
    Phi, scale = np.zeros((3 * m, 3 * N)), np.zeros((3 * m, 3 * N))
    for a in range(m):
        for i in range(3):
            F = [np.asarray(force_fn(vib_ref.displaced(pos_sc, a, i, q, delta)), np.float64).reshape(-1) for q in vib_ref.STENCIL[nfree]]
            Phi[3 * a + i] = vib_ref.row(F, nfree, delta)
            scale[3 * a + i] = sum(w * np.abs(f) for w, f in zip(vib_ref.WEIGHTS[nfree], F)) / delta
    return (Phi, scale) if with_scale else Phi


def sum_rule(Phi, m, acoustic=True):
    """-> (asr_defect, Phi after the correction): the sums over j run in ascending order"""
    Phi = np.asarray(Phi, np.float64)
    N = Phi.shape[1] // 3
    P4 = Phi.reshape(m, 3, N, 3).copy()
    total, others = np.zeros((m, 3, 3)), np.zeros((m, 3, 3))
    for j in range(N):
        total = total + P4[:, :, j, :]
        skip = np.zeros((m, 1, 1), bool)
        if j < m:
            skip[j] = True
        others = np.where(skip, others, others + P4[:, :, j, :])
    if acoustic:
        for a in range(m):
            P4[a, :, a, :] = -others[a]
    return float(np.abs(total).max()), P4.reshape(3 * m, 3 * N)


# ------------------------------------------------------------------------------------------------ images
def image_vector(d0, S, n):
    """d = d0 + n S, each component as the header writes it"""
    return np.array([d0[c] + ((float(n[0]) * S[0, c] + float(n[1]) * S[1, c]) + float(n[2]) * S[2, c]) for c in range(3)])


def _lengths(d0, S, trans):
    """|d0 + n S| for every row n of trans [T,3] (integers): the expressions of image_vector, elementwise over the rows"""
    n = np.asarray(trans, np.float64)
    d = [d0[c] + ((n[:, 0] * S[0, c] + n[:, 1] * S[1, c]) + n[:, 2] * S[2, c]) for c in range(3)]
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def images_brute(pos_sc, S, m, symprec=1e-5, span=SPAN):
    """{(alpha, j): [n, ...]}: the translations n (ascending) in {-span..span}^3 whose d = r_j - r_alpha + n S is within symprec of
    the shortest; and the smallest distance of any candidate's length from a threshold min + symprec (how safely the sets are decided)"""
    S = np.asarray(S, np.float64)
    trans = np.array(list(itertools.product(range(-span, span + 1), repeat=3)), np.int64)   # ascending (n1, n2, n3)
    out, margin = {}, np.inf
    for a in range(m):
        for j in range(len(pos_sc)):
            d0 = pos_sc[j] - pos_sc[a]
            length = _lengths(d0, S, trans)
            limit = length.min() + symprec
            margin = min(margin, float(np.abs(length - limit).min()))
            out[(a, j)] = [tuple(int(x) for x in n) for n in trans[length <= limit]]
    return out, margin


def images_27(pos_sc, S, S_inv, m, symprec=1e-5):
    """the route of snet_ph_images: wrap the pair with n0 = -rint((r_j - r_alpha) S^-1), then the 27 candidates n0 + {-1,0,1}^3
    -> (img_base int [m,N,3], img_mask int [m,N], and the kept translations as images_brute gives them)"""
    N = len(pos_sc)
    base, mask, kept = np.zeros((m, N, 3), np.int64), np.zeros((m, N), np.int64), {}
    for a in range(m):
        for j in range(N):
            d0 = pos_sc[j] - pos_sc[a]
            f = [(d0[0] * S_inv[0, c] + d0[1] * S_inv[1, c]) + d0[2] * S_inv[2, c] for c in range(3)]
            n0 = [-int(np.rint(x)) for x in f]
            cand = [(n0[0] + x, n0[1] + y, n0[2] + z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
            length = _lengths(d0, S, np.array(cand))
            keep = length <= length.min() + symprec
            base[a, j] = n0
            mask[a, j] = sum(1 << t for t in range(27) if keep[t])
            kept[(a, j)] = [cand[t] for t in range(27) if keep[t]]
    return base, mask, kept


def mask_to_translations(base, mask):
    """the translations a (img_base, img_mask) pair of arrays stands for, as images_brute gives them"""
    m, N = mask.shape
    out = {}
    for a in range(m):
        for j in range(N):
            out[(a, j)] = [(int(base[a, j, 0]) + t // 9 - 1, int(base[a, j, 1]) + (t // 3) % 3 - 1, int(base[a, j, 2]) + t % 3 - 1)
                           for t in range(27) if (int(mask[a, j]) >> t) & 1]
    return out


# ------------------------------------------------------------------------------------------------ R(q), D(q)
def dynmat(Phi, pos_sc, S, m, masses, images, q_cart):
    """R(q), D(q) (complex [3m,3m]) and max |R - R^H| at one q_cart (rad/A); also, per element of R, sum_c |Phi| w_alpha w_beta and
    the largest |q . d| met (what a rounding bound scales with)"""
    N = len(pos_sc)
    P4 = np.asarray(Phi, np.float64).reshape(m, 3, N, 3)
    w = 1.0 / np.sqrt(np.asarray(masses, np.float64))
    R_re, R_im, scale = np.zeros((3 * m, 3 * m)), np.zeros((3 * m, 3 * m)), np.zeros((3 * m, 3 * m))
    arg_max = 0.0
    for a in range(m):
        for beta in range(m):
            acc_re, acc_im, acc_abs = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
            for c in range(N // m):
                j = c * m + beta
                d0 = pos_sc[j] - pos_sc[a]
                s_re = s_im = 0.0
                for n in images[(a, j)]:
                    d = image_vector(d0, S, n)
                    arg = (q_cart[0] * d[0] + q_cart[1] * d[1]) + q_cart[2] * d[2]
                    arg_max = max(arg_max, abs(arg))
                    s_re, s_im = s_re + math.cos(arg), s_im + math.sin(arg)
                k = float(len(images[(a, j)]))
                acc_re = acc_re + P4[a, :, j, :] * (s_re / k)
                acc_im = acc_im + P4[a, :, j, :] * (s_im / k)
                acc_abs = acc_abs + np.abs(P4[a, :, j, :])
            ww = w[a] * w[beta]
            R_re[3 * a:3 * a + 3, 3 * beta:3 * beta + 3] = ww * acc_re
            R_im[3 * a:3 * a + 3, 3 * beta:3 * beta + 3] = ww * acc_im
            scale[3 * a:3 * a + 3, 3 * beta:3 * beta + 3] = ww * acc_abs
    R = R_re + 1j * R_im
    D = (R_re + R_re.T) * 0.5 + 1j * ((R_im - R_im.T) * 0.5)
    herm = float(np.hypot(R_re - R_re.T, R_im + R_im.T).max())
    return R, D, herm, scale, arg_max


def q_cartesian(q_frac, cell):
    """q_cart = 2 pi q C^-T (rad/A) of fractional q-points of the primitive reciprocal lattice"""
    return 2.0 * np.pi * (np.asarray(q_frac, np.float64) @ np.linalg.inv(np.asarray(cell, np.float64)).T)


def energies_of(lam):
    return vib_ref.HBAR * np.sqrt(vib_ref.ACC * np.abs(lam)) * np.sign(lam)


def phonons(force_fn, pos, cell, masses, repeats, q_frac, delta=0.01, nfree=2, acoustic=True, symprec=1e-5):
    """the whole analysis of one crystal: Phi (after the sum rule), asr_defect, D [n_q,3m,3m] and the eigenvalues"""
    m = len(pos)
    pos_sc, S = supercell(pos, cell, repeats)
    raw, scale = force_constants(force_fn, pos_sc, m, delta, nfree, with_scale=True)
    asr, Phi = sum_rule(raw, m, acoustic)
    images, _ = images_brute(pos_sc, S, m, symprec)
    D = np.stack([dynmat(Phi, pos_sc, S, m, masses, images, q)[1] for q in q_cartesian(q_frac, cell)])
    return dict(Phi=Phi, raw=raw, scale=scale, asr_defect=asr, D=D, eigenvalues=np.linalg.eigvalsh(D), pos_sc=pos_sc, S=S)


# ------------------------------------------------------------------------------------------------ thermodynamics
def thermodynamics(energies, temperatures, e_min=1e-5):
    """per primitive cell over an equal-weight mesh [n_mesh, 3m], the formulas as the header of sevennet_amd.phonon.thermodynamics
    states them, evaluated naively in fp64 (valid while e^x does not overflow)"""
    e = np.asarray(energies, np.float64)
    n_mesh = e.shape[0]
    hv = e[e > e_min]
    out = dict(zpe=0.5 * hv.sum() / n_mesh, n_imaginary=int((e < -e_min).sum()), n_skipped=int((np.abs(e) <= e_min).sum()),
               free_energy=[], entropy=[], heat_capacity=[])
    for T in np.atleast_1d(temperatures):
        if T == 0:
            F, S, C = out['zpe'], 0.0, 0.0
        else:
            x = hv / (KB * T)
            F = (hv / 2 + KB * T * np.log(1 - np.exp(-x))).sum() / n_mesh
            S = KB * (x / (np.exp(x) - 1) - np.log(1 - np.exp(-x))).sum() / n_mesh
            C = KB * (x ** 2 * np.exp(x) / (np.exp(x) - 1) ** 2).sum() / n_mesh
        out['free_energy'].append(F), out['entropy'].append(S), out['heat_capacity'].append(C)
    return {k: np.asarray(v) if isinstance(v, list) else v for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the diatomic chain
CHAIN = dict(a=1.7, L=7.3, m1=1.0, m2=3.0, k1=2.3, k2a=0.41, k2b=0.77)


def chain_cell():
    """the primitive cell of the chain along x: atom 0 (mass m1) at 0, atom 1 (mass m2) at a / 2; L keeps the other axes apart
    -> (positions [2,3], cell [3,3], masses [2])"""
    p = CHAIN
    return np.array([[0.0, 0.0, 0.0], [0.5 * p['a'], 0.0, 0.0]]), np.diag([p['a'], p['L'], p['L']]), np.array([p['m1'], p['m2']])


def chain_hessian(n):
    """K [6n,6n] of the supercell (n,1,1): nearest-neighbour springs k1, second-neighbour springs k2a between the atoms 0 and k2b
    between the atoms 1, along x, with the supercell's periodicity (at n = 2 both second neighbours of an atom are the same atom)"""
    p = CHAIN
    K = np.zeros((6 * n, 6 * n))

    def spring(i, j, k):
        if i != j:
            K[3 * i, 3 * i] += k
            K[3 * j, 3 * j] += k
            K[3 * i, 3 * j] -= k
            K[3 * j, 3 * i] -= k

    for c in range(n):
        nxt = (c + 1) % n
        spring(2 * c, 2 * c + 1, p['k1'])
        spring(2 * c + 1, 2 * nxt, p['k1'])
        spring(2 * c, 2 * nxt, p['k2a'])
        spring(2 * c + 1, 2 * nxt + 1, p['k2b'])
    return K


def chain_closed_form(q):
    """the two non-zero eigenvalues (ascending) of D at the fractional q along the chain"""
    p = CHAIN
    qa = 2.0 * np.pi * q
    A = (2 * p['k1'] + 2 * p['k2a'] * (1 - np.cos(qa))) / p['m1']
    B = (2 * p['k1'] + 2 * p['k2b'] * (1 - np.cos(qa))) / p['m2']
    C = -2 * p['k1'] * np.cos(qa / 2) / np.sqrt(p['m1'] * p['m2'])
    return np.linalg.eigvalsh(np.array([[A, C], [C, B]]))
