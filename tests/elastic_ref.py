"""The rule of sevennet_amd.elastic in fp64 numpy, written out independently of the kernels (include/snet_hip.h, "batched elastic
tensors from strained copies"): the strained copies, the stress of a copy, the central differences S = d sigma / d epsilon and
L = d F / d epsilon, the clamped tensor, the relaxed-ion correction and the polycrystal averages.  Every expression of the device
part is evaluated in the order the header states, so that the device results can be compared bit for bit where the inputs have
the same bits.  Also a smooth periodic pair potential with analytic forces and virial, and the brute-force route (relax the ions
in every strained cell) that the relaxed-ion formula is checked against."""
import numpy as np

STENCIL = {2: (-1, 1), 4: (-2, -1, 1, 2)}
# |weight| of each copy's value in a difference, in the order of STENCIL, as multiples of 1 / delta
WEIGHTS = {2: (0.5, 0.5), 4: (1.0 / 12.0, 8.0 / 12.0, 8.0 / 12.0, 1.0 / 12.0)}
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))   # ASE order: xx, yy, zz, yz, xz, xy
ENGINE_TO_VOIGT = (0, 1, 2, 4, 5, 3)                       # from the engine's xx, yy, zz, xy, yz, zx
GPA = 160.21766208


def pattern(j):
    """E_j [3,3]: e_a e_a^T for j < 3, (e_a e_b^T + e_b e_a^T) / 2 for the shears (engineering strain)"""
    a, b = VOIGT[j]
    E = np.zeros((3, 3))
    E[a, b] += 0.5
    E[b, a] += 0.5
    return E


def strained(x, j, q, delta):
    """rows x [m,3] times F = I + (q delta) E_j in the header's operation order; q = 0 is x itself"""
    out = np.array(x, np.float64, copy=True)
    if q == 0:
        return out
    x = np.asarray(x, np.float64)
    s = float(q) * delta
    a, b = VOIGT[j]
    if a == b:
        out[:, a] = x[:, a] + s * x[:, a]
    else:
        h = s * 0.5
        out[:, a] = x[:, a] + h * x[:, b]
        out[:, b] = x[:, b] + h * x[:, a]
    return out


def stress_of(virial, virial_extra, volume):
    """sigma [6] (ASE Voigt) = -((virial + virial_extra)[p] / V') from engine-order virials"""
    t = np.asarray(virial, np.float64)
    if virial_extra is not None:
        t = t + np.asarray(virial_extra, np.float64)
    return -(t / volume)[list(ENGINE_TO_VOIGT)]


def difference(f, nfree, delta):
    """the central difference of the values f[w] at the copies of STENCIL[nfree]: snet_vib_rows' stencil without its minus sign"""
    if nfree == 2:
        return (f[1] - f[0]) / (2.0 * delta)
    return (((8.0 * f[2] - f[3]) - 8.0 * f[1]) + f[0]) / (12.0 * delta)


def scale(f, nfree, delta):
    """sum_w |weight_w f_w| / delta: what a rounding bound of `difference` scales with"""
    return sum(w * np.abs(x) for w, x in zip(WEIGHTS[nfree], f)) / delta


def finish(S):
    """(C = (S + S^T) 0.5, asymmetry = max |S - S^T|)"""
    return (S + S.T) * 0.5, float(np.abs(S - S.T).max())


def stress_strain(eval_fn, pos, cell, delta, nfree):
    """S [6,6] and L [6,3n] of one structure.  eval_fn(pos [n,3], cell [3,3]) -> (forces [n,3], stress [6] in ASE Voigt order)."""
    n = len(pos)
    S, L = np.zeros((6, 6)), np.zeros((6, 3 * n))
    for j in range(6):
        res = [eval_fn(strained(pos, j, q, delta), strained(cell, j, q, delta)) for q in STENCIL[nfree]]
        S[:, j] = difference([np.asarray(r[1], np.float64) for r in res], nfree, delta)
        L[j] = difference([np.asarray(r[0], np.float64).reshape(-1) for r in res], nfree, delta)
    return S, L


def translations(n):
    T = np.zeros((3 * n, 3))
    for k in range(3):
        T[k::3, k] = 1.0 / np.sqrt(n)
    return T


def pseudo_inverse(phi):
    """Phi+ = (P Phi P + kappa T T^T)^-1 - T T^T / kappa, kappa the mean diagonal of Phi"""
    n3 = phi.shape[0]
    T = translations(n3 // 3)
    TT = T @ T.T
    P = np.eye(n3) - TT
    kappa = np.mean(np.diag(phi))
    return np.linalg.inv(P @ phi @ P + kappa * TT) - TT / kappa


def relaxed(S, L, phi, volume):
    """S_rel = S - L Phi+ L^T / V"""
    return S - L @ pseudo_inverse(phi) @ L.T / volume


def hessian(force_fn, pos, delta, nfree):
    """the symmetrised Gamma Hessian [3n,3n] by central differences of forces (the rule of vib_ref)"""
    import vib_ref
    D = vib_ref.difference_matrix(force_fn, pos, np.arange(len(pos)), delta, nfree)
    return vib_ref.finish(D, np.ones(len(pos)))[0]


def elastic(eval_fn, pos, cell, delta=0.005, nfree=2, relax_ions=False, ion_delta=0.01):
    """the whole analysis of one structure"""
    pos, cell = np.asarray(pos, np.float64), np.asarray(cell, np.float64)
    S, L = stress_strain(eval_fn, pos, cell, delta, nfree)
    C, asym = finish(S)
    out = dict(stress_strain=S, L=L, elastic_tensor=C, asymmetry=asym)
    if relax_ions:
        phi = hessian(lambda p: eval_fn(p, cell)[0], pos, ion_delta, nfree)
        S_rel = relaxed(S, L, phi, abs(np.linalg.det(cell)))
        C_rel, asym_rel = finish(S_rel)
        out.update(elastic_tensor_clamped=C, stress_strain_clamped=S, hessian=phi, stress_strain=S_rel, elastic_tensor=C_rel,
                   asymmetry=asym_rel)
    return out


def moduli(C):
    """Voigt / Reuss / Hill bulk and shear moduli, Young's modulus and Poisson's ratio from the Hill values"""
    s = np.linalg.inv(C)
    k_v = (C[:3, :3].trace() + 2.0 * (C[0, 1] + C[0, 2] + C[1, 2])) / 9.0
    g_v = (C[:3, :3].trace() - (C[0, 1] + C[0, 2] + C[1, 2]) + 3.0 * C[3:, 3:].trace()) / 15.0
    k_r = 1.0 / (s[:3, :3].trace() + 2.0 * (s[0, 1] + s[0, 2] + s[1, 2]))
    g_r = 15.0 / (4.0 * s[:3, :3].trace() - 4.0 * (s[0, 1] + s[0, 2] + s[1, 2]) + 3.0 * s[3:, 3:].trace())
    k, g = 0.5 * (k_v + k_r), 0.5 * (g_v + g_r)
    return dict(bulk=(k_v, k_r, k), shear=(g_v, g_r, g), youngs=9.0 * k * g / (3.0 * k + g), poisson=(3.0 * k - 2.0 * g) / (2.0 * (3.0 * k + g)))


# ------------------------------------------------------------------------------------------------ a smooth pair potential
class PairPotential:
    """E = (1/2) sum over ordered pairs and images of phi(r), phi(r) = D ((1 - exp(-a (r - r0)))^2 - 1) (1 - (r / rc)^2)^4 inside
    rc (four continuous derivatives at rc), under full periodicity.  eval(pos, cell) -> (energy, forces [n,3], virial [6] in
    the engine's order and sign: stress = -virial / volume)."""

    def __init__(self, D=0.4, a=1.3, r0=2.6, rc=5.0):
        self.D, self.a, self.r0, self.rc = D, a, r0, rc

    def phi(self, r):
        m = 1.0 - np.exp(-self.a * (r - self.r0))
        u = 1.0 - (r / self.rc) ** 2
        e = self.D * (m * m - 1.0)
        de = 2.0 * self.D * m * self.a * (1.0 - m)
        return e * u ** 4, de * u ** 4 + e * 4.0 * u ** 3 * (-2.0 * r / self.rc ** 2)

    def images(self, cell):
        inv = np.linalg.inv(cell)
        reach = np.ceil(self.rc * np.linalg.norm(inv, axis=0)).astype(int) + 1   # rc / height_k, plus one for atoms outside the cell
        g = np.stack(np.meshgrid(*[np.arange(-k, k + 1) for k in reach], indexing='ij'), -1).reshape(-1, 3)
        return g.astype(np.float64) @ cell

    def eval(self, pos, cell):
        pos, cell = np.asarray(pos, np.float64), np.asarray(cell, np.float64)
        frac = pos @ np.linalg.inv(cell)
        pos = (frac - np.floor(frac)) @ cell   # (wrapped: the image reach above then holds every pair)
        d = pos[None, :, None, :] + self.images(cell)[None, None, :, :] - pos[:, None, None, :]   # [i, j, image, 3]
        r = np.sqrt((d * d).sum(-1))
        keep = (r > 1e-9) & (r < self.rc)
        rs = np.where(keep, r, 1.0)
        e, de = self.phi(rs)
        e, de = np.where(keep, e, 0.0), np.where(keep, de, 0.0)
        g = (de / rs)[..., None] * d
        forces = g.sum((1, 2))
        w = -0.5 * np.einsum('ijma,ijmb->ab', g, d)
        return 0.5 * e.sum(), forces, np.array([w[0, 0], w[1, 1], w[2, 2], w[0, 1], w[1, 2], w[2, 0]])

    def eval_fn(self):
        """the (forces, ASE-Voigt stress) interface of `stress_strain`"""
        def fn(pos, cell):
            _, f, w = self.eval(pos, cell)
            return f, stress_of(w, None, abs(np.linalg.det(cell)))
        return fn


def relax_ions(pot, pos, cell, gtol=1e-11):
    """the ions of (pos, cell) relaxed at fixed cell with scipy's BFGS on the analytic forces -> (positions, largest |F| component)"""
    from scipy.optimize import minimize
    n = len(pos)

    def fun(x):
        e, f, _ = pot.eval(x.reshape(n, 3), cell)
        return e, -f.reshape(-1)
    x = np.asarray(pos, np.float64).reshape(-1)
    for _ in range(3):   # (restarts: BFGS stops on its own precision loss before gtol now and then)
        x = minimize(fun, x, jac=True, method='BFGS', options=dict(gtol=gtol, maxiter=2000)).x
    return x.reshape(n, 3), float(np.abs(pot.eval(x.reshape(n, 3), cell)[1]).max())


def brute_force_relaxed(pot, pos, cell, delta, nfree=2):
    """S_rel by relaxing the ions in every strained cell (started from the strained positions) and differencing the stresses
    -> (S_rel [6,6], the largest residual force component over the copies)"""
    fn = pot.eval_fn()
    S, worst = np.zeros((6, 6)), 0.0
    for j in range(6):
        sig = []
        for q in STENCIL[nfree]:
            c = strained(cell, j, q, delta)
            p, fmax = relax_ions(pot, strained(pos, j, q, delta), c)
            worst = max(worst, fmax)
            sig.append(fn(p, c)[1])
        S[:, j] = difference(sig, nfree, delta)
    return S, worst
