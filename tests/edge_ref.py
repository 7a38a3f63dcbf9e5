"""Test helper: what the edge kernels are measured against.

`reference64`   the oracle's own functions (oracle.model.bessel_basis x poly_cutoff / xplor_cutoff, oracle.e3.spherical_harmonics)
                in fp64 on the fp32 edge vectors the kernel reads, with d emb / d|r| and the Jacobian d sh / d v by autograd.
`restatement32` the arithmetic the kernels replace: the reference's modules (sevenn/nn/edge_embedding.py:101-103, 125-132, 150-160)
                in fp32, in their operation order -- numpy for the radial part, with the derivative summed the way reverse-mode
                differentiation of that expression sums it; the harmonics and their Jacobian by the oracle's recursion and autograd
                run in fp32 (e3nn's generated polynomials are not available here; the recursion contracts the same degree-l
                polynomials from fp32 Wigner coefficients).
`bound`         quantities without an asserted bar in this project (dsh entries, emb', emb at 16 basis functions) are judged by
                    |kernel - fp64|[e, k] <= 3 x max over the case group |restatement - fp64| + one fp32 ulp of max_k |fp64[e, :]|
                (3: the device's sinf / sincosf and reciprocal against correctly rounded library ones).

numpy / torch on the CPU only; nothing is imported from sevennet_amd."""
import functools

import numpy as np
import torch

from oracle.e3 import spherical_harmonics
from oracle.model import bessel_basis, poly_cutoff, xplor_cutoff

F32 = np.float32


def _envelope64(p, r):
    return poly_cutoff(r, p.rc, p.poly_p) if p.kind == 0 else xplor_cutoff(r, p.rc, p.r_on)


def _jacobian(sh, v):
    """[E, nsh, 3]: one backward pass per harmonic (every edge's harmonics depend on its own vector only); a constant column
    (l = 0) has no graph and a zero row"""
    rows = []
    for i in range(sh.shape[1]):
        g = torch.autograd.grad(sh[:, i].sum(), v, retain_graph=True, allow_unused=True)[0] if sh.requires_grad else None
        rows.append(torch.zeros_like(v) if g is None else g)
    return torch.stack(rows, 1).detach()


def reference64(p, vec, jacobian=True):
    """-> dict of fp64 torch tensors: r [E], emb [E, nb], demb [E, nb] = d emb / d|r|, sh [E, nsh], dsh [E, nsh, 3]"""
    v = torch.as_tensor(np.asarray(vec, np.float32)).double()
    coeffs = torch.as_tensor(p.coeffs()).double()
    r = v.norm(dim=1).requires_grad_(True)
    emb = bessel_basis(r, coeffs, p.rc) * _envelope64(p, r).unsqueeze(-1)
    demb = torch.stack([torch.autograd.grad(emb[:, k].sum(), r, retain_graph=True)[0] for k in range(p.n_basis)], 1)
    out = dict(r=r.detach(), emb=emb.detach(), demb=demb)
    vg = v.clone().requires_grad_(True)
    sh = spherical_harmonics(p.lmax, vg, bool(p.normalize))
    out['sh'] = sh.detach()
    if jacobian:
        out['dsh'] = _jacobian(sh, vg)
    return out


def g_vec_reference64(p, vec, g_emb, g_sh):
    """fp64 autograd of sum(emb * g_emb) + sum(sh * g_sh) with respect to the edge vectors (g_sh = None: the radial part alone)"""
    v = torch.as_tensor(np.asarray(vec, np.float32)).double().requires_grad_(True)
    coeffs = torch.as_tensor(p.coeffs()).double()
    r = v.norm(dim=1)
    emb = bessel_basis(r, coeffs, p.rc) * _envelope64(p, r).unsqueeze(-1)
    s = (emb * g_emb.double()).sum()
    if g_sh is not None:
        s = s + (spherical_harmonics(p.lmax, v, bool(p.normalize)) * g_sh.double()).sum()
    return torch.autograd.grad(s, v)[0]


def radial_restatement32(p, vec):
    """(emb, emb') as fp32 numpy arrays: BesselBasis x PolynomialCutoff / XPLORCutoff evaluated operation by operation in fp32,
    and the gradient with respect to |r| as reverse-mode differentiation of those operations forms it"""
    v = np.asarray(vec, F32)
    r = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])[:, None]          # torch.linalg.norm, fp32
    c = p.coeffs()[None, :]
    pref, rc = F32(2.0 / p.rc), F32(p.rc)
    arg = c * r
    num = pref * np.sin(arg)                        # self.prefactor * torch.sin(self.coeffs * ur)
    basis = num / r                                 # ... / ur
    dbasis = (pref * np.cos(arg) * c) / r - (num / r) / r      # d(num / ur): grad / ur through num, -num / ur^2 through ur
    if p.kind == 0:
        pp = F32(p.poly_p)
        c0, c1, c2 = F32((pp + 1) * (pp + 2) / 2), F32(pp * (pp + 2)), F32(pp * (pp + 1) / 2)
        x = r / rc
        env = F32(1) - c0 * np.power(x, pp) + c1 * np.power(x, pp + F32(1)) - c2 * np.power(x, pp + F32(2))
        denv = (-(c0 * (pp * np.power(x, pp - F32(1)))) + c1 * ((pp + F32(1)) * np.power(x, pp))
                - c2 * ((pp + F32(2)) * np.power(x, pp + F32(1)))) / rc
    else:
        on = F32(p.r_on)
        r2, o2, k2 = r * r, on * on, rc * rc
        a, b, D = k2 - r2, k2 + F32(2) * r2 - F32(3) * o2, (k2 - o2) * (k2 - o2) * (k2 - o2)
        inside = r < on
        env = np.where(inside, F32(1), a * a * b / D)
        # d/dr of a^2 b / D with a' = -2 r, b' = 4 r, term by term as the product rule accumulates them
        denv = np.where(inside, F32(0), (F32(2) * a * (F32(-2) * r) * b + a * a * (F32(4) * r)) / D)
    emb = basis * env
    demb = dbasis * env + basis * denv
    assert emb.dtype == F32 and demb.dtype == F32
    return emb, demb


def harmonics_restatement32(p, vec, jacobian=True):
    """(sh, dsh) as fp32 numpy arrays: the recursion and its autograd Jacobian carried out in fp32"""
    v = torch.as_tensor(np.asarray(vec, np.float32)).clone().requires_grad_(True)
    sh = spherical_harmonics(p.lmax, v, bool(p.normalize))
    assert sh.dtype == torch.float32
    dsh = None
    if jacobian:
        dsh = _jacobian(sh, v).numpy()
    return sh.detach().numpy(), dsh


def ulp32(scale):
    """one fp32 ulp at |scale| (fp64 array in, fp64 out)"""
    return np.spacing(np.abs(np.asarray(scale, np.float64)).astype(F32)).astype(np.float64)


def bound(ref, restated):
    """-> (per-entry bound [E, ...] broadcast over each edge's row, the restatement's largest error): see the module docstring"""
    ref = np.asarray(ref, np.float64)
    err32 = float(np.abs(np.asarray(restated, np.float64) - ref).max()) if ref.size else 0.0
    row_scale = np.abs(ref.reshape(len(ref), -1)).max(1) if ref.size else np.zeros(len(ref))
    per_edge = 3.0 * err32 + ulp32(row_scale)
    return per_edge.reshape((-1,) + (1,) * (ref.ndim - 1)), err32


@functools.lru_cache(maxsize=None)
def cached_reference(p, group):
    """the references of one (parameter set, case group), computed once and shared: (vec fp32 [E, 3], fp64 dict, fp32 dict);
    callers treat all three as read-only"""
    from edge_cases import lattice_edges, radial_edges
    vec = lattice_edges() if group == 'lattice' else radial_edges(p.rc, p.r_on)
    ref = {k: t.numpy() for k, t in reference64(p, vec).items()}
    emb32, demb32 = radial_restatement32(p, vec)
    sh32, dsh32 = harmonics_restatement32(p, vec)
    return vec, ref, dict(emb=emb32, demb=demb32, sh=sh32, dsh=dsh32)


def force_reference64(fg):
    """forces [n, 3] and per-atom virial [n, 6] (xx, yy, zz, xy, yz, zx) of tests/edge_cases.force_graph in fp64, by index_add_:
    an atom gains g of every edge it is the centre of, loses g of every edge it is the source of, and carries -r (x) g of the latter"""
    g, rij = torch.as_tensor(fg['g']).double(), torch.as_tensor(fg['rij']).double()
    center, src = torch.as_tensor(fg['center']), torch.as_tensor(fg['src'])
    F = torch.zeros(fg['n'], 3, dtype=torch.float64).index_add_(0, center, g).index_add_(0, src, -g)
    rg = torch.stack([rij[:, 0] * g[:, 0], rij[:, 1] * g[:, 1], rij[:, 2] * g[:, 2],
                      rij[:, 0] * g[:, 1], rij[:, 1] * g[:, 2], rij[:, 2] * g[:, 0]], 1)
    va = torch.zeros(fg['n'], 6, dtype=torch.float64).index_add_(0, src, -rg)
    return F.numpy(), va.numpy()
