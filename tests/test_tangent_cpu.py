"""Radial gradient by forward tangent: the identity the fused reverse kernels' tangent mode rests on, in fp64 on the oracle's own
radial MLP and edge embedding (no GPU).

The radial branch of an edge is a function of one scalar: |r| -> emb(|r|) -> h2 = MLP hidden layers -> w = h2 W2.  For any g_w,
    dE/d|r| = sum_k g_w[k] (h2' W2)[k],     h2' = d h2 / d|r|
with h2' by the chain rule from emb' = d emb / d|r| (`tangent_reference` below restates exactly what snet_edge_embed_tangent and
snet_radial_mlp_hidden_fwd_layers_tangent compute; tests/test_tangent_gpu.py measures the kernels against it)."""
import math

import pytest
import torch

from oracle.model import _act, bessel_basis, fcn_apply, normalize2mom_const, poly_cutoff, xplor_cutoff

ACTS = ('silu', 'tanh', 'relu', 'abs', 'ssp', 'sigmoid', 'elu')


def act_grad(name, z):
    """derivative of the radial activations with respect to the pre-activation (relu / abs at 0: torch's convention, 0)"""
    s = torch.sigmoid(z)
    return {'silu': lambda: s * (1 + z * (1 - s)), 'tanh': lambda: 1 - torch.tanh(z) ** 2, 'relu': lambda: (z > 0).to(z.dtype),
            'abs': lambda: torch.sign(z), 'ssp': lambda: s, 'sigmoid': lambda: s * (1 - s),
            'elu': lambda: torch.where(z > 0, torch.ones_like(z), torch.exp(z))}[name]()


def embedding_and_tangent(r, coeffs, rc, kind, p=6, r_on=0.0):
    """emb[n, nb] = Bessel basis x cutoff envelope of |r| and emb' = d emb / d|r|, analytically (what the edge kernels evaluate)"""
    ur = r.unsqueeze(-1)
    f = torch.sin(coeffs * ur) / ur
    df = (coeffs * torch.cos(coeffs * ur) - f) / ur
    if kind == 'poly_cut':
        x = r / rc
        a, b, c = (p + 1.0) * (p + 2.0) / 2.0, p * (p + 2.0), p * (p + 1.0) / 2.0
        env = 1 - a * x ** p + b * x ** (p + 1) - c * x ** (p + 2)
        denv = (-a * p * x ** (p - 1) + b * (p + 1) * x ** p - c * (p + 2) * x ** (p + 1)) / rc
    else:
        r2, c2, o2 = r * r, rc * rc, r_on * r_on
        D = (c2 - o2) ** 3
        env = torch.where(r < r_on, torch.ones_like(r), (c2 - r2) ** 2 * (c2 + 2 * r2 - 3 * o2) / D)
        denv = torch.where(r < r_on, torch.zeros_like(r), 12 * r * (c2 - r2) * (o2 - r2) / D)
    pref = 2.0 / rc
    return pref * f * env.unsqueeze(-1), pref * (df * env.unsqueeze(-1) + f * denv.unsqueeze(-1))


def tangent_reference(emb, demb, W0, W1, act):
    """(h2, h2') of the two hidden layers (weights already divided by sqrt(fan-in)) from emb and emb'"""
    cst = normalize2mom_const(act)
    z1, z1d = emb @ W0, demb @ W0
    a1, a1d = _act(act)(z1) * cst, act_grad(act, z1) * cst * z1d
    z2, z2d = a1 @ W1, a1d @ W1
    return _act(act)(z2) * cst, act_grad(act, z2) * cst * z2d


@pytest.mark.parametrize('kind', ['poly_cut', 'XPLOR'])
@pytest.mark.parametrize('act', ACTS)
def test_tangent_contraction_equals_autograd(act, kind):
    g = torch.Generator().manual_seed(ACTS.index(act) * 2 + (kind == 'XPLOR'))
    rc, r_on, nb, wn, n = 5.0, 4.2, 8, 96, 64
    coeffs = torch.arange(1, nb + 1, dtype=torch.float64) * math.pi / rc
    # lengths over the whole range, below and above the XPLOR switch, and close to the cutoff (the envelope and its slope vanish there)
    r = torch.cat([torch.rand(n - 8, generator=g, dtype=torch.float64) * (rc - 0.8) + 0.7,
                   torch.tensor([4.19, 4.21, rc - 1e-1, rc - 1e-2, rc - 1e-3, rc - 1e-4, rc - 1e-6, 0.5], dtype=torch.float64)])
    W = [torch.randn(a, b, generator=g, dtype=torch.float64) for a, b in ((nb, 64), (64, 64), (64, wn))]
    g_w = torch.randn(n, wn, generator=g, dtype=torch.float64)

    # autograd through the oracle's own functions
    rr = r.clone().requires_grad_(True)
    env = poly_cutoff(rr, rc, 6) if kind == 'poly_cut' else xplor_cutoff(rr, rc, r_on)
    emb_o = bessel_basis(rr, coeffs, rc) * env.unsqueeze(-1)
    w = fcn_apply(emb_o, W, act)
    (ref,) = torch.autograd.grad((w * g_w).sum(), rr)

    emb, demb = embedding_and_tangent(r, coeffs, rc, kind, 6, r_on)
    assert (emb - emb_o.detach()).abs().max() <= 1e-14 * emb_o.abs().max()
    Wn = [w_ / math.sqrt(w_.shape[0]) for w_ in W]
    h2, h2d = tangent_reference(emb, demb, Wn[0], Wn[1], act)
    assert (h2 @ Wn[2] - w.detach()).abs().max() <= 1e-13 * w.abs().max()
    got = (g_w * (h2d @ Wn[2])).sum(1)
    # fp64 rounding: both sides sum wn x 64 products of the same magnitudes in different orders
    assert (got - ref).abs().max() <= 1e-11 * max(1.0, ref.abs().max().item()), (got - ref).abs().max()
    # (close to the cutoff the gradient itself goes to zero with the envelope; the polynomial envelope is evaluated there as a
    # difference of O(30) terms on both sides, so only the absolute bound above is meaningful in fp64)
    assert got[r > rc - 1.5e-2].abs().max() < 1e-3 * ref.abs().max()
