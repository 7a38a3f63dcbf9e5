"""GPU: the kernels that PRODUCE the bounds the fp16-operand fused kernels scale by -- snet_row_absmax(_multi) (x_max, the plug-in's
g_max), snet_gate_bwd_norm / snet_row_norm2 (both hosts' g_max = t_norm ||g_y||_2 1.0001) -- with the gate kernels in both forms
(16-byte and scalar), every activation id, and the Cauchy-Schwarz link between t_norm and the transposed SI2 GEMM it bounds.
Accuracy is always against fp64 torch / the fp64 oracle on the CPU; bit-for-bit identities between two kernels say so."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_ops_gpu import _lib, _p

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ACTS = ('silu', 'tanh', 'relu', 'abs', 'ssp', 'sigmoid', 'elu')
NONVEC = '4x0o+6x0e+3x1o+5x1e+2x2e'   # multiplicities that are no multiples of 4: the scalar gate kernels + snet_row_norm2
# four fp32 roundings: the forms of snet_common.h are a handful of correctly rounded or ~1 ulp operations
ACT_TOL = 4e-7
# The one form that misses it: the silu DERIVATIVE s (1 + z (1 - s)), in libm (act_grad) and hardware exp2 / rcp form alike.  For
# 10 < z < 17.3 the sigmoid s is within a few ulp of 1, so 1 - s carries the rounding of s (up to 2^-24 absolute) and the derivative
# is off by up to z 2^-24 cst.  Observed worst error, over snet_act_bwd and both gate kernels: 9.7e-7 max(1, |ref|) = 2.41 x ACT_TOL
# (24 ulp, at z = 16 .. 17).  Its tolerance is twice the observed value; silu values, and sigmoid values and derivatives, hold ACT_TOL.
SILU_GRAD_TOL = 2 * 9.7e-7


def _z_grid():
    """pre-activations: a dense grid over [-30, 30], zero, tiny values of both signs, and +-87 / +-89 / +-100 where exp2 saturates
    and rcp meets inf and denormals"""
    sp = [0.0, 1e-4, -1e-4, 1e-30, -1e-30, 87.0, -87.0, 89.0, -89.0, 100.0, -100.0]
    return torch.cat([torch.linspace(-30, 30, 601), torch.tensor(sp)]).float()


def _act64(name, z):
    from oracle.model import _act
    from test_tangent_cpu import act_grad
    return _act(name)(z), act_grad(name, z)


def _report(tag, got, ref, tol=ACT_TOL):
    """worst error in units of tol * max(1, |ref|) (printed in units of ACT_TOL)"""
    r = ((got.double() - ref).abs() / (ACT_TOL * ref.abs().clamp(min=1.0))).max().item()
    big = ref.abs() > 1e-30     # (ulp figures only where the reference is far from fp32's denormal range)
    ulp = ((got.double() - ref).abs()[big] / 2.0 ** (torch.floor(torch.log2(ref.abs()[big])) - 23)).max().item() if bool(big.any()) else 0.0
    print(f'{tag}: worst error {r:.3f} x 4e-7 max(1, |ref|), {ulp:.3g} ulp of the reference')
    return r * ACT_TOL / tol


@pytest.mark.parametrize('act', ACTS)
def test_act_kernels_vs_fp64(act):
    """snet_act_fwd / snet_act_bwd (n = 1000), every id: finite, values and derivatives within 4e-7 max(1, |ref|) of fp64 torch
    (the silu derivative: SILU_GRAD_TOL, see there), relu / abs derivative exactly 0 at 0"""
    from sevennet_amd.model_spec import ACT_CST, ACT_ID
    L, lib = _lib()
    grid = _z_grid()
    z = grid[torch.arange(1000) % grid.numel()].contiguous()
    cst = float(np.float32(ACT_CST[act]))
    f64, d64 = _act64(act, z.double())
    zd, one = z.to(DEV), torch.ones(1000, device=DEV)
    a, gz = torch.full((1000,), float('nan'), device=DEV), torch.full((1000,), float('nan'), device=DEV)
    L.check(lib.snet_act_fwd(_p(zd), _p(a), 1000, ACT_ID[act], cst, None))
    L.check(lib.snet_act_bwd(_p(zd), _p(one), _p(gz), 1000, ACT_ID[act], cst, None))
    torch.cuda.synchronize()
    a, gz = a.cpu(), gz.cpu()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(gz).all())
    if act in ('relu', 'abs'):
        assert gz[z == 0].abs().max().item() == 0.0
    assert _report(f'snet_act_fwd {act}', a, f64 * cst) <= 1.0
    assert _report(f'snet_act_bwd {act}', gz, d64 * cst, SILU_GRAD_TOL if act == 'silu' else ACT_TOL) <= 1.0


def test_hidden_layers_silu_at_the_grid():
    """snet_radial_mlp_hidden_fwd (hardware exp2 / rcp silu) with weights that route one input straight through:
    h2[:, 0] = c silu(c silu(z) / 2).  The two matrix products are exact here (one non-zero term, split operands carry 24 bits), so
    the error is that of two activations in a row: 8e-7 max(1, |inner|, |ref|)."""
    from sevennet_amd.model_spec import ACT_CST
    L, lib = _lib()
    z = _z_grid()
    E, nb = z.numel(), 8
    emb = torch.zeros(E, nb)
    emb[:, 0] = z
    W0, W1, W2 = np.zeros((nb, 64), np.float32), np.zeros((64, 64), np.float32), np.zeros((64, 32), np.float32)
    W0[0, 0], W1[0, 0] = 1.0, 0.5
    fp = lambda t: t.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    cst = float(np.float32(ACT_CST['silu']))
    mlp = C.c_void_p()
    L.check(lib.snet_radial_mlp_plan_create(nb, 64, 64, 32, fp(W0), fp(W1), fp(W2), 0, cst, 1, C.byref(mlp)))
    h2 = torch.full((E, 64), float('nan'), device=DEV)
    embd = emb.to(DEV)
    L.check(lib.snet_radial_mlp_hidden_fwd(mlp, _p(embd), E, _p(h2), None))
    torch.cuda.synchronize()
    lib.snet_radial_mlp_plan_destroy(mlp)
    h2 = h2.cpu()
    assert bool(torch.isfinite(h2).all()) and h2[:, 1:].abs().max().item() == 0.0
    inner = torch.nn.functional.silu(z.double()) * cst
    ref = torch.nn.functional.silu(0.5 * inner) * cst
    err = (h2[:, 0].double() - ref).abs() / (2 * ACT_TOL * torch.maximum(inner.abs(), ref.abs()).clamp(min=1.0))
    print(f'snet_radial_mlp_hidden_fwd silu: worst error {err.max().item():.3f} x tolerance')
    assert err.max().item() <= 1.0


def _gate(irr, act):
    """(engine gate spec, oracle gate spec, C segment table) with one activation for scalars and gates of both parities"""
    from oracle.e3 import Irreps as OIrreps
    from oracle.model import GateSpec
    from sevennet_amd.irreps import Irreps
    from sevennet_amd.model_spec import ACT_CST, ACT_ID, make_gate
    L, _ = _lib()
    acts = {'e': act, 'o': act}
    gs = make_gate(Irreps(str(irr)), acts, acts)
    og = GateSpec(OIrreps(str(irr)), acts, acts)
    name = {v: k for k, v in ACT_ID.items()}
    segs = (L.GateSeg * len(gs.segs))()
    for i, s in enumerate(gs.segs):
        segs[i] = L.GateSeg(s.kind, s.in_off, s.out_off, s.mul, s.l, s.gate_off, s.act, ACT_CST[name[s.act]])
    return gs, og, segs


def _real_gate_irreps():
    from sevennet_amd.model_spec import build_model_spec, sevennet_0_config
    gate = build_model_spec(sevennet_0_config()).layers[1].gate
    assert all(s.mul % 4 == 0 and s.in_off % 4 == 0 and s.out_off % 4 == 0 and (s.kind == 0 or s.gate_off % 4 == 0) for s in gate.segs)
    return gate.irreps_out


def _gate_run(gs, segs, y_mi, go_mi, addend_mi=None, norm_mult=None):
    """the gate kernels on mul_ir rows (converted to the engine's ir_mul and back): out, y after the call, g_y of snet_gate_bwd,
    and with norm_mult (g_y, row_norm) of snet_gate_bwd_norm"""
    from sevennet_amd.irreps import irmul_to_mulir_index, mulir_to_irmul_index
    L, lib = _lib()
    N, din, dout = y_mi.shape[0], gs.irreps_in.dim, gs.irreps_out.dim
    to_in, to_out = torch.as_tensor(mulir_to_irmul_index(gs.irreps_in)), torch.as_tensor(mulir_to_irmul_index(gs.irreps_out))
    back_in, back_out = torch.as_tensor(irmul_to_mulir_index(gs.irreps_in)), torch.as_tensor(irmul_to_mulir_index(gs.irreps_out))
    y = y_mi[:, to_in].contiguous().to(DEV)
    go = go_mi[:, to_out].contiguous().to(DEV)
    ad = None if addend_mi is None else addend_mi[:, to_in].contiguous().to(DEV)
    out, gy = torch.full((N, dout), float('nan'), device=DEV), torch.full((N, din), float('nan'), device=DEV)
    L.check(lib.snet_gate_fwd(_p(y), _p(ad), _p(out), N, din, dout, segs, len(gs.segs), None))
    L.check(lib.snet_gate_bwd(_p(y), _p(go), _p(gy), N, din, dout, segs, len(gs.segs), None))
    res = dict(out=out, y=y, g_y=gy)
    if norm_mult is not None:
        gy2, rn = torch.full((N, din), float('nan'), device=DEV), torch.full((N,), float('nan'), device=DEV)
        L.check(lib.snet_gate_bwd_norm(_p(y), _p(go), _p(gy2), N, din, dout, segs, len(gs.segs), norm_mult, _p(rn), None))
        res.update(g_y_norm=gy2, row_norm=rn)
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in res.items()}
    for k, idx in (('out', back_out), ('y', back_in), ('g_y', back_in), ('g_y_norm', back_in)):
        if k in res:
            res[k] = res[k][:, idx]
    return res


def _gate_fwd_tol(og, y, ref):
    """entrywise bound of the gate's forward error: a scalar output is one activation value, ACT_TOL max(1, |ref|); a gated output
    v g multiplies the gate value's error ACT_TOL max(1, |g|) by |v| and rounds once more: ACT_TOL max(|v|, |ref|) + 2^-24 |ref|"""
    tol = ACT_TOL * ref.abs().clamp(min=1.0)
    o = sum(m for m, _ in og.scalars)
    for b in range(og.ng):
        s2, e2 = og._cols[og.ns + og.ng + b]
        v, r = y.double()[:, s2:e2].abs(), ref[:, o:o + e2 - s2].abs()
        tol[:, o:o + e2 - s2] = ACT_TOL * torch.maximum(v, r) + 2.0 ** -24 * r
        o += e2 - s2
    assert o == ref.shape[1]
    return tol


def _norm_bounds(row_norm, g_y, mult):
    """mult ||g_y[n]||_2 <= row_norm[n] <= 1.001 x that, the norm in fp64 over the kernel's own fp32 rows"""
    want = float(np.float32(mult)) * g_y.double().norm(dim=1)
    assert bool((row_norm.double() >= want).all()), ((row_norm.double() / want).min().item())
    assert bool((row_norm.double() <= 1.001 * want).all()), ((row_norm.double() / want).max().item())
    nz = want > 0
    return (row_norm.double()[nz] / want[nz]).min().item() if bool(nz.any()) else 1.0


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('form', ['vec', 'scalar'])
def test_gate_activations_at_the_grid(form, act):
    """both gate kernels, scalar and gate segments, every activation id, at the pre-activation grid.  Gated inputs are 1 and the
    incoming gradient is 1 on scalars and on the first component of every gated channel, so each output entry is one activation value
    or derivative times its constant (or an exact 0 / copy): entrywise within 4e-7 max(1, |ref|) of the fp64 oracle gate and its
    autograd (the silu derivative: SILU_GRAD_TOL).  form 'vec': the gate of SevenNet-0's middle layer (16-byte kernels); 'scalar': multiplicities 4, 6, 3, 5, 2."""
    irr = _real_gate_irreps() if form == 'vec' else NONVEC
    gs, og, segs = _gate(irr, act)
    grid = _z_grid()
    din, dout, N = og.irreps_in.dim, og.irreps_out.dim, grid.numel() + 1   # (the last block of four rows is partial)
    n_z = max(e for _, e in og._cols[:og.ns + og.ng])      # scalars and gates (l = 0) come first in the gate's sorted input
    assert n_z == sum(m for m, _ in og.scalars) + sum(m for m, _ in og.gates)
    y = torch.ones(N, din)
    y[:, :n_z] = grid[(torch.arange(N)[:, None] + 53 * torch.arange(n_z)[None, :]) % grid.numel()]   # every column sees every value
    go = torch.zeros(N, dout)
    o = 0
    for m, (l, _) in og.irreps_out:
        go[:, o:o + m * (2 * l + 1):2 * l + 1] = 1.0
        o += m * (2 * l + 1)
    y64 = y.double().requires_grad_(True)
    ref = og.apply(y64)
    (gref,) = torch.autograd.grad(ref, y64, go.double())
    got = _gate_run(gs, segs, y, go)
    assert bool(torch.isfinite(got['out']).all()) and bool(torch.isfinite(got['g_y']).all())
    assert _report(f'gate fwd {form} {act}', got['out'], ref.detach()) <= 1.0
    assert _report(f'gate bwd {form} {act}', got['g_y'], gref, SILU_GRAD_TOL if act == 'silu' else ACT_TOL) <= 1.0
    if act in ('relu', 'abs'):
        assert got['g_y'][:, :n_z][y[:, :n_z] == 0].abs().max().item() == 0.0


@pytest.mark.parametrize('N', [1, 3, 9, 301])
@pytest.mark.parametrize('form', ['vec', 'scalar'])
def test_gate_kernels_and_row_norm(form, N):
    """gate of a real layer (16-byte kernels; the last block of four rows is partial for N = 1, 3, 9, 301) and the scalar form:
    forward == fp64 oracle gate with and without addend, y += addend exactly; reverse == fp64 autograd; snet_gate_bwd_norm returns
    snet_gate_bwd's g_y bit for bit and row_norm within [1, 1.001] x norm_mult ||g_y||_2; a zero row gives 0.  The forward bound is
    _gate_fwd_tol (the real gate's products reach 25, where 2e-6 absolute is one ulp); the reverse one on these randn rows is
    test_gate_and_halo_kernels' (5e-6, absolute)."""
    irr = _real_gate_irreps() if form == 'vec' else NONVEC
    gs, og, segs = _gate(irr, 'silu')
    g = torch.Generator().manual_seed(5 + N)
    din, dout = og.irreps_in.dim, og.irreps_out.dim
    y, go, ad = torch.randn(N, din, generator=g), torch.randn(N, dout, generator=g), torch.randn(N, din, generator=g)
    go[N // 2] = 0.0                      # a row of zeros
    y64 = y.double().requires_grad_(True)
    ref = og.apply(y64)
    (gref,) = torch.autograd.grad(ref, y64, go.double())
    tight = []
    for mult in (1.0, 0.37):
        got = _gate_run(gs, segs, y, go, norm_mult=mult)
        assert bool(((got['out'].double() - ref.detach()).abs() <= _gate_fwd_tol(og, y, ref.detach())).all())
        assert (got['g_y'].double() - gref).abs().max().item() < 5e-6
        assert torch.equal(got['y'], y)                                  # no addend: the input is left alone
        assert torch.equal(got['g_y_norm'], got['g_y'])                  # identity between two kernels, bit for bit
        tight.append(_norm_bounds(got['row_norm'], got['g_y'], mult))
        assert got['row_norm'][N // 2].item() == 0.0 and got['g_y'][N // 2].abs().max().item() == 0.0
    print(f'gate row_norm {form} N={N}: smallest row_norm / (norm_mult ||g_y||) = {min(tight):.7f}')
    # self-connection add fused into the forward kernel: gate(y + a), y <- y + a (the fp32 sum, exactly)
    ysum = y + ad
    ref2 = og.apply(ysum.double())
    got = _gate_run(gs, segs, y, go, addend_mi=ad)
    assert torch.equal(got['y'], ysum)
    assert bool(((got['out'].double() - ref2).abs() <= _gate_fwd_tol(og, ysum, ref2)).all())


@pytest.mark.parametrize('dim', [480, 30, 1])
def test_row_norm2_two_sided(dim):
    """snet_row_norm2 alone, 16-byte and scalar loads, rows of magnitude 2^-40 .. 2^30 and a row of zeros"""
    L, lib = _lib()
    N = 203
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(N, dim, generator=g) * (2.0 ** torch.tensor([-40, -20, 0, 20, 30])[torch.arange(N) % 5].float())[:, None]
    x[7] = 0.0
    xd = x.to(DEV)
    for mult in (1.0, 0.37):
        out = torch.full((N,), float('nan'), device=DEV)
        L.check(lib.snet_row_norm2(_p(xd), N, dim, mult, _p(out), None))
        torch.cuda.synchronize()
        _norm_bounds(out.cpu(), x, mult)
        assert out[7].item() == 0.0


def test_row_absmax_exact_on_mixed_rows():
    """snet_row_absmax and snet_row_absmax_multi == x.abs().amax(1) exactly: entries of 2^-40 .. 2^30 inside one row, a row of zeros,
    dim = 1, row counts that are no multiples of 4 (four rows per workgroup)"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(3)
    shapes = [(37, 480), (5, 1), (203, 30), (1, 64)]
    xs = []
    for r, d in shapes:
        k = torch.randint(-40, 31, (r, d), generator=g).float()
        x = torch.randn(r, d, generator=g) * 2.0 ** k
        x[r // 2] = 0.0
        xs.append(x.to(DEV))
    n = len(xs)
    multi = [torch.full((r,), float('nan'), device=DEV) for r, _ in shapes]
    L.check(lib.snet_row_absmax_multi((C.c_void_p * n)(*[x.data_ptr() for x in xs]), (C.c_int64 * n)(*[r for r, _ in shapes]),
                                      (C.c_int32 * n)(*[d for _, d in shapes]), (C.c_void_p * n)(*[o.data_ptr() for o in multi]), n, None))
    for x, m, (r, d) in zip(xs, multi, shapes):
        one = torch.full((r,), float('nan'), device=DEV)
        L.check(lib.snet_row_absmax(_p(x), r, d, _p(one), None))
        torch.cuda.synchronize()
        want = x.abs().amax(1)
        assert torch.equal(one, want) and torch.equal(m, want)
        assert one[r // 2].item() == 0.0


@pytest.mark.parametrize('model,layer', [('sevennet_0', 1), ('sevennet_mf_ompa', 2)])
def test_t_norm_bounds_the_transposed_si2_gemm(model, layer):
    """the Cauchy-Schwarz link: with the engine's own operator for SI2 (random weights) and the transposed GEMM both hosts run,
    max_k |g_m[n, k]| <= t_norm ||g_y[n]||_2 1.0001 for every row -- randn rows, rows equal to +- the weight row that attains t_norm
    (the equality case: 1.0001 against the bf16x6 GEMM's rounding) and rows scaled by 2^+-20 -- and the bound the reverse pass really
    uses, snet_row_norm2(g_y, t_norm), covers every entry.  (Neither snet_model_info nor snet_model_meta exposes the native host's
    t_norm, so the two hosts' values are not compared here.)"""
    from sevennet_amd import model_spec as M
    from sevennet_amd.engine import _Linear, species_row_lists
    from sevennet_amd.model_spec import linear_weight_matrices
    L, lib = _lib()
    cfg = {'sevennet_0': M.sevennet_0_config, 'sevennet_mf_ompa': M.sevennet_mf_ompa_config}[model]()
    ms = M.build_model_spec(cfg)
    sp = ms.layers[layer].si2
    rng = np.random.default_rng(layer)
    flat = rng.normal(0, 1, sp.numel).astype(np.float32).astype(np.float64)
    lin = _Linear(sp, flat, torch.device(DEV), True, 0 if sp.n_modal else -1, None)
    mats = linear_weight_matrices(sp, flat)
    # the input entry whose transposed-map row is the longest, and that row laid out as a g_y row (first component of every block)
    best, row, species = -1.0, None, -1
    for key in {(b.in_off, b.species) for b in sp.blocks}:
        blocks = [(b, m) for b, m in zip(sp.blocks, mats) if (b.in_off, b.species) == key]
        v = sum((m.astype(np.float64) ** 2).sum(1) for _, m in blocks)
        k = int(v.argmax())
        if v[k] > best:
            best, species = float(v[k]), key[1]
            row = np.zeros(sp.dim_out)
            for b, m in blocks:
                row[b.out_off:b.out_off + b.mul_out] = m[k]
    assert abs(np.sqrt(best) - lin.t_norm) <= 1e-12 * lin.t_norm and abs(np.linalg.norm(row) - lin.t_norm) <= 1e-12 * lin.t_norm
    N = 64
    g = torch.Generator().manual_seed(layer)
    gy = torch.randn(N, sp.dim_out, generator=g, dtype=torch.float64)
    gy[0], gy[1] = torch.from_numpy(row), -torch.from_numpy(row)
    gy[2], gy[3] = torch.from_numpy(row) * 2.0 ** 20, torch.from_numpy(row) * 2.0 ** -20
    gy[4:24] *= 2.0 ** 20
    gy[24:44] *= 2.0 ** -20
    gy = gy.float().contiguous()
    n_species = max(sp.n_species, 1)
    types = torch.full((N,), max(species, 0), dtype=torch.int32)
    types[8:] = torch.randint(0, n_species, (N - 8,), generator=g).to(torch.int32)
    rows = species_row_lists(types.to(DEV), n_species)
    gyd = gy.to(DEV)
    gm = torch.full((N, sp.dim_in), float('nan'), device=DEV)
    for off, ln in lin.zero_in:
        gm[:, off:off + ln] = 0.0
    for s, arr, cnt in lin.groups_T:
        r, m = (None, N) if s < 0 else (rows[s], rows[s].numel())
        if m:
            L.check(lib.snet_gemm_grouped(arr, cnt, _p(gyd), _p(gm), m, sp.dim_out, sp.dim_in, _p(r), None))
    bound = torch.full((N,), float('nan'), device=DEV)
    L.check(lib.snet_row_norm2(_p(gyd), N, sp.dim_out, lin.t_norm, _p(bound), None))
    torch.cuda.synchronize()
    gm, bound = gm.cpu(), bound.cpu()
    assert bool(torch.isfinite(gm).all())
    top = gm.abs().amax(1).double()
    cs = lin.t_norm * gy.double().norm(dim=1)
    ratio = top / cs
    print(f'{model} SI2^T: t_norm {lin.t_norm:.6g}; max|g_m| / (t_norm ||g_y||): equality rows {ratio[:4].tolist()}, largest {ratio.max().item():.7f}; '
          f'smallest snet_row_norm2 bound / max|g_m| {(bound.double() / top).min().item():.7f}')
    assert bool((ratio[:4] > 0.999).all())            # the equality case really is one
    assert bool((top <= cs * 1.0001).all()), ratio.max().item()
    assert bool((bound.double() >= top).all())
