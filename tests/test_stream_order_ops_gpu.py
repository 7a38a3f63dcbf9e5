"""GPU: the stream contract of the C-ABI entry points, one by one (tests/stream_order.py has the method).

Every row makes its call on a fresh non-default stream whose first work item is a delay; the floating-point inputs arrive behind
the delay on that stream.  The outputs must be bit for bit those of the same call on the default stream: a launch, memset or copy
the library put elsewhere reads the stale inputs, or leaves the NaN the outputs were filled with.  Shapes are the smallest of the
direct tests (N <= 301 rows, the ragged graph of test_ops_gpu, systems of 1 / 5 / 64 atoms); every row is bit-repeatable on the default
stream (asserted per row).  The three reductions on the shared scratch (snet::reduce_scratch) and their _seg variants are also
checked against an fp64 torch restatement here: they had no direct test.

The positive control shows the harness catching a deliberate mistake: snet_act_fwd with a NULL stream while its input is late."""
import ctypes as C

import numpy as np
import pytest
import torch

from stream_order import MIN_DELAY_MS, assert_pending, delayed_stream, late_copy, run_ab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CST = 1.6791767923989418
SEG = [0, 1, 6, 70, 301]      # systems of 1, 5, 64 and 231 rows


def _lib():
    from sevennet_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _late(a, seed=1, keep_sign=False):
    """(buffer, A, B) for the device tensor A: B differs from A in every entry (a relative and an absolute perturbation)"""
    a = a.contiguous()
    g = _gen(1000 + seed)
    r = torch.randn(a.shape, generator=g, dtype=torch.float64).to(a.device)
    b = a.double() * (1.0 + 0.1 * r.clamp(-3, 3)) + (0.0 if keep_sign else 0.01) * torch.randn(a.shape, generator=g, dtype=torch.float64).to(a.device)
    return (a.clone(), a, b.to(a.dtype).contiguous())


def _dev(t):
    return t.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ the harness on itself
def test_positive_control_null_stream_reads_the_stale_input():
    """snet_act_fwd with stream NULL while its input is late on s: the output is the activation of A (the stale input); with s
    passed it is that of B.  Without this the file proves nothing about itself."""
    L, lib = _lib()
    n = 301 * 96
    buf, A, B = _late(_dev(torch.randn(n, generator=_gen(3))))
    want = {}
    for k, v in (('A', A), ('B', B)):
        out = torch.full((n,), float('nan'), device=DEV)
        L.check(lib.snet_act_fwd(_p(v), _p(out), n, 0, CST, L.stream()))
        torch.cuda.synchronize()
        want[k] = out
    assert not torch.equal(want['A'], want['B'])
    got = {}
    for how in ('null', 's'):
        buf.copy_(A)
        out = torch.full((n,), float('nan'), device=DEV)
        torch.cuda.synchronize()
        s = delayed_stream(MIN_DELAY_MS)
        late_copy(s, [(buf, A, B)], 2)
        with torch.cuda.stream(s):
            L.check(lib.snet_act_fwd(_p(buf), _p(out), n, 0, CST, None if how == 'null' else L.stream()))
        pending = assert_pending(s, f'positive control ({how})')
        s.synchronize()
        torch.cuda.synchronize()
        got[how] = out.clone()
        print(f'[stream_order] positive control ({how}): delay {MIN_DELAY_MS:.0f} ms, pending = {pending}, '
              f'output is act({"A" if torch.equal(out, want["A"]) else "B" if torch.equal(out, want["B"]) else "?"})', flush=True)
    assert torch.equal(got['null'], want['A'])      # the mistake is seen: the stale result
    assert torch.equal(got['s'], want['B'])         # ... and the correct call gives the fresh one


def test_control_stray_second_launch_reads_the_kept_intermediate():
    """A two-launch entry point emulated with snet_act_fwd twice through an intermediate buffer that lives between calls, as
    snet::reduce_scratch does (the harness neither resets nor NaN-fills it).  In order on the current stream the runner passes;
    with the SECOND launch on the NULL stream it must fail: the stray launch reads the intermediate the previous call left --
    A-derived, because the runner's last default-stream call has inputs A -- and produces A's result."""
    L, lib = _lib()
    n = 301 * 96
    x = _late(_dev(torch.randn(n, generator=_gen(4))))
    kept, out = torch.zeros(n, device=DEV), torch.empty(n, device=DEV)

    def two_launches(second_stream):
        def call():
            L.check(lib.snet_act_fwd(_p(x[0]), _p(kept), n, 0, CST, L.stream()))
            L.check(lib.snet_act_fwd(_p(kept), _p(out), n, 1, 1.0, second_stream()))
        return call
    run_ab('control[two launches, in order]', [x], two_launches(L.stream), [out])
    with pytest.raises(AssertionError, match='STALE'):
        run_ab('control[two launches, the second on the NULL stream]', [x], two_launches(lambda: None), [out])


# ------------------------------------------------------------------------------------------------ reductions on the shared scratch
def _reduction_inputs():
    g = _gen(7)
    n, dim, ns = SEG[-1], 96, 3
    types = torch.randint(0, ns, (n,), generator=g).to(torch.int32)
    scale = torch.tensor([0.8, 1.3, 1.1])
    shift = torch.tensor([-5.0, -3.5, -7.25])       # atomic energies of one sign: "relative" has no cancellation to hide behind
    x = torch.randn(n, dim, generator=g)
    v = 0.2 * torch.randn(dim, generator=g, dtype=torch.float64) / dim ** 0.5     # |x . v| and |e| stay below 1.5: every
    e = 0.2 * torch.randn(n, generator=g)                                           # atomic energy keeps the sign of its shift
    # a graph for snet_edge_force: edges sorted by centre, ragged degrees, atoms without in- or out-edges
    deg = torch.randint(0, 9, (n,), generator=g)
    deg[[0, 5, 300]] = 0
    center = torch.repeat_interleave(torch.arange(n), deg)
    E = int(deg.sum())
    src = torch.randint(1, n, (E,), generator=g)    # (atom 0 is nobody's source either)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(deg, 0)
    col_ptr = torch.zeros(n + 1, dtype=torch.int64)
    col_ptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
    eperm = torch.sort(src, stable=True).indices
    return dict(n=n, dim=dim, ns=ns, types=types, scale=scale, shift=shift, x=x, v=v, c=0.37, e=e, E=E, center=center, src=src,
                row_ptr=row_ptr.to(torch.int32), col_ptr=col_ptr.to(torch.int32), eperm=eperm.to(torch.int32),
                g_vec=torch.randn(E, 3, generator=g), edge_vec=torch.randn(E, 3, generator=g) * 2.0,
                seg_ptr=torch.tensor(SEG, dtype=torch.int32))


def _reduction_rows():
    """name -> (late, call, outs): the six reductions with their integer arrays on the device and synchronised"""
    L, lib = _lib()
    c = _reduction_inputs()
    n, dim, ns, E, B = c['n'], c['dim'], c['ns'], c['E'], len(SEG) - 1
    types, scale, shift, v, seg_ptr = (_dev(c[k]) for k in ('types', 'scale', 'shift', 'v', 'seg_ptr'))
    rp, cp, ep = (_dev(c[k]) for k in ('row_ptr', 'col_ptr', 'eperm'))
    f32 = lambda *s: torch.empty(*s, device=DEV)                          # noqa: E731
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=DEV)     # noqa: E731
    x, e, gv, ev = _late(_dev(c['x']), 1), _late(_dev(c['e']), 2), _late(_dev(c['g_vec']), 3), _late(_dev(c['edge_vec']), 4)
    ea, tot, eseg = f32(n), f64(1), f64(B)
    F, va, vt, vseg = f32(n, 3), f32(n, 6), f64(6), f64(B, 6)
    torch.cuda.synchronize()
    rows = {
        'snet_rescale_reduce': ([e], lambda: L.check(lib.snet_rescale_reduce(_p(e[0]), _p(types), _p(scale), _p(shift), ns, n, _p(ea), _p(tot),
                                                                            L.stream())), [ea, tot]),
        'snet_readout_energy': ([x], lambda: L.check(lib.snet_readout_energy(_p(x[0]), n, dim, _p(v), c['c'], _p(types), _p(scale), _p(shift), ns,
                                                                            _p(ea), _p(tot), L.stream())), [ea, tot]),
        'snet_edge_force': ([gv, ev], lambda: L.check(lib.snet_edge_force(_p(gv[0]), _p(ev[0]), _p(rp), _p(cp), _p(ep), n, E, _p(F), _p(va), _p(vt),
                                                                         L.stream())), [F, va, vt]),
        'snet_rescale_reduce_seg': ([e], lambda: L.check(lib.snet_rescale_reduce_seg(_p(e[0]), _p(types), _p(scale), _p(shift), ns, n, _p(seg_ptr), B,
                                                                                    _p(ea), _p(eseg), _p(tot), L.stream())), [ea, eseg, tot]),
        'snet_readout_energy_seg': ([x], lambda: L.check(lib.snet_readout_energy_seg(_p(x[0]), n, dim, _p(v), c['c'], _p(types), _p(scale), _p(shift),
                                                                                    ns, _p(seg_ptr), B, _p(ea), _p(eseg), _p(tot), L.stream())),
                                    [ea, eseg, tot]),
        'snet_edge_force_seg': ([gv, ev], lambda: L.check(lib.snet_edge_force_seg(_p(gv[0]), _p(ev[0]), _p(rp), _p(cp), _p(ep), n, E, _p(seg_ptr), B,
                                                                                 _p(F), _p(va), _p(vseg), _p(vt), L.stream())), [F, va, vseg, vt]),
    }
    return c, rows


REDUCTIONS = ['snet_rescale_reduce', 'snet_readout_energy', 'snet_edge_force', 'snet_rescale_reduce_seg', 'snet_readout_energy_seg',
              'snet_edge_force_seg']


@pytest.mark.parametrize('name', REDUCTIONS)
def test_reduction_on_a_delayed_stream_and_vs_fp64(name):
    """The stream contract, then the values of the default-stream call (inputs B) against an fp64 torch restatement:
    atomic energies within one fp32 rounding of the fp64 value (2^-23 of the largest term: the product and the sum round, or fuse);
    energies 1e-12 relative (an fp64 sum of 301 terms of one sign: 301 x 2^-53 = 3.4e-14); per-system sums equal to the fp64 sum of
    their rows and the total to the sum of the per-system sums at the same 1e-12; forces within (in + out degree) fp32 roundings
    of sum |g|; the virial, whose terms change sign, at 1e-12 of sum |terms|."""
    c, rows = _reduction_rows()
    late, call, outs = rows[name]
    ref, _ = run_ab(name, late, call, outs)
    h = lambda t: t.double().cpu()   # noqa: E731
    n, B, ns = c['n'], len(SEG) - 1, c['ns']
    t = c['types'].long()
    sc, sh = c['scale'].double()[t], c['shift'].double()[t]
    seg_sum = lambda a: torch.stack([a[SEG[b]:SEG[b + 1]].sum(0) for b in range(B)])   # noqa: E731
    if 'rescale' in name or 'readout' in name:
        if 'rescale' in name:
            inner = h(late[0][2]) * sc
        else:
            inner = (h(late[0][2]) @ c['v'] + c['c']) * sc
        e64 = inner + sh
        ea = h(ref[0])
        assert ((ea - e64).abs() <= 2.0 ** -23 * (inner.abs() + sh.abs())).all()
        assert (e64 < 0).all()
        rows64 = ea if 'rescale' in name else e64        # rescale sums the stored fp32 values, the readout its unrounded fp64 ones
        total = h(ref[-1])[0]
        assert abs(total - rows64.sum()) <= 1e-12 * abs(rows64.sum()), (total, rows64.sum())
        if name.endswith('_seg'):
            es = h(ref[1])
            assert ((es - seg_sum(rows64)).abs() <= 1e-12 * seg_sum(rows64).abs()).all()
            assert abs(total - es.sum()) <= 1e-12 * abs(es.sum())
    else:
        g, r = h(late[0][2]), h(late[1][2])
        ctr, src = c['center'], c['src']
        F64 = torch.zeros(n, 3, dtype=torch.float64).index_add_(0, ctr, g).index_add_(0, src, -g)
        mag = torch.zeros(n, 3, dtype=torch.float64).index_add_(0, ctr, g.abs()).index_add_(0, src, g.abs())
        cnt = torch.bincount(ctr, minlength=n) + torch.bincount(src, minlength=n)
        assert ((h(ref[0]) - F64).abs() <= (cnt[:, None] + 1) * 2.0 ** -24 * mag).all()
        assert (h(ref[0])[0] == 0).all()                                             # the atom without any edge
        six = -torch.stack([r[:, 0] * g[:, 0], r[:, 1] * g[:, 1], r[:, 2] * g[:, 2], r[:, 0] * g[:, 1], r[:, 1] * g[:, 2], r[:, 2] * g[:, 0]], 1)
        va64 = torch.zeros(n, 6, dtype=torch.float64).index_add_(0, src, six)
        vmag = torch.zeros(n, 6, dtype=torch.float64).index_add_(0, src, six.abs())
        n_out = torch.bincount(src, minlength=n)
        va = h(ref[1])
        assert ((va - va64).abs() <= (n_out[:, None] + 1) * 2.0 ** -23 * vmag).all()
        total = h(ref[-1])
        assert ((total - va.sum(0)).abs() <= 1e-12 * va.abs().sum(0)).all()
        if name.endswith('_seg'):
            vs = h(ref[2])
            assert ((vs - seg_sum(va)).abs() <= 1e-12 * seg_sum(va.abs())).all()
            assert ((total - vs.sum(0)).abs() <= 1e-12 * vs.abs().sum(0)).all()


# ------------------------------------------------------------------------------------------------ the table
def _pack_split(L, lib, B):
    Bh = np.ascontiguousarray(B.cpu().numpy(), np.float32)
    K, N = Bh.shape
    buf = np.empty(int(lib.snet_gemm_split_size(K, N)), np.uint8)
    L.check(lib.snet_gemm_split_pack(C.c_void_p(Bh.ctypes.data), K, N, C.c_void_p(buf.ctypes.data)))
    return torch.from_numpy(buf).to(DEV)


def _row_gemm(packed):
    L, lib = _lib()
    g = _gen(11)
    n, din, dout, probs = 301, 61, 83, [(1, 4, 7, 0, 0), (3, 9, 20, 4, 7), (5, 6, 3, 31, 67)]
    A = _late(_dev(torch.randn(n, din, generator=g)))
    Bs = [_dev(torch.randn(K, N, generator=g)) for (_, K, N, _, _) in probs]
    out = torch.empty(n, dout, device=DEV)
    if packed is None:      # snet_gemm: one block, strided, on a list of rows
        rows = _dev(torch.arange(0, n, 2, dtype=torch.int32))
        d, K, N, ao, co = probs[1]

        def call():
            out.zero_()     # (rows off the list are not written)
            L.check(lib.snet_gemm(_p(A[0]), _p(Bs[1]), _p(out), rows.numel(), d, K, N, din, ao, dout, co, _p(rows), 0, L.stream()))
        return dict(late=[A], call=call, outs=[out])
    keep = [_pack_split(L, lib, B) for B in Bs] if packed else Bs
    descs = (L.GemmDesc * 3)(*[L.GemmDesc(None if packed else W.data_ptr(), W.data_ptr() if packed else None, ao, co, d, K, N, 0)
                               for (d, K, N, ao, co), W in zip(probs, keep)])

    def call():
        out.zero_()         # (columns between the blocks are not written)
        L.check(lib.snet_gemm_grouped(descs, 3, _p(A[0]), _p(out), n, din, dout, None, L.stream()))
    return dict(late=[A], call=call, outs=[out], keep=keep)


def _row_gate(which):
    from test_bound_producers_gpu import NONVEC, _gate, _real_gate_irreps
    L, lib = _lib()
    vec = which != 'bwd_norm_scalar'
    gs, _, segs = _gate(_real_gate_irreps() if vec else NONVEC, 'silu')
    N, din, dout, g = 301, gs.irreps_in.dim, gs.irreps_out.dim, _gen(5)
    y = _late(_dev(torch.randn(N, din, generator=g)), 1)
    if which == 'fwd_addend':
        ad = _late(_dev(torch.randn(N, din, generator=g)), 2)
        out = torch.empty(N, dout, device=DEV)
        return dict(late=[y, ad], outs=[out, y[0]],     # (y is updated in place to y + addend)
                    call=lambda: L.check(lib.snet_gate_fwd(_p(y[0]), _p(ad[0]), _p(out), N, din, dout, segs, len(gs.segs), L.stream())))
    go = _late(_dev(torch.randn(N, dout, generator=g)), 3)
    gy, rn = torch.empty(N, din, device=DEV), torch.empty(N, device=DEV)
    # (the scalar form is two launches: the gate kernel, then snet_row_norm2 over what it wrote)
    return dict(late=[y, go], outs=[gy, rn],
                call=lambda: L.check(lib.snet_gate_bwd_norm(_p(y[0]), _p(go[0]), _p(gy), N, din, dout, segs, len(gs.segs), 1.25, _p(rn), L.stream())))


def _row_node(which):
    L, lib = _lib()
    g = _gen(6)
    if which in ('segment_sum_rows', 'segment_sum_rows_chunked'):
        E, N, dim = 301, 38, 96
        x = _late(_dev(torch.randn(E, dim, generator=g)))
        src = torch.randint(0, N, (E,), generator=g)
        perm = _dev(torch.sort(src, stable=True).indices.to(torch.int32))
        ptr = torch.zeros(N + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
        ptr = _dev(ptr.to(torch.int32))
        out = torch.empty(N, dim, device=DEV)
        if which == 'segment_sum_rows':
            return dict(late=[x], outs=[out], call=lambda: L.check(lib.snet_segment_sum_rows(_p(x[0]), _p(ptr), _p(perm), N, dim, _p(out), L.stream())))
        cpos = _dev(torch.tensor([3, 0, 5, 1, 4, 2], dtype=torch.int32))
        return dict(late=[x], outs=[out], keep=cpos,
                    call=lambda: L.check(lib.snet_segment_sum_rows_chunked(_p(x[0]), _p(ptr), _p(perm), N, dim, _p(cpos), _p(out), L.stream())))
    if which == 'row_absmax_multi':
        shapes = [(301, 96), (3, 128), (38, 30)]
        xs = [_late(_dev(torch.randn(r, d, generator=g)), k) for k, (r, d) in enumerate(shapes)]
        outs = [torch.empty(r, device=DEV) for r, _ in shapes]
        n = len(shapes)
        return dict(late=xs, outs=outs,
                    call=lambda: L.check(lib.snet_row_absmax_multi((C.c_void_p * n)(*[x[0].data_ptr() for x in xs]), (C.c_int64 * n)(*[r for r, _ in shapes]),
                                                                   (C.c_int32 * n)(*[d for _, d in shapes]), (C.c_void_p * n)(*[o.data_ptr() for o in outs]),
                                                                   n, L.stream())))
    x = _late(_dev(torch.randn(301, 30, generator=g)))
    out = torch.empty(301, device=DEV)
    return dict(late=[x], outs=[out], call=lambda: L.check(lib.snet_row_norm2(_p(x[0]), 301, 30, 1.5, _p(out), L.stream())))


def _edge_setup(E=301, nb=8, lmax=2):
    L, _ = _lib()
    g = _gen(3)
    v = torch.randn(E, 3, generator=g)
    v = v / v.norm(dim=1, keepdim=True) * (1.5 + 2.3 * torch.rand(E, 1, generator=g))     # 1.5 .. 3.8 A; B = A (1 +- 0.3) stays inside (1 A, 5 A)
    P = L.EdgeParams(5.0, nb, 0, 6, 4.5, lmax, 1)
    cf = (C.c_float * nb)(*[(k + 1) * np.pi / 5.0 for k in range(nb)])
    vec = _late(_dev(v), keep_sign=True)
    assert float(vec[2].norm(dim=1).max()) < 5.0 and float(vec[2].norm(dim=1).min()) > 1.0
    return L, g, P, cf, vec, (lmax + 1) ** 2


def _row_edge(which):
    L, lib = _lib()
    E, nb = 301, 8
    L, g, P, cf, vec, nsh = _edge_setup(E, nb)
    if which == 'fwd':
        emb, sh, dsh = torch.empty(E, nb, device=DEV), torch.empty(E, nsh, device=DEV), torch.empty(E, nsh, 3, device=DEV)
        return dict(late=[vec], outs=[emb, sh, dsh], keep=(P, cf),
                    call=lambda: L.check(lib.snet_edge_embed_fwd(C.byref(P), cf, _p(vec[0]), E, _p(emb), _p(sh), _p(dsh), L.stream())))
    if which == 'bwd':
        ge, gs = _late(_dev(torch.randn(E, nb, generator=g)), 2), _late(_dev(torch.randn(E, nsh, generator=g)), 3)
        gv = torch.empty(E, 3, device=DEV)
        return dict(late=[vec, ge, gs], outs=[gv], keep=(P, cf),
                    call=lambda: L.check(lib.snet_edge_embed_bwd(C.byref(P), cf, _p(vec[0]), E, _p(ge[0]), _p(gs[0]), _p(gv), 0, L.stream())))
    R = 150
    rows = _dev(torch.randint(0, E, (R,), generator=g).to(torch.int32))        # one radial row per pair: the edge it stands for
    demb = torch.empty(R, nb, device=DEV)
    return dict(late=[vec], outs=[demb], keep=(P, cf, rows),
                call=lambda: L.check(lib.snet_edge_embed_tangent(C.byref(P), cf, _p(vec[0]), _p(rows), R, _p(demb), L.stream())))


def _mlp_plan(L, lib, nb, wn, g):
    W0 = (torch.randn(nb, 64, generator=g) / nb ** 0.5).contiguous()
    W1 = (torch.randn(64, 64, generator=g) / 8).contiguous()
    W2 = (torch.randn(64, wn, generator=g) / 8).contiguous()
    fp = lambda t: t.numpy().ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    plan = C.c_void_p()
    L.check(lib.snet_radial_mlp_plan_create(nb, 64, 64, wn, fp(W0), fp(W1), fp(W2), 0, CST, 1, C.byref(plan)))
    return plan


def _row_mlp(which):
    L, lib = _lib()
    g = _gen(2)
    E, nb, wn = 257, 8, 224
    plan = _mlp_plan(L, lib, nb, wn, g)
    emb = _late(_dev(torch.randn(E, nb, generator=g)), 1)
    S = L.stream
    if which == 'fwd':
        w = torch.empty(E, wn, device=DEV)
        return dict(late=[emb], outs=[w], keep=plan, call=lambda: L.check(lib.snet_radial_mlp_fwd(plan, _p(emb[0]), E, _p(w), S())))
    if which == 'hidden_fwd':
        h2 = torch.empty(E, 64, device=DEV)
        return dict(late=[emb], outs=[h2], keep=plan, call=lambda: L.check(lib.snet_radial_mlp_hidden_fwd(plan, _p(emb[0]), E, _p(h2), S())))
    g_emb, one = torch.empty(E, nb, device=DEV), torch.ones(E, nb, device=DEV)      # accumulated into
    if which == 'bwd':
        gw = _late(_dev(torch.randn(E, wn, generator=g)), 2)
        return dict(late=[emb, gw], outs=[g_emb], prefill=[(g_emb, one)], keep=plan,
                    call=lambda: L.check(lib.snet_radial_mlp_bwd(plan, _p(emb[0]), _p(gw[0]), E, _p(g_emb), S())))
    gh = _late(_dev(torch.randn(E, 64, generator=g)), 3)
    return dict(late=[emb, gh], outs=[g_emb], prefill=[(g_emb, one)], keep=plan,
                call=lambda: L.check(lib.snet_radial_mlp_hidden_bwd(plan, _p(emb[0]), _p(gh[0]), E, _p(g_emb), S())))


def _row_conv(which):
    """the SevenNet-0 middle shape on the 38-node ragged graph of test_ops_gpu (degrees 0, 1, 15 .. 17, 31 .. 33, 70; ghost rows;
    pair-shared radial rows), fused kernels with terms = 4 (fp16 operands, the engine's default)"""
    from test_ops_gpu import _fused_case, _work_list
    L, lib = _lib()
    c = _fused_case('sevennet_0', 1, 41, True)
    spec, nb, wn, dx, dout, nsh, N, NT, E, R = (c[k] for k in ('spec', 'nb', 'wn', 'dx', 'dout', 'nsh', 'N', 'NT', 'E', 'R'))
    assert N == 37 and NT == 44        # (with the ghost rows the graph has 44 source rows)
    fp = lambda t: t.numpy().ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    mlp, plan, fplan = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.check(lib.snet_radial_mlp_plan_create(nb, 64, 64, wn, fp(c['W0']), fp(c['W1']), fp(c['W2']), 0, CST, 1, C.byref(mlp)))
    L.check(lib.snet_conv_plan_create(spec.tag.encode(), C.byref(plan)))
    L.check(lib.snet_fused_plan_create(plan, mlp, 4, C.byref(fplan)))
    rp, sr, wr = _dev(c['row_ptr']), _dev(c['src']), _dev(c['w_row'])
    g = _gen(9)
    x, sh, dsh, g_out = (_late(_dev(c[k]), i) for i, k in enumerate(('x', 'sh', 'dsh', 'g_out')))
    scale, S, keep = 0.25, L.stream, (mlp, plan, fplan)
    if which in ('conv_fwd', 'conv_bwd_edge_vec'):
        w = _late(_dev(torch.randn(R, wn, generator=g)), 7)
        if which == 'conv_fwd':
            out = torch.empty(N, dout, device=DEV)
            return dict(late=[x, sh, w], outs=[out], keep=keep,
                        call=lambda: L.check(lib.snet_conv_fwd(plan, _p(x[0]), _p(sh[0]), _p(w[0]), _p(wr), _p(rp), _p(sr), N, scale, _p(out), S())))
        g_w, g_xe, g_vec = torch.empty(E, wn, device=DEV), torch.empty(E, dx, device=DEV), torch.empty(E, 3, device=DEV)
        return dict(late=[x, sh, dsh, w, g_out], outs=[g_w, g_xe, g_vec], prefill=[(g_vec, torch.ones(E, 3, device=DEV))], keep=keep,
                    call=lambda: L.check(lib.snet_conv_bwd_edge_vec(plan, _p(x[0]), _p(sh[0]), _p(dsh[0]), _p(w[0]), _p(wr), _p(rp), _p(sr), N, scale,
                                                                    _p(g_out[0]), _p(g_w), _p(g_xe), _p(g_vec), S())))
    h2 = _late(_dev(torch.randn(R, 64, generator=g)), 8)
    if which == 'conv_fwd_fused':
        out = torch.empty(N, dout, device=DEV)
        return dict(late=[x, sh, h2], outs=[out], keep=keep,
                    call=lambda: L.check(lib.snet_conv_fwd_fused(fplan, _p(x[0]), _p(sh[0]), _p(h2[0]), _p(wr), _p(rp), _p(sr), N, scale, _p(out), S())))
    tile_ptr, tile_node, n_tiles = _work_list(L, lib, fplan, rp, c['row_ptr'], N, E, DEV)
    # the row maxima the fp16-operand mode bounds its products with belong to the late data: they are those of the late x / g_out
    rowmax = lambda t: tuple(v.abs().amax(1).contiguous() for v in t)   # noqa: E731
    x_max, g_max = rowmax(x), rowmax(g_out)
    g_xe, g_vec, ones3 = torch.empty(E, dx, device=DEV), torch.empty(E, 3, device=DEV), torch.ones(E, 3, device=DEV)
    keep = keep + (tile_ptr, tile_node)
    nt = n_tiles.value
    if which == 'conv_bwd_fused':
        g_h2 = torch.empty(E, 64, device=DEV)
        return dict(late=[x, sh, dsh, h2, g_out, x_max, g_max], outs=[g_xe, g_h2, g_vec], prefill=[(g_vec, ones3)], keep=keep,
                    call=lambda: L.check(lib.snet_conv_bwd_fused(fplan, _p(x[0]), _p(sh[0]), _p(dsh[0]), _p(h2[0]), _p(wr), _p(rp), _p(sr), _p(tile_ptr),
                                                                 _p(tile_node), nt, scale, _p(g_out[0]), _p(g_xe), _p(g_h2), None, None, _p(g_vec),
                                                                 _p(x_max[0]), _p(g_max[0]), S())))
    if which == 'conv_bwd_fused_tail':
        assert lib.snet_fused_plan_has_mlp_tail(fplan) == 1
        emb_e = _late(_dev(c['emb'][c['w_row'].long()]), 9)        # per directed edge
        g_emb = torch.empty(E, nb, device=DEV)
        return dict(late=[x, sh, dsh, h2, g_out, x_max, g_max, emb_e], outs=[g_xe, g_emb, g_vec],
                    prefill=[(g_vec, ones3), (g_emb, torch.ones(E, nb, device=DEV))], keep=keep,
                    call=lambda: L.check(lib.snet_conv_bwd_fused(fplan, _p(x[0]), _p(sh[0]), _p(dsh[0]), _p(h2[0]), _p(wr), _p(rp), _p(sr), _p(tile_ptr),
                                                                 _p(tile_node), nt, scale, _p(g_out[0]), _p(g_xe), None, _p(emb_e[0]), _p(g_emb),
                                                                 _p(g_vec), _p(x_max[0]), _p(g_max[0]), S())))
    h2d = _late(_dev(torch.randn(R, 64, generator=g)), 10)
    ev = torch.randn(E, 3, generator=g)
    vec = _late(_dev(ev / ev.norm(dim=1, keepdim=True) * (1.5 + 3.0 * torch.rand(E, 1, generator=g))), 11, keep_sign=True)
    return dict(late=[x, sh, dsh, h2, h2d, g_out, x_max, g_max, vec], outs=[g_xe, g_vec], prefill=[(g_vec, ones3)], keep=keep,
                call=lambda: L.check(lib.snet_conv_bwd_fused_tangent(fplan, _p(x[0]), _p(sh[0]), _p(dsh[0]), _p(h2[0]), _p(h2d[0]), _p(wr), _p(rp), _p(sr),
                                                                     _p(tile_ptr), _p(tile_node), nt, scale, _p(g_out[0]), _p(g_xe), _p(vec[0]), _p(g_vec),
                                                                     _p(x_max[0]), _p(g_max[0]), S())))


def _row_lastlayer():
    from test_lastlayer_gpu import SCALE, _problem
    L, lib = _lib()
    pr = _problem('last16_l2', True)
    spec, g, c = pr['spec'], pr['g'], pr['c']
    NT, E, dx = g['NT'], g['E'], spec.irreps_x.dim
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    X, G, H2, H2D = (_late(t(c[k]), i) for i, k in enumerate(('x', 'g_out', 'h2', 'h2d')))
    sh, dsh = _late(pr['sh'].clone(), 5), _late(pr['dsh'].clone(), 6)
    vec = _late(pr['vec'].clone(), 7, keep_sign=True)
    cp, ep, ct = t(g['col_ptr']), t(g['eperm']), t(g['center_t'])
    wrt = t(c['w_row'])[ep.long()].contiguous()
    gh, gv = torch.empty(NT + 1, dx, device=DEV), torch.empty(E + 1, 3, device=DEV)

    def call():
        L.check(lib.snet_lastlayer_conv_bwd(pr['mplan'], _p(X[0]), _p(G[0]), _p(sh[0]), _p(dsh[0]), _p(vec[0]), _p(H2[0]), _p(H2D[0]), _p(cp), _p(ct),
                                            _p(wrt), _p(ep), 0, NT, SCALE, _p(gh), _p(gv), L.stream()), 'snet_lastlayer_conv_bwd')
    return dict(late=[X, G, H2, H2D, sh, dsh, vec], outs=[gh[:NT], gv[:E]], prefill=[(gv, torch.ones(E + 1, 3, device=DEV))], call=call,
                keep=(pr, cp, ep, ct, wrt, gh, gv))


def _row_layer0():
    from test_layer0_moments_cpu import random_case
    from test_layer0_moments_gpu import DEGREES, _layer0_spec
    L, lib = _lib()
    spec = _layer0_spec('mini')
    mul, lmax = spec.irreps_x.dim, len(spec.paths) - 1
    present, n_species = (0, 2), 3
    c = random_case(mul=mul, lmax=lmax, n_species=n_species, present=present, degrees=DEGREES, n_ghost=3, seed=35, dtype=np.float32)
    N, E, Q = c['N'], c['E'], (lmax + 1) ** 2
    rng = np.random.default_rng(135)
    R = E // 2 + 3
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    wr = t(rng.integers(0, R, E).astype(np.int32))
    P = L.EdgeParams(5.0, 8, 0, 6, 0.0, lmax, 1)
    cf = (C.c_float * 8)(*[(k + 1) * np.pi / 5.0 for k in range(8)])
    vec0 = t(c['edge_vec'])
    emb, sh0, dsh0 = torch.empty(E, 8, device=DEV), torch.empty(E, Q, device=DEV), torch.empty(E, 3 * Q, device=DEV)
    L.check(lib.snet_edge_embed_fwd(C.byref(P), cf, _p(vec0), E, _p(emb), _p(sh0), _p(dsh0), None))
    torch.cuda.synchronize()
    plan, lplan = C.c_void_p(), C.c_void_p()
    L.check(lib.snet_conv_plan_create(spec.tag.encode(), C.byref(plan)))
    slot = np.zeros(n_species, np.int32)
    slot[list(present)] = np.arange(len(present), dtype=np.int32)
    table_s = np.ascontiguousarray(c['table'][list(present)])
    L.check(lib.snet_layer0_plan_create(plan, C.c_void_p(c['W2'].ctypes.data), C.c_void_p(table_s.ctypes.data), c['scale'], len(present),
                                        C.byref(lplan)), 'snet_layer0_plan_create')
    n_scr = int(lib.snet_layer0_scratch_size(lplan, N))
    scratch, gv = torch.empty(n_scr, device=DEV), torch.empty(E + 1, 3, device=DEV)
    gm = _late(t(rng.normal(0, 1, (N, Q * mul)).astype(np.float32)), 1)
    h2, h2d = _late(t(c['h2'][:R].copy()), 2), _late(t(c['h2d'][:R].copy()), 3)
    sh, dsh, vec = _late(sh0, 4), _late(dsh0, 5), _late(vec0, 6, keep_sign=True)
    rp, src, types, sl = t(c['row_ptr']), t(c['src']), t(c['types']), t(slot)

    def call():     # (two launches: the per-atom products into scratch, then the per-edge kernel that reads them)
        L.check(lib.snet_layer0_conv_bwd(lplan, _p(gm[0]), _p(h2[0]), _p(h2d[0]), _p(wr), _p(rp), _p(src), _p(types), _p(sl), _p(sh[0]), _p(dsh[0]),
                                         _p(vec[0]), N, _p(scratch), _p(gv), L.stream()), 'snet_layer0_conv_bwd')
    return dict(late=[gm, h2, h2d, sh, dsh, vec], outs=[scratch, gv[:E]], prefill=[(gv, torch.ones(E + 1, 3, device=DEV))], call=call,
                keep=(plan, lplan, wr, rp, src, types, sl, gv))


# ---- the steppers, through their Python wrappers (the docstrings' "on the current stream" lives there): systems of 1, 5, 64 atoms
SIZES = [1, 5, 64]


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(DEV)


def _f64(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)


def _here(t, seed, keep_sign=False):
    """(buffer, A, B) with the tensor `t` itself as the buffer: the state arrays of the direct tests' _DeviceState objects"""
    _, a, b = _late(t, seed, keep_sign)
    return (t, a.clone(), b)


def _ints(**kw):
    """integer state a step updates: (tensors by name, prefill list restoring them before every call)"""
    t = {k: _i32(v) for k, v in kw.items()}
    return t, [(v, v.clone()) for v in t.values()]


def _restored(*tensors):
    """prefill list that puts integer state a step updates back before every call"""
    return [(t, t.clone()) for t in tensors]


def _forces(rng, n):
    f32 = _late(torch.as_tensor(rng.normal(0, 1.0, (n, 3)).astype(np.float32)).to(DEV), 3)
    fx = _late(_f64(1e-3 * rng.normal(0, 1.0, (n, 3))), 4)
    return f32, fx


def _row_fire(cell):
    """the device state of the direct tests (test_relax_gpu / test_cell_relax_gpu ._DeviceState over the restatements' states),
    mid-run values as in test_frozen_means_frozen; their step() synchronises the device, so the wrapper is called here"""
    from sevennet_amd.relax import check_cell_params, check_fire_params, fire_cell_step, fire_step
    rng = np.random.default_rng(11)
    n = sum(SIZES)
    params = check_fire_params(0.01, 1, 0.5, {})
    f32, fx = _forces(rng, n)
    if not cell:
        import relax_ref
        from test_relax_gpu import _DeviceState
        states = [relax_ref.fire_init(rng.normal(0, 0.5, (k, 3))) for k in SIZES]
    else:
        import cellrelax_ref as ref
        from test_cell_relax_gpu import C0, F_INIT, _DeviceState
        states = [ref.cell_fire_init(rng.normal(0, 0.5, (k, 3)), C0 @ F_INIT.T, cell0=C0) for k in SIZES]
        for s_ in states:
            s_['vel_cell'] = rng.normal(0, 1e-3, (3, 3))
    for s_ in states:
        s_['vel'] = rng.normal(0, 0.01, s_['pos'].shape)
        s_['n_steps'], s_['n_pos'], s_['dt'], s_['alpha'] = 4, 2, 0.07, 0.09
    d = _DeviceState(states)
    pos, vel, dt, alpha = _here(d.pos, 1), _here(d.vel, 2), _here(d.dt, 5, True), _here(d.alpha, 6, True)
    if not cell:
        return dict(late=[pos, vel, f32, fx, dt, alpha], outs=[d.pos, d.vel, d.dt, d.alpha, d.fmax_sys],
                    prefill=_restored(d.n_pos, d.active, d.n_steps, d.n_active), keep=d,
                    call=lambda: fire_step(d.pos, d.vel, f32[0], d.seg_ptr, d.dt, d.alpha, d.n_pos, d.active, d.n_steps, d.fmax_sys, d.n_active,
                                           0.01, params, fx[0]))
    B = len(SIZES)
    cells, vel_cell = _here(d.cell, 7, True), _here(d.vel_cell, 8)
    vir, virx = _late(_f64(rng.normal(0, 1.0, (B, 6))), 9), _late(_f64(rng.normal(0, 0.02, (B, 6))), 10)
    cp = check_cell_params(**ref.CELL)
    return dict(late=[pos, vel, f32, fx, dt, alpha, cells, vel_cell, vir, virx], outs=[d.pos, d.vel, d.cell, d.vel_cell, d.fmax_sys],
                prefill=_restored(d.n_pos, d.active, d.n_steps, d.status, d.n_active), keep=d,
                call=lambda: fire_cell_step(d.pos, d.vel, d.cell, d.vel_cell, d.cell0, f32[0], vir[0], d.seg_ptr, d.dt, d.alpha, d.n_pos, d.active,
                                            d.n_steps, d.status, d.fmax_sys, d.n_active, 0.01, params, cp, 0.0, fx[0], virx[0]))


def _row_md(which):
    """the device state of test_md_batch_gpu / test_md_npt_gpu ._DeviceState over the restatements' states, one mid-run step
    (FINISH | START) with a thermostat and a second force array"""
    import md_ref
    from sevennet_amd.md import init_velocities, md_npt_step, md_step
    rng = np.random.default_rng(12)
    B, n = len(SIZES), sum(SIZES)
    masses = [rng.choice([1.008, 15.999, 28.0855], k) for k in SIZES]
    kT = md_ref.KB * np.array([100.0, 300.0, 600.0])
    c1, c2 = md_ref.langevin_coefficients(0.1, 0.5)
    phase = md_ref.FINISH | md_ref.START
    f32, fx = _forces(rng, n)
    start = [(rng.normal(0, 0.5, (k, 3)), rng.normal(0, 0.01, (k, 3))) for k in SIZES]
    if which != 'npt':
        from test_md_batch_gpu import _DeviceState
        d = _DeviceState([md_ref.md_init(p, v, step=5) for p, v in start], masses, kT)
        mass, kt = _here(d.mass, 5, True), _here(d.kT, 6, True)
        if which == 'init_velocities':
            return dict(late=[mass, kt], outs=[d.vel], keep=d, call=lambda: init_velocities(d.vel, d.mass, d.seg_ptr, d.sys_id, d.kT, 77, True))
        return dict(late=[_here(d.pos, 1), _here(d.vel, 2), f32, fx, mass, kt], outs=[d.pos, d.vel, d.e_kin], prefill=_restored(d.step_index), keep=d,
                    call=lambda: md_step(d.pos, d.vel, f32[0], d.mass, d.seg_ptr, d.sys_id, d.kT, d.step_index, d.e_kin, 0.5, c1, c2, 77, phase, fx[0]))
    import md_npt_ref as ref
    from test_md_npt_gpu import CAP, MIN_H, _DeviceState
    cells0 = [np.diag([9.0, 10.0, 11.0]) + rng.normal(0, 0.5, (3, 3)) for _ in SIZES]
    d = _DeviceState([ref.npt_init(p, c, v, step=5) for (p, v), c in zip(start, cells0)], masses, kT, np.array([0.05, -0.02, 0.1]),
                     np.array([0.02, 0.05, 0.03]))
    vir, virx = _late(_f64(rng.normal(0, 1.0, (B, 6))), 8), _late(_f64(rng.normal(0, 0.05, (B, 6))), 9)
    late = [_here(d.pos, 1), _here(d.vel, 2), f32, fx, _here(d.mass, 5, True), _here(d.kT, 6, True), _here(d.cell, 7, True), vir, virx,
            _here(d.p0, 10, True), _here(d.bt, 11, True)]
    return dict(late=late, outs=[d.pos, d.vel, d.cell, d.e_kin, d.volume, d.pressure], prefill=_restored(d.step_index, d.active, d.status), keep=d,
                call=lambda: md_npt_step(d.pos, d.vel, d.cell, f32[0], vir[0], d.mass, d.seg_ptr, d.sys_id, d.kT, d.p0, d.bt, d.step_index, d.e_kin,
                                         d.volume, d.pressure, d.active, d.status, 0.5, c1, c2, 77, phase, CAP, MIN_H, fx[0], virx[0]))


def _row_neb():
    from sevennet_amd import neb
    from test_neb_gpu import TRICLINIC, _synthetic_band
    rng = np.random.default_rng(21)
    open_ = (np.zeros((3, 3)), [False] * 3)
    bands = [_synthetic_band(rng, 1, 1, *open_), _synthetic_band(rng, 5, 3, *open_, energies=[0.0, 1.0, 2.0, 1.5, 3.0], k=0.3),
             _synthetic_band(rng, 64, 2, TRICLINIC, [True] * 3, fixed=rng.random(64) < 0.25, straddle=True)]
    B = len(bands)
    m = [b['images'].shape[0] - 2 for b in bands]
    n = [b['images'].shape[1] for b in bands]
    padded, inv = neb.mic_cells(np.stack([b['cell'] for b in bands]), np.array([b['pbc'] for b in bands]))
    fixed = _i32(np.concatenate([np.tile(np.zeros(nb, bool) if b['fixed'] is None else b['fixed'], mb) for b, mb, nb in zip(bands, m, n)]))
    N = sum(mb * nb for mb, nb in zip(m, n))
    # late: the interior images, their forces and energies (small perturbations: the order of the energies, hence the tangent
    # branches and the climbing image, may differ between A and B; no index depends on them)
    pos = _late(_f64(np.concatenate([b['images'][1:-1].reshape(-1, 3) for b in bands])), 1)
    f32 = _late(torch.as_tensor(np.concatenate([b['f32'].reshape(-1, 3) for b in bands])).to(DEV), 2)
    fx = _late(_f64(np.concatenate([b['fx'].reshape(-1, 3) for b in bands])), 3)
    en = _late(_f64(np.concatenate([b['e_model'][1:-1] for b in bands])), 4)
    ex = _late(_f64(np.concatenate([b['e_extra'][1:-1] for b in bands])), 5)
    seg_ptr, img_ptr = _i32(np.concatenate([[0], np.cumsum(np.repeat(n, m))])), _i32(np.concatenate([[0], np.cumsum(m)]))
    pos_end = _f64(np.concatenate([b['images'][[0, -1]].reshape(-1, 3) for b in bands]))
    end_ptr = _i32(np.concatenate([[0], np.cumsum(2 * np.array(n))]))
    e_end = _f64(np.array([[b['e_model'][0] + b['e_extra'][0], b['e_model'][-1] + b['e_extra'][-1]] for b in bands]))
    cells, invc, pbc = _f64(padded.reshape(B, 9)), _f64(inv.reshape(B, 9)), _i32(np.array([b['pbc'] for b in bands]))
    k = _f64([b['k'] for b in bands])
    it, pre = _ints(active=[1] * B, status=[0] * B, imax=[-7] * B)
    f_neb = torch.empty(N, 3, dtype=torch.float64, device=DEV)
    return dict(late=[pos, f32, fx, en, ex], outs=[f_neb], prefill=pre, keep=(it, fixed),
                call=lambda: neb.neb_forces(pos[0], f32[0], en[0], seg_ptr, img_ptr, pos_end, end_ptr, e_end, cells, invc, pbc, k, it['active'],
                                            it['status'], f_neb, it['imax'], climb=True, forces_extra=fx[0], energy_extra=ex[0], fixed=fixed))


def _row_vib(which):
    """the kernel case of test_vib_gpu (systems of 1, 5, 300 and 64 atoms, nfree = 2): its copies, forces, masses and selections"""
    from sevennet_amd.vib import vib_displace, vib_finish, vib_rows
    from test_vib_gpu import DELTA, KERNEL_N, _kernel_case
    case = _kernel_case(2)
    B = len(KERNEL_N)
    m = np.array([len(s_) for s_ in case.sel])
    d_off = np.concatenate([[0], np.cumsum(9 * m * m)])
    sel_ptr, off_d = _i32(np.concatenate([[0], np.cumsum(m)])), torch.as_tensor(d_off[:-1], dtype=torch.int64).to(DEV)
    cptr = _i32(case.copy_ptr)
    if which == 'displace':
        pos0 = _late(_f64(np.concatenate(case.pos0)), 1)
        it, pre = _ints(status=[0] * len(case.call.desc))
        pos = torch.empty(case.N, 3, dtype=torch.float64, device=DEV)
        seg0, desc = _i32(np.concatenate([[0], np.cumsum(case.n)])), _i32(case.call.desc)
        return dict(late=[pos0], outs=[pos], prefill=pre, keep=it, call=lambda: vib_displace(pos0[0], seg0, desc, cptr, DELTA, pos, it['status']))
    it, pre = _ints(status=[0] * B)
    D = torch.empty(int(d_off[-1]), dtype=torch.float64, device=DEV)
    if which == 'rows':
        f32, fx = _late(torch.as_tensor(case.f32).to(DEV), 2), _late(_f64(case.fx), 3)
        groups, selc = _i32(case.call.groups), _i32(np.concatenate(case.sel))
        return dict(late=[f32, fx], outs=[D], prefill=pre, keep=it,
                    call=lambda: vib_rows(f32[0], fx[0], cptr, groups, case.nfree, DELTA, selc, sel_ptr, off_d, D, it['status']))
    Din = _late(_f64(np.random.default_rng(4).normal(0.0, 1.0, int(d_off[-1]))), 4)
    w = _late(_f64(np.concatenate([1.0 / np.sqrt(ms[s_]) for ms, s_ in zip(case.masses, case.sel)])), 5, keep_sign=True)
    H, Hm, asym = torch.empty_like(D), torch.empty_like(D), torch.empty(B, dtype=torch.float64, device=DEV)
    return dict(late=[Din, w], outs=[H, Hm, asym], prefill=pre, keep=it,
                call=lambda: vib_finish(Din[0], off_d, sel_ptr, w[0], it['status'], H, Hm, asym))


TABLE = {
    'snet_gemm': lambda: _row_gemm(None),
    'snet_gemm_grouped[fp32]': lambda: _row_gemm(False),
    'snet_gemm_grouped[packed]': lambda: _row_gemm(True),
    'snet_gate_fwd[addend]': lambda: _row_gate('fwd_addend'),
    'snet_gate_bwd_norm[16-byte]': lambda: _row_gate('bwd_norm_vec'),
    'snet_gate_bwd_norm[scalar, two launches]': lambda: _row_gate('bwd_norm_scalar'),
    'snet_segment_sum_rows': lambda: _row_node('segment_sum_rows'),
    'snet_segment_sum_rows_chunked': lambda: _row_node('segment_sum_rows_chunked'),
    'snet_row_absmax_multi': lambda: _row_node('row_absmax_multi'),
    'snet_row_norm2': lambda: _row_node('row_norm2'),
    'snet_edge_embed_fwd': lambda: _row_edge('fwd'),
    'snet_edge_embed_bwd': lambda: _row_edge('bwd'),
    'snet_edge_embed_tangent': lambda: _row_edge('tangent'),
    'snet_radial_mlp_fwd': lambda: _row_mlp('fwd'),
    'snet_radial_mlp_bwd': lambda: _row_mlp('bwd'),
    'snet_radial_mlp_hidden_fwd': lambda: _row_mlp('hidden_fwd'),
    'snet_radial_mlp_hidden_bwd': lambda: _row_mlp('hidden_bwd'),
    'snet_conv_fwd': lambda: _row_conv('conv_fwd'),
    'snet_conv_bwd_edge_vec': lambda: _row_conv('conv_bwd_edge_vec'),
    'snet_conv_fwd_fused': lambda: _row_conv('conv_fwd_fused'),
    'snet_conv_bwd_fused': lambda: _row_conv('conv_bwd_fused'),
    'snet_conv_bwd_fused[mlp tail]': lambda: _row_conv('conv_bwd_fused_tail'),
    'snet_conv_bwd_fused_tangent': lambda: _row_conv('conv_bwd_fused_tangent'),
    'snet_lastlayer_conv_bwd[last16_l2]': _row_lastlayer,
    'snet_layer0_conv_bwd[mini, two launches]': _row_layer0,
    'fire_step': lambda: _row_fire(False),
    'fire_cell_step': lambda: _row_fire(True),
    'md_step': lambda: _row_md('step'),
    'md_npt_step': lambda: _row_md('npt'),
    'init_velocities': lambda: _row_md('init_velocities'),
    'neb_forces': _row_neb,
    'vib_displace': lambda: _row_vib('displace'),
    'vib_rows': lambda: _row_vib('rows'),
    'vib_finish': lambda: _row_vib('finish'),
}


@pytest.mark.parametrize('name', list(TABLE))
def test_entry_point_on_a_delayed_stream(name):
    """one row of the table: detectable (A and B differ in every compared output), repeatable on the default stream, pending when
    the call returns, and bit for bit the default stream's result (all four asserted by stream_order.run_ab)"""
    row = TABLE[name]()
    torch.cuda.synchronize()        # index arrays, plans and staged values are complete before the delayed section
    run_ab(name, row['late'], row['call'], row['outs'], row.get('prefill', ()))
