"""The fp64 reference of the uvu convolution for ANY ConvSpec of the catalogue (sevennet_amd.shapes.aot_conv_specs), the shared test case
and the comparison rule of the catalogue sweep.  CPU only: oracle.model.tp_uvu + autograd on engine (ir_mul) rows; nothing here comes
from a GPU kernel.  Used by tests/fused_range.py (fused_reference), tests/test_ops_gpu.py (_mid_index), tests/test_conv_shapes_cpu.py
and tests/test_conv_shapes_gpu.py.

A path's place in the output comes from path.out_off / path.out_ch, never from its rank among the paths: a spec may keep blocks in
irreps_mid / irreps_out that no path writes (model_spec.prune_unread_paths keeps the layout of MF-ompa's third layer and drops 34 of
its 68 paths; a transposed last-layer shape keeps source blocks that no path reads)."""
import functools

import torch

DEGREES = (0, 1, 2, 15, 16, 17, 33, 65, 0)   # rows without edges at both ends, rows that share a packed 16-edge tile, one-off around
N_GHOST = 3                                  # one and two tiles, one row past a wavefront: 149 edges; 3 ghost rows (sources only)
SCALE = 0.25
NB = 8
CST = 1.6791767923989418     # normalize2mom constant of silu
TOL_FUSED = 2e-5             # fused_range.TOL: what test_conv_fused_matches_separate_kernels grants terms = 4 and 3
TOL_SEPARATE = 3e-5          # test_conv_plugin_vs_oracle_autograd


def catalogue():
    """tag -> ConvSpec of every shape the build ships, in build order: what the sweep is parametrised over"""
    from sevennet_amd.shapes import aot_conv_specs
    return aot_conv_specs()


def fusable(spec):
    """the shapes codegen_fused.py generates fused kernels for: every multiplicity a multiple of 16"""
    return all(mul % 16 == 0 for mul, _, _ in spec.irreps_x)


def mid_layout(spec):
    """per irreps_mid block: (offset of its merged irreps_out block, multiplicity of that block, channel offset inside it), by the
    rule make_conv merges with: consecutive blocks of one irrep fill one merged block until it is full"""
    mid, merged = list(spec.irreps_mid), list(spec.irreps_out)
    assert spec.irreps_mid.dim == spec.irreps_out.dim
    m_off = spec.irreps_out.offsets()
    where, cur, ch = [], -1, 0
    for mul, l, p in mid:
        if cur < 0 or (merged[cur][1], merged[cur][2]) != (l, p) or ch + mul > merged[cur][0]:
            assert cur < 0 or ch == merged[cur][0], 'irreps_mid does not fill irreps_out block by block'
            cur, ch = cur + 1, 0
        assert (merged[cur][1], merged[cur][2]) == (l, p)
        where.append((m_off[cur], merged[cur][0], ch))
        ch += mul
    assert cur == len(merged) - 1 and ch == merged[cur][0]
    return where


def mid_index(spec):
    """index of each path's block inside irreps_mid, from the path's own out_off / out_ch"""
    at = {(off, ch): k for k, (off, _, ch) in enumerate(mid_layout(spec))}
    idx = [at[(p.out_off, p.out_ch)] for p in spec.paths]
    assert len(set(idx)) == len(idx)
    for p, k in zip(spec.paths, idx):
        assert (spec.irreps_mid[k][0], spec.irreps_mid[k][1]) == (p.mul, p.l3)
    return idx


def written_mask(spec):
    """bool[dout]: the columns of an engine (ir_mul) output row that some path writes"""
    mask = torch.zeros(spec.irreps_out.dim, dtype=torch.bool)
    for p in spec.paths:
        for a in range(2 * p.l3 + 1):
            o = p.out_off + a * p.out_mul + p.out_ch
            mask[o:o + p.mul] = True
    return mask


def unwritten_ranges(spec):
    """[(begin, end)] column ranges of an engine output row that no path writes"""
    m = written_mask(spec).tolist()
    out, c = [], 0
    while c < len(m):
        if m[c]:
            c += 1
            continue
        b = c
        while c < len(m) and not m[c]:
            c += 1
        out.append((b, c))
    return out


def conv_reference(spec, x, sh, dsh, w_row, row_ptr, src, scale, g_out, h2=None, W2=None, w=None, h2d=None, dtype=torch.float64):
    """Reference of the convolution on engine (ir_mul) rows in `dtype` (fp64: the truth; fp32: the arithmetic class the kernels
    replace): per-edge weights w_e = w[w_row[e]] (given) or h2[w_row[e]] W2 -> uvu tensor product -> segment sum over destination
    rows, and its gradients by autograd.  Returns
      out[N, dout], msg[E, dout] (out = their sum per destination row), g_w[E, wn], g_xe[E, dx], g_x[NT, dx] (g_xe summed per
      source), g_sh[E, nsh] = dE/dY including Y_0, g_vec[E, 3] = dE/dY . dsh without Y_0 (constant: its Jacobian row is not read),
      unwritten = the column ranges of out that no path writes (zero here),
      and with h2 / W2: g_h2[E, 64] = g_w W2^T; with h2d also g_rad[E] = sum_k g_w[e, k] (h2' W2)[k]."""
    from oracle.e3 import Irreps as OIrreps
    from oracle.model import tp_uvu
    from sevennet_amd.irreps import Irreps, irmul_to_mulir_index, mulir_to_irmul_index
    N, E, NT, nsh = row_ptr.numel() - 1, src.numel(), x.shape[0], sh.shape[1]
    node = torch.repeat_interleave(torch.arange(N), (row_ptr[1:] - row_ptr[:-1]).long())
    rows = torch.arange(E) if w_row is None else w_row.long()
    from_x = torch.as_tensor(irmul_to_mulir_index(spec.irreps_x))
    to_o = torch.as_tensor(mulir_to_irmul_index(spec.irreps_out))
    xe = x.to(dtype)[src.long()].clone().requires_grad_(True)
    she = sh.to(dtype).clone().requires_grad_(True)
    if w is not None:
        assert h2 is None
        we = w.to(dtype)[rows].clone().requires_grad_(True)
    else:
        W2 = W2.to(dtype)
        h2e = h2.to(dtype)[rows].clone().requires_grad_(True)
        we = h2e @ W2
        we.retain_grad()
    assert we.shape[1] == spec.weight_numel
    # the oracle wants one irreps_mid block per instruction: hand it the blocks that have a path, and put its columns where the
    # full irreps_mid has them (mul_ir: blocks in order, each [mul][2l + 1])
    idx = mid_index(spec)
    live = sorted(idx)
    sub = Irreps([spec.irreps_mid[k] for k in live])
    ins, o = [], 0
    for p, k in zip(spec.paths, idx):
        assert p.w_off == o, 'weight columns follow the path order'
        o += p.mul
        ins.append((p.i_x, p.i_sh, live.index(k)))
    part = tp_uvu(xe[:, from_x], she, we, OIrreps(str(spec.irreps_x)), OIrreps(str(spec.irreps_sh)), OIrreps(str(sub)), ins)
    offs = spec.irreps_mid.offsets()
    cols = torch.cat([torch.arange(offs[k], offs[k] + spec.irreps_mid[k][0] * (2 * spec.irreps_mid[k][1] + 1)) for k in live])
    msg = torch.zeros(E, spec.irreps_out.dim, dtype=dtype).index_add(1, cols, part)[:, to_o] * scale
    out = torch.zeros(N, msg.shape[1], dtype=dtype).index_add_(0, node, msg)
    (out * g_out.to(dtype)).sum().backward()
    g_sh = she.grad
    res = dict(out=out.detach(), msg=msg.detach(), g_w=we.grad, g_xe=xe.grad, g_sh=g_sh,
               g_x=torch.zeros(NT, x.shape[1], dtype=dtype).index_add_(0, src.long(), xe.grad),
               g_vec=torch.einsum('ei,eia->ea', g_sh[:, 1:], dsh.to(dtype).reshape(E, nsh, 3)[:, 1:]),
               unwritten=unwritten_ranges(spec))
    if w is None:
        res['g_h2'] = h2e.grad
        if h2d is not None:
            res['g_rad'] = (we.grad * (h2d.to(dtype)[rows] @ W2)).sum(1)
    return res


def shape_case(spec, seed, pairs):
    """the sweep's inputs for one shape: DEGREES, ghost source rows, optional pair-shared radial rows in scrambled order, seeded
    randn inputs as test_ops_gpu._fused_case draws them; the radial rows h2 / h2' are the fp64 hidden layers rounded to fp32 (the
    kernels' inputs: the reference takes the fp32 values as given), w = fp32(h2 W2) the separate kernels' weight rows.  g_out is
    zero on the columns that no path writes."""
    import fused_range as fr
    nb, wn, dx, dout, nsh = NB, spec.weight_numel, spec.irreps_x.dim, spec.irreps_out.dim, spec.irreps_sh.dim
    g = torch.Generator().manual_seed(seed)
    deg = torch.tensor(DEGREES)
    N = len(deg)
    row_ptr = torch.zeros(N + 1, dtype=torch.int32)
    row_ptr[1:] = torch.cumsum(deg, 0)
    E = int(row_ptr[-1])
    NT = N + N_GHOST
    src = torch.randint(0, NT, (E,), generator=g).to(torch.int32)
    R, w_row = E, None
    if pairs:
        R = E // 2 + 3
        w_row = torch.randint(0, R, (E,), generator=g).to(torch.int32)
    c = dict(spec=spec, nb=nb, wn=wn, dx=dx, dout=dout, nsh=nsh, N=N, NT=NT, E=E, R=R, row_ptr=row_ptr, src=src, w_row=w_row,
             x=torch.randn(NT, dx, generator=g), sh=torch.randn(E, nsh, generator=g), dsh=torch.randn(E, nsh * 3, generator=g),
             emb=torch.randn(R, nb, generator=g), g_out=torch.randn(N, dout, generator=g),
             W0=(torch.randn(nb, 64, generator=g) / nb ** 0.5).contiguous(), W1=(torch.randn(64, 64, generator=g) / 8).contiguous(),
             W2=(torch.randn(64, wn, generator=g) / 8).contiguous())
    c['demb'] = torch.randn(R, nb, generator=g)
    c['vec'] = torch.randn(E, 3, generator=g)
    c['written'] = written_mask(spec)
    c['g_out'][:, ~c['written']] = 0.0
    h2, h2d = fr.hidden_layers(c['emb'], c['demb'], c['W0'], c['W1'])
    c['h2'], c['h2d'] = h2.float().contiguous(), h2d.float().contiguous()
    c['w'] = (c['h2'].double() @ c['W2'].double()).float().contiguous()
    return c


def case_args(c):
    return dict(x=c['x'], sh=c['sh'], dsh=c['dsh'], w_row=c['w_row'], row_ptr=c['row_ptr'], src=c['src'], scale=SCALE, g_out=c['g_out'])


@functools.lru_cache(maxsize=4)
def tag_case(tag, pairs):
    """(inputs, fp64 reference of the separate kernels on the fp32 weight rows w, fp64 reference of the fused kernels on h2 / W2),
    computed once per shape and shared, never modified"""
    spec = catalogue()[tag]
    c = shape_case(spec, 1000 + sorted(catalogue()).index(tag), pairs)
    return c, conv_reference(spec, w=c['w'], **case_args(c)), conv_reference(spec, h2=c['h2'], W2=c['W2'], h2d=c['h2d'], **case_args(c))


def bar(tol, ref, floor=1.0):
    """the project's bar of one output: tol x max(floor, largest reference entry)"""
    return tol * max(floor, ref.abs().max().item())


def judge(got, ref, tol, floor=1.0, mask=None):
    """one output against its bar: |got - ref| <= tol max(floor, max|ref|), finite -- on the columns of `mask` (the bar's scale is
    taken there too).  Returns (holds, error / bar)."""
    g, r = got.double(), ref.double()
    if mask is not None:
        g, r = g[..., mask], r[..., mask]
    if not bool(torch.isfinite(g).all()):
        return False, float('inf')
    err, b = (g - r).abs().max().item(), bar(tol, r, floor)
    return err <= b, err / b
