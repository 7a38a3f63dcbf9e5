"""CPU: the conditions the mixed-magnitude GPU tests (tests/test_fused_range_gpu.py) rest on -- the exponent tables really put
edges of different magnitude into one 16-edge tile -- and the fp64 reference's scaling shortcut."""
import torch

import fused_range as fr
from test_ops_gpu import _fused_case


def test_magnitude_tables_mix_inside_tiles():
    """with the tables of fused_range.py on `_fused_case`'s degrees the packed work list has single-row tiles, two-row tiles whose
    rows share the g_out exponent and two-row tiles whose rows differ by each of 12, 20 and 32; the source-row and radial-row
    exponents mix inside tiles of either work-list format.  A condition of the GPU test, not a measurement."""
    c = _fused_case('sevennet_0', 1, 41, True)
    ex = fr.axis_exponents(c, 'pqr')
    node, src, rows = fr.edge_maps(c)
    e0, nodes = fr.work_list(c['row_ptr'], c['N'], 1)
    cls, gap = fr.tile_classes(nodes, ex['p'])
    counts = [int((cls == k).sum()) for k in range(3)]
    assert counts == [36, 7, 16], counts
    assert set(gap[cls == 2].tolist()) == {12, 20, 32}
    for mode in (0, 1):
        e0, nodes = fr.work_list(c['row_ptr'], c['N'], mode)
        tile = fr.tile_of_edge(e0)
        nt = e0.numel() - 1
        assert tile.numel() == c['E'] and int(tile.max()) == nt - 1
        if mode == 0:
            assert bool((fr.tile_classes(nodes, ex['p'])[0] == 0).all())
        for own, table in ((ex['q'][src], fr.Q_TAB), (ex['r'][rows], fr.R_TAB), (ex['rd'][rows], fr.RD_TAB)):
            hi = torch.full((nt,), -99).scatter_reduce(0, tile, own, 'amax')
            lo = torch.full((nt,), 99).scatter_reduce(0, tile, own, 'amin')
            spread = max(table) - min(table)
            assert int((hi - lo == spread).sum()) > 0       # the full spread of the table inside one tile
            k = fr.bound_exponent(own, tile, nt)
            assert bool((k == own).any()) and bool((k > own).any())   # edges inside and outside the documented window
    # the bound rule itself, on a hand-made tile: exponents 0, -12, -13 under a largest exponent of 0
    k = fr.bound_exponent(torch.tensor([0, -12, -13, 5]), torch.tensor([0, 0, 0, 1]), 2)
    assert k.tolist() == [0, -12, 0, 5]


def test_scaled_reference_equals_reference_of_scaled_inputs():
    """fused_range.scaled_reference (unit-scale reference times the factors) == fused_range.fused_reference on the scaled inputs,
    to fp64 rounding, all three axes at once and with a zeroed source row and g_out row"""
    c = _fused_case('sevennet_0', 0, 40, False)
    g = torch.Generator().manual_seed(1)
    h2, h2d = fr.hidden_layers(c['emb'], torch.randn(c['R'], c['nb'], generator=g), c['W0'], c['W1'])
    h2, h2d = h2.float(), h2d.float()
    args = lambda x, h, hd, go: (c['spec'], x, c['sh'], c['dsh'], h, c['W2'], c['w_row'], c['row_ptr'], c['src'], 0.25, go, hd)  # noqa: E731
    ref = fr.fused_reference(*args(c['x'], h2, h2d, c['g_out']))
    ex = fr.axis_exponents(c, 'pqr')
    fg, fx, fh, fhd = (2.0 ** ex[k].double() for k in ('p', 'q', 'r', 'rd'))
    fg[8], fx[3] = 0.0, 0.0
    want = fr.fused_reference(*args(c['x'] * fx[:, None].float(), h2 * fh[:, None].float(), h2d * fhd[:, None].float(),
                                    c['g_out'] * fg[:, None].float()))
    got = fr.scaled_reference(ref, c, fg, fx, fh, fhd)
    for k in ('out', 'g_xe', 'g_h2', 'g_vec', 'g_rad'):
        # row-wise: every row of the two agrees to fp64 rounding of ITS OWN magnitude (the rows span 2^-47 .. 2^28)
        a, b = got[k].reshape(got[k].shape[0], -1), want[k].reshape(want[k].shape[0], -1)
        assert a.shape == b.shape
        assert bool(((a - b).abs().amax(1) <= 1e-12 * b.abs().amax(1)).all()), k
