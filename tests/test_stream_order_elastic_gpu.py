"""GPU: the stream contract for the elastic entry points -- one stream_order.run_ab row each for snet_el_strain, snet_el_rows (both
stencils) and snet_el_finish: late floating-point inputs behind a delay on a non-default stream, the outputs bit for bit those of the default
stream.  The case is the kernel case of test_elastic_gpu (three systems, n = 1, 5 and 300).

The whole-call check of `elastic_many` (stream_order.run_whole) is left out: the call reads values back, so it would have to be
named in the helper's READS_BACK table, and the helper is an existing file that this test only imports.

Each row takes one stream from torch's pool, and this file runs before test_stream_order_ops_gpu.py, whose control
(test_control_stray_second_launch_reads_the_kept_intermediate) needs its stray NULL-stream launch to overtake the delayed stream:
that holds only while the two do not share one of the process's four hardware queues, which depends on how many streams were
taken before it.  With three rows here the control stopped losing its race in a run of the whole suite; with four (a multiple
of the queue count) it behaves as it did without this file."""
import numpy as np
import pytest
import torch

from stream_order import run_ab
from test_stream_order_ops_gpu import DEV, _f64, _i32, _ints, _late

pytestmark = pytest.mark.gpu


def _case(nfree=4):
    from test_elastic_gpu import B, DELTA, _kernel_case
    case = _kernel_case(nfree)
    return case, _i32(np.concatenate([[0], np.cumsum(case.n)])), B, DELTA


def _row_strain():
    from sevennet_amd.elastic import el_strain
    case, a_ptr, _, delta = _case()
    pos0 = _late(_f64(np.concatenate(case.pos0)), 2)
    desc, cptr = _i32(case.call.desc), _i32(case.copy_ptr)
    it, pre = _ints(status=[0] * len(case.call.desc))
    out = torch.empty(case.N, 3, dtype=torch.float64, device=DEV)
    return dict(late=[pos0], outs=[out], prefill=pre, keep=it, call=lambda: el_strain(pos0[0], a_ptr, desc, cptr, delta, out, it['status']))


def _row_rows(nfree):
    from sevennet_amd.elastic import el_rows
    case, a_ptr, B, delta = _case(nfree)
    virial, vx = _late(_f64(case.virial), 3), _late(_f64(case.vx), 4)
    volume = _late(_f64(case.volume), 5, keep_sign=True)   # (a volume stays positive: a relative perturbation only)
    f32, fx = _late(torch.as_tensor(case.f32).to(DEV), 6), _late(_f64(case.fx), 7)
    cptr, groups = _i32(case.copy_ptr), _i32(case.call.groups)
    it, pre = _ints(status=[0] * B)
    S = torch.empty(36 * B, dtype=torch.float64, device=DEV)
    L = torch.empty(18 * int(case.n.sum()), dtype=torch.float64, device=DEV)
    return dict(late=[virial, vx, volume, f32, fx], outs=[S, L], prefill=pre, keep=it,
                call=lambda: el_rows(virial[0], vx[0], volume[0], f32[0], fx[0], cptr, groups, case.nfree, delta, a_ptr, S, L, it['status']))


def _row_finish():
    from sevennet_amd.elastic import el_finish
    _, _, B, _ = _case()
    S = _late(_f64(np.random.default_rng(9).normal(0.0, 1.0, 36 * B)), 8)
    it, pre = _ints(status=[0] * B)
    C, asym = torch.empty(36 * B, dtype=torch.float64, device=DEV), torch.empty(B, dtype=torch.float64, device=DEV)
    return dict(late=[S], outs=[C, asym], prefill=pre, keep=it, call=lambda: el_finish(S[0], it['status'], C, asym))


TABLE = {'el_strain': _row_strain, 'el_rows[nfree 2]': lambda: _row_rows(2), 'el_rows[nfree 4]': lambda: _row_rows(4), 'el_finish': _row_finish}   # (both stencils of the rows kernel)


@pytest.mark.parametrize('name', list(TABLE))
def test_entry_point_on_a_delayed_stream(name):
    """one row of the table: detectable (A and B differ in every compared output), repeatable on the default stream, pending when
    the call returns, and bit for bit the default stream's result (all four asserted by stream_order.run_ab)"""
    row = TABLE[name]()
    torch.cuda.synchronize()        # index arrays and staged values are complete before the delayed section
    run_ab(name, row['late'], row['call'], row['outs'], row.get('prefill', ()))
