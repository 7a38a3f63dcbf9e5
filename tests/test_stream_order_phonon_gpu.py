"""GPU: the stream contract for the phonon entry points -- one stream_order.run_ab row each for snet_ph_rows, snet_ph_finish,
snet_ph_images and snet_ph_dynmat (two launches): late floating-point inputs behind a delay on a non-default stream, the outputs bit
for bit those of the default stream.  The cases are the kernel cases of test_phonon_gpu (five systems, N = 1 .. 300).

The whole-call check of `phonons_many` (stream_order.run_whole) is left out: the call reads values back, so it would have to be
named in the helper's READS_BACK table, and the helper is an existing file that this test only imports."""
import numpy as np
import pytest
import torch

from stream_order import run_ab
from test_stream_order_ops_gpu import DEV, _f64, _i32, _ints, _late

pytestmark = pytest.mark.gpu


def _case():
    from test_phonon_gpu import B, _kernel_case, _structures
    case = _kernel_case(2)
    pos, S = _structures(0.0)   # the exact lattices: equally near images, masks of more than one bit
    return case, case.lay, pos, S, B


def _row_rows():
    from sevennet_amd.phonon import ph_rows
    from test_phonon_gpu import DELTA
    case, lay, _, _, B = _case()
    f32, fx = _late(torch.as_tensor(case.f32).to(DEV), 2), _late(_f64(case.fx), 3)
    it, pre = _ints(status=[0] * B)
    phi = torch.empty(int(lay.p_off[-1]), dtype=torch.float64, device=DEV)
    cptr, groups = _i32(case.copy_ptr), _i32(case.call.groups)
    return dict(late=[f32, fx], outs=[phi], prefill=pre, keep=it,
                call=lambda: ph_rows(f32[0], fx[0], cptr, groups, case.nfree, DELTA, lay.m_ptr, lay.sc_ptr, lay.off_d, phi, it['status']))


def _row_finish():
    from sevennet_amd.phonon import ph_finish
    case, lay, _, _, B = _case()
    phi = _late(_f64(np.random.default_rng(4).normal(0.0, 1.0, int(lay.p_off[-1]))), 4)
    it, pre = _ints(status=[0] * B)
    out, asr = torch.empty_like(phi[0]), torch.empty(B, dtype=torch.float64, device=DEV)
    return dict(late=[phi], outs=[out, asr], prefill=pre, keep=it,
                call=lambda: ph_finish(phi[0], lay.off_d, lay.m_ptr, lay.sc_ptr, True, it['status'], out, asr))


def _image_inputs(pos, S, B):
    return (_f64(np.stack(S).reshape(B, 9)), _f64(np.stack([np.linalg.inv(s) for s in S]).reshape(B, 9)))


def _row_images():
    """the outputs are integers: they are reset by the prefill and handed to the comparison as fp64 copies made on the call's stream"""
    from sevennet_amd.phonon import ph_images
    case, lay, pos, S, B = _case()
    pos_l = _late(_f64(np.concatenate(pos)), 5)
    S_d, Si_d = _image_inputs(pos, S, B)
    n_pairs = int(lay.i_off[-1])
    it, pre = _ints(status=[0] * B, base=np.full((n_pairs, 3), -77), mask=np.full(n_pairs, -77))

    def call():
        ph_images(pos_l[0], lay.sc_ptr, lay.m_ptr, lay.home_sys, S_d, Si_d, lay.ioff_d, 1e-5, it['base'], it['mask'], it['status'])
        return [it['base'].double(), it['mask'].double()]
    return dict(late=[pos_l], outs=None, prefill=pre, keep=it, call=call)


def _row_dynmat():
    from sevennet_amd.phonon import ph_dynmat, ph_images
    from test_phonon_gpu import KERNEL_NQ, KERNEL_SYSTEMS, _q_points
    import phonon_ref
    case, lay, pos, S, B = _case()
    pos_d = _f64(np.concatenate(pos))
    S_d, Si_d = _image_inputs(pos, S, B)
    n_pairs = int(lay.i_off[-1])
    base, mask = torch.empty(n_pairs, 3, dtype=torch.int32, device=DEV), torch.empty(n_pairs, dtype=torch.int32, device=DEV)
    it, pre = _ints(status=[0] * B)
    ph_images(pos_d, lay.sc_ptr, lay.m_ptr, lay.home_sys, S_d, Si_d, lay.ioff_d, 1e-5, base, mask, it['status'])
    torch.cuda.synchronize()
    assert not it['status'].any()
    n_q = np.array(KERNEL_NQ, np.int64)
    blocks = np.concatenate([[0], np.cumsum(n_q * 9 * lay.m * lay.m)])
    phi = _late(_f64(np.random.default_rng(6).normal(0.0, 1.0, int(lay.p_off[-1]))), 6)
    w = _late(_f64(np.concatenate([1.0 / np.sqrt(ms) for ms in case.masses])), 7, keep_sign=True)
    q = _late(_f64(np.concatenate([phonon_ref.q_cartesian(x, KERNEL_SYSTEMS[b][2]) for b, x in enumerate(_q_points())])), 8)
    q_sys, q_ptr, d_off = _i32(np.repeat(np.arange(B), n_q)), _i32(np.concatenate([[0], np.cumsum(n_q)])), torch.as_tensor(blocks[:-1]).to(DEV)
    R = torch.empty(int(blocks[-1]), 2, dtype=torch.float64, device=DEV)
    D, herm = torch.empty_like(R), torch.empty(int(n_q.sum()), dtype=torch.float64, device=DEV)
    return dict(late=[phi, w, q], outs=[R, D, herm], prefill=pre, keep=(it, base, mask),
                call=lambda: ph_dynmat(phi[0], lay.off_d, pos_d, lay.sc_ptr, lay.m_ptr, w[0], S_d, base, mask, lay.ioff_d, q[0], q_sys, q_ptr, d_off,
                                       int(lay.m.max()), it['status'], R, D, herm))


TABLE = {'ph_rows': _row_rows, 'ph_finish': _row_finish, 'ph_images': _row_images, 'ph_dynmat[two launches]': _row_dynmat}


@pytest.mark.parametrize('name', list(TABLE))
def test_entry_point_on_a_delayed_stream(name):
    """one row of the table: detectable (A and B differ in every compared output), repeatable on the default stream, pending when
    the call returns, and bit for bit the default stream's result (all four asserted by stream_order.run_ab)"""
    row = TABLE[name]()
    torch.cuda.synchronize()        # index arrays and staged values are complete before the delayed section
    run_ab(name, row['late'], row['call'], row['outs'], row.get('prefill', ()))
