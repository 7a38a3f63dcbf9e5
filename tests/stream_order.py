"""Late inputs behind a delay: the harness of tests/test_stream_order_*_gpu.py (a helper module, not a conftest).

The stream contract says that all device work of a call is ordered on the caller's current stream.  On the legacy
default stream a launch that lands on another stream is harmless; on a stream made by torch.cuda.Stream() (non-blocking) it is a
race.  The race is made to lose deterministically:

  1. the input buffers hold values A, fully synchronised; a second set B is staged on the device;
  2. a fresh stream s starts with a delay kernel (torch.cuda._sleep, calibrated once per session);
  3. behind the delay, on s, the buffers are overwritten with B and the call under test is made inside torch.cuda.stream(s),
     its outputs pre-filled with NaN;
  4. after s.synchronize() the outputs must be torch.equal to those of the same call on the default stream with inputs B.

Whatever the library put on another stream runs while s still sleeps: it reads A, or an output nobody has written yet.
Only floating-point data is late: index and topology arrays are built and synchronised before, so a misordered reader can see
stale numbers but never a stale index."""
import time

import torch

MIN_DELAY_MS = 50.0
DELAY_FACTOR = 3.0      # launch overhead jitters: the delay is this many times the measured host time of the call

# calls that read a value back inside (and so wait for the stream, delay included): exempt from the pending assertion ONLY
READS_BACK = {
    'compute_many': 'builds its graph from host structures and returns host arrays',
    'D3Calculator.compute_many': 'returns host arrays',
    'md_many': 'edge counts per rebuild, host results',
    'md_many(pressure)': 'edge counts per rebuild, host results',
    'relax_many': 'one .item() per step (convergence), edge counts per rebuild',
    'neb_many': 'one .item() per step (convergence), edge counts per rebuild',
    'vibrations_many': 'edge counts per displaced batch, host Hessians',
    'SevenNetModel.forward': 'graph construction reads the edge count back',
    'BatchForces': 'edge count of the neighbour list',
}

_cycles_per_ms = None
_matmul = None          # fallback delay where torch.cuda._sleep is missing: (operand, result, ms per product)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cycles_per_ms():
    """torch.cuda._sleep counts device clock ticks: ticks per millisecond, measured once per session with two events"""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda._sleep(1000)          # (first launch: module load)
        n = 20_000_000
        ms = _timed(lambda: torch.cuda._sleep(n))
        assert ms > 0.5, f'torch.cuda._sleep({n}) took {ms} ms: not a usable delay'
        _cycles_per_ms = n / ms
        print(f'[stream_order] torch.cuda._sleep: {_cycles_per_ms:.0f} ticks / ms ({n} ticks = {ms:.2f} ms)', flush=True)
    return _cycles_per_ms


def _matmul_ms():
    """the fallback: a chain of 4096 x 4096 products into one result buffer, milliseconds per product measured once per session"""
    global _matmul
    if _matmul is None:
        x = torch.randn(4096, 4096, device='cuda')
        y = torch.empty_like(x)
        torch.mm(x, x, out=y)
        ms = _timed(lambda: [torch.mm(x, x, out=y) for _ in range(20)]) / 20
        assert ms > 0.05, f'a 4096 x 4096 product took {ms} ms: not a usable delay'
        _matmul = (x, y, ms)
        print(f'[stream_order] no torch.cuda._sleep: delaying with 4096 x 4096 products of {ms:.3f} ms each', flush=True)
    return _matmul


def _delay(ms):
    """enqueue a bounded delay of `ms` milliseconds on the current stream"""
    if not hasattr(torch.cuda, '_sleep'):
        x, y, each = _matmul_ms()
        for _ in range(int(ms / each) + 1):
            torch.mm(x, x, out=y)
        return
    left = int(ms * cycles_per_ms())
    while left > 0:                      # (pieces of at most 1 s keep any one kernel short)
        n = min(left, int(1000 * cycles_per_ms()))
        torch.cuda._sleep(n)
        left -= n


def delayed_stream(min_ms):
    """a fresh non-blocking stream whose first work item is a delay of at least `min_ms` (and MIN_DELAY_MS)"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _delay(max(min_ms, MIN_DELAY_MS))
    return s


def late_copy(s, late, which):
    """behind whatever `s` holds: overwrite every late buffer with its staged value (`late`: [(buffer, A, B)], which: 1 = A, 2 = B)"""
    with torch.cuda.stream(s):
        for item in late:
            item[0].copy_(item[which])


def assert_pending(s, name):
    """the delay still runs when the call has returned: otherwise the host overtook nothing and the case proves nothing"""
    pending = not s.query()
    assert pending, f'{name}: inconclusive, the delay ended before the call had been enqueued (lengthen it)'
    return pending


def _snapshot(outs):
    return [o.detach().clone() for o in outs]


def _set(late, which):
    for item in late:
        item[0].copy_(item[which])


def run_ab(name, late, call, outs=None, prefill=(), reads_back=False):
    """The A/B runner.

    late      [(buffer, A, B)]: floating-point device buffers and their two staged values (same shape and dtype)
    call      () -> None | list of tensors: the call under test, on the CURRENT stream; reads the buffers
    outs      the tensors `call` writes (when it returns None); NaN-filled before every call
    prefill   [(tensor, value tensor)]: outputs that are accumulated into or that `call` needs in a known state: restored (on the
              stream of the call) before every call
    reads_back  the call synchronises inside: must be named in READS_BACK; exempt from the pending assertion

    The last call the library sees before the delayed one has inputs A.  Whatever the library keeps between its own launches
    (snet::reduce_scratch, the arenas of the native sequencer, the work arrays of a D3 plan) therefore holds A-derived values when
    the delayed call starts: a LATER launch of a multi-launch entry point that strays from the stream reads those, writes an
    A-derived result, and the comparison with B's fails (test_stream_order_ops_gpu.py has a control for exactly this).

    returns (default-stream results for B, delayed-stream results)"""
    assert all(t.is_floating_point() and a.shape == t.shape == b.shape for t, a, b in late), f'{name}: late data is floating-point only'
    assert reads_back == (name.split('[')[0] in READS_BACK), f'{name}: list calls that read back in stream_order.READS_BACK'

    def once(which, delay_ms=None):
        if outs is not None:
            for o in outs:
                o.fill_(float('nan'))
        _set(late, 1)                                # (the buffers hold A whenever a call starts)
        torch.cuda.synchronize()
        if delay_ms is None:
            _set(late, which)
            for t, v in prefill:
                t.copy_(v)
            r = call()
            torch.cuda.synchronize()
            return _snapshot(outs if r is None else r), None
        stream = delayed_stream(delay_ms)            # (after the synchronisation above: nothing waits for the delay but `stream`)
        late_copy(stream, late, which)
        with torch.cuda.stream(stream):
            for t, v in prefill:
                t.copy_(v)
            r = call()
        pending = None if reads_back else assert_pending(stream, name)
        stream.synchronize()
        torch.cuda.synchronize()
        return _snapshot(outs if r is None else r), pending

    ref_a, _ = once(1)                               # (also the warm-up: plans, scratch and allocator pools exist afterwards)
    ref_b, _ = once(2)
    ref_b2, _ = once(2)
    assert len(ref_a) == len(ref_b) > 0
    for k, (x, y, z) in enumerate(zip(ref_a, ref_b, ref_b2)):
        assert not torch.isnan(y).any(), f'{name}: output {k} holds NaN on the default stream'
        assert torch.equal(z, y), f'{name}: output {k} is not repeatable on the default stream'
        assert not torch.equal(x, y), f'{name}: output {k} does not depend on the late input (A and B give the same bits)'
    # host time of enqueueing the call, after warm-up, on the default stream -- with inputs A: see above
    _set(late, 1)
    for t, v in prefill:
        t.copy_(v)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    enqueue_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    delay_ms = max(MIN_DELAY_MS, DELAY_FACTOR * enqueue_ms)
    got, pending = once(2, delay_ms)
    print(f'[stream_order] {name}: enqueue {enqueue_ms:.3f} ms, delay {delay_ms:.1f} ms, '
          + (f'pending = {pending}' if not reads_back else f'exempt ({READS_BACK[name.split("[")[0]]})'), flush=True)
    for k, (x, y) in enumerate(zip(got, ref_b)):
        what = 'it is the result of the STALE input' if torch.equal(x, ref_a[k]) else 'it is neither input\'s result'
        assert x.shape == y.shape and torch.equal(x, y), \
            f'{name}: output {k} on a delayed non-default stream differs from the default stream: {what}'
    return ref_b, got


def _flatten(res, prefix=''):
    """every array, tensor and scalar of a nested result (dicts / lists / tuples) as [(path, value)]"""
    import numpy as np
    if isinstance(res, dict):
        return [kv for k in sorted(res) for kv in _flatten(res[k], f'{prefix}.{k}')]
    if isinstance(res, (list, tuple)):
        return [kv for i, v in enumerate(res) for kv in _flatten(v, f'{prefix}[{i}]')]
    if isinstance(res, torch.Tensor):
        return [(prefix, res.detach().cpu().numpy().copy())]
    if isinstance(res, np.ndarray):
        return [(prefix, res.copy())]
    return [(prefix, res)]


def _same_results(a, b):
    """bit for bit: arrays equal entry by entry (a NaN where the other has one), everything else by =="""
    import numpy as np
    if [k for k, _ in a] != [k for k, _ in b]:
        return 'the results have different entries'
    for (k, x), (_, y) in zip(a, b):
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if not (isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.shape == y.shape and x.dtype == y.dtype
                    and np.array_equal(x, y, equal_nan=x.dtype.kind in 'fc')):
                return k
        elif x != y and not (isinstance(x, float) and isinstance(y, float) and x != x and y != y):
            return k
    return None


def run_whole(name, call, disturb):
    """A driver whose inputs live on the host: the whole call inside a delayed stream against the whole call on the default
    stream, every returned array bit for bit.  Such calls read values back, so they wait for the delay themselves: each must be
    named in READS_BACK, and the pending assertion does not apply.

    disturb   () -> result: the same driver on OTHER (rattled) inputs, run on the default stream right before the delayed call,
              so that every buffer the library or the host object keeps between calls holds values of another problem: work that
              strays from the stream and reads such a buffer before the stream has rewritten it gives a different result.

    This has less power than run_ab and says so: the first pageable host-to-device copy of a driver blocks the host until the
    delay is over, after which only the stream's own backlog separates it from a stray launch.  Returns the default-stream
    result."""
    assert name in READS_BACK, f'{name}: list calls that read back in stream_order.READS_BACK'
    torch.cuda.synchronize()
    ref = call()                                     # (also the warm-up)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again = call()
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    flat = _flatten(ref)
    assert sum(hasattr(v, 'shape') for _, v in flat) > 0
    bad = _same_results(_flatten(again), flat)
    assert bad is None, f'{name}: {bad} is not repeatable on the default stream'
    other = _flatten(disturb())
    torch.cuda.synchronize()
    assert _same_results(other, flat) is not None, f'{name}: the disturbing call returns the same bits: it disturbs nothing'
    delay_ms = max(MIN_DELAY_MS, DELAY_FACTOR * host_ms)
    s = delayed_stream(delay_ms)
    with torch.cuda.stream(s):
        got = call()
    s.synchronize()
    torch.cuda.synchronize()
    print(f'[stream_order] {name}: call {host_ms:.3f} ms, delay {delay_ms:.1f} ms, exempt ({READS_BACK[name]})', flush=True)
    bad = _same_results(_flatten(got), flat)
    assert bad is None, f'{name}: {bad} on a delayed non-default stream differs from the default stream'
    return ref


def same_edge_set(pos_a, pos_b, cell, pbc, cutoff, margin=0.01):
    """True iff A and B have the same neighbour list at `cutoff` and neither has a pair within `margin` (A) of it, by the brute-force
    list of tests/nl_ref.py on the CPU: a stale position then cannot overrun a buffer sized for the other set"""
    import numpy as np
    from nl_ref import brute_force_list

    def rows(pos, rc):
        ei, _, sh, _ = brute_force_list(pos, cell, pbc, rc)
        return np.concatenate([ei.T, sh], 1)
    lists = []
    for pos in (pos_a, pos_b):
        inner, at, outer = rows(pos, cutoff - margin), rows(pos, cutoff), rows(pos, cutoff + margin)
        if not (inner.shape == at.shape == outer.shape and np.array_equal(inner, at) and np.array_equal(at, outer)):
            return False
        lists.append(at)
    return lists[0].shape == lists[1].shape and bool(np.array_equal(lists[0], lists[1]))
