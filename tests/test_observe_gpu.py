"""GPU: the MD observables -- snet_obs_rdf and snet_obs_correlate on synthetic data against their fp64 restatement (observe_ref),
through the launch wrappers and without a model; then the driver on a model: the rattled two-species diamond cells, the
five-atom molecule and the isolated atom of tests/test_md_batch_gpu.py.

Kernel systems: 1, 5, 64 and 300 atoms in one batch (no pair, part of a wave, one wave, more than one stride of a 256-thread
loop and ten row tiles) with 1, 2 and 3 kinds, in a cubic cell, a triclinic cell with 60 degree angles, a thin cell whose
smallest height 2.13 A is below r_max / 2 (reach 2, self-images), a slab with an open axis and a molecule without a cell; every
atom displaced by up to three whole cell vectors per periodic axis, so that a difference that is not reduced lands in another bin."""
import ctypes as C

import numpy as np
import pytest
import torch

import md_ref
import observe_ref as ref
from stream_order import run_ab
from test_md_batch_gpu import DT, MASS_OF, _md_args, _start_velocities, model  # noqa: F401  (model: the fixture)
from test_batch_gpu import Z
from test_relax_gpu import D3_CUT, DEV, _all_systems, _cells

pytestmark = pytest.mark.gpu

R_MAX, BINS = 5.0, 50
SEED = 5          # test_no_pair_sits_on_a_bin_edge holds for it (chosen on the CPU, with the restatement alone)
TRI = np.array([[6.0, 0, 0], [3.0, 3 * np.sqrt(3), 0], [3.0, np.sqrt(3), 2 * np.sqrt(6)]])   # 60 degrees between all three


def _up(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _synthetic():
    """[(types, positions, cell, pbc)]: species indices out of 0 .. 4, so that local kinds are not the species"""
    rng = np.random.default_rng(SEED)
    spec = [(1, np.diag([9.0, 8.0, 2.13]), [True] * 3, [3]),
            (5, TRI, [True] * 3, [1, 4]),
            (64, np.eye(3) * 11.0, [True] * 3, [0, 2, 3]),
            (300, np.diag([20.0, 20.0, 0.0]), [True, True, False], [2, 4]),
            (5, np.zeros((3, 3)), [False] * 3, [0, 1, 4]),
            (64, np.diag([9.0, 8.0, 2.13]), [True] * 3, [1, 2])]
    out = []
    for n, cell, pbc, species in spec:
        box = np.where(np.asarray(pbc)[:, None], cell, np.eye(3) * 6.0)
        pos = rng.uniform(0, 1, (n, 3)) @ box
        pos = pos + (rng.integers(-3, 4, (n, 3)) * np.asarray(pbc)) @ cell     # whole cell vectors, per atom
        types = np.asarray(species)[np.arange(n) % len(species)] if n > 1 else np.asarray(species[:1])
        out.append((rng.permutation(types), pos, cell, np.asarray(pbc)))
    return out


def _plan(systems, obs):
    from sevennet_amd.observe import observe_plan
    return observe_plan(obs, np.concatenate([s[0] for s in systems]), np.array([len(s[0]) for s in systems]),
                        np.stack([s[2] for s in systems]), np.stack([s[3] for s in systems]))


def _accumulator(systems, obs, masses=None, hold=None):
    from sevennet_amd.observe import Accumulator
    plan = _plan(systems, obs)
    n = sum(len(s[0]) for s in systems)
    mass = _up(np.ones(n) if masses is None else np.concatenate(masses), torch.float64)
    return Accumulator(plan, mass, _up(plan['a_ptr'], torch.int32), None if hold is None else _up(hold, torch.int32), DEV), plan


def _rdf_reference(systems, frames=None):
    """per system (counts, margin) of the restatement, summed over `frames` (lists of per-system positions; default: the systems')"""
    out = []
    for b, (types, pos, cell, pbc) in enumerate(systems):
        _, kind = ref.local_kinds(types)
        S = int(kind.max()) + 1
        parts = [ref.rdf_counts(pos if f is None else f[b], kind, S, cell, pbc, R_MAX, BINS) for f in (frames or [None])]
        out.append((sum(p[0] for p in parts), min(p[1] for p in parts)))
    return out


@pytest.fixture(scope='module')
def synthetic():
    systems = _synthetic()
    return systems, _rdf_reference(systems)


def _device_counts(systems, frames=None):
    from sevennet_amd.observe import Observe
    acc, plan = _accumulator(systems, Observe(every=1, rdf_rmax=R_MAX, rdf_bins=BINS))
    for f in (frames or [[s[1] for s in systems]]):
        acc.sample(_up(np.concatenate(f), torch.float64), torch.zeros(len(plan['kind']), 3, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    counts, cp = acc.to_host()['counts'], plan['count_ptr']
    return [counts[cp[b]:cp[b + 1]].reshape(int(plan['n_kinds'][b]), int(plan['n_kinds'][b]), BINS) for b in range(len(systems))]


# ------------------------------------------------------------------------------------------------ snet_obs_rdf
def test_no_pair_sits_on_a_bin_edge(synthetic):
    """the precondition of exact counts, from the restatement alone: a pair within 1e-9 A of an edge could fall either way"""
    systems, want = synthetic
    from sevennet_amd.observe import image_reach
    reach = image_reach(np.stack([s[2] for s in systems]), np.stack([s[3] for s in systems]), R_MAX)
    assert reach.tolist() == [[1, 1, 2], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 2]]
    assert [len(np.unique(s[0])) for s in systems] == [1, 2, 3, 2, 3, 2]
    for b, (counts, margin) in enumerate(want):
        print(f'system {b}: {int(counts.sum())} counted triples, nearest to an edge {margin:.3e} A')
        assert margin > 1e-9, (b, margin)
    assert want[0][0].sum() > 0 and all(w[0].sum() > 50 for w in want[1:4])   # the lone atom sees its own images


def test_rdf_counts_equal_the_restatement(synthetic):
    systems, want = synthetic
    got = _device_counts(systems)
    for b, (g, (w, _)) in enumerate(zip(got, want)):
        assert g.dtype == np.int64 and g.shape == w.shape
        assert np.array_equal(g, w), (b, int(np.abs(g - w).sum()), int(w.sum()))
        assert np.array_equal(g, g.transpose(1, 0, 2))   # ordered pairs: (ka, kb) mirrors (kb, ka)


def test_rdf_accumulates_and_does_not_depend_on_the_batch(synthetic):
    systems, want = synthetic
    rng = np.random.default_rng(SEED + 1)
    second = [s[1] + rng.normal(0, 0.3, s[1].shape) for s in systems]
    w2 = _rdf_reference(systems, [second])
    assert min(m for _, m in w2) > 1e-9
    both = _device_counts(systems, [[s[1] for s in systems], second])
    for b in range(len(systems)):
        assert np.array_equal(both[b], want[b][0] + w2[b][0]), b
    for b in (0, 3, 5):
        assert np.array_equal(_device_counts(systems[b:b + 1])[0], want[b][0]), b
    from sevennet_amd.observe import Observe
    acc, plan = _accumulator(systems, Observe(every=1, rdf_rmax=R_MAX, rdf_bins=BINS, by_species=False))
    acc.sample(_up(np.concatenate([s[1] for s in systems]), torch.float64), torch.zeros(len(plan['kind']), 3, dtype=torch.float64, device=DEV))
    folded = acc.to_host()['counts'].reshape(len(systems), BINS)
    for b in range(len(systems)):
        assert np.array_equal(folded[b], want[b][0].sum((0, 1))), b


# ------------------------------------------------------------------------------------------------ snet_obs_correlate
T_SAMPLES, LAGS, ORIGIN_EVERY = 40, 7, 3
SIZES = [1, 5, 64, 300]


def _trajectory():
    """harmonic motion about sites plus a drift per system, velocities given (not derived): [T,N,3] each, and masses, types, hold"""
    rng = np.random.default_rng(17)
    t = np.arange(T_SAMPLES)[:, None, None] * 0.7
    pos, vel, masses, types, hold = [], [], [], [], []
    for b, n in enumerate(SIZES):
        x0, amp = rng.uniform(-8, 8, (n, 3)), rng.normal(0, 0.4, (n, 3))
        w, ph = rng.uniform(0.05, 0.6, (n, 3)), rng.uniform(0, 6.28, (n, 3))
        drift = rng.normal(0, 0.05, 3)
        pos.append(x0 + amp * np.sin(w * t + ph) + drift * t)
        vel.append(amp * w * np.cos(w * t + ph) + drift + rng.normal(0, 0.01, (T_SAMPLES, n, 3)))
        masses.append(rng.choice([1.008, 15.999, 28.0855], n))
        types.append(rng.integers(0, [1, 2, 3, 2][b], n) * 2)
        hold.append(np.zeros(n, np.int32))
    hold[2][[3, 40]] = [7, 2]                       # the 64-atom system is anchored: it is not corrected
    return pos, vel, masses, types, hold


@pytest.fixture(scope='module')
def trajectory():
    return _trajectory()


def _correlate_device(traj, sel, remove_com):
    from sevennet_amd.observe import Observe
    pos, vel, masses, types, hold = traj
    systems = [(types[b], pos[b][0], np.zeros((3, 3)), np.zeros(3, bool)) for b in sel]
    acc, plan = _accumulator(systems, Observe(every=1, lags=LAGS, origin_every=ORIGIN_EVERY, remove_com=remove_com),
                             [masses[b] for b in sel], np.concatenate([hold[b] for b in sel]))
    assert tuple(acc.ring_pos.shape) == (3, sum(SIZES[b] for b in sel), 3)          # 40 samples wrap a ring of 3 more than twice
    for s in range(T_SAMPLES):
        acc.sample(_up(np.concatenate([pos[b][s] for b in sel]), torch.float64), _up(np.concatenate([vel[b][s] for b in sel]), torch.float64))
    torch.cuda.synchronize()
    h = acc.to_host()
    kp = plan['kind_ptr']
    return [(h['msd_sum'][kp[i]:kp[i + 1]], h['vacf_sum'][kp[i]:kp[i + 1]]) for i in range(len(sel))]


@pytest.mark.parametrize('remove_com', [True, False], ids=['com', 'raw'])
def test_correlations_follow_the_restatement(trajectory, remove_com):
    """msd_sum / vacf_sum within 1e-12 of the system's largest entry: one fp64 sum of at most 300 terms in another order is about
    300 x 1.1e-16 = 3e-14; ten times that, rounded up"""
    from sevennet_amd.observe import origin_counts
    pos, vel, masses, types, hold = trajectory
    got = _correlate_device(trajectory, [0, 1, 2, 3], remove_com)
    for b, n in enumerate(SIZES):
        _, kind = ref.local_kinds(types[b])
        S = int(kind.max()) + 1
        msd, vacf, n_or = ref.correlate(pos[b], vel[b], masses[b], kind, S, LAGS, ORIGIN_EVERY, remove_com, anchored=bool(hold[b].any()))
        assert np.array_equal(origin_counts(T_SAMPLES, LAGS, ORIGIN_EVERY), n_or) and n_or.tolist() == [14, 13, 13, 13, 12, 12, 12]
        for name, g, w in (('msd', got[b][0], msd), ('vacf', got[b][1], vacf)):
            err, scale = np.abs(g - w).max(), np.abs(w).max()
            print(f'system {b} ({n} atoms) {name}: max error {err:.2e}, largest entry {scale:.3e}')
            assert g.shape == w.shape == (S, LAGS) and err <= 1e-12 * scale, (b, name, err, scale)
        if n == 1 and remove_com:
            assert not got[b][0].any() and not got[b][1].any()
        else:
            assert (got[b][0][:, 1:] > 0).all() and not got[b][0][:, 0].any()      # lag 0: no displacement, exactly
    if remove_com:   # the anchored system was not corrected: its sums are the raw ones, bit for bit
        raw = _correlate_device(trajectory, [2], False)
        assert np.array_equal(raw[0][0], got[2][0]) and np.array_equal(raw[0][1], got[2][1])


def test_a_systems_sums_do_not_depend_on_its_company(trajectory):
    full = _correlate_device(trajectory, [0, 1, 2, 3], True)
    for b in (1, 3):
        alone = _correlate_device(trajectory, [b], True)
        assert np.array_equal(alone[0][0], full[b][0]) and np.array_equal(alone[0][1], full[b][1]), b


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_without_launching(synthetic):
    """null pointers, bad shapes and arguments over the caps: rc 2 with a message, and nothing is written"""
    from sevennet_amd import _lib
    from sevennet_amd.observe import Observe, obs_correlate, obs_rdf
    lib = _lib.load()
    systems, want = synthetic
    acc, plan = _accumulator(systems, Observe(every=1, rdf_rmax=R_MAX, rdf_bins=BINS, lags=4, origin_every=2))
    N, B, T = len(plan['kind']), len(systems), len(plan['tile'])
    pos = _up(np.concatenate([s[1] for s in systems]), torch.float64)
    vel = torch.zeros_like(pos)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rdf(pos=pos, n_sys=B, dr=R_MAX / BINS, bins=BINS, kinds_max=3, reach_max=2, counts=acc.counts):
        return lib.snet_obs_rdf(P(pos), N, P(acc.seg_ptr), n_sys, P(acc.kind), P(acc.cell), P(acc.sys_desc), P(acc.tile), T, dr, bins,
                                kinds_max, reach_max, P(counts), acc.counts.numel(), st)
    for kw, msg in ((dict(pos=None), b'null argument'), (dict(counts=None), b'null argument'), (dict(n_sys=0), b'bad shape'),
                    (dict(dr=0.0), b'out of range'), (dict(dr=float('inf')), b'out of range'), (dict(bins=0), b'out of range'),
                    (dict(kinds_max=9), b'out of range'), (dict(kinds_max=0), b'out of range'), (dict(reach_max=5), b'out of range'),
                    (dict(kinds_max=8, bins=129), b'out of range')):
        assert rdf(**kw) == 2 and msg in lib.snet_last_error(), kw

    def cor(vel=vel, n_sys=B, sample=0, origin_every=2, ring=2, lags=4, msd=acc.msd_sum):
        return lib.snet_obs_correlate(P(pos), P(vel), P(acc.ring_pos), P(acc.ring_vel), P(acc.mass), None, N, P(acc.seg_ptr), n_sys,
                                      P(acc.kind), P(acc.kind_ptr), acc.msd_sum.shape[0], sample, origin_every, ring, lags, 1, P(msd),
                                      P(acc.vacf_sum), st)
    for kw, msg in ((dict(vel=None), b'null argument'), (dict(msd=None), b'null argument'), (dict(n_sys=0), b'bad shape'),
                    (dict(sample=-1), b'out of range'), (dict(origin_every=0), b'out of range'), (dict(lags=0), b'out of range'),
                    (dict(ring=1), b'out of range'), (dict(ring=3), b'out of range'), (dict(ring=70000, lags=140000), b'out of range')):
        assert cor(**kw) == 2 and msg in lib.snet_last_error(), kw
    torch.cuda.synchronize()
    assert not acc.counts.any() and not acc.msd_sum.any() and not acc.vacf_sum.any()
    with pytest.raises(ValueError, match='obs_rdf'):   # the wrappers check dtypes and shapes before the call
        obs_rdf(pos.float(), acc.seg_ptr, acc.kind, acc.cell, acc.sys_desc, acc.tile, 0.1, BINS, 3, 2, acc.counts)
    with pytest.raises(ValueError, match='obs_correlate'):
        obs_correlate(pos, vel[:-1], acc.ring_pos, acc.ring_vel, acc.mass, acc.seg_ptr, acc.kind, acc.kind_ptr, 0, 2, 4, True,
                      acc.msd_sum, acc.vacf_sum)
    assert rdf() == 0 and cor() == 0
    torch.cuda.synchronize()
    cp = plan['count_ptr']
    assert np.array_equal(acc.counts.cpu().numpy()[cp[2]:cp[3]].reshape(3, 3, BINS), want[2][0])


@pytest.mark.parametrize('case', ['com', 'raw', 'held', 'folded'])
def test_observe_launches_on_a_delayed_stream(synthetic, case):
    """the launches of two samples -- pair counts, the origin's copy into the ring, the correlation -- behind a delay on a
    non-default stream, positions and velocities arriving late: with the centre of mass removed, without, with a hold mask (the
    64-atom cell is anchored) and with all species folded into one kind.

    Four cases, not one: each takes one stream from torch's pool, and this file runs before test_stream_order_ops_gpu.py, whose
    controls need their stray NULL-stream launch to overtake the delayed stream -- which holds only while the two do not share
    one of the process's four hardware queues, and so depends on how many streams were taken before (see
    test_stream_order_elastic_gpu.py).  With one case here test_positive_control_null_stream_reads_the_stale_input stopped
    seeing the stale input in a run of the whole suite; with four it behaves as it did without this file."""
    from sevennet_amd.observe import Observe
    systems = synthetic[0]
    rng = np.random.default_rng(3)
    N = sum(len(s[0]) for s in systems)
    hold = np.zeros(N, np.int32)
    if case == 'held':
        hold[6 + 10] = 5                    # an atom of the 64-atom cubic cell (rows 6 .. 69)
    acc, plan = _accumulator(systems, Observe(every=1, rdf_rmax=R_MAX, rdf_bins=BINS, lags=2, remove_com=case != 'raw',
                                              by_species=case != 'folded'), hold=hold if case == 'held' else None)
    frames = [[_up(np.concatenate([s[1] for s in systems]) + rng.normal(0, 0.2, (N, 3)), torch.float64) for _ in range(2)] for _ in range(4)]
    bufs = [torch.empty(N, 3, dtype=torch.float64, device=DEV) for _ in range(4)]   # x_0, v_0, x_1, v_1
    zero = [(t, torch.zeros_like(t)) for t in (acc.counts, acc.msd_sum, acc.vacf_sum, acc.ring_pos, acc.ring_vel)]

    def call():
        acc.n_samples = 0
        acc.sample(bufs[0], bufs[1])
        acc.sample(bufs[2], bufs[3])
        return [acc.counts, acc.msd_sum, acc.vacf_sum]
    ref_b, got = run_ab('observe', [(b, f[0], f[1]) for b, f in zip(bufs, frames)], call, prefill=zero)
    assert got[0].sum() > 0 and got[1][:, 1].sum() > 0 and got[2].abs().sum() > 0


# ------------------------------------------------------------------------------------------------ the driver on a model
STEPS, EVERY = 12, 2
RDF_BINS = 37       # 4 A / 37: the molecule's bond of exactly 1.1 A, in frame 0 as the caller gave it, is on no edge


def _observe(**kw):
    from sevennet_amd.observe import Observe
    return Observe(**dict(dict(every=EVERY, rdf_rmax=4.0, rdf_bins=RDF_BINS, lags=4, origin_every=2), **kw))


@pytest.mark.parametrize('friction', [0.0, 0.01], ids=['nve', 'langevin'])
def test_observe_changes_no_bit_of_the_run(model, friction):
    """state, logs and trajectory with `observe` equal those without it; and the observables equal the restatement applied to
    the returned trajectory: counts exactly (no pair within 1e-9 A of an edge), msd within 1e-12 of its largest entry"""
    systems = _all_systems()
    kw = dict(velocities=_start_velocities(systems), traj_every=EVERY, seed=3, friction=friction,
              temperature=300.0 if friction else None)
    plain = model.calc.md_many(*_md_args(systems), DT, STEPS, **kw)
    info = dict(model.calc.md_info)
    res = model.calc.md_many(*_md_args(systems), DT, STEPS, observe=_observe(), **kw)
    n_samples = STEPS // EVERY + 1
    assert model.calc.md_info == dict(info, md_launches=STEPS + 1 + (n_samples - 2), observe_samples=n_samples)
    for b, (r, p) in enumerate(zip(res, plain)):
        assert set(r) == set(p) | {'observables'}
        for k in ('positions', 'velocities', 'e_pot', 'e_kin', 'temperature', 'trajectory', 'forces'):
            assert np.array_equal(r[k], p[k]), (b, k)
        assert r['energy'] == p['energy']
        types, _, cell, pbc = systems[b]
        present, kind = ref.local_kinds(types)
        o, S = r['observables'], len(present)
        assert o['every'] == EVERY and o['n_samples'] == n_samples == len(r['trajectory'])
        assert o['kinds'].tolist() == [Z[t] for t in present]
        parts = [ref.rdf_counts(x, kind, S, cell, pbc, 4.0, RDF_BINS) for x in r['trajectory']]
        assert min(m for _, m in parts) > 1e-9
        assert np.array_equal(o['rdf']['counts'], sum(c for c, _ in parts)), b
        assert (o['rdf']['g'] is None) == (not all(pbc)) and o['rdf']['edges'].shape == (RDF_BINS + 1,)
        vel0 = np.zeros_like(r['trajectory'])
        msd, _, n_or = ref.correlate(r['trajectory'], vel0, MASS_OF[types], kind, S, 4, 2)
        per_kind = np.bincount(kind, minlength=S)
        want = msd / (n_or[None, :] * per_kind[:, None])
        err, scale = np.abs(o['msd'] - want).max(), np.abs(want).max()
        print(f'system {b}: msd max error {err:.2e}, largest entry {scale:.3e} A^2; {int(o["rdf"]["counts"].sum())} counted triples')
        assert err <= 1e-12 * scale and np.array_equal(o['n_origins'], n_or) and o['lag_times'].tolist() == [0.0, 2.0, 4.0, 6.0]
        assert np.abs(o['msd_all'] - msd.sum(0) / (n_or * len(types))).max() <= 1e-12 * scale
        assert o['vacf'].shape == (S, 4) and np.isfinite(o['vacf']).all()


def test_vacf_at_lag_zero_is_the_kinetic_energy(model):
    """one species, remove_com=False, every sample an origin, log_every = every: vacf_all[0] n = mean over samples of sum |v|^2 =
    mean of 2 e_kin ACC / m, to 1e-12 relative -- v_k is the velocity after the finishing half kick, the one e_kin is taken of"""
    systems = [(np.zeros(len(s[0]), int), s[1], s[2], s[3]) for s in _cells()[:2]]
    res = model.calc.md_many(*_md_args(systems), DT, STEPS, velocities=_start_velocities(systems), log_every=EVERY,
                             observe=_observe(rdf_rmax=None, lags=3, origin_every=1, remove_com=False))
    for r, s in zip(res, systems):
        o = r['observables']
        assert o['kinds'].tolist() == [14] and 'rdf' not in o and o['n_origins'].tolist() == [7, 6, 5]
        want = np.mean(2.0 * r['e_kin'] * md_ref.ACC / MASS_OF[0])
        assert abs(o['vacf_all'][0] * len(s[0]) - want) <= 1e-12 * want, (o['vacf_all'][0] * len(s[0]), want)
        assert np.array_equal(o['vacf_all'], o['vacf'][0]) and o['msd_all'][0] == 0.0 and (o['msd_all'][1:] > 0).all()


def test_held_atoms_and_refusals(model):
    """with fixed_list the masked step is split the same way; pressure with observe raises before any device work"""
    systems = _all_systems()[:3]
    fixed = [np.array([0, 3]), None, np.arange(16) < 4]
    kw = dict(velocities=_start_velocities(systems), traj_every=EVERY, fixed_list=fixed)
    plain = model.calc.md_many(*_md_args(systems), DT, STEPS, **kw)
    res = model.calc.md_many(*_md_args(systems), DT, STEPS, observe=_observe(rdf_rmax=None), **kw)
    for b, (r, p) in enumerate(zip(res, plain)):
        for k in ('positions', 'velocities', 'e_pot', 'e_kin', 'trajectory'):
            assert np.array_equal(r[k], p[k]), (b, k)
        types = systems[b][0]
        present, kind = ref.local_kinds(types)
        msd, _, n_or = ref.correlate(r['trajectory'], np.zeros_like(r['trajectory']), MASS_OF[types], kind, len(present), 4, 2,
                                     anchored=fixed[b] is not None)
        want = msd / (n_or[None, :] * np.bincount(kind)[:, None])
        assert np.abs(r['observables']['msd'] - want).max() <= 1e-12 * np.abs(want).max(), b
    with pytest.raises(ValueError, match='observe with pressure'):
        model.calc.md_many(*_md_args(systems), DT, 2, temperature=300.0, pressure=0.01, compressibility=50.0, observe=_observe())


@pytest.mark.parametrize('d3_term', ['host', 'device'])
def test_d3_calculator_passes_observe_through(model, d3_term):
    from sevennet_amd.d3 import SevenNetD3Calculator
    systems = _cells()
    d3 = SevenNetD3Calculator((model.cfg, model.sd), file_type='model_instance', device=DEV, **D3_CUT)
    res = d3.md_many(*_md_args(systems), DT, 4, d3_term=d3_term, velocities=_start_velocities(systems), observe=_observe())
    for r, s in zip(res, systems):
        o = r['observables']
        assert o['n_samples'] == 3 and o['kinds'].tolist() == [14, 8] and o['rdf']['counts'].sum() > 0 and o['msd'].shape == (2, 4)
        assert np.isnan(o['msd'][:, 3]).all() and (o['msd'][:, 1:3] > 0).all()    # three samples: lag 3 has no origin yet
