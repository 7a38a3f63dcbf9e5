"""CPU: the first interaction layer from per-atom radial moments (csrc/snet_layer0.hip) -- the two identities the kernels
rest on in numpy fp64, the folded weights as the split-precision GEMM receives them, and the eligibility predicate."""
import ctypes as C

import numpy as np

HID = 64


def direct_reference(case, g_m=None):
    """fp64 evaluation of layer 0 as the per-edge kernels define it.  Forward: m[i, q, u] = scale sum_e Y_e[q] T[s(e), u] w_e[l(q) mul + u]
    with w_e = h2_e W2; reverse (g_m given): g_vec[e] = sum_{q >= 1} dE/dY_e[q] dY_e[q]/dr + dE/d|r_e| r_e / |r_e|."""
    f = lambda k: np.asarray(case[k], np.float64)  # noqa: E731
    mul, lmax, N = case['mul'], case['lmax'], case['N']
    Q = (lmax + 1) ** 2
    lq = np.array([l for l in range(lmax + 1) for _ in range(2 * l + 1)])
    rows = np.arange(case['E']) if case['w_row'] is None else np.asarray(case['w_row'])
    center = np.repeat(np.arange(N), np.diff(np.asarray(case['row_ptr'])))
    x = f('table')[np.asarray(case['types'])[np.asarray(case['src'])]]                      # [E, mul]
    w = (f('h2')[rows] @ f('W2')).reshape(-1, lmax + 1, mul)[:, lq, :]                      # [E, Q, mul]
    Y, scale = f('sh'), float(case['scale'])
    if g_m is None:
        m = np.zeros((N, Q, mul))
        np.add.at(m, center, scale * Y[:, :, None] * x[:, None, :] * w)
        return m
    wd = (f('h2d')[rows] @ f('W2')).reshape(-1, lmax + 1, mul)[:, lq, :]
    ge = np.asarray(g_m, np.float64).reshape(N, Q, mul)[center] * x[:, None, :] * scale     # [E, Q, mul]
    gY = (ge * w).sum(2)
    gr = (Y * (ge * wd).sum(2)).sum(1)
    v = f('edge_vec')
    return np.einsum('eq,eqa->ea', gY[:, 1:], f('dsh').reshape(-1, Q, 3)[:, 1:]) + gr[:, None] * v / np.linalg.norm(v, axis=1, keepdims=True)


def random_case(mul=4, lmax=2, n_species=3, present=(0, 2), degrees=(0, 1, 5, 3), n_ghost=2, seed=0, dtype=np.float64):
    rng = np.random.default_rng(seed)
    N, Q = len(degrees), (lmax + 1) ** 2
    row_ptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int32)
    E = int(row_ptr[-1])
    types = rng.choice(np.asarray(present), N + n_ghost).astype(np.int32)
    types[:len(present)] = present
    v = rng.normal(0, 1, (E, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.8, 4.5, (E, 1))
    return dict(mul=mul, lmax=lmax, N=N, E=E, row_ptr=row_ptr, src=rng.integers(0, N + n_ghost, E).astype(np.int32), types=types,
                w_row=None, table=rng.normal(0, 1, (n_species, mul)).astype(dtype), W2=(rng.normal(0, 1, (HID, (lmax + 1) * mul)) / 8).astype(dtype),
                h2=rng.normal(0, 1, (E, HID)).astype(dtype), h2d=rng.normal(0, 1, (E, HID)).astype(dtype), sh=rng.normal(0, 1, (E, Q)).astype(dtype),
                dsh=rng.normal(0, 1, (E, 3 * Q)).astype(dtype), edge_vec=v.astype(dtype), scale=0.25)


def moments_path(case, g_m=None):
    """the same two quantities with the neighbour sum taken first (fp64): moments M and one product per atom"""
    mul, lmax, N, E = case['mul'], case['lmax'], case['N'], case['E']
    Q = (lmax + 1) ** 2
    lq = np.array([l for l in range(lmax + 1) for _ in range(2 * l + 1)])
    present = sorted(set(np.asarray(case['types']).tolist()))
    slot_of = {s: i for i, s in enumerate(present)}
    S = len(present)
    center = np.repeat(np.arange(N), np.diff(case['row_ptr']))
    slot = np.array([slot_of[int(case['types'][j])] for j in case['src']])
    B = [(case['W2'][None, :, l * mul:(l + 1) * mul] * case['table'][present][:, None, :] * case['scale']).reshape(S * HID, mul) for l in range(lmax + 1)]
    if g_m is None:
        M = np.zeros((N, Q, S, HID))
        np.add.at(M, (center, slice(None), slot), case['sh'][:, :, None] * case['h2'][:, None, :])
        return np.stack([M[:, q].reshape(N, S * HID) @ B[lq[q]] for q in range(Q)], 1), M
    Bm = np.stack([g_m.reshape(N, Q, mul)[:, q] @ B[lq[q]].T for q in range(Q)], 1).reshape(N, Q, S, HID)
    be = Bm[center, :, slot]                                                    # [E, Q, HID]
    gY = np.einsum('ek,eqk->eq', case['h2'], be)
    gr = (case['sh'] * np.einsum('ek,eqk->eq', case['h2d'], be)).sum(1)
    v = case['edge_vec']
    return np.einsum('eq,eqa->ea', gY[:, 1:], case['dsh'].reshape(E, Q, 3)[:, 1:]) + gr[:, None] * v / np.linalg.norm(v, axis=1, keepdims=True)


def test_both_identities_in_fp64_with_a_species_absent_among_the_neighbours():
    """three species in the model, one of them on no atom at all, and a node whose neighbours miss a second one"""
    c = random_case(seed=3)
    c['types'][:] = [0, 2, 0, 2, 0, 2]
    c['src'][c['row_ptr'][2]:c['row_ptr'][3]] = [0, 2, 4, 0, 2]      # node 2 sees species 0 only
    m_ref = direct_reference(c)
    m, M = moments_path(c)
    assert np.abs(m - m_ref).max() <= 1e-13 * np.abs(m_ref).max()
    assert np.all(M[2, :, 1] == 0) and np.all(M[0] == 0)              # the absent slot's moments / a node without edges
    g_m = np.random.default_rng(1).normal(0, 1, m_ref.shape)
    gv_ref = direct_reference(c, g_m)
    gv = moments_path(c, g_m)
    assert np.abs(gv - gv_ref).max() <= 1e-13 * np.abs(gv_ref).max()
    # the reverse formula is the gradient of the forward one: directional derivative of <g_m, m> along a change of Y
    dY = np.random.default_rng(2).normal(0, 1, c['sh'].shape)
    c2 = dict(c, sh=c['sh'] + 1e-6 * dY)
    num = ((direct_reference(c2) - m_ref) * g_m).sum() / 1e-6
    rows, lq = np.arange(c['E']), np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
    center = np.repeat(np.arange(c['N']), np.diff(c['row_ptr']))
    w = (c['h2'][rows] @ c['W2']).reshape(-1, 3, c['mul'])[:, lq, :]
    gY = (g_m[center] * c['table'][c['types'][c['src']]][:, None, :] * c['scale'] * w).sum(2)
    assert abs(num - (gY * dY).sum()) <= 1e-6 * abs(num)


def test_folded_weights_reach_the_gemm_as_three_bf16_terms_of_the_fp64_product():
    """snet_layer0_fold (the host loop snet_layer0_plan_create packs from): B_l^T[u, s 64 + k] against the fp64 product, rounded once;
    then that matrix through snet_gemm_split_pack: every entry the sum of three bf16 terms, in the B-fragment layout"""
    from sevennet_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(0)
    mul, lmax, S = 16, 2, 3
    wn = (lmax + 1) * mul
    W2 = (rng.normal(0, 1, (HID, wn)) / 8).astype(np.float32)
    table = rng.normal(0, 1, (S, mul)).astype(np.float32)
    scale = np.float32(1.0 / 28.0)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for l in range(lmax + 1):
        want = (np.einsum('ku,su->usk', W2[:, l * mul:(l + 1) * mul].astype(np.float64), table.astype(np.float64)) * float(scale)).reshape(mul, S * HID)
        bt = np.full((mul, S * HID), np.nan, np.float32)
        assert lib.snet_layer0_fold(P(W2), wn, mul, P(table), scale, S, l, P(bt)) == 0
        assert np.array_equal(bt, want.astype(np.float32))                           # fp64 product, rounded once
        K, N = bt.shape
        buf = np.zeros(int(lib.snet_gemm_split_size(K, N)), np.uint8)
        assert lib.snet_gemm_split_pack(P(bt), K, N, P(buf)) == 0
        nt, nq = (N + 31) // 32, (K + 15) // 16
        f = (buf.view(np.uint16).reshape(nt, nq, 3, 64, 8).astype(np.uint32) << 16).view(np.float32).sum(axis=2, dtype=np.float64)
        lane, i = np.meshgrid(np.arange(64), np.arange(8), indexing='ij')
        for t in range(nt):
            for q in range(nq):
                k, n = 16 * q + 8 * (lane >> 5) + i, 32 * t + (lane & 31)
                ref = np.where((k < K) & (n < N), want[np.minimum(k, K - 1), np.minimum(n, N - 1)], 0.0)
                assert np.abs(f[t, q] - ref).max() <= 2.0 ** -21 * np.abs(want).max()
    assert lib.snet_layer0_fold(P(W2), wn, mul, P(table), scale, S, lmax + 1, P(bt)) != 0   # a column block past the matrix


def test_eligibility_predicate():
    from sevennet_amd.model_spec import (build_model_spec, layer0_moments_eligible, sevennet_0_config, sevennet_l3i5_config,
                                         sevennet_mf_ompa_config)
    from sevennet_amd.shapes import mini_sevennet_0_config, unit_test_config
    tags = {}
    for cfg in (sevennet_0_config(), sevennet_l3i5_config(), sevennet_mf_ompa_config()):
        layers = build_model_spec(cfg).layers
        assert layer0_moments_eligible(layers[0].conv, layers[0].mlp_dims)
        tags[layers[0].conv.tag] = True
        assert not layer0_moments_eligible(layers[1].conv, layers[1].mlp_dims)          # non-scalar irreps_x
        assert not layer0_moments_eligible(layers[-1].conv, layers[-1].mlp_dims)
    assert sorted(tags) == sorted(['ecc5d202727d', 'c611da7b78ef', '568ada5bb7a7'])
    l0 = build_model_spec(mini_sevennet_0_config()).layers[0]
    assert layer0_moments_eligible(l0.conv, l0.mlp_dims)
    assert not layer0_moments_eligible(l0.conv, [8, 32, 32, l0.conv.weight_numel])         # another radial network
    small = build_model_spec(unit_test_config()).layers[0]                               # 4 channels: no fused kernels supply h2
    assert not layer0_moments_eligible(small.conv, small.mlp_dims)
