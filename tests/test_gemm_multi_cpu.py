"""CPU: the launch plan of the two-source node GEMMs (model_spec.plan_multi_source) and the entry point's declaration.

The plan is pure Python: for every layer of the registered model shapes, the launch lists of y = SI2(m) + sc(x), of
g_x = sc^T(g_y) + SI1^T(g_h) and of layer 0's table launch must write every (row list, output column) exactly once -- by a
problem or by the zero fill -- and read every weight block exactly once per row list it applies to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sevennet_amd import model_spec as ms
from sevennet_amd.shapes import mini_sevennet_0_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_self_connection_config():
    cfg = dict(mini_sevennet_0_config())
    cfg['self_connection_type'] = 'none'
    return cfg


CONFIGS = {
    'mini_sevennet_0': mini_sevennet_0_config,
    'sevennet_0': ms.sevennet_0_config,
    'sevennet_mf_ompa': ms.sevennet_mf_ompa_config,
    'no_self_connection': _no_self_connection_config,
}


def _check_plan(linears, transpose):
    """every column of the output side once per row list; every block of every linear once per row list it belongs to"""
    plan = ms.plan_multi_source(linears, transpose)
    assert plan is not None, [sp.name for sp in linears]
    launches, zero = plan
    dim = linears[0].dim_in if transpose else linears[0].dim_out
    ns = max(sp.n_species for sp in linears)
    assert [s for s, _ in launches] == (list(range(ns)) if ns else [-1])
    for s, probs in launches:
        assert 1 <= len(probs) <= ms.MAX_GEMM_GROUP
        writes = np.zeros(dim, int)
        read = [np.zeros(len(sp.blocks), int) for sp in linears]
        for c_off, d, n, srcs in probs:
            writes[c_off:c_off + d * n] += 1
            assert 1 <= len(srcs) <= ms.MAX_GEMM_SRC and [i for i, _ in srcs] == sorted({i for i, _ in srcs})   # linears in the order given
            for i, j in srcs:
                b = linears[i].blocks[j]
                read[i][j] += 1
                assert b.species in (-1, s) and 2 * b.l + 1 == d
                assert (b.in_off, b.mul_in) == (c_off, n) if transpose else (b.out_off, b.mul_out) == (c_off, n)
        for off, ln in zero:
            writes[off:off + ln] += 1
        assert (writes == 1).all(), (s, np.nonzero(writes != 1)[0][:8])
        for sp, r in zip(linears, read):
            want = np.array([int(b.species in (-1, s)) for b in sp.blocks])
            assert (r == want).all(), (sp.name, s)
    return plan


@pytest.mark.parametrize('name', list(CONFIGS))
def test_plans_write_every_row_and_block_once(name):
    spec = ms.build_model_spec(CONFIGS[name]())
    n_pairs = 0
    for t, ls in enumerate(spec.layers):
        if ls.sc is None:
            continue
        fwd, _ = _check_plan([ls.si2, ls.sc], False)
        n_pairs += sum(len(srcs) == 2 for _, probs in fwd for _, _, _, srcs in probs)
        if t > 0:
            _check_plan([ls.sc, ls.si1], True)
        else:   # layer 0 with species tables: SI2 alone must reach every column, the table's row is added to what it writes
            assert _check_plan([ls.si2], False)[1] == []
    if name == 'no_self_connection':
        assert all(ls.sc is None for ls in spec.layers) and n_pairs == 0
    else:
        assert n_pairs > 0
    if name == 'sevennet_mf_ompa':   # 119 species lists per layer; the hosts launch the non-empty ones
        assert len(ms.plan_multi_source([spec.layers[1].si2, spec.layers[1].sc], False)[0]) == 119


def test_rule_refuses_what_it_cannot_write_once():
    from sevennet_amd.irreps import Irreps
    a = ms.make_linear('a.weight', Irreps('8x0e+8x0e+4x1e'), Irreps('8x0e+4x1e'))      # two blocks of one linear onto one target
    b = ms.make_linear('b.weight', Irreps('8x0e+4x1e'), Irreps('8x0e+4x1e'))
    assert ms.plan_multi_source([a, b], False) is None
    c = ms.make_linear('c.weight', Irreps('8x0e+4x1e'), Irreps('8x0e+4x1e+2x2e'))      # another output side
    assert ms.plan_multi_source([b, c], False) is None
    launches, zero = ms.plan_multi_source([b, b], False)
    assert zero == [] and [[len(s) for _, _, _, s in probs] for _, probs in launches] == [[2, 2]]
    d = ms.make_linear('d.weight', Irreps('8x0e'), Irreps('8x0e+4x1e'))                # 1e untouched by d alone, written by b
    assert ms.plan_multi_source([d], False)[1] == [(8, 12)] and ms.plan_multi_source([d, b], False)[1] == []


def test_header_library_and_binding_name_the_entry_point_alike():
    from sevennet_amd import _lib
    with open(os.path.join(ROOT, 'include', 'snet_hip.h')) as f:
        hdr = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    m = re.search(r'int\s+snet_gemm_multi\s*\(([^;]*)\)\s*;', hdr)
    assert m, 'snet_gemm_multi is not declared in include/snet_hip.h'
    args = [a.strip() for a in m.group(1).split(',')]
    res, argtypes = _lib.SIGNATURES['snet_gemm_multi']
    assert res is C.c_int and len(argtypes) == len(args) == 9 and args[-1] == 'void *stream'
    assert int(re.search(r'#define SNET_GEMM_MAX_SRC (\d+)', hdr).group(1)) == ms.MAX_GEMM_SRC
    assert int(re.search(r'#define SNET_MAX_GEMM_GROUP (\d+)', hdr).group(1)) == ms.MAX_GEMM_GROUP
    # the ctypes structures mirror the C ones field for field (names in order; sizes of the natural layout)
    fields = lambda body: re.findall(r'(\w+)(?:\[\w+\])?\s*[;,]', body)   # noqa: E731
    src = re.search(r'typedef struct snet_gemm_src \{(.*?)\} snet_gemm_src;', hdr, flags=re.S).group(1)
    desc = re.search(r'typedef struct snet_gemm_multi_desc \{(.*?)\} snet_gemm_multi_desc;', hdr, flags=re.S).group(1)
    assert fields(src) == [n for n, _ in _lib.GemmSrc._fields_]
    assert fields(desc) == [n for n, _ in _lib.GemmMultiDesc._fields_]
    assert C.sizeof(_lib.GemmSrc) == 48 and C.sizeof(_lib.GemmMultiDesc) == 2 * 48 + 24
    assert int(re.search(r'#define SNET_ABI_VERSION (\d+)', hdr).group(1)) == _lib.ABI_VERSION == 4   # additive: the version stays
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(C.CDLL(_lib.LIB_PATH), 'snet_gemm_multi')
