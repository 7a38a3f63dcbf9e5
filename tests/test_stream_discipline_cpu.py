"""Static guard of the stream contract ("Stream contract"): all device work of a call is ordered on the stream the
caller passes.  No GPU: the sources and the text the generators emit are read as text, the Python layer by AST.

  * every kernel launch names a stream (a fourth `<<<...>>>` argument that is not the null stream), and so does every
    hipMemsetAsync / hipMemcpyAsync / hipStreamSynchronize (last argument);
  * the host-blocking / null-stream calls hipMemcpy, hipMemset and hipDeviceSynchronize occur only inside the plan- and
    model-construction functions listed below, by name;
  * no Python call of an entry point whose last parameter is the stream passes the constant None for it.

tests/test_stream_order_*_gpu.py check the same property dynamically on the device."""
import ast
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sevennet_amd', 'csrc')
NULL_STREAMS = {'0', 'nullptr', 'NULL', '0u', 'hipStreamLegacy', 'hipStreamPerThread', '(hipStream_t)0', 'hipStream_t(0)',
                'static_cast<hipStream_t>(0)', 'static_cast<hipStream_t>(nullptr)'}
BLOCKING = ('hipMemcpy(', 'hipMemset(', 'hipDeviceSynchronize(')
STREAM_LAST = ('hipMemsetAsync', 'hipMemcpyAsync', 'hipStreamSynchronize')     # runtime calls whose last argument is the stream

# (file, enclosing function) -> why a host-blocking copy is in order there.  All of them build a plan or a model: they run once,
# before any launch that reads what they upload, and a pageable hipMemcpy has completed when it returns.
BLOCKING_ALLOWED = {
    ('snet_layer0.hip', 'upload_packed'): 'snet_layer0_plan_create: the folded layer-0 weights',
    ('snet_lastlayer.hip', 'snet_lastlayer_plan_create'): 'the last-layer kernel\'s weight image',
    ('snet_model.cpp', 'dev_upload'): 'snet_model_load_memory: fp32 tables',
    ('snet_model.cpp', 'upload_split'): 'snet_model_load_memory: packed GEMM weights',
    ('snet_model.cpp', 'snet_model_load_memory'): 'chunk order, readout vector, the constant one',
    ('snet_model.cpp', 'layer0_select'): 'first evaluation of a species set: its layer-0 plan\'s slot table',
    ('snet_halo.cpp', 'upload'): 'snet_halo_create: index lists',
    ('snet_mlp.hip', 'upload'): 'snet_radial_mlp_plan_create / pack_fused_slabs: weight fragments',
}


def _static_sources():
    out = {}
    for pat in ('*.hip', '*.cpp', '*.h'):
        for p in sorted(glob.glob(os.path.join(CSRC, pat))):
            with open(p) as f:
                out[os.path.basename(p)] = f.read()
    assert len(out) >= 20
    return out


def _generated_sources():
    """the text codegen.py / codegen_fused.py emit for every ahead-of-time shape (what build() compiles)"""
    from sevennet_amd import codegen, codegen_fused
    from sevennet_amd.shapes import aot_conv_specs, lastlayer_test_configs
    out = {'sh_generated.h': codegen.gen_sh_header(3)}
    for tag, spec in aot_conv_specs(list(lastlayer_test_configs().values())).items():
        out[f'conv_{tag}.hip'] = codegen.gen_conv(spec)
        if codegen_fused.fusable(spec):
            out[f'convf_{tag}.hip'] = codegen_fused.gen_conv_fused(spec)
            out[f'convft_{tag}.hip'] = codegen_fused.gen_conv_fused_tangent(spec)
    assert any(k.startswith('convft_') for k in out)
    return out


@pytest.fixture(scope='module')
def sources():
    return {**_static_sources(), **_generated_sources()}


def _strip_comments(text):
    """C++ text with comments blanked (same length, newlines kept)"""
    def blank(m):
        return re.sub(r'[^\n]', ' ', m.group(0))
    return re.sub(r'//[^\n]*|/\*.*?\*/', blank, text, flags=re.S)


def launch_configs(text):
    """[(line, [launch arguments])] of every <<<...>>> of `text`"""
    out = []
    text = _strip_comments(text)
    for m in re.finditer(r'<<<', text):
        i, depth, args, cur = m.end(), 0, [], ''
        while not (depth == 0 and text.startswith('>>>', i)):
            assert i < len(text), 'unterminated launch configuration'
            ch = text[i]
            depth += ch in '([{'
            depth -= ch in ')]}'
            if ch == ',' and depth == 0:
                args.append(cur.strip())
                cur = ''
            else:
                cur += ch
            i += 1
        out.append((text.count('\n', 0, m.start()) + 1, args + [cur.strip()]))
    return out


_HEAD = re.compile(r'^(?:  )?(?!(?:if|for|while|switch|return|else|do|case|namespace|struct|class|using|typedef|template)\b)'
                   r'[A-Za-z_][\w:<>,\*& "]*?[\s\*&](\w+)\((?:[^;]*)$')


def enclosing_function(text, pos):
    """name of the function whose body holds text[pos]: the nearest earlier line, at an indentation of 0 (free function) or 2
    (member function), that opens a definition `type name(...` and is not a statement"""
    lines = text[:pos].split('\n')
    for k in range(len(lines) - 1, -1, -1):
        m = _HEAD.match(lines[k])
        if m and not lines[k].rstrip().endswith(';'):
            return m.group(1)
    return None


def blocking_calls(sources):
    found = []
    for name, raw in sources.items():
        text = _strip_comments(raw)
        for what in BLOCKING:
            for m in re.finditer(r'(?<![\w])' + re.escape(what), text):
                found.append((name, enclosing_function(text, m.start()), what, text.count('\n', 0, m.start()) + 1))
    return found


def test_every_launch_names_a_stream(sources):
    n = 0
    for name, text in sources.items():
        for line, args in launch_configs(text):
            n += 1
            assert len(args) == 4, f'{name}:{line}: <<<{", ".join(args)}>>> names no stream'
            assert re.sub(r'\s+', '', args[3]) not in {re.sub(r'\s+', '', s) for s in NULL_STREAMS}, \
                f'{name}:{line}: launch on the null stream'
    assert n >= 98   # the static sources alone hold that many: the scan found them


def call_arguments(text, name):
    """[(line, [arguments])] of every call `name(...)` of `text`"""
    out = []
    text = _strip_comments(text)
    for m in re.finditer(r'(?<![\w])' + re.escape(name) + r'\(', text):
        i, depth, args, cur = m.end(), 0, [], ''
        while not (depth == 0 and text[i] == ')'):
            ch = text[i]
            depth += ch in '([{'
            depth -= ch in ')]}'
            if ch == ',' and depth == 0:
                args.append(cur.strip())
                cur = ''
            else:
                cur += ch
            i += 1
            assert i < len(text), 'unterminated call'
        out.append((text.count('\n', 0, m.start()) + 1, args + [cur.strip()]))
    return out


def test_async_runtime_calls_name_a_stream(sources):
    null = {re.sub(r'\s+', '', s) for s in NULL_STREAMS}
    n = 0
    for name, text in sources.items():
        for fn in STREAM_LAST:
            for line, args in call_arguments(text, fn):
                n += 1
                assert len(args) == {'hipMemsetAsync': 4, 'hipMemcpyAsync': 5, 'hipStreamSynchronize': 1}[fn], (name, line, args)
                assert re.sub(r'\s+', '', args[-1]) not in null, f'{name}:{line}: {fn} on the null stream'
    assert n >= 25   # the scan found the call sites
    assert call_arguments('ok = hipMemsetAsync(p, 0, (size_t)N * f(a, b),\n 0) == hipSuccess;', 'hipMemsetAsync')[0][1][-1] == '0'


def test_launch_parser_sees_what_it_should():
    """the scanner on text that breaks the rule"""
    assert launch_configs('k<<<g, b>>>(x);')[0][1] == ['g', 'b']
    assert launch_configs('k<T><<<dim3(a, 1), f(b, c),\n 0, 0>>>(x);')[0][1] == ['dim3(a, 1)', 'f(b, c)', '0', '0']
    assert launch_configs('// k<<<g, b>>>(x);\nk<<<g, b, 0, static_cast<hipStream_t>(s)>>>(x);')[0][1][3] == 'static_cast<hipStream_t>(s)'
    text = 'namespace {\nint f(int a,\n      int b) {\n  if (a) {\n    hipMemcpy(x);\n  }\n}\nstruct S {\n  bool up(const T &h) {\n    return hipMemcpy(y);\n  }\n};\n}\n'
    assert [c[1] for c in blocking_calls({'t.cpp': text})] == ['f', 'up']


def test_blocking_copies_only_in_construction(sources):
    found = blocking_calls(sources)
    where = {(f, fn) for f, fn, _, _ in found}
    stray = sorted(c for c in found if (c[0], c[1]) not in BLOCKING_ALLOWED)
    assert not stray, f'host-blocking / null-stream call outside plan or model construction: {stray}'
    # ... and the list is exact: an entry nobody needs any more is removed with the code
    assert where == set(BLOCKING_ALLOWED), sorted(set(BLOCKING_ALLOWED) - where)


def _stream_last_entry_points():
    """names of SIGNATURES (sevennet_amd/_lib.py) whose argument list ends in `c_stream`, read from the source: c_stream is an
    alias of c_void_p, so the loaded table cannot tell"""
    with open(os.path.join(ROOT, 'sevennet_amd', '_lib.py')) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == 'SIGNATURES' for t in node.targets):
            for k, v in zip(node.value.keys, node.value.values):
                args = v.elts[1].elts
                if args and isinstance(args[-1], ast.Name) and args[-1].id == 'c_stream':
                    names.add(k.value)
    return names


def none_stream_calls(tree, entry_points):
    bad = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in entry_points and node.args:
            last = node.args[-1]
            if not node.keywords and isinstance(last, ast.Constant) and last.value is None:
                bad.append((node.func.attr, node.lineno))
    return bad


def test_python_layer_never_passes_a_null_stream():
    eps = _stream_last_entry_points()
    assert {'snet_act_fwd', 'snet_model_eval', 'snet_fire_step', 'snet_d3_compute_device', 'snet_md_compute'} <= eps and len(eps) >= 70
    assert 'snet_model_load' not in eps and 'snet_gemm_split_pack' not in eps
    assert none_stream_calls(ast.parse('lib.snet_act_fwd(a, b, n, 0, 1.0, None)\nself.lib.snet_act_fwd(a, b, n, 0, 1.0, st)'), eps) == \
        [('snet_act_fwd', 1)]
    n_calls = 0
    for p in sorted(glob.glob(os.path.join(ROOT, 'sevennet_amd', '*.py'))):
        with open(p) as f:
            tree = ast.parse(f.read())
        n_calls += sum(isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in eps for n in ast.walk(tree))
        assert not none_stream_calls(tree, eps), (os.path.basename(p), none_stream_calls(tree, eps))
    assert n_calls >= 60   # the walk found the package's calls
