"""CPU: pin the LAMMPS MOCK (tests/lammps_mock/) to LAMMPS itself.

The glue (lammps/pair_e3gnn_hip.cpp, pair_d3_hip.cpp) is compiled and executed against a mock this repository wrote, so a signature
that differs from LAMMPS would compile here and fail for the first user.  No LAMMPS tree is at hand, but the reference
holds stock LAMMPS text and code written against the target release (stable_2Aug2023_update3): the vendored
sevenn/pair_e3gnn/comm_brick.{h,cpp} (LAMMPS' own CommBrick) and the reference's pair styles pair_e3gnn.cpp,
pair_e3gnn_parallel.cpp, pair_d3.cu.  oracle/tools/make_golden_lammps_calls.py extracted from them, with the parser below, every
LAMMPS call and member access those sources make (names and argument counts only: tests/golden/lammps_reference_calls.json), and
this test checks:
  * the mock declares CommBrick's entry points and the pair-side hooks with the argument lists stock LAMMPS calls them with;
  * every LAMMPS call / member the GLUE uses is one the reference's sources use too, with the same number of arguments --
    whatever is not is exactly the list INTEGRATION.md publishes as unverified."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'lammps_reference_calls.json')

OBJECTS = ('memory', 'error', 'atom', 'comm', 'neighbor', 'domain', 'force', 'list', 'utils', 'NeighConst')
# unqualified members inherited from LAMMPS' Pair that the mock declares (the fixture records which of them the reference uses)
PAIR_MEMBERS = ('eng_vdwl', 'eng_coul', 'virial', 'eatom', 'vatom', 'comm_forward', 'comm_reverse', 'single_enable', 'restartinfo',
                'one_coeff', 'manybody_flag', 'no_virial_fdotr_compute', 'list', 'allocated', 'setflag', 'cutsq', 'map', 'eflag_either',
                'eflag_global', 'eflag_atom', 'vflag_either', 'vflag_global', 'vflag_atom', 'ev_setup', 'evflag', 'vflag_fdotr',
                'maxeatom', 'maxvatom')


def _reference():
    with open(GOLDEN) as f:
        return json.load(f)


def _strip(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    return re.sub(r'"(?:\\.|[^"\\])*"', '""', text)


def _args(text, k):
    """text[k] == '(' -> number of top-level arguments of the call"""
    depth, n, seen = 0, 0, False
    for ch in text[k:]:
        if ch in '([{':
            depth += 1
        elif ch in ')]}':
            depth -= 1
            if depth == 0:
                return n + (1 if seen else 0)
        elif ch == ',' and depth == 1:
            n += 1
        elif depth >= 1 and not ch.isspace():
            seen = True
    raise AssertionError('unbalanced call')


def lammps_uses(text):
    """{(object, name): set of argument counts, or {None} for a data member} over the LAMMPS singletons a pair style reaches"""
    text = _strip(text)
    out = {}
    for m in re.finditer(r'\b(' + '|'.join(OBJECTS) + r')\s*(?:->|::)\s*(\w+)\s*(\()?', text):
        key = (m.group(1), m.group(2))
        out.setdefault(key, set()).add(_args(text, m.end() - 1) if m.group(3) else None)
    return out


def _read(*names, base):
    return '\n'.join(open(os.path.join(base, n)).read() for n in names)


def test_comm_brick_entry_points_and_pair_hooks_match_stock_lammps():
    """stock LAMMPS (the reference's vendored CommBrick): Comm::forward_comm(Pair *) / reverse_comm(Pair *) and the four pair-side hooks
    with the arguments CommBrick passes them; the mock's Comm / Pair must declare exactly those"""
    ref = _reference()
    assert {'forward_comm', 'reverse_comm'} <= set(ref['comm_overrides_taking_pair'])
    calls = {fn: set(n) for fn, n in ref['pair_calls_from_comm'].items()}
    assert calls['pack_forward_comm'] == {5} and calls['unpack_forward_comm'] == {3}
    assert calls['pack_reverse_comm'] == {3} and calls['unpack_reverse_comm'] == {3}
    # argument TYPES at the stock call sites, from CommBrick's own member declarations (the generator's member_type / arg_type)
    want = ref['pair_hook_arg_types']
    assert want == {'pack_forward_comm': 'int, int *, double *, int, int *', 'unpack_forward_comm': 'int, int, double *',
                    'pack_reverse_comm': 'int, int, double *', 'unpack_reverse_comm': 'int, int *, double *'}, want
    norm = lambda s_: re.sub(r'\s+', ' ', re.sub(r'\s*\*\s*', ' *', s_)).strip()  # noqa: E731
    mock = _strip(_read('pair.h', 'lmp_mock_core.h', base=os.path.join(ROOT, 'tests', 'lammps_mock')))
    for fn, sig in want.items():
        m = re.search(r'virtual\s+(?:int|void)\s+' + fn + r'\s*\(([^)]*)\)', mock)
        assert m and norm(m.group(1)) == norm(sig), (fn, m and m.group(1))
    assert re.search(r'virtual\s+void\s+forward_comm\s*\(\s*Pair\s*\*\s*\)', mock) and re.search(r'virtual\s+void\s+reverse_comm\s*\(\s*Pair\s*\*\s*\)', mock)
    # ... and the glue overrides them with the same lists
    glue_h = _strip(_read('pair_e3gnn_hip.h', base=os.path.join(ROOT, 'lammps')))
    for fn in ('pack_forward_comm', 'unpack_forward_comm'):
        m = re.search(r'\b(?:int|void)\s+' + fn + r'\s*\(([^)]*)\)\s*override', glue_h)
        assert m and norm(m.group(1)) == norm(want[fn]), (fn, m and m.group(1))


def _unverified_block():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    m = re.search(r'<!-- lammps-unverified:begin -->(.*?)<!-- lammps-unverified:end -->', text, flags=re.S)
    assert m, 'INTEGRATION.md lost its lammps-unverified block'
    return set(re.findall(r'`(\w+(?:->|::)\w+)`', m.group(1)))


def test_every_lammps_call_of_the_glue_is_one_the_reference_makes():
    ref = {(o, n): set(counts) for o, n, counts in _reference()['lammps_uses']}
    # stock Comm entry points declared in the vendored header count as LAMMPS text too (the reference itself calls its own overloads)
    for name, counts in _reference()['comm_overrides'].items():
        ref.setdefault(('comm', name), set()).update(counts)
    glue = lammps_uses(_read('pair_e3gnn_hip.cpp', 'pair_e3gnn_hip.h', 'pair_d3_hip.cpp', 'pair_d3_hip.h', base=os.path.join(ROOT, 'lammps')))
    assert len(glue) >= 20 and ('memory', 'create') in glue and ('neighbor', 'add_request') in glue
    unverified, arity = set(), []
    for key, counts in sorted(glue.items()):
        sep = '::' if key[0] in ('utils', 'NeighConst') else '->'
        name = f'{key[0]}{sep}{key[1]}'
        if key not in ref:
            unverified.add(name)
            continue
        extra = {c for c in counts if c is not None} - {c for c in ref[key] if c is not None}
        if key == ('utils', 'logmesg'):
            extra = set()                       # variadic ({fmt} arguments)
        if extra:
            arity.append((name, sorted(extra), sorted(c for c in ref[key] if c is not None)))
    assert arity == [], f'called with argument counts the reference never uses: {arity}'
    assert unverified == {u for u in _unverified_block() if not u.startswith('Pair::')}, (sorted(unverified), sorted(_unverified_block()))
    # the mock declares everything the glue reaches (it compiles against it: tests/test_lammps_glue_cpu.py); here: every name exists
    mock = _strip(_read('pair.h', 'lmp_mock_core.h', 'mpi.h', base=os.path.join(ROOT, 'tests', 'lammps_mock')))
    for (obj, name) in glue:
        assert re.search(r'\b' + name + r'\b', mock), (obj, name)


def test_pair_base_members_the_glue_uses_are_the_ones_the_reference_uses():
    """unqualified members inherited from LAMMPS' Pair (flags, accumulators, ev_setup): the mock declares them; the glue may use
    only those the reference's pair styles use too"""
    mock = _strip(_read('pair.h', base=os.path.join(ROOT, 'tests', 'lammps_mock')))
    body = mock[mock.index('class Pair'):]
    members = PAIR_MEMBERS
    for m in members:
        assert re.search(r'\b' + m + r'\b', body), m                 # the list above is what the mock's Pair declares
    ref = _reference()
    assert ref['pair_members_checked'] == list(members), 'the member list changed: regenerate the fixture'
    glue = _strip(_read('pair_e3gnn_hip.cpp', 'pair_d3_hip.cpp', base=os.path.join(ROOT, 'lammps')))
    used = {m for m in members if re.search(r'(?<![\w>.])' + m + r'\b', glue)}
    assert {'eng_vdwl', 'virial', 'setflag', 'cutsq', 'ev_setup', 'evflag', 'vflag_fdotr'} <= used
    missing = {'Pair::' + m for m in used if m not in ref['pair_members_used']}
    # (the reference adds its energy / virial unconditionally; the glue honours LAMMPS' global flags)
    assert missing == {u for u in _unverified_block() if u.startswith('Pair::')}, sorted(missing)
