#!/usr/bin/env python3
"""Generate tests/golden/lammps_reference_calls.json from the reference's LAMMPS-side sources.

tests/test_lammps_mock_pinned_cpu.py pins the LAMMPS mock (tests/lammps_mock/) and the pair-style glue (lammps/) to LAMMPS itself.
No LAMMPS tree is at hand, but the reference holds stock LAMMPS text and code written against the target release
(stable_2Aug2023_update3): its vendored sevenn/pair_e3gnn/comm_brick.{h,cpp} (LAMMPS' own CommBrick) and its pair styles
pair_e3gnn.cpp, pair_e3gnn_parallel.cpp, pair_d3.cu.  This script extracts from them, with the parser the test applies to the
glue, facts about the LAMMPS API only -- names, argument counts, argument types; no source text:

  comm_overrides              Comm entry points CommBrick overrides -> argument counts of their overloads
  comm_overrides_taking_pair  those with an overload whose one parameter is `class Pair *`
  pair_calls_from_comm        the four pack / unpack hooks of Pair that CommBrick calls -> argument counts at its call sites
  pair_hook_arg_types         argument types at the four pack / unpack call sites (from CommBrick's own declarations)
  lammps_uses                 [object, member, argument counts] of every LAMMPS singleton member the reference's pair styles and
                              CommBrick reach (a null count: data member access)
  pair_members_checked / pair_members_used
                              the Pair base members the test knows, and those the reference's pair styles use

Usage:  python oracle/tools/make_golden_lammps_calls.py <reference checkout>
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'tests', 'golden', 'lammps_reference_calls.json')

from test_lammps_mock_pinned_cpu import PAIR_MEMBERS, _args, _read, _strip, lammps_uses  # noqa: E402

HOOKS = ('pack_forward_comm', 'unpack_forward_comm', 'pack_reverse_comm', 'unpack_reverse_comm')


def _counts(s):
    """set of argument counts (None: data member) -> JSON list, data member last"""
    return sorted(c for c in s if c is not None) + ([None] if None in s else [])


def extract(ref_dir):
    rd = lambda *names: _read(*names, base=ref_dir)  # noqa: E731
    h, c = _strip(rd('comm_brick.h')), _strip(rd('comm_brick.cpp'))

    overrides, taking_pair = {}, set()
    for m in re.finditer(r'\bvoid\s+(\w+)\s*\(([^)]*)\)\s*override', h):
        overrides.setdefault(m.group(1), set()).add(len([a for a in m.group(2).split(',') if a.strip()]))
        if re.fullmatch(r'\s*class\s+Pair\s*\*\s*', m.group(2)):
            taking_pair.add(m.group(1))

    calls = {}
    for m in re.finditer(r'\bpair\s*->\s*(\w+)\s*\(', c):
        if m.group(1) in HOOKS:
            calls.setdefault(m.group(1), set()).add(_args(c, m.end() - 1))

    # argument TYPES at the stock call sites, from CommBrick's own member declarations (comm_brick.h): indexed once, an
    # `int *` member is an int and an `int **` member an int *; the buffers are double *
    def member_type(name):
        m = re.search(r'\b(int|double)\s*([^;]*?)(\*{0,2})\s*' + name + r'\b[^;]*;', h)
        if m is None:   # a local of the calling function (double *buf)
            m = re.search(r'\b(int|double)\s*(\*{0,2})\s*' + name + r'\s*;', c)
        assert m, name
        decl = re.search(r'(\*{0,2})\s*' + name + r'\b', m.group(0)).group(1)
        return m.group(1), len(decl)

    def arg_type(expr):
        base, idx = re.match(r'(\w+)((?:\[[^\]]*\])*)$', expr.strip()).groups()
        t, stars = member_type(base)
        stars -= idx.count('[')
        return t + (' ' + '*' * stars if stars else '')
    sites = {fn: re.search(r'pair\s*->\s*' + fn + r'\s*\(([^;]*?)\)\s*;', c).group(1).split(',') for fn in HOOKS}
    hook_types = {fn: ', '.join(arg_type(a) for a in args) for fn, args in sites.items()}

    uses = lammps_uses(rd('pair_e3gnn.cpp', 'pair_e3gnn_parallel.cpp', 'pair_d3.cu', 'pair_e3gnn.h', 'pair_e3gnn_parallel.h',
                          'pair_d3.h', 'comm_brick.cpp'))
    styles = _strip(rd('pair_e3gnn.cpp', 'pair_e3gnn_parallel.cpp', 'pair_d3.cu'))
    members_used = [m for m in PAIR_MEMBERS if re.search(r'(?<![\w>.])' + m + r'\b', styles)]
    return {
        '__about__': 'LAMMPS API facts (names, argument counts and types) extracted from the reference\'s vendored CommBrick '
                     '(comm_brick.h / .cpp) and its pair styles (pair_e3gnn.cpp, pair_e3gnn_parallel.cpp, pair_d3.cu + headers), '
                     'target release stable_2Aug2023_update3; written by oracle/tools/make_golden_lammps_calls.py',
        'comm_overrides': {k: _counts(v) for k, v in sorted(overrides.items())},
        'comm_overrides_taking_pair': sorted(taking_pair),
        'pair_calls_from_comm': {k: _counts(v) for k, v in sorted(calls.items())},
        'pair_hook_arg_types': hook_types,
        'lammps_uses': [[o, n, _counts(v)] for (o, n), v in sorted(uses.items())],
        'pair_members_checked': list(PAIR_MEMBERS),
        'pair_members_used': members_used,
    }


def main(argv):
    if len(argv) != 1:
        raise SystemExit(__doc__)
    ref_dir = os.path.join(argv[0], 'sevenn', 'pair_e3gnn')
    if not os.path.isdir(ref_dir):
        raise SystemExit(f'{ref_dir}: not a reference checkout')
    with open(OUT, 'w') as f:
        json.dump(extract(ref_dir), f, indent=1)
        f.write('\n')
    print(f'wrote {OUT}')


if __name__ == '__main__':
    main(sys.argv[1:])
