"""The object stamp of sevennet_amd/build.py covers every header of csrc/: a header that is edited or added makes the objects
stale without an entry anywhere (snet_system.h is included by eight translation units and named by no list)."""
import os

from sevennet_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_stamp_hashes_every_header_of_csrc(tmp_path, monkeypatch):
    (tmp_path / 'generated').mkdir()
    for name, text in (('a.hip', 'kernel'), ('one.h', '1'), ('two.h', '2'), ('generated/sh_generated.h', 'sh'), ('note.txt', 'x')):
        (tmp_path / name).write_text(text)
    monkeypatch.setattr(build, 'CSRC', str(tmp_path))
    src = str(tmp_path / 'a.hip')
    s0 = build._stamp(src)
    assert build._stamp(src) == s0
    (tmp_path / 'note.txt').write_text('y')          # not a header
    assert build._stamp(src) == s0
    (tmp_path / 'two.h').write_text('2 edited')
    s1 = build._stamp(src)
    assert s1 != s0
    (tmp_path / 'three.h').write_text('3')           # a new header is on the list at once
    s2 = build._stamp(src)
    assert s2 != s1
    (tmp_path / 'generated' / 'sh_generated.h').write_text('sh edited')
    assert build._stamp(src) != s2


def test_the_shared_device_header_is_where_the_build_looks():
    assert os.path.exists(os.path.join(build.CSRC, 'snet_system.h'))
    for f in ('snet_relax', 'snet_relax_cell', 'snet_mdstep', 'snet_mdnpt', 'snet_neb', 'snet_vib', 'snet_phonon', 'snet_elastic'):
        assert f + '.hip' in build.STATIC_SOURCES
        with open(os.path.join(build.CSRC, f + '.hip')) as fh:
            assert '#include "snet_system.h"' in fh.read()
