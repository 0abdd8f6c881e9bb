"""CPU: the source and header lists of rag_application_amd/build.py against the files of csrc/.

The five host files (engine.hip, lifecycle.hip, paystore.hip, poolstage.hip, byexample.hip) share struct hx_index
through index.hpp.  A source
outside SOURCES is not linked; a header outside HEADERS leaves stale objects behind an edit to that struct, and the
translation units then disagree about its layout.  Needs no GPU and no compiler."""
from __future__ import annotations

import os
import re

from rag_application_amd import build as hxbuild

CSRC = hxbuild.CSRC
INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _headers():
    return {os.path.normpath(os.path.join(CSRC, h)) for h in hxbuild.HEADERS}


def test_every_source_file_is_built():
    on_disk = {f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp"))}
    listed = {s for s, _, _ in hxbuild.SOURCES}
    assert on_disk == listed
    objects = [o for _, o, _ in hxbuild.SOURCES]
    assert len(objects) == len(set(objects)), "two sources share an object file"


def test_every_header_is_a_dependency():
    root = os.path.dirname(os.path.dirname(CSRC))
    want = {os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")}
    want.add(os.path.join(root, "include", "hx.h"))
    assert want <= _headers(), sorted(want - _headers())
    assert all(os.path.isfile(h) for h in _headers())


def test_every_local_include_is_a_listed_header():
    headers = _headers()
    files = {os.path.join(CSRC, s) for s, _, _ in hxbuild.SOURCES} | headers
    seen = 0
    for path in sorted(files):
        for inc in INCLUDE.findall(open(path).read()):
            seen += 1
            target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            assert target in headers, f"{os.path.relpath(path, CSRC)} includes {inc}: not in build.HEADERS"
    assert seen > 0                               # (the walk did find include lines)
