"""The kernels of the nested blocks of the payload index (paynested.hip: k_payload_nested, the per-element conjunction, and
k_payload_same_offsets, the alignment check) are in the shipped libhx.so, use no scratch memory and spill no scalar and no
vector register -- read from the code object's notes as tests/test_payload_lists_codeobj.py does.  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

NESTED_KERNELS = ("k_payload_nested", "k_payload_same_offsets")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_nested_kernels_have_no_scratch_and_no_spills(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    seen, bad = set(), []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            hit = [m for m in NESTED_KERNELS if m in kn["name"]]
            if not hit:
                continue
            seen.update(hit)
            if (int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0
                    or int(kn.get("sgpr_spill_count", "0")) != 0):
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count"),
                            kn.get("sgpr_spill_count")))
    assert not bad, f"kernels with scratch / spilled registers: {bad}"
    assert seen == set(NESTED_KERNELS), f"missing from the library: {set(NESTED_KERNELS) - seen}"
