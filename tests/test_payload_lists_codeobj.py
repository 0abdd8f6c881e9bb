"""The kernels the list columns of the payload index add or touch (payload.hip: k_payload_mask with the list ops;
compact.hip: k_csr_compact_u32, the element copy of hx_retain_rows) use no scratch memory and spill no vector register
in the shipped libhx.so -- read from the code object's notes as tests/test_payload_codeobj.py does.  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

LIST_KERNELS = ("k_payload_mask", "k_csr_compact_u32")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_list_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    seen, bad = set(), []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            hit = [m for m in LIST_KERNELS if m in kn["name"]]
            if not hit:
                continue
            seen.update(hit)
            if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0:
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")))
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    assert seen == set(LIST_KERNELS), f"missing from the library: {set(LIST_KERNELS) - seen}"
