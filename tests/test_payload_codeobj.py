"""The payload index's kernel (payload.hip: k_payload_mask) in the shipped libhx.so uses no scratch memory and spills no
vector register -- the check test_codeobj.py makes of the hot kernels.  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

PAYLOAD_KERNELS = ("k_payload_mask",)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_payload_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    seen, bad = set(), []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            hit = [m for m in PAYLOAD_KERNELS if m in kn["name"]]
            if not hit:
                continue
            seen.update(hit)
            if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0:
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")))
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    assert seen == set(PAYLOAD_KERNELS), f"missing from the library: {set(PAYLOAD_KERNELS) - seen}"
