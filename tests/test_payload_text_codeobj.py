"""The text matcher of the payload index (paytext.hip: k_payload_text) is in the shipped libhx.so
and uses no scratch memory and spills no vector register; k_payload_mask, which gained the device-only plane op, still
has neither -- read from the code object's notes as tests/test_payload_lists_codeobj.py does.  Both stay at or below 64
VGPRs: a SIMD of gfx950 holds 512 per lane, so 64 is the most a kernel may use and still run 8 waves per SIMD, the
occupancy k_payload_mask had before it gained the op (DESIGN.md sections 17 and 19).  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

TEXT_KERNELS = ("k_payload_text", "k_payload_mask")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_text_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    seen, bad, vgprs = set(), [], {}
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            hit = [m for m in TEXT_KERNELS if m in kn["name"]]
            if not hit:
                continue
            seen.update(hit)
            vgprs[hit[0]] = max(vgprs.get(hit[0], 0), int(kn["vgpr_count"]))
            if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0:
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")))
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    assert seen == set(TEXT_KERNELS), f"missing from the library: {set(TEXT_KERNELS) - seen}"
    assert all(v <= 64 for v in vgprs.values()), f"more than 64 VGPRs (fewer than 8 waves per SIMD): {vgprs}"
