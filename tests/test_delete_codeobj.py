"""The compaction kernels of per-point deletes (compact.hip: the row gathers, the copies out of the bounce buffer, the
CSR kernels) in the shipped libhx.so use no scratch memory and spill no vector register -- the check test_codeobj.py
makes of the hot kernels.  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

COMPACT_KERNELS = ("k_compact_rows16", "k_compact_u32", "k_copy16", "k_copy_u32", "k_csr_keep_len", "k_csr_compact",
                   "k_csr_new_indptr")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_compaction_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    seen, bad = set(), []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            hit = [m for m in COMPACT_KERNELS if m in kn["name"]]
            if not hit:
                continue
            seen.update(hit)
            if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0:
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")))
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    assert seen == set(COMPACT_KERNELS), f"missing from the library: {set(COMPACT_KERNELS) - seen}"
