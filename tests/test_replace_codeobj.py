"""The kernels of upsert by an existing id (replace.hip: the row scatters, the CSR splice for the sparse vectors and for
the list columns) in the shipped libhx.so use no scratch memory and spill no vector register -- the check
test_delete_codeobj.py makes of the compaction kernels, from the same metadata notes.  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

REPLACE_KERNELS = ("k_scatter_rows16", "k_scatter_u32", "k_csr_splice_len", "k_csr_splice", "k_csr_splice_u32")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_replace_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    seen, bad = {}, []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            hit = [m for m in REPLACE_KERNELS if m in kn["name"]]
            if not hit:
                continue
            for m in hit:
                seen.setdefault(m, []).append(kn["name"])
            if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0:
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")))
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    assert set(seen) == set(REPLACE_KERNELS), f"missing from the library: {set(REPLACE_KERNELS) - set(seen)}"
    # k_csr_splice names three kernels (itself, _len, _u32): each was met on its own
    assert len(seen["k_csr_splice"]) == 3, seen["k_csr_splice"]
