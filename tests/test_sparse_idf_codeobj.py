"""The three kernels of the sparse statistics (spstats.hip: k_sparse_df, k_sparse_rows_nonempty, k_sparse_idf; DESIGN.md
section 31) are in the shipped libhx.so, use no scratch memory, spill no scalar or vector register and keep their static
LDS inside 64 KB -- read from the code object's notes as tests/test_fusion_codeobj.py does.  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

KERNELS = ("k_sparse_df", "k_sparse_rows_nonempty", "k_sparse_idf")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_statistics_kernels_have_no_scratch_no_spills_and_little_lds(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    found = {}
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            for want in KERNELS:
                if want + "E" in kn["name"] or kn["name"].endswith(want):     # (mangled: <len>name E ...)
                    found.setdefault(want, []).append(kn)
    assert sorted(found) == sorted(KERNELS), f"kernels found: {sorted(found)}"
    for want, kns in found.items():
        assert len(kns) == 1, (want, [kn["name"] for kn in kns])
        kn = kns[0]
        assert int(kn.get("private_segment_fixed_size", "0")) == 0, (want, kn)
        assert int(kn.get("vgpr_spill_count", "0")) == 0 and int(kn.get("sgpr_spill_count", "0")) == 0, (want, kn)
        assert int(kn["group_segment_fixed_size"]) <= 64 * 1024, (want, kn)
    # the search needs no LDS at all, the count one word per workgroup, the weights none
    assert int(found["k_sparse_df"][0]["group_segment_fixed_size"]) == 0
    assert int(found["k_sparse_rows_nonempty"][0]["group_segment_fixed_size"]) <= 64
    assert int(found["k_sparse_idf"][0]["group_segment_fixed_size"]) == 0
