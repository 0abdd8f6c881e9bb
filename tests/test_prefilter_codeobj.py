"""The kernels of the pre-filtered query (mask.hip: the row list, the gathers, the id map; the masked variants of the
sparse select pass and of the document-at-a-time kernel) in the shipped libhx.so use no scratch memory and spill no vector
register -- the check test_codeobj.py makes of the hot kernels -- and the unmasked sparse select pass keeps its register
budget.  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

MASK_KERNELS = ("k_mask_count", "k_mask_offsets", "k_mask_rows", "k_gather_rows16", "k_gather_u32", "k_view_ids")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_mask_and_gather_kernels_have_no_scratch_and_no_vgpr_spills(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    seen, bad = set(), []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            hit = [m for m in MASK_KERNELS if m in kn["name"]]
            if not hit:
                continue
            seen.update(hit)
            if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0:
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")))
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    assert seen == set(MASK_KERNELS), f"missing from the library: {set(MASK_KERNELS) - seen}"


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_both_variants_of_the_sparse_kernels_and_no_scratch(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    found = {}
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            for base in ("k_sparse_select", "k_sparse_range"):
                if base in kn["name"]:
                    variant = "masked" if "ILb1E" in kn["name"] else "plain" if "ILb0E" in kn["name"] else "?"
                    found.setdefault((base, variant), []).append(kn)
    for base, n_seg in (("k_sparse_select", 2), ("k_sparse_range", 1)):
        for variant in ("plain", "masked"):
            kns = found.get((base, variant), [])
            assert len(kns) == n_seg, (base, variant, len(kns))      # the select pass: both segment sizes
            for kn in kns:
                assert int(kn.get("private_segment_fixed_size", "0")) == 0 and int(kn.get("vgpr_spill_count", "0")) == 0
    # the masked select pass does not change the occupancy of the plain one: same LDS, VGPRs within the same budget
    for plain, masked in zip(sorted(found[("k_sparse_select", "plain")], key=lambda k: k["group_segment_fixed_size"]),
                             sorted(found[("k_sparse_select", "masked")], key=lambda k: k["group_segment_fixed_size"])):
        assert plain["group_segment_fixed_size"] == masked["group_segment_fixed_size"]
