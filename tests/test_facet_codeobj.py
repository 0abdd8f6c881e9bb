"""The facet kernels (facet.hip: k_facet_count_u32 and k_facet_count_list in their LDS and global tiers, k_facet_keys with
and without the fold) are in the shipped libhx.so, use no scratch memory and spill no vector
register -- read from the code object's notes as tests/test_group_codeobj.py does -- and the LDS tier's histogram leaves
room for two workgroups per CU.  No GPU needed."""
from __future__ import annotations

import os
import re

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

PREFIX = "k_facet_"
CU_LDS = 160 * 1024
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hx.h")


def _lds_codes():
    return int(re.search(r"#define\s+HX_FACET_LDS_CODES\s+(\d+)", open(HDR).read()).group(1))


@pytest.fixture(scope="module")
def facet_kernels(tmp_path_factory):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    tmp = tmp_path_factory.mktemp("facet_codeobj")
    return [kn for k, blob in enumerate(_code_objects(lib)) for kn in _kernel_notes(blob, tmp, k) if PREFIX in kn["name"]]


def test_facet_kernels_have_no_scratch_and_no_vgpr_spills(facet_kernels):
    names = [kn["name"] for kn in facet_kernels]
    for base, forms in (("k_facet_count_u32", 2), ("k_facet_count_list", 2), ("k_facet_keys", 2)):
        assert sum(base in n for n in names) == forms, (base, names)
    bad = [(kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")) for kn in facet_kernels
           if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0]
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"


def test_the_lds_tier_leaves_room_for_two_workgroups_per_cu(facet_kernels):
    hist = 4 * _lds_codes()
    tiers = {"lds": [], "global": []}
    for kn in facet_kernels:
        if "k_facet_count" in kn["name"]:
            tiers["lds" if int(kn["group_segment_fixed_size"]) >= hist else "global"].append(kn)
    assert len(tiers["lds"]) == 2 and len(tiers["global"]) == 2, {t: [k["name"] for k in v] for t, v in tiers.items()}
    for kn in tiers["lds"]:
        assert int(kn["group_segment_fixed_size"]) <= CU_LDS // 2, (kn["name"], kn["group_segment_fixed_size"])
        # two workgroups per CU fit the registers too: 1024 threads (the scalar kernel) are 4 waves per SIMD, 512 are 2
        assert int(kn["vgpr_count"]) <= (64 if "k_facet_count_u32" in kn["name"] else 128), (kn["name"], kn["vgpr_count"])
    for kn in tiers["global"]:
        assert int(kn["group_segment_fixed_size"]) < 8 * 1024, (kn["name"], kn["group_segment_fixed_size"])
