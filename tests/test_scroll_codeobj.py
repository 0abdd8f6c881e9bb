"""The scroll kernels (scroll.hip: k_order_init, k_order_hist in its two forms, k_order_pick, k_order_sort, and
k_first_count / k_first_prefix / k_first_emit in their two forms) are in the shipped libhx.so, use
no scratch memory, spill no register and keep their static LDS within 64 KB -- read from the code object's notes as
tests/test_facet_codeobj.py does.  No GPU needed."""
from __future__ import annotations

import os

import pytest

from tests.test_codeobj import READELF, _code_objects, _kernel_notes

PREFIXES = ("k_order_", "k_first_")
FORMS = (("k_order_init", 1), ("k_order_hist", 2), ("k_order_pick", 1), ("k_order_sort", 1), ("k_first_count", 2),
         ("k_first_prefix", 2), ("k_first_emit", 2))


@pytest.fixture(scope="module")
def scroll_kernels(tmp_path_factory):
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not found")
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    tmp = tmp_path_factory.mktemp("scroll_codeobj")
    return [kn for k, blob in enumerate(_code_objects(lib)) for kn in _kernel_notes(blob, tmp, k)
            if any(p in kn["name"] for p in PREFIXES)]


def test_every_scroll_kernel_is_in_the_library(scroll_kernels):
    names = [kn["name"] for kn in scroll_kernels]
    for base, forms in FORMS:
        assert sum(base in n for n in names) == forms, (base, names)


def test_scroll_kernels_have_no_scratch_and_no_spills(scroll_kernels):
    bad = [(kn["name"], kn.get("private_segment_fixed_size"), kn.get("sgpr_spill_count"), kn.get("vgpr_spill_count"))
           for kn in scroll_kernels
           if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("sgpr_spill_count", "0")) != 0 or
           int(kn.get("vgpr_spill_count", "0")) != 0]
    assert scroll_kernels and not bad, f"kernels with scratch / spilled registers: {bad}"


def test_scroll_kernels_keep_static_lds_within_64_kb(scroll_kernels):
    sizes = {kn["name"]: int(kn["group_segment_fixed_size"]) for kn in scroll_kernels}
    assert sizes and all(v <= 64 * 1024 for v in sizes.values()), sizes
