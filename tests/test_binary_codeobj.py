"""The kernels of binary quantization -- k_bin_scan in its four query-group forms (binscan.hip) and
k_binarize_rows (prep.hip) -- are in the shipped libhx.so, use no scratch memory and spill no vector register -- read from
the code object's notes as tests/test_fusion_codeobj.py does -- and their static LDS stays inside 64 KB (the scan's tile is
dynamic LDS, at most 52 KB by construction: BIN_PASS_SLOTS; the staged query words are 4 KB of static LDS).  The five entries are declared, bound and exported, and the
ABI version is still 3.  No GPU needed."""
from __future__ import annotations

import ctypes as C
import os

import pytest

from tests.test_abi import declared_functions
from tests.test_codeobj import READELF, _code_objects, _kernel_notes

ENTRIES = ("hx_binary_enable", "hx_binary_enabled", "hx_binary_debug_row", "hx_search_bin", "hx_search_bin_masked")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_binary_kernels_have_no_scratch_no_vgpr_spills_and_fit_64k_of_lds(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    found = {"k_bin_scan": [], "k_binarize_rows": [], "k_bin_queries": [], "k_bin_tau": []}
    bad = []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            for want in found:
                if want in kn["name"]:
                    found[want].append(kn)
                    if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0:
                        bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")))
                    assert int(kn["group_segment_fixed_size"]) <= 64 * 1024, (kn["name"], kn["group_segment_fixed_size"])
                    assert int(kn["vgpr_count"]) <= 128, (kn["name"], kn["vgpr_count"])
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    names = sorted(kn["name"] for kn in found["k_bin_scan"])
    assert len(names) == 4 and all(f"ILi{q}E" in n for q, n in zip((1, 2, 4, 8), names)), names
    for want in ("k_binarize_rows", "k_bin_queries", "k_bin_tau"):
        assert len(found[want]) == 1, (want, [kn["name"] for kn in found[want]])


def test_the_binary_entries_are_declared_bound_and_exported():
    from rag_application_amd import _lib
    from rag_application_amd import build as hxbuild
    for n in ENTRIES:
        assert n in declared_functions() and n in _lib.EXPORTS, n
    assert sorted(_lib.EXPORTS) == declared_functions()
    assert len(_lib._SIGS["hx_search_bin"]) == 7 and len(_lib._SIGS["hx_search_bin_masked"]) == 9
    assert len(_lib._SIGS["hx_binary_debug_row"]) == 4
    cdll = C.CDLL(hxbuild.build(force=False))
    for n in ENTRIES:
        assert hasattr(cdll, n), n
    assert cdll.hx_abi_version() == 3
