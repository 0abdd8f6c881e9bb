"""The kernel of the score-boosting search (formula.hip: k_formula) is in the shipped libhx.so, uses
no scratch memory -- the fp64 stack lives in LDS, not in a private array -- and spills no scalar or vector register, read
from the code object's notes as tests/test_reco_codeobj.py does; its static LDS (the stack, the sort keys of a 2048-key
pool, the program) stays inside a CU's 160 KB.  The two ABI entries are declared, bound and exported.  No GPU needed."""
from __future__ import annotations

import ctypes as C
import os

import pytest

from tests.test_abi import declared_functions
from tests.test_codeobj import READELF, _code_objects, _kernel_notes

KERNEL = "k_formula"


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_formula_kernel_has_no_scratch_no_spills_and_fits_the_lds(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    found, bad = [], []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            if KERNEL not in kn["name"]:
                continue
            found.append(kn)
            if (int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0
                    or int(kn.get("sgpr_spill_count", "0")) != 0):
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count"),
                            kn.get("sgpr_spill_count")))
    assert len(found) == 1, f"want one {KERNEL}, found {[kn['name'] for kn in found]}"
    assert not bad, f"kernels with scratch / spilled registers: {bad}"
    kn = found[0]
    lds = int(kn["group_segment_fixed_size"])
    assert lds <= 160 * 1024, lds
    assert lds >= 16 * 256 * 8 + 2048 * 8, lds            # the [depth][thread] stack and the sort keys are in it
    assert int(kn["vgpr_count"]) <= 128, kn["vgpr_count"]  # 256 threads: room for more than one workgroup per SIMD
    print(KERNEL, "lds", lds, "vgprs", kn["vgpr_count"])


def test_the_two_entries_are_declared_bound_and_exported():
    from rag_application_amd import _lib
    from rag_application_amd import build as hxbuild
    new = {"hx_formula", "hx_hybrid_query_formula_host"}
    assert new <= set(declared_functions()) and new <= set(_lib.EXPORTS)
    assert sorted(_lib.EXPORTS) == declared_functions()
    cdll = C.CDLL(hxbuild.build(force=False))
    for name in new:
        assert hasattr(cdll, name), name
    assert cdll.hx_abi_version() == 3
