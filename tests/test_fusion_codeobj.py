"""Both forms of the fusion kernel (fuse.hip: k_fuse, the one-wave form and the general one) are in
the shipped libhx.so, use no scratch memory and spill no vector register -- read from the code object's notes as
tests/test_mmr_codeobj.py does -- and their LDS (tags and fused keys of 4096 slots, the contributions) stays inside 64
KB.  hx_fuse is declared, bound and exported.  No GPU needed."""
from __future__ import annotations

import ctypes as C
import os

import pytest

from tests.test_abi import declared_functions
from tests.test_codeobj import READELF, _code_objects, _kernel_notes

KERNEL = "k_fuse"


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_fusion_kernels_have_no_scratch_no_vgpr_spills_and_fit_64k_of_lds(tmp_path):
    from rag_application_amd import build as hxbuild
    lib = hxbuild.build(force=False)
    found, bad = [], []
    for k, blob in enumerate(_code_objects(lib)):
        for kn in _kernel_notes(blob, tmp_path, k):
            if KERNEL not in kn["name"]:
                continue
            found.append(kn)
            if int(kn.get("private_segment_fixed_size", "0")) != 0 or int(kn.get("vgpr_spill_count", "0")) != 0:
                bad.append((kn["name"], kn.get("private_segment_fixed_size"), kn.get("vgpr_spill_count")))
    assert len(found) == 2, f"want the one-wave and the general form of {KERNEL}, found {[kn['name'] for kn in found]}"
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    names = sorted(kn["name"] for kn in found)                  # k_fuse<64, 4> and k_fuse<512, 8>, mangled
    assert "Li512ELi8E" in names[0] and "Li64ELi4E" in names[1], names
    for kn in found:
        assert int(kn["group_segment_fixed_size"]) <= 64 * 1024, (kn["name"], kn["group_segment_fixed_size"])
        assert int(kn["vgpr_count"]) <= 128, (kn["name"], kn["vgpr_count"])


def test_hx_fuse_is_declared_bound_and_exported():
    from rag_application_amd import _lib
    from rag_application_amd import build as hxbuild
    assert "hx_fuse" in declared_functions() and "hx_fuse" in _lib.EXPORTS
    assert sorted(_lib.EXPORTS) == declared_functions()
    cdll = C.CDLL(hxbuild.build(force=False))
    assert hasattr(cdll, "hx_fuse")
    assert cdll.hx_abi_version() == 3
