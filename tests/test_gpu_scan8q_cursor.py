"""GPU: the item cursor of k_scan8q (scan8.hip; Scan8qCursor, kernels.hpp) at the shapes where its walk can go wrong.

The pattern is tests/test_gpu_scan8_qs.py's: a default index, whose int8 scans take k_scan8q (hx_scan8_form is asserted
first), beside one created under HX_DEBUG_NO_QS, whose scans take k_scan8 and its own tile walk.  search_dense with int8
candidates and search_i8 must agree with each other in every bit and with CO.search_dense / CO.search_i8 in ids and fp32
score bits; cand8_queries rises by B and the fallback counters stand still, so a wrong walk cannot hide behind the exact
path.

The first chunk of every scan (4096 rows) goes through k_scan; k_scan8q takes the tiles behind it, dealt to 8 XCDs x
32 / nq streams as 128-row halves, a PAIR of 64-row items each.  The shapes are chosen for the cursor, not for size:
  17 tiles   one tile behind the first chunk: two halves, most workgroups leave at once;
  24, 31, 57 8, 15 and 41 tiles behind it: XCDs with equal and unequal tile counts, workgroups with no, one and two pairs
             (B = 1024: 8 streams per XCD);
  57 tiles + 1 row: the last tile holds one row, planted as the best row of query 0;
  57 tiles at B = 256 .. 4096: nq = 1, 2, 8, 16, i.e. 32 down to 2 streams per XCD -- the step of the cursor is
             (4 * nstreams * mul) mod n, another constant for each, and at 2 streams a workgroup walks up to six pairs;
  65,536 rows under HX_DEBUG_NO_PERM: the identity order, perm_n = 0, no wrap at all."""
import numpy as np
import pytest

from oracle import c_oracle as CO
from tests.test_gpu_scan8_qs import DIM, FORM_QS, Ref, both_forms, index_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
B4K = 4096


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def eng():
    from rag_application_amd import engine
    return engine


class Data:
    """Rows and queries shared by every cell (computed once, never written)"""

    def __init__(self, torch_mod):
        self.X = CO.synth_dense(41, 0, 65536, DIM) * F32(2.5)
        self.Q = CO.synth_dense(42, 0, B4K, DIM) * F32(0.3)
        self.Qd = torch_mod.from_numpy(self.Q).cuda()
        self.Qu = torch_mod.from_numpy(CO.cosine_preprocess(self.Q)).cuda()


@pytest.fixture(scope="module")
def data(torch_mod):
    return Data(torch_mod)


def run_cell(eng, torch_mod, data, X, batches, what):
    """both forms on the rows X for every batch size (the reference lists are those of the largest, shared)"""
    bmax = max(batches)
    ref = Ref(X, data.Q[:bmax])
    ixs, ixs8 = index_pair(eng, X), index_pair(eng, ref.Xn)
    try:
        for B in batches:
            assert eng.scan8_form(B, DIM, "i8") == FORM_QS
            both_forms(eng, torch_mod, ixs, ixs8, data.Qd, data.Qu, ref, B, f"{what} B={B}")
    finally:
        for ix in (*ixs, *ixs8):
            ix.close()
    return ref


@pytest.mark.parametrize("tiles", [17, 24, 31, 57])
def test_tile_counts_behind_the_first_chunk(eng, torch_mod, data, tiles):
    run_cell(eng, torch_mod, data, data.X[:tiles * 256], [1024], f"{tiles} tiles")


def test_one_row_in_the_last_tile(eng, torch_mod, data):
    n = 256 * 57 + 1
    X = data.X[:n].copy()
    X[n - 1] = data.Q[0] * F32(8.0)
    ref = run_cell(eng, torch_mod, data, X, [1024], "57 tiles + 1 row")
    assert ref.dense[1][0, 0] == n - 1 and ref.i8[1][0, 0] == n - 1


def test_every_stream_count(eng, torch_mod, data):
    """nq = 1, 2, 8, 16 (B = 1024, nq = 4, is the cell above)"""
    run_cell(eng, torch_mod, data, data.X[:57 * 256], [256, 512, 2048, B4K], "57 tiles")


def test_identity_order(eng, torch_mod, data, monkeypatch):
    monkeypatch.setenv("HX_DEBUG_NO_PERM", "1")
    run_cell(eng, torch_mod, data, data.X, [1024], "65536 rows, identity order")
