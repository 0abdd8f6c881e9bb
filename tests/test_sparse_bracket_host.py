"""CPU: the contract the sparse select pass states in the header of rag_application_amd/csrc/sparse2.hip, checked on the
restatement of its integer arithmetic (tests/sparse_bracket_helpers.py: int_model) and on a corpus built so that the
integer order and the exact order DISAGREE around rank L (adversarial_cell):

  (a) bracket        a - 1.0078 k <= u <= a + 0.0078 k for every touched document
  (b) preconditions  the corpus bites: the exact top-L sits far down the integer order, and the margin set still fits
                     the pass's list (lout = 2048) with room to spare
  (c) margin         the exact top-L (oracle, upstream arithmetic) lies inside {a > a_L - M}, M = T + T/16 + 4, and the
                     top-L of the exact scores inside that set IS the exact top-L
  (d) mutation       with M replaced by T/2 - 2 the containment breaks: a margin that much too short would not pass (c)

Measured on the CPU (seed 1, 3000 background documents; a_L = L-th best integer score, gap = a_L - the lowest integer
score in the exact top-L, inverted = documents of the exact top-L whose integer rank is >= L, keep = |{a > a_L - M - 3}|):

      T   M |  L = 10: gap inverted keep |  L = 100: gap inverted keep |  L = 300: gap inverted keep
      1   5 |           0     0     101  |            0     0     277  |            0     0     683
      2   6 |           0     0     108  |            0     0     304  |            0     0     703
     15  19 |          12    10     228  |           10   100     431  |           10   300     849
     16  21 |          12    10     240  |           12   100     453  |           11   300     883
     17  22 |          14    10     270  |           13   100     459  |           12   300     909
     32  38 |          28    10     397  |           28   100     576  |           27   300     998
     48  55 |          45    10     559  |           44   100     743  |           43   300    1152
     63  70 |          59    10     682  |           58   100     850  |           57   300    1247
     64  72 |          60    10     654  |           59   100     863  |           58   300    1236

For T >= 15 the whole exact top-L lies below integer rank L, T - 6 .. T - 4 units under a_L: the top-L survives only
because of the margin.  The mutated margin T/2 - 2 loses documents in every cell with T >= 32."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import sparse_bracket_helpers as H

SEED = 1
CELLS = [(T, L) for L in (10, 100, 300) for T in H.T_HOST]


@functools.lru_cache(maxsize=None)
def cell(T, L):
    """corpus, integer model and the oracle's exact top-L of one cell: computed once, shared, never changed"""
    c = H.adversarial_corpus([T], L, SEED)
    m = c.model(0)
    ora = H.exact_oracle(O, c)
    ids, s = ora.sparse_scores(*c.queries[0], fix_bits=None)
    es, ei = O.topk(s, ids, L)                        # = ora.search_sparse(..., L, fix_bits=None)
    return c, m, (ids, s), (es, ei)


@pytest.mark.parametrize("T,L", CELLS)
def test_bracket(T, L):
    """(a) on every touched document of the restatement, inflated, deflated, background and all"""
    c, m, _, _ = cell(T, L)
    assert len(m["rows"]) == c.n - 1                  # every document but the sentinel shares a term with the query
    assert (m["a"] < 65536).all() and (m["a"] >= m["k"]).all()
    lo = m["a"] - 1.0078 * m["k"]
    hi = m["a"] + 0.0078 * m["k"]
    bad = np.nonzero(~((lo <= m["u"]) & (m["u"] <= hi)))[0]
    assert len(bad) == 0, (T, L, m["rows"][bad][:5], m["a"][bad][:5], m["u"][bad][:5], m["k"][bad][:5])


@pytest.mark.parametrize("T,L", CELLS)
def test_populations_are_what_the_generator_says(T, L):
    """inflated: a - u ~ 0.98 T; deflated: a - u = 0.02 k and truly above every inflated document; the model sees the
    sentinel's weight as wmax (no generated weight reaches it)"""
    c, m, _, _ = cell(T, L)
    kind = c.cells[0]["kind"]
    rows = c.cell_rows[0]
    u_of = np.zeros(c.n)
    u_of[m["rows"]] = m["u"]
    d = m["a_of"][rows] - u_of[rows]
    assert np.allclose(d[kind == 0], (1 - H.FRAC_LO) * T, atol=1e-2)
    kd = np.diff(c.indptr)[rows][kind == 1]
    assert np.allclose(d[kind == 1], (1 - H.FRAC_HI) * kd, atol=1e-2) and set(kd.tolist()) <= {1, 2}
    assert u_of[rows][kind == 1].min() > u_of[rows][kind == 0].max() + 1.9
    assert u_of[rows][kind == 2].max() < u_of[rows][kind == 0].min() - 1.0
    assert float(c.val.max()) == H.W_SENTINEL and np.count_nonzero(c.val == np.float32(H.W_SENTINEL)) == 1


@pytest.mark.parametrize("T,L", CELLS)
def test_generator_preconditions(T, L):
    """(b): conditions on the corpus, not measurements (the measured values are in the module docstring)"""
    c, m, _, (es, ei) = cell(T, L)
    aL = H.a_L_of(m["a"], L)
    assert len(H.keep_rows(m, L, slack=3)) <= 1500
    if T >= 15 and L >= 100:
        assert aL - int(m["a_of"][ei].min()) >= T / 2
        keys = np.sort(H.int_keys(m["a"], m["rows"]))[::-1]
        top_int = set((np.uint64(0xFFFFFFFF) - (keys[:L] & np.uint64(0xFFFFFFFF))).astype(np.int64).tolist())
        assert sum(1 for d_ in ei.tolist() if d_ not in top_int) >= L - 1


@pytest.mark.parametrize("T,L", CELLS)
def test_margin_keeps_the_exact_top(T, L):
    """(c) on the full corpus"""
    c, m, (ids, s), (es, ei) = cell(T, L)
    assert len(ei) == L
    keep = H.keep_rows(m, L)
    assert set(ei.tolist()) <= set(keep.tolist())
    inside = np.isin(ids, keep)
    ks, ki = O.topk(s[inside], ids[inside], L)
    np.testing.assert_array_equal(ki, ei)
    np.testing.assert_array_equal(ks.view(np.uint32), es.view(np.uint32))


def test_a_short_margin_would_be_caught():
    """(d): the containment of (c) with M = T/2 - 2 fails -- in at least one cell with T >= 32 (here: in all of them)"""
    lost = []
    for T, L in CELLS:
        if T < 32:
            continue
        c, m, _, (es, ei) = cell(T, L)
        short = H.keep_rows(m, L, M=T // 2 - 2)
        if not set(ei.tolist()) <= set(short.tolist()):
            lost.append((T, L))
    assert lost, "the corpus does not notice a margin of T/2 - 2"


def test_select_model_on_one_segment_is_the_keep_set_up_to_the_histogram_bin():
    """select_model (what the GPU test predicts the pass's list with): on one segment the list lies between
    {a > a_L - M} and {a > a_L - M - 3} (bins of 4 scores) / {a > a_L - M - 1} (bins of 2), best key first"""
    c, m, _, _ = cell(64, 100)
    for hshift in (1, 2):
        keys, ncand, fail = H.select_model(m, 100, 2048, hshift, [(0, c.n)])
        rows = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
        assert not fail and (np.diff(keys.astype(np.int64)) < 0).all()
        assert set(H.keep_rows(m, 100).tolist()) <= set(rows.tolist())
        assert set(rows.tolist()) <= set(H.keep_rows(m, 100, slack=(1 << hshift) - 1).tolist())
        assert ncand == len(H.keep_rows(m, 100))
