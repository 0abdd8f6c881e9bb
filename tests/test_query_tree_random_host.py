"""CPU: the seeded random query trees of tests/query_tree_helpers.py.  Every generated request parses (a refused one is a
generator bug: the refused share is 0), the committed seeds plus the hand-written trees cover every structural class, and
query_tree.run over the oracle's stages gives the same keys whether the fusion nodes go through
rag_application_amd/fusion.py or through tests/fusion_helpers.py, node by node, on a small OracleIndex."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from rag_application_amd import query_tree as QT
from tests import fusion_helpers as H
from tests import query_tree_helpers as T

DIM, MS, N, B = 64, (16, 32), 300, 2


@pytest.fixture(scope="module")
def world(synth_tables):
    rows = T.synth_rows(N, DIM, synth_tables)
    q = O.synth_sparse_queries(O.SEED_SPQUERY, 0, B, synth_tables)
    pools = [T.sparse_pool(*rows[1:], *q, b) for b in range(B)]
    return T.oracle_index(rows, DIM, MS), T.seeded_requests(DIM, MS, B, pools)


def limits_of(req, out):
    out.append(req.get("limit"))
    for c in req.get("prefetch", ()):
        limits_of(c, out)
    return out


def depth_of(shape):
    return 1 + max((depth_of(c) for c in shape[-1]), default=0)


def test_every_generated_request_parses_and_stays_inside_the_limits():
    """600 seeds beyond the committed ones, default vectors: nothing is refused, nothing is deeper than 5"""
    refused, seen, usings = 0, set(), set()
    for seed in range(1000, 1600):
        req = T.random_tree(np.random.default_rng(seed), DIM, MS)
        try:
            shape, _ = QT.parse(req, DIM, MS)
        except ValueError:
            refused += 1
            continue
        assert depth_of(shape) <= T.MAX_DEPTH
        seen.update(limits_of(req, []))
        usings.update(s for s in str(shape).replace("'", " ").split() if s in ("dense", "quantized", "sparse")
                      or s.startswith("matryoshka_"))
    assert refused == 0
    assert seen >= set(T.LIMITS), sorted(set(T.LIMITS) - seen, key=str)
    assert usings == {"dense", "quantized", "sparse", "matryoshka_16", "matryoshka_32"}


def test_one_seed_gives_one_shape_whatever_the_vectors(world):
    for name, reqs in world[1]:
        shapes = {QT.parse(r, DIM, MS)[0] for r in reqs}
        assert len(shapes) == 1, name
    again = T.random_tree(np.random.default_rng(T.SEEDS[0]), DIM, MS)
    assert QT.parse(again, DIM, MS)[0] == QT.parse(world[1][0][1][0], DIM, MS)[0]


def test_the_seeds_and_the_hand_written_trees_cover_every_class(world):
    found, by_seed = set(), set()
    for name, reqs in world[1]:
        shape, vecs = QT.parse(reqs[0], DIM, MS)
        c = T.shape_classes(shape, vecs)
        assert c <= set(T.CLASSES)
        found |= c
        if name.startswith("seed "):
            by_seed |= c
    assert found == set(T.CLASSES), sorted(set(T.CLASSES) - found)
    # the random part does most of it alone; the hand-written trees pin the exact 8192 / 4096 / 8-list corners
    assert len(by_seed) >= len(T.CLASSES) - 3, sorted(set(T.CLASSES) - by_seed)


def test_every_sparse_kind_reaches_a_leaf(world):
    _, trees = world
    seen = set()
    for _, reqs in trees:
        _, vecs = QT.parse(reqs[0], DIM, MS)
        for v in vecs:
            if isinstance(v, tuple):
                seen.add("absent" if set(v[0].tolist()) <= set(T.ABSENT_TERMS) else "nonpositive" if (v[1] <= 0).any()
                         else "rare" if len(v[0]) == 1 else "ordinary")
    assert seen == set(T.SPARSE_KINDS)


def test_the_oracle_interpreter_is_the_same_through_either_fusion_model(world):
    ora, trees = world
    for name, reqs in trees:
        parsed = [QT.parse(r, DIM, MS) for r in reqs]
        vectors = QT.batch_vectors([v for _, v in parsed])
        a, b = T.Recorder(T.OracleStages(ora)), T.Recorder(T.OracleStages(ora, fuse=H))
        ka, ca = QT.run(parsed[0][0], vectors, a)
        kb, cb = QT.run(parsed[0][0], vectors, b)
        T.assert_same_nodes(a.nodes, b.nodes, name)
        assert np.array_equal(ka, kb) and ca.tolist() == cb.tolist()
        assert ka.shape == (B, QT.shape_limit(parsed[0][0]))
