"""GPU: random point-level sequences through QdrantHandler against the host model of the collection
(tests/handler_model.py).

store (documents, chats, refills), upsert (five forms), refused upserts (the rollback among them), delete (by ids, by
filters on indexed keys and on their unindexed twins, by has_id), payload-index create / re-create / drop / poison / cure,
the token index and save + load onto a NEW handler, in seeded random order on one collection.  After EVERY op `check`
compares with plain Python over the model's points: the counts under a fixed set of filters (met again after every op, so
cached masks are), chained scrolls in row and payload order, facets, retrieve, the token cells of the engine column, the
live flag of every key -- and WHICH PATH ran: the device counters advance by exactly one per read on a live key, the
Python counters on a dead one, "engine refused" never.  Where the op's `search` flag is set the lists of every searching
call are compared bit for bit with a fresh handler of the model's points; on the first and last such step also with the
numpy oracle and the host models of the four pool stages.  The searching calls include the later entries: query_points_batch
(the hand trees and two random trees per step, node filters with a score threshold, the filter in every leaf),
hybrid_search_boost (a number column, a keyword condition, a datetime decay in turn), discover_batch, search_matrix_pairs /
_offsets (sampled, filtered, by point ids), term_stats, and on the `binary` profile search_binary_batch and a
using="binary" leaf; on the deep steps each also against its host model over the model's points: the trees node by node
against query_tree.run over the oracle's stages (masks, keep and bin included), boost against formula_helpers.formula_stage
over the pool, discover against discover_helpers.request_model, the matrix calls against matrix_helpers.model over the
sample they returned, search_binary_batch against tests/binary_helpers.py, term_stats against tests/sparse_idf_helpers.py,
and on the `idf` profile the oracle is fed the helper's scaled weights.  After every op the
index's binary_enabled() equals the collection's flag (a load must enable the copy again) and on the `idf` profile
term_stats' n_docs the model's count.  tests/test_handler_model_host.py asserts what the committed
sequences cover.  A failure names the seed, the step and the ops so far; handler_model.sequence(seed, step + 1, profile,
pool) replays it.

Wall time per case on an MI355X (24 ops each), measured with the later reads and their deep models: 3-idf 9.2 s,
30-small 7.7 s, 22-binary 7.3 s, 19-idf 7.2 s, 32-bare 7.2 s, 36-small 6.7 s, 26-binary 6.6 s, 24-padded 6.0 s, 1-small
6.0 s, 7-chunked 5.7 s, 32-persist 5.5 s, 4-chunked 5.5 s, 7-persist 4.9 s, 2-small 4.1 s; the fourteen together 91 s
(before the later reads the first ten took 2.0-4.6 s, 29 s together)."""
import pytest

from tests import handler_model as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,profile", H.CASES)
def test_sequence(synth_tables, monkeypatch, tmp_path, seed, profile):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd.handler import QdrantHandler
    for k, v in H.PROFILES[profile]["env"].items():
        monkeypatch.setenv(k, v)                     # (read by hx_create: the fresh and the loaded handlers see them too)
    H.run_case(lambda persist: QdrantHandler(persist_dir=persist), seed, profile, synth_tables, tmp_path)
