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
numpy oracle and the host models of the four pool stages.  tests/test_handler_model_host.py asserts what the committed
sequences cover.  A failure names the seed, the step and the ops so far; handler_model.sequence(seed, step + 1, profile,
pool) replays it.

Wall time per case on an MI355X (24 ops each), measured: 32-bare 4.6 s, 30-small 3.8 s, 32-persist 3.1 s, 24-padded
3.1 s, 36-small 2.8 s, 7-chunked 2.7 s, 4-chunked 2.5 s, 1-small 2.3 s, 7-persist 2.2 s, 2-small 2.0 s; the ten
together 29 s."""
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
