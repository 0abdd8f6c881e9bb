"""GPU: random lifecycle sequences against the host model of the index (tests/lifecycle_model.py; DESIGN.md sections
1a, 14, 18).

add, retain, replace (both forms), truncate, save / load, finalize / rebuild / searches and the payload calls in seeded
random order on one HxIndex; after EVERY op `check` compares count, nnz and n_segments with the model, the bytes of
every stored copy and the cells of every payload column of sampled rows with a fresh index of the model's rows and with
the model, a random compiled filter's mask word for word with the host interpreter and -- where the op's `search` flag
is set -- the lists of 8 queries in both modes bit for bit with the fresh index (unmasked and under the filter's mask)
and the first query with the numpy oracle.  The binary copy is checked after every op too:
binary_enabled() against the model, the refusals without the copy, the sign bits of the sampled rows and the Hamming scan
of the 8 queries and of the first alone (unmasked and under the filter's mask) word for word against the fresh index and
tests/binary_helpers.py; the profiles `binary`, `binary_padded` and `binary_chunks` enable it at a random step and lose it
at every load.  Behind the `search` flag df, N and the IDF weights of probe terms (hx_sparse_idf_host) are compared bit for
bit with the fresh index and with counts over the model's rows weighed by tests/sparse_idf_helpers.py, in every profile.
tests/test_lifecycle_model_host.py asserts what the committed sequences cover.  A failure names the seed, the step and the ops so far; lifecycle_model.sequence(seed, step + 1, profile)
replays it."""
import pytest

from tests import lifecycle_model as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from rag_application_amd import engine
    return engine


@pytest.mark.parametrize("seed,profile", L.CASES)
def test_sequence(eng, synth_tables, monkeypatch, tmp_path, seed, profile):
    for k, v in L.PROFILES[profile]["env"].items():
        monkeypatch.setenv(k, v)                     # (read by hx_create: the fresh and the loaded indexes see them too)
    L.run(eng, eng.HxIndex, seed, profile, synth_tables, tmp_path)
