"""CPU, world size 2 over gloo: the row-sharded exchange of the sparse IDF modifier (sharded.ShardedCollection with
sparse_modifier="idf").  Each rank's stand-in shard counts (df, N) over its own rows, one
all_reduce sums them, and every rank scales the batch's weights alike -- so the lists of both modes must equal, bit for
bit, the oracle on the UNSHARDED corpus fed weights pre-scaled by the header's restatement with the global df and N.
The corpus holds a term that lives on one shard only; a second collection of one row leaves the front rank's shard
empty."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import sparse_idf_helpers as H
from tests.test_distributed_cpu import CpuOps, GrowingShard, P, _orig_init, unkey

LONELY = 1999999          # a term of rows in the second half only: rank 1's shard
N_ROWS, DIM, B = 301, 256, 6
MSIZES = (64, 128, 256)


class StatsShard(GrowingShard):
    """... that also counts its rows' term statistics (engine.HxIndex.sparse_df)"""

    def __init__(self, dim, msizes, id_base):
        _orig_init(self, dim, msizes, id_base)       # (none of that module's planned failures)

    def sparse_df(self, q_idx):
        o = self.ora
        ip = np.asarray(o.sp_indptr, np.int64) if o.n else np.zeros(1, np.int64)
        ix = np.asarray(o.sp_idx, np.int64)[: int(ip[-1])]
        df = np.array([int((ix == int(t)).sum()) if int(t) >= 0 else 0 for t in q_idx.tolist()], np.int64)
        return torch.from_numpy(df), torch.tensor([int((np.diff(ip) > 0).sum())], dtype=torch.int64)


def corpus(O):
    tabs = O.synth_tables()
    X = O.synth_dense(O.SEED_CORPUS, 0, N_ROWS, DIM)
    ip, si, sv = O.synth_sparse_docs(O.SEED_SPDOC, 0, N_ROWS, tabs)
    # rows 200, 250 and 300 also hold LONELY (the largest id of its row: the rows stay ascending); row 7 loses its vector
    rows = [(si[ip[r]:ip[r + 1]].astype(np.int64), sv[ip[r]:ip[r + 1]]) for r in range(N_ROWS)]
    for r in (200, 250, 300):
        rows[r] = (np.append(rows[r][0], LONELY), np.append(rows[r][1], np.float32(1.5)))
    rows[7] = (np.zeros(0, np.int64), np.zeros(0, np.float32))
    ip = np.concatenate([[0], np.cumsum([len(i) for i, _ in rows])]).astype(np.int64)
    si = np.concatenate([i for i, _ in rows]).astype(np.int64)
    sv = np.concatenate([v for _, v in rows]).astype(np.float32)
    Q = O.synth_dense(O.SEED_QUERY, 0, B, DIM)
    qip, qsi, qsv = O.synth_sparse_queries(O.SEED_SPQUERY, 0, B, tabs)
    qs = [(qsi[qip[b]:qip[b + 1]].astype(np.int64), qsv[qip[b]:qip[b + 1]]) for b in range(B)]
    common = int(np.bincount(si[si < LONELY]).argmax())          # the most frequent term of the corpus
    qs[1] = (np.append(qs[1][0][qs[1][0] < LONELY], LONELY), np.append(qs[1][1][qs[1][0] < LONELY], np.float32(1.0)))
    qs[2] = (np.array([common, LONELY]), np.array([1.0, 1.0], np.float32))     # equal weights: only the IDF tells them apart
    qs[3] = (np.array([LONELY + 5]), np.array([2.0], np.float32))              # a term nobody holds
    qs[4] = (np.zeros(0, np.int64), np.zeros(0, np.float32))
    qip = np.concatenate([[0], np.cumsum([len(i) for i, _ in qs])]).astype(np.int64)
    qsi = np.concatenate([i for i, _ in qs]).astype(np.int32)
    qsv = np.concatenate([v for _, v in qs]).astype(np.float32)
    return X, ip, si, sv, Q, qip, qsi, qsv


def worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import oracle as O
    from rag_application_amd.sharded import ShardedCollection
    X, ip, si, sv, Q, qip, qsi, qsv = corpus(O)
    front = rank == 0
    out = {}
    for name, n in (("full", N_ROWS), ("one", 1)):
        col = ShardedCollection(DIM, MSIZES, index_factory=StatsShard, ops=CpuOps, sparse_modifier="idf")
        plain = ShardedCollection(DIM, MSIZES, index_factory=StatsShard, ops=CpuOps)
        for c in (col, plain):
            c.store(*((X[:n], ip[:n + 1], si[:ip[n]], sv[:ip[n]]) if front else (None,) * 4))
        if name == "one":
            assert col.counts.tolist() == [0, 1] and (col.local.count() == 0) == front      # the front rank's shard is empty
        df, nd = col.local.sparse_df(torch.tensor([LONELY]))
        out[name + "_local"] = (int(df[0]), int(nd[0]))
        for mode in ("tree", "h1"):
            for c, tag in ((col, "idf"), (plain, "plain")):
                k, cnt = c.search(*((Q, qip, qsi, qsv, P, mode) if front else (None,) * 6))
                out[name, mode, tag] = (k.numpy().copy(), cnt.numpy().copy())
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_idf_exchange_equals_the_unsharded_oracle_fed_scaled_weights():
    from oracle import oracle as O
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(worker, args=(world, port, ret), nprocs=world, join=True)
    X, ip, si, sv, Q, qip, qsi, qsv = corpus(O)
    # the lonely term lives on rank 1 only; the one-row collection leaves rank 0 without a row
    assert ret[0]["full_local"] == (0, 149) and ret[1]["full_local"] == (3, 151)
    assert ret[0]["one_local"] == (0, 0) and ret[1]["one_local"][1] == 1
    differs = 0
    for name, n in (("full", N_ROWS), ("one", 1)):
        full = O.OracleIndex(DIM, MSIZES)
        full.add(X[:n], ip[:n + 1], si[:ip[n]], sv[:ip[n]])
        full.finalize()
        df, n_docs = H.stats(ip[:n + 1], si[:ip[n]], qsi)
        assert n_docs == (300 if name == "full" else 1)
        scaled = H.weights(qsv, df, n_docs)
        for mode in ("tree", "h1"):
            for tag, w in (("idf", scaled), ("plain", qsv)):
                for rank in range(world):
                    k, c = ret[rank][name, mode, tag]
                    for b in range(B):
                        sp = (qsi[qip[b]:qip[b + 1]], w[qip[b]:qip[b + 1]])
                        es, ei = (O.hybrid_tree(full, Q[b], *sp, P) if mode == "tree" else
                                  O.hybrid_h1(full, Q[b], *sp, P["dense_limit"], P["sparse_limit"], P["final_limit"]))
                        m = len(ei)
                        assert int(c[b]) == m, (name, mode, tag, rank, b)
                        s, i = unkey(k[b, :m])
                        np.testing.assert_array_equal(i, ei)
                        np.testing.assert_array_equal(s.view(np.uint32), es.view(np.uint32))
            a, b_ = ret[0][name, mode, "idf"][0], ret[0][name, mode, "plain"][0]
            differs += int(not np.array_equal(a, b_))
    assert differs, "the modifier must change some list: the comparison above would otherwise show nothing"
