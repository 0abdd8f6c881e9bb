"""CPU: hx_h1_plan (the list sizes of the candidates-first sharded H1 exchange) against the argument checks of the calls
its plan feeds, over every world size and limit the ABI takes, and H1Pipeline's choice of exchange built on it.

The checks are restated here from rag_application_amd/csrc/engine.hip; each one names the HX_CHECK it mirrors:
  geometry()             HX_CHECK(g.Lp * 2 <= g.C && g.Lp >= L, "limit too large"), with cand8 and lp_force = k1
  hx_h1_nominate_async   k1 in [1, CAND_CAP / 4], k2 in [1, lout], limits in [1, MAX_LIMIT]
  hx_h1_rescore_async    dense_limit <= lp <= MAX_LIMIT; world x k1, k2, k3 <= CAND_CAP; k >= 1; k3 <= 256
  hx_h1_finish           dense_limit <= lp <= MAX_LIMIT; k3 >= 1; world x k3 <= CAND_CAP
  hx_h1_fuse             world x max(dense_limit, sparse_limit) <= CAND_CAP (the per-shard exchange, and the redo path)
A plan these checks would reject makes H1Pipeline.submit() raise on a combination the per-shard exchange serves."""
import math

import numpy as np
import pytest

CAND_CAP, MAX_LIMIT, K3_MAX, WORLD_MAX = 8192, 2048, 256, 64


@pytest.fixture(scope="module")
def eng():
    from rag_application_amd import build
    build.build()
    from rag_application_amd import engine
    return engine


# ---- restatements of the host arithmetic (engine.hip) -------------------------------------------------------------------
def next_pow2(v):
    return 1 << max(0, (int(v) - 1).bit_length())


def round_up(x, m):
    return (x + m - 1) // m * m


def cand8_lprime(L):                  # engine.hip cand8_lprime (defaults: mul2 = 9, add = 288)
    return min(max(9 * L // 2, L + 288), max(L, CAND_CAP // 4))


def sparse_lout(L):                   # engine.hip sparse_lout
    return max(2048, next_pow2(L + L // 2 + 64))


def share(n, world):                  # hx_h1_plan: a shard's binomial share of a global list of n, mean + 10 sigma
    p = 1.0 / world
    return min(round_up(math.ceil(n * p + 10.0 * math.sqrt(n * p * (1.0 - p))), 32), round_up(n, 32))


def cap_of(world):                    # world x k keys are merged in one CAND_CAP-key buffer
    return CAND_CAP // world // 32 * 32


def geometry_C(k1):                   # engine.hip geometry(dense_limit, approx, !safe, cand8, lp_force = k1): C
    return min(max(next_pow2(max(8 * k1, 1024)), 1024), CAND_CAP)


def contract_violations(world, dl, sl, k1, k2, lp, k3, lout):
    """Every argument check the plan's shares meet in nominate / rescore / finish; [] when all hold."""
    bad = []
    C = geometry_C(k1)
    if not (k1 >= dl and 2 * k1 <= C):                                   # geometry(): "limit too large"
        bad.append(f"geometry: k1 {k1} vs dense_limit {dl}, C {C}")
    if not (1 <= k1 <= CAND_CAP // 4):                                   # nominate: "k1 / k2 out of range"
        bad.append(f"nominate: k1 {k1}")
    if not (1 <= k2 <= sparse_lout(sl)):                                 # nominate: "k1 / k2 out of range"
        bad.append(f"nominate: k2 {k2} vs lout {sparse_lout(sl)}")
    if not (dl <= lp <= MAX_LIMIT):                                      # rescore / finish: "limits out of range"
        bad.append(f"rescore: lp {lp}")
    if not all(world * k <= CAND_CAP for k in (k1, k2, k3)):             # rescore: "world x k out of range"
        bad.append(f"rescore: world x k ({k1}, {k2}, {k3})")
    if not (1 <= k3 <= K3_MAX):                                          # rescore: k3 <= 256; finish: k3 >= 1
        bad.append(f"rescore: k3 {k3}")
    if any(k % 32 for k in (k1, k2, k3)):                                # the kernels' lists are whole waves
        bad.append(f"k not a multiple of 32: ({k1}, {k2}, {k3})")
    if lout != sparse_lout(sl):
        bad.append(f"lout {lout} != {sparse_lout(sl)}")
    return bad


def minimal_plan(world, dl, sl):
    """The smallest shares that keep the plan's completeness margin (k >= the binomial share, capped) and meet the
    contract, or None when no such shares exist.  A plan may be wider; it must not be refused when this exists."""
    cap = cap_of(world)
    lp = cand8_lprime(dl)
    if lp > MAX_LIMIT:
        return None
    k1 = max(min(share(lp, world), cap), round_up(dl, 32))
    ks = min(share(sl, world), cap)
    if k1 > cap or ks > K3_MAX:
        return None
    return k1, ks, lp, ks, sparse_lout(sl)


def plan_or_none(eng, dl, sl, world):
    try:
        return tuple(eng.h1_plan(dl, sl, world))
    except eng.HxError:
        return None


# ---- the sweep -----------------------------------------------------------------------------------------------------------
def sweep_points():
    pts = []
    lims = np.arange(1, MAX_LIMIT + 1)
    for w in range(1, WORLD_MAX + 1):
        for sl in (1, 100, 2048):             # every dense_limit at a few sparse_limits
            pts += [(w, int(dl), sl) for dl in lims]
        for dl in (1, 100):                   # every sparse_limit at a few dense_limits
            pts += [(w, dl, int(sl)) for sl in lims]
    rng = np.random.default_rng(2024)
    r = rng.integers(1, [WORLD_MAX + 1, MAX_LIMIT + 1, MAX_LIMIT + 1], size=(4000, 3))
    pts += [tuple(int(x) for x in p) for p in r]
    return pts


@pytest.fixture(scope="module")
def plans(eng):
    return {p: plan_or_none(eng, p[1], p[2], p[0]) for p in sweep_points()}


# the combinations of the issue that the plan got wrong: (world, dense_limit, sparse_limit)
KNOWN_BAD = [(8, 500, 100), (13, 100, 100), (2, 100, 400), (1, 100, 300), (8, 2048, 10), (8, 400, 100), (8, 289, 64),
             (4, 737, 100), (2, 1281, 100), (13, 97, 100), (2, 100, 257), (2, 100, 330), (8, 100, 1150)]


@pytest.mark.parametrize("world,dl,sl", KNOWN_BAD)
def test_plan_for_known_bad_limits(eng, world, dl, sl):
    got = plan_or_none(eng, dl, sl, world)
    if got is None:
        assert minimal_plan(world, dl, sl) is None, f"refused, but {minimal_plan(world, dl, sl)} serves it"
    else:
        assert contract_violations(world, dl, sl, *got) == [], got


def test_every_plan_meets_the_calls_it_feeds(plans):
    bad = []
    for (w, dl, sl), p in plans.items():
        if p is not None:
            v = contract_violations(w, dl, sl, *p)
            if v:
                bad.append(((w, dl, sl), p, v))
    assert not bad, f"{len(bad)} plans the calls reject, e.g. {bad[:5]}"


def test_plan_keeps_its_margin(plans):
    """An accepted plan is at least the minimal one: it did not make a case fit by cutting the binomial margin."""
    bad = []
    for (w, dl, sl), p in plans.items():
        if p is not None:
            m = minimal_plan(w, dl, sl)
            if m is None or not (p[0] >= m[0] and p[1] >= m[1] and p[2] == m[2] and p[3] >= m[3] and p[4] == m[4]):
                bad.append(((w, dl, sl), p, m))
    assert not bad, f"{len(bad)} plans below the margin, e.g. {bad[:5]}"


def test_plan_refuses_only_what_no_shares_serve(plans):
    bad = [(k, minimal_plan(*k)) for k, p in plans.items() if p is None and minimal_plan(*k) is not None]
    assert not bad, f"{len(bad)} refusals the exchange could serve, e.g. {bad[:5]}"


def test_plan_rejects_its_own_bad_arguments(eng):
    for dl, sl, w in ((0, 10, 2), (10, 0, 2), (2049, 10, 2), (10, 2049, 2), (10, 10, 0), (10, 10, 65)):
        with pytest.raises(eng.HxError):
            eng.h1_plan(dl, sl, w)


# ---- H1Pipeline: which exchange it picks --------------------------------------------------------------------------------
class _Local:
    """The method names H1Pipeline looks for on a shard; nothing here runs (no GPU)."""

    def __init__(self, i8=True):
        self.i8 = i8

    def h1_local(self, *a):
        raise AssertionError("not called at construction")

    h1_local_async = h1_nominate_async = h1_rescore_async = h1_local

    def dense_candidates(self):
        return "i8" if self.i8 else "f16"


class _Sharded:
    """A ShardedIndex of `world` ranks seen from rank 0: the collectives of the constructor are answered here."""

    def __init__(self, world, eng, others_i8=True, local_i8=True):
        self.world, self.rank, self.ops = world, 0, eng
        self.local = _Local(local_i8)
        self.others_i8 = others_i8
        self.synced = 0
        self.min_calls = 0

    def sync_sparse_scale(self):
        self.synced += 1

    def all_min(self, v):
        self.min_calls += 1
        return min(int(v), 1 if self.others_i8 else 0) if self.world > 1 else int(v)


def widenings(pipe):
    """Every (k1, k2, k3) the doubling in H1Pipeline._verify can reach, in order (pure arithmetic)."""
    k = (pipe.k1, pipe.k2, pipe.k3)
    out = [k]
    while not (k[0] >= pipe.k1max and k[1] >= pipe.k2max and k[2] >= pipe.k3max):
        k = (min(2 * k[0], pipe.k1max), min(2 * k[1], pipe.k2max), min(2 * k[2], pipe.k3max))
        out.append(k)
    return out


PIPE_DL = (1, 10, 32, 33, 100, 288, 289, 400, 500, 737, 1000, 1281, 1600, 2048)
PIPE_SL = (1, 25, 64, 100, 256, 257, 300, 330, 400, 1150, 2048)


def test_pipeline_construction_over_worlds_and_limits(eng):
    from rag_application_amd.distributed import H1Pipeline
    seen = {"cf": 0, "per-shard": 0, "raises": 0}
    for world in range(1, WORLD_MAX + 1):
        for dl in PIPE_DL:
            for sl in PIPE_SL:
                sh = _Sharded(world, eng)
                serves_per_shard = world * max(dl, sl) <= CAND_CAP
                try:
                    pipe = H1Pipeline(sh, dl, sl, 10, force_side_stream=(world == 1))
                except ValueError as e:
                    assert not serves_per_shard, f"({world}, {dl}, {sl}): raised although the per-shard exchange serves it"
                    assert "dense_limit" in str(e) and "sparse_limit" in str(e), str(e)
                    seen["raises"] += 1
                    continue
                assert serves_per_shard, f"({world}, {dl}, {sl}): constructed, but no exchange serves the limits"
                assert pipe.deferred and pipe.side is None
                plan = plan_or_none(eng, dl, sl, world)
                if pipe.cf:
                    seen["cf"] += 1
                    assert plan is not None
                    assert (pipe.k1, pipe.k2, pipe.lp, pipe.k3, pipe.lout) == plan
                    assert sh.synced == 1
                    for k1, k2, k3 in widenings(pipe):
                        v = contract_violations(world, dl, sl, k1, k2, pipe.lp, k3, pipe.lout)
                        assert v == [], f"({world}, {dl}, {sl}) widened to ({k1}, {k2}, {k3}): {v}"
                else:
                    seen["per-shard"] += 1
                    assert plan is None, f"({world}, {dl}, {sl}): plan {plan} accepted, candidates-first not enabled"
    assert all(seen.values()), seen


@pytest.mark.parametrize("world", [1, 2, 8])
def test_pipeline_needs_the_int8_copy_on_every_rank(eng, world):
    from rag_application_amd.distributed import H1Pipeline
    for local_i8, others_i8 in ((True, True), (False, True), (True, False), (False, False)):
        sh = _Sharded(world, eng, others_i8=others_i8, local_i8=local_i8)
        pipe = H1Pipeline(sh, 100, 100, 10, force_side_stream=True)
        want = local_i8 and (others_i8 or world == 1)
        assert pipe.cf == want, (world, local_i8, others_i8)
        assert sh.min_calls == 1              # the collective happens on every rank, whatever this rank's answer
    # asked NOT to use it: no collective at all (every rank was asked the same)
    sh = _Sharded(world, eng)
    assert not H1Pipeline(sh, 100, 100, 10, force_side_stream=True, candidates_first=False).cf
    assert sh.min_calls == 0
