"""No GPU: the item cursor of k_scan8q (Scan8qCursor, kernels.hpp) run on the host through hx_scan8q_items, against the
closed form it replaces inside the kernel's item loop.

Workgroup (xcd, i0) of the 256 keeps query tile i0 mod nq and is stream i0 // nq of nstreams = 32 // nq.  It scans the
128-row halves u = stream + j * nstreams of its XCD, two 64-row items each: logical tile row_begin / 256 + (u >> 1) * 8 + xcd,
physical tile (t * mul) mod n in integers (n = 0: t itself), first row tile * 256 + (u & 1) * 128 + 64 * (item & 1).  The
cursor forms the physical tile by adding (4 * nstreams * mul) mod n per pair with one conditional subtract."""
import ctypes as C
import math

import numpy as np
import pytest

from rag_application_amd import _lib

PERM_N = [0, 8, 9, 15, 17, 31, 57, 250, 255, 39063]
NQ = [1, 2, 4, 8, 16]
IDENTITY_TILES = 256        # tile count of the perm_n = 0 cases (the identity order has no modulus to take it from)


def perm_mul(n):
    """chunked_scan's multiplier: about 0.618 n, odd, coprime to n"""
    if n == 0:
        return 1
    m = int(float(n) * 0.6180339887498949) | 1
    while math.gcd(m, n) != 1:
        m += 2
    return m % n


def launches(n):
    """(row_begin, row_end) of the cases: begins 0, 4096 and a mid-range multiple of 256; ends at the tile count and one
    tile short of it -- those with at least one row"""
    tiles = n if n else IDENTITY_TILES
    out = []
    for rb in (0, 4096, (tiles // 2) * 256):
        for re_ in (tiles * 256, (tiles - 1) * 256):
            if re_ > rb and (rb, re_) not in out:
                out.append((rb, re_))
    return out


def closed_form(rb, re_, nq, mul, n, block):
    xcd, i0 = block & 7, block >> 3
    stream, nstreams = i0 // nq, 32 // nq
    T = (re_ - rb + 255) // 256
    halves_x = 2 * ((T - xcd + 7) >> 3)
    u = np.arange(stream, max(halves_x, stream), nstreams, dtype=np.int64)
    t = rb // 256 + (u >> 1) * 8 + xcd
    p = (t * mul) % n if n else t
    tiles = np.repeat(p, 2)
    rows = np.repeat(p * 256 + (u & 1) * 128, 2) + np.tile(np.array([0, 64], np.int64), len(u))
    # n_items as the kernel states it
    n_items = 2 * ((halves_x - stream + nstreams - 1) // nstreams) if stream < halves_x else 0
    assert n_items == len(rows)
    return tiles, rows


def walk(rb, re_, nq, mul, n, block):
    lib = _lib.lib()
    cnt = C.c_int32()
    assert lib.hx_scan8q_items(rb, re_, nq, mul, n, block, 0, None, None, C.byref(cnt)) == 0, lib.hx_last_error()
    k = cnt.value
    tiles, rows = np.zeros(max(k, 1), np.uint32), np.zeros(max(k, 1), np.int64)
    rc = lib.hx_scan8q_items(rb, re_, nq, mul, n, block, k, tiles.ctypes.data_as(C.POINTER(C.c_uint32)),
                             rows.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cnt))
    assert rc == 0 and cnt.value == k
    return tiles[:k].astype(np.int64), rows[:k]


@pytest.mark.parametrize("nq", NQ)
@pytest.mark.parametrize("n", PERM_N)
def test_every_workgroup_walks_the_closed_form_and_the_union_is_the_range(n, nq):
    mul = perm_mul(n)
    assert n == 0 or math.gcd(mul, n) == 1
    for rb, re_ in launches(n):
        T = (re_ - rb) // 256
        lt = rb // 256 + np.arange(T, dtype=np.int64)
        pt = (lt * mul) % n if n else lt
        want = np.sort((pt[:, None] * 256 + np.arange(0, 256, 64)[None, :]).ravel())
        per_qt = {q: [] for q in range(nq)}
        early, uneven = 0, set()
        for block in range(256):
            tiles, rows = walk(rb, re_, nq, mul, n, block)
            et, er = closed_form(rb, re_, nq, mul, n, block)
            np.testing.assert_array_equal(tiles, et, err_msg=f"tiles n={n} nq={nq} [{rb},{re_}) block {block}")
            np.testing.assert_array_equal(rows, er, err_msg=f"rows n={n} nq={nq} [{rb},{re_}) block {block}")
            per_qt[(block >> 3) % nq].append(rows)
            early += len(rows) == 0
            uneven.add(len(rows))
        for q, parts in per_qt.items():      # the workgroups of one query tile: every 64-row item exactly once
            got = np.sort(np.concatenate(parts))
            np.testing.assert_array_equal(got, want, err_msg=f"union n={n} nq={nq} [{rb},{re_}) query tile {q}")
        if T * 2 < 8 * (32 // nq):
            assert early > 0                  # fewer halves than streams: some workgroups leave at once
        if T % 8:
            assert len(uneven) > 1            # XCDs with one tile fewer


def test_the_step_wraps_on_consecutive_pairs():
    """step > n / 2: the conditional subtract fires pair after pair (57 tiles, 2 streams per XCD: step 52)"""
    n, nq = 57, 16
    mul = perm_mul(n)
    step = (4 * (32 // nq) * mul) % n
    assert step > n / 2
    runs = 0
    for block in range(256):
        tiles, _ = walk(0, n * 256, nq, mul, n, block)
        p = tiles[::2]
        wrapped = (p[1:] < p[:-1])                     # p + step passed n
        runs += int((wrapped[1:] & wrapped[:-1]).sum())
        np.testing.assert_array_equal(p[1:], (p[:-1] + step) % n)
    assert runs > 0
    # and at the largest table: the 10M-row index's 39,063 tiles, every stream count
    n = 39063
    mul = perm_mul(n)
    assert any((4 * (32 // q) * mul) % n > n / 2 for q in NQ)


def test_bad_arguments_are_refused():
    lib = _lib.lib()
    cnt = C.c_int32()
    for args in ((0, 4096, 3, 1, 0, 0), (0, 4096, 32, 1, 0, 0), (100, 4096, 4, 1, 0, 0), (4096, 4096, 4, 1, 0, 0),
                 (0, 4096, 4, 1, 0, 256), (0, 4096, 4, 16, 16, 0)):
        assert lib.hx_scan8q_items(*args, 0, None, None, C.byref(cnt)) != 0, args
