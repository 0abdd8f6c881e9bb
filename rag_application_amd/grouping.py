"""Grouped search on the host: the model of hx_group and the path a grouped search takes when the
group key has no live `keyword` or `bool` column.

Qdrant's `query_points_groups(group_by, limit, group_size)`: the best `limit` groups of a ranked list, at most
`group_size` hits each.  The list -- the POOL of a query -- is walked in rank order:

  a row whose key is missing or null is skipped (Qdrant leaves out points without the field);
  a row whose group is open and holds fewer than `group_size` hits joins it;
  a row whose group is not open opens it while fewer than `limit` groups are open;
  every other row is dropped (once `limit` groups are open, later rows of open groups with room are still taken).

Groups come out ordered by their best hit, hits inside a group by rank.  The engine's order is total (score descending,
id ascending), so the result is a pure function of the pool and the keys: the kernel (group.hip) computes the same
thing in closed form and is tested against `group_ranked` key for key, as `filters.matches` is both the oracle and the
fallback of the payload index's masks."""
from __future__ import annotations

from typing import Any, Hashable, List, Optional, Sequence, Tuple

from . import filters as _filters

MAX_SLOTS = 2048      # limit * group_size, and the pool, at most (hx.h: hx_group)


def check_sizes(limit: int, group_size: int) -> None:
    if isinstance(limit, bool) or isinstance(group_size, bool) or not isinstance(limit, int) or not isinstance(group_size, int):
        raise ValueError("limit and group_size must be integers")
    if limit < 1 or group_size < 1 or limit * group_size > MAX_SLOTS:
        raise ValueError(f"limit and group_size must be at least 1 and limit * group_size at most {MAX_SLOTS}, "
                         f"got {limit} x {group_size}")


def group_ranked(codes: Sequence[Optional[Hashable]], G: int, S: int) -> List[List[int]]:
    """codes[i] = the group key of the row at rank i (None = skip the row).  Returns the groups, best first, each the
    ranks of its hits in rank order: at most G groups of at most S ranks."""
    check_sizes(G, S)
    groups: List[List[int]] = []
    place = {}
    for rank, code in enumerate(codes):
        if code is None:
            continue
        g = place.get(code)
        if g is None:
            if len(groups) < G:
                place[code] = len(groups)
                groups.append([rank])
        elif len(groups[g]) < S:
            groups[g].append(rank)
    return groups


def group_value(payload, key: str) -> Optional[Tuple[str, Any]]:
    """What forms a group on the Python path: the `str`, `bool` or `int` at `key` (a dotted path, as filters._get reads
    it), tagged with its type -- 1 and True are different groups, as "1" and 1 are.  None (the row is skipped) for a
    missing value, None, a float, a list, a dict or anything else."""
    v = _filters._get(payload, key)
    if v is _filters._MISSING or v is None:
        return None
    if type(v) is bool:
        return ("bool", v)
    if type(v) is int:
        return ("int", v)
    if type(v) is str:
        return ("str", v)
    return None
