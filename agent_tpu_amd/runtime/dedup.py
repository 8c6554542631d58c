"""Near-duplicate groups over device-resident vectors: the middle of ``map_dedup``.

:func:`near_duplicates` is a similarity self-join with a threshold (``ops.sim_join``: every pair ``i < j`` with
``dot(x[i], x[j]) >= threshold``) followed by the connected components of those pairs
(``ops.cc_min_labels``: a row's label is the smallest id of its group, the row to keep).

Under DP every rank holds all rows and joins the row blocks ``b = rank (mod ws)`` of :data:`BLOCK_ROWS` rows
against the whole input. The blocks are dealt round-robin because the join only computes the triangle above
the diagonal: a contiguous split would give the first rank about twice the mean share. The pairs are
all-gathered to every rank and sorted by ``I << 32 | J``. A pair's score is a function of its two rows alone
and the sorted list of a set has one order, so the edge list, the labels and everything derived from them
have the same bits for every world size, block size and launch shape.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

BLOCK_ROWS = 4096
MIN_CAP = 65536


class Duplicates(NamedTuple):
    labels: torch.Tensor  # [N] int32: the smallest id of the row's group (equal on every rank)
    pairs: torch.Tensor  # [P, 2] int32, sorted by (I, J): every pair at or above the threshold
    scores: torch.Tensor  # [P] fp32
    rounds: int  # hook rounds of the connected components


def join_block(x: torch.Tensor, b0: int, b1: int, threshold: float, max_wgs: int = 0):
    """The pairs of the rows ``[b0, b1)`` against every row: (pairs ``[n, 2]``, scores ``[n]``), unordered. A
    block whose count exceeds the first ``cap`` is rerun once with ``cap = count``."""
    from .. import ops

    cap = max(4 * (b1 - b0), MIN_CAP)
    pairs, scores, count = ops.sim_join(x[b0:b1], x, threshold, b0, 0, cap, max_wgs)
    n = int(count.item())
    if n > cap:
        pairs, scores, count = ops.sim_join(x[b0:b1], x, threshold, b0, 0, n, max_wgs)
        assert int(count.item()) == n
    return pairs[:n], scores[:n]


def near_duplicates(x: torch.Tensor, threshold: float, rank: int = 0, ws: int = 1, total: Optional[int] = None,
                    block_rows: Optional[int] = None, max_wgs: int = 0) -> Duplicates:
    """The near-duplicate groups of the contiguous fp32 ``x [N, D]``, which every one of the ``ws`` ranks holds
    whole: ``total``, when given, must be ``N`` (every rank calls it and gets the same result). For the cosine
    metric the rows are expected normalised."""
    from .. import ops
    from ..parallel.dp import all_gather_rows

    N = int(x.shape[0])
    if total is not None and int(total) != N:
        raise ValueError("near_duplicates: every rank holds all rows")
    block_rows = BLOCK_ROWS if block_rows is None else int(block_rows)
    if block_rows < 1:
        raise ValueError("near_duplicates: block_rows must be >= 1")
    parts_p, parts_s = [], []
    for b, b0 in enumerate(range(0, N, block_rows)):
        if b % ws != rank:
            continue
        p, s = join_block(x, b0, min(b0 + block_rows, N), threshold, max_wgs)
        parts_p.append(p)
        parts_s.append(s)
    if parts_p:
        pairs, scores = torch.cat(parts_p, 0), torch.cat(parts_s, 0)
    else:
        pairs = torch.empty((0, 2), dtype=torch.int32, device=x.device)
        scores = torch.empty((0,), dtype=torch.float32, device=x.device)
    if ws > 1:
        pairs, scores = all_gather_rows(pairs.contiguous(), scores.contiguous())
    pairs, scores = ops.sort_pairs(pairs, scores)
    labels, rounds = ops.cc_min_labels(pairs, N, with_rounds=True)
    return Duplicates(labels, pairs, scores, rounds)
