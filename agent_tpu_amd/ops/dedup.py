"""Near-duplicate building blocks: the similarity join with a threshold and the connected components of its pairs.

``sim_join`` (``csrc/kernels/sim_join.hip``) emits every pair ``(I, J) = (x_base + i, y_base + j)`` with
``I < J`` and ``score(i, j) = dot(x[i], y[j]) >= threshold`` (an fp32 compare). The ``[Nx, Ny]`` score matrix is
never written. A score is ONE fp32 accumulator on the exact f32 MFMA fed in ``sim_topk``'s column order (a
function of ``D`` alone), so it has the bits ``sim_topk(x[i:i+1], y, ...)`` reports for row ``j`` whatever the
launch shape, ``Nx`` or ``Ny``, and the emitted SET is a function of the rows alone. The lower id is always the
``x``-side operand, and a row never pairs with itself. The self-join of a corpus is ``y = corpus`` with
``x = corpus[b0:b1]``, ``x_base = b0``; a rectangle join is the same call with ``y_base >= x_base + Nx``.

At most ``cap`` pairs are stored, in arbitrary order; ``count`` is always the true total. Every consumer sorts
the list (:func:`sort_pairs`) or reduces it order-free.

``cc_min_labels`` gives every node the smallest id in its connected component: rounds of ``atomicMin`` hooks
and pointer-jumping compression until a round changes nothing. The fixed point is unique, so the result does
not depend on the order of the edges or of the hooks.

Every ``_ref`` twin is also the CPU path. ``sim_join_ref`` accumulates fp32 scores one column at a time, as
``kmeans_assign_ref`` does, so a pair's score does not depend on the batch it is in.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .._native import native, ptr, launch_stream
from ._util import check, same_device

MAX_ID = 2 ** 31 - 256


def sim_join_ok(D: int) -> bool:
    """The ``D`` the kernel takes: ``sim_topk_ok``'s, a multiple of 64 from 64 to 1024."""
    return D % 64 == 0 and 64 <= D <= 1024


def sort_pairs(pairs: torch.Tensor, scores: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The list ordered by the int64 key ``I << 32 | J`` (pairs are distinct: the order is total)."""
    key = (pairs[:, 0].to(torch.int64) << 32) | pairs[:, 1].to(torch.int64)
    order = torch.sort(key).indices
    return pairs[order].contiguous(), scores[order].contiguous()


def _check_join(x, y, threshold, x_base, y_base, cap) -> None:
    check(x.dim() == 2 and y.dim() == 2 and x.shape[1] == y.shape[1], "sim_join: x [Nx, D] and y [Ny, D]")
    check(x.dtype == torch.float32 and y.dtype == torch.float32, "sim_join: x and y must be fp32")
    check(x.is_contiguous() and y.is_contiguous(), "sim_join: contiguous tensors")
    check(isinstance(threshold, (int, float)) and not isinstance(threshold, bool), "sim_join: threshold must be a number")
    for name, v in (("x_base", x_base), ("y_base", y_base)):
        check(isinstance(v, int) and not isinstance(v, bool) and v >= 0, f"sim_join: {name} must be an int >= 0")
    check(x.shape[0] >= 1 and y.shape[0] >= 1 and x_base + x.shape[0] <= MAX_ID and y_base + y.shape[0] <= MAX_ID,
          "sim_join: Nx, Ny >= 1 and every id below 2^31 - 256")
    check(isinstance(cap, int) and not isinstance(cap, bool) and cap >= 0, "sim_join: cap must be an int >= 0")
    same_device(x, y)


def sim_join_ref(x: torch.Tensor, y: torch.Tensor, threshold: float, x_base: int = 0, y_base: int = 0,
                 cap: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """PyTorch twin and CPU path: fp32 scores accumulated one column at a time, the threshold and ``I < J``
    applied, the pairs SORTED (the first ``cap`` of them when ``cap`` is given) -> (pairs ``[n, 2]`` int32,
    scores ``[n]`` fp32, count ``[1]`` int64, the true total)."""
    _check_join(x, y, threshold, x_base, y_base, 0 if cap is None else cap)
    Nx, D = x.shape
    Ny = y.shape[0]
    yt = y.T.contiguous()
    s = torch.zeros((Nx, Ny), dtype=torch.float32, device=x.device)
    for d in range(D):
        s += x[:, d:d + 1] * yt[d]
    I = torch.arange(Nx, device=x.device)[:, None] + x_base
    J = torch.arange(Ny, device=x.device)[None, :] + y_base
    hit = (s >= torch.tensor(threshold, dtype=torch.float32, device=x.device)) & (I < J)
    ij = hit.nonzero()  # row-major: already sorted by (I, J)
    pairs = torch.stack([ij[:, 0] + x_base, ij[:, 1] + y_base], 1).to(torch.int32)
    scores = s[hit]
    count = torch.tensor([pairs.shape[0]], dtype=torch.int64, device=x.device)
    if cap is not None:
        pairs, scores = pairs[:cap], scores[:cap]
    return pairs.contiguous(), scores.contiguous(), count


def sim_join(x: torch.Tensor, y: torch.Tensor, threshold: float, x_base: int = 0, y_base: int = 0, cap: int = 65536,
             max_wgs: int = 0, panel_rows: int = 0, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pairs ``[cap, 2]`` int32, scores ``[cap]`` fp32, count ``[1]`` int64) of the contiguous fp32 ``x [Nx, D]``
    against ``y [Ny, D]``. The first ``min(count, cap)`` entries are valid, in arbitrary order; on a CPU tensor
    they are the twin's (sorted) and the lists have that length. ``max_wgs`` caps the persistent grid and
    ``panel_rows`` (a multiple of 32) sets the rows of ``y`` per work item (0: the defaults); both exist for
    tests and benches and the emitted set depends on neither. ``out``: preallocated ``(pairs, scores)``."""
    _check_join(x, y, threshold, x_base, y_base, cap)
    D = x.shape[1]
    check(sim_join_ok(D), f"sim_join: unsupported shape D={D}")
    check(isinstance(max_wgs, int) and max_wgs >= 0, "sim_join: max_wgs must be an int >= 0")
    check(isinstance(panel_rows, int) and panel_rows >= 0 and panel_rows % 32 == 0,
          "sim_join: panel_rows must be a multiple of 32")
    if not x.is_cuda:
        return sim_join_ref(x, y, threshold, x_base, y_base, cap)
    if out is None:
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=x.device)
        scores = torch.empty((cap,), dtype=torch.float32, device=x.device)
    else:
        pairs, scores = out
        check(pairs.dtype == torch.int32 and pairs.shape == (cap, 2) and pairs.is_contiguous()
              and scores.dtype == torch.float32 and scores.shape == (cap,) and scores.is_contiguous(),
              "sim_join: out must be a contiguous int32 [cap, 2] and fp32 [cap]")
        same_device(x, pairs, scores)
    count = torch.empty((1,), dtype=torch.int64, device=x.device)
    native().sim_join(ptr(x), ptr(y), float(threshold), x.shape[0], y.shape[0], D, x_base, y_base,
                      ptr(pairs) if cap else 0, ptr(scores) if cap else 0, ptr(count), cap, max_wgs, panel_rows // 32,
                      launch_stream(x))
    return pairs, scores, count


# ------------------------------------------------------------------------------------ connected components
def _check_cc(pairs, N) -> None:
    check(isinstance(N, int) and not isinstance(N, bool) and 1 <= N <= MAX_ID, "cc_min_labels: N must be in [1, 2^31 - 256]")
    check(pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.dtype == torch.int32 and pairs.is_contiguous(),
          "cc_min_labels: pairs must be a contiguous int32 [E, 2]")
    if pairs.shape[0]:
        check(int(pairs.min()) >= 0 and int(pairs.max()) < N, "cc_min_labels: node ids must be in [0, N)")


def cc_min_labels_ref(pairs: torch.Tensor, N: int, with_rounds: bool = False):
    """PyTorch twin and CPU path: ``scatter_reduce(amin)`` hooks plus pointer jumping, to a fixed point."""
    _check_cc(pairs, N)
    parent = torch.arange(N, dtype=torch.int64, device=pairs.device)
    u, v = pairs[:, 0].to(torch.int64), pairs[:, 1].to(torch.int64)
    rounds = 0
    while pairs.shape[0] and rounds < N:
        rounds += 1
        pu, pv = parent[u], parent[v]
        hooked = parent.scatter_reduce(0, torch.maximum(pu, pv), torch.minimum(pu, pv), "amin")
        changed = not torch.equal(hooked, parent)
        parent = hooked
        while True:
            jumped = parent[parent]
            if torch.equal(jumped, parent):
                break
            parent = jumped
        if not changed:
            break
    labels = parent.to(torch.int32)
    return (labels, rounds) if with_rounds else labels


def cc_min_labels(pairs: torch.Tensor, N: int, with_rounds: bool = False):
    """labels ``[N]`` int32: the smallest id in every node's connected component of the graph with the edges
    ``pairs [E, 2]`` (``E = 0``: ``arange(N)``). ``with_rounds`` also returns the number of hook rounds."""
    _check_cc(pairs, N)
    if not pairs.is_cuda:
        return cc_min_labels_ref(pairs, N, with_rounds)
    nat, stream = native(), launch_stream(pairs)
    parent = torch.empty((N,), dtype=torch.int32, device=pairs.device)
    nat.cc_init(ptr(parent), N, stream)
    changed = torch.empty((1,), dtype=torch.int32, device=pairs.device)
    rounds, E = 0, int(pairs.shape[0])
    while E and rounds < N:  # parents only decrease: the rounds end; N is the hard cap
        rounds += 1
        nat.cc_round(ptr(pairs), E, ptr(parent), N, ptr(changed), stream)
        if int(changed.item()) == 0:
            break
    return (parent, rounds) if with_rounds else parent
