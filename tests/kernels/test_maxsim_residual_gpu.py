"""``maxsim_index_rc`` and ``residual_encode`` (csrc/kernels/maxsim_residual.hip) on the GPU: the encoder equal to
its twin byte for byte (residuals on a cutoff and one ulp either side included), the scores with the bits of
``ops.maxsim_index`` on the decoded fp32 tensor in all three forms and within the derived bound of an fp64 loop,
clamped centroid ids, blind to what the neighbouring passages' codes and ids hold, and the op end to end on
``bert-tiny?late=64``.

Shapes: ``test_maxsim_index_gpu.py``'s. N = 7 passages of 17, 1, 33, 16, 70, 2 and 31 tokens (tails of the 16-row
tile, one-token passages), S = 20 with ``lens_q`` = (16, 20, 1), an empty list item, K = 5 centroids; at P = 1024
the fp32 tile holds 16 rows, so the 70-token passage is decoded in five tiles.

Bound. ``test_maxsim_gpu.py``'s derivation with rows that are not unit: with unit query rows and decoded rows of
norm at most R, a dot product of P terms errs by at most ``P * 2^-24 * R``, every maximum has magnitude at most R
and each of the ``len_q`` adds rounds once, so ``|err| <= len_q * (P + len_q) * 2^-23 * R``."""
import functools

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.ops.maxsim import maxsim_index_rc_ref, residual_encode_ref

pytestmark = pytest.mark.gpu

S, QN, K = 20, 3, 5
LENS = (17, 1, 33, 16, 70, 2, 31)
LENS_Q = (16, 20, 1)
PIDX = [4, 0, 6, 0, 2, 5]  # not monotone, with a repeat
QOFF = [0, 2, 2, 3, 6, 7, 9]  # item 1 is empty
QSEL = [2, 0, 1, 1, 2, 0, 1, 0, 2]  # not monotone
T = sum(LENS)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(P, b):
    """``(qv, lens_q, codes, cid, centroids, weights, off)`` on the host, built once and never changed: unit
    queries and centroids, random codes and ids, ascending weights of the size of a unit row's entries."""
    g = torch.Generator().manual_seed(8 * P + b)
    qv = torch.nn.functional.normalize(torch.randn(QN, S, P, generator=g), dim=-1)
    cent = torch.nn.functional.normalize(torch.randn(K, P, generator=g), dim=-1)
    w = (torch.randn(2 ** b, generator=g) * 0.5 / P ** 0.5).sort().values.contiguous()
    codes = torch.randint(0, 256, (T, P * b // 8), generator=g).to(torch.uint8)
    cid = torch.randint(0, K, (T,), generator=g).to(torch.int32)
    off = torch.tensor([0] + np.cumsum(LENS).tolist(), dtype=torch.int64)
    return qv, _i32(list(LENS_Q)), codes, cid, cent, w, off


def _run(gpu, fn, *tensors, **kw):
    out = fn(*[None if t is None else t.to(gpu) for t in tensors], **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("b", [1, 2, 4])
@pytest.mark.parametrize("P", [64, 192])
def test_encode_equals_the_twin(gpu, P, b):
    g = torch.Generator().manual_seed(P + b)
    cent = torch.randint(-64, 65, (K, P), generator=g).float() / 64
    cuts = (torch.arange(1, 2 ** b).float() - 2 ** (b - 1)) / 64  # exact next to the centroids' grid
    cid = torch.randint(0, K, (T,), generator=g).to(torch.int32)
    base = cent[cid.long()]
    x = base + 0.05 * torch.randn(T, P, generator=g)
    # every 7th value: a residual exactly on a cutoff, and one ulp above and below it (c + cutoff is exact, so the
    # fp32 subtraction returns the cutoff, or the cutoff moved by that ulp)
    n = torch.arange(0, T * P, 7)
    on = base.view(-1)[n] + cuts[(n // 21) % cuts.numel()]
    side = torch.tensor([0.0, float("inf"), float("-inf")])[(n // 7) % 3]
    x.view(-1)[n] = torch.where(side == 0, on, torch.nextafter(on, side))
    want = residual_encode_ref(x, cid, cent, cuts)
    r = (x - base).view(-1)[n]
    assert (r == cuts[(n // 21) % cuts.numel()]).sum() >= n.numel() // 3  # the on-cutoff residuals are exact
    got = _run(gpu, ops.residual_encode, x, cid, cent, cuts)
    assert got.dtype == torch.uint8 and got.shape == (T, P * b // 8) and torch.equal(got, want)


@pytest.mark.parametrize("b", [1, 2, 4])
@pytest.mark.parametrize("P", [64, 192, 1024])
def test_scores_have_the_bits_of_maxsim_index_on_the_decoded_rows(gpu, P, b):
    qv, lens_q, codes, cid, cent, w, off = _case(P, b)
    dec = ops.residual_decode(codes, cid, cent, w)  # [T, P] fp32 on the host
    forms = [(None, None, None), (_i32(PIDX), None, None), (_i32(PIDX), _i32(QOFF), _i32(QSEL))]
    for pidx, qoff, qsel in forms:
        got = _run(gpu, ops.maxsim_index_rc, qv, lens_q, codes, cid, cent, w, off, pidx, qoff, qsel)
        want = _run(gpu, ops.maxsim_index, qv, lens_q, dec, off, pidx, qoff, qsel)
        assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    # the all form against an fp64 loop over the same decoded values
    got = _run(gpu, ops.maxsim_index_rc, qv, lens_q, codes, cid, cent, w, off)
    q64, t64 = qv.double().numpy(), dec.double().numpy()
    want64 = torch.tensor([[sum(max(float(np.dot(q64[a, i], t64[j])) for j in range(int(off[p]), int(off[p + 1])))
                                for i in range(LENS_Q[a])) for p in range(len(LENS))] for a in range(QN)])
    lq = lens_q.double().view(-1, 1)
    bound = lq * (P + lq) * 2.0 ** -23 * float(dec.double().norm(dim=1).max())
    err = (got.double() - want64).abs()
    print(f"rc P={P} b={b}: max |gpu - fp64| {err.max():.3e}, bound {bound.min():.3e}..{bound.max():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("P,b", [(64, 1), (192, 4), (1024, 2)])
def test_device_data(gpu, P, b):
    qv, lens_q, codes, cid, cent, w, off = _case(P, b)
    want = _run(gpu, ops.maxsim_index_rc, qv, lens_q, codes, cid, cent, w, off)
    # ids outside [0, K) score as the clamped ids do, on the device and in the twin
    wild, clamped = cid.clone(), cid.clone()
    at = [0, 16, 17, 60, T - 1]
    wild[at] = _i32([-1, K + 7, -2 ** 31, 2 ** 31 - 1, K])
    clamped[at] = _i32([0, K - 1, 0, K - 1, K - 1])
    got = _run(gpu, ops.maxsim_index_rc, qv, lens_q, codes, wild, cent, w, off)
    assert torch.equal(_bits(got), _bits(_run(gpu, ops.maxsim_index_rc, qv, lens_q, codes, clamped, cent, w, off)))
    assert torch.equal(maxsim_index_rc_ref(qv, lens_q, codes, wild, cent, w, off),
                       maxsim_index_rc_ref(qv, lens_q, codes, clamped, cent, w, off))
    # the neighbours' codes and ids overwritten: a tile's clamped reads land on them, and no bit moves
    for p in range(len(LENS)):
        a, e = int(off[p]), int(off[p + 1])
        c2, i2 = codes ^ 0xFF, (cid + 1 + p) % K
        c2[a:e], i2[a:e] = codes[a:e], cid[a:e]
        got = _run(gpu, ops.maxsim_index_rc, qv, lens_q, c2, i2.to(torch.int32), cent, w, off, _i32([p]))
        assert torch.equal(_bits(got[:, 0]), _bits(want[:, p])), p


MODEL = "bert-tiny?late=64&batch=8&seq=32"
QUERIES = ["how do gpus multiply matrices", "Weather tomorrow?", "kalo mira ten"]
POOL = ["matrix cores multiply tiles", "", "gpus have many compute units", "rain, then sun", "kalo " * 40,
        "it's (not) here", "x"] + [f"passage number {i} about topic {i % 5}" for i in range(13)]  # 20 passages


@pytest.mark.parametrize("bits", [2, 4])
def test_map_maxsim_on_a_residual_index(gpu, tmp_path, monkeypatch, bits):
    from agent_tpu_amd.runtime import maxsim_index as mi
    from agent_tpu_amd.runtime import maxsim_residual as mr
    from agent_tpu_amd.runtime import search as rs
    from ops.map_maxsim import map_maxsim

    monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
    rs.clear_cache()
    uri, ref = str(tmp_path / "rc.npy"), str(tmp_path / "dec.npy")
    b = map_maxsim({"passages": POOL, "model_path": MODEL, "index_out": {
        "uri": uri, "compression": {"type": "residual", "bits": bits, "centroids": 16, "iterations": 4}}})
    main = np.load(uri)
    assert b["bits"] == bits and b["centroids"] == 16 and main.dtype == np.uint8 and main.shape == (b["token_count"], 64 * bits // 8)
    parts = [torch.from_numpy(np.load(p)) for p in (uri, mr.companion(uri, "cids"), mr.companion(uri, "centroids"),
                                                    mr.companion(uri, "weights"))]
    lens = torch.from_numpy(np.diff(np.load(b["offsets_uri"])))
    mi.write_index(ref, ops.residual_decode(*parts), lens, "float32")
    for extra in ({"top_k": 5}, {"candidates": [[19, 0, 4, 7], [], [4, 1, 18]], "return_scores": True}):
        got = map_maxsim(dict({"queries": QUERIES, "index_uri": uri, "model_path": MODEL}, **extra))
        want = map_maxsim(dict({"queries": QUERIES, "index_uri": ref, "model_path": MODEL}, **extra))
        assert got["index_dtype"] == f"residual{bits}" and got["passage_count"] == 20
        assert got["ranked"] == want["ranked"] and got.get("scores") == want.get("scores")  # the same floats
    assert got["index_cached"] is True
    rs.clear_cache()
