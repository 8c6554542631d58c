"""pool_embed (csrc/kernels/pool_embed.hip) against its PyTorch twin, BertClassifier.embed against
the fp32 CPU oracle and ATPU_EMBED_FUSED=0, the engine's embed paths and the map_embed op.

Tolerance of the kernel tests, per element, nothing hand-picked (:func:`_expect`): the fp32 twin's
measured error against its own fp64 run, plus the standard fp32 summation bound of the element's
pooling sum, ``len * 2^-24 * sum_j |term_j|`` with the terms in fp64 (``rstd_j g_j[n]`` and
``rstd_j mu_j`` scaled by ``|gamma[n]| / len``, and ``beta[n]``; ``x_j[n] / len`` without ``fin``).
With ``normalize`` the output is ``e_n / ||e||``: the bound ``d`` of ``e`` propagates as
``d_n / ||e|| + |e_n| ||d||_2 / ||e||^2`` (first order), and the norm is itself a sum of H squares
(relative bound ``H 2^-24`` on the sum, half of it on its root) followed by a square root, the
``max`` and a division (half an ulp, ``2^-24`` relative, each).
"""
import base64
import os

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.models.bert import BertClassifier, BertConfig, config_for, init_random

pytestmark = pytest.mark.gpu

LENS = [1, 2, 15, 16, 17, 127, 128]
U = 2.0 ** -24
_cache = {}


def _expect(x, lens, B, fin, gamma, beta, mode, normalize):
    """-> (fp32 twin's output, per-element tolerance) for CPU inputs; see the module docstring."""
    twin = ops.pool_embed_ref(x, lens, B, fin, gamma, beta, mode, normalize)
    d64 = lambda t: None if t is None else t.double()  # noqa: E731
    exact = ops.pool_embed_ref(x, lens, B, d64(fin), d64(gamma), d64(beta), mode, normalize, dtype=torch.float64)
    twin_err = (twin.double() - exact).abs().max().item()
    H = x.shape[1]
    S = x.shape[0] // B
    n = (torch.ones(B, dtype=torch.int64) if mode == "cls" else lens.long().clamp(1, S)).view(B, 1)
    live = (torch.arange(S).view(1, S) < n).view(B, S, 1)
    zero = torch.zeros((), dtype=torch.float64)
    xx = torch.where(live, x.double().view(B, S, H), zero)
    if fin is not None:
        rstd = torch.where(live, fin[:, 0].double().view(B, S, 1), zero)
        rm = torch.where(live, fin[:, 1].double().view(B, S, 1), zero)
        terms = ((xx * rstd).abs().sum(1) + rm.abs().sum(1)) * gamma.double().abs().view(1, H) / n + beta.double().abs()
    else:
        terms = xx.abs().sum(1) / n
    d = n * U * terms
    if normalize:
        e = ops.pool_embed_ref(x, lens, B, d64(fin), d64(gamma), d64(beta), mode, False, dtype=torch.float64)
        nrm = e.norm(dim=1, keepdim=True).clamp_min(1e-12)
        d = d / nrm + e.abs() * d.norm(dim=1, keepdim=True) / nrm ** 2 + exact.abs() * (H * U / 2 + 3 * U)
    return twin, twin_err + d


def _case(H, S, B):
    """Inputs (CPU) shared by the tests of one shape: raw rows, their statistics, gamma / beta."""
    key = (H, S, B)
    if key not in _cache:
        gen = torch.Generator().manual_seed(H + 7 * S + B)
        lens = torch.tensor([min(LENS[(3 * i + B) % len(LENS)], S) if S > 1 else 1 for i in range(B)],
                            dtype=torch.int32)
        if S == 512:
            lens = torch.tensor([512, 257][:B] + [100] * (B - 2), dtype=torch.int32)
        g = (torch.randn(B * S, H, generator=gen) * (0.5 + torch.randn(B * S, 1, generator=gen).abs())
             + 0.3 * torch.randn(B * S, 1, generator=gen)).bfloat16()
        xf = g.float()
        rs = torch.rsqrt(xf.var(1, unbiased=False) + 1e-12)
        fin = torch.stack([rs, rs * xf.mean(1)], -1).contiguous()
        gamma = 1 + 0.1 * torch.randn(H, generator=gen)
        beta = 0.05 * torch.randn(H, generator=gen)
        _cache[key] = (g, fin, gamma, beta, lens)
    return _cache[key]


def _poisoned(g, lens, B, S, H, dev, mode):
    dg = g.to(dev).view(B, S, H).clone()
    for b in range(B):  # rows >= len (>= 1 in cls mode) contribute nothing: poison them
        dg[b, (1 if mode == "cls" else int(lens[b])):] = float("nan")
    return dg.view(B * S, H)


def _run_kernel_case(gpu, H, S, B, with_fin, mode, normalize):
    g, fin, gamma, beta, lens = _case(H, S, B)
    f, ga, be = (fin, gamma, beta) if with_fin else (None, None, None)
    twin, tol = _expect(g, lens, B, f, ga, be, mode, normalize)
    dev = lambda t: None if t is None else t.to(gpu)  # noqa: E731
    dg = _poisoned(g, lens, B, S, H, gpu, mode)
    dfin = dev(f)
    if dfin is not None:  # the statistics of dead rows are never used either
        dfin = dfin.view(B, S, 2).clone()
        for b in range(B):
            dfin[b, (1 if mode == "cls" else int(lens[b])):] = float("nan")
        dfin = dfin.view(B * S, 2)
    e = ops.pool_embed(dg, lens.to(gpu), B, dfin, dev(ga), dev(be), mode, normalize)
    torch.cuda.synchronize()
    assert e.shape == (B, H) and e.dtype == torch.float32
    diff = (e.cpu().double() - twin.double()).abs()
    print(f"H={H} S={S} B={B} fin={with_fin} {mode} norm={normalize}: max diff {diff.max().item():.3e} "
          f"min tol {tol.min().item():.3e} worst diff/tol {(diff / tol).max().item():.3f}")
    assert torch.isfinite(e).all() and (diff <= tol).all(), (diff - tol).max().item()
    e2 = ops.pool_embed(dg, lens.to(gpu), B, dfin, dev(ga), dev(be), mode, normalize)
    assert torch.equal(e, e2)  # bit-equal run to run
    return e


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("mode", ["mean", "cls"])
@pytest.mark.parametrize("with_fin", [True, False])
@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("H", [256, 768, 1024])
def test_pool_embed_matches_twin(gpu, H, B, with_fin, mode, normalize):
    _run_kernel_case(gpu, H, 128, B, with_fin, mode, normalize)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("mode", ["mean", "cls"])
@pytest.mark.parametrize("with_fin", [True, False])
@pytest.mark.parametrize("S", [1, 512])
def test_pool_embed_shortest_and_longest_sequences(gpu, S, with_fin, mode, normalize):
    _run_kernel_case(gpu, 768, S, 2, with_fin, mode, normalize)


@pytest.mark.parametrize("with_fin", [True, False])
@pytest.mark.parametrize("H", [256, 768, 1024])
def test_pool_embed_sequence_bits_do_not_depend_on_batch(gpu, H, with_fin):
    S = 128
    g, fin, gamma, beta, lens = _case(H, S, 17)
    f = (lambda t: t.to(gpu)) if with_fin else (lambda t: None)
    e17 = ops.pool_embed(g.to(gpu), lens.to(gpu), 17, f(fin), f(gamma), f(beta))
    for b in (0, 5, 16):
        fb = fin[b * S:(b + 1) * S].to(gpu).contiguous() if with_fin else None
        e1 = ops.pool_embed(g[b * S:(b + 1) * S].to(gpu), lens[b:b + 1].to(gpu), 1, fb, f(gamma), f(beta))
        assert torch.equal(e1[0], e17[b]), b


def test_pool_embed_zero_rows_and_unsupported_shapes(gpu):
    z = ops.pool_embed(torch.zeros((2 * 8, 64), dtype=torch.bfloat16, device=gpu),
                       torch.tensor([8, 3], dtype=torch.int32, device=gpu), 2)
    assert torch.equal(z, torch.zeros_like(z))  # 0 / max(0, 1e-12), not NaN
    lens = torch.ones(1, dtype=torch.int32, device=gpu)
    for H in (96, 1088):  # not a multiple of 64; above 1024
        with pytest.raises(ValueError):
            ops.pool_embed(torch.zeros((128, H), dtype=torch.bfloat16, device=gpu), lens, 1)
    with pytest.raises(ValueError):  # 513 tokens
        ops.pool_embed(torch.zeros((513, 64), dtype=torch.bfloat16, device=gpu), lens, 1)
    with pytest.raises(ValueError):
        ops.pool_embed(torch.zeros((128, 64), dtype=torch.bfloat16, device=gpu), lens, 1, mode="max")


# ------------------------------------------------------------------ model
S = 128


def _model_case(cfg, seed):
    """The perturbed gammas / betas and the 16 rows of test_cls_attend_gpu._model_case."""
    pack = init_random(cfg, seed=seed, bias_std=0.02)
    gen = torch.Generator().manual_seed(seed + 1)
    for name in pack.names():
        if name.endswith("_g"):
            pack[name].copy_(1 + 0.1 * torch.randn(pack[name].shape, generator=gen))
        elif name.endswith("ln_b") or name.endswith("ln1_b") or name.endswith("ln2_b"):
            pack[name].copy_(0.05 * torch.randn(pack[name].shape, generator=gen))
    B = 16
    ids = torch.randint(1000, cfg.vocab_size, (B, S), generator=gen, dtype=torch.int32)
    ids[:, 0] = 101
    lens = torch.tensor([2, 3, 15, 16, 17, 31, 40, 64, 65, 90, 100, 111, 120, 127, 128, 128], dtype=torch.int32)
    ids[torch.arange(S).view(1, S) >= lens.view(B, 1)] = 0
    return pack, ids, lens


def _cfg(name):
    return (config_for("bert-tiny", num_labels=3) if name == "bert-tiny"
            else BertConfig(vocab_size=4096, hidden=768, layers=2, heads=12, intermediate=3072, num_labels=3))


@pytest.mark.parametrize("name", ["bert-tiny", "h768-2layer"])
def test_fused_mean_embedding_against_oracle(gpu, name, monkeypatch):
    """B = 16, S = 128 (the smallest batch the folded encoder takes): the fused path's error against
    the fp32 CPU oracle is at most 1.5x that of ATPU_EMBED_FUSED=0 on the same rows."""
    cfg = _cfg(name)
    pack, ids, lens = _model_case(cfg, seed=31)
    oracle = BertClassifier(cfg, pack, fp32=True)
    dpack = pack.to(gpu)
    for normalize in (True, False):
        ref = oracle.embed(ids, lens, "mean", normalize)
        err = {}
        for flag in ("0", "1"):
            monkeypatch.setenv("ATPU_EMBED_FUSED", flag)
            m = BertClassifier(cfg, dpack)
            assert m.can_fold(16, S) and m.embed_fused == (flag == "1")
            e = m.embed(ids.to(gpu), lens.to(gpu), "mean", normalize)
            assert e.shape == (16, cfg.hidden) and e.dtype == torch.float32 and torch.isfinite(e).all()
            err[flag] = (e.cpu() - ref).abs().max().item()
        print(f"{name} normalize={normalize}: mean-embedding err vs fp32 oracle: unfused {err['0']:.3e} "
              f"fused {err['1']:.3e} ratio {err['1'] / err['0']:.3f}")
        assert err["1"] <= 1.5 * err["0"], err


def test_cls_embedding_is_the_normalised_encoder_output(gpu):
    cfg = _cfg("bert-tiny")
    pack, ids, lens = _model_case(cfg, seed=31)
    m = BertClassifier(cfg, pack.to(gpu))
    h = m.encoder(ids.to(gpu), lens.to(gpu))
    assert h.shape == (16, cfg.hidden)  # the pruned last layer: [CLS] states
    e = m.embed(ids.to(gpu), lens.to(gpu), "cls", True)
    twin, tol = _expect(h.cpu(), lens, 16, None, None, None, "cls", True)
    assert ((e.cpu().double() - twin.double()).abs() <= tol).all()
    ref = BertClassifier(cfg, pack, fp32=True).embed(ids, lens, "cls", True)
    print(f"cls embedding err vs fp32 oracle {(e.cpu() - ref).abs().max().item():.3e}")


@pytest.mark.parametrize("pooling", ["mean", "cls"])
def test_int8_embed_pools_its_own_encoder_output(gpu, pooling):
    cfg = _cfg("bert-tiny")
    pack, ids, lens = _model_case(cfg, seed=31)
    m = BertClassifier(cfg, pack.to(gpu), quant="int8")
    dids, dlens = ids.to(gpu), lens.to(gpu)
    e = m.embed(dids, dlens, pooling, True)
    h = m.encode(dids, dlens, cls_only_last=False) if pooling == "mean" else m.encoder(dids, dlens)
    twin, tol = _expect(h.cpu().contiguous(), lens, 16, None, None, None, pooling, True)
    diff = (e.cpu().double() - twin.double()).abs()
    assert (diff <= tol).all(), (diff - tol).max().item()


# ----------------------------------------------------------------- engine
@pytest.fixture
def invariant():
    prev = ops.set_batch_invariant(True)
    yield
    ops.set_batch_invariant(prev)


def _engine(gpu, **kw):
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    cfg = config_for("bert-tiny", num_labels=3)
    return ClassifyEngine(cfg, init_random(cfg, seed=5, device=gpu), gpu, batch_rows=32, seq_len=128, topk=3, **kw)


def _texts(n, seed=3):
    from agent_tpu_amd.utils.synthetic import make_text_rows

    rows = make_text_rows(n, 40, seed)
    rows[1] = ""
    rows[2] = "one"
    return rows


@pytest.mark.parametrize("pooling,normalize", [("mean", True), ("cls", False)])
def test_embed_texts_graph_equals_eager(gpu, pooling, normalize):
    rows = _texts(21)
    a = _engine(gpu).embed_texts(rows, pooling, normalize)
    b = _engine(gpu, use_graph=False).embed_texts(rows, pooling, normalize)
    assert a.rows == 21 and a.emb.shape == (21, 256) and a.emb.dtype == torch.float32 and not a.emb.is_cuda
    assert torch.isfinite(a.emb).all() and torch.equal(a.emb, b.emb)
    if normalize:
        torch.testing.assert_close(a.emb.norm(dim=1), torch.ones(21), atol=1e-5, rtol=0)


def test_embed_table_equals_embed_texts_and_leaves_classify_alone(gpu, invariant, tmp_path):
    from agent_tpu_amd._native import native
    from agent_tpu_amd.utils.synthetic import write_csv

    path = write_csv(str(tmp_path / "e.csv"), 80, 40)
    tab = native().CsvTable(path)
    col = tab.column_index("text")
    eng = _engine(gpu)
    rows = [tab.row(i)[col] for i in range(80)]
    before = eng.classify_texts(rows[:21])
    # the slots' classify graphs exist first: the embed graphs are captured into their pools
    ti, ts, _ = eng.classify_table(tab, 0, 80, col)
    ti, ts = ti.clone(), ts.clone()
    m0 = eng.memory_bytes()
    # 3 .. 74: two full batches and a partial one (n larger than two batches); 40 .. 49: one partial batch
    for start, n in ((3, 71), (40, 9)):
        emb, st = eng.embed_table(tab, start, n, col, "mean", True)
        assert emb.is_cuda and emb.shape == (n, 256) and st.rows == n and st.batches == (n + 31) // 32
        ref = eng.embed_texts(rows[start:start + n], "mean", True)
        assert torch.equal(emb.cpu(), ref.emb), (start, n)
    emb2, st2 = eng.embed_table(tab, 3, 71, col, "mean", True, stage_timing=True)
    assert torch.equal(emb2.cpu(), eng.embed_texts(rows[3:74], "mean", True).emb) and "device_embed_ms" in st2.timing_ms
    assert eng.memory_bytes() > m0  # the embed graphs' outputs are counted once they exist
    after = eng.classify_texts(rows[:21])
    assert torch.equal(before.idx, after.idx) and torch.equal(before.score, after.score)
    ti2, ts2, _ = eng.classify_table(tab, 0, 80, col)
    assert torch.equal(ti, ti2) and torch.equal(ts, ts2)


def test_embed_first_then_classify_on_one_engine(gpu, tmp_path):
    """An engine whose first job is an embed (its graphs get pools of their own) still classifies,
    and embeds the same bits afterwards."""
    from agent_tpu_amd._native import native
    from agent_tpu_amd.utils.synthetic import write_csv

    tab = native().CsvTable(write_csv(str(tmp_path / "f.csv"), 70, 40))
    col = tab.column_index("text")
    eng = _engine(gpu)
    e1 = eng.embed_table(tab, 0, 70, col, "cls", False)[0].clone()
    idx, sc, _ = eng.classify_table(tab, 0, 70, col)
    ref = _engine(gpu).classify_table(tab, 0, 70, col)
    assert torch.equal(idx, ref[0]) and torch.equal(sc, ref[1])
    assert torch.equal(eng.embed_table(tab, 0, 70, col, "cls", False)[0], e1)


# --------------------------------------------------------------------- op
def test_map_embed_op_csv_equals_texts_and_float16_is_rounded(gpu, invariant, tmp_path, monkeypatch):
    from agent_tpu_amd._native import native
    from agent_tpu_amd.utils.synthetic import write_csv
    from ops.map_embed import map_embed

    monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
    model = "bert-tiny?batch=32&seed=2"
    path = write_csv(str(tmp_path / "o.csv"), 50, 30)
    tab = native().CsvTable(path)
    rows = [tab.row(i)[tab.column_index("text")] for i in range(5, 42)]
    a = map_embed({"texts": rows, "model_path": model, "output": "base64"})
    b = map_embed({"source_uri": path, "start_row": 5, "shard_size": 37, "model_path": model, "output": "base64"})
    assert a["ok"] and b["ok"] and a["shape"] == b["shape"] == [37, 256] and a["dim"] == 256
    assert a["embeddings_b64"] == b["embeddings_b64"] and b["start_row"] == 5 and b["end_row"] == 42
    f32 = np.frombuffer(base64.b64decode(a["embeddings_b64"]), dtype="<f4").reshape(37, 256)
    h = map_embed({"texts": rows, "model_path": model, "output": "base64", "dtype": "float16"})
    f16 = np.frombuffer(base64.b64decode(h["embeddings_b64"]), dtype="<f2").reshape(37, 256)
    assert h["dtype"] == "float16" and np.array_equal(f16, f32.astype(np.float16))
    out = str(tmp_path / "e.npy")
    n = map_embed({"texts": rows, "model_path": model, "output": "npy", "output_uri": out})
    assert np.array_equal(np.load(out), f32) and n["bytes"] == os.path.getsize(out)
