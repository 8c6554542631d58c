"""INT8 (W8A8) classify path on the CPU: the quantisation and GEMM references (the oracles of
``tests/kernels/test_int8_gpu.py``), the quantised model against the unquantised fp32 oracle,
and the ``?quant=`` model-path option of ``map_classify``."""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random


def special_rows(K: int, dtype=torch.float32) -> torch.Tensor:
    """Rows of width ``K`` (>= 16) that pin the scheme down (also used by the GPU test):
    0 all zero; 1 / 2 the only extreme first / last; 3 -amax; 4 ties at k + 0.5."""
    x = torch.zeros((5, K), dtype=torch.float32)
    g = torch.Generator().manual_seed(5)
    x[1] = torch.rand(K, generator=g) * 0.5
    x[1, 0] = 3.0
    x[2] = torch.rand(K, generator=g) * 0.5
    x[2, K - 1] = -2.0
    x[3] = torch.rand(K, generator=g) - 0.5
    x[3, 7] = -1.5
    # amax 127 -> inv = 1 exactly: x * inv = x, so k + 0.5 values are exact ties (bf16-exact too)
    x[4, 0] = 127.0
    x[4, 1:9] = torch.tensor([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 62.5])
    return x.to(dtype)


# ------------------------------------------------------------------ quantisation reference
def test_quantize_ref_special_rows():
    x = special_rows(64)
    q, s = ops.quantize_rows_i8_ref(x)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and q.shape == x.shape and s.shape == (5,)
    assert torch.equal(q[0], torch.zeros(64, dtype=torch.int8)) and s[0].item() == 1.0
    assert q[1, 0].item() == 127 and s[1].item() == (torch.tensor(3.0) / torch.tensor(127.0)).item()
    assert q[1, 1:].abs().max().item() <= 22  # 0.5 / 3 * 127 = 21.2
    assert q[2, 63].item() == -127 and s[2].item() == (torch.tensor(2.0) / torch.tensor(127.0)).item()
    assert q[3, 7].item() == -127 and q[3].min().item() == -127 and q[3].max().item() < 127
    # ties round to even
    assert q[4, :9].tolist() == [127, 0, 2, 2, 4, 0, -2, -2, 62]
    assert s[4].item() == 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_ref_error_bound(dtype):
    g = torch.Generator().manual_seed(2)
    x = (torch.randn((9, 256), generator=g) * torch.logspace(-3, 2, 9).unsqueeze(1)).to(dtype)
    q, s = ops.quantize_rows_i8_ref(x)
    assert q.abs().max().item() <= 127
    assert torch.equal(q.abs().amax(dim=1), torch.full((9,), 127, dtype=torch.int8))
    err = (q.double() * s.double().unsqueeze(1) - x.double()).abs()
    # Half a level. In exact arithmetic the bound is scale / 2; the scheme's three fp32 roundings
    # move a value that sits on a tie by at most 127 * 3 * 2^-24 = 2.3e-5 levels: x * inv is rounded
    # (half an ulp of <= 127), and inv * scale = (127 / amax) * (amax / 127) is 1 only to two
    # roundings, which scales q <= 127. bf16 inputs land on such ties routinely.
    levels = err / s.double().unsqueeze(1)
    print(f"max error {levels.max().item():.9f} levels")
    assert bool((levels <= 0.5 + 127 * 3 * 2.0 ** -24).all())
    # the op dispatches CPU tensors to the reference
    q2, s2 = ops.quantize_rows_i8(x)
    assert torch.equal(q, q2) and torch.equal(s, s2)


# ------------------------------------------------------------------ GEMM reference
def _operands(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    xq = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int8)
    wq = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8)
    xs = torch.rand(M, generator=g) * 0.02 + 0.001
    ws = torch.rand(N, generator=g) * 0.002 + 0.0001
    bias = torch.randn(N, generator=g) * 0.5
    res = torch.randn((M, N), generator=g).to(torch.bfloat16)
    return xq, xs, wq, ws, bias, res


def test_linear_i8_ref_raw_is_the_integer_matmul():
    xq, xs, wq, ws, _, _ = _operands(37, 48, 3072)
    xq[0], xq[1], wq[0], wq[1] = 127, -127, 127, -127  # |acc| = 127^2 * 3072 = 4.95e7 in the corner
    acc = ops.linear_i8_ref(xq, xs, wq, ws, raw=True)
    assert acc.dtype == torch.int32
    assert torch.equal(acc, (xq.int() @ wq.int().t()))
    assert acc.abs().max().item() > 1 << 24  # past fp32's exact integers: an fp32 accumulation would differ
    assert torch.equal(ops.linear_i8(xq, xs, wq, ws, raw=True), acc)


@pytest.mark.parametrize("use_bias,act,use_res", [(False, None, False), (True, None, False), (True, "gelu", False),
                                                  (True, None, True), (True, "gelu", True)])
def test_linear_i8_ref_epilogue_order(use_bias, act, use_res):
    xq, xs, wq, ws, bias, res = _operands(19, 32, 192, seed=1)
    y = ops.linear_i8(xq, xs, wq, ws, bias if use_bias else None, act=act, residual=res if use_res else None)
    # the formula, written out: (float(acc) * a_scale) * w_scale, + bias, GELU, + residual, RNE to bf16
    acc = (xq.int() @ wq.int().t())
    e = acc.to(torch.float32) * xs.view(-1, 1)
    e = e * ws.view(1, -1)
    if use_bias:
        e = e + bias.view(1, -1)
    if act == "gelu":
        e = torch.nn.functional.gelu(e)
    if use_res:
        e = e + res.to(torch.float32)
    assert y.dtype == torch.bfloat16
    assert torch.equal(y, e.to(torch.bfloat16))


def test_linear_i8_rejects_bad_operands():
    xq, xs, wq, ws, _, _ = _operands(4, 16, 64)
    with pytest.raises(ValueError):
        ops.linear_i8(xq, xs, wq[:, :32], ws)
    with pytest.raises(ValueError):
        ops.linear_i8(xq, xs, wq, ws, act="tanh")
    assert ops.linear_i8_ok(1, 16, 64) and ops.linear_i8_ok(300, 768, 3072)
    assert not ops.linear_i8_ok(8, 24, 64) and not ops.linear_i8_ok(8, 16, 96) and not ops.linear_i8_ok(0, 16, 64)
    assert not ops.linear_i8_ok(8, 16, (1 << 17) + 64)


# ------------------------------------------------------------------ quantised model vs the fp32 oracle
def _inputs(cfg, B, S):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, cfg.vocab_size, (B, S), generator=g, dtype=torch.int32)
    ids[:, 0] = 101
    lens = torch.tensor([S - 5 * i for i in range(B)], dtype=torch.int32).clamp(min=2)
    return ids, lens


def _model_err(preset, seed, B, S):
    cfg = config_for(preset, num_labels=7)
    pack = init_random(cfg, seed=seed, bias_std=0.02)
    ids, lens = _inputs(cfg, B, S)
    rl, _, _ = BertClassifier(cfg, pack, fp32=True, quant="none").forward(ids, lens, k=3)
    model = BertClassifier(cfg, pack, fp32=True, quant="int8")
    assert model.quant == "int8" and not model.can_fold(B, S)
    ql, _, _ = model.forward(ids, lens, k=3)
    z = model.quantized()
    assert z["l0.qkv_q"].dtype == torch.int8 and z["l0.qkv_s"].shape == (3 * cfg.hidden,)
    return ((ql - rl).abs().max() / rl.abs().max()).item()


@pytest.mark.parametrize("seed", [3, 11])
@pytest.mark.parametrize("B,S", [(8, 128), (3, 64)])
def test_int8_bert_tiny_vs_fp32_oracle(seed, B, S):
    err = _model_err("bert-tiny", seed, B, S)
    print(f"bert-tiny seed={seed} B={B} S={S}: max|dlogit|/max|logit| = {err:.5f}")
    assert err < 1e-2, err


@pytest.mark.parametrize("seed", [3, 11])
def test_int8_bert_base_vs_fp32_oracle(seed):
    err = _model_err("bert-base", seed, 4, 128)
    print(f"bert-base seed={seed} B=4 S=128: max|dlogit|/max|logit| = {err:.5f}")
    assert err < 5e-2, err


def test_quant_option_values(monkeypatch):
    cfg = config_for("bert-tiny", num_labels=3)
    pack = init_random(cfg, seed=0)
    monkeypatch.delenv("CLASSIFY_QUANT", raising=False)
    assert BertClassifier(cfg, pack).quant is None
    for off in ("", "none"):
        monkeypatch.setenv("CLASSIFY_QUANT", off)
        assert BertClassifier(cfg, pack).quant is None
    monkeypatch.setenv("CLASSIFY_QUANT", "int8")
    assert BertClassifier(cfg, pack).quant == "int8"
    assert BertClassifier(cfg, pack, quant="none").quant is None  # the argument wins over the environment
    with pytest.raises(ValueError, match="unknown quant"):
        BertClassifier(cfg, pack, quant="int4")
    monkeypatch.setenv("CLASSIFY_QUANT", "fp8")
    with pytest.raises(ValueError, match="unknown quant"):
        BertClassifier(cfg, pack)


def test_engine_counts_quantized_weights():
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    cfg = config_for("bert-tiny", num_labels=3)
    pack = init_random(cfg, seed=0)
    cpu = torch.device("cpu")
    plain = ClassifyEngine(cfg, pack, cpu, batch_rows=4, seq_len=32, topk=2, quant="none")
    quant = ClassifyEngine(cfg, pack, cpu, batch_rows=4, seq_len=32, topk=2, quant="int8")
    H, I, L = cfg.hidden, cfg.intermediate, cfg.layers
    extra = L * ((4 * H * H + 2 * H * I) + 4 * (3 * H + H + I + H))  # int8 weights + fp32 scales
    assert quant.memory_bytes() - plain.memory_bytes() == extra


# ------------------------------------------------------------------ the op's model-path option
def test_parse_spec_quant():
    from ops._gpu_runtime import parse_spec

    assert parse_spec("bert-tiny?quant=int8&labels=5").quant == "int8"
    assert parse_spec("bert-tiny?quant=int8&labels=5").labels == 5
    assert parse_spec("bert-tiny?labels=5").quant is None
    assert parse_spec("bert-tiny").quant is None
    with pytest.raises(ValueError, match="int4"):
        parse_spec("bert-tiny?quant=int4")


def test_map_classify_quant_option(monkeypatch):
    from ops import _gpu_runtime as rt
    from ops import map_classify as mc

    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("CLASSIFY_QUANT", raising=False)
    texts = ["the quick brown fox", "jumps over the lazy dog", ""]
    path = "bert-tiny?quant=int8&labels=5"
    out = mc.map_classify({"texts": texts, "model_path": path, "topk": 2, "allow_fallback": False})
    assert out["ok"] is True and out["model_path"] == path and out["row_count"] == 3
    plain = mc.map_classify({"texts": texts, "model_path": "bert-tiny?labels=5", "topk": 2, "allow_fallback": False})
    assert plain["ok"] is True and plain["model_path"] == "bert-tiny?labels=5"
    entries = rt.cache_info()["entries"] if hasattr(rt, "cache_info") else [k[0] for k in rt._cache]
    assert path in entries and "bert-tiny?labels=5" in entries  # distinct LRU entries
    assert rt._cache[(path, "cpu")].engine.model.quant == "int8"
    assert rt._cache[("bert-tiny?labels=5", "cpu")].engine.model.quant is None
    # an unknown value: the fallback stub with the reason, or raised without allow_fallback
    bad = mc.map_classify({"texts": texts, "model_path": "bert-tiny?quant=int4&labels=5"})
    assert bad["fallback"] == "cpu" and bad["topk"] == [] and "int4" in bad["reason"]
    with pytest.raises(ValueError, match="int4"):
        mc.map_classify({"texts": texts, "model_path": "bert-tiny?quant=int4&labels=5", "allow_fallback": False})
