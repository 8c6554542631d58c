"""map_embed on a CPU engine: the pooling twin, parity with transformers ``BertModel``, the op's
forms, errors, lease batching and encoder-only (``"head": "none"``) models."""
import base64
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops as registry
from agent_tpu_amd import ops
from agent_tpu_amd.models.bert import BertClassifier, config_for, from_hf_state_dict, init_random, param_specs

LENS = [1, 2, 15, 16, 17, 127, 128]
MODEL = "bert-tiny?batch=8&seq=32&seed=4"


# ------------------------------------------------------------------- twin
def _rows(B, S, H, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, S, H, generator=gen, dtype=torch.float64) * (0.5 + torch.rand(B, S, 1, generator=gen))
         + 0.3 * torch.randn(B, S, 1, generator=gen, dtype=torch.float64))
    gamma = 1 + 0.1 * torch.randn(H, generator=gen, dtype=torch.float64)
    beta = 0.05 * torch.randn(H, generator=gen, dtype=torch.float64)
    rs = torch.rsqrt(x.var(2, unbiased=False) + 1e-12)
    fin = torch.stack([rs, rs * x.mean(2)], -1).view(B * S, 2)
    return x, fin, gamma, beta


@pytest.mark.parametrize("S,lens", [(128, LENS), (1, [1, 1, 1]), (8, [8, 3, 1, 0, 9])])
def test_pool_embed_ref_is_layernorm_then_masked_mean(S, lens):
    B, H = len(lens), 64
    x, fin, gamma, beta = _rows(B, S, H, seed=S)
    ln = F.layer_norm(x, (H,), gamma, beta, 1e-12)
    lt = torch.tensor(lens, dtype=torch.int32)
    n = [min(max(v, 1), S) for v in lens]  # len is clamped to [1, S]
    want_mean = torch.stack([ln[b, :n[b]].mean(0) for b in range(B)])
    flat = x.view(B * S, H)
    for normalize in (False, True):
        norm = (lambda e: e / e.norm(dim=1, keepdim=True).clamp_min(1e-12)) if normalize else (lambda e: e)
        for mode, want in (("mean", want_mean), ("cls", ln[:, 0])):
            got = ops.pool_embed_ref(flat, lt, B, fin, gamma, beta, mode, normalize, dtype=torch.float64)
            torch.testing.assert_close(got, norm(want), atol=1e-12, rtol=1e-12)
            # rows already normalised (no fin): the plain masked mean / row 0
            got = ops.pool_embed_ref(ln.reshape(B * S, H), lt, B, mode=mode, normalize=normalize, dtype=torch.float64)
            torch.testing.assert_close(got, norm(want), atol=1e-12, rtol=1e-12)
    # rows >= len hold NaN (statistics too): the output is finite and unchanged
    px, pf = x.clone(), fin.view(B, S, 2).clone()
    for b in range(B):
        px[b, n[b]:] = float("nan")
        pf[b, n[b]:] = float("nan")
    a = ops.pool_embed_ref(flat, lt, B, fin, gamma, beta, "mean", True, dtype=torch.float64)
    p = ops.pool_embed_ref(px.view(B * S, H), lt, B, pf.view(B * S, 2), gamma, beta, "mean", True, dtype=torch.float64)
    assert torch.isfinite(p).all() and torch.equal(a, p)
    # the CPU path of the op wrapper is the fp32 twin
    e = ops.pool_embed(flat.float(), lt, B, fin.float(), gamma.float(), beta.float())
    assert e.dtype == torch.float32 and torch.equal(e, ops.pool_embed_ref(flat.float(), lt, B, fin.float(),
                                                                          gamma.float(), beta.float()))


def test_zero_embedding_normalises_to_zeros():
    e = ops.pool_embed_ref(torch.zeros(16, 64), torch.tensor([8, 3]), 2)
    assert torch.equal(e, torch.zeros(2, 64))
    assert ops.pool_embed_ok(128, 768) and ops.pool_embed_ok(1, 64) and ops.pool_embed_ok(512, 1024)
    assert not ops.pool_embed_ok(513, 768) and not ops.pool_embed_ok(128, 96) and not ops.pool_embed_ok(128, 1088)
    with pytest.raises(ValueError):
        ops.pool_embed(torch.zeros(16, 64), torch.tensor([8, 3]), 2, mode="max")


# -------------------------------------------------------------- HF parity
def test_embeddings_match_hf_bert_model():
    transformers = pytest.importorskip("transformers")
    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2,
                                   hidden_act="gelu", layer_norm_eps=1e-12, attn_implementation="eager")
    torch.manual_seed(11)
    hf = transformers.BertModel(hcfg).eval()
    with torch.no_grad():
        for p in hf.parameters():  # our pack stores bf16 weights: give HF the same values
            p.copy_(p.bfloat16().float())
    cfg = config_for("bert-tiny")
    sd = hf.state_dict()
    assert "embeddings.word_embeddings.weight" in sd  # a plain BertModel dict: no "bert." prefix, no classifier
    pack = from_hf_state_dict(cfg, sd)
    assert not pack["cls_w"].any() and not pack["cls_b"].any()
    ours = BertClassifier(cfg, pack, fp32=True)
    B, S = 4, 64
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 4096, (B, S), generator=g)
    lens = torch.tensor([64, 40, 7, 2])
    mask = (torch.arange(S).view(1, S) < lens.view(B, 1)).long()
    ids = ids * mask
    ids[:, 0] = 101
    with torch.no_grad():
        hs = hf(input_ids=ids, attention_mask=mask).last_hidden_state
    want = {"mean": (hs * mask.unsqueeze(-1)).sum(1) / lens.view(B, 1), "cls": hs[:, 0]}
    for pooling in ("mean", "cls"):
        for normalize in (False, True):
            got = ours.embed(ids.to(torch.int32), lens.to(torch.int32), pooling, normalize)
            ref = F.normalize(want[pooling], dim=1, eps=1e-12) if normalize else want[pooling]
            assert got.dtype == torch.float32 and got.shape == (B, 256)
            torch.testing.assert_close(got, ref, atol=2e-4, rtol=1e-4)
    sd.pop("pooler.dense.weight"), sd.pop("pooler.dense.bias")  # the pooler is optional
    assert not from_hf_state_dict(cfg, sd)["pool_w"].any()
    with pytest.raises(ValueError):
        ours.embed(ids.to(torch.int32), lens.to(torch.int32), "max")


# --------------------------------------------------------------------- op
@pytest.fixture
def embed(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("TASKS", raising=False)
    return registry.get_op("map_embed")


TEXTS = ["the quick brown fox", "", "jumps over, the lazy dog!", None, "MI355X " * 30, "x", "seven rows in all"]


def _b64(res, dt):
    return np.frombuffer(base64.b64decode(res["embeddings_b64"]), dtype=dt).reshape(res["shape"])


def test_op_output_forms_describe_the_same_array(embed, tmp_path):
    base = {"texts": TEXTS, "model_path": MODEL}
    rows = embed(dict(base))
    for k in ("ok", "op", "model_path", "row_count", "dim", "pooling", "normalize", "elapsed_ms", "rows_per_sec"):
        assert k in rows, k
    assert rows["op"] == "map_embed" and rows["row_count"] == 7 and rows["dim"] == 256 and rows["model_path"] == MODEL
    assert rows["pooling"] == "mean" and rows["normalize"] is True
    arr = np.asarray(rows["embeddings"], dtype=np.float32)
    assert arr.shape == (7, 256) and np.allclose(np.linalg.norm(arr, axis=1), 1.0, atol=1e-5)
    json.dumps(rows)
    b32 = embed(dict(base, output="base64"))
    assert b32["shape"] == [7, 256] and b32["dtype"] == "float32" and "embeddings" not in b32
    assert np.array_equal(_b64(b32, "<f4"), arr)
    b16 = embed(dict(base, output="base64", dtype="float16"))
    assert b16["dtype"] == "float16" and np.array_equal(_b64(b16, "<f2"), arr.astype(np.float16))
    r16 = embed(dict(base, dtype="float16"))
    assert np.array_equal(np.asarray(r16["embeddings"], dtype=np.float16), arr.astype(np.float16))
    out = tmp_path / "emb.npy"
    npy = embed(dict(base, output="npy", output_uri=str(out)))
    assert npy["output_uri"] == str(out) and npy["shape"] == [7, 256] and npy["bytes"] == os.path.getsize(out)
    assert np.array_equal(np.load(out), arr) and os.listdir(tmp_path) == ["emb.npy"]  # no temporary file left
    npy16 = embed(dict(base, output="npy", output_uri="file://" + str(out), dtype="float16"))
    assert npy16["dtype"] == "float16" and np.array_equal(np.load(out), arr.astype(np.float16))
    summ = embed(dict(base, output="summary"))
    assert np.allclose(summ["centroid"], arr.astype(np.float64).mean(0), atol=1e-7) and len(summ["centroid"]) == 256
    assert abs(summ["norm_mean"] - np.linalg.norm(arr.astype(np.float64), axis=1).mean()) < 1e-7
    raw = np.asarray(embed(dict(base, normalize=False, pooling="cls"))["embeddings"])
    assert not np.allclose(np.linalg.norm(raw, axis=1), 1.0, atol=1e-3)
    assert embed({"texts": [], "model_path": MODEL})["row_count"] == 0


def test_op_csv_form_equals_texts_form(embed, tmp_path):
    from agent_tpu_amd.io.csv import open_csv
    from agent_tpu_amd.utils.synthetic import write_csv

    path = write_csv(str(tmp_path / "t.csv"), 30, 12)
    tab = open_csv(path)
    col = tab.native.column_index("text")
    texts = [tab.native.row(i)[col] for i in range(4, 23)]
    a = embed({"texts": texts, "model_path": MODEL})
    b = embed({"source_uri": path, "start_row": 4, "shard_size": 19, "model_path": MODEL, "dataset_id": "d7"})
    assert b["row_count"] == 19 and a["embeddings"] == b["embeddings"]
    assert b["dataset_id"] == "d7" and b["start_row"] == 4 and b["end_row"] == 23 and b["dp_world_size"] == 1
    assert "embed_ms" in b["timing_ms"]
    tail = embed({"source_uri": path, "start_row": 25, "shard_size": 100, "model_path": MODEL, "output": "summary"})
    assert tail["row_count"] == 5 and tail["end_row"] == 30


def test_op_errors_are_fixed_and_listed_in_the_contract(embed, tmp_path, monkeypatch):
    from agent_tpu_amd.utils.synthetic import write_csv
    from ops import map_embed as me

    contract = open(os.path.join(os.path.dirname(me.__file__), "map_embed.CONTRACT.md")).read()
    for msg in me.ERRORS.values():
        assert msg in contract, msg
    path = write_csv(str(tmp_path / "t.csv"), 10, 8)
    cases = {
        "missing": {"model_path": MODEL},
        "texts": {"texts": "not a list", "model_path": MODEL},
        "pooling": {"texts": ["a"], "pooling": "max"},
        "normalize": {"texts": ["a"], "normalize": "yes"},
        "dtype": {"texts": ["a"], "dtype": "bfloat16"},
        "output": {"texts": ["a"], "output": "columns"},
        "output_uri": {"texts": ["a"], "output": "npy"},
        "range": {"source_uri": path, "start_row": -1, "model_path": MODEL},
        "column": {"source_uri": path, "text_column": "nope", "model_path": MODEL},
    }
    for key, payload in cases.items():
        with pytest.raises(ValueError) as ei:
            embed(payload)
        assert str(ei.value) == me.ERRORS[key], key
    with pytest.raises(ValueError) as ei:
        embed({"texts": ["a"], "output": "npy", "output_uri": "s3://bucket/e.npy"})
    assert str(ei.value) == me.ERRORS["output_uri"]
    assert set(cases) | {"too_large"} == set(me.ERRORS)
    with pytest.raises(ValueError) as ei:
        embed(None)
    assert str(ei.value) == me.ERRORS["missing"]
    # the JSON-size refusal: rows only, and it names the two forms that scale
    monkeypatch.setenv("MAP_EMBED_MAX_JSON_VALUES", str(256 * 3))
    assert embed({"texts": ["a", "b", "c"], "model_path": MODEL})["row_count"] == 3
    for payload in ({"texts": ["a", "b", "c", "d"], "model_path": MODEL},
                    {"source_uri": path, "shard_size": 4, "model_path": MODEL}):
        with pytest.raises(ValueError) as ei:
            embed(payload)
        assert str(ei.value) == me.ERRORS["too_large"] and "base64" in str(ei.value) and "npy" in str(ei.value)
        assert embed(dict(payload, output="base64"))["row_count"] == 4
    with pytest.raises(FileNotFoundError):  # no fallback stub
        embed({"texts": ["a"], "model_path": "/nope/model.safetensors"})


def test_batch_handler_matches_single_jobs_and_a_bad_job_fails_alone(embed):
    from ops import map_embed as me

    batch = registry.get_batch_op("map_embed")
    assert batch is not None
    payloads = [
        {"texts": TEXTS[:3], "model_path": MODEL},
        {"texts": TEXTS[3:], "model_path": MODEL, "pooling": "cls", "normalize": False},
        {"texts": "oops", "model_path": MODEL},
        {"texts": TEXTS[4:6], "model_path": MODEL, "output": "base64", "dtype": "float16"},
        {"texts": ["a"], "model_path": MODEL, "pooling": "max"},
        {"model_path": MODEL},
        {"texts": TEXTS[:2], "model_path": MODEL, "output": "summary"},
    ]
    res = batch([dict(p) for p in payloads])
    assert [r[0] for r in res] == ["ok", "ok", "err", "ok", "err", "err", "ok"]
    assert str(res[2][1]) == me.ERRORS["texts"] and str(res[4][1]) == me.ERRORS["pooling"]
    assert str(res[5][1]) == me.ERRORS["missing"] and all(isinstance(res[i][1], ValueError) for i in (2, 4, 5))
    for i in (0, 1, 3, 6):
        one, got = embed(dict(payloads[i])), res[i][1]
        assert set(one) == set(got), i
        for k in one:
            if k in ("elapsed_ms", "rows_per_sec"):
                continue
            if k in ("embeddings", "centroid"):
                assert np.allclose(np.asarray(got[k]), np.asarray(one[k]), atol=1e-6, rtol=0), (i, k)
            elif k == "embeddings_b64":
                assert np.allclose(_b64(got, "<f2").astype(np.float32), _b64(one, "<f2").astype(np.float32),
                                   atol=1e-6 + 2.0 ** -11, rtol=0), i  # fp16 rounding of values below 1
            elif k == "norm_mean":
                assert abs(got[k] - one[k]) < 1e-6
            else:
                assert got[k] == one[k], (i, k)


def test_encoder_only_model_embeds_and_classify_refuses_it(embed, tmp_path):
    from safetensors.torch import save_file

    cfg = config_for("bert-tiny")
    pack = init_random(cfg, seed=9)
    path = str(tmp_path / "enc.safetensors")
    save_file({n: pack[n].clone() for n, _, _ in param_specs(cfg) if not n.startswith(("pool_", "cls_"))}, path)
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny", "head": "none"}, f)
    model = path + "?batch=8&seq=32"
    got = np.asarray(embed({"texts": TEXTS, "model_path": model})["embeddings"], dtype=np.float32)
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    eng = ClassifyEngine(cfg, pack, torch.device("cpu"), batch_rows=8, seq_len=32)
    ref = eng.embed_texts(["" if t is None else t for t in TEXTS]).emb.numpy()
    assert np.allclose(got, ref, atol=1e-6, rtol=0)
    classify = registry.get_op("map_classify")
    with pytest.raises(ValueError) as ei:
        classify({"texts": ["a"], "model_path": model, "allow_fallback": False})
    assert str(ei.value) == "model has no classifier head"
    stub = classify({"texts": ["a"], "model_path": model})
    assert stub["fallback"] == "cpu" and stub["reason"] == "model has no classifier head" and stub["topk"] == []
    # without "head": "none" the same file is refused at load: it lacks tensors
    with open(path + ".json", "w") as f:
        json.dump({"preset": "bert-tiny"}, f)
    with pytest.raises(KeyError):
        embed({"texts": ["a"], "model_path": path + "?batch=8&seq=32&x=1"})
