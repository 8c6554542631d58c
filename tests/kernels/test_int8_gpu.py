"""INT8 (W8A8) kernels on the GPU (csrc/kernels/gemm_i8.hip) against their CPU twins
(ops/linear_i8.py): exact accumulators, bit-identical quantisation, epilogues, batch invariance,
the fused LayerNorm + quantise pass, the quantised model and the engine under graph capture."""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random
from agent_tpu_amd.runtime.classify import ClassifyEngine

pytestmark = pytest.mark.gpu


def _int8(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-127, 128, shape, generator=g, dtype=torch.int8)


def _ones(n, gpu):
    return torch.ones(n, dtype=torch.float32, device=gpu)


def _raw(a, w, gpu):
    a, w = a.to(gpu), w.to(gpu)
    return ops.linear_i8(a, _ones(a.shape[0], gpu), w, _ones(w.shape[0], gpu), raw=True)


def _bits(t):
    return t.cpu().view(torch.int32)


# ------------------------------------------------------------------ raw accumulators
@pytest.mark.parametrize("M,N,K", [(1, 16, 64), (130, 48, 192), (257, 272, 768), (64, 768, 3072)])
def test_gemm_i8_raw_exact(gpu, M, N, K):
    a, w = _int8((M, K), 1), _int8((N, K), 2)
    if K == 3072:
        # constant-sign rows: |acc| = 127^2 * 3072 = 4.95e7 > 2^24, so an fp32 accumulation cannot be exact
        a[0], w[0], w[1] = 127, 127, -127
        a[M - 1, ::2], w[N - 1, ::2] = -127, 127
    ref = ops.linear_i8_ref(a, None, w, None, raw=True)
    assert torch.equal(ref, a.int() @ w.int().t())
    if K == 3072:
        assert ref.abs().max().item() == 127 * 127 * 3072
    reps = 3 if (M, N, K) == (257, 272, 768) else 1  # repeated launches: races show as a changed tile
    for _ in range(reps):
        acc = _raw(a, w, gpu)
        assert acc.dtype == torch.int32 and torch.equal(acc.cpu(), ref)


def test_gemm_i8_identity_against_ramp(gpu):
    """A = I, asymmetric B: a swapped row/column map or a transposed store cannot pass."""
    a = torch.eye(128, dtype=torch.int8)
    n = torch.arange(256, dtype=torch.int32).view(256, 1)
    k = torch.arange(128, dtype=torch.int32).view(1, 128)
    w = ((3 * n + 7 * k) % 255 - 127).to(torch.int8)  # [256, 128] ramp, w[n][k] != w[k][n]
    acc = _raw(a, w, gpu)
    assert torch.equal(acc.cpu(), w.int().t())


def test_gemm_i8_strided_a(gpu):
    M, N, K = 130, 48, 192
    buf = _int8((M, K + 64), 3)
    a, w = buf[:, :K], _int8((N, K), 4)
    a_dev = buf.to(gpu)[:, :K]  # lda = K + 64
    assert a_dev.stride(0) == K + 64
    acc = ops.linear_i8(a_dev, _ones(M, gpu), w.to(gpu), _ones(N, gpu), raw=True)
    assert torch.equal(acc.cpu(), a.int() @ w.int().t())


# ------------------------------------------------------------------ quantiser
def _special_rows(K):
    """0 all zero; 1 / 2 the only extreme first / last; 3 -amax; 4 exact ties (amax 127 -> inv = 1)."""
    x = torch.zeros((5, K), dtype=torch.float32)
    g = torch.Generator().manual_seed(5)
    x[1] = torch.rand(K, generator=g) * 0.5
    x[1, 0] = 3.0
    x[2] = torch.rand(K, generator=g) * 0.5
    x[2, K - 1] = -2.0
    x[3] = torch.rand(K, generator=g) - 0.5
    x[3, 7] = -1.5
    x[4, 0] = 127.0
    x[4, 1:9] = torch.tensor([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 62.5])
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("K", [256, 768, 3072])
def test_quantize_rows_matches_cpu_twin(gpu, K):
    g = torch.Generator().manual_seed(K)
    rnd = (torch.randn((5, K), generator=g) * torch.logspace(-2, 1, 5).unsqueeze(1)).to(torch.bfloat16)
    for x in (rnd, _special_rows(K)):
        rq, rs = ops.quantize_rows_i8_ref(x)
        q, s = ops.quantize_rows_i8(x.to(gpu))
        assert q.dtype == torch.int8 and s.dtype == torch.float32
        assert torch.equal(q.cpu(), rq)
        assert torch.equal(_bits(s), _bits(rs))
    sq, ss = ops.quantize_rows_i8(_special_rows(K).to(gpu))
    assert ss[0].item() == 1.0 and not sq[0].any() and sq[1, 0].item() == 127 and sq[2, K - 1].item() == -127
    assert sq[3, 7].item() == -127 and sq[4, :9].tolist() == [127, 0, 2, 2, 4, 0, -2, -2, 62]
    # strided input: the left K columns of a wider buffer
    wide = torch.cat([rnd, rnd.flip(1)], dim=1).to(gpu)
    view = wide[:, :K]
    assert view.stride(0) == 2 * K
    q, s = ops.quantize_rows_i8(view)
    rq, rs = ops.quantize_rows_i8_ref(rnd)
    assert torch.equal(q.cpu(), rq) and torch.equal(_bits(s), _bits(rs))


# ------------------------------------------------------------------ epilogues
def _epi_operands(M, N, K):
    g = torch.Generator().manual_seed(M + N)
    xq, wq = _int8((M, K), 5), _int8((N, K), 6)
    xs = torch.rand(M, generator=g) * 0.02 + 0.001
    ws = torch.rand(N, generator=g) * 0.002 + 0.0001
    bias = torch.randn(N, generator=g) * 0.5
    res = torch.randn((M, N), generator=g).to(torch.bfloat16)
    return xq, xs, wq, ws, bias, res


@pytest.fixture(scope="module", params=[(130, 48, 192), (300, 768, 768)], ids=lambda s: "x".join(map(str, s)))
def epi_case(request):
    return _epi_operands(*request.param)


@pytest.mark.parametrize("use_bias,act,use_res", [(True, None, False), (True, "gelu", False), (True, None, True),
                                                  (False, None, False)],
                         ids=["bias", "bias_gelu", "bias_residual", "none"])
def test_gemm_i8_epilogues(gpu, epi_case, use_bias, act, use_res):
    xq, xs, wq, ws, bias, res = epi_case
    b, r = (bias if use_bias else None), (res if use_res else None)
    ref = ops.linear_i8_ref(xq, xs, wq, ws, b, act=act, residual=r).float()
    y = ops.linear_i8(xq.to(gpu), xs.to(gpu), wq.to(gpu), ws.to(gpu), b.to(gpu) if use_bias else None, act=act,
                      residual=r.to(gpu) if use_res else None)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == tuple(ref.shape)
    y = y.float().cpu()
    if act == "gelu":  # the kernels' polynomial GELU against erf: the bound of test_gemm_epilogues
        rel = ((y - ref).abs().max() / (ref.abs().max() + 1e-6)).item()
        print(f"gelu rel err {rel:.3e}")
        assert rel < 2e-2
        return
    # one bf16 ulp: FMA contraction may move the fp32 value by an ulp before the bf16 rounding
    excess = (y - ref).abs() - (2.0 ** -7 * ref.abs() + 1e-5 * ref.abs().max())
    print(f"mismatching elements {(y != ref).sum().item()} of {y.numel()}, worst excess {excess.max().item():.3e}")
    assert bool((excess <= 0).all())


# ------------------------------------------------------------------ batch invariance
def test_int8_batch_invariance(gpu):
    """16 rows alone (M = 16) and at offset 131 inside M = 300: the same bits."""
    K, N = 768, 272
    g = torch.Generator().manual_seed(8)
    big = (torch.randn((300, K), generator=g) * (torch.rand((300, 1), generator=g) + 0.1)).to(torch.bfloat16).to(gpu)
    small = big[131:147].contiguous()
    bq, bs = ops.quantize_rows_i8(big)
    sq, ss = ops.quantize_rows_i8(small)
    assert torch.equal(bq[131:147], sq) and torch.equal(_bits(bs[131:147]), _bits(ss))
    wq, ws = ops.quantize_rows_i8((torch.randn((N, K), generator=g) * 0.02).to(torch.bfloat16).to(gpu))
    bias = torch.randn(N, generator=g).to(gpu)
    res = torch.randn((300, N), generator=g).to(torch.bfloat16).to(gpu)
    yb = ops.linear_i8(bq, bs, wq, ws, bias, residual=res)
    ysm = ops.linear_i8(sq, ss, wq, ws, bias, residual=res[131:147].contiguous())
    assert torch.equal(yb[131:147].view(torch.int16), ysm.view(torch.int16))


# ------------------------------------------------------------------ LayerNorm + quantise
@pytest.mark.parametrize("N", [256, 768, 1024])
@pytest.mark.parametrize("with_res", [False, True])
def test_layernorm_quant_i8(gpu, N, with_res):
    g = torch.Generator().manual_seed(N)
    x = torch.randn((5, N), generator=g).to(torch.bfloat16).to(gpu)
    res = torch.randn((5, N), generator=g).to(torch.bfloat16).to(gpu) if with_res else None
    gamma = (torch.rand(N, generator=g) + 0.5).to(gpu)
    beta = (torch.randn(N, generator=g) * 0.1).to(gpu)
    ref = ops.layernorm(x, gamma, beta, 1e-12, residual=res)
    rq, rs = ops.quantize_rows_i8(ref)
    y, q, s = ops.layernorm_quant_i8(x, gamma, beta, 1e-12, residual=res)
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(q, rq) and torch.equal(_bits(s), _bits(rs))


# ------------------------------------------------------------------ model and engine
@pytest.mark.parametrize("preset,B,S", [("bert-tiny", 8, 128), ("bert-tiny", 3, 64), ("bert-base", 4, 128)])
def test_int8_model_gpu_vs_cpu_twin(gpu, preset, B, S):
    """Observed max|dlogit| / max|logit| on an MI355X: see docs/PERF_NOTES.md (INT8 encoder GEMMs)."""
    cfg = config_for(preset, num_labels=7)
    pack = init_random(cfg, seed=3, bias_std=0.02)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, cfg.vocab_size, (B, S), generator=g, dtype=torch.int32)
    ids[:, 0] = 101
    lens = torch.tensor([S - 5 * i for i in range(B)], dtype=torch.int32).clamp(min=2)
    rl, _, _ = BertClassifier(cfg, pack, fp32=True, quant="int8").forward(ids, lens, k=3)
    dev = BertClassifier(cfg, pack.to(gpu), quant="int8")
    gl, _, _ = dev.forward(ids.to(gpu), lens.to(gpu), k=3)
    ratio = (gl.cpu() - rl).abs().max().item() / rl.abs().max().item()
    print(f"int8 {preset} B={B} S={S}: max|dlogit|/max|logit| = {ratio:.5f}")
    assert ratio < 0.05, ratio


def test_int8_engine_graph_vs_eager(gpu, tmp_path, nat):
    from agent_tpu_amd.utils.synthetic import write_csv

    cfg = config_for("bert-tiny", num_labels=5)
    pack = init_random(cfg, seed=0)
    path = write_csv(str(tmp_path / "rows.csv"), 300, words_per_row=60, seed=9)
    table = nat.CsvTable(path)
    col = table.column_index("text")
    eng_g = ClassifyEngine(cfg, pack, gpu, batch_rows=64, seq_len=128, topk=3, use_graph=True, quant="int8")
    eng_e = ClassifyEngine(cfg, pack, gpu, batch_rows=64, seq_len=128, topk=3, use_graph=False, quant="int8")
    assert eng_g.model.quant == "int8" and eng_g.model._quantized is not None
    ig, sg, st = eng_g.classify_table(table, 10, 250, col)
    ie, se, _ = eng_e.classify_table(table, 10, 250, col)
    assert st.rows == 250 and st.batches == 4
    assert torch.equal(ig.cpu(), ie.cpu())
    torch.testing.assert_close(sg.cpu(), se.cpu())
