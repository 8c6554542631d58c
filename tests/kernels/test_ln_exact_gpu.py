"""LayerNorm folding and the norm kernels against exact fp64 references (constructions: `_exact_ln.py`).

Rows and columns carry an identity (every row its own dyadic mean and sigma, every column its own
power-of-two gamma), all values are short dyadic numbers, so the kernels' fp32 arithmetic is exact and
the outputs must equal the fp64 reference bit for bit: another row's statistics, another column's
colsum or gamma, or an rstd 0.2 % off changes the bits (tests/contract/test_ln_exact_cpu.py shows each
of these mutants failing the same assertions on the CPU twins). Where statistics come from a HIP
kernel (and may be an fp32 ulp off), the weights are sparse and the rule is: bit-equal where the
reference is not 0, inside 4 * 2^-24 * (the reference's own terms) where it is.
"""
import os
import subprocess
import sys

import pytest
import torch

import _exact_ln as E
from _exact_ln import few_cus  # noqa: F401  (fixture)
from agent_tpu_amd import ops
from agent_tpu_amd._native import native
from agent_tpu_amd.ops.linear import EPI_BIAS, EPI_RES_LN, EPI_RESIDUAL, EPI_ROW_LN, EPI_ROW_STATS
from agent_tpu_amd.ops.linear_i8 import quantize_rows_i8_ref

pytestmark = pytest.mark.gpu

BF, F64 = E.BF, E.F64
GEMM_SHAPES = [(M, K, N) for M in (2048, 2304) for K in (256, 768) for N in (256, 768)]
NAN = float("nan")


# ------------------------------------------------------------------ the finalize kernel
@pytest.mark.parametrize("slots", [1, 3, 12, 16])
def test_finalize_exact_rows(gpu, slots):
    """Identity rows of width 256 * slots: the kernel's (rstd, rstd*mu) against the exact (1/s, a/s).
    Expected 0 ulps at a power-of-two width (every operation exact, rsqrt of 1, 4, 16 exact) and at most 2
    at 768 / 3072, where 1/K is rounded."""
    K = 256 * slots
    x, a, s, _ = E.identity_rows(2304, K, seed=slots)
    part_all = E.partials(x, 256).float()
    exact = E.exact_fin(a, s)
    worst = 0
    for M in (1, 255, 257, 2304):
        part = part_all[:, :M].contiguous().to(gpu)
        fin = torch.full((M + 1, 2), NAN, device=gpu)
        ops.ln_finalize(part, K, 1e-12, out=fin[:M])
        assert torch.isnan(fin[M]).all()  # nothing written past row M
        worst = max(worst, E.ulps(fin[:M], exact[:M]).max().item())
    print(f"finalize K={K}: {worst} ulps from the exact statistics")
    assert worst <= (0 if K & (K - 1) == 0 else 2)


@pytest.mark.parametrize("slots", [1, 3, 12, 16])
def test_finalize_adversarial_partials(gpu, slots):
    """fp32 partials of rows with mean / sigma in {0, 1, 8, 64} (and constant rows: the clamp keeps them
    finite) against an fp64 finalize of the same partials; relative rstd error within
    2^-22 (1 + (E[x^2] + mu^2) / (var + eps)) (the fp32 formula's own worst ratio on the CPU twin: 0.61)."""
    K = 256 * slots
    for M in (1, 255, 257, 2304):
        part = E.adversarial_partials(2304, slots)[:, :M].contiguous()
        fin = ops.ln_finalize(part.to(gpu), K, 1e-12)
        assert torch.isfinite(fin).all()
        ratio = E.finalize_worst_ratio(fin, part, K, 1e-12)
        print(f"finalize adversarial slots={slots} M={M}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0


def test_hardware_rsqrt_at_powers_of_four(gpu):
    """One-slot partials with sum 0 and sumsq 256 * {1, 4, 16}: rstd must be exactly 1, 1/2, 1/4."""
    part = torch.tensor([[[0.0, 256.0], [0.0, 1024.0], [0.0, 4096.0]]], device=gpu)
    fin = ops.ln_finalize(part, 256, 0.0).cpu()
    print("rsqrt(1, 4, 16) =", [repr(v) for v in fin[:, 0].tolist()])
    assert fin[:, 0].tolist() == [1.0, 0.5, 0.25] and fin[:, 1].tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ the folded 256x256 epilogues
@pytest.mark.parametrize("M,K,N", GEMM_SHAPES)
def test_in_norm_exact(gpu, few_cus, M, K, N):
    """InNorm with host-exact statistics and dense weights: bf16_rne of the fp64 reference, three times."""
    c = E.in_norm_case(M, K, N, False)
    x, wf, bf, fin, cs = (t.to(gpu) for t in (c.x, c.wf, c.bf, c.fin, c.colsum))
    ref = c.ref_bf.to(gpu)
    for _ in range(3):
        y = torch.full((M, N), NAN, dtype=BF, device=gpu)
        ops.linear_ln(x, wf, bf, in_fin=fin, colsum=cs, out=y)
        assert torch.equal(y, ref)


@pytest.mark.parametrize("M,K,N", [(2048, 256, 768), (2304, 768, 768)])
def test_in_norm_statistics_an_ulp_off(gpu, few_cus, M, K, N):
    """Sparse weights, every statistic moved one fp32 ulp up or down: the zero-entry rule on the kernel's
    own arithmetic (the accumulators start at -mu * colsum with mu = rstd*mu / rstd, no longer dyadic)."""
    c = E.in_norm_case(M, K, N, True)
    g = torch.Generator().manual_seed(5)
    step = torch.randint(0, 2, c.fin.shape, generator=g, dtype=torch.int32) * 2 - 1
    fin = (c.fin.view(torch.int32) + step * (c.fin != 0)).view(torch.float32)
    y = ops.linear_ln(c.x.to(gpu), c.wf.to(gpu), c.bf.to(gpu), in_fin=fin.to(gpu), colsum=c.colsum.to(gpu))
    z = (y.cpu().to(F64)[c.ref == 0].abs() / c.bound[c.ref == 0].clamp_min(2.0 ** -60)).max().item()
    print(f"ulp-off statistics M={M} K={K}: worst zero-entry residue / bound {z:.3f}")
    assert E.zero_rule_ok(y, c.ref, c.bound)


@pytest.mark.parametrize("res_norm", [True, False])
@pytest.mark.parametrize("M,K,N", GEMM_SHAPES)
def test_res_norm_stats_out_exact(gpu, few_cus, M, K, N, res_norm):
    """ResNorm + StatsOut and residual + StatsOut: C and the fp32 partials, both exact."""
    c = E.res_stats_case(M, K, N, res_norm)
    assert E.partials_exact(c.ref, 256) and torch.equal(c.part.float().to(F64), c.part)
    part = torch.full((N // 256, M, 2), NAN, device=gpu)
    kw = dict(res_fin=c.fin.to(gpu), res_gamma=c.gamma.to(gpu)) if res_norm else {}
    y = ops.linear_ln(c.ctx.to(gpu), c.w.to(gpu), c.bias.to(gpu), residual=c.r.to(gpu), part_out=part, **kw)
    assert torch.equal(y, c.ref_bf.to(gpu))
    assert torch.equal(part.cpu().to(F64), c.part)


@pytest.mark.parametrize("M,H,N", [(2048, 768, 768), (2304, 768, 256), (2304, 256, 768)])
def test_stats_finalize_in_norm_chain(gpu, few_cus, M, H, N):
    """One layer's production sequence: StatsOut GEMM (its output is the identity rows) -> HIP finalize ->
    InNorm GEMM with sparse weights, under the zero-entry rule."""
    p = E.producer_case(M, H, H, 256)
    c = E.in_norm_case(M, H, N, True)
    assert torch.equal(p.T_bf, c.x)
    part = torch.full((H // 256, M, 2), NAN, device=gpu)
    x = ops.linear_ln(p.ctx0.to(gpu), p.w0.to(gpu), p.b0.to(gpu), residual=p.res0_bf.to(gpu), part_out=part)
    assert torch.equal(x.cpu(), p.T_bf) and torch.equal(part.cpu().to(F64), p.part)
    fin = ops.ln_finalize(part, H, 1e-12)
    print(f"chain H={H}: finalize {E.ulps(fin, c.fin).max().item()} ulps from exact")
    y = ops.linear_ln(x, c.wf.to(gpu), c.bf.to(gpu), in_fin=fin, colsum=c.colsum.to(gpu))
    assert E.zero_rule_ok(y, c.ref, c.bound)


# ------------------------------------------------------------------ the decode fold, family by family
def _decode_family(nat, family, M, N, K):
    """Assert that the default dispatch sends the fold's GEMMs of this M to `family` (read from
    gemm_bf16 in gemm_bf16.hip: <= 4 rows the GEMV, 5..16 the few-row kernel, then the 64x64 dec kernel
    while the 128x128 grid is small; `gemm_dec_mode(0)` selects the 128x128 kernel instead of dec)."""
    epis = (EPI_BIAS | EPI_RESIDUAL | EPI_ROW_STATS, EPI_BIAS | EPI_ROW_LN, EPI_BIAS | EPI_RESIDUAL | EPI_RES_LN)
    widths = (K, N, K)
    for epi, n in zip(epis, widths):
        assert nat.gemv_selected(M, n, epi) == (family == "gemv"), (family, M, n, epi)
    assert not nat.batch_invariant(-1)
    assert {"gemv": M <= 4, "few": 5 <= M <= 16, "dec": M > 16, "tile128": M > 16}[family]
    assert nat.gemm_dec_mode(-1) == (0 if family == "tile128" else 1)


@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("family,M", [("gemv", 1), ("gemv", 4), ("few", 5), ("dec", 17), ("tile128", 17),
                                      ("dec", 129), ("tile128", 129)])
def test_decode_fold_exact(gpu, family, M, K):
    """RowStats producer -> RowLn consumer and ResLn consumer at the smallest M of each kernel family
    (and 129: a second, partial row block). eps = 2^-60 (`ops.linear` wants eps > 0; absorbed by var >= 1)."""
    nat = native()
    N, eps = 768, E.EPS_ABSORBED
    d = E.decode_case(M, K, N)
    p = d.p
    prev = nat.gemm_dec_mode(-1)
    if family == "tile128":
        nat.gemm_dec_mode(0)
    try:
        _decode_family(nat, family, M, N, K)
        part = torch.full((K // 32, M, 2), NAN, device=gpu)
        x = ops.linear(p.ctx0.to(gpu), p.w0.to(gpu), p.b0.to(gpu), residual=p.res0_bf.to(gpu), stats_out=part)
        assert torch.equal(x.cpu(), p.T_bf) and torch.equal(part.cpu().to(F64), p.part)
        y = ops.linear(x, d.wf.to(gpu), d.bf.to(gpu), row_ln=(eps, d.cs.to(gpu), part))
        assert E.zero_rule_ok(y, d.ref_y, d.bound_y)
        # the decode QKV form: columns >= 256 land in row m * T + step of the KV cache
        T, t, col0 = 3, 2, 256
        cache = torch.full((M * T, N - col0), NAN, dtype=BF, device=gpu)
        q = ops.linear(x, d.wf.to(gpu), d.bf.to(gpu), row_ln=(eps, d.cs.to(gpu), part),
                       kv_cache=(cache, T, torch.tensor([t], dtype=torch.int32, device=gpu), col0))
        assert E.zero_rule_ok(q, d.ref_y[:, :col0], d.bound_y[:, :col0])
        cache = cache.view(M, T, N - col0)
        assert E.zero_rule_ok(cache[:, t], d.ref_y[:, col0:], d.bound_y[:, col0:]) and torch.isnan(cache[:, :t]).all()
        z = ops.linear(d.ctx.to(gpu), d.wo.to(gpu), d.bo_beta.to(gpu), residual=x,
                       res_ln=(eps, part, d.gamma.to(gpu)))
        assert E.zero_rule_ok(z, d.ref_z, d.bound_z)
    finally:
        nat.gemm_dec_mode(prev)


@pytest.mark.parametrize("M,K", [(1, 256), (4, 256), (3, 1024), (4, 1024)])
def test_gemv_self_statistics_exact(gpu, M, K):
    """<= 4 rows: `row_ln=(eps, cs, None)` takes the statistics from the rows it reads, `row_ln_out` hands
    them on (totals in slot 0, exact) to the ResLn GEMV."""
    nat = native()
    N, eps = 768, E.EPS_ABSORBED
    d = E.decode_case(M, K, N)
    assert nat.gemv_selected(M, N, EPI_BIAS | EPI_ROW_LN) and nat.gemv_selected(M, K, EPI_BIAS | EPI_RESIDUAL | EPI_RES_LN)
    x = d.p.T_bf.to(gpu)
    tot = torch.full((K // 32, M, 2), NAN, device=gpu)
    y = ops.linear(x, d.wf.to(gpu), d.bf.to(gpu), row_ln=(eps, d.cs.to(gpu), None), row_ln_out=tot)
    assert E.zero_rule_ok(y, d.ref_y, d.bound_y)
    assert torch.equal(tot.cpu(), ops.row_totals_parts_ref(d.p.T_bf))
    z = ops.linear(d.ctx.to(gpu), d.wo.to(gpu), d.bo_beta.to(gpu), residual=x, res_ln=(eps, tot, d.gamma.to(gpu)))
    assert E.zero_rule_ok(z, d.ref_z, d.bound_z)


# ------------------------------------------------------------------ the materialised norm kernels
def test_layernorm_exact(gpu):
    assert E.layernorm_sweep(gpu) == []


@pytest.mark.parametrize("mode", ["wave", "hw"])
def test_layernorm_exact_other_kernels(gpu, mode):
    """ATPU_LN_KERNEL=wave (wave per row) and =hw (half wave, plain loads): the same sweep in a fresh
    process (the mode is read once per process)."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path.insert(0, {here!r}); import torch, _exact_ln as E; "
            "print(E.layernorm_sweep(torch.device('cuda', 0)))")
    env = dict(os.environ, ATPU_LN_KERNEL=mode)
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(here)), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "[]", r.stdout[-2000:]


@pytest.mark.parametrize("N", E.WIDTHS)
def test_rmsnorm_exact(gpu, N):
    """Rows +-s_m: RMSNorm is exactly +-gamma, with eps 0 and with eps 1e-6."""
    for rows in E.ROWS:
        c = E.norm_case(rows, N)
        x = (c.s[:, None] * c.sign).to(BF).to(gpu)
        for eps in (0.0, 1e-6):
            y = ops.rmsnorm(x, c.gamma.to(gpu), eps)
            assert torch.equal(y.cpu().to(F64), c.sign * c.gamma.to(F64)), (rows, eps)


@pytest.mark.parametrize("N", E.WIDTHS)
def test_layernorm_quant_i8_exact(gpu, N):
    for rows in E.ROWS:
        c = E.norm_case(rows, N)
        g, b = c.gamma.to(gpu), c.beta.to(gpu)
        for x, res in ((c.x, None), (c.xmr, c.r)):
            y, q, sc = ops.layernorm_quant_i8(x.to(gpu), g, b, 1e-12, residual=None if res is None else res.to(gpu))
            assert torch.equal(y.cpu().to(F64), c.ref), rows
            q_ref, sc_ref = quantize_rows_i8_ref(y.cpu())
            assert torch.equal(q.cpu(), q_ref) and torch.equal(sc.cpu(), sc_ref), rows


def _embed_tables(V, P, TV, N, seed):
    """Word rows +-s_v (zero mean), position and type rows constant: they carry the mean only (sigma varies
    with the word row; `_split_tables` makes the position and type rows visible)."""
    w, _, s, sign = E.identity_rows(V, N, seed=seed, zero_mean=True)
    pos = (torch.arange(P, dtype=F64) % 9 - 4).view(P, 1).expand(P, N)
    typ = (torch.arange(TV, dtype=F64) * 3 - 2).view(TV, 1).expand(TV, N)
    return w.to(BF), pos.to(BF).contiguous(), typ.to(BF).contiguous(), sign


def _split_tables(V, P, TV, N, seed):
    """Every table carries a part of the row's sign pattern on columns of its own (word k % 4 < 2, position
    k % 4 == 2, type k % 4 == 3; without a type table word the even and position the odd columns), each part
    balanced on its support, sigma 2 throughout; position and type rows add a constant each. The output is
    (sw[id] + sp[pos] + st[type]) * gamma + beta: a wrong row of ANY table changes bits."""
    col = torch.arange(N)
    gw, gp, gt = (col % 4 < 2, col % 4 == 2, col % 4 == 3) if TV else (col % 2 == 0, col % 2 == 1, col < 0)
    sw, sp, st = (torch.zeros((n, N), dtype=F64) for n in (V, P, max(TV, 1)))
    sw[:, gw] = E.balanced_signs(V, int(gw.sum()), seed)
    sp[:, gp] = E.balanced_signs(P, int(gp.sum()), seed + 1)
    if TV:
        st[:, gt] = E.balanced_signs(TV, int(gt.sum()), seed + 2)
    pos = (torch.arange(P, dtype=F64) % 9 - 4).view(P, 1) + 2 * sp
    typ = (torch.arange(max(TV, 1), dtype=F64) * 3 - 2).view(-1, 1) + 2 * st
    return (2 * sw).to(BF), pos.to(BF), typ.to(BF), sw, sp, st


@pytest.mark.parametrize("N", E.WIDTHS)
def test_embed_layernorm_exact(gpu, N):
    """Ids below 0 and at or above the vocabulary (clamped), type ids given (also out of range) and None,
    token counts that are no multiple of 4."""
    V, TV = 61, 2
    gamma, beta = E.col_gamma_beta(N)[0].float(), E.col_beta_odd8(N).float()
    for B, S in ((1, 1), (1, 7), (2, 4), (3, 3), (17, 59)):
        word, pos, typ, sign = _embed_tables(V, S, TV, N, seed=N + S)
        g = torch.Generator().manual_seed(B * S)
        ids = torch.randint(-5, V + 5, (B, S), generator=g, dtype=torch.int32)
        ids.view(-1)[0], ids.view(-1)[-1] = -1, V
        tt = torch.randint(-1, TV + 1, (B, S), generator=g, dtype=torch.int32)
        ref = sign[ids.long().clamp(0, V - 1).view(-1)] * gamma.to(F64) + beta.to(F64)
        for type_ids in (tt, None):
            y = ops.embed_layernorm(ids.to(gpu), word.to(gpu), pos.to(gpu), typ.to(gpu), gamma.to(gpu),
                                    beta.to(gpu), 1e-12, type_ids=None if type_ids is None else type_ids.to(gpu))
            assert torch.equal(y.cpu().to(F64), ref), (B, S, type_ids is None)
        # every table visible in the output: position t % S, the clamped type id (0 without type ids)
        word, pos, typ, sw, sp, st = _split_tables(V, S, TV, N, seed=N + S)
        tok = torch.arange(B * S)
        for type_ids in (tt, None):
            tc = tt.long().clamp(0, TV - 1).view(-1) if type_ids is not None else torch.zeros(B * S, dtype=torch.long)
            ref = (sw[ids.long().clamp(0, V - 1).view(-1)] + sp[tok % S] + st[tc]) * gamma.to(F64) + beta.to(F64)
            y = ops.embed_layernorm(ids.to(gpu), word.to(gpu), pos.to(gpu), typ.to(gpu), gamma.to(gpu),
                                    beta.to(gpu), 1e-12, type_ids=None if type_ids is None else type_ids.to(gpu))
            assert torch.equal(y.cpu().to(F64), ref), (B, S, type_ids is None, "split")


@pytest.mark.parametrize("N", E.WIDTHS)
def test_embed_gather_exact(gpu, N):
    V = 61
    table = torch.randn((V, N), generator=torch.Generator().manual_seed(N)).to(BF)
    for rows in E.ROWS:
        g = torch.Generator().manual_seed(rows)
        ids = torch.randint(-5, V + 5, (rows,), generator=g, dtype=torch.int32)
        ids[0], ids[-1] = (V, -1) if rows > 1 else (V, V)
        out = torch.full((rows + 1, N), NAN, dtype=BF, device=gpu)
        ops.embed_gather(ids.to(gpu), table.to(gpu), out=out[:rows])
        assert torch.equal(out[:rows].cpu(), table[ids.long().clamp(0, V - 1)]) and torch.isnan(out[rows]).all()


@pytest.mark.parametrize("N", E.WIDTHS)
def test_embed_pos_layernorm_exact(gpu, N):
    """The device-side step, clamped at both ends of the position table."""
    V, P = 61, 11
    gamma, beta = E.col_gamma_beta(N)[0].float(), E.col_beta_odd8(N).float()
    table, pos, _, sign = _embed_tables(V, P, 1, N, seed=N + 1)
    for rows in E.ROWS:
        g = torch.Generator().manual_seed(rows)
        ids = torch.randint(-5, V + 5, (rows,), generator=g, dtype=torch.int32)
        ref = sign[ids.long().clamp(0, V - 1)] * gamma.to(F64) + beta.to(F64)
        for step, off in ((0, 2), (3, -7), (9, 5)):
            y = ops.embed_pos_layernorm(ids.to(gpu), table.to(gpu), pos.to(gpu),
                                        torch.tensor([step], dtype=torch.int32, device=gpu), off, gamma.to(gpu),
                                        beta.to(gpu), 1e-5)
            assert torch.equal(y.cpu().to(F64), ref), (rows, step, off)
    # the position row visible in the output: row clamp(step + off, 0, P - 1)
    table, pos, _, sw, sp, _ = _split_tables(V, P, 0, N, seed=N + 2)
    ids = torch.randint(-5, V + 5, (9,), generator=torch.Generator().manual_seed(N), dtype=torch.int32)
    for step, off in ((0, 2), (3, -7), (9, 5), (10, 0)):
        ref = (sw[ids.long().clamp(0, V - 1)] + sp[min(max(step + off, 0), P - 1)]) * gamma.to(F64) + beta.to(F64)
        y = ops.embed_pos_layernorm(ids.to(gpu), table.to(gpu), pos.to(gpu),
                                    torch.tensor([step], dtype=torch.int32, device=gpu), off, gamma.to(gpu),
                                    beta.to(gpu), 1e-5)
        assert torch.equal(y.cpu().to(F64), ref), (step, off, "split")


# ------------------------------------------------------------------ one realistic random case per norm kernel
@pytest.mark.parametrize("N", [768, 1536])
def test_norm_kernels_random_rows(gpu, N):
    """Rows with a mean of up to 8 sigma, judged per element against fp64:
    |y - ref| <= 2^-8 |ref| + 2^-20 ((|v| + |mean|) rstd |gamma| + |beta|), bf16's half ulp plus 16 fp32 ulps
    of the terms that cancel. An fp32 two-pass evaluation reaches 0.995 of it (the half ulp at the bottom
    of a binade; tests/contract/test_ln_exact_cpu.py). Here the position and type rows of the embedding
    kernels are random too, so a wrong position or type row shows."""
    rows, worst = 1003, {}
    v, gamma, beta = E.random_rows(rows, N, seed=N)
    r = (0.5 * torch.randn((rows, N), generator=torch.Generator().manual_seed(N + 1))).to(BF)
    gd, bd = gamma.to(gpu), beta.to(gpu)

    def judge(name, y, vv, eps, rms=False):
        ref, tol = E.ln_ref_tol(vv, gamma, beta, eps, rms)
        worst[name] = E.worst_ratio(y, ref, tol)

    judge("layernorm", ops.layernorm(v.to(gpu), gd, bd, 1e-12), v, 1e-12)
    judge("layernorm+res", ops.layernorm(v.to(gpu), gd, bd, 1e-12, residual=r.to(gpu)), v.to(F64) + r.to(F64), 1e-12)
    judge("rmsnorm", ops.rmsnorm(v.to(gpu), gd, 1e-6), v, 1e-6, rms=True)
    y, q, sc = ops.layernorm_quant_i8(v.to(gpu), gd, bd, 1e-12, residual=r.to(gpu))
    judge("layernorm_quant_i8", y, v.to(F64) + r.to(F64), 1e-12)
    q_ref, sc_ref = quantize_rows_i8_ref(y.cpu())
    assert torch.equal(q.cpu(), q_ref) and torch.equal(sc.cpu(), sc_ref)
    # embeddings: B x S = 17 x 59 tokens over random word / position / type rows
    B, S, V, TV = 17, 59, 200, 2
    g = torch.Generator().manual_seed(N + 2)
    word, pos, typ = v[:V], (0.5 * torch.randn((S + 3, N), generator=g)).to(BF), torch.randn((TV, N), generator=g).to(BF)
    ids = torch.randint(0, V, (B, S), generator=g, dtype=torch.int32)
    tt = torch.randint(0, TV, (B, S), generator=g, dtype=torch.int32)
    x = word.to(F64)[ids.long().view(-1)] + pos.to(F64)[:S].repeat(B, 1) + typ.to(F64)[tt.long().view(-1)]
    judge("embed_layernorm", ops.embed_layernorm(ids.to(gpu), word.to(gpu), pos.to(gpu), typ.to(gpu), gd, bd, 1e-12,
                                                 type_ids=tt.to(gpu)), x, 1e-12)
    step = torch.tensor([4], dtype=torch.int32, device=gpu)
    x = word.to(F64)[ids.long().view(-1)] + pos.to(F64)[4 + 2]
    judge("embed_pos_layernorm", ops.embed_pos_layernorm(ids.view(-1).to(gpu), word.to(gpu), pos.to(gpu), step, 2, gd,
                                                         bd, 1e-5), x, 1e-5)
    print(f"N={N} worst |y - ref| / tol:", {k: round(w, 3) for k, w in worst.items()})
    assert max(worst.values()) <= 1.0, worst
