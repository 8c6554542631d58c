"""The exact-arithmetic LayerNorm constructions (tests/kernels/_exact_ln.py) and the CPU twins.

No GPU. This file is the proof that the assertions of tests/kernels/test_ln_exact_gpu.py can fail:
the constructions have the properties the GPU tests rely on, the CPU twins of the kernels pass the
very assertions the GPU tests make, and every mutant (another row's statistics, another column's
colsum, rstd 0.2 % high) fails them.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kernels"))
import _exact_ln as E  # noqa: E402

from agent_tpu_amd import ops  # noqa: E402

BF, F64 = E.BF, E.F64


# ------------------------------------------------------------------ the constructions
@pytest.mark.parametrize("K", [256, 768, 1024])
def test_identity_rows_have_exact_statistics(K):
    M = 2304
    x, a, s, sign = E.identity_rows(M, K, seed=1)
    assert E.bf16_exact(x) and x.abs().max() <= 12
    assert torch.equal(x.mean(-1), a) and torch.equal(((x - a[:, None]) ** 2).mean(-1), s * s)
    assert torch.equal(sign.sum(-1), torch.zeros(M, dtype=F64))
    fin = E.exact_fin(a, s)
    assert torch.equal(fin.to(F64), torch.stack([1 / s, a / s], -1))  # dyadic: exact in fp32
    for d in (1, 16, 256):  # a mutant that reads a row 1 / 16 / 256 away sees other statistics
        assert ((fin[d:] != fin[:-d]).any(-1)).all(), d
    # the fp32 sums a kernel forms are exact too: sum = K a, sumsq = K (a^2 + s^2) below 2^24
    assert (x * x).sum(-1).max() < 2 ** 24


@pytest.mark.parametrize("K", [256, 768])
def test_columns_and_weights(K):
    gamma, beta = E.col_gamma_beta(K)
    assert set(gamma.abs().tolist()) == {0.5, 1.0, 2.0} and (gamma < 0).any() and (gamma > 0).any()
    assert torch.equal(beta * 4, (beta * 4).round()) and beta.abs().max() <= 1
    for d in (1, 64):
        assert (gamma[d:] != gamma[:-d]).float().mean() > 0.6, d
    w = E.sparse_weights(768, K, seed=3)
    assert torch.equal((w != 0).sum(1), torch.full((768,), 16)) and set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
    nz = (w != 0).nonzero()[:, 1].view(768, 16)
    assert torch.equal(nz // (K // 16), torch.arange(16).expand(768, 16))  # spread over all of K
    # the production fold of these operands is exact
    b = E.int_bias(768, seed=4)
    wf, colsum, bf = ops.fold_ln_into_linear(w.to(BF), b.float(), gamma.float(), beta.float())
    assert torch.equal(wf.to(F64), w * gamma) and torch.equal(colsum.to(F64), (w * gamma).sum(1))
    assert torch.equal(bf.to(F64), b + w @ beta)
    # odd-eighth beta never cancels +-gamma and stays representable
    b8 = E.col_beta_odd8(K)
    for sg in (-1, 1):
        v = sg * gamma + b8
        assert (v != 0).all() and E.bf16_exact(v)


@pytest.mark.parametrize("K,N", [(256, 256), (768, 768), (768, 256)])
def test_sparse_references_are_representable(K, N):
    c = E.in_norm_case(2048, K, N, True)
    assert torch.equal(c.ref * 4, (c.ref * 4).round()) and c.ref.abs().max() < 64 and E.bf16_exact(c.ref)
    assert c.bound.max() < 2.0 ** -11
    assert 0 < (c.ref == 0).float().mean() < 0.05  # the zero-entry half of the rule is exercised
    d = E.decode_case(17, K if K == 256 else 1024, 768)
    for ref, bound in ((d.ref_y, d.bound_y), (d.ref_z, d.bound_z)):
        assert ref.abs().max() < 64 and E.bf16_exact(ref) and bound.max() < 2.0 ** -11


@pytest.mark.parametrize("res_norm", [False, True])
def test_stats_out_partials_are_exact(res_norm):
    c = E.res_stats_case(2048, 768, 768, res_norm)
    assert E.partials_exact(c.ref, 256) and E.bf16_exact(c.ref)
    assert torch.equal(c.part.float().to(F64), c.part)
    p = E.producer_case(2048, 768, 768, 256)
    assert E.bf16_exact(p.res0) and p.res0.abs().max() <= 32 and E.partials_exact(p.T, 256)


# ------------------------------------------------------------------ the CPU twins pass the GPU tests' assertions
def _in_norm_twin(c, fin=None, colsum=None):
    return ops.linear_ln(c.x, c.wf, c.bf, in_fin=c.fin if fin is None else fin,
                         colsum=c.colsum if colsum is None else colsum)


@pytest.mark.parametrize("M,K,N,sparse", [(2048, 512, 256, False), (2304, 768, 768, False), (2048, 256, 768, True),
                                          (2304, 768, 768, True)])
def test_linear_ln_twin_in_norm_bit_equal_and_mutants_fail(M, K, N, sparse):
    c = E.in_norm_case(M, K, N, sparse)
    assert torch.equal(_in_norm_twin(c), c.ref_bf)
    if sparse:
        assert E.zero_rule_ok(_in_norm_twin(c), c.ref, c.bound)
    rows_off = lambda t: (t != c.ref_bf).any(-1).float().mean().item()  # noqa: E731
    for d in (1, 16, 256):  # statistics of row m + d
        y = _in_norm_twin(c, fin=c.fin.roll(-d, 0))
        assert not torch.equal(y, c.ref_bf) and rows_off(y) > 0.9, d
        assert not sparse or not E.zero_rule_ok(y, c.ref, c.bound)
    for d in (1, 64, 256):  # colsum of column n + d
        if d % N == 0:
            continue
        y = _in_norm_twin(c, colsum=c.colsum.roll(-d, 0))
        assert not torch.equal(y, c.ref_bf) and rows_off(y) > 0.9, d
        assert not sparse or not E.zero_rule_ok(y, c.ref, c.bound)
    hi = c.fin.clone()
    hi[:, 0] *= 1.002  # rstd 0.2 % high
    y = _in_norm_twin(c, fin=hi)
    assert not torch.equal(y, c.ref_bf) and rows_off(y) > 0.9
    assert not sparse or not E.zero_rule_ok(y, c.ref, c.bound)


@pytest.mark.parametrize("K,N", [(256, 768), (768, 768)])
def test_zero_rule_holds_with_statistics_an_ulp_off(K, N):
    """Every statistic moved by one fp32 ulp, up or down at random: still bit-equal where ref != 0, the
    residue where ref == 0 inside the bound (what a HIP finalize or a hardware rsqrt may do)."""
    c = E.in_norm_case(2048, K, N, True)
    g = torch.Generator().manual_seed(5)
    step = torch.randint(0, 2, c.fin.shape, generator=g, dtype=torch.int32) * 2 - 1
    fin = (c.fin.view(torch.int32) + step * (c.fin != 0)).view(torch.float32)
    y = _in_norm_twin(c, fin=fin)
    assert E.zero_rule_ok(y, c.ref, c.bound)
    z = y.to(F64)[c.ref == 0].abs()
    print(f"zero-entry residue max {z.max().item():.3g}, bound max {c.bound.max().item():.3g}")


@pytest.mark.parametrize("M,K,N", [(2048, 256, 256), (2304, 768, 768)])
@pytest.mark.parametrize("res_norm", [False, True])
def test_linear_ln_twin_res_norm_stats_out(M, K, N, res_norm):
    c = E.res_stats_case(M, K, N, res_norm)
    part = torch.full((N // 256, M, 2), float("nan"))
    kw = dict(res_fin=c.fin, res_gamma=c.gamma) if res_norm else {}
    y = ops.linear_ln(c.ctx, c.w, c.bias, residual=c.r, part_out=part, **kw)
    assert torch.equal(y, c.ref_bf) and torch.equal(part.to(F64), c.part)
    if res_norm:
        for d in (1, 16, 256):
            y = ops.linear_ln(c.ctx, c.w, c.bias, residual=c.r, part_out=part, res_fin=c.fin.roll(-d, 0),
                              res_gamma=c.gamma)
            assert not torch.equal(y, c.ref_bf) and not torch.equal(part.to(F64), c.part)
        for d in (1, 64):
            y = ops.linear_ln(c.ctx, c.w, c.bias, residual=c.r, part_out=part, res_fin=c.fin,
                              res_gamma=c.gamma.roll(-d, 0))
            assert not torch.equal(y, c.ref_bf)


@pytest.mark.parametrize("slots", [1, 3, 12, 16])
def test_ln_finalize_twin_exact_on_identity_rows(slots):
    K = 256 * slots
    x, a, s, _ = E.identity_rows(2304, K, seed=slots)
    part = E.partials(x, 256)
    assert torch.equal(part.float().to(F64), part)
    fin = ops.ln_finalize(part.float().contiguous(), K, 1e-12)
    assert E.ulps(fin, E.exact_fin(a, s)).max().item() == 0


@pytest.mark.parametrize("slots", [1, 3, 12, 16])
def test_ln_finalize_fp32_formula_within_bound(slots):
    """The fp32 formula itself (the CPU twin) stays inside the bound the GPU test applies to the kernel."""
    part = E.adversarial_partials(2304, slots)
    fin = ops.ln_finalize(part, 256 * slots, 1e-12)
    assert torch.isfinite(fin).all()
    ratio = E.finalize_worst_ratio(fin, part, 256 * slots, 1e-12)
    print(f"slots {slots}: worst finalize error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("N", E.WIDTHS)
def test_norm_twins_bit_equal(N):
    for rows in E.ROWS:
        c = E.norm_case(rows, N)
        assert (c.ref != 0).all() and E.bf16_exact(c.ref) and E.bf16_exact((c.x.to(F64) - c.r.to(F64)))
        assert torch.equal(ops.layernorm(c.x, c.gamma, c.beta, 1e-12).to(F64), c.ref)
        assert torch.equal(ops.layernorm(c.xmr, c.gamma, c.beta, 1e-12, residual=c.r).to(F64), c.ref)
        xr = (c.s[:, None] * c.sign).to(BF)  # rows +-s_m: RMSNorm gives +-gamma
        for eps in (0.0, 1e-6):
            assert torch.equal(ops.rmsnorm(xr, c.gamma, eps).to(F64), c.sign * c.gamma.to(F64)), eps
        # a mutant: gamma of the next column
        assert not torch.equal(ops.layernorm(c.x, c.gamma.roll(-1), c.beta, 1e-12).to(F64), c.ref)


def test_layernorm_sweep_on_the_twin():
    """The sweep the GPU tests run in-process and in the ATPU_LN_KERNEL child processes."""
    assert E.layernorm_sweep("cpu") == []


@pytest.mark.parametrize("M,K", [(4, 256), (17, 1024), (129, 256)])
def test_linear_twin_decode_fold(M, K):
    """`ops.linear` on CPU tensors with stats_out / row_ln / res_ln (and the <= 4-row self statistics)."""
    N, eps = 768, E.EPS_ABSORBED
    d = E.decode_case(M, K, N)
    p = d.p
    part = torch.full((K // 32, M, 2), float("nan"))
    x = ops.linear(p.ctx0, p.w0, p.b0, residual=p.res0_bf, stats_out=part)
    assert torch.equal(x, p.T_bf) and torch.equal(part.to(F64), p.part)
    y = ops.linear(x, d.wf, d.bf, row_ln=(eps, d.cs, part))
    assert torch.equal(y.to(F64), d.ref_y) and E.zero_rule_ok(y, d.ref_y, d.bound_y)
    z = ops.linear(d.ctx, d.wo, d.bo_beta, residual=x, res_ln=(eps, part, d.gamma))
    assert torch.equal(z.to(F64), d.ref_z) and E.zero_rule_ok(z, d.ref_z, d.bound_z)
    if M <= 4:
        tot = torch.full_like(part, float("nan"))
        y = ops.linear(x, d.wf, d.bf, row_ln=(eps, d.cs, None), row_ln_out=tot)
        assert torch.equal(y.to(F64), d.ref_y) and torch.equal(tot, ops.row_totals_parts_ref(p.T_bf))
    # mutants: the partials of the next row, the colsum of the next column
    if M > 1:
        bad = part.roll(-1, 1).contiguous()
        assert not E.zero_rule_ok(ops.linear(x, d.wf, d.bf, row_ln=(eps, d.cs, bad)), d.ref_y, d.bound_y)
        assert not E.zero_rule_ok(ops.linear(d.ctx, d.wo, d.bo_beta, residual=x, res_ln=(eps, bad, d.gamma)),
                                  d.ref_z, d.bound_z)
    assert not E.zero_rule_ok(ops.linear(x, d.wf, d.bf, row_ln=(eps, d.cs.roll(-1).contiguous(), part)), d.ref_y,
                              d.bound_y)


# ------------------------------------------------------------------ the random cases' tolerance
def test_fp32_two_pass_layernorm_within_tolerance():
    """An fp32 two-pass LayerNorm (mean, centred variance, (v - mean) * rstd * gamma + beta, bf16 store)
    of rows with a mean of up to 8 sigma stays inside the per-element tolerance of the GPU random cases.
    Worst ratio observed: 0.995 (fp32 two-pass), 0.995 (`ops.layernorm` on CPU), 0.996 (RMSNorm): bf16's half
    ulp at the bottom of a binade is 2^-8 |ref| itself, the fp32 terms add under 0.001."""
    worst = {}
    for N in (256, 768, 2048):
        v, gamma, beta = E.random_rows(1003, N, seed=N)
        ref, tol = E.ln_ref_tol(v, gamma, beta, 1e-12)
        x = v.float()
        mean = x.mean(-1, keepdim=True)
        d = x - mean
        rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + 1e-12)
        y = (d * rstd * gamma + beta).to(BF)
        worst["two-pass"] = max(worst.get("two-pass", 0), E.worst_ratio(y, ref, tol))
        worst["twin"] = max(worst.get("twin", 0), E.worst_ratio(ops.layernorm(v, gamma, beta, 1e-12), ref, tol))
        ref, tol = E.ln_ref_tol(v, gamma, beta, 1e-6, rms=True)
        worst["rms"] = max(worst.get("rms", 0), E.worst_ratio(ops.rmsnorm(v, gamma, 1e-6), ref, tol))
    print("worst |y - ref| / tol:", {k: round(r, 3) for k, r in worst.items()})
    assert max(worst.values()) <= 1.0
    # the tolerance is tight enough to see gamma or the mean 1 % off
    v, gamma, beta = E.random_rows(64, 768, seed=1)
    ref, tol = E.ln_ref_tol(v, gamma, beta, 1e-12)
    assert E.worst_ratio(ops.layernorm(v, gamma * 1.01, beta, 1e-12), ref, tol) > 1.0
