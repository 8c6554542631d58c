"""Exact-arithmetic inputs and fp64 references for the LayerNorm-folding and norm-kernel tests.

A plain helper module (no tests, no conftest): `tests/contract/test_ln_exact_cpu.py` proves the
constructions and runs them through the CPU twins, `tests/kernels/test_ln_exact_gpu.py` runs the
HIP kernels on the same cases.

Rows with an identity. Row m of width K holds a_m + s_m * sign[m, k] with a_m = (7m mod 17) - 8,
s_m = 2^((5m + m//256) mod 3) and exactly K/2 entries of sign -1: small integers (exact in bf16),
mean exactly a_m, variance exactly s_m^2, so (rstd, rstd*mu) = (1/s_m, a_m/s_m) are dyadic, and
rows 1, 16 and 256 apart never share their statistics.

Columns with an identity. gamma_k = +-2^((3k + k//64) mod 3 - 1), beta_k = ((5k mod 9) - 4) / 4;
weights in {-1, 0, 1}, biases integers in [-4, 4]. With exact statistics every intermediate value
of a folded epilogue is a short dyadic number: fp32 FMAs are exact in any order and the kernel's
output must be bf16_rne(fp64 reference), bit for bit.

Statistics that may be an fp32 ulp off (a HIP finalize, the hardware rsqrt): weights with 16
nonzeros of +-1 per output column. Every reference value is then a multiple of 1/4 below 64 in
magnitude, representable in bf16, so a few fp32 ulps cannot cross a rounding boundary: the output is
bit-equal wherever the reference is not 0, and where it is 0 the output is bounded by
4 * 2^-24 * (sum of the magnitudes of the reference's own terms) -- `zero_rule_ok`.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from agent_tpu_amd import ops

BF, F64 = torch.bfloat16, torch.float64
# `ops.linear` refuses eps = 0 for row_ln / res_ln; 2^-60 is absorbed by var >= 1 in fp32 (var + eps == var)
EPS_ABSORBED = 2.0 ** -60
WIDTHS = tuple(256 * g for g in (1, 2, 3, 4, 6, 8))
ROWS = (1, 7, 8, 9, 1003)


@pytest.fixture
def few_cus():
    """Persistent GEMM grids held to 8 workgroups: each walks several tiles, statistics staged a tile ahead."""
    from agent_tpu_amd._native import native

    nat = native()
    nat.cu_budget(8)
    try:
        yield
    finally:
        nat.cu_budget(0)


# ------------------------------------------------------------------ constructions (fp64, CPU)
def row_stats(M):
    m = torch.arange(M, dtype=torch.int64)
    a = (7 * m % 17 - 8).to(F64)
    s = 2.0 ** ((5 * m + m // 256) % 3).to(F64)
    return a, s


def balanced_signs(M, K, seed):
    """+-1 [M, K] with exactly K/2 entries of -1 per row, at random positions."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand((M, K), generator=g).argsort(dim=1)
    return torch.where(perm < K // 2, -1.0, 1.0).to(F64)


def identity_rows(M, K, seed=0, zero_mean=False):
    """(x, a, s, sign): x[m] = a_m + s_m * sign[m] (a_m = 0 with `zero_mean`)."""
    a, s = row_stats(M)
    if zero_mean:
        a = torch.zeros_like(a)
    sign = balanced_signs(M, K, seed)
    return a[:, None] + s[:, None] * sign, a, s, sign


def exact_fin(a, s):
    """The exact (rstd, rstd*mu) of identity rows, fp32 [M, 2]."""
    return torch.stack([1.0 / s, a / s], -1).float().contiguous()


def col_gamma_beta(K):
    k = torch.arange(K, dtype=torch.int64)
    mag = 2.0 ** (((3 * k + k // 64) % 3) - 1).to(F64)
    gamma = torch.where((11 * k % 7) < 3, -mag, mag)
    beta = ((5 * k % 9) - 4).to(F64) / 4
    return gamma, beta


def col_beta_odd8(K):
    """beta for the materialised norms: odd multiples of 1/8, so +-gamma + beta is never 0."""
    k = torch.arange(K, dtype=torch.int64)
    return (2 * ((5 * k % 9) - 4) + 1).to(F64) / 8


def dense_weights(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (N, K), generator=g).to(F64)


def sparse_weights(N, K, seed, nnz=16):
    """[N, K] with `nnz` entries of +-1 per output column, one in each K/nnz-wide span of K."""
    g = torch.Generator().manual_seed(seed)
    span = K // nnz
    pos = torch.arange(nnz).view(1, nnz) * span + torch.randint(0, span, (N, nnz), generator=g)
    val = (torch.randint(0, 2, (N, nnz), generator=g) * 2 - 1).to(F64)
    return torch.zeros((N, K), dtype=F64).scatter_(1, pos, val)


def int_bias(N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (N,), generator=g).to(F64)


def int_rows(M, K, lim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, (M, K), generator=g).to(F64)


def partials(y, slab):
    """[N/slab, M, 2] per-row (sum, sum of squares) over each `slab`-column slab, in y's dtype."""
    M, N = y.shape
    t = y.view(M, N // slab, slab).transpose(0, 1)
    return torch.stack([t.sum(-1), (t * t).sum(-1)], -1).contiguous()


def partials_exact(y, slab):
    """Every fp32 summation order gives the same partials: all values are multiples of 1/4 and each
    slab's sum of magnitudes (in units of 1/4) and of squares (in units of 1/16) stays below 2^24."""
    M, N = y.shape
    t = y.view(M, N // slab, slab)
    return bool(((y * 4) == (y * 4).round()).all() and (t.abs().sum(-1) * 4).max() < 2 ** 24
                and ((t * t).sum(-1) * 16).max() < 2 ** 24)


def bf16_exact(t):
    return bool((t.to(BF).to(F64) == t).all())


def zero_rule_ok(y, ref, bound):
    """Bit-equal where ref != 0, |y| <= bound where ref == 0. Valid only for references that bf16
    holds exactly and bounds far below a bf16 rounding step of 1/4-multiples (2^-11)."""
    assert bound.max().item() < 2.0 ** -11 and bf16_exact(ref)
    y = y.detach().cpu().to(F64)
    nz = ref != 0
    return bool(torch.equal(y[nz], ref[nz]) and (y[~nz].abs() <= bound[~nz]).all())


def ulps(x, exact):
    """Distance in fp32 ulps (integer steps) between fp32 tensors of the same sign."""
    return (x.detach().cpu().contiguous().view(torch.int32).long() - exact.contiguous().view(torch.int32).long()).abs()


# ------------------------------------------------------------------ GEMM cases (cached: built once, never modified)
@functools.lru_cache(maxsize=None)
def in_norm_case(M, K, N, sparse):
    """InNorm consumer: LN(x) @ w.T + b on identity rows x; folded operands from `ops.fold_ln_into_linear`."""
    x, a, s, sign = identity_rows(M, K, seed=M + K)
    gamma, beta = col_gamma_beta(K)
    w = sparse_weights(N, K, seed=N + K + 1) if sparse else dense_weights(N, K, seed=N + K + 2)
    b = int_bias(N, seed=N + 3)
    wf, colsum, bf = ops.fold_ln_into_linear(w.to(BF), b.float(), gamma.float(), beta.float())
    ref = ((x - a[:, None]) / s[:, None] * gamma + beta) @ w.t() + b
    acc = x @ wf.to(F64).t()
    bound = 4 * 2.0 ** -24 * ((acc / s[:, None]).abs() + ((a / s)[:, None] * colsum.to(F64)).abs() + bf.to(F64).abs())
    return SimpleNamespace(x=x.to(BF), a=a, s=s, fin=exact_fin(a, s), gamma=gamma, beta=beta, w=w, b=b, wf=wf,
                           colsum=colsum, bf=bf, ref=ref, ref_bf=ref.to(BF), bound=bound)


@functools.lru_cache(maxsize=None)
def res_stats_case(M, K, N, res_norm):
    """ResNorm + StatsOut (or plain residual + StatsOut) producer: ctx @ w.T + bias + LN(r) (or + r),
    r the identity rows; |y| < 64 in multiples of 1/4, so C and the fp32 partials are exact."""
    ctx = int_rows(M, K, 2, seed=M + K + 5)
    w = sparse_weights(N, K, seed=N + K + 6)
    b = int_bias(N, seed=N + 7)
    r, a, s, sign = identity_rows(M, N, seed=M + N)
    gamma, beta = col_gamma_beta(N)
    if res_norm:
        bias = b + beta
        ref = ctx @ w.t() + bias + (r - a[:, None]) / s[:, None] * gamma
    else:
        bias = b
        ref = ctx @ w.t() + bias + r
    return SimpleNamespace(ctx=ctx.to(BF), w=w.to(BF), bias=bias.float().contiguous(), r=r.to(BF), a=a, s=s,
                           fin=exact_fin(a, s), gamma=gamma.float().contiguous(), ref=ref, ref_bf=ref.to(BF),
                           part=partials(ref, 256))


@functools.lru_cache(maxsize=None)
def producer_case(M, W, K0, slab):
    """A producer GEMM whose output IS the identity rows T [M, W]: ctx0 @ w0.T + b0 is an integer
    matrix P and the residual res0 = T - P still holds small integers (|res0| <= 32)."""
    T, a, s, sign = identity_rows(M, W, seed=M + W)
    ctx0 = int_rows(M, K0, 1, seed=M + K0 + 8)
    w0 = sparse_weights(W, K0, seed=W + K0 + 9)
    b0 = int_bias(W, seed=W + 10)
    res0 = T - (ctx0 @ w0.t() + b0)
    return SimpleNamespace(T=T, T_bf=T.to(BF), a=a, s=s, sign=sign, ctx0=ctx0.to(BF), w0=w0.to(BF),
                           b0=b0.float().contiguous(), res0=res0, res0_bf=res0.to(BF), part=partials(T, slab))


@functools.lru_cache(maxsize=None)
def decode_case(M, K, N):
    """Decode fold on rows of width K: the RowStats producer of `producer_case(M, K, 256, 32)`, a RowLn
    consumer (sparse [N, K] weights) and a ResLn consumer (ctx [M, 256] @ wo.T + LN(x) as the residual)."""
    p = producer_case(M, K, 256, 32)
    gamma, beta = col_gamma_beta(K)
    w = sparse_weights(N, K, seed=N + K + 11)
    b = int_bias(N, seed=N + 12)
    wf, cs, bf = ops.fold_ln_into_linear(w.to(BF), b.float(), gamma.float(), beta.float())
    ln = p.sign * gamma + beta
    ref_y = ln @ w.t() + b
    rs, rmu = (1.0 / p.s)[:, None], (p.a / p.s)[:, None]
    bound_y = 4 * 2.0 ** -24 * ((p.T @ wf.to(F64).t() * rs).abs() + (rmu * cs.to(F64)).abs() + bf.to(F64).abs())
    ctx = int_rows(M, 256, 2, seed=M + 13)
    wo = sparse_weights(K, 256, seed=K + 14)
    bo = int_bias(K, seed=K + 15)
    acc = ctx @ wo.t()
    ref_z = acc + bo + beta + p.sign * gamma
    bound_z = 4 * 2.0 ** -24 * (acc.abs() + (bo + beta).abs() + ((p.T * rs).abs() + rmu.abs()) * gamma.abs())
    return SimpleNamespace(p=p, gamma=gamma.float().contiguous(), wf=wf, cs=cs, bf=bf, ref_y=ref_y, bound_y=bound_y,
                           ctx=ctx.to(BF), wo=wo.to(BF), bo_beta=(bo + beta).float().contiguous(), ref_z=ref_z,
                           bound_z=bound_z)


# ------------------------------------------------------------------ materialised norms
@functools.lru_cache(maxsize=None)
def norm_case(rows, N):
    """LayerNorm of identity rows: the output is sign * gamma + beta (odd-eighth beta: never 0, always
    representable), also as x - r plus a residual r of small integers."""
    x, a, s, sign = identity_rows(rows, N, seed=rows + N)
    gamma, _ = col_gamma_beta(N)
    beta = col_beta_odd8(N)
    r = int_rows(rows, N, 3, seed=rows + N + 1)
    return SimpleNamespace(x=x.to(BF), xmr=(x - r).to(BF), r=r.to(BF), gamma=gamma.float().contiguous(),
                           beta=beta.float().contiguous(), ref=sign * gamma + beta, sign=sign, s=s)


def layernorm_sweep(dev):
    """`ops.layernorm` with and without residual at every width and row count; the cases not bit-equal."""
    bad = []
    for N in WIDTHS:
        for rows in ROWS:
            c = norm_case(rows, N)
            g, b = c.gamma.to(dev), c.beta.to(dev)
            y0 = ops.layernorm(c.x.to(dev), g, b, 1e-12)
            y1 = ops.layernorm(c.xmr.to(dev), g, b, 1e-12, residual=c.r.to(dev))
            for tag, y in (("plain", y0), ("residual", y1)):
                if not torch.equal(y.cpu().to(F64), c.ref):
                    bad.append((N, rows, tag))
    return bad


# ------------------------------------------------------------------ adversarial partials for the finalize kernel
@functools.lru_cache(maxsize=None)
def adversarial_partials(M, slots, seed=0):
    """fp32 StatsOut partials [slots, M, 2] of rows with mean / sigma in {0, 1, 8, 64} (row m: the
    (m mod 4)-th), sigma in 2^-3 .. 2^3, and every 37th row constant (variance 0: the clamp)."""
    K = 256 * slots
    g = torch.Generator().manual_seed(seed + M + slots)
    ratio = torch.tensor([0.0, 1.0, 8.0, 64.0])[torch.arange(M) % 4].view(M, 1)
    sigma = 2.0 ** torch.randint(-3, 4, (M, 1), generator=g).float()
    x = (sigma * ratio + sigma * torch.randn((M, K), generator=g)).float()
    x[::37] = 3.3 * sigma[::37]
    return partials(x.to(F64), 256).float().contiguous()


def finalize_ref_bound(part, K, eps):
    """fp64 finalize of the fp32 partials: (rstd, rstd*mu, bound on the relative rstd error
    2^-22 (1 + (E[x^2] + mu^2) / (var + eps)))."""
    p = part.to(F64).sum(0)
    mu, e2 = p[:, 0] / K, p[:, 1] / K
    var = (e2 - mu * mu).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return rstd, rstd * mu, 2.0 ** -22 * (1 + (e2 + mu * mu) / (var + eps))


def finalize_worst_ratio(fin, part, K, eps):
    """Worst ratio of fin's error to its bound: rstd relative to `bound`; rstd*mu to bound * |rstd*mu| plus
    the fp32 summation of the slots' sums ((slots + 2) roundings of at most 2^-24 sum |s_k| / K, times rstd)."""
    rstd, rmu, bound = finalize_ref_bound(part, K, eps)
    f = fin.detach().cpu().to(F64)
    r0 = ((f[:, 0] - rstd).abs() / rstd / bound).max().item()
    slots = part.shape[0]
    b1 = bound * rmu.abs() + (slots + 2) * 2.0 ** -24 * rstd * part.to(F64)[:, :, 0].abs().sum(0) / K
    r1 = ((f[:, 1] - rmu).abs() / b1.clamp_min(1e-300)).max().item()
    return max(r0, r1)


# ------------------------------------------------------------------ realistic random rows, per-element tolerance
def random_rows(rows, N, seed):
    """bf16 rows with sigma in [0.25, 4] and a mean of up to 8 sigma; fp32 gamma ~ 1 +- 0.2, beta ~ 0.1."""
    g = torch.Generator().manual_seed(seed)
    sigma = 0.25 * 16.0 ** torch.rand((rows, 1), generator=g)
    mean = sigma * (16 * torch.rand((rows, 1), generator=g) - 8)
    mean[0] = 8 * sigma[0]
    v = (mean + sigma * torch.randn((rows, N), generator=g)).to(BF)
    gamma = (1 + 0.2 * torch.randn(N, generator=g)).float()
    beta = (0.1 * torch.randn(N, generator=g)).float()
    return v, gamma, beta


def ln_ref_tol(v, gamma, beta, eps, rms=False):
    """fp64 LayerNorm (RMSNorm) of the fp64 rows v, and the per-element tolerance
    2^-8 |ref| + 2^-20 ((|v| + |mean|) rstd |gamma| + |beta|): bf16's half ulp plus 16 fp32 ulps of the
    terms that cancel."""
    v, gamma, beta = v.to(F64), gamma.to(F64), beta.to(F64) * (0.0 if rms else 1.0)
    mean = torch.zeros_like(v[:, :1]) if rms else v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + eps)
    ref = (v - mean) * rstd * gamma + beta
    tol = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * ((v.abs() + mean.abs()) * rstd * gamma.abs() + beta.abs())
    return ref, tol


def worst_ratio(y, ref, tol):
    return ((y.detach().cpu().to(F64) - ref).abs() / tol).max().item()
