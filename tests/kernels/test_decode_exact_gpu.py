"""Decode attention, every kernel route, on inputs whose correct output is known bit for bit
(constructions and case lists: `_exact_attn.py`).

Every V row carries its address (cache row or item, position, head, dim order); the scores make exactly
one key (or two tying keys) of each (row, head) win with e^-200 or less for every other key it may read,
and keys it must not read (past the length, the backpointer of the current position, the neighbouring
item, row and head) hold decoys that would win. So one key too many or too few, a backpointer from the
wrong row, another item's K/V, a bias indexed the wrong way round or a chunk left out of the combine
changes the bits, and the failure message names the address that was read.
tests/contract/test_decode_exact_cpu.py shows each of these mistakes failing the same case lists.

Each test first asserts that its cases reach the kernel it names, by the dispatcher's own rules
(`decode_attention` in csrc/kernels/decode.hip): the split workspace size, the CU count, the switches.
"""
import os
import subprocess
import sys

import pytest
import torch

import _exact_attn as X

pytestmark = pytest.mark.gpu


def _self_kernel_default():
    return not os.environ.get("ATPU_DEC_SELF", "1").startswith("0")


def _ws(nat, c, cross=True):
    g = c.geo
    return nat.decode_attention_ws_floats(g.R, g.group, g.H, g.S, cross)


def _run(cases, gpu):
    bad = X.run_cases(cases, gpu)
    assert not bad, f"{len(bad)} of {len(cases)} cases wrong:\n" + "\n".join(bad[:8])


def test_self_few_kernel(gpu, nat):
    """decode_self_few_kernel<1 | 2 | 3>: T = 64, 128, 130, 192, with and without hist and bias."""
    cases = X.route_cases("self_few")
    prev_few, prev_inv = nat.decode_self_few(-1), nat.batch_invariant(-1)
    try:
        nat.decode_self_few(1)
        nat.batch_invariant(0)
        assert _self_kernel_default()
        if 4 * 4 > nat.num_cus():
            pytest.skip(f"the few-row kernel takes rows * heads <= CUs: 16 > {nat.num_cus()}")
        for c in cases:
            g = c.geo
            assert g.S <= 192 and g.R * g.H <= nat.num_cus() and not g.cross, c.name
        assert {c.geo.S for c in cases} == {64, 128, 130, 192}
        assert any(c.q_wide is not None for c in cases)
        _run(cases, gpu)
    finally:
        nat.decode_self_few(prev_few)
        nat.batch_invariant(prev_inv)


@pytest.mark.parametrize("T", [70, 200])
def test_self_row_kernel_head_groups(gpu, nat, T):
    """decode_self_attention_kernel with the heads over grid.y (rows < 128): 5 heads, 2 head groups of 4 waves.
    T = 70 with the few-row kernel switched off, T = 200 above its cache length."""
    cases = X.route_cases(f"self_rows_head_groups_t{T}")
    prev_few, prev_inv = nat.decode_self_few(-1), nat.batch_invariant(-1)
    try:
        nat.batch_invariant(0)
        if T <= 192:
            nat.decode_self_few(0)
        assert _self_kernel_default() and (T > 192 or nat.decode_self_few(-1) == 0)
        for c in cases:
            assert c.geo.S == T and c.geo.R < 128 and c.geo.H == 5 and not c.geo.cross, c.name
        assert any(c.q_wide is not None for c in cases)
        _run(cases, gpu)
    finally:
        nat.decode_self_few(prev_few)
        nat.batch_invariant(prev_inv)


def test_self_row_kernel_one_workgroup(gpu, nat):
    """rows >= 128: one workgroup per row for all 5 heads, wave 0 owns two of them."""
    cases = X.route_cases("self_rows_one_workgroup")
    prev_inv = nat.batch_invariant(-1)
    try:
        nat.batch_invariant(0)
        assert _self_kernel_default()
        for c in cases:
            assert c.geo.R >= 128 and c.geo.S > 192 and c.geo.H % 4 != 0, c.name
        assert any(c.q_wide is not None for c in cases)
        _run(cases, gpu)
    finally:
        nat.batch_invariant(prev_inv)


def test_cross_short_source(gpu, nat):
    """decode_attention_kernel<1 | 4 | 8>: S = 100 is below two 64-key chunks, so nothing is split; groups 3 and 5
    run the 4- and 8-beam instantiations partly filled, the last item is a row short."""
    cases = X.route_cases("cross_short")
    for c in cases:
        assert c.geo.S < 2 * X.CHUNK and _ws(nat, c) == 0, c.name
    assert {c.geo.group for c in cases} == {1, 3, 4, 5, 8}
    assert any(c.geo.R % c.geo.group for c in cases) and any(c.q_wide is not None for c in cases)
    _run(cases, gpu)


def test_cross_large_grid(gpu, nat):
    """decode_attention_kernel<4, 4> at a grid too large to split (items * heads >= 512), 300 keys."""
    cases = X.route_cases("cross_large_grid")
    prev_inv = nat.batch_invariant(-1)
    try:
        nat.batch_invariant(0)
        for c in cases:
            assert c.geo.nseq * c.geo.H >= 512 and _ws(nat, c) == 0 and nat.batch_invariant(-1) == 0, c.name
        assert any(c.q_wide is not None for c in cases)
        _run(cases, gpu)
    finally:
        nat.batch_invariant(prev_inv)


def test_cross_split_combine16(gpu, nat):
    """decode_cross_split_kernel<1 | 4 | 8, bias?> and decode_attn_combine_kernel over 4 chunk records (S = 200)."""
    cases = X.route_cases("cross_split16")
    for c in cases:
        g = c.geo
        assert _ws(nat, c) == g.R * g.H * 4 * 66, c.name
    assert {c.geo.group for c in cases} == {1, 3, 4, 8}
    assert any(c.bias is not None for c in cases) and any(c.bias is None for c in cases)
    assert any(c.q_wide is not None for c in cases)
    _run(cases, gpu)


def test_cross_split_combine32(gpu, nat):
    """S = 1088: 17 chunk records per row, the 32-slot combine."""
    cases = X.route_cases("cross_split32")
    for c in cases:
        g = c.geo
        assert _ws(nat, c) == g.R * g.H * 17 * 66, c.name
    assert any(c.q_wide is not None for c in cases)
    _run(cases, gpu)


def test_cross_chunked16(gpu, nat):
    """Batch invariance at a grid too large to split: decode_cross_chunked_kernel<4, 4, 16, bias?> on the cases of
    the large-grid test (5 chunk records per row in LDS)."""
    cases = X.route_cases("cross_chunked16")
    prev_inv = nat.batch_invariant(-1)
    try:
        nat.batch_invariant(1)
        for c in cases:
            g = c.geo
            assert nat.batch_invariant(-1) == 1 and _ws(nat, c) == 0 and g.nseq * g.H >= 512, c.name
            assert 2 * X.CHUNK <= g.S <= 16 * X.CHUNK and g.group <= 8, c.name
        _run(cases, gpu)
    finally:
        nat.batch_invariant(prev_inv)


def test_cross_chunked32(gpu, nat):
    """decode_cross_chunked_kernel<1, 4, 32, bias?>: 32 items x 16 heads, S = 1088 (17 chunks over 4 waves)."""
    cases = X.route_cases("cross_chunked32")
    prev_inv = nat.batch_invariant(-1)
    try:
        nat.batch_invariant(1)
        for c in cases:
            g = c.geo
            assert nat.batch_invariant(-1) == 1 and _ws(nat, c) == 0 and g.nseq * g.H >= 512, c.name
            assert g.S > 16 * X.CHUNK, c.name
        assert any(c.q_wide is not None for c in cases)
        _run(cases, gpu)
    finally:
        nat.batch_invariant(prev_inv)


def test_step_chain_reads_the_ancestors_cache_row(gpu):
    """5 decode steps, 6 rows, 2 heads, T = 20: kv_append, beam_reorder_hist with a non-identity parent, then a
    one-hot query aimed at the key written 2 steps earlier: the V row of the ancestor beam at that step."""
    bad = X.step_chain(gpu)
    assert not bad, "\n".join(bad)


def test_fallback_kernel_in_a_child_process(gpu):
    """ATPU_DEC_SELF=0 (read once per process): decode_attention_kernel<1, 4> with hist and prow, the self
    attention cases at T = 70 and T = 300 in one fresh interpreter."""
    torch.cuda.synchronize()  # this process has no GPU work in flight while the child runs
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path.insert(0, {here!r}); import torch, _exact_attn as X; "
            "bad = X.fallback_sweep(torch.device('cuda', 0)); print('\\n'.join(bad[:8])); sys.exit(1 if bad else 0)")
    env = dict(os.environ, ATPU_DEC_SELF="0")
    try:
        r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(here)), env=env,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("the ATPU_DEC_SELF=0 child did not finish in 120 s")
    assert r.returncode >= 0, f"the child died on signal {-r.returncode}: {r.stderr[-2000:]}"
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
