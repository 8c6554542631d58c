"""The exact decode-attention constructions (tests/kernels/_exact_attn.py) on the CPU path, and their mutants.

No GPU. This file is the proof that the assertions of tests/kernels/test_decode_exact_gpu.py can fail:
every case of every kernel route gives its expected output exactly on the CPU path of
`ops.decode_attention` and on the by-definition fp64 evaluator, and for each route every deliberate
addressing mistake (`MUTANTS`) that applies to it is rejected by at least one of the route's cases.
The same mutants against the random-data tests of tests/kernels/test_decode_gpu.py and their 2e-2
criterion are measured (printed, not asserted): docs/PERF_NOTES.md keeps the table.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kernels"))
import _exact_attn as X  # noqa: E402

from agent_tpu_amd.ops.decode import _decode_attention_ref  # noqa: E402

BF, F64 = X.BF, X.F64


def test_patterns_share_at_most_one_dim():
    p = X.patterns()
    ov = p @ p.t()
    assert torch.equal(ov.diag(), torch.full((72,), 8.0, dtype=F64))
    assert (ov - 8 * torch.eye(72, dtype=F64)).max() <= 1
    # rows up to 24 apart (three items of 8 beams) and the two heads h, h ^ 1 never share a pattern
    ids = {X.pattern_id(r, h) for r in range(36) for h in range(2)}
    assert len(ids) == 72


def test_address_rows_are_exact_and_unique():
    geo = X.Geo(32, 16, 1088, lens=[1088] * 32)
    v = X._address_cache(geo)[:, :, 1]
    assert torch.equal(v.double().to(BF), v) and v.max() <= 255
    flat = v.reshape(-1, X.D)[:, :4].double()
    key = ((flat[:, 0] * 256 + flat[:, 1]) * 8 + flat[:, 2]) * 16 + flat[:, 3]
    assert key.unique().numel() == key.numel()
    assert X.decode_address(v[3, 300, 5]) == "row/item 3 pos 300 head 5 dims in order"
    hist = X.beam_hist(130, 200)
    assert hist.min() >= 0 and hist.max() < 130
    own = hist == torch.arange(130).view(-1, 1)
    assert not own[:128].any()  # complete beam groups never point at themselves
    # the backpointer depends on the position: neighbours differ in two steps of three (also across 63 | 64 and
    # 127 | 128), positions 64 apart always, and position 0 from most others
    for R, T in ((4, 64), (4, 192), (130, 200), (4, 300)):
        h = X.beam_hist(R, T)[:4 * (R // 4)]
        assert (h[:, 1:] != h[:, :-1]).float().mean() > 0.6, (R, T)
        assert (h[:, 1:] != h[:, :-1]).float().mean(0).min() >= 0.5, (R, T)  # at every j, in at least half the rows
        assert (h[:, 1:] != h[:, :1]).float().mean() > 0.6
        if T > 64:
            assert (h[:, 63] != h[:, 64]).sum() >= len(h) // 2 and (h[:, 64:] != h[:, :-64]).all(), (R, T)
        if T > 128:
            assert (h[:, 127] != h[:, 128]).sum() >= len(h) // 2


@pytest.mark.parametrize("route", X.ROUTES)
def test_route_cases_exact_on_cpu_and_mutants_rejected(route):
    cases = X.route_cases(route)
    one_hots = [c for c in cases if c.kind == "equal" and c.name.startswith(("one_hot", "ties", "combine", "bias_hot"))]
    assert one_hots and min(c.margin for c in one_hots) >= X.MARGIN  # asserted per case by the builders, in fp64
    placed = {}
    for c in cases:
        assert X.check(c, c.run("cpu")) == "", c.name  # the CPU path of ops.decode_attention
        assert X.check(c, X.evaluate(c).to(BF)) == "", c.name  # by definition, fp64
        for kind, n in c.decoys.items():
            placed[kind] = placed.get(kind, 0) + n
        if c.q_wide is not None:
            a = c.args()
            assert a["q"].stride(0) == 3 * c.geo.H * X.D and not a["q"].is_contiguous()
    # what the hot keys cover: the current position and an earlier one, the first and the last chunk of a tie,
    # d* = 0 and d* = len - 1
    hots = [(c, rh, js) for c in cases for rh, js in c.hot.items()]
    assert any(js == [c.geo.n(rh[0]) - 1] for c, rh, js in hots if c.geo.n(rh[0]) > 1)
    assert any(js[0] < c.geo.n(rh[0]) - 1 for c, rh, js in hots)
    # every tie of a row longer than one chunk has its keys in the first and in the last chunk that holds keys; the
    # one exception: the item's other beams have filled that last chunk (65 keys: it holds one), then the chunk before
    long_ties = [(c, rh, js) for c, rh, js in hots if c.name.startswith("ties") and c.geo.n(rh[0]) > X.CHUNK]
    assert long_ties
    for c, (r, h), js in long_ties:
        g, n = c.geo, c.geo.n(r)
        last = (n - 1) // X.CHUNK
        assert len(js) == 2 and js[0] < X.CHUNK, (c.name, r, h, js)
        if js[1] // X.CHUNK != last:
            k_last = c.kv.view(g.NP, g.S, 2, g.H, X.D)[r // g.group, last * X.CHUNK:n, 0, h]
            assert g.cross and js[1] // X.CHUNK == last - 1 and (k_last != 0).any(-1).all(), (c.name, r, h, js)
    for c in cases:
        if c.name.startswith("bias_hot"):
            ns = {c.geo.n(r) for r in range(c.geo.R)}
            assert c.dstar[0] == max(ns) - 1 and c.dstar[1] == 0 and len(set(c.dstar)) >= 2 - (max(ns) == 1), c.name
    assert placed["past_len"] and placed["neighbour_item_or_row"] and placed["neighbour_head"]
    assert placed["hist_current"] or not route.startswith("self")
    assert any(c.q_wide is not None for c in cases) and any(c.q_wide is None for c in cases)
    unseen = {}
    for m in X.ROUTE_MUTANTS[route]:
        tried = 0
        for c in cases:
            if (m.startswith("bias") and c.bias is None or m.startswith("hist") and c.hist is None
                    or m == "hist_mod64" and c.geo.step < X.CHUNK
                    or m == "item_is_row" and c.geo.group == 1):  # the mistake changes nothing in such a case
                continue
            tried += 1
            if X.check(c, X.evaluate(c, mutant=m).to(BF)):
                break
        else:
            if tried:
                unseen[m] = tried
        assert tried or (m == "item_is_row" and route == "cross_chunked32"), (route, m)  # one beam per item there
    assert not unseen, f"{route}: mutants no case rejects (cases tried): {unseen}"


def test_check_messages_decode_the_address():
    c = X.route_cases("cross_split32")[0]
    msg = X.check(c, X.evaluate(c, mutant="v_heads_swapped").to(BF))
    assert "head" in msg and "want [row/item" in msg and "got [" in msg
    c = [c for c in X.route_cases("cross_split16") if c.kind == "count"][0]
    assert "count" in X.check(c, X.evaluate(c, mutant="last_twice").to(BF))


def test_count_rule_sees_one_key_more_or_less():
    """One key more, less or twice changes round(out * len) (or the exact quotient at a power of two) at every
    length of the route tables: the rule's error bound 0.07 is far from the 0.5 a wrong count moves it by."""
    for n in (1, 2, 8, 9, 31, 33, 63, 64, 65, 100, 129, 200, 255, 257, 300, 1025, 1087):
        geo = X.Geo(2, 2, min(n + 2, 2048), step=n - 1)
        c = X.counts(geo)
        assert X.check(c, X.evaluate(c).to(BF)) == "", n
        for m in ("len_plus", "len_minus", "last_twice")[:3 if n > 1 else 2]:  # one key twice is still that key
            assert X.check(c, X.evaluate(c, mutant=m).to(BF)) != "", (n, m)


def test_step_chain_on_cpu():
    assert X.step_chain("cpu") == []


# ------------------------------------------------------------------ the old random-data tests against the mutants
def _r(shape, scale=1.0, dtype=BF, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _random_inputs():
    """The inputs of three tests of tests/kernels/test_decode_gpu.py at their committed shapes and seeds."""
    for rows, group, S, H in [(8, 4, 37, 12), (3, 1, 130, 4), (16, 4, 512, 12)]:
        nseq = rows // group
        kv = _r((nseq * S, 2 * H * 64), seed=2)
        lens = torch.tensor([S - 5 * i for i in range(nseq)], dtype=torch.int32).clamp(min=1)
        yield "test_decode_attention_cross", dict(q=_r((rows, H * 64), seed=1), k=kv[:, :H * 64], v=kv[:, H * 64:], H=H,
                                                  seq_stride=S, group=group, lens=lens, step=None, bias_dist=None,
                                                  scale=1.0, hist=None)
    for rows, H, T, t, scale in [(9, 16, 300, 257, 0.125), (64, 12, 130, 64, 1.0), (5, 12, 131, 0, 1.0),
                                 (3, 2, 2048, 2047, 0.125)]:
        d = H * 64
        cache = _r((rows * T, 2 * d), seed=31)
        q = _r((rows, 3 * d), seed=32)[:, :d]
        hist = torch.randint(0, rows, (rows, T), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
        for bias in (None, _r((H, T), 1.0, torch.float32, seed=33)):
            yield "test_decode_self_rows_all_heads", dict(q=q, k=cache[:, :d], v=cache[:, d:], H=H, seq_stride=T, group=1,
                                                          lens=None, step=torch.tensor([t], dtype=torch.int32),
                                                          bias_dist=bias, scale=scale, hist=hist)
    for lens, group, S, H, scale in [([1, 63, 64, 65, 128, 1024], 4, 1024, 12, 1.0), ([1000], 4, 1024, 12, 0.125),
                                     ([130, 7], 1, 130, 16, 1.0), ([700, 3, 640], 8, 704, 12, 1.0),
                                     ([200, 199], 3, 256, 12, 1.0)]:
        nseq = len(lens)
        rows = nseq * group - (1 if group > 2 else 0)
        q = _r((rows, 3 * H * 64), seed=41)[:, :H * 64]
        kv = _r((nseq * S, 2 * H * 64), seed=42)
        for bias in (None, _r((H, S), 1.0, torch.float32, seed=43)):
            yield "test_decode_cross_split_keys", dict(q=q, k=kv[:, :H * 64], v=kv[:, H * 64:], H=H, seq_stride=S,
                                                       group=group, lens=torch.tensor(lens, dtype=torch.int32), step=None,
                                                       bias_dist=bias, scale=scale, hist=None)


def test_random_data_tests_against_the_mutants():
    """Measured, not asserted: with the CPU reference as the truth and a mutant of the evaluator as the kernel,
    in how many parameter cases of each random-data test does the mutant stay under max|a-b| / max|b| < 2e-2?
    Only the unmutated evaluator is asserted to pass."""
    table = {}
    for test, a in _random_inputs():
        ref = _decode_attention_ref(a["q"], a["k"], a["v"], a["H"], a["seq_stride"], a["group"], a["lens"], a["step"],
                                    a["bias_dist"], a["scale"], None, a["hist"])
        plain = X.evaluate_args(**a).to(BF)
        assert _rel(plain, ref) < 2e-2
        muts = X.SELF_MUTANTS if a["lens"] is None else X.CHUNK_MUTANTS
        for m in muts:
            if m.startswith("bias") and a["bias_dist"] is None:
                continue
            out = X.evaluate_args(mutant=m, **a).to(BF)
            rel = _rel(out, ref)
            t = table.setdefault((test, m), [0, 0, 0, []])
            t[0] += rel < 2e-2
            t[1] += torch.equal(out, plain)  # the mistake changes nothing here (one key, one beam, a full cache)
            t[2] += 1
            t[3].append(rel)
    print("\ntest, mutant: cases passing 2e-2 (of which the mutant changes no bit) / cases; smallest error that fails")
    for (test, m), (ok, same, n, rels) in sorted(table.items()):
        fails = [r for r in rels if r >= 2e-2]
        print(f"  {test:34s} {m:18s} {ok} ({same}) / {n}   {min(fails):.3g}")
