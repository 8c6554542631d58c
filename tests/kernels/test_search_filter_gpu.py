"""Filtered sim_topk (csrc/kernels/sim_topk_masked.hip): the row mask in the kernel's epilogue and
step walk, the mask builders, and map_search with ``filter`` on the GPU engine.

The reference is the unmasked kernel itself. A (query, row) score is one fp32 accumulator fed in a
column order that depends on D alone, so "search the allowed rows R" has one right answer: the
result of ``sim_topk`` over the gathered rows ``c[R]`` with the ids mapped back through ``R``, bit
for bit. Every comparison below is ``torch.equal``; no tolerance is involved. The data is
test_search_gpu.py's integer recipe with duplicated rows, so equal scores occur and the
(score desc, id asc) tie order is checked through the mapping (R is ascending, so it keeps order).

The masks of the kernel tests are packed with PyTorch (``ops.row_mask_from_bits``), not with the
builder kernels, which have their own tests against ``numpy.packbits(..., bitorder="little")``.
"""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops

pytestmark = pytest.mark.gpu

_cache = {}
DTYPES = ["f32", "f16", "f16s"]  # fp32 corpus, fp16 corpus, fp16 corpus with row_scale


def _exact_case(D, N, nq):
    key = ("exact", D, N, nq)
    if key not in _cache:
        gen = torch.Generator().manual_seed(D + 3 * N + 5 * nq)
        col = torch.tensor([1.0, 2.0, -1.0, -2.0])[(torch.arange(D) * 7 + torch.arange(D) // 5) % 4]
        base = torch.randint(-1, 2, (max(1, (N + 2) // 3), D), generator=gen).float() * col
        c = base[torch.randint(0, base.shape[0], (N,), generator=gen)].contiguous()  # duplicated rows: ties
        q = torch.randint(-2, 3, (nq, D), generator=gen).float()
        _cache[key] = (q, c)
    return _cache[key]


def _pow2_scale(N):
    n = torch.arange(N)
    return torch.tensor([0.25, 0.5, 1.0, 2.0])[(n * 3 + n // 7 + n // 3) % 4].contiguous()


def _operands(gpu, dt, D, N, nq):
    """(q, c, row_scale or None) on the device for a dtype form."""
    q, c = _exact_case(D, N, nq)
    if dt == "f32":
        return q.to(gpu), c.to(gpu), None
    return q.to(gpu), c.half().to(gpu), (_pow2_scale(N).to(gpu) if dt == "f16s" else None)


def _pattern(name, N):
    """bool [N]: the allowed rows of a named mask pattern."""
    n = torch.arange(N)
    nwords = (N + 31) // 32
    if name == "row0":
        return n == 0
    if name == "last":
        return n == N - 1
    if name == "every_other":
        return n % 2 == 0
    if name == "one_per_word":
        return n % 32 == (n // 32 * 7) % 32
    if name == "alt_words":  # alternately empty and full words
        return (n // 32) % 2 == 1
    if name == "first_word_empty":
        return n >= 32
    if name == "last_quarter":  # only the last quarter of the words live
        return n // 32 >= nwords - max(1, nwords // 4)
    if name in ("rand50", "rand03"):
        gen = torch.Generator().manual_seed(N + len(name))
        return torch.rand(N, generator=gen) < (0.5 if name == "rand50" else 0.03)
    if name == "few":  # fewer allowed rows than k
        b = torch.zeros(N, dtype=torch.bool)
        b[torch.tensor([3, 40, 41, N // 2, N - 1])] = True
        return b
    if name == "none":
        return torch.zeros(N, dtype=torch.bool)
    raise KeyError(name)


def _gathered(q, c, rs, bits, k, id_base=0):
    """The reference: plain sim_topk over the gathered allowed rows, ids mapped back."""
    R = bits.to(c.device).nonzero().flatten()
    if R.numel() == 0:
        return (torch.empty((q.shape[0], 0), dtype=torch.float32, device=c.device),
                torch.empty((q.shape[0], 0), dtype=torch.int64, device=c.device))
    s, i = ops.sim_topk(q, c[R].contiguous(), k, row_scale=rs[R].contiguous() if rs is not None else None)
    return s, id_base + R[i]


def _check_equal(got, want, what):
    s, i = got
    ws, wi = want
    assert s.shape == ws.shape and i.shape == wi.shape, (what, s.shape, ws.shape)
    assert s.dtype == torch.float32 and i.dtype == torch.int64
    assert torch.equal(i, wi), (what, (i != wi).nonzero()[:4])
    assert torch.equal(s, ws), what


# ------------------------------------------------------------------------------------ all-ones mask
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", [1, 31, 32, 33, 4099])
def test_all_ones_mask_equals_the_unmasked_kernel(gpu, dt, N):
    q, c, rs = _operands(gpu, dt, 64, N, 17)
    ones = ops.row_mask_from_bits(torch.ones(N, dtype=torch.bool, device=gpu))
    assert ones.count == N
    for k in (8, 10):
        _check_equal(ops.sim_topk(q, c, k, row_scale=rs, mask=ones), ops.sim_topk(q, c, k, row_scale=rs), (dt, N, k))


# ------------------------------------------------------------------------ gathered-subset equality
PATTERNS = ["row0", "last", "every_other", "one_per_word", "alt_words", "first_word_empty", "last_quarter", "rand50",
            "rand03", "few", "none"]
# every nq and every k at least once over the patterns; with the dtype forms, every KM / QH / NW form
SHAPES = [(1, 1), (16, 8), (17, 10), (33, 16), (70, 17), (1, 32), (33, 32), (16, 16), (70, 8), (17, 32), (33, 10)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pattern,shape", list(zip(PATTERNS, SHAPES)))
def test_masked_search_equals_the_search_of_the_gathered_rows(gpu, dt, pattern, shape):
    N, (nq, k) = 4099, shape
    q, c, rs = _operands(gpu, dt, 64, N, nq)
    bits = _pattern(pattern, N)
    mask = ops.row_mask_from_bits(bits.to(gpu))
    splits = 4 if pattern == "last_quarter" else None
    got = ops.sim_topk(q, c, k, splits=splits, row_scale=rs, mask=mask)
    assert got[0].shape == (nq, min(k, int(bits.sum())))
    _check_equal(got, _gathered(q, c, rs, bits, k), (dt, pattern))
    if pattern == "none":
        assert got[0].shape == (nq, 0) and got[0].is_cuda


@pytest.mark.parametrize("dt", DTYPES)
def test_every_launch_form(gpu, dt):
    """nq in {1, 16, 17, 33, 70} x k in {1, 8, 10, 16, 17, 32}: KM 8 / 16 / 32, one and two query halves."""
    N = 1000
    bits = _pattern("rand50", N)
    mask = ops.row_mask_from_bits(bits.to(gpu))
    for nq in (1, 16, 17, 33, 70):
        q, c, rs = _operands(gpu, dt, 64, N, nq)
        for k in (1, 8, 10, 16, 17, 32):
            _check_equal(ops.sim_topk(q, c, k, row_scale=rs, mask=mask), _gathered(q, c, rs, bits, k), (dt, nq, k))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D,N,nq,k,pattern", [(768, 4099, 33, 10, "rand50"), (1024, 1000, 17, 17, "alt_words"),
                                              (192, 1000, 16, 8, "rand03")])
def test_wide_rows_and_an_id_base(gpu, dt, D, N, nq, k, pattern):
    """D = 768 and 1024 (several column steps per row step), 192 (fp16: the two-chunk tail step); id_base."""
    q, c, rs = _operands(gpu, dt, D, N, nq)
    bits = _pattern(pattern, N)
    mask = ops.row_mask_from_bits(bits.to(gpu))
    _check_equal(ops.sim_topk(q, c, k, 12345, row_scale=rs, mask=mask), _gathered(q, c, rs, bits, k, 12345),
                 (dt, D, pattern))


# ---------------------------------------------------------------------------------------- invariance
@pytest.mark.parametrize("dt", DTYPES)
def test_result_does_not_depend_on_splits_batch_or_run(gpu, dt):
    N, k = 4099, 10
    q, c, rs = _operands(gpu, dt, 64, N, 70)
    mask = ops.row_mask_from_bits(_pattern("rand50", N).to(gpu))
    s0, i0 = ops.sim_topk(q, c, k, row_scale=rs, mask=mask)
    for splits in (1, 2, 7, 64):
        _check_equal(ops.sim_topk(q, c, k, splits=splits, row_scale=rs, mask=mask), (s0, i0), splits)
    _check_equal(ops.sim_topk(q, c, k, row_scale=rs, mask=mask), (s0, i0), "second run")
    _check_equal(ops.sim_topk(q[:17].contiguous(), c, k, row_scale=rs, mask=mask), (s0[:17], i0[:17]), "prefix")
    for a in (0, 16, 69):
        s1, i1 = ops.sim_topk(q[a:a + 1].contiguous(), c, k, row_scale=rs, mask=mask)
        assert torch.equal(s1[0], s0[a]) and torch.equal(i1[0], i0[a]), a
    sc, ic = s0.cpu(), i0.cpu()  # the duplicated rows tie: equal scores come back in ascending id
    same = sc[:, 1:] == sc[:, :-1]
    assert same.any() and (ic[:, 1:][same] > ic[:, :-1][same]).all()


# ----------------------------------------------------------------------- nothing extra is read or used
@pytest.mark.parametrize("dt", DTYPES)
def test_masked_rows_cannot_leak(gpu, dt):
    """1e30 (inf in fp16) and NaN in the masked rows, and in their row scales: by select, never times 0."""
    N, k = 4099, 10
    q, c, rs = _operands(gpu, dt, 64, N, 33)
    for pattern in ("rand50", "alt_words"):
        bits = _pattern(pattern, N).to(gpu)
        mask = ops.row_mask_from_bits(bits)
        clean = ops.sim_topk(q, c, k, row_scale=rs, mask=mask)
        for poison in (1e30, float("nan")):
            c2 = c.clone()
            c2[~bits] = torch.tensor(poison, device=gpu).to(c2.dtype)
            rs2 = None
            if rs is not None:
                rs2 = rs.clone()
                rs2[~bits] = float("nan")
            s, i = ops.sim_topk(q, c2, k, row_scale=rs2, mask=mask)
            assert torch.isfinite(s).all()
            _check_equal((s, i), clean, (dt, pattern, poison))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", [1, 31, 33, 4099])
def test_nothing_outside_the_corpus_the_words_and_the_list_is_read(gpu, dt, N):
    """The corpus, the row scale, the words and ``live`` each as a view inside a larger poisoned buffer
    (the words' poison is all-ones: a word read past the end would allow 32 rows)."""
    D, pad, k = 64, 64, 10
    q, c, rs = _operands(gpu, dt, D, N, 17)
    bits = _pattern("every_other", N).to(gpu)
    mask = ops.row_mask_from_bits(bits)
    clean = ops.sim_topk(q, c, k, row_scale=rs, mask=mask)

    def inside(t, poison):
        shape = (t.shape[0] + 2 * pad,) + tuple(t.shape[1:])
        if t.dtype == torch.float16:  # 1e30 is inf there
            big = torch.full(shape, poison, dtype=torch.float32, device=gpu).half()
        else:
            big = torch.full(shape, poison, dtype=t.dtype, device=gpu)
        big[pad:pad + t.shape[0]] = t
        view = big[pad:pad + t.shape[0]]
        assert view.is_contiguous()
        return view

    for poison in (1e30, float("nan")):
        m2 = ops.RowMask(inside(mask.words, -1), inside(mask.live, 2 ** 31 - 1), mask.rows, mask.count)
        s, i = ops.sim_topk(q, inside(c, poison), k, row_scale=inside(rs, poison) if rs is not None else None, mask=m2)
        assert torch.isfinite(s).all()
        _check_equal((s, i), clean, (dt, N, poison))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", [1, 31, 33, 4099])
def test_tail_bits_of_the_last_word_are_ignored(gpu, dt, N):
    k = 10
    q, c, rs = _operands(gpu, dt, 64, N, 17)
    for pattern in ("every_other", "row0"):
        mask = ops.row_mask_from_bits(_pattern(pattern, N).to(gpu))
        clean = ops.sim_topk(q, c, k, row_scale=rs, mask=mask)
        words = mask.words.clone()
        words[-1] |= torch.tensor(-(1 << (N % 32)), dtype=torch.int32, device=gpu)  # the bits of rows N .. 32 w + 31
        live = torch.nonzero(words).flatten().to(torch.int32)  # the last word is live now, whatever it was
        dirty = ops.RowMask(words, live, N, mask.count)
        _check_equal(ops.sim_topk(q, c, k, row_scale=rs, mask=dirty), clean, (dt, N, pattern))


# ------------------------------------------------------------------------------------------ builders
def _np_words(bits):
    """numpy twin: bool [N] -> int32 words [ceil(N / 32)], bit b of word w = row 32 w + b, zero tail."""
    N = len(bits)
    padded = np.zeros((N + 31) // 32 * 32, dtype=bool)
    padded[:N] = bits
    return np.packbits(padded, bitorder="little").view("<i4")


def _check_mask(mask, bits, gpu):
    want = _np_words(bits)
    assert mask.words.dtype == torch.int32 and mask.live.dtype == torch.int32 and mask.words.device == gpu
    assert np.array_equal(mask.words.cpu().numpy(), want)  # the tail bits included: the twin's are zero
    assert np.array_equal(mask.live.cpu().numpy(), np.nonzero(want)[0].astype(np.int32))
    assert mask.rows == len(bits) and isinstance(mask.count, int) and mask.count == int(bits.sum())


BUILDER_N = [1, 31, 32, 33, 63, 64, 65, 4099]


@pytest.mark.parametrize("N", BUILDER_N)
def test_row_mask_from_ids_against_packbits(gpu, N):
    rng = np.random.default_rng(N)
    base = 1000
    inside = rng.integers(base, base + N, size=max(1, N // 3))
    ids = np.concatenate([inside, inside[: len(inside) // 2 + 1],  # duplicates
                          np.array([0, base - 1, base + N, base + N + 31, 2 ** 40])]).astype(np.int64)  # other slices
    rng.shuffle(ids)
    bits = np.zeros(N, dtype=bool)
    bits[inside - base] = True
    for form in (torch.from_numpy(ids).to(gpu), ids.tolist()):
        _check_mask(ops.row_mask_from_ids(form, N, base=base, device=gpu), bits, gpu)
        _check_mask(ops.row_mask_from_ids(form, N, base=base, exclude=True, device=gpu), ~bits, gpu)
    _check_mask(ops.row_mask_from_ids([], N, device=gpu), np.zeros(N, dtype=bool), gpu)
    _check_mask(ops.row_mask_from_ids([], N, exclude=True, device=gpu), np.ones(N, dtype=bool), gpu)
    _check_mask(ops.row_mask_from_ids(list(range(N)), N, device=gpu), np.ones(N, dtype=bool), gpu)
    twin = ops.row_mask_from_ids_ref(ids.tolist(), N, base=base)
    assert np.array_equal(twin.words.numpy(), _np_words(bits)) and twin.count == int(bits.sum())


@pytest.mark.parametrize("N", BUILDER_N)
def test_row_mask_from_labels_against_packbits(gpu, N):
    rng = np.random.default_rng(100 + N)
    lab = rng.integers(-300, 300, size=N).astype(np.int64)
    lo64, hi64 = -2 ** 63, 2 ** 63 - 1
    lab[rng.integers(0, N)] = lo64
    lab[rng.integers(0, N)] = hi64
    dl = torch.from_numpy(lab).to(gpu)
    one = int(lab[N // 2])
    _check_mask(ops.row_mask_from_labels(dl, values=[one]), lab == one, gpu)
    many = list(range(-128, 128))  # 256 values, given unsorted
    _check_mask(ops.row_mask_from_labels(dl, values=many[::-1]), np.isin(lab, many), gpu)
    _check_mask(ops.row_mask_from_labels(dl, values=[lo64, hi64, 7]), np.isin(lab, [lo64, hi64, 7]), gpu)
    lo, hi = int(np.sort(lab)[N // 3]), int(np.sort(lab)[(2 * N) // 3])  # endpoints are labels: inclusive
    _check_mask(ops.row_mask_from_labels(dl, lo=lo, hi=hi), (lab >= lo) & (lab <= hi), gpu)
    _check_mask(ops.row_mask_from_labels(dl, lo=lo64, hi=lo64), lab == lo64, gpu)
    _check_mask(ops.row_mask_from_labels(dl, lo=hi64, hi=hi64), lab == hi64, gpu)
    _check_mask(ops.row_mask_from_labels(dl, lo=lo64, hi=hi64), np.ones(N, dtype=bool), gpu)
    _check_mask(ops.row_mask_from_labels(dl, lo=1000, hi=2000), np.zeros(N, dtype=bool), gpu)
    twin = ops.row_mask_from_labels_ref(torch.from_numpy(lab), values=many)
    assert np.array_equal(twin.words.numpy(), _np_words(np.isin(lab, many)))
    with pytest.raises(ValueError):
        ops.row_mask_from_labels(dl, values=list(range(257)))
    with pytest.raises(ValueError):
        ops.row_mask_from_labels(dl, values=[1], lo=0, hi=1)


def test_built_masks_drive_the_search(gpu):
    """The builders' masks through the kernel: ids with a slice base, and labels."""
    N, k, base = 1000, 10, 300
    q, c, _ = _operands(gpu, "f32", 64, N, 17)
    bits = _pattern("rand50", N)
    ids = (bits.nonzero().flatten() + base).tolist() + [5, base + N + 3]
    mask = ops.row_mask_from_ids(ids, N, base=base, device=gpu)
    _check_equal(ops.sim_topk(q, c, k, base, mask=mask), _gathered(q, c, None, bits, k, base), "ids")
    lab = (torch.arange(N) * 7 % 13).to(gpu)
    mask = ops.row_mask_from_labels(lab, lo=3, hi=5)
    _check_equal(ops.sim_topk(q, c, k, mask=mask), _gathered(q, c, None, ((lab >= 3) & (lab <= 5)).cpu(), k), "labels")


# ---------------------------------------------------------------------------------------- rejections
def test_rejections(gpu):
    N = 100
    q, c = torch.zeros((2, 64), device=gpu), torch.zeros((N, 64), device=gpu)
    good = ops.row_mask_from_bits(torch.ones(N, dtype=torch.bool, device=gpu))
    ops.sim_topk(q, c, 4, mask=good)
    cpu = ops.row_mask_from_bits(torch.ones(N, dtype=torch.bool))
    bad = [cpu,  # another device
           good._replace(live=good.live.cpu()),
           good._replace(words=good.words[:-1].contiguous()),  # wrong length
           good._replace(words=torch.cat([good.words, good.words])),
           good._replace(words=good.words.to(torch.int64)),  # wrong dtype
           good._replace(live=good.live.to(torch.int64)),
           good._replace(live=torch.cat([good.live, good.live])),
           good._replace(rows=N + 1), good._replace(rows=N - 1),  # rows != N
           good._replace(count=N + 1), good._replace(count=0),
           (good.words, good.live, N, N)]  # not a RowMask
    for m in bad:
        with pytest.raises(ValueError):
            ops.sim_topk(q, c, 4, mask=m)
    with pytest.raises(ValueError):
        ops.sim_topk(q, torch.zeros((N + 32, 64), device=gpu), 4, mask=good)


# -------------------------------------------------------------------------------------------- the op
def test_map_search_filters_on_the_gpu_engine_agree_with_the_cpu_engine(gpu, tmp_path, monkeypatch):
    """Each filter form on both engines, compared as
    test_map_search_op_on_the_gpu_engine_agrees_with_the_cpu_engine compares: the rankings agree
    wherever the CPU run's margins exceed what the measured embedding difference can move a score by
    (``2 (|dq| + |dc| + |dq| |dc|)``). What does not depend on the embeddings is compared exactly:
    ``filter_rows``, the list lengths, and that every returned id passes the filter."""
    from agent_tpu_amd.utils.synthetic import make_text_rows
    from ops.map_embed import map_embed
    from ops.map_search import map_search

    model = "bert-tiny?batch=32&seed=2"
    corpus = make_text_rows(60, 30, 11)
    queries = corpus[:5] + make_text_rows(4, 20, 12)
    labels = np.arange(60, dtype=np.int64) * 7 % 10
    lpath = str(tmp_path / "labels.npy")
    np.save(lpath, labels.astype(np.int32))
    allow = [0, 1, 2, 3, 4, 17, 33, 34, 35, 59, 59]
    deny = [5, 6, 17, 33, 34, 35, 59, 59]
    # every form keeps at least one of rows 0 .. 4, which are queries too: their own rows are clear winners
    filters = {
        "ids": ({"ids": allow}, set(allow)),
        "exclude_ids": ({"exclude_ids": deny}, set(range(60)) - set(deny)),
        "labels": ({"labels": [3, 8]}, {r for r in range(60) if labels[r] in (3, 8)}),
        "label_range": ({"label_range": [0, 0]}, {r for r in range(60) if labels[r] == 0}),  # 6 rows: fewer than top_k
    }
    out = {}
    for dev in ("gpu", "cpu"):
        if dev == "cpu":
            monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
        else:
            monkeypatch.delenv("CLASSIFY_DEVICE", raising=False)
        path = str(tmp_path / f"corpus_{dev}.npy")
        assert map_embed({"texts": corpus, "model_path": model, "output": "npy", "output_uri": path})["ok"]
        res = {}
        for name, (flt, _) in filters.items():
            job = {"queries": queries, "corpus_uri": path, "model_path": model, "top_k": 8, "filter": flt,
                   "corpus_labels_uri": lpath}
            res[name] = map_search(job)
        qemb = map_embed({"texts": queries, "model_path": model})["embeddings"]
        out[dev] = (res, np.load(path).astype(np.float64), np.asarray(qemb, dtype=np.float64))
    (g, gc, gq), (h, hc, hq) = out["gpu"], out["cpu"]
    dc = np.linalg.norm(gc - hc, axis=1).max()
    dq = np.linalg.norm(gq - hq, axis=1).max()
    move = 2 * (dq + dc + dq * dc)
    print(f"embedding difference GPU vs CPU engine: corpus {dc:.3e} queries {dq:.3e}; score margin needed {move:.3e}")
    for name, (_, rows) in filters.items():
        kk = min(8, len(rows))
        checked = 0
        for r in (g[name], h[name]):
            assert r["ok"] and r["filter_rows"] == len(rows) and r["corpus_rows"] == 60
            assert all(len(x) == kk and set(x) <= rows and len(set(x)) == kk for x in r["ids"])
        for a in range(len(queries)):
            hs, hi, gi = h[name]["scores"][a], h[name]["ids"][a], g[name]["ids"][a]
            for j in range(kk):
                above = hs[j - 1] - hs[j] if j > 0 else float("inf")
                # the score after the last is unknown when the list was cut at top_k: no claim on the last then
                below = hs[j] - hs[j + 1] if j + 1 < kk else (float("inf") if kk == len(rows) else 0.0)
                if above > move and below > move:
                    assert gi[j] == hi[j], (name, a, j)
                    checked += 1
        assert checked > 0, name
    for a in range(5):  # an allowed corpus text used as a query finds its own row first
        for name in ("ids", "exclude_ids"):
            assert g[name]["ids"][a][0] == a and abs(g[name]["scores"][a][0] - 1.0) < 1e-5
