"""Exact-arithmetic inputs for decode attention: the correct output is known bit for bit.

A plain helper module (no tests, no conftest): `tests/contract/test_decode_exact_cpu.py` proves the
constructions on the CPU path of `ops.decode_attention` and shows every mutant of the by-definition
evaluator failing them, `tests/kernels/test_decode_exact_gpu.py` runs the HIP kernels on the same cases.

All values are small integers or powers of two (exact in bf16 and in every fp32 partial sum), the scale
is 1 or 1/8. What the decode kernels can get wrong is addressing, so every V row carries its address:
dim 0 the physical cache row (self attention) or the item (cross attention), dims 1-2 the position
(low byte, high part), dim 3 the head, dims 4..63 the dim index. A decoy row has dim 0 = -100.

Queries. (row, head) owns one of 72 patterns of 8 dims out of 64 (the lines of the affine plane over
GF(8): two patterns share at most one dim); pattern (row % 36) * 2 + (head & 1). The query is 16 on its
pattern; a *hot* key is 16 on the same pattern (score 2048 * scale), any other row's hot key scores at
most 256 * scale, an empty key 0: at least 224 lower. Then exp(s - max) is exactly 1 for the hot key and
exactly 0 for every other key in fp32 (e^-200 underflows), the denominator is 1 and the output is the hot
key's V row. A *targeted decoy* (32 on the pattern, -32 off it) scores twice the hot key for its row and
below 0 for every other pattern; a *universal decoy* (32 everywhere) wins for every query.

Constructions (each returns a `Case`; `Case.expect` is the exact bf16 output):
  one_hot   one hot key per (row, head), decoys at positions len and len + 1, at position len - 1 of the
            row hist[r, len - 1] names, and at the hot position of the neighbouring item / row / head;
  bias_hot  q = 0, bias_dist[h] = 512 at one distance d*_h (256 at distance 0): key len - 1 - d*_h wins
            (key len - 1 where the item is shorter than d*_h);
  ties      two hot keys, in the first and the last 64-key chunk that holds keys: (Va + Vb) / 2;
  combine   a local winner in every 64-key chunk, one global winner: the other chunks' weights underflow;
  counts    q = 0, V[j][d] = (j % 64 == d): out[d] * len is the number of attended keys j = d mod 64.
"""
import functools
from types import SimpleNamespace

import torch

from agent_tpu_amd import ops

BF, F64 = torch.bfloat16, torch.float64
D = 64
CHUNK = 64
MARGIN = 200.0
DECOY = -100.0

MUTANTS = ("len_plus", "len_minus", "hist_at_current", "hist_ignored", "hist_next", "hist_first", "hist_mod64",
           "bias_by_j", "bias_head0", "item_is_row", "last_twice", "first_chunk_only", "v_heads_swapped")
SELF_MUTANTS = ("len_plus", "len_minus", "hist_at_current", "hist_ignored", "hist_next", "hist_first", "hist_mod64",
                "bias_by_j", "bias_head0", "last_twice", "v_heads_swapped")
CROSS_MUTANTS = ("len_plus", "len_minus", "bias_by_j", "bias_head0", "item_is_row", "last_twice", "v_heads_swapped")
CHUNK_MUTANTS = CROSS_MUTANTS + ("first_chunk_only",)


# ------------------------------------------------------------------ patterns
def _gf8_mul(a, b):
    r = 0
    for i in range(3):
        if (b >> i) & 1:
            r ^= a << i
    for i in (4, 3):
        if (r >> i) & 1:
            r ^= 0b1011 << (i - 3)
    return r


@functools.lru_cache(maxsize=None)
def patterns():
    """[72, 64] 0/1: the lines y = a x + b and x = c of the affine plane over GF(8), point (x, y) = dim 8x + y."""
    p = torch.zeros((72, D), dtype=F64)
    for a in range(8):
        for b in range(8):
            for x in range(8):
                p[a * 8 + b, 8 * x + (_gf8_mul(a, x) ^ b)] = 1
    for c in range(8):
        p[64 + c, 8 * c:8 * c + 8] = 1
    return p


def pattern_id(r, h):
    return (r % 36) * 2 + (h & 1)


# ------------------------------------------------------------------ geometry of one launch
class Geo:
    """Rows, heads, cache length and which keys a row may attend to (by definition).

    Self attention: `step` (len = step + 1 for every row), optional `hist` [R, T]; the physical rows are
    the R cache rows. Cross attention: `lens` per item, rows of item r // group; the physical rows are
    the items."""

    def __init__(self, R, H, S, group=1, lens=None, step=None, hist=None):
        assert (lens is None) != (step is None)
        self.R, self.H, self.S, self.group = R, H, S, group
        self.cross = lens is not None
        self.nseq = (R + group - 1) // group
        self.lens = None if lens is None else [int(x) for x in lens]
        self.step = step
        self.hist = hist
        assert not self.cross or len(self.lens) == self.nseq
        assert self.cross or group == 1
        self.NP = self.nseq if self.cross else R

    def n(self, r):
        return min(self.lens[r // self.group] if self.cross else self.step + 1, self.S)

    def phys(self, r, j):
        """Physical row (item) that holds key j of row r."""
        if self.cross:
            return r // self.group
        if self.hist is not None and j < self.n(r) - 1:
            return int(self.hist[r, j])
        return r


def beam_hist(R, T):
    """Backpointers as a beam search leaves them: row r of the 4-row beam group 4 (r // 4) points at rows of
    its own group, at an offset of 1 + (j // 3 + j + r) % 3 from itself (never at itself in a complete group).
    The offset changes from j to j + 1 in two steps out of three and always from j to j + 64, so a backpointer
    read one position off, at position 0 or a 64-key chunk off names another cache row."""
    r = torch.arange(R).view(R, 1)
    j = torch.arange(T).view(1, T)
    base = 4 * (r // 4)
    gs = (R - base).clamp(max=4)
    return (base + (r - base + 1 + (j // 3 + j + r) % 3) % gs).to(torch.int32).contiguous()


# ------------------------------------------------------------------ cases
class Case(SimpleNamespace):
    """One launch: q [R, H*64] (a column slice of a wider tensor with `wide`), k / v (column slices of one
    [NP*S, 2*H*64] cache), lens or step, hist, bias, scale; `expect` bf16 [R, H*64] (kind "equal") or
    `count` int64 [R, H*64] with `n_rows` [R] (kind "count")."""

    def args(self, dev="cpu"):
        g = self.geo
        to = lambda t: None if t is None else t.to(dev)  # noqa: E731
        q = to(self.q_wide)[:, :g.H * D] if self.q_wide is not None else to(self.q)
        kv = to(self.kv)
        return dict(q=q, k=kv[:, :g.H * D], v=kv[:, g.H * D:], H=g.H, seq_stride=g.S, group=g.group,
                    lens=to(self.lens), step=to(self.step), bias_dist=to(self.bias), scale=self.scale, hist=to(self.hist))

    def run(self, dev="cpu"):
        return ops.decode_attention(**self.args(dev))


def _address_cache(geo):
    """Zero K, address-carrying V: [NP, S, 2, H, 64] bf16."""
    kv = torch.zeros((geo.NP, geo.S, 2, geo.H, D), dtype=BF)
    v = kv[:, :, 1]
    v[..., 4:] = torch.arange(4, D, dtype=torch.float32)
    v[..., 0] = torch.arange(geo.NP, dtype=torch.float32).view(-1, 1, 1)
    v[..., 1] = (torch.arange(geo.S) & 255).float().view(1, -1, 1)
    v[..., 2] = (torch.arange(geo.S) >> 8).float().view(1, -1, 1)
    v[..., 3] = torch.arange(geo.H, dtype=torch.float32).view(1, 1, -1)
    return kv


def decode_address(row):
    """A V row (or an output row of 64 values) as text: where it was read from."""
    x = [float(t) for t in row[:4]]
    dims_ok = bool((row[4:].double() == torch.arange(4, D, dtype=F64)).all())
    tag = "decoy " if x[0] == DECOY else ""
    return f"{tag}row/item {x[0]:g} pos {x[1] + 256 * x[2]:g} head {x[3]:g} dims {'in order' if dims_ok else 'PERMUTED'}"


class _Build:
    def __init__(self, geo, scale, wide, name):
        self.geo, self.scale, self.wide, self.name = geo, float(scale), wide, name
        self.kv = _address_cache(geo)
        self.q = torch.zeros((geo.R, geo.H, D), dtype=F64)
        self.taken = torch.zeros((geo.NP, geo.S, geo.H), dtype=torch.bool)
        self.hot = {}  # (r, h) -> [positions]
        self.decoys = {"past_len": 0, "hist_current": 0, "neighbour_item_or_row": 0, "neighbour_head": 0}

    def K(self, p, j, h):
        return self.kv[p, j, 0, h]

    def V(self, p, j, h):
        return self.kv[p, j, 1, h]

    def free_pos(self, r, h, start, lo, hi):
        """First position from `start` (cyclic in [lo, hi)) whose slot for row r, head h is free, or None."""
        for i in range(hi - lo):
            j = lo + (start - lo + i) % (hi - lo)
            if not self.taken[self.geo.phys(r, j), j, h]:
                return j
        return None

    def put_hot(self, r, h, j, dims=8):
        """Key j of row r, head h <- 16 on the first `dims` dims of the row's pattern."""
        pat = patterns()[pattern_id(r, h)].clone()
        if dims < 8:
            pat[pat.nonzero().view(-1)[dims:]] = 0
        p = self.geo.phys(r, j)
        self.K(p, j, h).copy_(16 * pat)
        self.taken[p, j, h] = True

    def put_decoy(self, p, j, h, pid, kind):
        """A decoy aimed at the query pattern pid (None: at every query) in slot (p, j, h), if that exists and is free."""
        g = self.geo
        if not (0 <= p < g.NP and 0 <= j < g.S and 0 <= h < g.H) or self.taken[p, j, h]:
            return
        pat = torch.ones(D, dtype=F64) if pid is None else 2 * patterns()[pid] - 1
        self.K(p, j, h).copy_(32 * pat)
        self.V(p, j, h)[0] = DECOY
        self.taken[p, j, h] = True
        self.decoys[kind] += 1

    def finish(self, expect=None, bias=None, count=None, check_margin=True):
        g = self.geo
        q = self.q.view(g.R, g.H * D).to(BF)
        q_wide = None
        if self.wide:  # the stride of a fused QKV output; the other columns hold values that would show
            q_wide = torch.full((g.R, 3 * g.H * D), 16.0, dtype=BF)
            q_wide[:, :g.H * D] = q
        c = Case(name=self.name, geo=g, q=q, q_wide=q_wide, kv=self.kv.view(g.NP * g.S, 2 * g.H * D),
                 lens=None if not g.cross else torch.tensor(g.lens, dtype=torch.int32),
                 step=None if g.cross else torch.tensor([g.step], dtype=torch.int32), hist=g.hist, bias=bias,
                 scale=self.scale, expect=None if expect is None else expect.view(g.R, g.H * D).to(BF), count=count,
                 kind="equal" if count is None else "count", hot=self.hot, decoys=self.decoys,
                 n_rows=torch.tensor([g.n(r) for r in range(g.R)]))
        if check_margin:
            c.margin = assert_margin(c)
        return c


def assert_margin(c):
    """The condition on the inputs (fp64, by definition): for every (row, head) the hot keys hold the maximum
    score and every other key the row may attend to scores at least MARGIN lower. Returns the smallest gap."""
    g = c.geo
    worst = float("inf")
    _, scores = evaluate(c, want_scores=True)
    for r in range(g.R):
        for h in range(g.H):
            s = scores[r][h]
            hot = torch.zeros(s.numel(), dtype=torch.bool)
            hot[c.hot[(r, h)]] = True
            assert bool((s[hot] == s.max()).all()), (c.name, r, h, "the hot key does not hold the maximum")
            if (~hot).any():
                gap = (s.max() - s[~hot].max()).item()
                assert gap >= MARGIN, (c.name, r, h, gap)
                worst = min(worst, gap)
    return worst


def _hot_candidates(n, r, h):
    c = [n - 1, 0, n - 2, 63, 64, n // 2, 65, 1, n - 65, 127, 128, (7 * r + 13 * h) % n]
    return [x for x in c if 0 <= x < n]


def one_hot(geo, scale=1.0, wide=True, decoys=True, zero_bias=False, variant=0, name="one_hot"):
    b = _Build(geo, scale, wide, name)
    g = geo
    expect = torch.zeros((g.R, g.H, D), dtype=F64)
    for r in range(g.R):
        for h in range(g.H):
            n = g.n(r)
            cand = _hot_candidates(n, r, h)
            j = b.free_pos(r, h, cand[(r + h + variant) % len(cand)], 0, n)
            b.q[r, h] = 16 * patterns()[pattern_id(r, h)]
            if j is None:  # more rows than keys: only a one-key item shares its key, and needs no margin
                assert n == 1, (name, r, h, n)
                j = 0
            else:
                b.put_hot(r, h, j)
            b.hot[(r, h)] = [j]
    for r in range(g.R):
        for h in range(g.H):
            j = b.hot[(r, h)][0]
            expect[r, h] = b.V(g.phys(r, j), j, h).double()
    if decoys:
        for h in range(g.H):  # positions nobody may read: the first two past the length
            for p in range(g.NP):
                n = g.n(p * g.group)
                b.put_decoy(p, n, h, None, "past_len")
                b.put_decoy(p, n + 1, h, None, "past_len")
        for r in range(g.R):
            for h in range(g.H):
                n, j, pid = g.n(r), b.hot[(r, h)][0], pattern_id(r, h)
                p = g.phys(r, j)
                if g.hist is not None and n >= 1 and int(g.hist[r, n - 1]) != r:
                    b.put_decoy(int(g.hist[r, n - 1]), n - 1, h, pid, "hist_current")
                b.put_decoy(p + 1, j, h, pid, "neighbour_item_or_row")
                b.put_decoy(p - 1, j, h, pid, "neighbour_item_or_row")
                b.put_decoy(p, j, h ^ 1, pid, "neighbour_head")
    bias = torch.zeros((g.H, g.S), dtype=torch.float32) if zero_bias else None
    return b.finish(expect, bias=bias)


def bias_hot(geo, scale=1.0, wide=True, name="bias_hot"):
    """q = 0: the scores are the bias alone. bias_dist[h, d*_h] = 512, bias_dist[h, 0] = 256 (so an item
    shorter than d*_h + 1 has the winner len - 1), d*_h from 0, every len - 1 of the launch and the chunk edges."""
    b = _Build(geo, scale, wide, name)
    g = geo
    b.kv[:, :, 0] = 3.0  # K does not matter with q = 0
    ns = sorted({g.n(r) for r in range(g.R)})
    cand = sorted({0, 1, 62, 63, 64, 65} | {n - 1 for n in ns} | {n - 2 for n in ns})
    cand = [d for d in cand if 0 <= d < g.S]
    bias = torch.zeros((g.H, g.S), dtype=torch.float32)
    expect = torch.zeros((g.R, g.H, D), dtype=F64)
    dstar = []
    for h in range(g.H):
        # head 0: d* = len - 1 of the longest item (its first key wins), head 1: d* = 0, then the candidates in turn
        d = max(ns) - 1 if h == 0 else 0 if h == 1 else cand[(5 * h + 1) % len(cand)]
        bias[h, 0] = 256.0
        bias[h, d] = 512.0
        dstar.append(d)
    for r in range(g.R):
        for h in range(g.H):
            n = g.n(r)
            j = n - 1 - (dstar[h] if dstar[h] < n else 0)
            b.hot[(r, h)] = [j]
            expect[r, h] = b.V(g.phys(r, j), j, h).double()
    c = b.finish(expect, bias=bias)
    c.dstar = dstar
    return c


def ties(geo, scale=1.0, wide=True, name="ties"):
    """Two hot keys per (row, head), one in the first and one in the last 64-key chunk that holds keys (where the
    row has room for two): the output is (Va + Vb) / 2, rounded to bf16 once."""
    b = _Build(geo, scale, wide, name)
    g = geo
    for r in range(g.R):  # every (row, head) its first key, then the second where a slot is left
        for h in range(g.H):
            n = g.n(r)
            b.q[r, h] = 16 * patterns()[pattern_id(r, h)]
            ja = b.free_pos(r, h, (3 * r + 5 * h) % min(n, CHUNK), 0, n)
            if ja is None:
                assert n == 1, (name, r, h, n)
                ja = 0
            else:
                b.put_hot(r, h, ja)
            b.hot[(r, h)] = [ja]
    for r in range(g.R):
        for h in range(g.H):
            n = g.n(r)
            lo = CHUNK * ((n - 1) // CHUNK)
            jb = b.free_pos(r, h, n - 1 - (r + 2 * h) % min(n - lo, 8), lo, n)
            if jb is None and lo > 0:  # the item's other beams fill the last chunk: the last free key before it
                jb = next((j for j in range(lo - 1, -1, -1) if not b.taken[g.phys(r, j), j, h]), None)
            if jb is not None:
                b.put_hot(r, h, jb)
                b.hot[(r, h)].append(jb)
    expect = torch.zeros((g.R, g.H, D), dtype=F64)
    for (r, h), js in b.hot.items():
        expect[r, h] = sum(b.V(g.phys(r, j), j, h).double() for j in js) / len(js)
    return b.finish(expect)


def combine(geo, scale=1.0, wide=True, name="combine"):
    """One global winner per (row, head) and a local winner (16 on a part of the pattern only) in every other
    64-key chunk that holds keys: e^(local - global) underflows, the output is the global winner's V row."""
    b = _Build(geo, scale, wide, name)
    g = geo
    nk = lambda n, c: min(CHUNK, n - c * CHUNK)  # noqa: E731
    where = {}
    for r in range(g.R):  # the global winners first, then the local ones where slots are left
        for h in range(g.H):
            n = g.n(r)
            cg = (r + h) % ((n + CHUNK - 1) // CHUNK)
            b.q[r, h] = 16 * patterns()[pattern_id(r, h)]
            j = b.free_pos(r, h, cg * CHUNK + (5 * r + 3 * h) % nk(n, cg), cg * CHUNK, cg * CHUNK + nk(n, cg))
            if j is None:
                j = b.free_pos(r, h, 0, 0, n)
            if j is None:
                assert n == 1, (name, r, h, n)
                j = 0
            else:
                b.put_hot(r, h, j)
            b.hot[(r, h)] = [j]
            where[(r, h)] = j // CHUNK
    for r in range(g.R):
        for h in range(g.H):
            n = g.n(r)
            for c in range((n + CHUNK - 1) // CHUNK):
                if c != where[(r, h)]:
                    jl = b.free_pos(r, h, c * CHUNK + (7 * r + 11 * h + c) % nk(n, c), c * CHUNK, c * CHUNK + nk(n, c))
                    if jl is not None:
                        b.put_hot(r, h, jl, dims=1 + c % 4 if scale == 1.0 else 1)
    expect = torch.zeros((g.R, g.H, D), dtype=F64)
    for (r, h), js in b.hot.items():
        expect[r, h] = b.V(g.phys(r, js[0]), js[0], h).double()
    return b.finish(expect)


def counts(geo, scale=1.0, wide=True, name="counts"):
    """q = 0, no bias, V[j][d] = (j % 64 == d) in every row and head: every key has weight 1 / len."""
    b = _Build(geo, scale, wide, name)
    g = geo
    assert g.S <= 2048
    b.kv[:, :, 0] = 3.0
    onehot = (torch.arange(g.S).view(-1, 1) % D == torch.arange(D).view(1, -1)).float()
    b.kv[:, :, 1] = onehot.view(1, g.S, 1, D)
    cnt = torch.zeros((g.R, g.H, D), dtype=torch.int64)
    for r in range(g.R):
        cnt[r] = onehot[:g.n(r)].sum(0).long().view(1, D)
    return b.finish(count=cnt.view(g.R, g.H * D), check_margin=False)


def check(c, out):
    """"" if `out` is what the case demands, else a message naming the first wrong (row, head) and what it read.
    kind "equal": bit equality. kind "count": rows whose length is a power of two are bit-equal to count / len;
    the others satisfy round(out * len) == count (counts <= 32, one bf16 rounding: |error| < 0.07)."""
    g = c.geo
    out = out.detach().cpu()
    if c.kind == "equal":
        if torch.equal(out, c.expect):
            return ""
        bad = (out != c.expect).view(g.R, g.H, D).any(-1).nonzero()
        r, h = (int(x) for x in bad[0])
        got, want = out.view(g.R, g.H, D)[r, h], c.expect.view(g.R, g.H, D)[r, h]
        return (f"{c.name}: {len(bad)} of {g.R * g.H} (row, head) wrong; first row {r} head {h} len {g.n(r)} "
                f"hot {c.hot.get((r, h))}: got [{decode_address(got)}] {got[:4].tolist()}, want [{decode_address(want)}]")
    n = c.n_rows.view(-1, 1).double()
    pow2 = (c.n_rows & (c.n_rows - 1)) == 0
    exact = (c.count.double() / n).to(BF)
    ok = torch.where(pow2.view(-1, 1), out == exact, (out.double() * n).round() == c.count.double())
    if bool(ok.all()):
        return ""
    r, col = (int(x) for x in (~ok).nonzero()[0])
    return (f"{c.name}: row {r} head {col // D} dim {col % D} len {g.n(r)}: out * len = {float(out[r, col]) * g.n(r):.4f}, "
            f"count {int(c.count[r, col])}; {int((~ok).sum())} entries wrong")


# ------------------------------------------------------------------ the by-definition evaluator and its mutants
def evaluate(c, mutant=None, want_scores=False):
    """softmax(q k^T scale + bias) v over the keys each row may attend to, in fp64 (probabilities rounded to
    fp32 once, so e^-200 is the 0 it is on the device). `mutant`: one deliberate mistake, see MUTANTS."""
    a = c.args()
    return evaluate_args(mutant=mutant, want_scores=want_scores, **a)


def evaluate_args(q, k, v, H, seq_stride, group, lens, step, bias_dist, scale, hist, mutant=None, want_scores=False):
    assert mutant is None or mutant in MUTANTS
    R, S = q.shape[0], seq_stride
    out = torch.zeros((R, H * D), dtype=F64)
    nseq = (R + group - 1) // group
    scores = []
    hswap = torch.arange(H) ^ 1
    hswap = torch.where(hswap < H, hswap, torch.arange(H))
    for r in range(R):
        s = r // group
        if mutant == "item_is_row" and lens is not None:
            s = r % nseq
        n = min(int(lens[s]) if lens is not None else int(step.reshape(-1)[0]) + 1, S)
        if mutant == "len_plus":
            n = min(n + 1, S)
        if mutant == "len_minus":
            n -= 1
        pos = torch.arange(n)
        phys = torch.full((n,), r if lens is None else s, dtype=torch.int64)
        if hist is not None and mutant != "hist_ignored":
            upto = n if mutant == "hist_at_current" else max(n - 1, 0)
            at = torch.arange(upto)  # the position whose backpointer is read for key j
            if mutant == "hist_next":
                at = (at + 1).clamp(max=hist.shape[1] - 1)
            if mutant == "hist_first":
                at = at * 0
            if mutant == "hist_mod64":
                at = at % CHUNK
            phys[:upto] = hist[r, at].long()
        dist = n - 1 - pos
        if mutant == "bias_by_j":
            dist = pos
        if mutant == "first_chunk_only":
            pos, phys, dist = pos[:CHUNK], phys[:CHUNK], dist[:CHUNK]
        if mutant == "last_twice" and n > 0:
            pos, phys, dist = (torch.cat([t, t[-1:]]) for t in (pos, phys, dist))
        if pos.numel() == 0:
            scores.append(torch.zeros((H, 0), dtype=F64))
            continue
        idx = phys * S + pos
        kk = k[idx][:, :H * D].double().view(-1, H, D)
        vv = v[idx][:, :H * D].double().view(-1, H, D)
        if mutant == "v_heads_swapped":
            vv = vv[:, hswap]
        sc = torch.einsum("hd,nhd->hn", q[r, :H * D].double().view(H, D), kk) * scale
        if bias_dist is not None:
            bb = bias_dist.double()
            if mutant == "bias_head0":
                bb = bb[:1].expand(H, -1)
            sc = sc + bb[:, dist.clamp(0, bias_dist.shape[1] - 1)]
        scores.append(sc)
        p = torch.exp(sc - sc.max(-1, keepdim=True).values).float().double()
        out[r] = (torch.einsum("hn,nhd->hd", p, vv) / p.sum(-1, keepdim=True)).reshape(-1)
    return (out, scores) if want_scores else out


# ------------------------------------------------------------------ the case lists, route by route
def _self_cases(R, H, T, n, hist_on, with_bias, scale, wide):
    geo = Geo(R, H, T, step=n - 1, hist=beam_hist(R, T) if hist_on else None)
    tag = f"self R{R} H{H} T{T} len{n} hist{int(hist_on)}"
    out = [one_hot(geo, scale, wide, name=f"one_hot {tag}"), ties(geo, scale, not wide, name=f"ties {tag}"),
           counts(geo, scale, wide, name=f"counts {tag}")]
    if with_bias:
        out += [bias_hot(geo, scale, wide, name=f"bias_hot {tag}"),
                one_hot(geo, scale, not wide, zero_bias=True, variant=3, name=f"one_hot zero-bias {tag}")]
    if n > CHUNK:
        out.append(combine(geo, scale, wide, name=f"combine {tag}"))
    return out


def _cross_cases(R, H, S, group, lens, with_bias, scale, wide, big=False):
    geo = Geo(R, H, S, group=group, lens=lens)
    tag = f"cross R{R} H{H} S{S} group{group} lens{lens if len(lens) <= 4 else str(lens[:4]) + '...'}"
    out = [one_hot(geo, scale, wide, name=f"one_hot {tag}"), ties(geo, scale, not wide, name=f"ties {tag}"),
           counts(geo, scale, wide, name=f"counts {tag}")]
    if with_bias:
        out.append(bias_hot(geo, scale, wide, name=f"bias_hot {tag}"))
        if not big:
            out.append(one_hot(geo, scale, not wide, zero_bias=True, variant=3, name=f"one_hot zero-bias {tag}"))
    if max(lens) > CHUNK:
        out.append(combine(geo, scale, wide, name=f"combine {tag}"))
    return out


def _fit(lens, T):
    return sorted({min(n, T) for n in lens if n <= T} | {T})


def _triples(lens):
    """The lengths three at a time (one per item), every length once, the last triple filled up from the front."""
    lens = list(lens)
    lens += lens[:-len(lens) % 3]
    return [lens[i:i + 3] for i in range(0, len(lens), 3)]


ROUTES = ("self_few", "self_rows_head_groups_t70", "self_rows_head_groups_t200", "self_rows_one_workgroup", "self_fallback",
          "cross_short", "cross_large_grid", "cross_chunked16", "cross_split16", "cross_split32", "cross_chunked32")
ROUTE_MUTANTS = {r: SELF_MUTANTS if r.startswith("self") else CROSS_MUTANTS if r in ("cross_short", "cross_large_grid")
                 else CHUNK_MUTANTS for r in ROUTES}


def route_cases(route):
    """The cases of one kernel route, built anew at every call (the largest list holds 0.7 GB of K/V: it lives
    as long as the test that asked for it). cross_chunked16 is the cross_large_grid list under batch invariance."""
    out = []
    if route == "self_few":  # decode_self_few_kernel<1 | 2 | 3>
        for T in (64, 128, 130, 192):
            for i, n in enumerate(_fit((1, 2, 8, 9, 63, 64, 65), T)):
                for hist_on in (True, False):
                    out += _self_cases(4, 4, T, n, hist_on, with_bias=(i + hist_on) % 2 == 0,
                                       scale=0.125 if i % 2 else 1.0, wide=i % 2 == 0)
    elif route in ("self_rows_head_groups_t70", "self_rows_head_groups_t200"):  # decode_self_attention_kernel, grid.y
        T = 70 if route.endswith("t70") else 200
        for i, n in enumerate(_fit((1, 31, 32, 33, 63, 64, 65, 129), T)):
            out += _self_cases(4, 5, T, n, hist_on=i % 3 != 2, with_bias=i % 2 == 0, scale=0.125 if i % 2 else 1.0,
                               wide=i % 2 == 0)
    elif route == "self_rows_one_workgroup":  # rows >= 128: the waves own 2, 1, 1, 1 of the 5 heads
        for i, n in enumerate((1, 65, 200)):
            out += _self_cases(130, 5, 200, n, hist_on=True, with_bias=i != 1, scale=0.125 if i % 2 else 1.0,
                               wide=i % 2 == 0)
    elif route == "self_fallback":  # ATPU_DEC_SELF=0: decode_attention_kernel<1, 4> with hist and prow
        for T in (70, 300):
            for i, n in enumerate(_fit((1, 16, 17, 64, 65, 129), T)):
                out += _self_cases(4, 5, T, n, hist_on=i % 3 != 2, with_bias=i % 2 == 0, scale=0.125 if i % 2 else 1.0,
                                   wide=i % 2 == 0)
    elif route == "cross_short":  # decode_attention_kernel<1 | 4 | 8>, S < 128; groups 3 and 5: G < GM
        for gi, group in enumerate((1, 3, 4, 5, 8)):
            for i, lens in enumerate(_triples((1, 15, 16, 17, 63, 64, 65, 100))):
                lens = lens[gi % 3:] + lens[:gi % 3]
                out += _cross_cases(3 * group - (group > 1), 3, 100, group, lens, with_bias=(i + gi) % 2 == 0,
                                    scale=0.125 if (i + gi) % 2 else 1.0, wide=i % 2 == 0)
    elif route in ("cross_large_grid", "cross_chunked16"):  # nseq * H >= 512: decode_attention_kernel<4>; chunked<4, 4, 16>
        cyc = (1, 128, 129, 255, 256, 257, 300, 63, 64, 65, 2, 299)
        lens = [cyc[i % len(cyc)] for i in range(43)]
        out += _cross_cases(85, 12, 300, 2, lens, with_bias=True, scale=0.125, wide=True, big=True)
    elif route == "cross_split16":  # decode_cross_split_kernel + combine<16>
        for gi, group in enumerate((1, 3, 4, 8)):
            for i, lens in enumerate(_triples((1, 63, 64, 65, 128, 129, 200))):
                lens = lens[gi % 3:] + lens[:gi % 3]
                out += _cross_cases(3 * group - (group > 1), 3, 200, group, lens, with_bias=(i + gi) % 2 == 0,
                                    scale=0.125 if (i + gi) % 2 else 1.0, wide=i % 2 == 0)
    elif route == "cross_split32":  # S > 1024: 17 chunks, combine<32>
        for i, lens in enumerate(([1088, 1025], [64, 1088])):
            out += _cross_cases(7, 2, 1088, 4, lens, with_bias=i == 0, scale=0.125 if i else 1.0, wide=i == 0)
    elif route == "cross_chunked32":  # batch invariance, nseq * H >= 512, S > 1024
        cyc = (1088, 1025, 1, 1024, 64, 65, 1087, 600)
        lens = [cyc[i % len(cyc)] for i in range(32)]
        out += _cross_cases(32, 16, 1088, 1, lens, with_bias=True, scale=0.125, wide=True, big=True)
    else:
        raise KeyError(route)
    return out


def run_cases(cases, dev):
    """Every case on `dev`; the messages of those that fail."""
    bad = []
    for c in cases:
        msg = check(c, c.run(dev))
        if msg:
            bad.append(msg)
    return bad


def fallback_sweep(dev):
    """The self-attention cases of the ATPU_DEC_SELF=0 child process (T = 70 and T = 300); the failures' messages."""
    return run_cases(route_cases("self_fallback"), dev)


# ------------------------------------------------------------------ five decode steps through the real cache ops
def step_chain(dev, rows=6, H=2, T=20, steps=5):
    """kv_append, beam_reorder_hist with a non-identity parent, self attention: at step t every row's query is
    aimed at the key written 2 steps earlier (at step 0 and 1: at step 0), which lives in the cache row of the
    row's ANCESTOR at that step. The ancestor is followed here through the parents, by definition, not through
    the hist table the ops maintain. Returns the mismatch messages."""
    d = H * D
    pat = patterns()
    cache = torch.zeros((rows * T, 2 * d), dtype=BF, device=dev)
    hist = [torch.zeros((rows, T), dtype=torch.int32, device=dev) for _ in range(2)]
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    parents, bad = [], []
    pid = lambda r, t, h: (r * steps + t) * 2 + (h & 1)  # noqa: E731  (60 distinct patterns: scale 1 margin 1792)
    assert rows * steps * 2 <= 72
    for t in range(steps):
        step.fill_(t)
        qkv = torch.zeros((rows, 3, H, D), dtype=F64)
        want = torch.zeros((rows, H, D), dtype=F64)
        tj = max(t - 2, 0)
        for r in range(rows):
            anc = r
            for s in range(t - 1, tj - 1, -1):  # the beam in row r at step t sat in row anc at step tj
                anc = parents[s][anc]
            for h in range(H):
                qkv[r, 0, h] = 16 * pat[pid(anc, tj, h)]
                qkv[r, 1, h] = 16 * pat[pid(r, t, h)]
                qkv[r, 2, h] = torch.cat([torch.tensor([r, t, 0, h], dtype=F64), torch.arange(4, D, dtype=F64)])
                want[r, h] = torch.cat([torch.tensor([anc, tj, 0, h], dtype=F64), torch.arange(4, D, dtype=F64)])
        qkv = qkv.view(rows, 3 * d).to(BF).to(dev)
        ops.kv_append(qkv, d, 2 * d, cache, T, step)
        out = ops.decode_attention(qkv[:, :d], cache[:, :d], cache[:, d:], H, T, 1, step=step, hist=hist[t % 2])
        if not torch.equal(out.cpu(), want.view(rows, d).to(BF)):
            o = out.cpu().view(rows, H, D)
            r, h = (int(x) for x in (o != want.to(BF)).any(-1).nonzero()[0])
            bad.append(f"step {t} row {r} head {h}: got [{decode_address(o[r, h])}], want [{decode_address(want[r, h])}]")
        parent = [(r * 2 + t + 1) % rows if (r + t) % 3 else (r + 2) % rows for r in range(rows)]
        parents.append(parent)
        ops.beam_reorder_hist(hist[t % 2], hist[(t + 1) % 2], torch.tensor(parent, dtype=torch.int32, device=dev), step)
    return bad
