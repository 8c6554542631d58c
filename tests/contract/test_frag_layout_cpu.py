"""Fragment order of an activation tensor (`ops.to_fragment_order`): index map and lane model.

The lane model follows the kernels (csrc/kernels/gemm_bf16.hip): MFMA 16x16x32 bf16 with the
operands swapped, so lane (fr, fc) = (lane % 16, lane // 16) of a wave holds, per 16-row block and
fragment j, row fr and columns j*16 + fc*4 .. + 3 (two packed dwords). v_permlane16_swap(x, y)
trades lane rows 1, 3 of x with rows 0, 2 of y.
"""
import numpy as np
import torch

from agent_tpu_amd import ops

PERM = (0, 2, 1, 3)


def _offset(r, c, W):
    """Element offset of (r, c) in a fragment-order [M, W] tensor, written from the definition."""
    image = (r // 256) * (W // 64) + c // 64
    rr, cc = r % 256, c % 64
    group, fr = rr // 16, rr % 16
    half, chunk, e = cc // 32, (cc % 32) // 8, cc % 8
    unit = PERM.index(chunk) * 16 + fr  # unit u holds chunk PERM[u // 16] of row u % 16
    return image * (256 * 64) + group * 1024 + half * 512 + unit * 8 + e


def test_fragment_order_index_map_and_round_trip():
    M, W = 512, 192
    x = torch.arange(M * W, dtype=torch.float32).view(M, W)
    frag = ops.to_fragment_order(x)
    assert frag.shape == x.shape and frag.is_contiguous()
    flat = frag.view(-1).numpy()
    want, xn = np.empty(M * W, dtype=np.float32), x.numpy()
    for r in range(M):
        for c in range(W):
            want[_offset(r, c, W)] = xn[r, c]
    assert np.array_equal(flat, want)
    assert torch.equal(ops.from_fragment_order(frag), x)
    y = torch.randn(256, 64).to(torch.bfloat16)
    assert torch.equal(ops.from_fragment_order(ops.to_fragment_order(y)), y)
    assert torch.equal(ops.to_fragment_order(ops.from_fragment_order(y)), y)
    assert ops.LAYOUT_A_FRAG & ops.LAYOUT_A and ops.LAYOUT_C_FRAG & ops.LAYOUT_C and ops.LAYOUT_R_FRAG & ops.LAYOUT_R


def _swap16(x, y):
    """v_permlane16_swap on [64]-lane arrays (any trailing shape): rows 1, 3 of x <-> rows 0, 2 of y."""
    x, y = x.copy(), y.copy()
    for a, b in ((1, 0), (3, 2)):
        t = x[a * 16:(a + 1) * 16].copy()
        x[a * 16:(a + 1) * 16] = y[b * 16:(b + 1) * 16]
        y[b * 16:(b + 1) * 16] = t
    return x, y


def test_producer_lane_holds_its_unit():
    """Pack + swap of fragments (2h, 2h+1) leaves lane u with unit u of k-half h; the inverse swap of a
    loaded unit gives back the per-fragment columns (the residual path)."""
    W = 64
    blk = np.arange(16 * W, dtype=np.int64).reshape(16, W)  # one 16-row block of a wave: value = r*64 + c
    lane = np.arange(64)
    fr, fc = lane % 16, lane // 16
    # frag[j][lane] = the 4 columns j*16 + fc*4 .. + 3 of row fr
    frag = [np.stack([blk[fr, j * 16 + fc * 4 + e] for e in range(4)], axis=1) for j in range(4)]
    x = torch.from_numpy(np.tile(blk, (16, 1)).astype(np.float32))  # [256, 64]: 16 equal row groups
    group0 = ops.to_fragment_order(x).view(-1)[:16 * W].numpy().astype(np.int64).reshape(2, 64, 8)
    for h in range(2):
        lo, hi = _swap16(frag[2 * h], frag[2 * h + 1])
        unit = np.concatenate([lo, hi], axis=1)  # the lane's 16 bytes: {x dwords, y dwords}
        assert np.array_equal(unit, group0[h]), h
        # residual: load unit u, swap back
        back_lo, back_hi = _swap16(unit[:, :4], unit[:, 4:])
        assert np.array_equal(back_lo, frag[2 * h]) and np.array_equal(back_hi, frag[2 * h + 1])


def test_consumer_read_offsets():
    """The A-fragment read of lane (fr, fc) for k-step ks: its 8 columns ks*32 + fc*8 .. + 7 in k order,
    every 16 lanes 256 contiguous bytes, and every piece a linear 1 KiB copy of global memory."""
    x = torch.arange(256 * 64, dtype=torch.float32).view(256, 64)  # one image: value = r*64 + c
    img = ops.to_fragment_order(x).view(-1).numpy().astype(np.int64)  # the LDS A image = the global image
    for group in range(16):
        for ks in range(2):
            piece = group * 2048 + ks * 1024  # bytes
            offs = []
            for lane in range(64):
                fr, fc = lane % 16, lane // 16
                off = piece + (PERM[fc] * 16 + fr) * 16
                offs.append(off)
                got = img[off // 2: off // 2 + 8]
                want = (group * 16 + fr) * 64 + ks * 32 + fc * 8 + np.arange(8)
                assert np.array_equal(got, want), (group, ks, lane)
            for q in range(4):  # a quarter-wave of the ds_read_b128
                o = sorted(offs[q * 16:(q + 1) * 16])
                assert o == list(range(o[0], o[0] + 256, 16)) and o[0] % 256 == 0
            assert sorted(offs) == list(range(piece, piece + 1024, 16))


def test_staging_quarters_cover_the_same_rows():
    """Quarter 0 / 3 of the DMA program: 16 pieces each, the row groups {0-3, 8-11} / {4-7, 12-15}
    (rows 0-63 + 128-191 / 64-127 + 192-255, as the row-major quarters), every piece once."""
    def fpiece(q, p):
        return (((p >> 1) & 3) + (p >> 3) * 8 + (4 if q == 3 else 0)) * 2048 + (p & 1) * 1024

    seen = []
    for q, groups in ((0, [0, 1, 2, 3, 8, 9, 10, 11]), (3, [4, 5, 6, 7, 12, 13, 14, 15])):
        pieces = [fpiece(q, i * 8 + wave) for i in range(2) for wave in range(8)]
        assert sorted(pieces) == sorted(g * 2048 + h * 1024 for g in groups for h in range(2))
        seen += pieces
    assert sorted(seen) == list(range(0, 32768, 1024))
