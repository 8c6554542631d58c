"""K-tile image order of an activation tensor (`ops.to_image_order`): the index map."""
import torch

from agent_tpu_amd import ops


def test_image_order_round_trip():
    x = torch.arange(512 * 192, dtype=torch.float32).view(512, 192)
    img = ops.to_image_order(x)
    assert torch.equal(ops.from_image_order(img), x)
    # element (r, c) at (((r/256)*(W/64) + c/64)*256 + r%256)*64 + c%64
    for r, c in ((0, 0), (255, 63), (256, 64), (300, 191), (511, 5)):
        at = (((r // 256) * 3 + c // 64) * 256 + r % 256) * 64 + c % 64
        assert img.view(-1)[at].item() == x[r, c].item()
