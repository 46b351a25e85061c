"""ops.window_attention on CPU fp32 against the Swin block's own roll /
partition / get_attn_mask / reverse path: pins the addressing and the
analytic shift mask."""
import pytest
import torch

from timm_amd import ops
from timm_amd.models.swin_transformer import SwinTransformerBlock

# (map, window, shift): both dims shifted, one dim, none, non-square window
CASES = [
    ((14, 14), 7, (3, 3)),
    ((8, 16), (4, 8), (2, 0)),
    ((8, 16), (4, 8), (0, 3)),
    ((14, 7), 7, (0, 0)),
    ((8, 12), (4, 6), (1, 5)),
]


@pytest.mark.parametrize('res,window,shift', CASES)
def test_matches_block_attn(res, window, shift):
    torch.manual_seed(0)
    heads, dim = 2, 16
    blk = SwinTransformerBlock(dim, res, num_heads=heads, window_size=window, shift_size=shift,
                               always_partition=True).eval()
    assert tuple(blk.shift_size) == tuple(shift)
    torch.nn.init.normal_(blk.attn.relative_position_bias_table, std=0.5)
    x = torch.randn(2, *res, dim)
    with torch.no_grad():
        want = blk._attn(x)
        o = ops.window_attention(blk.attn.qkv(x), heads, blk.window_size, blk.shift_size,
                                 bias=blk.attn._get_rel_pos_bias()[0], scale=blk.attn.scale)
        got = blk.attn.proj(o)
    assert torch.allclose(got, want, atol=1e-5, rtol=0), (got - want).abs().max()
