"""mit_conv_gemm with a live-block list and mit_conv_small_cout with a live-cell map against their dense launches: live positions carry
the dense launch's bits, everything else keeps the sentinel the output was filled with (a skipped or dead row stores nothing)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
B, HI, WI, CIN, COUT = 3, 12, 20, 16, 64     # sub-grid 12 x 20: 2 x 3 blocks of 8 x 8 per image, both sides clipped
BH, BW = 2, 3


def _patterns():
    rng = np.random.default_rng(11)
    empty = np.zeros((B, BH, BW), bool)
    full = np.ones((B, BH, BW), bool)
    corners = empty.copy()
    corners[1, 0, 0] = corners[1, 0, BW - 1] = corners[1, BH - 1, 0] = corners[1, BH - 1, BW - 1] = True  # the blocks of the four corner positions
    odd = empty.copy()
    odd[0, 1, 2] = odd[1, 0, 1] = odd[2, 1, 0] = True    # three blocks: one and a half 128-row tiles, crossing the image boundaries
    return dict(empty=empty, full=full, corners=corners, odd=odd, random=rng.random((B, BH, BW)) < 0.3)


PATTERNS = _patterns()


def _lists(blk, device):
    flat = blk.reshape(blk.shape[0], -1)
    ids = torch.from_numpy(np.flatnonzero(flat.reshape(-1)).astype(np.int32))
    # (a list of zero entries still needs an address)
    blocks = torch.zeros(max(ids.numel(), 1), dtype=torch.int32)
    blocks[:ids.numel()] = ids
    start = torch.from_numpy(np.concatenate([[0], np.cumsum(flat.sum(1))]).astype(np.int32))
    return blocks.to(device), start.to(device)


def _live_outputs(blk, Ho, Wo):
    """[B, Ho, Wo] bool: the output positions of the live sub-grid blocks (all four parities)."""
    return torch.from_numpy(np.kron(blk, np.ones((16, 16), bool))[:, :Ho, :Wo])


def _logical(out5):
    """planar parity-major [P, B, Ho, Wo, C / P] storage -> the NHWC tensor it holds."""
    P, nb, Ho, Wo, pc = out5.shape
    return out5.reshape(P, nb, 2, 2, Ho // 2, Wo // 2, pc).permute(1, 4, 2, 5, 3, 0, 6).reshape(nb, Ho, Wo, P * pc)


@pytest.fixture(scope="module")
def layer(cuda, shipped_mode):
    from manga_image_translator_amd import ops

    g = torch.Generator().manual_seed(3)
    with shipped_mode():
        up = ops.ConvTranspose2d(torch.randn(CIN, COUT, 3, 3, generator=g) * 0.2, torch.randn(COUT, generator=g), stride=2, padding=1,
                                 output_padding=1, act=ops.ACT_RELU, device=cuda)
    x = torch.randn(B, HI, WI, CIN, generator=g).to(cuda)
    return up, x


@pytest.mark.parametrize("layout", ["nhwc", "planar"])
@pytest.mark.parametrize("mode,nprod,tile", [(6, 0, None), (6, 0, "split128x64x16p6o"), (0, 0, None), (0, 0, "fast128x64x16w5c"), (6, 1, None)],
                         ids=["split6", "split6-bm128", "fp32mfma", "fp32mfma-bm128", "p1"])
def test_live_blocks_carry_the_dense_bits_and_nothing_else_is_written(cuda, layer, mode, nprod, tile, layout):
    from manga_image_translator_amd import lib, ops

    up, x = layer
    Ho, Wo = 2 * HI, 2 * WI
    cfg = -1
    if tile is not None:
        h, cfg = lib.load(), 0
        while h.mit_conv_gemm_config_name(cfg).decode() != tile:
            cfg += 1
    kw = dict(planes=16, parity_major=True) if layout == "planar" else {}
    shape = (16, B, Ho, Wo, COUT // 16) if layout == "planar" else (B, Ho, Wo, COUT)
    view = _logical if layout == "planar" else (lambda t: t)
    with ops.gemm_mode(mode, 0):
        dense = torch.full(shape, SENTINEL, device=cuda)
        up(x, out=dense, cfg=cfg, nprod=nprod, **kw)
        assert not (view(dense) == SENTINEL).any()
        for name, blk in PATTERNS.items():
            out = torch.full(shape, SENTINEL, device=cuda)
            up(x, out=out, cfg=cfg, nprod=nprod, live=_lists(blk, cuda), **kw)
            live = _live_outputs(blk, Ho, Wo).to(cuda)
            got, ref = view(out), view(dense)
            assert torch.equal(got[live].view(torch.int32), ref[live].view(torch.int32)), (name, "live positions differ from the dense launch")
            assert (got[~live] == SENTINEL).all(), (name, "a dead position was written")


def test_list_is_refused_on_a_tile_that_cannot_read_it(cuda):
    from manga_image_translator_amd import ops

    head = ops.ConvTranspose2d(torch.randn(16, 1, 3, 3), None, stride=2, padding=1, output_padding=1, device=cuda)  # N = 1: a gemv launch
    x = torch.randn(1, 8, 8, 16, device=cuda)
    with pytest.raises(RuntimeError, match="live-block list"):
        head(x, live=_lists(np.ones((1, 1, 1), bool), cuda))


# ---- the output convolution's live-cell map ----
OB, OH, OW, OCIN = 2, 24, 80, 16     # cells 3 x 3 per image (8 x 32; the last column is clipped at 80), 16 x 64 tiles 2 x 2 (the second row is clipped)


def _cell_patterns():
    rng = np.random.default_rng(12)
    return dict(empty=np.zeros((OB, 3, 3), np.uint8), full=np.ones((OB, 3, 3), np.uint8), random=(rng.random((OB, 3, 3)) < 0.3).astype(np.uint8) * 255)


@pytest.mark.parametrize("kernel", ["dma_parity_major", "nhwc_cout3", "nhwc_plain"])
def test_live_cells_of_the_output_convolution(cuda, kernel):
    from manga_image_translator_amd import ops

    g = torch.Generator().manual_seed(4)
    cout = 4 if kernel == "nhwc_plain" else 3
    conv = ops.ConvSmallCout(torch.randn(cout, OCIN, 7, 7, generator=g) * 0.05, torch.randn(cout, generator=g), pad_mode=ops.PAD_REFLECT,
                             act=ops.ACT_SIGMOID, device=cuda)
    x = torch.randn(OB, OH, OW, OCIN, generator=g).to(cuda)
    kw = {}
    th, tw = (8, 32) if kernel == "nhwc_plain" else (16, 64)
    if kernel == "dma_parity_major":   # [Cin / 4, B, H, W, 4] with every image stored as its four parity sub-images
        x = (x.reshape(OB, OH // 2, 2, OW // 2, 2, OCIN // 4, 4).permute(5, 0, 2, 4, 1, 3, 6).contiguous().reshape(OCIN // 4, OB, OH, OW, 4))
        kw = dict(parity_major=True)
    dense = torch.full((OB, OH, OW, cout), SENTINEL, device=cuda)
    conv(x, out=dense, **kw)
    assert not (dense == SENTINEL).any()
    for name, cells in _cell_patterns().items():
        out = torch.full((OB, OH, OW, cout), SENTINEL, device=cuda)
        conv(x, out=out, cells=torch.from_numpy(cells).to(cuda), **kw)
        px = np.kron(cells != 0, np.ones((8, 32), bool))[:, :OH, :OW]      # pixels of the non-zero cells
        tiles = np.zeros_like(px)                                          # pixels of the tiles that cover one
        for y0 in range(0, OH, th):
            for x0 in range(0, OW, tw):
                tiles[:, y0:y0 + th, x0:x0 + tw] = px[:, y0:y0 + th, x0:x0 + tw].any(axis=(1, 2), keepdims=True)
        live = torch.from_numpy(tiles).to(cuda)
        assert torch.equal(out[live].view(torch.int32), dense[live].view(torch.int32)), (name, "live tiles differ from the dense launch")
        assert (out[~live] == SENTINEL).all(), (name, "a dead tile was written")
