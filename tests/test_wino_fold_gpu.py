"""convl2g's Winograd output transform folded into conv2's epilogue (MitConvGemm.wino_m) against the three-launch form (products ->
mit_wino43_output into a staging tensor P -> the 1x1 convolution with P as ``pre``): the same bits, at the kernel and through LamaEngine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
# (h, w), 3x3 channels, K of the 1x1, tiles to force (None = the automatic choice) per GEMM mode
CASES = {
    "10x14-k16": ((10, 14), (16, 24), 16, {6: (None,), 0: (None,)}),     # partial tiles and partial blocks
    "10x14-k48": ((10, 14), (16, 24), 48, {6: (None,), 0: (None,)}),
    "8x12-k16": ((8, 12), (16, 24), 16, {6: (None,), 0: (None,)}),       # the edge block's second tile lies past tw
    # LaMa's own 128 -> 384 and K = 192: the automatic choice (an under-filled launch: 64 x 64) and the shipped 128 x 128 tiles with
    # their wave tilings (2 x 2 waves of 64 x 64; 1 x 4 waves of 128 x 32)
    "16x22-lama": ((16, 22), (128, 384), 192, {6: (None, "split128x128x16p6u", "split128x128x16p6o"), 0: (None, "fast128x128x16w4c")}),
}


def _cfg(name):
    from manga_image_translator_amd import lib

    if name is None:
        return -1
    h, i = lib.load(), 0
    while h.mit_conv_gemm_config_name(i).decode() != name:
        i += 1
    return i


@pytest.fixture(scope="module")
def layers(cuda, shipped_mode):
    """Per case: the 3x3 (Winograd, raw), the 1x1 with BatchNorm + ReLU, their inputs, a residual, and V / M / P of the 3x3."""
    from manga_image_translator_amd import ops

    out = {}
    g = torch.Generator().manual_seed(22)
    with shipped_mode():
        for name, ((h, w), (c_in, c_out), K, tiles) in CASES.items():
            l2g = ops.WinogradConv3x3(torch.randn(c_out, c_in, 3, 3, generator=g) * (2.0 / (3 * c_in ** 0.5)), None, pad_mode=ops.PAD_REFLECT, device=cuda)
            bn = (torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g) * 0.1, torch.randn(c_out, generator=g) * 0.1,
                  torch.rand(c_out, generator=g) + 0.5, 1e-5)
            conv = ops.Conv2d(torch.randn(c_out, K, 1, 1, generator=g) * (1.0 / K ** 0.5), None, bn=bn, act=ops.ACT_RELU, device=cuda)
            x3 = torch.randn(B, h, w, c_in, generator=g).to(cuda)
            x1 = torch.randn(B, h, w, K, generator=g).to(cuda)
            post = torch.randn(B, h, w, c_out, generator=g).to(cuda)
            out[name] = (l2g, conv, x3, x1, post, tiles)
    return out


@pytest.mark.parametrize("with_post", [False, True], ids=["nopost", "post"])
@pytest.mark.parametrize("mode", [6, 0], ids=["split6", "fp32mfma"])
@pytest.mark.parametrize("case", list(CASES))
def test_folded_launch_has_the_bits_of_the_three_launch_form(cuda, layers, case, mode, with_post):
    from manga_image_translator_amd import ops

    l2g, conv, x3, x1, post, tiles = layers[case]
    _, h, w, c_out = post.shape
    T = ops.WinogradConv3x3.tiles(B, h, w)
    res = post if with_post else None
    with ops.gemm_mode(mode, 0):
        V = l2g.transform_input(x3, torch.empty(36, T, x3.shape[3], device=cuda))
        M = torch.empty(36, T, c_out, device=cuda)
        P = l2g.gemm_output(V, M, torch.empty(B, h, w, c_out, device=cuda))
        plain = conv(x1, post=res)
        assert P.abs().max() > 0.1 and not torch.equal(conv(x1, pre=P, post=res), plain)      # the operand matters
        for tile in tiles[mode]:
            want = conv(x1, pre=P, post=res, cfg=_cfg(tile))
            got = torch.full((B, h, w, c_out), float("nan"), device=cuda)
            conv(x1, out=got, wino_pre=M, post=res, cfg=_cfg(tile))
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (tile, "folded launch differs from pre = P")


def test_fold_is_refused_on_a_launch_that_cannot_take_it(cuda):
    from manga_image_translator_amd import ops

    conv = ops.Conv2d(torch.randn(24, 16, 3, 3), None, padding=1, device=cuda)   # nine taps
    x = torch.randn(1, 8, 8, 16, device=cuda)
    with pytest.raises(RuntimeError, match="one tap"):
        conv(x, wino_pre=torch.zeros(36, 4, 24, device=cuda))


# ---- LamaEngine ----
PAGES = ((64, 88), (72, 104))
ENGINES = {"1block-mpe": (1, True), "2blocks-mpe": (2, True), "1block-large": (1, False)}   # lama_large: no position encoding


@pytest.fixture(scope="module")
def engines(cuda, shipped_mode):
    from manga_image_translator_amd import lama, lama_schema, synth

    out = {}
    mpe_sd = synth.synth_state_dict(lama_schema.lama_mpe_schema(), seed=0)
    with shipped_mode():
        for name, (nb, mpe) in ENGINES.items():
            sd = synth.synth_state_dict(lama_schema.lama_generator_schema(nb), seed=nb)
            out[name] = (lama.LamaEngine(sd, mpe_sd if mpe else None, n_blocks=nb, device=cuda),
                         lama.LamaEngine(sd, mpe_sd if mpe else None, n_blocks=nb, device=cuda, fold_l2g=False))
    return out


@pytest.mark.parametrize("mode", [6, 0], ids=["split6", "fp32mfma"])
@pytest.mark.parametrize("page", PAGES, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("name", list(ENGINES))
def test_engine_output_does_not_depend_on_the_fold(cuda, engines, name, page, mode):
    from manga_image_translator_amd import ops

    folded, plain = engines[name]
    assert folded.fold_l2g and not plain.fold_l2g
    H, W = page
    rng = np.random.default_rng(H)
    img = torch.from_numpy(rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)).to(cuda)
    mask = np.zeros((B, H, W), np.uint8)
    mask[0, 10:40, 20:70] = 255
    mask[1, H - 9:, :30] = 255
    mask[1, 5:20, W - 12:] = 200
    mask = torch.from_numpy(mask).to(cuda)
    with ops.gemm_mode(mode, 0):
        for composite in (True, False):
            want = plain.forward(img, mask, composite=composite)
            got = folded.forward(img, mask, composite=composite)
            assert torch.equal(got, want), ("composite" if composite else "prediction", "bytes differ")
    assert "ffc_P" not in {k[0] for k in folded._ws._slabs}, "the folded engine allocated the staging tensor"
