"""LamaEngine's masked decoder tail (masked_tail=True: the up-convolutions and the output convolution run only where the composite takes
the prediction) against the dense tail (masked_tail=False): the same bytes, whatever the dead positions of the workspace hold."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W = 2, 64, 96


def _masks():
    zero = np.zeros((H, W), np.uint8)
    full = np.full((H, W), 255, np.uint8)
    px127 = zero.copy()
    px127[29, 50] = 127          # blend weight 0, yet the byte comes from the prediction
    corner128 = zero.copy()
    corner128[H - 1, W - 1] = 128
    rects = zero.copy()
    rects[0:9, 0:30] = 255       # top-left corner
    rects[20:41, W - 7:W] = 255  # right border
    rects[H - 3:H, 40:70] = 255  # bottom border
    rects[30:34, 10:13] = 200
    rects[45:50, 60:62] = 126    # below the threshold: not needed
    # two pages per call: the case and another one, so that the lists cross an image boundary in both orders
    return dict(zero=(zero, zero), full=(full, rects), px127=(px127, zero), corner128=(rects, corner128), rects=(rects, rects[::-1, ::-1].copy()))


MASKS = _masks()


@pytest.fixture(scope="module")
def engines(cuda, shipped_mode):
    from manga_image_translator_amd import lama, lama_schema, synth

    sd = synth.synth_state_dict(lama_schema.lama_generator_schema(1), seed=0)
    mpe_sd = synth.synth_state_dict(lama_schema.lama_mpe_schema(), seed=0)
    with shipped_mode():
        masked = lama.LamaEngine(sd, mpe_sd, n_blocks=1, device=cuda)
        dense = lama.LamaEngine(sd, mpe_sd, n_blocks=1, device=cuda, masked_tail=False)
    assert masked.masked_tail and not dense.masked_tail
    img = torch.from_numpy(np.random.default_rng(2).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)).to(cuda)
    return masked, dense, img


def _mask(name, cuda):
    return torch.from_numpy(np.stack(MASKS[name])).to(cuda)


@pytest.mark.parametrize("name", list(MASKS))
@pytest.mark.parametrize("mode,precision", [(6, "fp32"), (6, "bf16"), (0, "fp32")], ids=["split6-fp32", "split6-bf16", "fp32mfma"])
def test_masked_tail_returns_the_dense_tails_bytes(cuda, engines, mode, precision, name):
    from manga_image_translator_amd import ops

    masked, dense, img = engines
    msk = _mask(name, cuda)
    with ops.gemm_mode(mode, 0):
        want = dense.forward(img, msk, precision=precision)
        got = masked.forward(img, msk, precision=precision)
        assert torch.equal(got, want)
        # composite=False shows the prediction everywhere: the dense path must be taken
        assert torch.equal(masked.forward(img, msk, composite=False, precision=precision), dense.forward(img, msk, composite=False, precision=precision))


@pytest.mark.parametrize("name", ["px127", "rects", "zero"])
def test_nothing_dead_reaches_a_byte(cuda, engines, name):
    """The workspace tensors of the tail filled with NaN before a masked call: dead positions keep the poison (or stale encoder values),
    and the page is still the dense engine's."""
    masked, dense, img = engines
    msk = _mask(name, cuda)
    want = dense.forward(img, msk)
    for buf, shape in (("d1", (B, H // 2, W // 2, 128)), ("d2", (B, H // 4, W // 4, 256)), ("full64", (B, H, W, 64)), ("pred", (B, H, W, 3))):
        masked._buf(buf, *shape).fill_(float("nan"))
    got = masked.forward(img, msk)
    assert torch.equal(got, want)
    if name != "zero":   # the call really left dead positions alone: the poison is still in the prediction buffer
        assert torch.isnan(masked._buf("pred", B, H, W, 3)).any()
    taps = {}
    assert torch.equal(masked.forward(img, msk, taps=taps), want) and not torch.isnan(taps["pred"]).any()  # with taps the tail is dense
