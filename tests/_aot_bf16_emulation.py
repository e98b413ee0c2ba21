"""Test helper: the CPU emulation of the AOT inpainter's opt-in bf16 precision (``AotEngine.forward(precision="bf16")``) on
``tests/_aot_oracle.py``, and the cases of tests/golden/aot_bf16.npz (scripts/make_golden_aot_bf16.py).

Inside ``emulated_bf16()`` every ``F.conv2d`` / ``F.conv_transpose2d`` call rounds its input and its weight to bf16 (round to nearest
even, ``tensor.to(torch.bfloat16)``) and computes in the tensors' own type — what ``mit_aot_conv3x3_bf16`` and the one-product tiles
(MitConvGemm.nprod = 1) do.  head.0 (4 input channels) and tail.8 (3 output channels a half) keep their operands, as in the engine; weight
standardisation, gating, the plane statistics and the blend are untouched, and no layer output is rounded (which is what separates
the mode from torch.autocast)."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import _aot_oracle as O

CASES = tuple(tag for tag, *_ in O.GEN_CASES)


def _r(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _stays(x, w, transposed):
    return (not transposed) and (x.shape[1] == 4 or w.shape[0] == 3)      # head.0 / tail.8


@contextlib.contextmanager
def emulated_bf16():
    conv2d, conv_t = F.conv2d, F.conv_transpose2d

    def c2(x, w, *a, **k):
        if _stays(x, w, False):
            return conv2d(x, w, *a, **k)
        return conv2d(_r(x), _r(w), *a, **k)

    def ct(x, w, *a, **k):
        return conv_t(_r(x), _r(w), *a, **k)

    F.conv2d, F.conv_transpose2d = c2, ct
    try:
        yield
    finally:
        F.conv2d, F.conv_transpose2d = conv2d, conv_t


def quarter_mask(H, W):
    """A rectangular hole of a quarter of the page, centred; one pixel at 127 (below the 0.5 threshold of the network's mask, at the
    composite's ``>= 127``)."""
    m = np.zeros((H, W), np.uint8)
    m[H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 255
    m[3, 5] = 127
    return m


def case_inputs(fx, name):
    """(page u8 [H,W,3], mask u8 [H,W]) of a fixture case, rebuilt from its seed and size."""
    from manga_image_translator_amd import synth

    seed, H, W = (int(v) for v in fx[name + "/meta"])
    page, _, _ = synth.synth_page(seed, H, W, n_boxes=3)
    return page, quarter_mask(H, W)


def oracle_preclip(sd, page, mask, dtype=torch.float32):
    """The oracle's output before the clip, [1,3,H,W] numpy in ``dtype`` (float64: the truth of the accuracy tests)."""
    img, m = O.prep(page, mask)
    if dtype != torch.float32:
        sd = {k: v.to(dtype) for k, v in sd.items()}
        img, m = img.to(dtype), m.to(dtype)
    taps = {}
    O.generator(sd, img, m, taps)
    return taps["preclip"].numpy()


def mean_max(x, ref):
    d = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    return float(d.mean()), float(d.max())
