"""Test helper: the CPU emulation of LaMa's opt-in bf16 precision (``LamaEngine.forward(precision="bf16")``) on ``oracle.lama``.

Inside ``emulated_bf16()`` every ``F.conv2d`` / ``F.conv_transpose2d`` call rounds its input and its weight to bf16 (round to nearest
even, ``tensor.to(torch.bfloat16)``) and computes in fp32 — what the one-product tiles do (MitConvGemm.nprod = 1).  The 7x7 stem and the
7x7 output convolution keep their fp32 operands, as in the engine; BatchNorm, activations, residual adds and the FFTs are untouched, and
no layer output is rounded (which is what separates the mode from torch.autocast)."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

CASES = ("mpe9_64x72", "large18_48x40", "mpe9_128x160")


def _r(t):
    return t.to(torch.bfloat16).to(torch.float32)


@contextlib.contextmanager
def emulated_bf16():
    conv2d, conv_t = F.conv2d, F.conv_transpose2d

    def c2(x, w, *a, **k):
        if w.shape[-1] == 7:            # stem and output convolution stay fp32
            return conv2d(x, w, *a, **k)
        return conv2d(_r(x), _r(w), *a, **k)

    def ct(x, w, *a, **k):
        return conv_t(_r(x), _r(w), *a, **k)

    F.conv2d, F.conv_transpose2d = c2, ct
    try:
        yield
    finally:
        F.conv2d, F.conv_transpose2d = conv2d, conv_t


def case_inputs(fx, name):
    """(n_blocks, mpe, page u8 [H,W,3], mask u8 [H,W]) of a fixture case, rebuilt from its seeds."""
    from manga_image_translator_amd import synth

    nb, mpe, seed, H, W, nbox = (int(v) for v in fx[name + "/meta"])
    page, _, mask = synth.synth_page(seed, H, W, n_boxes=nbox)
    return nb, bool(mpe), page, mask


def weights(nb, mpe):
    from manga_image_translator_amd import lama_schema, synth

    sd = synth.synth_state_dict(lama_schema.lama_generator_schema(nb))
    return sd, (synth.synth_state_dict(lama_schema.lama_mpe_schema()) if mpe else None)


def oracle_float(sd, mpe_sd, page, mask, nb):
    """``oracle.lama``'s float output [1,3,H,W] (pred inside the mask, the page outside)."""
    from oracle import lama as OL

    taps = {}
    OL.infer(sd, mpe_sd, page, mask, nb, taps)
    return taps["out_float"].numpy()


def mask01(mask):
    return (mask.astype(np.float32) / 255.0 >= 0.5)


def masked_err(x, ref, mask):
    """|x - ref| over the masked pixels of [1,3,H,W] arrays -> (mean, max)."""
    d = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(ref, dtype=np.float64))[0][:, mask01(mask)]
    return float(d.mean()), float(d.max())


def u8_levels(a, b, mask):
    """Largest difference in uint8 levels of (x * 255) truncated, over the masked pixels."""
    ua, ub = ((np.asarray(t)[0] * 255.0).astype(np.uint8).astype(np.int32) for t in (a, b))
    return int(np.abs(ua - ub)[:, mask01(mask)].max())
