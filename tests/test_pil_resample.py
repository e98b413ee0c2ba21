"""Pillow's 8-bit resize restated (imgproc.pil_coeffs / pil_resize_u8_host) against the REAL Pillow, byte for byte, and the size
arithmetic of the upscaler's pass loop (esrgan.upscale_plan) against the reference's ``CommonUpscaler.upscale``.

No tolerance anywhere: the restatement is integer arithmetic on coefficients computed the way the library computes them."""
import asyncio
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
from PIL import Image

from manga_image_translator_amd import esrgan, imgproc

# source (H, W) -> destination (H, W)
SIZES = [((64, 96), (32, 48)), ((61, 97), (46, 73)), ((40, 52), (10, 13)), ((17, 23), (51, 40)), ((33, 20), (33, 7)), ((8, 8), (1, 1)),
         ((128, 36), (37, 36)), ((5, 300), (9, 101))]
FILTERS = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}
CASES = [(s, d, c, f) for s, d in SIZES for c in (1, 3) for f in FILTERS]


def planted(seed: int, h: int, w: int, c: int) -> np.ndarray:
    """Random bytes with runs of 0 and 255 next to each other, so that BICUBIC's overshoot reaches both clamps."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    a[: max(1, h // 3), : max(1, w // 2)] = 0
    a[: max(1, h // 3), max(1, w // 2):] = 255
    a[h // 2:, w // 3: w // 3 + 3] = 255
    a[h // 2:, w // 3 + 3: w // 3 + 6] = 0
    return a


def pillow(a: np.ndarray, w: int, h: int, f: str) -> np.ndarray:
    return np.asarray(Image.fromarray(a[..., 0] if a.ndim == 3 and a.shape[2] == 1 else a).resize((w, h), resample=FILTERS[f]))


@pytest.mark.parametrize("src,dst,c,f", CASES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}-c{c}-{f}" for s, d, c, f in CASES])
def test_host_form_equals_pillow(src, dst, c, f):
    a = planted(src[0] * 131 + src[1], src[0], src[1], c)
    arr = a[..., 0] if c == 1 else a
    want = pillow(a, dst[1], dst[0], f)
    got = imgproc.pil_resize_u8_host(arr, (dst[1], dst[0]), f)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    if f == "bicubic" and min(src) >= 17:
        assert want.min() == 0 and want.max() == 255


def test_host_form_accepts_pillow_enum_and_leaves_input_alone():
    a = planted(3, 20, 30, 3)
    keep = a.copy()
    got = imgproc.pil_resize_u8_host(a, (11, 20), Image.Resampling.BICUBIC)
    assert np.array_equal(got, pillow(a, 11, 20, "bicubic")) and np.array_equal(a, keep)
    same = imgproc.pil_resize_u8_host(a, (30, 20), "bilinear")
    assert np.array_equal(same, a) and same is not a


@pytest.mark.parametrize("n_in,n_out", [(96, 48), (97, 73), (52, 13), (23, 40), (17, 51), (8, 1), (300, 101), (5, 9), (5760, 2880)])
@pytest.mark.parametrize("f", list(FILTERS))
def test_coefficient_tables(n_in, n_out, f):
    coef, bounds = imgproc.pil_coeffs(n_in, n_out, f)
    support = {"bilinear": 1.0, "bicubic": 2.0}[f] * max(n_in / n_out, 1.0)
    ksize = int(np.ceil(support)) * 2 + 1
    assert coef.dtype == np.int32 and bounds.dtype == np.int32 and coef.shape == (n_out, ksize) and bounds.shape == (n_out, 2)
    xmin, cnt = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (xmin >= 0).all() and (cnt >= 1).all() and (cnt <= ksize).all() and (xmin + cnt <= n_in).all()
    assert (np.abs(coef.astype(np.int64).sum(1) - (1 << 22)) <= cnt).all()       # each of the cnt roundings moves the sum by < 1
    assert all((coef[i, cnt[i]:] == 0).all() for i in range(n_out))
    # the sums stay inside int32 for any bytes: 2^21 + 255 * (sum of the positive / of the negative coefficients)
    pos = np.where(coef > 0, coef, 0).astype(np.int64).sum(1)
    neg = np.where(coef < 0, coef, 0).astype(np.int64).sum(1)
    assert (1 << 21) + 255 * pos.max() < 2 ** 31 and (1 << 21) + 255 * neg.min() >= -2 ** 31


def test_value_errors():
    a = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8_host(a, (4, 4), "lanczos")
    with pytest.raises(ValueError):
        imgproc.pil_coeffs(8, 4, "nearest")
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8_host(a.astype(np.float32), (4, 4), "bilinear")
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8_host(np.zeros((2, 8, 8, 3), np.uint8), (4, 4), "bilinear")
    import torch

    t = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8(t, (4, 4), "lanczos")
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8(t.float(), (4, 4), "bilinear")
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8(t[0], (4, 4), "bilinear")


# ---- the pass loop of CommonUpscaler.upscale as size arithmetic ---------------------------------------------------------------------
PAGE_H, PAGE_W = 37, 51
# hand-computed from upscaling/common.py:17-33 with valid ratios [2, 3, 4] and _infer's size int(round(4 side * ratio / 4)):
#   2: one pass by 2.  5: 4 (1 left), then 2 (-1 left) -> correction by (2 - 1) / 2 = 0.5, truncated.  8: 4 (4 left), then 4.
EXPECTED = {
    2: ([(2, (102, 74))], None),
    5: ([(4, (204, 148)), (2, (408, 296))], (204, 148)),
    8: ([(4, (204, 148)), (4, (816, 592))], None),
}


@pytest.mark.parametrize("ratio", sorted(EXPECTED))
def test_upscale_plan_hand_computed(ratio):
    assert esrgan.upscale_plan(PAGE_W, PAGE_H, ratio) == EXPECTED[ratio]


def test_upscale_plan_ratio_one_and_fraction():
    assert esrgan.upscale_plan(PAGE_W, PAGE_H, 1) == ([], None)
    # 1.5: one pass by 2 (-0.5 left) -> correction by 0.75: int(102 * 0.75) = 76, int(74 * 0.75) = 55
    assert esrgan.upscale_plan(PAGE_W, PAGE_H, 1.5) == ([(2, (102, 74))], (76, 55))


def _reference_common_upscaler():
    """The reference's own ``CommonUpscaler`` (upscaling/common.py), loaded by path through the oracle's reference-import harness with
    plain stand-ins for the two base classes it imports; None where the reference tree is absent."""
    from oracle import ref_import as R

    if not R.available():
        return None
    import logging

    R._prepare()
    R._pkg("manga_translator.upscaling")
    utils = types.ModuleType("manga_translator.utils")
    utils.InfererModule = type("InfererModule", (), {"logger": logging.getLogger("ref-upscaler")})
    utils.ModelWrapper = type("ModelWrapper", (), {})
    saved = sys.modules.get("manga_translator.utils")
    sys.modules["manga_translator.utils"] = utils
    try:
        spec = importlib.util.spec_from_file_location("manga_translator.upscaling._common_by_path", os.path.join(R.PKG, "upscaling", "common.py"))
        mod = importlib.util.module_from_spec(spec)
        mod.__package__ = "manga_translator.upscaling"
        spec.loader.exec_module(mod)
    finally:
        if saved is not None:
            sys.modules["manga_translator.utils"] = saved
        else:
            del sys.modules["manga_translator.utils"]
    return mod.CommonUpscaler


@pytest.mark.parametrize("ratio", [2, 3, 4, 5, 6, 8])
def test_upscale_plan_equals_reference_loop(ratio):
    Common = _reference_common_upscaler()
    if Common is None:
        pytest.skip("reference tree not present")
    trace = []

    class Stub(Common):
        _VALID_UPSCALE_RATIOS = [2, 3, 4]

        async def _upscale(self, image_batch, upscale_ratio):   # the size ESRGANUpscalerPytorch._infer returns (esrgan_pytorch.py:539,546)
            r = upscale_ratio / 4
            out = [im.resize((int(round(4 * im.size[0] * r)), int(round(4 * im.size[1] * r))), resample=Image.Resampling.BILINEAR)
                   for im in image_batch]
            trace.append((upscale_ratio, out[0].size))
            return out

    page = Image.fromarray(planted(1, PAGE_H, PAGE_W, 3))
    res = asyncio.new_event_loop().run_until_complete(Stub().upscale([page], ratio))
    passes, correction = esrgan.upscale_plan(PAGE_W, PAGE_H, ratio)
    assert passes == trace
    assert res[0].size == (correction if correction is not None else passes[-1][1])
    assert (correction is not None) == (res[0].size != trace[-1][1])
