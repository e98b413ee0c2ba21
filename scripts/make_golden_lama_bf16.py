#!/usr/bin/env python3
"""Writes tests/golden/lama_bf16.npz: the reference LaMa module's own fp32 output and its output under
torch.autocast("cpu", dtype=torch.bfloat16) — the yardstick of the engine's opt-in bf16 precision (tests/test_lama_bf16_gpu.py,
tests/test_lama_precision.py).  Needs the reference package (CPU box only); seeded weights from ``synth`` as in the other goldens.

Per case ``<name>/meta`` = (n_blocks, mpe, page seed, H, W, n_boxes) — the page and mask are rebuilt from the seed by
``synth.synth_page`` —, ``<name>/fp32`` and ``<name>/autocast``: float32 [1,3,H,W] (LamaFourier.__call__: the prediction inside the
mask, the masked page outside)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from manga_image_translator_amd import synth  # noqa: E402
from oracle.make_golden import GOLDEN, build_ref_lama  # noqa: E402

CASES = (("mpe9_64x72", 9, True, 3, 64, 72, 4), ("large18_48x40", 18, False, 4, 48, 40, 4), ("mpe9_128x160", 9, True, 5, 128, 160, 4))


def run(m, page, mask, autocast):
    img_t = torch.from_numpy(page).permute(2, 0, 1).unsqueeze(0).float() / 255.0     # inpainting_lama_mpe.py:82-92
    mask_t = torch.from_numpy(mask).unsqueeze(0).unsqueeze(0).float() / 255.0
    mask_t[mask_t < 0.5] = 0
    mask_t[mask_t >= 0.5] = 1
    with torch.no_grad():
        img_t = img_t * (1 - mask_t)
        if autocast:                                                                 # :97-107 with the CPU as the device
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out = m(img_t, mask_t)
        else:
            out = m(img_t, mask_t)
    return out.to(torch.float32).numpy()


def main():
    out = {}
    for name, nb, mpe, seed, H, W, nbox in CASES:
        m, _, _ = build_ref_lama(nb, mpe)
        page, _, mask = synth.synth_page(seed, H, W, n_boxes=nbox)
        f32, ac = run(m, page, mask, False), run(m, page, mask, True)
        inm = (mask.astype(np.float32) / 255.0 >= 0.5)
        d = np.abs(ac.astype(np.float64) - f32)[0][:, inm]
        print(f"{name}: {int(inm.sum())} masked pixels, autocast vs fp32 mean {d.mean():.3e} max {d.max():.3e}")
        out[name + "/meta"] = np.array([nb, int(mpe), seed, H, W, nbox], dtype=np.int32)
        out[name + "/fp32"], out[name + "/autocast"] = f32, ac
    path = os.path.join(GOLDEN, "lama_bf16.npz")
    np.savez_compressed(path, source="manga_translator/inpainting/inpainting_lama_mpe.py:97-107,713-726", **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
