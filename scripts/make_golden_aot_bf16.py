#!/usr/bin/env python3
"""Writes tests/golden/aot_bf16.npz: the reference AOTGenerator's own fp32 output and its output under
torch.autocast("cpu", dtype=torch.bfloat16), both before the final clip — the yardstick of the AOT engine's opt-in bf16 precision
(tests/test_aot_bf16_gpu.py, tests/test_aot_precision.py).  Needs the reference package (CPU box only); seeded weights from ``synth``
as in the other goldens.

Per case ``<name>/meta`` = (page seed, H, W) — the page is rebuilt from the seed by ``synth.synth_page`` and the mask is
``_aot_bf16_emulation.quarter_mask`` —, ``<name>/fp32`` and ``<name>/autocast``: float32 [1,3,H,W], the generator's value range
[-1, 1] before ``torch.clip`` (inpainting_aot.py:266-274)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _aot_bf16_emulation as E  # noqa: E402
import _aot_oracle as O  # noqa: E402
from manga_image_translator_amd import synth  # noqa: E402


def run(m, page, mask, autocast):
    img, mk = O.prep(page, mask)                                                     # inpainting_lama_mpe.py:82-91,99
    with torch.no_grad():
        if autocast:                                                                 # :97-107 with the CPU as the device
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out = m.tail(m.body_conv(m.head(torch.cat([mk, img], dim=1))))       # AOTGenerator.forward without its clip
        else:
            out = m.tail(m.body_conv(m.head(torch.cat([mk, img], dim=1))))
    return out.to(torch.float32).numpy()


def main():
    sd = O.weights()
    m = O.ref_generator(sd)
    out = {}
    for tag, H, W, seed in O.GEN_CASES:
        page, _, _ = synth.synth_page(seed, H, W, n_boxes=3)
        mask = E.quarter_mask(H, W)
        f32, ac = run(m, page, mask, False), run(m, page, mask, True)
        truth = E.oracle_preclip(sd, page, mask, torch.float64)
        with E.emulated_bf16():
            emu = E.oracle_preclip(sd, page, mask)
        print(f"{tag} ({H}x{W}): against the float64 oracle — autocast mean %.3e max %.3e | emulation mean %.3e max %.3e | fp32 mean %.3e"
              % (*E.mean_max(ac, truth), *E.mean_max(emu, truth), E.mean_max(f32, truth)[0]))
        out[tag + "/meta"] = np.array([seed, H, W], dtype=np.int32)
        out[tag + "/fp32"], out[tag + "/autocast"] = f32, ac
    path = os.path.join(O.GOLDEN, "aot_bf16.npz")
    np.savez_compressed(path, source="manga_translator/inpainting/inpainting_aot.py:240-274 under inpainting_lama_mpe.py:97-107", **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
