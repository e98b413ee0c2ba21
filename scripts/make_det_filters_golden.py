"""Generate tests/golden/det_filters.npz: what the reference's OWN ``CommonDetector.detect`` (detection/common.py:12-64) returns around
a deterministic stand-in for the network.

    python scripts/make_det_filters_golden.py        # needs the reference checkout (oracle/ref_import.py); no GPU

``detection/common.py`` is loaded by path under a private package name, with a stub ``utils`` module that carries the reference's
own ``Quadrilateral`` (``ref_import.generic()``), ``cv2 = ref_import.cv2_shim()`` (``bitwise_not``, the fixed-point ``COLOR_BGR2GRAY``
and an INTER_LINEAR resize that is the identity at equal size) and a ``logger`` on the class.  The stand-in ``_detect`` records the
page it is given and returns masks derived from that page and a fixed list of quads in the filtered frame, so every byte of the
filtered page and every decision of the filter removal shows in the result.

Pages are seeded (``page``), so the fixture holds expected outputs only — and, to stay small, the SHA-256 of each image-sized result
with its shape instead of its bytes; the points of the lines are stored whole.  tests/test_det_filters.py imports ``CASES``, ``page``,
``quads_for`` and ``StubNet`` from here, and regenerates every case with ``reference_detect`` where the reference is present.
"""
from __future__ import annotations

import asyncio
import hashlib
import importlib.util
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "det_filters.npz")

PAGES = [(96, 160), (300, 520), (399, 640), (400, 400), (450, 410)]   # (h, w): three get the border, 400 x 400 does not (strict <)
FLAGS = [(r, i, g) for r in (False, True) for i in (False, True) for g in (False, True)]   # rotate, invert, gamma_correct
AUTO = ["v", "h", "none"]   # the auto-rotate outcomes: majority 'v' (no re-run), majority 'h' (re-run), no lines (re-run)
DETECT_ARGS = (1536, 0.3, 0.6, 1.5)   # detect_size, text_threshold, box_threshold, unclip_ratio: passed through untouched

# (name, h, w, rotate, invert, gamma_correct, auto_rotate, lines): every case of the fixture
CASES = [(f"p{h}x{w}_r{int(r)}i{int(i)}g{int(g)}", h, w, r, i, g, False, "mixed") for h, w in PAGES for r, i, g in FLAGS]
CASES += [(f"auto_{kind}_p{h}x{w}_r{int(r)}", h, w, r, True, True, True, kind) for kind in AUTO for (h, w), r in (((96, 160), False), ((450, 410), True))]


def page(h: int, w: int) -> np.ndarray:
    """The seeded page u8 [h,w,3]: noise over a gradient, so that rows, columns and channels all differ."""
    rng = np.random.default_rng(h * 10007 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + 2 * yy) % 256)], axis=-1)
    return ((base + rng.integers(0, 64, (h, w, 3))) % 256).astype(np.uint8)


def _box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.int64)


def quads_for(fh: int, fw: int, kind: str):
    """The stand-in detector's lines (points, prob) in a filtered frame of fh x fw.  "mixed": a horizontal and a vertical box, one of
    area 1 (dropped by ``area > 1``), one in the far corner (inside the border of a small page: dropped or clipped by
    ``_remove_border``), one across the middle, a slanted one and one at the right of the top rows (right of a small page but not below
    it: kept, its abscissae clipped to the page width); "v" / "h": a majority of vertical / horizontal boxes; "none": no line."""
    if kind == "none":
        return []
    hbox, vbox = _box(10, 12, 70, 30), _box(20, 40, 36, 92)
    if kind == "h":
        return [(hbox, 0.9), (_box(8, 50, 90, 70), 0.8), (vbox, 0.7)]
    if kind == "v":
        return [(vbox, 0.9), (_box(50, 8, 64, 80), 0.8), (hbox, 0.7)]
    return [(hbox, 0.9), (vbox, 0.8), (_box(5, 5, 6, 6), 0.7), (_box(fw - 30, fh - 20, fw - 5, fh - 5), 0.6),
            (_box(fw // 2, fh // 2, fw // 2 + 80, fh // 2 + 24), 0.5),
            (np.array([[30, 60], [80, 70], [76, 90], [26, 80]], dtype=np.int64), 0.4), (_box(fw - 120, 20, fw - 40, 44), 0.3)]


class StubNet:
    """The stand-in for ``_detect`` / ``infer``: records the pages it is given; raw_mask = channel 0 ^ 0x5a, mask = channel 1 ^ 0xa5
    (None when ``with_mask`` is off, as the DBNet plugins return), lines = ``quads_for`` built with ``quad_cls``."""

    def __init__(self, quad_cls, kind: str, with_mask: bool):
        self.quad_cls, self.kind, self.with_mask, self.pages, self.args = quad_cls, kind, with_mask, [], []

    def __call__(self, image, *args):
        image = np.asarray(image)
        self.pages.append(image.copy())
        self.args.append(args)
        fh, fw = image.shape[:2]
        lines = [self.quad_cls(pts.copy(), "", prob) for pts, prob in quads_for(fh, fw, self.kind)]
        raw = np.ascontiguousarray(image[..., 0] ^ 0x5A)
        mask = np.ascontiguousarray(image[..., 1] ^ 0xA5) if self.with_mask else None
        return lines, raw, mask


def with_mask(h: int, w: int, rotate: bool, invert: bool) -> bool:
    """Which cases return a second mask: about half of them, spread over pages and flags."""
    return (h + int(rotate) + int(invert)) % 2 == 0


def digest(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def pack(name: str, out: dict, net: StubNet, textlines, raw_mask, mask) -> None:
    """One case's results under ``name/...``: the pages the network was given, the lines' points and probabilities, both masks."""
    out[f"{name}/n_pages"] = np.array(len(net.pages))
    for k, p in enumerate(net.pages):
        out[f"{name}/page{k}_shape"], out[f"{name}/page{k}_sha"] = np.array(p.shape), digest(p)
    out[f"{name}/pts"] = np.array([np.asarray(t.pts) for t in textlines], dtype=np.int64).reshape(-1, 4, 2)
    out[f"{name}/prob"] = np.array([t.prob for t in textlines], dtype=np.float64)
    out[f"{name}/raw_shape"], out[f"{name}/raw_sha"] = np.array(raw_mask.shape), digest(raw_mask)
    out[f"{name}/has_mask"] = np.array(mask is not None)
    if mask is not None:
        out[f"{name}/mask_shape"], out[f"{name}/mask_sha"] = np.array(mask.shape), digest(mask)


def reference_detector():
    """-> (an instance of the reference's CommonDetector with ``_detect`` left to set, the reference's Quadrilateral)."""
    sys.path.insert(0, ROOT)
    from oracle import ref_import

    G = ref_import.generic()
    shp = ref_import.shapely_shim()
    G.Polygon, G.MultiPoint = shp.Polygon, shp.MultiPoint
    for name in ("_ref_det", "_ref_det.detection"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    utils = types.ModuleType("_ref_det.utils")
    utils.InfererModule, utils.ModelWrapper, utils.Quadrilateral = type("InfererModule", (), {}), type("ModelWrapper", (), {}), G.Quadrilateral
    sys.modules["_ref_det.utils"] = utils
    spec = importlib.util.spec_from_file_location("_ref_det.detection.common", os.path.join(ref_import.PKG, "detection", "common.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["_ref_det.detection.common"] = mod
    spec.loader.exec_module(mod)
    mod.cv2 = ref_import.cv2_shim()

    class Detector(mod.CommonDetector):
        logger = logging.getLogger("det_filters_golden")
        net = None

        async def _detect(self, image, *args):
            return self.net(image, *args)

    return Detector(), G.Quadrilateral


def reference_detect(det, quad_cls, case):
    """Run one case through the reference's detect -> (net, textlines, raw_mask, mask)."""
    name, h, w, rotate, invert, gamma, auto, kind = case
    det.net = StubNet(quad_cls, kind, with_mask(h, w, rotate, invert))
    with np.errstate(all="ignore"):
        res = asyncio.run(det.detect(page(h, w), *DETECT_ARGS, invert, gamma, rotate, auto))
    return (det.net,) + tuple(res)


def main():
    det, quad_cls = reference_detector()
    out = {}
    for case in CASES:
        pack(case[0], out, *reference_detect(det, quad_cls, case))
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(CASES)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
