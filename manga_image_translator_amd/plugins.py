"""Drop-in detector / OCR / inpainter plugins: the reference's plugin interface over the gfx950 engine.

Each class honours the contract of its reference counterpart:

  HipComicTextDetector   <- ComicTextDetector   (/root/reference/manga_translator/detection/ctd.py:60-179)
  HipDefaultDetector     <- DefaultDetector     (detection/default.py:27-103)
  HipDBConvNextDetector  <- DBConvNextDetector  (detection/dbnet_convnext.py:512-588)
  HipModel48pxOCR        <- Model48pxOCR        (ocr/model_48px.py:25-180)
  HipModel48pxCTCOCR     <- Model48pxCTCOCR     (ocr/model_48px_ctc.py:30-160)
  HipModel32pxOCR        <- Model32pxOCR        (ocr/model_32px.py:19-140)
  HipLamaMPEInpainter    <- LamaMPEInpainter    (inpainting/inpainting_lama_mpe.py:26-118)
  HipLamaLargeInpainter  <- LamaLargeInpainter  (inpainting/inpainting_lama_mpe.py:121-136)
  HipAotInpainter        <- AotInpainter        (inpainting/inpainting_aot.py:11-33), the reference's ``Inpainter.default``
  HipESRGANUpscaler      <- ESRGANUpscalerPytorch (upscaling/esrgan_pytorch.py:512-549)
  HipMangaColorizer      <- MangaColorizationV2 (colorization/manga_colorization_v2.py:13-74), the reference's ``Colorizer.mc2``

Same lifecycle (``__init__`` touches no GPU; ``await load(device)`` / ``unload()`` / ``infer(...)``; infer before load
raises), same ``_infer`` signatures, argument meaning and return types, errors as Python exceptions.  When the
reference package is importable the classes derive from its ``OfflineDetector`` / ``OfflineOCR`` /
``OfflineInpainter`` and ``register()`` adds them to ``DETECTORS`` / ``OCRS`` / ``INPAINTERS``;
otherwise they derive from a minimal mirror of ``ModelWrapper`` (utils/inference.py:330-350) so the contract can be
exercised stand-alone.  The detectors' box extraction (contours -> min-area boxes -> unclip) runs on the native host routines of the C-ABI library
(hostglue.py; the reference's OpenCV/pyclipper version can be injected instead); mask refinement and image resizing are
NOT part of the dense path: they are taken from the reference package when present, or injected by the caller.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import pipeline
from .textline import Quadrilateral

try:  # inside the reference's environment: be a real plugin
    from manga_translator.detection.common import OfflineDetector as _DetBase  # type: ignore
    from manga_translator.inpainting.common import OfflineInpainter as _InpBase  # type: ignore
    from manga_translator.ocr.common import OfflineOCR as _OcrBase  # type: ignore
    from manga_translator.upscaling.common import OfflineUpscaler as _UpBase  # type: ignore
    from manga_translator.colorization.common import OfflineColorizer as _ColBase  # type: ignore
    from manga_translator.utils import Quadrilateral as _RefQuadrilateral  # type: ignore

    HAVE_REFERENCE = True
except Exception:  # stand-alone: mirror the ModelWrapper lifecycle
    HAVE_REFERENCE = False
    _RefQuadrilateral = Quadrilateral

    class _Wrapper:
        """Mirror of ModelWrapper's load/unload/infer protocol (utils/inference.py:318-350)."""
        _key = "hip"

        _MODEL_SUB_DIR = ""
        _MODEL_DIR = os.environ.get("MIT_MODEL_DIR", "models")   # ModelWrapper._MODEL_DIR (utils/inference.py:94): BASE_PATH/models there

        def __init__(self, *args, **kwargs):
            self._loaded = False
            self._downloaded = self._check_downloaded()

        def is_loaded(self) -> bool:
            return self._loaded

        def is_downloaded(self) -> bool:
            return self._downloaded

        @property
        def model_dir(self) -> str:
            return os.path.join(self._MODEL_DIR, self._MODEL_SUB_DIR)

        def _get_file_path(self, *args) -> str:
            return os.path.join(self.model_dir, *args)

        def _check_downloaded(self) -> bool:
            """The files named by ``_MODEL_MAPPING`` exist under model_dir (utils/inference.py:262-293)."""
            for key, m in self._MODEL_MAPPING.items():
                names = list(m["archive"]) if "archive" in m else [m["file"] if m.get("file", ".") != "." else m["url"].rsplit("/", 1)[-1]]
                if not all(os.path.exists(self._get_file_path(n)) for n in names):
                    return False
            return True

        async def download(self, force: bool = False):
            """Stand-alone mode has no downloader (that is the reference's ModelWrapper.download): the checkpoints must already be
            in place, or the weights handed to the constructor."""
            if not self.is_downloaded():
                raise FileNotFoundError(f"{self._key}: checkpoint files {sorted(self._MODEL_MAPPING)} are not under {self.model_dir!r} "
                                        "and there is no downloader outside the reference package; pass weights= or copy the files")

        async def load(self, device: str, *args, **kwargs):
            if not self.is_downloaded():
                await self.download()
            if not self.is_loaded():
                await self._load(*args, **kwargs, device=device)
                self._loaded = True

        async def unload(self):
            if self.is_loaded():
                await self._unload()
                self._loaded = False

        async def reload(self, device: str, *args, **kwargs):
            await self.unload()
            await self.load(*args, **kwargs, device=device)

        async def infer(self, *args, **kwargs):
            if not self.is_loaded():
                raise Exception(f"{self._key}: Tried to forward pass without having loaded the model.")
            return await self._infer(*args, **kwargs)

    # the sub-directories the reference's OfflineDetector / OfflineOCR / OfflineInpainter / OfflineUpscaler keep their files in
    # (detection/common.py:138, ocr/common.py:54, inpainting/common.py:17, upscaling/common.py): a checkpoint tree laid out for the
    # reference is found by the stand-alone plugins as it is
    _DetBase = type("_DetBase", (_Wrapper,), {"_MODEL_SUB_DIR": "detection"})
    _OcrBase = type("_OcrBase", (_Wrapper,), {"_MODEL_SUB_DIR": "ocr"})
    _InpBase = type("_InpBase", (_Wrapper,), {"_MODEL_SUB_DIR": "inpainting"})
    _UpBase = type("_UpBase", (_Wrapper,), {"_MODEL_SUB_DIR": "upscaling"})
    _ColBase = type("_ColBase", (_Wrapper,), {"_MODEL_SUB_DIR": "colorization"})


_RELEASE = "https://github.com/zyddnys/manga-image-translator/releases/download/beta-0.3/"


def set_model_dir(path: str) -> None:
    """Root directory of the checkpoint files for every plugin constructed afterwards — ``ModelWrapper._MODEL_DIR`` (utils/inference.py:94),
    of the reference's class when the plugins subclass it, of the stand-alone mirror otherwise.  ``<path>/<_MODEL_SUB_DIR>/<file>`` as
    the reference lays them out."""
    if HAVE_REFERENCE:
        from manga_translator.utils.inference import ModelWrapper as base  # type: ignore
    else:
        base = _Wrapper
    base._MODEL_DIR = str(path)


def _own_quad(q) -> Quadrilateral:
    """A text line in this package's geometry type: the object itself when it already is one (the detector plugins of this package return
    them; building it again would re-sort its corners with five numpy calls, 65 us a line), else built from the reference object's points."""
    return q if type(q) is Quadrilateral else Quadrilateral(np.asarray(q.pts))


class _EnginePlugin:
    """What the plugins share around their engine.  A mixin listed before the reference's ``Offline*`` class (or its stand-alone mirror),
    whose ``__init__`` it leaves alone: a plugin's constructor calls ``_hand_over`` once the base's has run."""

    def _hand_over(self, weights, *also) -> None:
        """The constructor's tail.  State dicts injected through the constructor (``also``: what else the model needs, e.g. the OCR
        dictionary) stand for the checkpoint files: nothing is left to download, so ModelWrapper.load() (utils/inference.py:330-338)
        must not try to fetch ``_MODEL_MAPPING`` (there is no network offline)."""
        self._weights, self.engine = weights, None
        if all(g is not None for g in (weights, *also)):
            self._downloaded = True

    async def _unload(self):
        if self.engine is not None:
            self.engine.release_workspace()  # device slabs go back to the allocator before the weights do
        self.engine = None

    def _page_on_device(self, image: np.ndarray) -> torch.Tensor:
        """Host page [H,W,C] -> [1,H,W,C] on the engine's device: the page crosses PCIe once, as bytes."""
        return torch.from_numpy(np.ascontiguousarray(image)).to(self.engine.device)[None]


class _FilteredDetector(_EnginePlugin):
    """``CommonDetector.detect`` (detection/common.py:12-64) for the detector plugins, in both forms — it stands before the reference's
    ``OfflineDetector`` in the method order, so it replaces the numpy ``detect`` the plugins would inherit there, and it gives the
    stand-alone mirror the method it lacks.  The page is uploaded once and filtered on the device (``det_filters.apply``: rotate, the
    border for pages under 400 px, invert, gamma), the network and the box extraction run where the filtered page is
    (``_infer_device``), both masks are un-rotated and cropped on the device (``det_filters.undo``) and come down once.  The text lines
    go the reference's way on the host, quirks included (``det_filters``).  ``infer`` / ``_infer`` are what they were."""

    async def detect(self, image: np.ndarray, detect_size: int, text_threshold: float, box_threshold: float, unclip_ratio: float,
                     invert: bool, gamma_correct: bool, rotate: bool, auto_rotate: bool = False, verbose: bool = False):
        """-> (textlines, raw_mask, mask), the reference's signature and results."""
        from . import det_filters as DF

        if not self.is_loaded():
            raise Exception(f"{self._key}: Tried to forward pass without having loaded the model.")
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"expected uint8 RGB [H,W,3], got {image.dtype} {image.shape}")

        if torch.device(self.engine.device).type != "cuda":   # a stand-in engine that lives on the host (tests/boundary_checks.py): the
            # page never was on a device, so the numpy statements go around ``infer``, as the reference's own detect would
            return await DF.detect(self.infer, image, detect_size, text_threshold, box_threshold, unclip_ratio, invert, gamma_correct,
                                   rotate, auto_rotate, verbose)

        async def net(filtered, *args):
            return await self._infer_device(filtered[None], *args)

        textlines, raw_mask, mask = await DF.detect(net, self._page_on_device(image)[0], detect_size, text_threshold, box_threshold,
                                                    unclip_ratio, invert, gamma_correct, rotate, auto_rotate, verbose,
                                                    apply_fn=DF.apply, undo_masks_fn=DF.undo)
        down = lambda m: None if m is None else m.contiguous().cpu().numpy()   # noqa: E731
        return textlines, down(raw_mask), down(mask)

    async def _infer_device(self, page: torch.Tensor, detect_size: int, text_threshold: float, box_threshold: float,
                            unclip_ratio: float, verbose: bool = False):
        """``_infer`` for a page u8 [1,H,W,3] that is already on the device -> (textlines, raw_mask, mask), the masks device tensors.
        This form is the one for every case a plugin has no device route for (an injected host step, a webtoon strip whose stitched mask
        is finished on the host): the page goes through ``_infer`` on the host and the masks come back up."""
        textlines, raw_mask, mask = await self._infer(np.ascontiguousarray(page[0].cpu().numpy()), detect_size, text_threshold,
                                                      box_threshold, unclip_ratio, verbose)
        up = lambda m: None if m is None else torch.from_numpy(np.ascontiguousarray(m)).to(page.device)   # noqa: E731
        return textlines, up(raw_mask), up(mask)


def _gpu_device(device: str) -> torch.device:
    """The reference passes 'cpu' | 'cuda' | 'mps' | 'xpu' (ROCm = 'cuda').  This backend has no CPU path."""
    if not str(device).startswith("cuda"):
        raise RuntimeError(f"the HIP backend runs on an MI355X only: device={device!r} (use --use-gpu)")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the HIP backend has no CPU fallback")
    return torch.device(device)


def _ocr_options(config, default_threshold: float) -> Tuple[float, int]:
    """(probability threshold, ignore_bubble) of an OCR call: ``config.prob`` or the model's default, ``config.ignore_bubble`` or 0."""
    threshold = default_threshold if config is None or getattr(config, "prob", None) is None else config.prob
    ignore_bubble = int(getattr(config, "ignore_bubble", 0) or 0) if config is not None else 0
    return threshold, ignore_bubble


def _bubble_reject(ignore_bubble: int) -> Optional[Callable]:
    """``textline.is_ignore`` at this setting as a ``reject`` of ``textline.rectified_chunks`` — the host form of the rule, for callers
    that inject or wrap one (the plugins themselves pass ``ignore_bubble=`` and the test runs on the device); None where the filter is
    off (outside 1..50), so that no crop is fetched to the host for it."""
    from . import textline as TL

    return (lambda crop: TL.is_ignore(crop, ignore_bubble)) if 1 <= ignore_bubble <= 50 else None


def _accept(q, text: str, prob: float, fg, bg):
    """Write a recognised line's result on its Quadrilateral, the way every reference OCR does; returns the object."""
    q.text, q.prob = text, prob
    q.fg_r, q.fg_g, q.fg_b = fg
    q.bg_r, q.bg_g, q.bg_b = bg
    return q


class HipComicTextDetector(_FilteredDetector, _DetBase):
    """``--detector ctd`` on the HIP engine."""
    _KEY = _key = "ctd_hip"
    # the torch checkpoint of the reference's own mapping (detection/ctd.py:63-74; its ONNX twin is the reference's CPU path)
    _MODEL_MAPPING: Dict = {
        "model-cuda": {
            "url": _RELEASE + "comictextdetector.pt",
            "hash": "1f90fa60aeeb1eb82e2ac1167a66bf139a8a61b8780acd351ead55268540cccb",
            "file": ".",
        },
    }

    def __init__(self, *args, weights: Optional[Dict[str, Dict[str, torch.Tensor]]] = None,
                 boxes_from_maps: Optional[Callable] = None, refine: Optional[Callable] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self._boxes, self._refine = boxes_from_maps, refine
        self.input_size = (1024, 1024)  # ctd.py:84: fixed, whatever detect_size the caller passes
        self._hand_over(weights)

    async def _load(self, device: str, input_size=1024, **_):
        from . import ctd

        dev = _gpu_device(device)
        w = self._weights or _load_ctd_checkpoint(self)
        self.engine = ctd.CtdEngine(w["ctd.yolo"], w["ctd.seg"], w["ctd.det"], device=dev)
        self.device, self.input_size = device, (input_size, input_size)

    @torch.no_grad()
    async def _infer(self, image: np.ndarray, detect_size: int, text_threshold: float, box_threshold: float,
                     unclip_ratio: float, verbose: bool = False):
        """-> (textlines, mask_refined u8 [H,W], None).  Like the reference, ignores detect_size / thresholds /
        unclip_ratio (fixed 1024, 0.3, 0.6, 1.5: ctd.py:84,102,157)."""
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"expected uint8 RGB [H,W,3], got {image.dtype} {image.shape}")
        textlines, mask = self._detect_page(self._page_on_device(image), image)
        return textlines, mask if isinstance(mask, np.ndarray) else mask.cpu().numpy(), None

    async def _infer_device(self, page: torch.Tensor, detect_size: int, text_threshold: float, box_threshold: float,
                            unclip_ratio: float, verbose: bool = False):
        """``_infer`` on a device page [1,H,W,3]: the refined mask stays on the device (an injected ``refine=`` works on the host)."""
        textlines, mask = self._detect_page(page, None)
        return textlines, torch.from_numpy(mask).to(page.device) if isinstance(mask, np.ndarray) else mask, None

    @torch.no_grad()
    def _detect_page(self, page: torch.Tensor, image: Optional[np.ndarray]):
        """The body of ``_infer`` for the page on the device [1,H,W,3] -> (textlines, refined mask: a device tensor, or the host array
        of an injected ``refine=``).  ``image``: the same page on the host when the caller has it; the host steps that can be injected
        fetch it otherwise."""
        from . import hostglue, imgproc, rearrange

        im_h, im_w = int(page.shape[1]), int(page.shape[2])
        S = self.input_size[0]
        strip = rearrange.plan(im_h, im_w, S) is not None    # webtoon strip: det_rearrange_forward (ctd.py:137, generic.py:876-997)
        if strip and self._boxes is None and self._refine is None and torch.device(self.engine.device).type == "cuda":
            # nothing injected: bands, squares, network, stitch and postprocess_mask (:155) stay on the device (csrc/rearrange.hip); the
            # stitched maps then go the whole page's way below, so only the boxes and the final mask cross PCIe
            def net(squares):  # det_batch_forward_ctd (ctd.py:106-127): at S x S the engine's letterbox is the identity
                _, sq_lines, _ = self.engine.forward(squares)
                return sq_lines, self.engine.last_mask_f32

            lines, (_, mask_u8) = rearrange.forward_gpu(page[0], net, S, mask_u8=True)
            mask_u8, lines_map = mask_u8[0], None
        elif strip:
            image = image if image is not None else page[0].cpu().numpy()
            lines_map, mask_f = rearrange.forward(image, self._tiles_forward, S)
            mask_u8 = torch.from_numpy((mask_f.squeeze() * 255).astype(np.uint8)).to(self.engine.device)[None]  # postprocess_mask (:155)
        else:
            mask_u8, lines, _ = self.engine.forward(page)    # postprocess_mask already applied on the GPU (ctd.py:30-44)
            lines_map = None                          # [1,2,h,w] on the device, cropped to the un-padded area (:152-153)
        if self._refine is None:                         # cv2.resize(mask, (w, h), INTER_LINEAR) (:162) on the GPU as well
            mask_full = imgproc.resize_u8(mask_u8[:1].contiguous(), (im_w, im_h))[0]
        # SegDetectorRepresenter(thresh=0.3) (:102,156): on the GPU where the map already is (csrc/ctd_boxes.hip: only the boxes cross
        # PCIe); an injected extractor, or a rearranged strip whose stitched map was assembled on the host (see above), takes the numpy map
        if self._boxes is None and lines_map is None and lines.is_cuda:   # (a map that lives on the host — an injected stand-in engine,
            # tests/boundary_checks.py — goes to the host routine as well)
            boxes, scores = hostglue.ctd_boxes_gpu(lines, im_h, im_w)[0]
        else:
            boxes_fn = self._boxes or _native_ctd_boxes
            boxes, scores = boxes_fn(lines_map if lines_map is not None else lines.cpu().numpy(), im_h, im_w)
        keep = np.where(scores > 0.6)                        # box_thresh (:157-159)
        boxes, scores = boxes[keep], scores[keep]
        textlines = [_RefQuadrilateral(pts.astype(int), "", float(s)) for pts, s in zip(boxes, scores)]
        if self._refine is not None:                         # injected resize + refine_mask (e.g. the reference's OpenCV one)
            image = image if image is not None else page[0].cpu().numpy()
            return textlines, self._refine(image, mask_u8[0].cpu().numpy(), textlines, im_h, im_w)
        # refine_mask(image, mask, textlines, refine_mode=None) (:177): page and mask are already on the device (csrc/ctd_refine.hip)
        return textlines, hostglue.refine_mask_gpu(page[0], mask_full, textlines, None)


    def _tiles_forward(self, squares: np.ndarray):
        """det_batch_forward_ctd (ctd.py:106-127) for <= 4 rearranged squares: u8 [n,s,s,3] -> (lines [n,2,S,S], mask [n,1,S,S])
        float32.  Squares larger than the input size are shrunk on the GPU (square_pad_resize's INTER_LINEAR, generic.py:870-872);
        at exactly S x S the engine's letterbox is the identity, i.e. the reference's plain ``/ 255``."""
        from . import imgproc

        S = self.input_size[0]
        t = torch.from_numpy(np.ascontiguousarray(squares)).to(self.engine.device)
        if t.shape[1] != S:
            t = imgproc.resize_u8(t, (S, S))
        _, lines, _ = self.engine.forward(t)
        return lines.cpu().numpy(), self.engine.last_mask_f32.cpu().numpy()[:, None]


class HipDefaultDetector(_FilteredDetector, _DetBase):
    """``--detector default`` (DBNet on ResNet-34) on the HIP engine."""
    _KEY = _key = "default_hip"
    _MODEL_MAPPING: Dict = {  # detection/default.py:28-34
        "model": {
            "url": _RELEASE + "detect-20241225.ckpt",
            "hash": "67ce1c4ed4793860f038c71189ba9630a7756f7683b1ee5afb69ca0687dc502e",
            "file": ".",
        },
    }

    def __init__(self, *args, weights: Optional[Dict[str, torch.Tensor]] = None, preprocess: Optional[Callable] = None,
                 boxes_from_maps: Optional[Callable] = None, resize2x: Optional[Callable] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self._pre, self._boxes, self._resize2x = preprocess, boxes_from_maps, resize2x
        self._hand_over(weights)

    async def _load(self, device: str):
        from . import dbnet

        dev = _gpu_device(device)
        sd = self._weights
        if sd is None:
            sd = _bare_state_dict(torch.load(_ckpt_path(self, "detect-20241225.ckpt"), map_location="cpu"))
        self.engine = dbnet.DbnetEngine(sd, device=dev)
        self.device = device

    @torch.no_grad()
    async def _infer(self, image: np.ndarray, detect_size: int, text_threshold: float, box_threshold: float,
                     unclip_ratio: float, verbose: bool = False):
        """-> (textlines, raw_mask u8 [H,W], None) (default.py:56-103).  bilateralFilter + resize_aspect_ratio (:62) and the
        network run on the GPU, SegDetectorRepresenter (:73-77) and the x2 mask resize with its crop and cast (:89-95) as well
        (``dbnet_detect_pages``: the page function the batch engine shares); every step can still be injected (preprocess= /
        boxes_from_maps= / resize2x=) and then takes its host path: the native host extraction (csrc/hostglue.hip), the numpy
        bilinear ``_resize2x_f32``.  A webtoon strip's stitched mask takes the numpy resize as well."""
        from . import imgproc, rearrange

        boxes_fn = self._boxes or _native_dbnet_boxes
        resize2x = self._resize2x or (lambda m: _resize2x_f32(m))
        strip = rearrange.plan(image.shape[0], image.shape[1], detect_size) is not None  # webtoon strip (default.py:60, generic.py:876-997)
        if strip and self._boxes is None and self._pre is None and torch.device(self.engine.device).type == "cuda":
            # nothing injected: bands, squares, network and stitch on the device (csrc/rearrange.hip), the boxes extracted where the
            # stitched map is; the stitched float mask comes down once for the host x2 resize below
            from . import hostglue

            db, mask4 = rearrange.forward_gpu(self._page_on_device(image)[0], self.engine.forward, detect_size)
            mask = mask4[0, 0].cpu().numpy()
            h, w = image.shape[:2]
            ratio, pad_w, pad_h = 1.0, 0, 0
            boxes_fn = lambda d, hh, ww, tt, bt, ur: hostglue.dbnet_boxes_gpu(d, hh, ww, tt, bt, ur)[0]   # noqa: E731
        elif strip:
            def tiles(squares):  # det_batch_forward_default (:15-25): x / 127.5 - 1 happens inside the engine
                t = torch.from_numpy(np.ascontiguousarray(squares)).to(self.engine.device)
                if t.shape[1] != detect_size:
                    t = imgproc.resize_u8(t, (detect_size, detect_size))
                d, m = self.engine.forward(t)
                return d.cpu().numpy(), m.cpu().numpy()[:, None]

            db, mask4 = rearrange.forward(image, tiles, detect_size)
            mask = mask4[0, 0]
            h, w = image.shape[:2]
            ratio, pad_w, pad_h = 1.0, 0, 0
        else:
            if self._pre is None and self._boxes is None and self._resize2x is None and torch.device(self.engine.device).type == "cuda":
                # nothing injected: the page function the batch engine runs, for one page — only the boxes and the finished mask come down
                tls, masks = dbnet_detect_pages(self.engine, self._page_on_device(image), detect_size, text_threshold, box_threshold,
                                                unclip_ratio, micro_batch=1)
                return tls[0], masks[0].cpu().numpy(), None
            if self._pre is not None:
                img_resized, target_ratio, pad_w, pad_h = self._pre(image, detect_size)
                page = self._page_on_device(img_resized)
            else:  # cv2.bilateralFilter + resize_aspect_ratio (:62) on the device: the page crosses PCIe once, as bytes
                page, target_ratio, pad_w, pad_h = default_preprocess_gpu(self._page_on_device(image)[0], detect_size)
            ratio = 1 / target_ratio
            h, w = int(page.shape[1]), int(page.shape[2])
            db, mask = self.engine.forward(page)
            if self._boxes is None and db.is_cuda:   # SegDetectorRepresenter (:73-77) where the map is: csrc/ctd_boxes.hip
                from . import hostglue

                boxes_fn = lambda d, hh, ww, tt, bt, ur: hostglue.dbnet_boxes_gpu(d, hh, ww, tt, bt, ur)[0]   # noqa: E731
            else:
                db = db.cpu().numpy()
            mask = mask[0] if self._resize2x is None and mask.is_cuda else mask[0].cpu().numpy()
        boxes, scores = boxes_fn(db, h, w, text_threshold, box_threshold, unclip_ratio)
        textlines = _dbnet_textlines(boxes, scores, ratio)
        if torch.is_tensor(mask):     # no resize2x injected: the mask tail (:89-95) where the mask is (csrc/dbnet_tail.hip)
            mh, mw = 2 * int(mask.shape[0]), 2 * int(mask.shape[1])
            oh, ow = (mh - pad_h, mw) if pad_h > 0 else ((mh, mw - pad_w) if pad_w > 0 else (mh, mw))
            return textlines, imgproc.dbnet_mask_tail(mask, oh, ow).cpu().numpy(), None
        mask_resized = resize2x(mask)
        if pad_h > 0:
            mask_resized = mask_resized[:-pad_h, :]
        elif pad_w > 0:
            mask_resized = mask_resized[:, :-pad_w]
        return textlines, np.clip(mask_resized * 255, 0, 255).astype(np.uint8), None


    @torch.no_grad()
    async def _infer_device(self, page: torch.Tensor, detect_size: int, text_threshold: float, box_threshold: float,
                            unclip_ratio: float, verbose: bool = False):
        """``_infer`` on a device page [1,H,W,3]: with nothing injected and no webtoon strip, ``dbnet_detect_pages`` on the page where
        it is, its mask left on the device; everything else through the host form."""
        from . import rearrange

        injected = self._pre is not None or self._boxes is not None or self._resize2x is not None
        if injected or page.device.type != "cuda" or rearrange.plan(int(page.shape[1]), int(page.shape[2]), detect_size) is not None:
            return await super()._infer_device(page, detect_size, text_threshold, box_threshold, unclip_ratio, verbose)
        tls, masks = dbnet_detect_pages(self.engine, page, detect_size, text_threshold, box_threshold, unclip_ratio, micro_batch=1)
        return tls[0], masks[0], None


class HipDBConvNextDetector(HipDefaultDetector):
    """``--detector dbconvnext`` (DBNet on ConvNeXt) on the HIP engine.  ``DBConvNextDetector._infer`` (detection/dbnet_convnext.py:541-588)
    is ``DefaultDetector._infer`` line for line, so only the network behind it differs: ``_infer`` is inherited."""
    _KEY = _key = "dbconvnext_hip"
    CKPT = "dbnet_convnext.ckpt"
    _MODEL_MAPPING: Dict = {  # detection/dbnet_convnext.py:513-519: nothing to download, the file is expected beside the program
        "model": {
            "url": "",
            "hash": "",
            "file": ".",
        },
    }

    def __init__(self, *args, **kwargs):
        import shutil

        if os.path.exists(self.CKPT):                       # :522-524: a checkpoint in the working directory moves to the model directory
            os.makedirs(self.model_dir, exist_ok=True)
            shutil.move(self.CKPT, self._get_file_path(self.CKPT))
        super().__init__(*args, **kwargs)

    def _check_for_malformed_model_mapping(self):
        """The reference's mapping has an empty URL — the user supplies the file — which ModelWrapper's check (utils/inference.py:129-134)
        refuses, so the reference's own class cannot be constructed over it.  Nothing is ever downloaded for this model: nothing to check."""

    def _check_downloaded(self) -> bool:
        return os.path.exists(self._get_file_path(self.CKPT))

    async def _load(self, device: str):
        from . import dbconvnext

        dev = _gpu_device(device)
        sd = self._weights
        if sd is None:
            sd = _load_dbconvnext_checkpoint(self)
        self.engine = dbconvnext.DbconvnextEngine(sd, device=dev)
        self.device = device


class HipModel48pxOCR(_EnginePlugin, _OcrBase):
    """``--ocr 48px`` on the HIP engine."""
    _KEY = _key = "48px_hip"
    _MODEL_MAPPING: Dict = {  # ocr/model_48px.py:28-37
        "model": {
            "url": _RELEASE + "ocr_ar_48px.ckpt",
            "hash": "29daa46d080818bb4ab239a518a88338cbccff8f901bef8c9db191a7cb97671d",
        },
        "dict": {
            "url": _RELEASE + "alphabet-all-v7.txt",
            "hash": "f5722368146aa0fbcc9f4726866e4efc3203318ebb66c811d8cbbe915576538a",
        },
    }

    def __init__(self, *args, weights: Optional[Dict[str, torch.Tensor]] = None, dictionary: Optional[Sequence[str]] = None,
                 **kwargs):
        super().__init__(*args, **kwargs)
        self.dictionary = dictionary
        self._hand_over(weights, dictionary)

    async def _load(self, device: str):
        from . import ocr48

        dev = _gpu_device(device)
        if self._weights is None or self.dictionary is None:
            self._weights, self.dictionary = _load_ocr_checkpoint(self)
        self.engine = ocr48.Ocr48Engine(self._weights, len(self.dictionary), device=dev)
        self.device = device

    def _directions(self, textlines):
        """(line, direction) in processing order: the merge-graph majority vote of ocr/common.py:12-39 (the reference's own
        method when the package is present, textline.generate_text_direction otherwise)."""
        if HAVE_REFERENCE:
            return list(self._generate_text_direction(textlines))
        from . import textline as TL

        own = [_own_quad(q) for q in textlines]
        back = {id(o): q for o, q in zip(own, textlines)}
        return [(back[id(o)], d) for o, d in TL.generate_text_direction(own)]

    def _prepare(self, textlines):
        """-> (quads, dirs, own): the caller's lines in processing order, the direction of each, and the same lines in this package's
        geometry type.  Three empty lists for a page without lines."""
        pairs = self._directions(textlines)
        quads = [q for q, _ in pairs]
        return quads, [d for _, d in pairs], [_own_quad(q) for q in quads]

    @torch.no_grad()
    async def _infer(self, image: np.ndarray, textlines: List, config=None, verbose: bool = False, ignore_bubble: int = 0,
                     max_seq_length: int = 255, suppress_eos: bool = False):
        """Sets text / prob / fg_* / bg_* on the same Quadrilateral objects and returns those above the threshold,
        in the reference's sorted-by-width chunk order (model_48px.py:67-180)."""
        threshold, _ = _ocr_options(config, 0.2)
        quads, dirs, own = self._prepare(textlines)
        if not quads:
            return []
        r = self.engine.recognize_pages(self._page_on_device(image), [own], max_seq_length=max_seq_length, suppress_eos=suppress_eos,
                                        directions=[dirs])
        toks, lens = r["tokens"].cpu().numpy(), r["length"].cpu().numpy()
        probs, cols = r["prob"].cpu().numpy(), r["colors"].cpu().numpy()
        out = []
        decoded = decode_lines(toks, lens, cols, self.dictionary, rows=[row for row in range(len(r["order"])) if probs[row] >= threshold])
        for row, (_, i) in enumerate(r["order"]):
            q, prob = quads[i], float(probs[row])
            q.assigned_direction = dirs[i]
            if prob < threshold:
                continue
            txt, fgc, bgc = decoded[row]            # (decode_line of the tokens after the start symbol)
            out.append(_accept(q, txt, prob, fgc, bgc))
        return out


class HipModel48pxCTCOCR(HipModel48pxOCR):
    """``--ocr 48px_ctc`` on the HIP engine (ocr/model_48px_ctc.py:62-160)."""
    _KEY = _key = "48px_ctc_hip"
    _MODEL_MAPPING: Dict = {  # ocr/model_48px_ctc.py:19-28
        "model": {
            "url": _RELEASE + "ocr-ctc.zip",
            "hash": "fc61c52f7a811bc72c54f6be85df814c6b60f63585175db27cb94a08e0c30101",
            "archive": {
                "ocr-ctc.ckpt": ".",
                "alphabet-all-v5.txt": ".",
            },
        },
    }

    async def _load(self, device: str):
        from . import ocr_ctc

        dev = _gpu_device(device)
        if self._weights is None or self.dictionary is None:
            self._weights, self.dictionary = _load_ocr_ctc_checkpoint(self)
        self.engine = ocr_ctc.OcrCtcEngine(self._weights, len(self.dictionary), device=dev)
        self.device = device

    _rectify = None   # a callable here replaces textline.rectify (``rectify_fn`` of textline.rectified_chunks): host stand-ins in tests

    @torch.no_grad()
    async def _infer(self, image: np.ndarray, textlines: List, config=None, verbose: bool = False):
        """Same contract as the 48px plugin; chunks are padded to max_w + 7 + 128 (:84), the line probability is
        exp(mean log-prob) against a 0.5 default threshold (:66,:124), colours average over non-space characters (:116-123).
        ``config.ignore_bubble`` in 1..50 applies the reference's frame / colour heuristic to every rectified crop (:91-93, utils/bubble.py):
        a rejected line's row of the chunk stays zero and is recognised as such, exactly as the reference's ``continue`` leaves it.  The
        test runs on the device, where the chunk is (``textline.bubble_crop_flags``)."""
        from . import ocr_ctc, textline as TL

        threshold, ignore_bubble = _ocr_options(config, 0.5)
        quads, dirs, own = self._prepare(textlines)
        if not quads:
            return []
        out = []
        for idx, _, region in TL.rectified_chunks(self._page_on_device(image), own, dirs, 48, ocr_ctc.CHUNK_EXTRA, None, self._rectify,
                                                  ignore_bubble=ignore_bubble):
            logits, colors = self.engine.forward(region)
            for j, line in enumerate(self.engine.decode(logits, colors, 0)):
                q = quads[idx[j]]
                q.assigned_direction = dirs[idx[j]]
                res = decode_ctc_line(line, self.dictionary)
                if res is None or res[1] < threshold:
                    continue
                out.append(_accept(q, *res))
        return out


class HipModel32pxOCR(HipModel48pxOCR):
    """``--ocr 32px`` on the HIP engine (ocr/model_32px.py:19-140)."""
    _KEY = _key = "32px_hip"
    _MODEL_MAPPING: Dict = {  # ocr/model_32px.py:20-29
        "model": {
            "url": "https://github.com/zyddnys/manga-image-translator/releases/download/beta-0.3/ocr.zip",
            "hash": "47405638b96fa2540a5ee841a4cd792f25062c09d9458a973362d40785f95d7a",
            "archive": {
                "ocr.ckpt": ".",
                "alphabet-all-v5.txt": ".",
            },
        },
    }

    async def _load(self, device: str):
        from . import ocr32

        dev = _gpu_device(device)
        if self._weights is None or self.dictionary is None:
            self._weights, self.dictionary = _load_ocr32_checkpoint(self)
        self.engine = ocr32.Ocr32Engine(self._weights, len(self.dictionary), device=dev)
        self.device = device

    @torch.no_grad()
    async def _infer(self, image: np.ndarray, textlines: List, config=None, verbose: bool = False, max_seq_length: int = 255):
        """Same contract as the 48px plugin with the 32px model's rules (:58-140): text height 32, chunks padded to max_w + 7, the line
        probability exp(mean log-prob) against a 0.7 default threshold (:62), each colour the mean of the clipped head over ALL positions of
        the chosen hypothesis's history (:104-109).  ``config.ignore_bubble`` in 1..50: a rejected line's rows of the chunk stay zero and it
        is decoded as such (:84-86).  Returns the accepted lines in processing order."""
        threshold, ignore_bubble = _ocr_options(config, 0.7)
        quads, dirs, own = self._prepare(textlines)
        if not quads:
            return []
        r = self.engine.recognize_lines(self._page_on_device(image), own, dirs, max_seq_length=max_seq_length, ignore_bubble=ignore_bubble)
        toks, lens = r["tokens"].cpu().numpy(), r["length"].cpu().numpy()
        probs, cols = r["prob"].cpu().numpy(), r["colors"].cpu().numpy()
        out = []
        for row, i in enumerate(r["order"]):
            q, prob = quads[i], float(probs[row])
            q.assigned_direction = dirs[i]
            if prob < threshold:
                continue
            n = int(lens[row])
            txt, fgc, bgc = decode_32px_line(toks[row, :n], cols[row, :n - 1], self.dictionary)
            out.append(_accept(q, txt, prob, fgc, bgc))
        return out


MOCR_SUBDIR = "manga-ocr-base"   # <model_dir>/ocr/manga-ocr-base/: config.json (+ generation_config.json), weights, vocab.txt
MOCR_MAX_LENGTH = 300            # manga_ocr calls model.generate(x[None], max_length=300)
BERT_SPECIAL_TOKENS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")


def mocr_tokens_to_text(token_ids: Sequence[int], vocab: Sequence[str], special_ids: Sequence[int] = ()) -> str:
    """BertTokenizer.decode(ids, skip_special_tokens=True) over ``vocab.txt``: special tokens are skipped, the rest joined with blanks and
    every ``" ##"`` dropped (convert_tokens_to_string)."""
    skip = set(int(i) for i in special_ids)
    toks = [vocab[int(t)] for t in token_ids if int(t) not in skip and vocab[int(t)] not in BERT_SPECIAL_TOKENS]
    return " ".join(toks).replace(" ##", "").strip()


def mocr_post_process(text: str) -> str:
    """``manga_ocr.ocr.post_process``: the package's own function when it imports; otherwise its whitespace / ellipsis part restated
    (all whitespace removed, "…" -> "...", runs of "・" / "." -> as many "."), WITHOUT the final half-width -> full-width step
    (``jaconv.h2z(text, ascii=True, digit=True)``), which needs ``jaconv`` and is applied only when that package imports."""
    try:
        from manga_ocr.ocr import post_process  # type: ignore

        return post_process(text)
    except ImportError:
        pass
    import re

    text = "".join(text.split())
    text = text.replace("…", "...")
    text = re.sub("[・.]{2,}", lambda x: (x.end() - x.start()) * ".", text)
    try:
        import jaconv  # type: ignore

        text = jaconv.h2z(text, ascii=True, digit=True)
    except ImportError:
        pass
    return text


def mocr_aggregate(groups: Sequence[Sequence[int]], lines: Dict[int, object]):
    """model_manga_ocr.py:239-275 for every merged group: ``lines`` holds the 48px results (prob, area, fg_*, bg_*) of the line indices
    that passed prob >= 0.2.  -> [(prob, (fr, fg, fb), (br, bg, bb))]: prob = exp(sum(log(prob_i) * area_i) / sum(area_i)), or 0.0 without
    area; each colour the rounded mean over the group's lines, 0 without lines."""
    out = []
    for nodes in groups:
        total_logprobs, total_area = 0, 0
        cols = [[] for _ in range(6)]
        for idx in nodes:
            if idx not in lines:
                continue
            r = lines[idx]
            total_logprobs += np.log(r.prob) * r.area
            total_area += r.area
            for acc, name in zip(cols, ("fg_r", "fg_g", "fg_b", "bg_r", "bg_g", "bg_b")):
                acc.append(getattr(r, name))
        prob = float(np.exp(total_logprobs / total_area)) if total_area > 0 else 0.0
        c = [round(np.mean(v)) if v else 0 for v in cols]
        out.append((prob, tuple(c[:3]), tuple(c[3:])))
    return out


class HipModelMangaOCR(HipModel48pxOCR):
    """``--ocr mocr`` on the HIP engine (ocr/model_manga_ocr.py:132-295): the 48px model for every line's probability and colours (a line
    under 0.2 contributes none; its text is discarded), the manga-ocr VisionEncoderDecoderModel (``mocr.MocrEngine``) for the text.

    ``weights``: {"ocr48": 48px state dict, "mocr": state dict in mocr_schema's names}; with them ``dictionary`` (48px), ``vocab``
    (the lines of vocab.txt), ``mocr_config`` (the config.json dict) and ``generation`` (mocr_schema.GenerationParams).  Without them
    ``_load`` reads ocr_ar_48px.ckpt + alphabet-all-v7.txt and ``<model_dir>/ocr/manga-ocr-base/``.  ``ocr48``: a loaded
    ``HipModel48pxOCR`` to share instead of loading the 48px model a second time.
    ``config.use_mocr_merge = True`` is refused: it needs ``merge_bboxes`` with its own tolerances and a minimum rotated rectangle."""
    _KEY = _key = "mocr_hip"

    def __init__(self, *args, weights: Optional[Dict[str, Dict[str, torch.Tensor]]] = None, dictionary: Optional[Sequence[str]] = None,
                 vocab: Optional[Sequence[str]] = None, mocr_config: Optional[Dict] = None, generation=None, ocr48=None, **kwargs):
        self._ocr48_weights = None if weights is None else weights.get("ocr48")
        self._shared48 = ocr48
        super().__init__(*args, weights=None if weights is None else weights.get("mocr"), dictionary=dictionary, **kwargs)
        self.vocab, self.mocr_config, self.generation = vocab, mocr_config, generation
        have48 = ocr48 is not None or (self._ocr48_weights is not None and dictionary is not None)
        self._downloaded = self._downloaded if weights is None else all(g is not None for g in (self._weights, vocab, mocr_config, generation)) and have48

    async def _load(self, device: str):
        from . import mocr, mocr_schema

        dev = _gpu_device(device)
        if self._shared48 is not None:
            self.ocr48 = self._shared48
        else:
            self.ocr48 = HipModel48pxOCR(weights=self._ocr48_weights, dictionary=self.dictionary if self._ocr48_weights is not None else None)
        if not self.ocr48.is_loaded():
            await self.ocr48.load(device)
        if self._weights is None:
            self._weights, self.mocr_config, self.generation, self.vocab = _load_mocr_checkpoint(self)
        self.engine = mocr.MocrEngine(self._weights, self.mocr_config, self.generation, device=dev)
        if len(self.vocab) != self.engine.cfg.vocab:
            raise ValueError(f"vocab.txt has {len(self.vocab)} lines, the model's vocabulary is {self.engine.cfg.vocab}")
        self.device = device

    async def _unload(self):
        await super()._unload()
        if self._shared48 is None and getattr(self, "ocr48", None) is not None:
            await self.ocr48.unload()

    @torch.no_grad()
    async def _infer(self, image: np.ndarray, textlines: List, config=None, verbose: bool = False, ignore_bubble: int = 0):
        """Sets text / prob / fg_* / bg_* on the same Quadrilateral objects and returns ALL of them in processing order, as the reference
        does (no threshold on the result: a line under 0.2 in the 48px model keeps its text with prob 0.0 and black colours)."""
        if config is not None and getattr(config, "use_mocr_merge", False):
            raise ValueError("ocr.use_mocr_merge = True is not implemented by the HIP mocr plugin (supported: use_mocr_merge = False)")
        quads, dirs, own = self._prepare(textlines)
        if not quads:
            return []
        # the 48px pass (:164-237): fixed 0.2 threshold, max_seq_length 255, no ignore_bubble
        accepted = await self.ocr48._infer(image, quads, None, verbose, 0, 255)
        passed = {id(q) for q in accepted}
        lines = {i: _own_stats(q, own[i]) for i, q in enumerate(quads) if id(q) in passed}
        r = self.engine.recognize_lines(self._page_on_device(image), own, dirs)
        toks, lens = r["tokens"].cpu().numpy(), r["length"].cpu().numpy()
        g = self.engine.generation
        special = [t for t in (g.eos_token_id, g.pad_token_id, g.decoder_start_token_id) if t is not None]
        agg = mocr_aggregate([[i] for i in range(len(quads))], lines)
        out = []
        for i, (q, (prob, fgc, bgc)) in enumerate(zip(quads, agg)):
            txt = mocr_post_process(mocr_tokens_to_text(toks[i, :int(lens[i])], self.vocab, special))
            q.assigned_direction = dirs[i]
            out.append(_accept(q, txt, prob, fgc, bgc))
        return out


def _own_stats(q, own):
    """What the aggregation reads of a line that passed the 48px threshold: its probability and colours, and the area of its quad."""
    import types

    return types.SimpleNamespace(prob=q.prob, area=own.area, fg_r=q.fg_r, fg_g=q.fg_g, fg_b=q.fg_b, bg_r=q.bg_r, bg_g=q.bg_g, bg_b=q.bg_b)


def decode_32px_line(tokens, colour_history, dictionary: Sequence[str]) -> Tuple[str, Tuple[int, int, int], Tuple[int, int, int]]:
    """Tokens (start symbol included) + the six colour heads over the hypothesis's output history [len, 6] -> (text, fg rgb, bg rgb):
    model_32px.py:104-120.  Each colour is ``(clip(head, 0, 1).mean() * 255)`` truncated, in float32 like the reference, over every
    position — the one that predicted ``</S>`` too; the text skips ``<S>``, stops at ``</S>`` and maps ``<SP>`` to a blank."""
    col = np.clip(np.asarray(colour_history, dtype=np.float32).reshape(-1, 6), np.float32(0), np.float32(1))
    mean = col.mean(axis=0, dtype=np.float32) * np.float32(255)
    c = [int(v) for v in mean]   # .long(): truncation
    seq: List[str] = []
    for t in tokens:
        ch = dictionary[int(t)]
        if ch == "<S>":
            continue
        if ch == "</S>":
            break
        seq.append(" " if ch == "<SP>" else ch)
    return "".join(seq), (c[0], c[1], c[2]), (c[3], c[4], c[5])


def decode_ctc_line(line, dictionary: Sequence[str]):
    """[(char id, log-prob, fr, fg, fb, br, bg, bb)] -> (text, prob, fg rgb, bg rgb) or None for an empty line:
    model_48px_ctc.py:105-134 (AvgMeter means; colours only over non-space characters; prob = exp(mean log-prob))."""
    if not line:
        return None
    chars, lp_sum = [], 0.0
    acc = [0] * 6
    n_col = 0
    for chid, logprob, *cols in line:
        ch = dictionary[int(chid)]
        if ch == "<SP>":
            ch = " "
        chars.append(ch)
        lp_sum += logprob
        if ch != " ":
            for k in range(6):
                acc[k] += int(cols[k] * 255)
            n_col += 1
    prob = float(np.exp(lp_sum / len(line)))
    mean = [int(a / n_col) if n_col else 0 for a in acc]
    return "".join(chars), prob, tuple(mean[:3]), tuple(mean[3:])


def decode_line(token_ids: np.ndarray, colors: np.ndarray, dictionary: Sequence[str]) -> Tuple[str, Tuple[int, int, int], Tuple[int, int, int]]:
    """Token ids + colour-head rows -> (text, fg rgb, bg rgb): model_48px.py:124-158 (AvgMeter means of int(c*255))."""
    has_fg = colors[:, 7] > colors[:, 6]
    has_bg = colors[:, 9] > colors[:, 8]
    seq: List[str] = []
    acc = [[0, 0] for _ in range(6)]  # sum, count for fr fg fb br bg bb

    def add(k, v):
        acc[k][0] += int(v * 255)
        acc[k][1] += 1

    for t, chid in enumerate(token_ids):
        ch = dictionary[int(chid)]
        if ch == "<S>":
            continue
        if ch == "</S>":
            break
        seq.append(" " if ch == "<SP>" else ch)
        if has_fg[t]:
            for k in range(3):
                add(k, colors[t, k])
        src = colors[t, 3:6] if has_bg[t] else colors[t, 0:3]
        for k in range(3):
            add(3 + k, src[k])
    mean = [min(max(int(s / c) if c else 0, 0), 255) for s, c in acc]
    return "".join(seq), tuple(mean[:3]), tuple(mean[3:])


def decode_lines(tokens: np.ndarray, lengths: np.ndarray, colors: np.ndarray, dictionary: Sequence[str], rows=None
                 ) -> List[Tuple[str, Tuple[int, int, int], Tuple[int, int, int]]]:
    """``decode_line`` for all result rows of a decode at once (tokens [n, T + 1] with the start symbol in column 0, lengths [n],
    colours [n, T, 10]): the same integer arithmetic, vectorised over lines and positions — a page group's 512 lines cost one pass of
    numpy instead of half a millisecond of interpreter each.  ``rows``: only these rows (others give None)."""
    tokens, lengths, colors = np.asarray(tokens), np.asarray(lengths), np.asarray(colors, dtype=np.float32)
    n, T = tokens.shape[0], colors.shape[1]
    if n == 0:
        return []
    ids = tokens[:, 1:1 + T].astype(np.int64)
    pos = np.arange(ids.shape[1])[None, :]
    inside = pos < (lengths.astype(np.int64)[:, None] - 1)
    s_id, e_id = dictionary.index("<S>"), dictionary.index("</S>")
    is_end = inside & (ids == e_id)
    cut = np.where(is_end.any(1), is_end.argmax(1), ids.shape[1])          # the first </S> ends the line
    keep = inside & (pos < cut[:, None]) & (ids != s_id)                   # <S> is skipped, not counted
    c = colors[:, :ids.shape[1]]
    q = (c[..., :6] * np.float32(255)).astype(np.int64)                    # int(v * 255) on float32 values: truncation
    has_fg = keep & (c[..., 7] > c[..., 6])
    has_bg = c[..., 9] > c[..., 8]
    fg_sum = (q[..., 0:3] * has_fg[..., None]).sum(1)
    fg_cnt = has_fg.sum(1)
    bsrc = np.where(has_bg[..., None], q[..., 3:6], q[..., 0:3])
    bg_sum = (bsrc * keep[..., None]).sum(1)
    bg_cnt = keep.sum(1)

    def mean(sm, cnt):   # int(sum / count) clamped to a byte; 0 without samples
        m = np.where(cnt[:, None] > 0, np.trunc(sm / np.maximum(cnt, 1)[:, None]), 0).astype(np.int64)
        return np.clip(m, 0, 255)

    fg, bg = mean(fg_sum, fg_cnt), mean(bg_sum, bg_cnt)
    chars = np.asarray([" " if ch == "<SP>" else ch for ch in dictionary], dtype=object)
    out: List = [None] * n
    for r in (range(n) if rows is None else rows):
        out[r] = ("".join(chars[ids[r, keep[r]]]), tuple(int(v) for v in fg[r]), tuple(int(v) for v in bg[r]))
    return out


LAMA_PRECISIONS = ("fp32", "bf16", "config")


def lama_precision_default() -> str:
    """The ``precision`` of a LaMa plugin created without one (``register()``, ``serve.py``): ``MIT_LAMA_PRECISION`` in the
    environment ("fp32" | "bf16" | "config"), else "fp32"."""
    v = os.environ.get("MIT_LAMA_PRECISION", "").strip().lower() or "fp32"
    if v not in LAMA_PRECISIONS:
        raise ValueError(f"MIT_LAMA_PRECISION must be one of {LAMA_PRECISIONS} (got {v!r})")
    return v


def resolve_lama_precision(setting: str, config=None) -> str:
    """A plugin's ``precision`` setting and the ``config`` of a call -> the engine's precision, "fp32" or "bf16".  "config" follows
    ``config.inpainting_precision`` the way the reference's GPU path does (inpainting_lama_mpe.py:97-107: ``bf16`` -> bf16, ``fp16``
    -> bf16 as well, :102-104; ``fp32`` -> fp32); without a config it is fp32."""
    if setting not in LAMA_PRECISIONS:
        raise ValueError(f"LaMa precision must be one of {LAMA_PRECISIONS} (got {setting!r})")
    if setting != "config":
        return setting
    if config is None:
        return "fp32"
    v = getattr(config, "inpainting_precision", None)
    v = str(getattr(v, "value", v)).lower()      # the reference's InpaintPrecision is a str enum
    if v in ("bf16", "fp16"):
        return "bf16"
    if v == "fp32":
        return "fp32"
    raise ValueError(f"config.inpainting_precision must be fp32, fp16 or bf16 (got {v!r})")


class HipLamaMPEInpainter(_EnginePlugin, _InpBase):
    """``--inpainter lama_mpe`` on the HIP engine.  ``precision``: "fp32" (default), "bf16", or "config" = what the call's
    ``config.inpainting_precision`` says, as in the reference (``resolve_lama_precision``); None = ``lama_precision_default()``."""
    _KEY = _key = "lama_mpe_hip"
    _MODEL_MAPPING: Dict = {  # inpainting/inpainting_lama_mpe.py:32-38
        "model": {
            "url": _RELEASE + "inpainting_lama_mpe.ckpt",
            "hash": "d625aa1b3e0d0408acfd6928aa84f005867aa8dbb9162480346a4e20660786cc",
            "file": ".",
        },
    }
    N_BLOCKS, USE_MPE, CKPT = 9, True, "inpainting_lama_mpe.ckpt"

    def __init__(self, *args, weights: Optional[Dict[str, Dict[str, torch.Tensor]]] = None,
                 resize: Optional[Callable] = None, precision: Optional[str] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self._resize = resize
        self.precision = lama_precision_default() if precision is None else precision
        resolve_lama_precision(self.precision)      # a bad value raises here, not at the first page
        self._hand_over(weights)

    def precision_for(self, config=None) -> str:
        """The engine precision of a call with this ``config``: "fp32" or "bf16"."""
        return resolve_lama_precision(self.precision, config)

    async def _load(self, device: str):
        from . import lama

        dev = _gpu_device(device)
        w = self._weights or _load_lama_checkpoint(self)
        self.engine = lama.LamaEngine(w["lama.gen"], w.get("lama.mpe") if self.USE_MPE else None, n_blocks=self.N_BLOCKS,
                                      device=dev)
        self.device = device

    @torch.no_grad()
    async def _infer(self, image: np.ndarray, mask: np.ndarray, config=None, inpainting_size: int = 1024,
                     verbose: bool = False) -> np.ndarray:
        """image u8 [H,W,3], mask u8 [H,W] -> inpainted [H,W,3] (inpainting_lama_mpe.py:56-118), any page size: the
        resize_keep_aspect / multiple-of-8 / back-to-page resizes and the final composite run on the GPU (imgproc.py).  The
        network runs in ``self.precision_for(config)``: fp32 by default (the reference's CPU path never autocasts, :93-95, and that
        is the parity target), bf16 when the plugin was created with ``precision="bf16"`` or with ``"config"`` and the config asks
        for bf16 / fp16 — the reference's GPU path (:97-107); see ``LamaEngine.forward``."""
        if image.ndim != 3 or image.shape[2] != 3 or mask.shape != image.shape[:2]:
            raise ValueError(f"bad shapes: image {image.shape}, mask {mask.shape}")
        if image.dtype != np.uint8 or mask.dtype != np.uint8:
            raise ValueError(f"expected uint8 page and mask, got {image.dtype} / {mask.dtype}")
        img0, msk0 = self._page_on_device(image), self._page_on_device(mask)
        # optional injected callable (img, (w, h), "keep_aspect" | "linear") -> ndarray: e.g. the real OpenCV
        return inpaint_pages(self.engine, img0, msk0, inpainting_size, self._resize, precision=self.precision_for(config))[0].cpu().numpy()

    @staticmethod
    def _resized(t: torch.Tensor, dsize, mode: str, injected: Optional[Callable]) -> torch.Tensor:
        """[B,H,W(,C)] u8 device tensor -> (w, h) = dsize: ``mit_resize_u8`` on the GPU, or the injected host callable page by page."""
        from . import imgproc

        if injected is None:
            return imgproc.resize_u8(t, dsize, exact=(mode == "keep_aspect"))
        return torch.from_numpy(np.ascontiguousarray(np.stack([injected(x.cpu().numpy(), dsize, mode) for x in t]))).to(t.device)


@torch.no_grad()
def inpaint_pages(engine, img0: torch.Tensor, msk0: torch.Tensor, inpainting_size: int, resize: Optional[Callable] = None,
                  micro_batch: int = 16, precision: str = "fp32") -> torch.Tensor:
    """The resize / composite legs of LamaMPEInpainter._infer (inpainting_lama_mpe.py:56-118) around ``engine.forward`` for device
    pages u8 [B,H,W,3] and masks u8 [B,H,W] of one size: what the plugin runs for its one page and the coupled batch engine for a
    group — the same kernels in the same order, so a page's bytes do not depend on how many pages travel with it.
    ``precision`` ("fp32" | "bf16") goes to ``engine.forward``; an engine is handed the argument only when it is not "fp32"."""
    if precision not in ("fp32", "bf16"):
        raise ValueError(f"inpaint_pages: precision must be 'fp32' or 'bf16' (got {precision!r})")
    fwd_kw = {} if precision == "fp32" else {"precision": precision}
    from . import imgproc

    B, height, width, _ = img0.shape
    rs = HipLamaMPEInpainter._resized
    out_all = torch.empty_like(img0)
    for a in range(0, B, micro_batch):
        i0, m0 = img0[a:a + micro_batch], msk0[a:a + micro_batch]
        img, msk = i0, m0
        if max(height, width) > inpainting_size:                                # resize_keep_aspect = INTER_LINEAR_EXACT (:64-66)
            dsize = imgproc.keep_aspect_size(height, width, inpainting_size)
            img, msk = rs(img, dsize, "keep_aspect", resize), rs(msk, dsize, "keep_aspect", resize)
        h, w = img.shape[1:3]
        new_h, new_w = (h + 7) // 8 * 8, (w + 7) // 8 * 8                      # pad_size 8, by RESIZING (INTER_LINEAR, :67-79)
        if (new_h, new_w) != (h, w):
            img, msk = rs(img, (new_w, new_h), "linear", resize), rs(msk, (new_w, new_h), "linear", resize)
        resized = (new_h, new_w) != (height, width)
        out = engine.forward(img, msk, composite=not resized, **fwd_kw)  # resized: img_inpainted of :111, every pixel from the network
        if resized:                                                             # back to the page size (:112-113)
            out = rs(out, (width, height), "linear", resize)
        # img_inpainted * mask_original + img_original * (1 - mask_original), mask_original = mask >= 127 (:57-61,116)
        out_all[a:a + micro_batch] = imgproc.select_u8(m0, 127, out, i0)
    return out_all


class HipLamaLargeInpainter(HipLamaMPEInpainter):
    """``--inpainter lama_large``: 18 blocks, no MPE (inpainting_lama_mpe.py:121-136)."""
    _KEY = _key = "lama_large_hip"
    _MODEL_MAPPING: Dict = {  # inpainting/inpainting_lama_mpe.py:123-129
        "model": {
            "url": "https://huggingface.co/dreMaz/AnimeMangaInpainting/resolve/main/lama_large_512px.ckpt",
            "hash": "11d30fbb3000fb2eceae318b75d9ced9229d99ae990a7f8b3ac35c8d31f2c935",
            "file": ".",
        },
    }
    N_BLOCKS, USE_MPE, CKPT = 18, False, "lama_large_512px.ckpt"


class HipAotInpainter(HipLamaMPEInpainter):
    """``--inpainter default``: the AOT generator (inpainting_aot.py:11-33).  Like the reference's AotInpainter it subclasses the
    LaMa-MPE plugin and reuses its ``_infer`` unchanged (input / 127.5 - 1, output (x + 1) * 127.5 truncated: the model is not a
    LamaFourier, inpainting_lama_mpe.py:84,114); only the model and its checkpoint differ.  ``weights``: {"aot": state_dict}.
    ``aot_precision``: "fp32" (default), "bf16" (the blocks on bf16-resident convolution operands, ``AotEngine``), or "config" = what
    the call's ``config.inpainting_precision`` says, as in the reference (``resolve_lama_precision``: bf16 and fp16 -> bf16); None =
    ``aot_precision_default()`` (``MIT_AOT_PRECISION``).  The inherited ``precision`` option and ``MIT_LAMA_PRECISION`` are LaMa's:
    here they are validated and have no effect."""
    _KEY = _key = "default_hip"
    _MODEL_MAPPING: Dict = {  # inpainting/inpainting_aot.py:12-18
        "model": {
            "url": _RELEASE + "inpainting.ckpt",
            "hash": "878d541c68648969bc1b042a6e997f3a58e49b6c07c5636ad55130736977149f",
            "file": ".",
        },
    }
    CKPT = "inpainting.ckpt"
    MB = 4   # pages per micro-batch of the engine: 16 full 2048 x 1456 pages run as four of them within one workspace

    def __init__(self, *args, aot_precision: Optional[str] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.aot_precision = aot_precision_default() if aot_precision is None else aot_precision
        if self.aot_precision not in LAMA_PRECISIONS:    # a bad value raises here, not at the first page
            raise ValueError(f"AOT precision must be one of {LAMA_PRECISIONS} (got {self.aot_precision!r})")

    def precision_for(self, config=None) -> str:
        """The engine precision of a call with this ``config``: what ``aot_precision`` resolves to, "fp32" or "bf16"."""
        resolve_lama_precision(self.precision, config)   # the inherited option is validated like the parent's
        return resolve_lama_precision(self.aot_precision, config)

    async def _load(self, device: str):
        from . import aot

        dev = _gpu_device(device)
        w = self._weights or _load_aot_checkpoint(self)
        # a plugin fixed to bf16 packs the bf16 weights at load; "config" decides per call, so they are packed at the first bf16 call
        self.engine = aot.AotEngine(w["aot"], device=dev, mb=self.MB, precision="bf16" if self.aot_precision == "bf16" else "fp32")
        self.device = device


def aot_precision_default() -> str:
    """The ``aot_precision`` of an AOT plugin created without one (``register()``, ``serve.py``): ``MIT_AOT_PRECISION`` in the
    environment ("fp32" | "bf16" | "config"), else "fp32"."""
    v = os.environ.get("MIT_AOT_PRECISION", "").strip().lower() or "fp32"
    if v not in LAMA_PRECISIONS:
        raise ValueError(f"MIT_AOT_PRECISION must be one of {LAMA_PRECISIONS} (got {v!r})")
    return v


ESRGAN_PRECISIONS = ("fp32", "bf16")


def esrgan_precision_default() -> str:
    """The ``precision`` of an ESRGAN plugin created without one (``register()``, ``serve.py``): ``MIT_ESRGAN_PRECISION`` in the
    environment ("fp32" | "bf16"), else "fp32"."""
    v = os.environ.get("MIT_ESRGAN_PRECISION", "").strip().lower() or "fp32"
    if v not in ESRGAN_PRECISIONS:
        raise ValueError(f"MIT_ESRGAN_PRECISION must be one of {ESRGAN_PRECISIONS} (got {v!r})")
    return v


class HipESRGANUpscaler(_EnginePlugin, _UpBase):
    """``--upscaler 4xultrasharp`` (RRDBNet 4x) on the HIP engine.  ``precision``: "fp32" (default) or "bf16" (the dense blocks on
    bf16-resident activations, ``EsrganEngine``); None = ``esrgan_precision_default()``."""
    _KEY = _key = "4xultrasharp_hip"
    _MODEL_MAPPING: Dict = {  # upscaling/esrgan_pytorch.py:513-518
        "4x-UltraSharp": {
            "url": _RELEASE + "4xESRGAN.pth",
            "hash": "545805ce2d861ee90972b5fa50b851f19ee4bb35dedd2eb090be1f7c935b6b00",
        },
    }
    _VALID_UPSCALE_RATIOS = [2, 3, 4]

    def __init__(self, *args, weights: Optional[Dict[str, torch.Tensor]] = None, precision: Optional[str] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.precision = esrgan_precision_default() if precision is None else precision
        if self.precision not in ESRGAN_PRECISIONS:      # a bad value raises here, not at the first page
            raise ValueError(f"ESRGAN precision must be one of {ESRGAN_PRECISIONS} (got {self.precision!r})")
        self._hand_over(weights)

    async def _load(self, device: str):
        from . import esrgan

        dev = _gpu_device(device)
        sd = self._weights or _load_esrgan_checkpoint(self)
        self.engine = esrgan.EsrganEngine(sd, nb=_esrgan_blocks(sd), device=dev, precision=self.precision)
        self.device = device

    @staticmethod
    def _pil_resized(t: torch.Tensor, size, resample: str) -> torch.Tensor:
        """[B,H,W,3] u8 -> (w, h) = size as Pillow resizes it: ``mit_resample_pil_u8`` for the engine's device tensor; what a host
        stand-in for the engine returns (the boundary checks against the reference's ``_infer`` run without a GPU) goes through the
        numpy form of the same tables, page by page."""
        from . import imgproc

        if t.is_cuda:
            return imgproc.pil_resize_u8(t, size, resample)
        return torch.from_numpy(np.stack([imgproc.pil_resize_u8_host(x.numpy(), size, resample) for x in t]))

    MAX_LR_PIXELS = 2048 * 1440   # low-resolution pixels of one ``forward``: the page the engine is known to hold (bench.py's config-5 leg)

    @torch.no_grad()
    async def _infer(self, image_batch: List, upscale_ratio: float) -> List:
        """List[PIL.Image] -> List[PIL.Image] (RGB), in input order: 4x on the GPU, then Pillow's bilinear resize by ratio / 4 on the GPU
        too (esrgan_pytorch.py:537-549, ``imgproc.pil_resize_u8``), so only the final page crosses PCIe.  Images of equal size go through
        one ``forward`` together, as the reference concatenates its batch (:541), in micro-batches of at most ``MAX_LR_PIXELS``
        low-resolution pixels; images of other sizes form groups of their own."""
        from PIL import Image

        from . import esrgan

        assert upscale_ratio <= 4
        pages = [np.array(img.convert("RGB")) for img in image_batch]
        groups: Dict[Tuple[int, int], List[int]] = {}
        for i, p in enumerate(pages):
            groups.setdefault(p.shape[:2], []).append(i)
        out: List = [None] * len(pages)
        fwd_kw = {} if self.precision == "fp32" else {"precision": self.precision}   # an engine is handed the argument only when it is not fp32
        for (h, w), idx in groups.items():
            mb = max(1, self.MAX_LR_PIXELS // max(1, h * w))
            size = esrgan.pass_size(w, h, upscale_ratio)
            for a in range(0, len(idx), mb):
                run = idx[a:a + mb]
                dev = torch.from_numpy(np.ascontiguousarray(np.stack([pages[i] for i in run]))).to(self.engine.device)
                res = self._pil_resized(self.engine.forward(dev, **fwd_kw), size, "bilinear").cpu().numpy()
                for k, i in enumerate(run):
                    out[i] = Image.fromarray(res[k])
        return out


MC2_PRECISIONS = ("fp32", "bf16")


def mc2_precision_default() -> str:
    """The ``precision`` of an mc2 colorizer plugin created without one (``register()``, ``serve.py``): ``MIT_MC2_PRECISION`` in the
    environment, fp32 when unset."""
    v = os.environ.get("MIT_MC2_PRECISION", "").strip().lower() or "fp32"
    if v not in MC2_PRECISIONS:
        raise ValueError(f"MIT_MC2_PRECISION must be one of {MC2_PRECISIONS} (got {v!r})")
    return v


class HipMangaColorizer(_EnginePlugin, _ColBase):
    """``--colorizer mc2`` (manga-colorization-v2: FFDNet denoiser + SE-ResNeXt generator) on the HIP engine.  Same ``_infer(image,
    colorization_size, denoise_sigma=25)`` -> RGB ``PIL.Image`` at the network's size, like the reference.  ``weights``:
    {"generator": state_dict, "denoiser": state_dict}.  ``precision``: "fp32" (default) or "bf16" (FFDNet on bf16-resident
    activations, the generator's dense convolutions on the one-product bf16 tiles, ``Mc2Engine``); None = ``mc2_precision_default()``."""
    _KEY = _key = "mc2_hip"
    _MODEL_SUB_DIR = os.path.join(_ColBase._MODEL_SUB_DIR, "manga-colorization-v2")
    _MODEL_MAPPING: Dict = {  # colorization/manga_colorization_v2.py:15-27
        "generator": {
            "url": _RELEASE + "manga-colorization-v2-generator.zip",
            "file": "generator.zip",
            "hash": "087e6a0bc02770e732a52f33878b71a272a6123c9ac649e9b5bfb75e39e5c1d5",
        },
        "denoiser": {
            "url": _RELEASE + "manga-colorization-v2-net_rgb.pth",
            "file": "net_rgb.pth",
            "hash": "0fe98bfd2ac870b15f360661b1c4789eecefc6dc2e4462842a0dd15e149a0433",
        },
    }

    def __init__(self, *args, weights: Optional[Dict[str, Dict[str, torch.Tensor]]] = None, precision: Optional[str] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.precision = mc2_precision_default() if precision is None else precision
        if self.precision not in MC2_PRECISIONS:         # a bad value raises here, not at the first page
            raise ValueError(f"mc2 precision must be one of {MC2_PRECISIONS} (got {self.precision!r})")
        self._hand_over(weights)

    async def _load(self, device: str):
        from . import mc2

        dev = _gpu_device(device)
        w = self._weights or _load_mc2_checkpoint(self)
        self.engine = mc2.Mc2Engine(w["generator"], w["denoiser"], device=dev, precision=self.precision)
        self.device = device

    @torch.no_grad()
    async def _infer(self, image, colorization_size: int, denoise_sigma=25, **kwargs):
        """PIL page -> colorized RGB PIL image (manga_colorization_v2.py:42-74); ``kwargs`` takes the context keys dispatch passes."""
        from PIL import Image

        out = self.engine.forward(self._page_on_device(np.array(image.convert("RGBA"))), colorization_size, denoise_sigma)
        return Image.fromarray(out[0].cpu().numpy())


# ---- host / device helpers of the detector plugins ---------------------------------------------------------------

def _native_ctd_boxes(lines_map, im_h, im_w):
    """SegDetectorRepresenter(thresh=0.3)(None, lines_map, height, width) on the native host routines (hostglue.py)."""
    from . import hostglue

    return hostglue.ctd_boxes(lines_map, im_h, im_w)


def _native_dbnet_boxes(db, h, w, text_threshold, box_threshold, unclip_ratio):
    from . import hostglue

    return hostglue.dbnet_boxes(db, h, w, text_threshold, box_threshold, unclip_ratio)


def default_preprocess_gpu(image: torch.Tensor, detect_size: int):
    """``imgproc.resize_aspect_ratio(cv2.bilateralFilter(image, 17, 80, 80), detect_size, cv2.INTER_LINEAR, mag_ratio=1)``
    (detection/default.py:62, default_utils/imgproc.py:37-70) on the device: bilateral filter (mit_bilateral_u8c3), 8-bit
    INTER_LINEAR resize of the long side to ``detect_size`` (mit_resize_u8), zero canvas padded right / bottom to a multiple of 256.
    image u8 [H,W,3] (device) -> (page u8 [1,H',W',3], ratio, pad_w, pad_h)."""
    return default_preprocess_pages(image[None], detect_size)


def default_preprocess_pages(pages: torch.Tensor, detect_size: int):
    """``default_preprocess_gpu`` for pages of one size: u8 [B,H,W,3] (device) -> (pages u8 [B,H',W',3], ratio, pad_w, pad_h).  The three
    steps are batched launches of the kernels a single page goes through, so a page's bytes do not depend on its company."""
    from . import imgproc

    n, height, width = int(pages.shape[0]), int(pages.shape[1]), int(pages.shape[2])
    ratio = detect_size / max(height, width)
    target_h, target_w = int(round(height * ratio)), int(round(width * ratio))
    proc = imgproc.resize_u8(imgproc.bilateral_filter_u8(pages, 17, 80.0, 80.0), (target_w, target_h))
    pad_h = (256 - target_h % 256) % 256
    pad_w = (256 - target_w % 256) % 256
    if pad_h or pad_w:
        canvas = torch.zeros(n, target_h + pad_h, target_w + pad_w, 3, dtype=torch.uint8, device=pages.device)
        canvas[:, :target_h, :target_w] = proc
        proc = canvas
    return proc, ratio, pad_w, pad_h


def _dbnet_textlines(boxes: np.ndarray, scores, ratio: float, quad_type=None) -> list:
    """The boxes of SegDetectorRepresenter at the network's page size -> the page's text lines (default.py:78-87): empty boxes dropped,
    ``adjustResultCoordinates`` with ratio_net = 1 (:83), the int cast, then only lines of an area above 16."""
    quad_type = quad_type or _RefQuadrilateral
    if boxes.size == 0:
        polys, scores = [], []
    else:
        idx = boxes.reshape(boxes.shape[0], -1).sum(axis=1) > 0
        polys = (boxes[idx].astype(np.float64) * ratio).astype(np.int64)
    textlines = [quad_type(pts.astype(int), "", float(s)) for pts, s in zip(polys, scores)]
    return [q for q in textlines if q.area > 16]


@torch.no_grad()
def dbnet_detect_pages(engine, pages_u8: torch.Tensor, detect_size: int, text_threshold: float, box_threshold: float, unclip_ratio: float,
                       micro_batch: int = 16, inject=None, quad_type=None):
    """DefaultDetector._infer (detection/default.py:56-103; dbnet_convnext.py:541-588 is the same text) for device pages u8 [B,H,W,3]
    of one size that are no webtoon strips, around ``engine.forward`` (a ``DbnetEngine`` or ``DbconvnextEngine``): what the plugin runs
    for its one page and the coupled batch engine for a group — the same kernels in the same order, so a page's results do not
    depend on how many pages travel with it.  Nothing but the boxes leaves the device:

    * bilateralFilter + resize_aspect_ratio (:62) for the whole micro-batch (``default_preprocess_pages``);
    * the network, ``micro_batch`` pages at a time;
    * SegDetectorRepresenter (:73-77) where the map is (csrc/ctd_boxes.hip), enqueued per micro-batch and collected after the loop (the
      handle owns its copy of the map, so the next micro-batch may overwrite the engine's workspace);
    * the x2 resize of the float mask, the crop of the padding and the cast to bytes (:89-95) in one kernel (csrc/dbnet_tail.hip).  The
      crop follows the reference's ``if pad_h > 0 … elif pad_w > 0``: only one side is ever cropped.

    ``inject`` (a stand-in for trained weights, as in ``CoupledPageEngine.detect``; applied after the network has run): ``prob`` f32
    [B,h,w] at the network's map size replaces ``db[:, 0]``, ``mask`` f32 [B,h/2,w/2] the mask head's output.
    -> (text lines per page, raw masks u8 [B,h',w'] on the device)."""
    from . import hostglue, imgproc

    if pages_u8.dtype != torch.uint8 or pages_u8.dim() != 4 or pages_u8.shape[-1] != 3 or not pages_u8.is_cuda:
        raise ValueError(f"dbnet_detect_pages expects a uint8 device tensor [B,H,W,3], got {pages_u8.dtype} {tuple(pages_u8.shape)}")
    B = int(pages_u8.shape[0])
    micro_batch = max(1, int(micro_batch))
    masks, handles, ratio = None, [], 1.0
    for a in range(0, B, micro_batch):
        page, target_ratio, pad_w, pad_h = default_preprocess_pages(pages_u8[a:a + micro_batch], detect_size)
        ratio = 1 / target_ratio
        n, h, w = int(page.shape[0]), int(page.shape[1]), int(page.shape[2])
        db, mask = engine.forward(page)
        prob = db[:, 0]
        if inject is not None:
            prob, mask = inject["prob"][a:a + n], inject["mask"][a:a + n]
            if tuple(prob.shape[1:]) != (h, w) or tuple(mask.shape[1:]) != (h // 2, w // 2):
                raise ValueError(f"dbnet_detect_pages: inject must hold prob [B,{h},{w}] and mask [B,{h // 2},{w // 2}] "
                                 f"(got {tuple(prob.shape)} / {tuple(mask.shape)})")
        handles.append(hostglue.boxes_from_bitmap_gpu_launch(prob, text_threshold, w, h, unclip_ratio=unclip_ratio, min_sside=3.0,
                                                             box_thresh=box_threshold, min_sside_out=5.0, roll_start=True))
        oh, ow = (h - pad_h, w) if pad_h > 0 else ((h, w - pad_w) if pad_w > 0 else (h, w))
        if masks is None:
            masks = torch.empty(B, oh, ow, dtype=torch.uint8, device=pages_u8.device)
        imgproc.dbnet_mask_tail(mask, oh, ow, out=masks[a:a + n])
    textlines = []
    for hd in handles:
        for boxes, scores in hostglue.boxes_from_bitmap_gpu_collect(hd):
            textlines.append(_dbnet_textlines(boxes, scores, ratio, quad_type))
    return textlines, masks


def _resize2x_f32(m: np.ndarray) -> np.ndarray:
    """cv2.resize(mask, (2w, 2h), INTER_LINEAR) on a float32 map (default.py:89): plain bilinear at pixel centres with edge
    replication — float data takes OpenCV's unquantised path (coefficients 1 - f, f in float32)."""
    h, w = m.shape

    def taps(n):
        f = ((np.arange(2 * n, dtype=np.float64) + 0.5) * 0.5 - 0.5).astype(np.float32)
        i0 = np.floor(f).astype(np.int64)
        fr = (f - i0.astype(np.float32)).astype(np.float32)
        lo, hi = i0 < 0, i0 >= n - 1
        i0 = np.where(lo, 0, np.where(hi, n - 1, i0))
        fr = np.where(lo | hi, np.float32(0), fr).astype(np.float32)
        return i0, np.minimum(i0 + 1, n - 1), (np.float32(1) - fr).astype(np.float32), fr

    y0, y1, wy0, wy1 = taps(h)
    x0, x1, wx0, wx1 = taps(w)
    m = m.astype(np.float32)
    rows = m[:, x0] * wx0[None, :] + m[:, x1] * wx1[None, :]
    return (rows[y0] * wy0[:, None] + rows[y1] * wy1[:, None]).astype(np.float32)


def _bare_state_dict(ck):
    """A checkpoint saved as {'model': state_dict} or as the bare state_dict -> the state_dict."""
    return ck["model"] if "model" in ck else ck


def _esrgan_blocks(sd) -> int:
    """RRDB blocks of an RRDBNet state_dict, from its keys (esrgan_pytorch.py infer_params :470-509)."""
    nb = 1 + max((int(k.split(".")[3]) for k in sd if k.startswith("model.1.sub.") and ".RDB" in k), default=-1)
    if nb <= 0:
        raise ValueError("4xESRGAN.pth: no RRDB trunk (model.1.sub.<n>.…) in the state_dict")
    return nb


def _ckpt_path(plugin, name: str) -> str:
    if hasattr(plugin, "_get_file_path"):
        return plugin._get_file_path(name)
    return os.path.join("models", name)


def _load_ctd_checkpoint(plugin):
    """comictextdetector.pt = {'blk_det': {'cfg','weights'}, 'text_seg', 'text_det'} (ctd_utils/basemodel.py:205-214)."""
    from . import ctd_schema as S, synth

    ck = torch.load(_ckpt_path(plugin, "comictextdetector.pt"), map_location="cpu")
    S.check_yolo_cfg(ck["blk_det"]["cfg"])  # the reference builds the backbone from it (yolov5/yolo.py:286-292)
    return {"ctd.yolo": synth.check_state_dict(ck["blk_det"]["weights"], S.yolo_schema(), "comictextdetector.pt blk_det.weights"),
            "ctd.seg": synth.check_state_dict(ck["text_seg"], S.unet_head_schema(), "comictextdetector.pt text_seg"),
            "ctd.det": synth.check_state_dict(ck["text_det"], S.db_head_schema(), "comictextdetector.pt text_det")}


def _read_dictionary(path: str):
    with open(path, "r", encoding="utf-8") as fp:
        return [s[:-1] for s in fp.readlines()]  # model_48px.py:47-48: every line loses its last character (the newline)


def _load_ocr_checkpoint(plugin):
    """ocr_ar_48px.ckpt (a bare state_dict) + alphabet-all-v7.txt (model_48px.py:46-52)."""
    from . import ocr_schema, synth

    dictionary = _read_dictionary(_ckpt_path(plugin, "alphabet-all-v7.txt"))
    sd = torch.load(_ckpt_path(plugin, "ocr_ar_48px.ckpt"), map_location="cpu")
    return synth.check_state_dict(sd, ocr_schema.ocr48_schema(len(dictionary)), "ocr_ar_48px.ckpt"), dictionary


def _load_ocr_ctc_checkpoint(plugin):
    """ocr-ctc.ckpt ({'model': state_dict} or bare; its three ``encoders.layers.N.pe.pe`` tables are dropped by the reference and
    unused here) + alphabet-all-v5.txt (model_48px_ctc.py:19-28,38-48)."""
    from . import ocr_ctc_schema, synth

    dictionary = _read_dictionary(_ckpt_path(plugin, "alphabet-all-v5.txt"))
    sd = _bare_state_dict(torch.load(_ckpt_path(plugin, "ocr-ctc.ckpt"), map_location="cpu"))
    return synth.check_state_dict(sd, ocr_ctc_schema.ocr_ctc_schema(len(dictionary)), "ocr-ctc.ckpt"), dictionary


def _load_ocr32_checkpoint(plugin):
    """ocr.ckpt ({'model': state_dict} or bare, ``pe.pe`` included) + alphabet-all-v5.txt (model_32px.py:39-45)."""
    from . import ocr32_schema, synth

    dictionary = _read_dictionary(_ckpt_path(plugin, "alphabet-all-v5.txt"))
    sd = _bare_state_dict(torch.load(_ckpt_path(plugin, "ocr.ckpt"), map_location="cpu"))
    return synth.check_state_dict(sd, ocr32_schema.ocr32_schema(len(dictionary)), "ocr.ckpt"), dictionary


def _load_mocr_checkpoint(plugin):
    """``<model_dir>/ocr/manga-ocr-base/``: config.json (+ generation_config.json), the weights and vocab.txt -> (state dict, config dict,
    GenerationParams, vocab).  When ``transformers`` imports the weights go through ``VisionEncoderDecoderModel.from_pretrained(dir,
    local_files_only=True)``, so that the key names of older checkpoints are converted by HuggingFace itself; otherwise
    ``pytorch_model.bin`` (or ``model.safetensors`` when ``safetensors`` imports) must already hold mocr_schema's names.
    ``max_length`` is the 300 manga_ocr passes to ``generate``."""
    from . import mocr_schema, synth

    d = _ckpt_path(plugin, MOCR_SUBDIR)
    cfg, c, gen = mocr_schema.load_model_dir(d, max_length=MOCR_MAX_LENGTH)
    with open(os.path.join(d, "vocab.txt"), "r", encoding="utf-8") as fp:
        vocab = [s.rstrip("\n") for s in fp.readlines()]
    try:
        from transformers import VisionEncoderDecoderModel  # type: ignore
    except ImportError:
        VisionEncoderDecoderModel = None
    if VisionEncoderDecoderModel is not None:
        sd = VisionEncoderDecoderModel.from_pretrained(d, local_files_only=True).state_dict()
    elif os.path.exists(os.path.join(d, "pytorch_model.bin")):
        sd = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu")
    else:
        from safetensors.torch import load_file  # type: ignore

        sd = load_file(os.path.join(d, "model.safetensors"))
    return synth.check_state_dict(sd, mocr_schema.mocr_schema(c, pooler=False), MOCR_SUBDIR), cfg, gen, vocab


def _load_lama_checkpoint(plugin):
    """{'gen_state_dict', 'str_state_dict'?} (inpainting_lama_mpe.py:818-825)."""
    from . import lama_schema, synth

    ck = torch.load(_ckpt_path(plugin, plugin.CKPT), map_location="cpu")
    out = {"lama.gen": synth.check_state_dict(ck["gen_state_dict"], lama_schema.lama_generator_schema(plugin.N_BLOCKS), plugin.CKPT)}
    if "str_state_dict" in ck:
        out["lama.mpe"] = ck["str_state_dict"]
        if plugin.USE_MPE:
            synth.check_state_dict(out["lama.mpe"], lama_schema.lama_mpe_schema(), plugin.CKPT + " str_state_dict")
    return out


def _load_aot_checkpoint(plugin):
    """inpainting.ckpt: {'model': state_dict} or a bare state_dict (inpainting_aot.py:27-28), schema-checked."""
    from . import aot_schema, synth

    sd = _bare_state_dict(torch.load(_ckpt_path(plugin, plugin.CKPT), map_location="cpu"))
    return {"aot": synth.check_state_dict(sd, aot_schema.aot_generator_schema(), plugin.CKPT)}


def _load_dbconvnext_checkpoint(plugin):
    """dbnet_convnext.ckpt: {'model': state_dict} or a bare state_dict (detection/dbnet_convnext.py:529-530), schema-checked.  The 1x1
    shortcut of an up-block may come without its bias (whether timm's ``create_conv2d`` gives it one depends on the timm release the
    checkpoint was trained with; the engine takes either)."""
    from . import dbconvnext_schema, synth

    sd = _bare_state_dict(torch.load(_ckpt_path(plugin, plugin.CKPT), map_location="cpu"))
    schema = [e for e in dbconvnext_schema.dbnet_convnext_schema() if e[0] in sd or not e[0].endswith(".shortcut.conv.bias")]
    return synth.check_state_dict(sd, schema, plugin.CKPT)


def _load_esrgan_checkpoint(plugin):
    """4xESRGAN.pth: a bare RRDBNet state_dict; the block count comes from its keys (esrgan_pytorch.py:526-528, infer_params :476-510)."""
    from . import esrgan_schema, synth

    sd = torch.load(_ckpt_path(plugin, "4xESRGAN.pth"), map_location="cpu")
    return synth.check_state_dict(sd, esrgan_schema.rrdbnet_schema(_esrgan_blocks(sd)), "4xESRGAN.pth")


def _load_mc2_checkpoint(plugin):
    """generator.zip (a bare Generator state_dict, manga_colorization_v2.py:33-34) and net_rgb.pth (FFDNet, with or without the
    DataParallel ``module.`` prefix, denoising/denoiser.py:36-48), schema-checked."""
    from . import mc2_schema, synth

    g = torch.load(_ckpt_path(plugin, "generator.zip"), map_location="cpu")
    d = mc2_schema.strip_dataparallel(torch.load(_ckpt_path(plugin, "net_rgb.pth"), map_location="cpu"))
    return {"generator": synth.check_state_dict(g, mc2_schema.generator_schema(), "generator.zip"),
            "denoiser": synth.check_state_dict(d, mc2_schema.ffdnet_schema(), "net_rgb.pth")}


def register() -> None:
    """Add the HIP backends to the reference's registries (needs the reference package; INTEGRATION.md shows the
    matching enum members)."""
    if not HAVE_REFERENCE:
        raise RuntimeError("manga_translator is not importable: nothing to register into")
    from manga_translator.detection import DETECTORS  # type: ignore
    from manga_translator.inpainting import INPAINTERS  # type: ignore
    from manga_translator.ocr import OCRS  # type: ignore

    from manga_translator.upscaling import UPSCALERS  # type: ignore
    from manga_translator.colorization import COLORIZERS  # type: ignore
    from manga_translator import config as _cfg  # type: ignore

    def key(enum_name: str, value: str):
        """The enum member when the maintainer has added it to config.py, else the plain string: the
        registries are ordinary dicts and ``get_detector`` & co only look the key up (detection/__init__.py:22-28)."""
        enum = getattr(_cfg, enum_name, None)
        try:
            return enum(value)
        except Exception:
            return value

    for reg, enum_name, cls in ((DETECTORS, "Detector", HipComicTextDetector), (DETECTORS, "Detector", HipDefaultDetector),
                                (DETECTORS, "Detector", HipDBConvNextDetector),
                                (OCRS, "Ocr", HipModel48pxOCR), (OCRS, "Ocr", HipModel48pxCTCOCR),
                                (OCRS, "Ocr", HipModel32pxOCR), (OCRS, "Ocr", HipModelMangaOCR),
                                (INPAINTERS, "Inpainter", HipLamaMPEInpainter), (INPAINTERS, "Inpainter", HipLamaLargeInpainter),
                                (INPAINTERS, "Inpainter", HipAotInpainter),
                                (UPSCALERS, "Upscaler", HipESRGANUpscaler), (COLORIZERS, "Colorizer", HipMangaColorizer)):
        reg[key(enum_name, cls._KEY)] = cls
