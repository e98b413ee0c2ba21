"""Worker-pool serving over the GPUs of a node: one reference ``shared``-mode worker per GPU.

What the reference has (nothing here replaces its server):

* ``manga_translator/mode/share.py:47-174`` ``MangaShare`` — a worker process that owns one ``MangaTranslator`` and serves
  ``POST /simple_execute/{method}`` (pickled attributes in, pickled result out) and ``POST /execute/{method}`` (a stream of frames
  ``status:1 | length:4 big-endian | payload`` — 0 result, 1 progress, 2 error), one request at a time (``429`` while busy), guarded by
  an ``X-Nonce`` header, with a restricted unpickler for the request body;
* ``server/instance.py:10-67`` ``ExecutorInstance`` / ``Executors`` — the front server's table of such workers (ip, port, busy) with
  ``find_executor`` / ``free_executor``; workers are entered through ``POST /register`` (``server/main.py:45-50``);
* ``server/main.py:244-276`` starts exactly ONE worker, on port + 1, and lets the framework pick the GPU.

What this module adds, and nothing more: the worker of that protocol with the HIP plugins inside, pinned to ONE GPU
(``HIP_VISIBLE_DEVICES=<i>`` is set by the pool before the process imports torch), and a pool that starts one per visible GPU and
registers each with a front server.  With ``manga_translator`` importable the worker IS the reference's ``MangaShare`` (``make_worker``: the
plugins are added to its registries first, ``plugins.register()``); without it (this image has no OpenCV, so the orchestrator cannot be imported) the
same endpoints serve ``DenseStages`` — the three dense stages chained the way the orchestrator chains them
(``manga_translator.py:432-622``: detect -> OCR -> text-line merge -> mask refinement -> inpaint) — so the pool, the wire format and the
GPU pinning are testable here.  The product path has no CPU fallback: a worker without a GPU fails at load.
"""
# (no `from __future__ import annotations` here: FastAPI resolves the endpoint parameters' annotations at decoration time)
import asyncio
import io
import os
import pickle
import secrets
import subprocess
import sys
import time
from threading import Lock
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# ---- wire format (mode/share.py:63-66, server/sent_data_internal.py:44-66) -----------------------------------------------------------
STATUS_RESULT, STATUS_PROGRESS, STATUS_ERROR = 0, 1, 2


def frame(status: int, payload: bytes) -> bytes:
    """One chunk of the ``/execute`` stream: status (1 byte), payload length (4 bytes, big endian), payload."""
    if not 0 <= status <= 255:
        raise ValueError("status must fit one byte")
    return bytes([status]) + len(payload).to_bytes(4, "big") + payload


def parse_frames(buffer: bytes) -> Tuple[List[Tuple[int, bytes]], bytes]:
    """All complete frames at the head of ``buffer`` and the unconsumed rest (``handle_buffer``, sent_data_internal.py:44-58)."""
    out = []
    while len(buffer) >= 5:
        n = int.from_bytes(buffer[1:5], "big")
        if len(buffer) < 5 + n:
            break
        out.append((buffer[0], buffer[5:5 + n]))
        buffer = buffer[5 + n:]
    return out, buffer


# The reference's allow-list is by MODULE (mode/share.py:14-24) and admits all of ``builtins`` — eval, exec, getattr, __import__ … —
# so its "restricted" unpickler still executes whatever a request asks for.  Same modules here, but by (module, name): the container
# and scalar types a request body is made of, numpy's array reconstruction, PIL images, and the reference's config / geometry classes.
SAFE_PICKLE_MODULES = frozenset({   # modules whose classes are admitted wholesale: data-only packages of the reference and PIL (below)
    "manga_translator", "manga_translator.utils", "manga_translator.utils.generic", "manga_translator.config",
})
SAFE_PICKLE_NAMES = frozenset({
    ("builtins", n) for n in ("dict", "list", "tuple", "set", "frozenset", "int", "float", "complex", "bytes", "bytearray", "str", "bool", "slice",
                              "range", "object")
} | {("collections", "OrderedDict"), ("collections", "defaultdict"), ("collections", "deque")} | {
    (m, n) for m in ("numpy", "numpy.core.multiarray", "numpy._core.multiarray", "numpy.core.numeric", "numpy._core.numeric")
    for n in ("ndarray", "dtype", "_reconstruct", "scalar", "_frombuffer")
} | {("numpy.dtypes", n) for n in ("UInt8DType", "Int8DType", "Int16DType", "UInt16DType", "Int32DType", "UInt32DType", "Int64DType", "UInt64DType",
                                    "Float16DType", "Float32DType", "Float64DType", "BoolDType")})


class RestrictedUnpickler(pickle.Unpickler):
    def find_class(self, module: str, name: str):
        if (module, name) in SAFE_PICKLE_NAMES or module in SAFE_PICKLE_MODULES or module.startswith("PIL."):
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"Deserialization of {module}.{name} is not allowed")


def restricted_loads(data: bytes):
    return RestrictedUnpickler(io.BytesIO(data)).load()


# ---- which stages a request names ----------------------------------------------------------------------------------------------------
STAGE_MODES = ("fixed", "config")
FIXED_STAGE_KEYS = ("ctd", "48px", "lama_mpe")                # what a worker in "fixed" mode serves whatever the request says
DEFAULT_STAGE_KEYS = ("default", "48px", "lama_large")        # the reference's defaults (config.py:274, :312, :294)
SUPPORTED_STAGE_KEYS = {                                      # (section, field) -> the values this worker has a HIP plugin for
    ("detector", "detector"): ("default", "dbconvnext", "ctd"),
    ("ocr", "ocr"): ("48px", "48px_ctc", "32px"),
    ("inpainter", "inpainter"): ("lama_large", "lama_mpe", "default"),
}
# what a caller of ``stage_keys`` accepts beside them when it says so (``mocr=True``): a config-mode worker always does
OPTIONAL_STAGE_KEYS = {("ocr", "ocr"): ("mocr",)}
DETECTOR_FILTER_OPTIONS = ("det_rotate", "det_auto_rotate", "det_invert", "det_gamma_correct")   # DetectorConfig, config.py:280-286


def _field(section, name):
    """``section.name`` of a config section given as a dict, a pydantic model or a plain object; None when absent.  An enum member
    (the reference's Detector / Ocr / Inpainter are str enums) gives its value."""
    if section is None:
        return None
    v = section.get(name) if isinstance(section, dict) else getattr(section, name, None)
    return getattr(v, "value", v)


def detector_filter_options(config) -> Tuple[bool, bool, bool, bool]:
    """(invert, gamma_correct, rotate, auto_rotate) of a request — ``detector.det_invert`` / ``det_gamma_correct`` / ``det_rotate`` /
    ``det_auto_rotate`` (config.py:280-286), false where absent — in the order ``CommonDetector.detect`` takes them."""
    det = _as_dict(config).get("detector")
    return tuple(bool(_field(det, opt)) for opt in ("det_invert", "det_gamma_correct", "det_rotate", "det_auto_rotate"))


def stage_keys(config, detector_filters: bool = False, mocr: bool = False) -> Tuple[str, str, str]:
    """(detector, ocr, inpainter) a request's ``Config`` names: ``config.detector.detector``, ``config.ocr.ocr``,
    ``config.inpainter.inpainter``, each the reference's default where the field (or its section, or the config) is absent.  Raises
    ValueError, naming the key and the supported set, for a model this worker has no HIP plugin for (craft, paddle, none, mocr, sd,
    original, …) and for a detector filter option that is set (rotate / auto-rotate / invert / gamma-correct run inside the reference's
    ``CommonDetector.detect``, which the worker does not go through): a request is never served by something else silently.
    ``detector_filters``: the worker goes through the plugins' ``detect`` (``DenseStages(params={"detector_filters": True})``), so the
    four options are served and accepted.  ``mocr``: the caller has the manga-ocr plugin, so ``ocr.ocr = "mocr"``
    (``OPTIONAL_STAGE_KEYS``) is accepted too — every ``DenseStages`` in "config" mode passes it; the bare call keeps the set it had."""
    cfg = _as_dict(config)
    out = []
    for (section, name), default in zip(SUPPORTED_STAGE_KEYS, DEFAULT_STAGE_KEYS):
        v = _field(cfg.get(section), name)
        v = default if v is None else str(v)
        optional = OPTIONAL_STAGE_KEYS.get((section, name), ())
        if v not in SUPPORTED_STAGE_KEYS[(section, name)] and not (mocr and v in optional):
            extra = "" if mocr or not optional else f"; {', '.join(optional)} with stage_keys(..., mocr=True), as a config-mode worker calls it"
            served = SUPPORTED_STAGE_KEYS[(section, name)] + (optional if mocr else ())
            raise ValueError(f"{section}.{name} = {v!r} is not served by this worker (supported: {', '.join(served)}{extra})")
        out.append(v)
    for opt in DETECTOR_FILTER_OPTIONS:
        if not detector_filters and _field(cfg.get("detector"), opt):
            raise ValueError(f"detector.{opt} is set, and this worker does not apply it (supported: {opt} unset / false; the detector "
                             "runs on the page as it is)")
    return tuple(out)


SUPPORTED_COLORIZER_KEYS = ("none", "mc2")


def colorizer_options(config) -> Tuple[str, int, float]:
    """(colorizer, colorization_size, denoise_sigma) of a request: ``config.colorizer.colorizer`` / ``colorization_size`` /
    ``denoise_sigma`` (ColorizerConfig, config.py:301-307), an absent field (or section, or config) at the reference's default
    ("none", 576, 30).  Raises ValueError, naming the key and the supported set, for a colorizer this worker has no HIP plugin for
    (mc2 is the only one): a request is never served by something else silently."""
    col = _as_dict(config).get("colorizer")
    key = _field(col, "colorizer")
    key = "none" if key is None else str(key)
    if key not in SUPPORTED_COLORIZER_KEYS:
        raise ValueError(f"colorizer.colorizer = {key!r} is not served by this worker (supported: {', '.join(SUPPORTED_COLORIZER_KEYS)})")
    size, sigma = _field(col, "colorization_size"), _field(col, "denoise_sigma")
    return key, 576 if size is None else int(size), 30 if sigma is None else float(sigma)


# ---- what a worker hosts when the orchestrator itself cannot be imported ---------------------------------------------------------------
class DenseStages:
    """The three HIP plugins of one GPU, chained as ``MangaTranslator._translate`` chains the stages it owns
    (manga_translator.py:432-622): detection -> OCR of the detected lines -> text-line merge -> mask refinement -> inpainting.
    ``translate(image, config)`` has the worker method's name and argument names (``server/instance.py:19-20`` sends
    ``{"image": …, "config": …}`` to ``…/translate``); it returns the dense stages' results as plain numpy / builtins."""

    def __init__(self, params: Optional[dict] = None):
        self.params = dict(params or {})
        # "fixed" (the default): ctd + 48px + lama_mpe whatever a request names, as this worker has always served.  "config": the
        # stages the request's Config names (``stage_keys``), each plugin loaded at the first request that asks for it.
        self.stages = str(self.params.get("stages") or os.environ.get("MIT_SERVE_STAGES") or "fixed").strip().lower()
        if self.stages not in STAGE_MODES:
            raise ValueError(f"stages must be one of {STAGE_MODES} (params['stages'], --stages or MIT_SERVE_STAGES; got {self.stages!r})")
        # detector filters (off by default): the detector is called through the plugin's ``detect`` — CommonDetector.detect's rotate /
        # auto-rotate / invert / gamma-correct options and its border for pages with a side under 400 px — instead of ``infer``
        flag = self.params.get("detector_filters")
        if flag is None:
            flag = os.environ.get("MIT_SERVE_DETECTOR_FILTERS", "").strip().lower() in ("1", "true", "yes", "on")
        self.detector_filters = bool(flag)
        if self.detector_filters and self.stages != "config":
            raise ValueError("detector_filters needs stages='config' (params['detector_filters'], --detector-filters or "
                             "MIT_SERVE_DETECTOR_FILTERS with params['stages'], --stages or MIT_SERVE_STAGES = config): a worker in "
                             "'fixed' mode serves no request option of the detector")
        self._plugins: Dict[Tuple[str, str], object] = {}     # config mode: (stage, key) -> the loaded plugin
        # the stages self.det / self.ocr / self.inp are (to be) loaded for: ``_select`` sets them from each request
        self._keys = DEFAULT_STAGE_KEYS if self.stages == "config" else FIXED_STAGE_KEYS
        self.last_stage_keys: Optional[Tuple[str, str, str]] = None    # (detector, ocr, inpainter) that served the last request
        self._loaded = False
        self._coupled = None
        self.pages_batched = 0     # pages of translate_batch requests that went through one CoupledPageEngine.run with others
        self.pages_looped = 0      # pages of translate_batch requests that took the page loop (translate); last_batch_plan says why
        self.last_batch_plan: List[Tuple[List[int], str]] = []
        self.last_coupled_seconds: List[Dict[str, float]] = []
        self.up = None             # the upscaler plugin: loaded by the first request that asks for upscaling
        self.col = None            # the mc2 colorizer plugin: loaded by the first request (config mode) that names it
        self.last_colorizer: Optional[str] = None    # the colorizer that served the last request: "mc2" | "none"

    MC2_SYNTH_SEED = 0     # the seed of the synthetic colorizer weights (generator: this seed, FFDNet: this seed + 1)

    async def _load_colorizer(self):
        """The ``mc2`` plugin, on the first request whose ``config.colorizer.colorizer`` is ``mc2``: from the checkpoint under
        ``<model_dir>/colorization/manga-colorization-v2``, else seeded synthetic weights of ``mc2_schema`` (``MC2_SYNTH_SEED`` = 0 for
        the generator, 1 for FFDNet), identical in every worker."""
        if self.col is None:
            from . import mc2_schema, plugins as P, synth

            if self.params.get("model_dir"):
                col = P.HipMangaColorizer()
            else:
                seed = self.MC2_SYNTH_SEED
                col = P.HipMangaColorizer(weights={"generator": synth.synth_state_dict(mc2_schema.generator_schema(), seed=seed),
                                                   "denoiser": synth.synth_state_dict(mc2_schema.ffdnet_schema(), seed=seed + 1)})
            await col.load("cuda")
            self.col = col
        return self.col

    def _colorizer_options(self, cfg) -> Tuple[str, int, float]:
        """``colorizer_options`` of a request in "config" mode; a worker in "fixed" mode ignores the section, as it ignores every stage
        name."""
        return colorizer_options(cfg) if self.stages == "config" else ("none", 576, 30.0)

    async def _load_upscaler(self):
        """The ``4xultrasharp`` plugin, on the first request with ``config["upscale"]["upscale_ratio"]``: from the checkpoint under
        ``model_dir``, else seeded synthetic weights of the RRDBNet schema with ``esrgan_blocks`` blocks (default 23, the checkpoint's)."""
        if self.up is None:
            from . import esrgan_schema, plugins as P, synth

            if self.params.get("model_dir"):
                up = P.HipESRGANUpscaler()
            else:
                up = P.HipESRGANUpscaler(weights=synth.synth_state_dict(esrgan_schema.rrdbnet_schema(int(self.params.get("esrgan_blocks", 23)))))
            await up.load("cuda")
            self.up = up
        return self.up

    @staticmethod
    def _upscale_options(cfg: dict) -> Tuple[float, bool]:
        """(upscale_ratio or 0, revert_upscaling) of a request: the fields of the reference's UpscaleConfig (config.py:211-216)."""
        up = _as_dict(cfg.get("upscale")) if cfg.get("upscale") is not None else {}
        return (up.get("upscale_ratio") or 0), bool(up.get("revert_upscaling", False))

    def _select(self, config) -> Tuple[str, str, str]:
        """The stages that serve a request with this config — ``FIXED_STAGE_KEYS`` in "fixed" mode, ``stage_keys(config)`` in
        "config" mode — noted for ``_load`` (which brings ``self.det`` / ``self.ocr`` / ``self.inp`` to them) and in ``last_stage_keys``."""
        self._keys = stage_keys(config, self.detector_filters, mocr=True) if self.stages == "config" else FIXED_STAGE_KEYS
        self._colorizer_options(config)     # an unknown colorizer is refused here, with the other stage names
        self.last_stage_keys = self._keys
        return self._keys

    async def _load_selected(self):
        """Config mode: the plugins of ``self._keys``, each loaded once and kept by (stage, key) like the upscaler — from the checkpoint
        under ``model_dir``, else seeded synthetic weights (``pipeline.synthetic_stage_weights``), identical in every worker."""
        from . import pipeline, plugins as P

        classes = {("detector", "ctd"): P.HipComicTextDetector, ("detector", "default"): P.HipDefaultDetector,
                   ("detector", "dbconvnext"): P.HipDBConvNextDetector, ("ocr", "48px"): P.HipModel48pxOCR,
                   ("ocr", "48px_ctc"): P.HipModel48pxCTCOCR, ("ocr", "32px"): P.HipModel32pxOCR, ("ocr", "mocr"): P.HipModelMangaOCR,
                   ("inpainter", "lama_mpe"): P.HipLamaMPEInpainter, ("inpainter", "lama_large"): P.HipLamaLargeInpainter,
                   ("inpainter", "default"): P.HipAotInpainter}
        got = []
        for stage, key in zip(("detector", "ocr", "inpainter"), self._keys):
            if (stage, key) not in self._plugins:
                shared = {"ocr48": self._plugins[("ocr", "48px")]} if (stage, key) == ("ocr", "mocr") and ("ocr", "48px") in self._plugins else {}
                if self.params.get("model_dir"):
                    p = classes[(stage, key)](**shared)
                else:
                    d = int(self.params.get("dict_size", 512))
                    w = pipeline.synthetic_stage_weights(stage, key, dict_size=d)
                    kw = {"dictionary": ["<PAD>", "<S>", "</S>", "<SP>"] + [chr(0x4E00 + i) for i in range(d - 4)]} if stage == "ocr" else {}
                    if (stage, key) == ("ocr", "mocr"):   # the 48px model (shared where loaded) + the seeded stand-in of the model directory
                        mcfg, _, mgen, mvocab = pipeline.mocr_synthetic()
                        kw.update(vocab=mvocab, mocr_config=mcfg, generation=mgen, **shared)
                    p = classes[(stage, key)](weights=w, **kw)
                await p.load("cuda")
                self._plugins[(stage, key)] = p
            got.append(self._plugins[(stage, key)])
        self.det, self.ocr, self.inp = got

    async def _load(self):
        if self._loaded:
            if self.stages == "config":
                await self._load_selected()
            return
        import torch

        from . import pipeline, plugins as P

        if not torch.cuda.is_available():
            raise RuntimeError("a serving worker needs its GPU (HIP_VISIBLE_DEVICES selects it); there is no CPU path")
        ckpt = self.params.get("model_dir")
        if ckpt and not os.path.isdir(ckpt):
            raise FileNotFoundError(f"--model-dir {ckpt!r} is not a directory")
        if self.stages == "config":      # the plugins come with the requests (``_load_selected``); a worker loaded before its first
            if ckpt:                     # request brings up the reference's default stages, so that a missing checkpoint shows at start
                P.set_model_dir(os.path.abspath(ckpt))
            self.device_name = torch.cuda.get_device_name(0)
            await self._load_selected()
            self._loaded = True
            return
        if ckpt:      # real checkpoints in the reference's layouts (plugins._load_*_checkpoint), under <model_dir>/<detection|ocr|inpainting>/
            P.set_model_dir(os.path.abspath(ckpt))
            self.det, self.ocr, self.inp = P.HipComicTextDetector(), P.HipModel48pxOCR(), P.HipLamaMPEInpainter()
        else:         # no checkpoint offline: seeded synthetic weights of the reference architectures (synth.py), identical in every worker
            d = int(self.params.get("dict_size", 512))
            w = pipeline.synthetic_weights(dict_size=d)
            dictionary = ["<PAD>", "<S>", "</S>", "<SP>"] + [chr(0x4E00 + i) for i in range(d - 4)]
            self.det = P.HipComicTextDetector(weights=w)
            self.ocr = P.HipModel48pxOCR(weights=w["ocr48"], dictionary=dictionary)
            self.inp = P.HipLamaMPEInpainter(weights=w)
        for p in (self.det, self.ocr, self.inp):
            await p.load("cuda")
        self.device_name = torch.cuda.get_device_name(0)
        self._loaded = True

    async def translate(self, image, config=None):
        from . import mask_refinement as MR, textline_merge as TM

        cfg = _as_dict(config)
        keys = self._select(cfg)
        await self._load()
        page = np.ascontiguousarray(np.asarray(image.convert("RGB") if hasattr(image, "convert") else image, dtype=np.uint8))
        if page.ndim != 3 or page.shape[2] != 3:
            raise ValueError(f"image must be HxWx3 (got {page.shape})")
        ratio, revert = self._upscale_options(cfg)
        in_h, in_w = page.shape[:2]      # ctx.input.size: what revert_upscaling returns to, colorized or not (manga_translator.py:626-629)
        col_key, col_size, col_sigma = self._colorizer_options(cfg)
        self.last_colorizer = col_key
        page_dev = None
        if col_key == "mc2":   # colorize -> upscale -> detect -> ... (manga_translator.py:437-463): the colorized RGB image, at the
            import torch       # network's size, is the page of every later stage

            col = await self._load_colorizer()
            page_dev = col.engine.forward(torch.from_numpy(page).to(col.engine.device)[None], col_size, col_sigma)   # the one upload
            if not ratio:
                page = np.ascontiguousarray(page_dev[0].cpu().numpy())
        if ratio:   # the page is upscaled first and every later stage sees the upscaled page (manga_translator.py:453-465, :683)
            import torch

            up = await self._load_upscaler()
            src = page_dev.to(up.engine.device) if page_dev is not None else torch.from_numpy(page).to(up.engine.device)[None]
            page = np.ascontiguousarray(up.engine.upscale(src, ratio)[0].cpu().numpy())
        H, W = page.shape[:2]
        if self.detector_filters:   # CommonDetector.detect (detection/common.py:12-64): the request's filters, the small-page border
            tls, mask_raw, _ = await self.det.detect(page, *self._detector_args(cfg), *detector_filter_options(cfg))
        else:
            tls, mask_raw, _ = await self.det.infer(page, *self._detector_args(cfg))
        raw_in = cfg.get("mask_raw")        # a request may bring the raw text mask ([H, W] uint8) instead of the detector's: unlike "mask"
        if raw_in is not None:              # it goes through text-line merge + mask refinement
            mask_raw = np.ascontiguousarray(np.asarray(raw_in, dtype=np.uint8))
            if mask_raw.shape != (H, W):
                raise ValueError(f"mask_raw must be {H}x{W} (got {mask_raw.shape})")
        lines_in = cfg.get("textlines")     # a request may bring its own text lines (quads [n,4,2]) instead of the detector's
        if lines_in is not None:
            from .textline import Quadrilateral

            tls = [Quadrilateral(np.asarray(p, dtype=np.int64), "", 1.0) for p in lines_in]
        ocr = cfg.get("ocr", {})

        class _Cfg:   # OcrConfig.prob (config.py): None unless the request sets it — the plugin then keeps the reference's 0.2 (model_48px.py:104)
            prob = None if ocr.get("prob") is None else float(ocr["prob"])
            ignore_bubble = int(ocr.get("ignore_bubble", 0) or 0)     # (the ctc and 32px plugins read it from the config)
            use_mocr_merge = bool(ocr.get("use_mocr_merge", False))   # (refused by the mocr plugin when set)

        steps = int(ocr.get("max_seq_length", 255))
        if keys[1] == "48px":
            ocr_args = (_Cfg(), False, int(ocr.get("ignore_bubble", 0)), steps, bool(ocr.get("suppress_eos", False)))
        else:       # config mode: Model48pxCTCOCR._infer(image, textlines, config, verbose), Model32pxOCR's with max_seq_length after it
            if ocr.get("suppress_eos"):
                raise ValueError(f"ocr.suppress_eos is set, and ocr.ocr = {keys[1]!r} has no such option (supported: ocr.ocr = '48px')")
            if keys[1] == "48px_ctc" and ocr.get("max_seq_length") is not None:
                raise ValueError("ocr.max_seq_length is set, and ocr.ocr = '48px_ctc' has no step limit (supported: ocr.ocr = '48px', '32px')")
            if keys[1] == "mocr" and ocr.get("max_seq_length") is not None:
                raise ValueError("ocr.max_seq_length is set, and ocr.ocr = 'mocr' takes its length limit from the model's generation config "
                                 "(supported: ocr.ocr = '48px', '32px')")
            ocr_args = (_Cfg(), False) + ((steps,) if keys[1] == "32px" else ())
        lines = await self.ocr.infer(page, tls, *ocr_args) if tls else []
        lines = [l for l in lines if l.text.strip()]
        inp = cfg.get("inpainter", {})
        mask_in = cfg.get("mask")          # a request may bring the mask to inpaint ([H, W] uint8) instead of the refined detector mask
        if mask_in is not None:
            mask = np.ascontiguousarray(np.asarray(mask_in, dtype=np.uint8))
            if mask.shape != (H, W):
                raise ValueError(f"mask must be {H}x{W} (got {mask.shape})")
            out = await self.inp.infer(page, mask, None, int(inp.get("inpainting_size", 2048)))
        elif lines:
            regions = TM.dispatch_sync(lines, W, H)
            mask = MR.dispatch_sync(regions, page, mask_raw, "fit_text", int(cfg.get("mask_dilation_offset", 20)), 0, False, int(cfg.get("kernel_size", 3)))
            out = await self.inp.infer(page, mask, None, int(inp.get("inpainting_size", 2048)))
        else:   # no text: the orchestrator returns the page as it is (manga_translator.py:500-504)
            mask, out = np.zeros((H, W), np.uint8), page
        if ratio and revert and (W, H) != (in_w, in_h):   # ctx.result.resize(ctx.input.size): Pillow's default BICUBIC (manga_translator.py:626-629)
            import torch

            from . import imgproc

            dev = torch.from_numpy(np.ascontiguousarray(np.asarray(out, dtype=np.uint8))).to(self.up.engine.device)[None]
            out = imgproc.pil_resize_u8(dev, (in_w, in_h), "bicubic")[0].cpu().numpy()
        return {"textlines": [{"pts": np.asarray(l.pts).tolist(), "text": l.text, "prob": float(l.prob),
                               "fg": [int(l.fg_r), int(l.fg_g), int(l.fg_b)], "bg": [int(l.bg_r), int(l.bg_g), int(l.bg_b)]} for l in lines],
                "mask_raw": np.asarray(mask_raw), "mask": np.asarray(mask), "inpainted": np.asarray(out), "device": self.device_name,
                "visible_devices": os.environ.get("HIP_VISIBLE_DEVICES")}

    PER_PAGE_KEYS = ("textlines", "mask", "mask_raw")

    @classmethod
    def page_configs(cls, config, n: int) -> List[dict]:
        """The config of each page of a batch request: the shared config with ``config["per_page"][i]`` (a dict of ``textlines`` /
        ``mask`` / ``mask_raw``) laid over it."""
        cfg = dict(_as_dict(config))
        per_page = cfg.pop("per_page", None)
        if per_page is None:
            return [cfg] * n
        if len(per_page) != n:
            raise ValueError(f"per_page must have one entry per image ({len(per_page)} for {n} images)")
        out = []
        for i, pp in enumerate(per_page):
            pp = dict(pp or {})
            bad = sorted(set(pp) - set(cls.PER_PAGE_KEYS))
            if bad:
                raise ValueError(f"per_page[{i}]: only {', '.join(cls.PER_PAGE_KEYS)} may differ between the pages of a batch (got {', '.join(bad)})")
            out.append({**cfg, **pp})
        return out

    @staticmethod
    def plan_batches(shapes: Sequence[Tuple[int, int]], loop_reason: Sequence[Optional[str]], batch_size: int) -> List[Tuple[List[int], str]]:
        """How a batch request is served: [(page indices, "" for one coupled run | the reason for the page loop)].  Pages of equal
        (H, W) form a size group in request order, cut into runs of up to ``batch_size``; a run of one page, a page with a
        ``loop_reason`` of its own and everything when ``batch_size <= 1`` take the loop."""
        if batch_size <= 1:
            return [([i], "batch_size <= 1") for i in range(len(shapes))]
        plan, groups = [], {}
        for i, (hw, why) in enumerate(zip(shapes, loop_reason)):
            if why:
                plan.append(([i], why))
            else:
                groups.setdefault(tuple(hw), []).append(i)
        for idx in groups.values():
            for a in range(0, len(idx), batch_size):
                run = idx[a:a + batch_size]
                plan.append((run, "" if len(run) > 1 else "alone in its size group"))
        return sorted(plan, key=lambda e: e[0][0])

    def _detector_args(self, cfg: dict) -> Tuple[int, float, float, float]:
        """(detect_size, text_threshold, box_threshold, unclip_ratio) of a request: DetectorConfig's fields (config.py:274-290), an
        absent one at the reference's default in "config" mode (2048, 0.5, 0.7, 2.3); "fixed" mode keeps its 1024 for the size (the
        ctd detector ignores all four)."""
        det = _as_dict(cfg.get("detector")) if cfg.get("detector") is not None else {}
        size = det.get("detection_size")
        return (int(size) if size is not None else (2048 if self.stages == "config" else 1024), float(det.get("text_threshold", 0.5)),
                float(det.get("box_threshold", 0.7)), float(det.get("unclip_ratio", 2.3)))

    def _loop_reason(self, page: np.ndarray, cfg: dict) -> Optional[str]:
        """Why a page cannot join a coupled run (None: it can)."""
        from . import rearrange

        if page.ndim != 3 or page.shape[2] != 3:
            return "not HxWx3"
        if self._colorizer_options(cfg)[0] != "none":
            return "colorizer"      # the coupled engine starts at the detector
        if self._upscale_options(cfg)[0]:
            return "upscale"
        if self.detector_filters and (any(detector_filter_options(cfg)) or min(page.shape[:2]) < 400):
            return "detector filters"      # the coupled engine calls the network on the page as it is
        if self._keys[1] != "48px":     # (config mode only) the coupled engine is written around the 48px model's pooled beam search
            return f"ocr.ocr = {self._keys[1]} is not in the coupled engine"
        # a strip is one at the size its detector tiles at: 1024 for ctd whatever the request says (ctd.py:84), detection_size for DBNet
        size = 1024 if self._keys[0] == "ctd" else self._detector_args(cfg)[0]
        if rearrange.plan(page.shape[0], page.shape[1], size) is not None and not getattr(self._coupled_engine(), "takes_strips", False):
            if self._keys[0] != "ctd":
                return f"webtoon strip with detector.detector = {self._keys[0]} (DBNet strips are not batched)"
            return "webtoon strip (rearranged detection)"      # (the engine is asked only when the page is a strip)
        if int(_as_dict(cfg.get("ocr", {})).get("ignore_bubble", 0)):
            return "ocr.ignore_bubble is not implemented by the coupled engine"
        return None

    def _inpaint_precision(self) -> str:
        """What the page loop's ``self.inp.infer(page, mask, None, ...)`` runs in (the plugin's ``precision`` option, ``MIT_LAMA_PRECISION``
        by default): a batch follows it.  An inpainter without the option is fp32."""
        fn = getattr(getattr(self, "inp", None), "precision_for", None)
        return fn(None) if fn is not None else "fp32"

    def _coupled_engine(self):
        from . import coupled

        engines = (self.det.engine, self.ocr.engine, self.inp.engine)
        if self._coupled is None or self._coupled[0] != tuple(id(e) for e in engines):
            if self._coupled is not None:
                self._coupled[1].close()
            self._coupled = (tuple(id(e) for e in engines), coupled.CoupledPageEngine.from_engines(*engines, self.ocr.dictionary))
        return self._coupled[1]

    async def translate_batch(self, images, config=None, batch_size: int = 1):
        """``/simple_execute/translate_batch`` (server/instance.py:22-26 sends ``{"images", "config", "batch_size"}``).  With
        ``batch_size`` > 1 the pages of equal size are grouped, up to ``batch_size`` per group; each group is uploaded once and goes
        through ONE ``CoupledPageEngine.run`` on the engines the loaded plugins own.  Results come back in request order, each the
        dict ``translate`` returns for that page with ``config`` and its ``config["per_page"][i]`` overlay.  A page alone in its size
        group and a request option the coupled engine does not implement take the page loop (``translate``), as every page does
        with ``batch_size <= 1``; webtoon strips of equal size batch like any other page when the coupled engine has the
        rearranged detection (``takes_strips``, which ``CoupledPageEngine`` sets), else they take the loop as well; ``last_batch_plan`` and the ``pages_batched`` / ``pages_looped`` counters of
        ``device_info`` say which way the pages went."""
        import torch

        images = list(images)
        cfgs = self.page_configs(config, len(images))
        self._select(cfgs[0] if cfgs else config)     # (the pages of a request share everything but textlines / mask / mask_raw)
        self.last_colorizer = self._colorizer_options(cfgs[0] if cfgs else config)[0]
        await self._load()
        pages = [np.ascontiguousarray(np.asarray(im.convert("RGB") if hasattr(im, "convert") else im, dtype=np.uint8)) for im in images]
        plan = self.plan_batches([p.shape[:2] for p in pages], [self._loop_reason(p, c) for p, c in zip(pages, cfgs)], int(batch_size))
        self.last_batch_plan = plan
        self.last_coupled_seconds = []      # CoupledResult.seconds of each coupled run of this request
        results: List[Optional[dict]] = [None] * len(images)
        for idx, why in plan:
            if why:
                for i in idx:
                    results[i] = await self.translate(pages[i], cfgs[i])
                self.pages_looped += len(idx)
                continue
            cfg = cfgs[idx[0]]      # everything but textlines / mask / mask_raw is shared by the pages of a request
            ocr, inp = _as_dict(cfg.get("ocr", {})), _as_dict(cfg.get("inpainter", {}))
            H, W = pages[idx[0]].shape[:2]
            for i in idx:
                m = cfgs[i].get("mask")
                if m is not None and np.asarray(m).shape != (H, W):
                    raise ValueError(f"mask must be {H}x{W} (got {np.asarray(m).shape})")
            eng = self._coupled_engine()
            pages_dev = torch.from_numpy(np.stack([pages[i] for i in idx])).to(eng.device)      # one upload per group
            det_kw = {}
            if self.stages == "config":     # the detector's parameters travel with the run (a DBNet engine uses them, ctd ignores them)
                det_kw = dict(zip(("detect_size", "text_threshold", "box_threshold", "unclip_ratio"), self._detector_args(cfg)))
                for i in idx:               # the page loop's check (translate): a request's raw mask is page-sized
                    m = cfgs[i].get("mask_raw")
                    if m is not None and np.asarray(m).shape != (H, W):
                        raise ValueError(f"mask_raw must be {H}x{W} (got {np.asarray(m).shape})")
            r = eng.run(pages_dev, max_seq_length=int(ocr.get("max_seq_length", 255)), suppress_eos=bool(ocr.get("suppress_eos", False)),
                        prob_threshold=0.2 if ocr.get("prob") is None else float(ocr["prob"]),
                        textlines=[cfgs[i].get("textlines") for i in idx], mask_raw=[cfgs[i].get("mask_raw") for i in idx],
                        mask=[cfgs[i].get("mask") for i in idx], mask_dilation_offset=int(cfg.get("mask_dilation_offset", 20)),
                        kernel_size=int(cfg.get("kernel_size", 3)), inpainting_size=int(inp.get("inpainting_size", 2048)),
                        precision=self._inpaint_precision(), **det_kw)
            self.last_coupled_seconds.append(dict(r.seconds))
            # (a DBNet run's raw masks have the detector's size, and come as a per-page list once a request replaced some of them)
            mask_raw = [m.cpu().numpy() for m in r.mask_raw] if isinstance(r.mask_raw, list) else r.mask_raw.cpu().numpy()
            mask, out = r.mask.cpu().numpy(), r.inpainted.cpu().numpy()
            for k, i in enumerate(idx):
                results[i] = {"textlines": [{"pts": np.asarray(l.pts).tolist(), "text": l.text, "prob": float(l.prob),
                                             "fg": [int(l.fg_r), int(l.fg_g), int(l.fg_b)], "bg": [int(l.bg_r), int(l.bg_g), int(l.bg_b)]}
                                            for l in r.textlines[k]],
                              "mask_raw": mask_raw[k], "mask": mask[k], "inpainted": out[k], "device": self.device_name,
                              "visible_devices": os.environ.get("HIP_VISIBLE_DEVICES")}
            self.pages_batched += len(idx)
        return results

    async def device_info(self, image=None, config=None):   # (the executor's send calls always carry both attributes)
        await self._load()
        import torch

        return {"device": self.device_name, "visible_devices": os.environ.get("HIP_VISIBLE_DEVICES"), "n_visible": torch.cuda.device_count(),
                "pid": os.getpid(), "pages_batched": self.pages_batched, "pages_looped": self.pages_looped, "stages": self.stages,
                "last_stage_keys": self.last_stage_keys, "last_colorizer": self.last_colorizer}


def _as_dict(config) -> dict:
    if config is None:
        return {}
    if isinstance(config, dict):
        return config
    for m in ("model_dump", "dict"):
        if hasattr(config, m):
            return getattr(config, m)()
    return dict(vars(config))


def _make_engine(params: dict):
    """The object whose methods the worker exposes: the reference's MangaTranslator (HIP plugins registered) when it imports,
    else DenseStages; MIT_SERVE_ENGINE=module:callable substitutes another factory (protocol tests without a GPU)."""
    hook = os.environ.get("MIT_SERVE_ENGINE")
    if hook:
        import importlib

        mod, _, fn = hook.partition(":")
        return getattr(importlib.import_module(mod), fn)(params)
    try:
        from manga_translator import MangaTranslator  # type: ignore  # noqa: F401
    except Exception:
        return DenseStages(params)
    from . import plugins as P

    P.register()    # ctd_hip / 48px_hip / lama_mpe_hip … become detector / ocr / inpainter choices of Config
    return MangaTranslator(params)


def make_worker(params: dict):
    """The worker process's server object.  With the reference importable it IS the reference's ``MangaShare`` (mode/share.py:47-174) —
    its endpoints, its unpickler, its ``MangaTranslator`` — and this package only adds its plugins to the registries first
    (``plugins.register()``: ``ctd_hip`` / ``48px_hip`` / ``lama_mpe_hip`` … become choices of ``Config``).  Only where the reference cannot
    be imported (this image: no OpenCV) the stand-alone mirror below serves the same protocol around ``DenseStages``."""
    if not os.environ.get("MIT_SERVE_ENGINE"):
        try:
            from manga_translator.mode.share import MangaShare  # type: ignore
        except Exception:
            MangaShare = None
        if MangaShare is not None:
            from . import plugins as P

            P.register()
            if params.get("model_dir"):
                P.set_model_dir(os.path.abspath(params["model_dir"]))
            return MangaShare(params)
    return HipShareWorker(params)


class HipShareWorker:
    """Stand-alone mirror of ``MangaShare`` (mode/share.py:47-174) around ``_make_engine``: same endpoints, nonce rule, one-request lock
    and stream framing — pinned to the reference's own CLIENT (server/sent_data_internal.py) by tests/test_serve.py."""

    def __init__(self, params: Optional[dict] = None):
        params = dict(params or {})
        self.manga = _make_engine(params)
        self.host = params.get("host", "127.0.0.1")
        self.port = int(params.get("port", 5003))
        nonce = params.get("nonce", None)
        if not nonce:
            nonce = secrets.token_hex(16)
        if nonce == "None":   # the reference's way of switching the check off: only for a loopback listener (a request body is a pickle)
            if self.host not in ("127.0.0.1", "localhost", "::1"):
                raise ValueError(f"nonce 'None' (no authentication) is refused on host {self.host!r}: bind to 127.0.0.1 or set a nonce")
            nonce = None
        self.nonce = nonce
        self.lock = Lock()
        self.progress_queue: Optional[asyncio.Queue] = None
        if hasattr(self.manga, "add_progress_hook"):
            async def hook(state: str, finished: bool):
                await self.progress_queue.put(frame(STATUS_PROGRESS, state.encode("utf-8")))
                await asyncio.sleep(0)

            self.manga.add_progress_hook(hook)

    def app(self):
        from fastapi import FastAPI, HTTPException, Path, Request, Response
        from starlette.responses import StreamingResponse

        app = FastAPI()
        self.progress_queue = asyncio.Queue()

        def check_nonce(request: Request):
            if self.nonce and request.headers.get("X-Nonce") != self.nonce:
                raise HTTPException(401, detail="Nonce does not match")

        def check_lock():
            if not self.lock.acquire(blocking=False):
                raise HTTPException(status_code=429, detail="some Method is already being executed.")

        def get_fn(method_name: str):
            if method_name.startswith("_"):
                raise HTTPException(status_code=403, detail="These functions are not allowed to be executed remotely")
            method = getattr(self.manga, method_name, None)
            if not callable(method):
                raise HTTPException(status_code=404, detail="Method not found")
            return method

        async def call(method, attr):
            return await method(**attr) if asyncio.iscoroutinefunction(method) else method(**attr)

        @app.get("/is_locked")
        async def is_locked():
            return {"locked": self.lock.locked()}

        @app.post("/simple_execute/{method_name}")
        async def simple_execute(request: Request, method_name: str = Path(...)):
            check_nonce(request)
            method = get_fn(method_name)
            try:
                attr = restricted_loads(await request.body())
            except Exception as e:
                raise HTTPException(status_code=400, detail=f"bad request body: {e}")
            check_lock()
            try:
                return Response(content=pickle.dumps(await call(method, attr)), media_type="application/octet-stream")
            except Exception as e:  # noqa: BLE001 - reported to the caller as the reference does
                raise HTTPException(status_code=500, detail=str(e))
            finally:
                self.lock.release()

        @app.post("/execute/{method_name}")
        async def execute(request: Request, method_name: str = Path(...)):
            check_nonce(request)
            method = get_fn(method_name)
            try:
                attr = restricted_loads(await request.body())
            except Exception as e:
                raise HTTPException(status_code=400, detail=f"bad request body: {e}")
            check_lock()
            while not self.progress_queue.empty():   # progress frames of earlier /simple_execute calls (nobody read them) do not belong
                self.progress_queue.get_nowait()     # to this stream

            async def run():
                try:
                    await self.progress_queue.put(frame(STATUS_RESULT, pickle.dumps(await call(method, attr))))
                except Exception as e:  # noqa: BLE001
                    await self.progress_queue.put(frame(STATUS_ERROR, str(e).encode("utf-8")))
                finally:
                    self.lock.release()

            async def stream():
                while True:
                    chunk = await self.progress_queue.get()
                    yield chunk
                    if chunk[0] != STATUS_PROGRESS:
                        break

            asyncio.create_task(run())
            return StreamingResponse(stream(), media_type="application/octet-stream")

        return app

    async def listen(self):
        import uvicorn

        server = uvicorn.Server(uvicorn.Config(self.app(), host=self.host, port=self.port, log_level="warning"))
        await server.serve()


# ---- the pool: one worker per GPU, and the front server's view of it -----------------------------------------------------------------
class ExecutorInstance:
    """``server/instance.py:10-33``: a worker's address and its busy flag, with the two send calls."""

    def __init__(self, ip: str, port: int, nonce: Optional[str] = None, gpu: Optional[int] = None):
        self.ip, self.port, self.busy, self.nonce, self.gpu = ip, int(port), False, nonce, gpu

    @property
    def url(self) -> str:
        return f"http://{self.ip}:{self.port}"

    def _headers(self) -> Dict[str, str]:
        return {"X-Nonce": self.nonce} if self.nonce else {}

    async def sent(self, image, config, method: str = "translate"):
        import aiohttp

        data = pickle.dumps({"image": image, "config": config})
        async with aiohttp.ClientSession() as s:
            async with s.post(f"{self.url}/simple_execute/{method}", data=data, headers=self._headers()) as r:
                body = await r.read()
                if r.status != 200:
                    raise RuntimeError(f"worker {self.url}: HTTP {r.status}: {body[:300]!r}")
                return pickle.loads(body)   # our own worker's reply

    async def sent_batch(self, images, config, batch_size: int = 1):
        """``ExecutorInstance.sent_batch`` (server/instance.py:22-26)."""
        import aiohttp

        data = pickle.dumps({"images": list(images), "config": config, "batch_size": int(batch_size)})
        async with aiohttp.ClientSession() as s:
            async with s.post(f"{self.url}/simple_execute/translate_batch", data=data, headers=self._headers()) as r:
                body = await r.read()
                if r.status != 200:
                    raise RuntimeError(f"worker {self.url}: HTTP {r.status}: {body[:300]!r}")
                return pickle.loads(body)

    async def sent_stream(self, image, config, sender: Callable[[int, bytes], None], method: str = "translate"):
        import aiohttp

        data = pickle.dumps({"image": image, "config": config})
        async with aiohttp.ClientSession() as s:
            async with s.post(f"{self.url}/execute/{method}", data=data, headers=self._headers()) as r:
                if r.status != 200:
                    raise RuntimeError(f"worker {self.url}: HTTP {r.status}: {(await r.read())[:300]!r}")
                buf = b""
                async for chunk in r.content.iter_any():
                    frames, buf = parse_frames(buf + chunk)
                    for st, payload in frames:
                        sender(st, payload)


class Executors:
    """``server/instance.py:35-65``: the table of workers; ``find_executor`` hands out a free one (waiting for a release when all are
    busy), ``free_executor`` returns it."""

    def __init__(self):
        self.list: List[ExecutorInstance] = []
        self.lock = asyncio.Lock()
        self.event = asyncio.Event()

    def register(self, instance: ExecutorInstance):
        self.list.append(instance)

    def free_executors(self) -> int:
        return len([x for x in self.list if not x.busy])

    async def find_executor(self) -> ExecutorInstance:
        async with self.lock:
            while True:
                inst = next((x for x in self.list if not x.busy), None)
                if inst is not None:
                    inst.busy = True
                    return inst
                await self.event.wait()

    async def free_executor(self, instance: ExecutorInstance):
        instance.busy = False
        self.event.set()
        self.event.clear()


def visible_gpus() -> List[Tuple[str, str]]:
    """The devices a pool starts workers on, as (environment variable, value) pairs that pin ONE process to ONE of them.
    HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES entries are HIP ordinals (within whatever ROCR_VISIBLE_DEVICES leaves); an entry of
    ROCR_VISIBLE_DEVICES (index or GPU-UUID) is a ROCr-level name and can only be narrowed at that level — ``HIP_VISIBLE_DEVICES=<entry>``
    beside an inherited ROCR list would index INTO the filtered list and find nothing.  With none set: 0 … n-1 as rocm reports them
    (counted in a child process so that THIS process never initialises a GPU it would then keep memory on)."""
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v:
            return [("HIP_VISIBLE_DEVICES", x) for x in v.split(",") if x != ""]
    v = os.environ.get("ROCR_VISIBLE_DEVICES")
    if v:
        return [("ROCR_VISIBLE_DEVICES", x) for x in v.split(",") if x != ""]
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True, timeout=600)
    n = int(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 and out.stdout.strip() else 0
    return [("HIP_VISIBLE_DEVICES", str(i)) for i in range(n)]


def pin_env(env: Dict[str, str], gpu) -> Dict[str, str]:
    """``env`` narrowed to one device: ``gpu`` is a (variable, value) pair of ``visible_gpus()`` or a bare HIP ordinal."""
    var, val = gpu if isinstance(gpu, tuple) else ("HIP_VISIBLE_DEVICES", str(gpu))
    env = dict(env)
    env.pop("CUDA_VISIBLE_DEVICES", None)
    if var == "ROCR_VISIBLE_DEVICES":
        env.pop("HIP_VISIBLE_DEVICES", None)     # the one device ROCr leaves is HIP ordinal 0
        env["ROCR_VISIBLE_DEVICES"] = str(val)
    else:
        env["HIP_VISIBLE_DEVICES"] = str(val)    # an inherited ROCR_VISIBLE_DEVICES stays: the ordinal counts within it
    return env


class WorkerPool:
    """Starts one worker process per GPU — ``python -m manga_image_translator_amd.serve worker --port P`` with ``HIP_VISIBLE_DEVICES=<gpu>`` —
    on consecutive ports from ``base_port`` (the reference's single worker sits on port + 1, server/main.py:288), waits until each answers
    ``/is_locked``, and can enter them into a front server's table (``POST /register``, server/main.py:45-50)."""

    def __init__(self, gpus: Optional[Sequence[str]] = None, host: str = "127.0.0.1", base_port: int = 5003, nonce: Optional[str] = None,
                 worker_args: Sequence[str] = (), env: Optional[Dict[str, str]] = None):
        self.gpus = list(gpus) if gpus is not None else visible_gpus()
        if not self.gpus:
            raise RuntimeError("no GPU visible: a worker pool needs at least one (HIP_VISIBLE_DEVICES)")
        self.host, self.base_port = host, int(base_port)
        self.nonce = nonce or secrets.token_hex(16)
        self.worker_args, self.env = list(worker_args), dict(env or {})
        self.procs: List[subprocess.Popen] = []
        self.executors = Executors()

    def start(self, timeout: float = 900.0) -> "WorkerPool":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        for k, gpu in enumerate(self.gpus):
            env = dict(os.environ)
            env.update(self.env)
            env = pin_env(env, gpu)                          # the worker sees exactly one device, as cuda:0
            env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
            port = self.base_port + k
            cmd = [sys.executable, "-m", "manga_image_translator_amd.serve", "worker", "--host", self.host, "--port", str(port),
                   "--nonce", self.nonce, *self.worker_args]
            self.procs.append(subprocess.Popen(cmd, env=env, cwd=root))
            self.executors.register(ExecutorInstance(self.host, port, self.nonce, gpu=k))
        self._wait_ready(timeout)
        return self

    def _wait_ready(self, timeout: float):
        import urllib.request

        t_end = time.time() + timeout
        for inst, proc in zip(self.executors.list, self.procs):
            while True:
                if proc.poll() is not None:
                    self.stop()
                    raise RuntimeError(f"worker on port {inst.port} exited with code {proc.returncode} before it was ready")
                try:
                    with urllib.request.urlopen(f"{inst.url}/is_locked", timeout=2) as r:
                        if r.status == 200:
                            break
                except OSError:
                    pass
                if time.time() > t_end:
                    self.stop()
                    raise TimeoutError(f"worker on port {inst.port} did not come up within {timeout:.0f} s")
                time.sleep(0.25)

    def register_with(self, server_url: str, server_nonce: str):
        """Enter every worker into a running front server (``python server/main.py``): what ``start_translator_client_proc`` does for
        its one local worker, done for one per GPU.  The server takes the ip from the connection and the port from the body."""
        import json
        import urllib.request

        for inst in self.executors.list:
            req = urllib.request.Request(server_url.rstrip("/") + "/register", data=json.dumps({"ip": inst.ip, "port": inst.port}).encode(),
                                         headers={"Content-Type": "application/json", "X-Nonce": server_nonce}, method="POST")
            with urllib.request.urlopen(req, timeout=30) as r:
                if r.status != 200:
                    raise RuntimeError(f"register of {inst.url} failed: HTTP {r.status}")

    async def run(self, image, config=None, method: str = "translate"):
        """One request on whichever worker is free (the front server's ``find_executor`` -> ``sent`` -> ``free_executor`` cycle)."""
        inst = await self.executors.find_executor()
        try:
            return await inst.sent(image, config, method)
        finally:
            await self.executors.free_executor(inst)

    async def map(self, images: Sequence, config=None) -> List:
        """All images over the pool, as many in flight as there are workers; results in the order of ``images``."""
        return list(await asyncio.gather(*[self.run(im, config) for im in images]))

    def stop(self):
        for p in self.procs:
            if p.poll() is None:
                p.terminate()
        for p in self.procs:
            try:
                p.wait(timeout=20)
            except subprocess.TimeoutExpired:
                p.kill()
        self.procs = []

    def __enter__(self):
        return self.start()

    def __exit__(self, *exc):
        self.stop()


def _main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(prog="python -m manga_image_translator_amd.serve")
    sub = ap.add_subparsers(dest="cmd", required=True)
    w = sub.add_parser("worker", help="one shared-mode worker on the GPU HIP_VISIBLE_DEVICES names (mode/share.py)")
    w.add_argument("--host", default="127.0.0.1")
    w.add_argument("--port", type=int, default=5003)
    w.add_argument("--nonce", default=os.getenv("MT_WEB_NONCE") or None)
    w.add_argument("--model-dir", default=None, help="directory with the reference's checkpoints; synthetic weights without it")
    w.add_argument("--dict-size", type=int, default=512)
    w.add_argument("--esrgan-blocks", type=int, default=23, help="RRDB blocks of the synthetic upscaler weights (without --model-dir)")
    w.add_argument("--stages", choices=STAGE_MODES, default=None,
                   help="fixed: ctd + 48px + lama_mpe whatever a request names (default); config: the detector / ocr / inpainter the request's "
                        "Config names, loaded at first use (MIT_SERVE_STAGES sets the default)")
    w.add_argument("--detector-filters", action="store_true", default=None,
                   help="with --stages config: call the detector through CommonDetector.detect's filters (det_rotate / det_auto_rotate / "
                        "det_invert / det_gamma_correct and the border for pages under 400 px); off by default "
                        "(MIT_SERVE_DETECTOR_FILTERS=1 sets the default)")
    w.add_argument("--lazy", action="store_true", help="load the plugins at the first request instead of before listening (default: before, so "
                                                      "that a worker without its GPU or its checkpoints never reports ready)")
    w.add_argument("--preload", action="store_true", help=argparse.SUPPRESS)   # the default since round 6
    a = ap.parse_args(argv)
    params = {"host": a.host, "port": a.port, "nonce": a.nonce, "model_dir": a.model_dir, "dict_size": a.dict_size, "esrgan_blocks": a.esrgan_blocks,
              "use_gpu": True, "stages": a.stages, "detector_filters": a.detector_filters}
    worker = make_worker(params)
    loop = asyncio.new_event_loop()
    asyncio.set_event_loop(loop)
    if not a.lazy and hasattr(worker.manga, "_load"):    # DenseStages: GPU visible? checkpoints found? — fail before /is_locked answers
        loop.run_until_complete(worker.manga._load())
    loop.run_until_complete(worker.listen())
    return 0


if __name__ == "__main__":
    sys.exit(_main())
