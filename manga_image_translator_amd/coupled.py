"""The COUPLED page path: detector -> boxes -> refine_mask -> OCR -> text-line merge -> mask refinement -> inpainting, for a batch
of pages, in the order and with the arguments the reference's orchestrator uses for one page
(/root/reference/manga_translator/manga_translator.py:432-622: ``_run_detection`` :1208, ``_run_ocr`` :745,
``_run_textline_merge`` :772, ``_run_mask_refinement`` :1356-1358 with ``mask_dilation_offset`` = 20 and ``kernel_size`` = 3
(config.py:342-344), ``_run_inpainting`` :1360-1364).

``pipeline.PageEngine`` times the three dense stages fed independently; here each stage consumes what the previous one
produced, so the glue between them — box extraction (a4), the detector's ``refine_mask`` (a5), the merge graph (f3), the mask
refinement with its DenseCRF (f1) — is inside the measured path.  Dense work runs batched on the GPU; the per-page host steps
(contours -> boxes in native C++, direction vote, merge graph, component labelling) run on a thread pool (ctypes / numpy / scipy
release the GIL) while the stream keeps executing.  A batch larger than one group of 16 pages flows through three stage threads
(detector + boxes + refine_mask | OCR | merge + mask refinement + LaMa) that work on different groups at the same time (``run(group=)``).

``CoupledPageEngine`` itself builds the ctd detector, the 48px OCR and a LaMa; ``from_engines`` takes the engines loaded plugins own,
and there the detector may be of the DBNet kind (``default`` / ``dbconvnext``: ``plugins.dbnet_detect_pages``, no ``refine_mask``, the
raw mask at the detector's own size) and the inpainter a LaMa of either depth or the AOT engine.

Random-init networks do not detect text (their sigmoid maps hover around 0.5 everywhere), so a benchmark passes ``inject``: per-page
maps a trained head would have produced for the synthetic page (``synthetic_head_outputs``); they replace the network's own outputs
AFTER the network has run (its cost is paid in full) — a stand-in for trained weights, never part of the product path (the plugins do
not know about it).
"""
from __future__ import annotations

import concurrent.futures as cf
import math
import os
import threading
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ctd, hostglue, imgproc, lama, mask_refinement as MR, ocr48, rearrange, textline_merge as TM
from .textline import Quadrilateral

BOX_THRESH = 0.6          # ctd.py:157-159
MASK_DILATION_OFFSET = 20  # config.py:344
KERNEL_SIZE = 3            # config.py:342


@dataclass
class CoupledResult:
    textlines: List[List[Quadrilateral]]      # per page: the detector's lines with OCR text / prob / colours set
    regions: List[list]                        # per page: TextBlocks of the merge
    mask: torch.Tensor                         # u8 [B,H,W] final inpainting mask (device)
    inpainted: torch.Tensor                    # u8 [B,H,W,3] (device)
    seconds: Dict[str, float] = field(default_factory=dict)   # host wall time per phase (the GPU runs asynchronously underneath)
    # the mask the refinement started from (the detector's, or the request's): u8 [B,H,W] from the ctd engine (its refined mask, page
    # size); u8 [B,h',w'] from a DBNet engine (its raw mask at the detector's own size, which mask refinement resizes), or a list of B
    # such masks when a request brought page-sized ones for some pages
    mask_raw: Optional[object] = None


class RawMasks(list):
    """Per-page raw masks of unequal sizes (a DBNet run in which a request replaced some pages' masks), with what ``merge_and_refine``
    asks of the one-tensor form: the event recorded behind the last writer, and ``record_stream``."""
    mit_ready_event = None

    def record_stream(self, stream):
        for m in self:
            m.record_stream(stream)


def is_dbnet_engine(engine) -> bool:
    """Whether a detector engine is one of the DBNet kind (``DbnetEngine`` / ``DbconvnextEngine``: ``forward`` -> (db, mask), the page
    function ``plugins.dbnet_detect_pages`` around it) rather than the ctd engine."""
    from . import dbconvnext, dbnet

    return isinstance(engine, (dbnet.DbnetEngine, dbconvnext.DbconvnextEngine))


# DefaultDetector's parameters as the reference's Config sets them (config.py:276-290); ``run`` hands them to a DBNet engine only
DETECT_SIZE, TEXT_THRESHOLD, DET_BOX_THRESHOLD, UNCLIP_RATIO = 2048, 0.5, 0.7, 2.3


def synthetic_head_outputs(page: np.ndarray, quads: np.ndarray, map_hw, shrink_ratio: float = 0.4, unclip_ratio: float = 1.5):
    """What a TRAINED ctd head would emit for a synthetic page (benchmark stand-in for weights, see the module docstring):
    * the DB shrink map [h, w] float32: 0.9 inside every text box shrunk so that SegDetectorRepresenter's unclip
      (distance = area * 1.5 / perimeter, db_utils.py:150-155) grows it back to the box — d solves d * 2(w + h - 4d) = 1.5 (w - 2d)(h - 2d);
    * the text mask [h, w] uint8: 255 on the dark (glyph) pixels inside the boxes.
    ``map_hw`` = the network's un-padded output size (page / 2 for a 2048 x 1456 page)."""
    H, W = page.shape[:2]
    h, w = map_hw
    sy, sx = h / H, w / W
    prob = np.zeros((h, w), np.float32)
    box = np.zeros((H, W), bool)
    for q in np.asarray(quads):
        x0, y0, x1, y1 = q[:, 0].min() * sx, q[:, 1].min() * sy, q[:, 0].max() * sx, q[:, 1].max() * sy
        bw, bh = x1 - x0, y1 - y0
        S = bw + bh
        disc = 25 * S * S - 84 * bw * bh
        d = (5 * S - math.sqrt(max(disc, 0.0))) / 28 if bw > 0 and bh > 0 else 0.0
        d = min(d, 0.45 * min(bw, bh))
        ya, yb, xa, xb = int(round(y0 + d)), int(round(y1 - d)), int(round(x0 + d)), int(round(x1 - d))
        if yb > ya and xb > xa:
            prob[ya:yb, xa:xb] = 0.9
        box[int(q[:, 1].min()):int(q[:, 1].max()), int(q[:, 0].min()):int(q[:, 0].max())] = True
    glyph = ((page.min(-1) < 128) & box).astype(np.uint8) * 255
    mask = imgproc.resize_u8_host(glyph, (w, h))
    mask[mask > 0] = 255
    return prob, mask


_STAGE_OF = {"detect+boxes+refine_mask": "det", "ocr": "ocr", "textline_merge+mask_refinement": "tail", "inpaint (enqueue)": "tail"}


class CoupledPageEngine:
    """Owns the stage engines of one GPU and a host thread pool."""

    takes_strips = True   # detect() has det_rearrange_forward's branch: a batch of equal webtoon strips is one coupled run (serve.py)

    def __init__(self, weights: Dict[str, Dict[str, torch.Tensor]], dictionary: Sequence[str], device="cuda", lama_blocks: int = 9,
                 ctd_mb: int = 16, lama_mb: int = 16, host_workers: int = 16, mask_workers: int = 4, side_stream: Optional[bool] = None):
        self.device = torch.device(device)
        self.dictionary = list(dictionary)
        self.ctd = ctd.CtdEngine(weights["ctd.yolo"], weights["ctd.seg"], weights["ctd.det"], device=self.device)
        self.ocr = ocr48.Ocr48Engine(weights["ocr48"], len(self.dictionary), device=self.device)
        self.lama = lama.LamaEngine(weights["lama.gen"], weights.get("lama.mpe"), n_blocks=lama_blocks, device=self.device)
        self.dbnet = False
        self._init_host(ctd_mb, lama_mb, host_workers, mask_workers, side_stream)

    @classmethod
    def from_engines(cls, ctd_engine, ocr_engine, lama_engine, dictionary: Sequence[str], ctd_mb: int = 16, lama_mb: int = 16,
                     host_workers: int = 16, mask_workers: int = 4, side_stream: Optional[bool] = None) -> "CoupledPageEngine":
        """On the engines loaded plugins already own (``plugin.engine``): no second copy of any weight.  The engine objects are kept,
        not their methods, so whatever a caller hangs on ``engine.forward`` afterwards is what a run calls.

        The detector slot takes the ctd engine or one of the DBNet kind (``DbnetEngine``, ``DbconvnextEngine``; ``ctd_mb`` is its
        micro-batch as well), the inpainter slot a ``LamaEngine`` of either depth or the ``AotEngine``.  With a DBNet detector
        ``detect`` is ``plugins.dbnet_detect_pages``: no ``refine_mask``, the raw mask at the detector's own size, and no webtoon
        strips (``takes_strips`` is False: a server sends those pages through its page loop)."""
        self = cls.__new__(cls)
        self.device = torch.device(ctd_engine.device)
        self.dictionary = list(dictionary)
        self.ctd, self.ocr, self.lama = ctd_engine, ocr_engine, lama_engine
        self.dbnet = is_dbnet_engine(ctd_engine)
        if self.dbnet:
            self.takes_strips = False
        self._init_host(ctd_mb, lama_mb, host_workers, mask_workers, side_stream)
        return self

    def _init_host(self, ctd_mb, lama_mb, host_workers, mask_workers, side_stream):
        self.ctd_mb, self.lama_mb = ctd_mb, lama_mb
        self.pool = cf.ThreadPoolExecutor(max_workers=host_workers, thread_name_prefix="mit-host")
        # mask refinement: a few pages in flight at once — each worker thread owns a backend (its DenseCRF workspace); their launches
        # go to the same stream, a page's own launches stay in order on it, and the host parts (labelling, assignment) of one page
        # run while another page's kernels execute
        self.mask_pool = cf.ThreadPoolExecutor(max_workers=mask_workers, thread_name_prefix="mit-mask")
        self._tls = threading.local()
        self.side_stream = bool(int(os.environ.get("MIT_COUPLED_SIDE_STREAM", "1"))) if side_stream is None else bool(side_stream)
        self._side = None
        self.stage_streams = bool(int(os.environ.get("MIT_COUPLED_STAGE_STREAMS", "0")))
        self._stage = None

    def _mask_backend(self):
        be = getattr(self._tls, "backend", None)
        if be is None:
            be = self._tls.backend = MR.GpuMaskBackend(self.device)
        return be

    def close(self):
        self.pool.shutdown(wait=True)
        self.mask_pool.shutdown(wait=True)

    # ---- stage 1: detector network + boxes (host pool) + mask resize + refine_mask ------------------------------------------
    @torch.no_grad()
    def detect(self, pages_u8: torch.Tensor, inject=None, det: Optional[dict] = None):
        """-> (textlines per page, refined mask u8 [B,H,W] on the device): ComicTextDetector._infer (ctd.py:129-179) for a batch.

        Webtoon strips (``rearrange.plan(H, W, 1024)`` is not None) take det_rearrange_forward's branch (ctd.py:137) like the plugin
        does, on the device: see ``_detect_strips``.  ``inject`` on a strip holds maps of the STITCHED geometry: ``prob`` f32
        [B, hh, pw] and ``mask`` u8 [B, hh, pw] ([B, pw, hh] for a wide strip), ``(step, pw, hh, _) = rearrange.stitch_geometry(plan, 1024)``.

        With a DBNet engine in the detector slot: DefaultDetector._infer (default.py:56-103) for the batch, which is
        ``plugins.dbnet_detect_pages`` with the parameters of ``det`` (``detect_size`` / ``text_threshold`` / ``box_threshold`` /
        ``unclip_ratio``; the ctd engine ignores them, as the reference's ctd does) -> (textlines per page, the RAW mask u8 [B,h',w'] at the
        detector's own size): that detector has no ``refine_mask``."""
        if self.dbnet:
            return self._detect_dbnet(pages_u8, inject, det or {})
        B, H, W, _ = pages_u8.shape
        mask_full = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        keep = []
        pl = rearrange.plan(H, W, ctd.INPUT_SIZE)
        if pl is not None:
            keep.append((0, B, self._detect_strips(pages_u8, pl, inject, mask_full)))
        else:
            for i in range(0, B, self.ctd_mb):
                j = min(B, i + self.ctd_mb)
                mask_u8, lines, _ = self.ctd.forward(pages_u8[i:j])
                if inject is not None:   # benchmark stand-in for trained weights: the maps a trained head would emit REPLACE the random-init
                    lines[:, 0] = inject["prob"][i:j]     # network's (its sigmoid output hovers around 0.5 everywhere: one page-sized blob);
                    mask_u8 = inject["mask"][i:j]         # the network has run in full by now, its cost is in the measurement
                # SegDetectorRepresenter (db_utils.py:40-216) where the map is (csrc/ctd_boxes.hip): enqueued behind the network, collected below
                keep.append((i, j, hostglue.boxes_from_bitmap_gpu_launch(lines[:, 0], 0.3, W, H, unclip_ratio=1.5, min_sside=2.0)))
                mask_full[i:j] = imgproc.resize_u8(mask_u8.contiguous(), (W, H))      # cv2.resize(mask, (w, h), INTER_LINEAR) (ctd.py:162)
        textlines = [None] * B
        for i, j, h in keep:
            for b, (boxes, scores) in zip(range(i, j), hostglue.boxes_from_bitmap_gpu_collect(h)):
                k = scores > BOX_THRESH
                textlines[b] = [Quadrilateral(pts.astype(np.int64), "", float(s)) for pts, s in zip(boxes[k], scores[k])]
        refined = torch.empty_like(mask_full)
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()

        caller = torch.cuda.current_stream()

        def refine(b):  # refine_mask(img, mask, textlines) (ctd.py:177): batched over the page's lines on the device; its three phases
            torch.cuda.set_device(dev_index)   # alternate with host arithmetic (histograms -> candidates), so a few pages run interleaved
            with torch.no_grad(), torch.cuda.stream(caller):   # a pool thread's own current stream is the default one: launch into the caller's
                return hostglue.refine_mask_gpu(pages_u8[b], mask_full[b], textlines[b], None)

        for b, m in enumerate(self.mask_pool.map(refine, range(B))):
            refined[b] = m
        # the event recorded behind the raw masks' last writer TRAVELS WITH THE TENSOR (merge_and_refine's side stream waits for this, not
        # for the whole queue): no table keyed by address that a failed stage could leave behind for an unrelated tensor to inherit
        refined.mit_ready_event = torch.cuda.current_stream().record_event()
        return textlines, refined

    def _detect_dbnet(self, pages_u8: torch.Tensor, inject, det: dict):
        from . import plugins as P

        size = int(det.get("detect_size", DETECT_SIZE))
        if rearrange.plan(int(pages_u8.shape[1]), int(pages_u8.shape[2]), size) is not None:
            raise NotImplementedError("CoupledPageEngine: webtoon strips with a DBNet detector are not batched (takes_strips is False); "
                                      "run such pages through the detector plugin")
        textlines, raw = P.dbnet_detect_pages(self.ctd, pages_u8, size, float(det.get("text_threshold", TEXT_THRESHOLD)),
                                              float(det.get("box_threshold", DET_BOX_THRESHOLD)), float(det.get("unclip_ratio", UNCLIP_RATIO)),
                                              self.ctd_mb, inject, quad_type=Quadrilateral)
        raw.mit_ready_event = torch.cuda.current_stream().record_event()    # as detect() does behind its refined masks
        return textlines, raw

    def _detect_strips(self, pages_u8: torch.Tensor, pl, inject, mask_full: torch.Tensor):
        """The network part of ``detect`` for a batch of equal webtoon strips, det_rearrange_forward (utils/generic.py:876-997) on the
        device: the squares of all pages (``rearrange.squares_gpu``) go through the network in micro-batches of ``ctd_mb`` — more than the
        reference's four at a time, which changes nothing because the engine's results do not depend on the batch size — each page's
        maps are stitched (``rearrange.stitch_gpu``), the box extraction is enqueued on the stitched maps and the stitched u8 mask is
        resized into ``mask_full``.  -> the handle of the enqueued box extraction."""
        B, H, W, _ = pages_u8.shape
        S = ctd.INPUT_SIZE
        sq = torch.cat([rearrange.squares_gpu(pages_u8[b], pl, S) for b in range(B)])
        n = sq.shape[0]
        lines_sq = torch.empty(n, 2, S, S, dtype=torch.float32, device=self.device)    # the engine's outputs are workspace views that
        mask_sq = torch.empty(n, S, S, dtype=torch.float32, device=self.device)        # the next micro-batch overwrites
        for i in range(0, n, self.ctd_mb):
            _, lines, _ = self.ctd.forward(sq[i:i + self.ctd_mb])
            lines_sq[i:i + self.ctd_mb] = lines
            mask_sq[i:i + self.ctd_mb] = self.ctd.last_mask_f32
        prob, mask_u8 = [], []
        for b in range(B):
            prob.append(rearrange.stitch_gpu(lines_sq[b * pl.p_num:(b + 1) * pl.p_num], pl)[0, 0])
            mask_u8.append(rearrange.stitch_gpu(mask_sq[b * pl.p_num:(b + 1) * pl.p_num], pl, u8=True)[1][0, 0])   # postprocess_mask (ctd.py:155)
        prob, mask_u8 = torch.stack(prob), torch.stack(mask_u8)
        if inject is not None:   # see detect: the stand-in for trained weights, here at the stitched size
            prob, mask_u8 = inject["prob"], inject["mask"]
        h = hostglue.boxes_from_bitmap_gpu_launch(prob, 0.3, W, H, unclip_ratio=1.5, min_sside=2.0)
        mask_full[:] = imgproc.resize_u8(mask_u8.contiguous(), (W, H))
        return h

    # ---- stage 2: OCR ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def recognize(self, pages_u8: torch.Tensor, textlines: List[List[Quadrilateral]], max_seq_length: int, suppress_eos: bool,
                  prob_threshold: float):
        """Model48pxOCR._infer (model_48px.py:67-180) for a batch: direction vote per page (host pool), rectification + recognition
        + one pooled beam search on the GPU, text / probability / colours written back into the lines; lines under the threshold dropped."""
        from . import plugins as P, textline as TL

        def vote(lines):
            return list(TL.generate_text_direction(lines))

        pairs = list(self.pool.map(vote, textlines))
        quads = [[q for q, _ in pr] for pr in pairs]
        dirs = [[d for _, d in pr] for pr in pairs]
        r = self.ocr.recognize_pages(pages_u8, quads, max_seq_length=max_seq_length, suppress_eos=suppress_eos, directions=dirs)
        out: List[List[Quadrilateral]] = [[] for _ in textlines]
        if not r["order"]:
            return out
        toks, lens = r["tokens"].cpu().numpy(), r["length"].cpu().numpy()
        probs, cols = r["prob"].cpu().numpy(), r["colors"].cpu().numpy()
        decoded = P.decode_lines(toks, lens, cols, self.dictionary, rows=[row for row in range(len(r["order"])) if probs[row] >= prob_threshold])
        for row, (p, i) in enumerate(r["order"]):
            q, prob = quads[p][i], float(probs[row])
            q.assigned_direction = dirs[p][i]
            if prob < prob_threshold:
                continue
            q.text, (q.fg_r, q.fg_g, q.fg_b), (q.bg_r, q.bg_g, q.bg_b) = decoded[row]
            q.prob = prob
            if q.text.strip():                   # manga_translator.py:762-770: lines without text are dropped after OCR
                out[p].append(q)
        return out

    # ---- stages 3 + 4: text-line merge, mask refinement -------------------------------------------------------------------
    def merge_and_refine(self, pages_u8: torch.Tensor, textlines: List[List[Quadrilateral]], mask_raw: torch.Tensor,
                         given: Optional[Sequence] = None, dilation_offset: int = MASK_DILATION_OFFSET, kernel_size: int = KERNEL_SIZE,
                         ignore_bubble: int = 0):
        """``given``: per page None or the request's final mask (u8 [H,W], host or device): that page skips merge + refinement.
        ``ignore_bubble`` in 1..50: the refinement's bubble stage (``MR.dispatch_device``), on the device like the rest."""
        B, H, W, _ = pages_u8.shape
        given = list(given) if given is not None else [None] * B
        main = torch.cuda.current_stream()
        # Mask refinement alternates short kernels with host arithmetic (labelling -> assignment -> CRF -> dilation): on the caller's
        # stream each of its read-backs waits for whatever the other stages queued ahead (a LaMa group: a quarter of a second), and the
        # GPU idles through its host phases once that has drained.  With ``side_stream`` (the default; MIT_COUPLED_SIDE_STREAM=0 turns it
        # off) the page workers launch into a high-priority stream of their own instead, beside the queued work: it waits for the event
        # the detector stage recorded behind the raw masks (not for the queue), and the inpainter's launches (caller's stream) wait for
        # its end.  23.4 -> 26.2 pages/s; same bytes as the one-stream path (bench: coupled.batch.pipeline.side_stream_results_equal_one_stream)
        # — since the library is built without the SLP vectoriser's packed-fp32 instructions (with them 3-7 of 64 pages
        # came back with a few dozen mask bytes different whenever two streams' kernels were resident at once).
        ready = getattr(mask_raw, "mit_ready_event", None)   # set by detect(); a mask from anywhere else has none: one-stream path
        side = self._side_stream() if self.side_stream and ready is not None else main
        with torch.cuda.stream(side):
            if side is not main:
                side.wait_event(ready)
                mask_raw.record_stream(side)
            final = torch.zeros(B, H, W, dtype=torch.uint8, device=self.device)   # (from the side stream's own pool of blocks)
        regions = list(self.pool.map(lambda b: TM.dispatch_sync(textlines[b], W, H) if textlines[b] and given[b] is None else [], range(B)))
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()

        def refine(b):
            if given[b] is not None:
                torch.cuda.set_device(dev_index)
                with torch.cuda.stream(side):
                    g = given[b]
                    final[b] = g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g, dtype=np.uint8)).to(self.device)
                return True
            if not regions[b]:
                return None      # no text: the orchestrator returns the page as it is (manga_translator.py:500-504)
            torch.cuda.set_device(dev_index)
            with torch.no_grad(), torch.cuda.stream(side):
                m = MR.dispatch_device(regions[b], pages_u8[b], mask_raw[b], dilation_offset=dilation_offset, kernel_size=kernel_size,
                                       backend=self._mask_backend(), ignore_bubble=ignore_bubble)
                final[b] = m
                return True

        list(self.mask_pool.map(refine, range(B)))
        if side is not main:
            main.wait_stream(side)
            final.record_stream(main)
        return regions, final

    def _stage_stream_set(self):
        if self._stage is None:
            self._stage = {k: torch.cuda.Stream(device=self.device) for k in ("det", "ocr", "tail")}
        return self._stage

    def _side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device, priority=-1)
        return self._side

    # ---- the whole path -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def run(self, pages_u8: torch.Tensor, max_seq_length: int = 255, suppress_eos: bool = False, prob_threshold: float = 0.2,
            inject=None, group: Optional[int] = 16, textlines: Optional[Sequence] = None, mask_raw: Optional[Sequence] = None,
            mask: Optional[Sequence] = None, mask_dilation_offset: int = MASK_DILATION_OFFSET, kernel_size: int = KERNEL_SIZE,
            inpainting_size: Optional[int] = None, precision: str = "fp32", detect_size: int = DETECT_SIZE,
            text_threshold: float = TEXT_THRESHOLD, box_threshold: float = DET_BOX_THRESHOLD, unclip_ratio: float = UNCLIP_RATIO,
            ignore_bubble: int = 0) -> CoupledResult:
        """``group``: pages per pipeline slot.  A batch larger than one group flows through three stage threads (detector + boxes +
        refine_mask | OCR | merge + mask refinement + LaMa), each working on a different group at a time, so the host phases of one
        group run while the kernels of its neighbours execute; every stage sees the groups in order and owns its engines, and each
        page's result is what the unpipelined call (``group=None``) gives.

        What a request may carry, per page (each a sequence of B entries, None where the page brings nothing): ``textlines`` — quads
        [n,4,2] that replace the detector's (the detector still runs, as in ``serve.DenseStages.translate``); ``mask_raw`` — u8 [H,W]
        that replaces the detector's refined mask ahead of merge + refinement; ``mask`` — the final mask, which skips merge +
        refinement.  ``inpainting_size``: the inpainter plugin's resize rule (``plugins.inpaint_pages``); None = the pages go to the
        network as they are (H, W multiples of 8).  ``precision``: the inpainter's, "fp32" | "bf16" (``LamaEngine.forward``) —
        a server passes its plugin's ``precision_for(config)``.  The defaults are the constants the benchmark path has always used.
        ``detect_size`` / ``text_threshold`` / ``box_threshold`` / ``unclip_ratio``: the detector's parameters (DetectorConfig,
        config.py:274-290), for a DBNet engine; the ctd engine ignores them as the reference's ctd does (fixed 1024, 0.3, 0.6, 1.5).
        With a DBNet engine a request's ``mask_raw`` may be page-sized or of the detector's mask size; ``CoupledResult.mask_raw`` is
        then a list when the sizes differ between pages.  ``ignore_bubble`` (``--ignore-bubble``, 1..50; 0 = off): mask refinement
        ends with the bubble stage (mask_refinement/__init__.py:31-50), on the device; a page whose ``mask`` the request brings skips
        it with the rest of the refinement.  (The OCR models' crop test of the same option belongs to the ctc / 32px models.)"""
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"CoupledPageEngine.run: precision must be 'fp32' or 'bf16' (got {precision!r})")
        if pages_u8.dtype != torch.uint8 or pages_u8.dim() != 4 or pages_u8.shape[-1] != 3 or not pages_u8.is_cuda:
            raise ValueError(f"CoupledPageEngine.run expects a uint8 device tensor [B,H,W,3], got {pages_u8.dtype} {tuple(pages_u8.shape)}")
        B = pages_u8.shape[0]
        for name, v in (("textlines", textlines), ("mask_raw", mask_raw), ("mask", mask)):
            if v is not None and len(v) != B:
                raise ValueError(f"CoupledPageEngine.run: {name} must have one entry per page ({len(v)} for {B} pages)")
        req = {"textlines": textlines, "mask_raw": mask_raw, "mask": mask, "offset": int(mask_dilation_offset), "kernel": int(kernel_size),
               "ignore_bubble": int(ignore_bubble),
               "inpainting_size": inpainting_size, "precision": precision,
               "det": {"detect_size": int(detect_size), "text_threshold": float(text_threshold), "box_threshold": float(box_threshold),
                       "unclip_ratio": float(unclip_ratio)}}
        if group is not None and B > group:
            return self._run_pipelined(pages_u8, max_seq_length, suppress_eos, prob_threshold, inject, int(group), req)
        sec = {}
        t = time.perf_counter()
        tl, mraw = self._requested(*self.detect(pages_u8, inject, req["det"]), req, 0, B, tuple(pages_u8.shape[1:3]))
        sec["detect+boxes+refine_mask"] = time.perf_counter() - t
        t = time.perf_counter()
        tl = self.recognize(pages_u8, tl, max_seq_length, suppress_eos, prob_threshold)
        sec["ocr"] = time.perf_counter() - t
        t = time.perf_counter()
        regions, final = self.merge_and_refine(pages_u8, tl, mraw, mask, req["offset"], req["kernel"], req["ignore_bubble"])
        sec["textline_merge+mask_refinement"] = time.perf_counter() - t
        t = time.perf_counter()
        inpainted = torch.empty_like(pages_u8)
        self._inpaint(pages_u8, final, inpainted, inpainting_size, precision)
        sec["inpaint (enqueue)"] = time.perf_counter() - t
        return CoupledResult(tl, regions, final, inpainted, sec, mraw)

    def _requested(self, textlines, mask_raw, req, a, b, page_hw=None):
        """The detector's lines / refined masks of pages a..b with what the request brings for them laid over.  ``page_hw``: the pages'
        (H, W); a DBNet engine's raw masks have a size of their own, and a request's page-sized ``mask_raw`` then turns the group's
        masks into a per-page list (``RawMasks``: mask refinement resizes a raw mask of any size)."""
        tin, min_ = req["textlines"], req["mask_raw"]
        if tin is not None:
            for k in range(a, b):
                if tin[k] is not None:
                    textlines[k - a] = [Quadrilateral(np.asarray(p, dtype=np.int64), "", 1.0) for p in tin[k]]
        if min_ is not None and any(min_[k] is not None for k in range(a, b)):
            ready = getattr(mask_raw, "mit_ready_event", None)
            own = tuple(mask_raw.shape[1:])
            sizes = (own,) if page_hw is None or not self.dbnet else (own, tuple(page_hw))
            for k in range(a, b):
                if min_[k] is not None:
                    m = min_[k]
                    m = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8))
                    if tuple(m.shape) not in sizes:
                        raise ValueError(f"mask_raw of page {k} must be {' or '.join(str(s) for s in sizes)} (got {tuple(m.shape)})")
                    if tuple(m.shape) != own and not isinstance(mask_raw, RawMasks):
                        mask_raw = RawMasks(mask_raw[i] for i in range(b - a))
                    mask_raw[k - a] = m.to(self.device)
            if ready is not None:
                mask_raw.mit_ready_event = torch.cuda.current_stream().record_event()
        return textlines, mask_raw

    def _inpaint(self, pages_u8: torch.Tensor, mask: torch.Tensor, out: torch.Tensor, inpainting_size: Optional[int] = None,
                 precision: str = "fp32"):
        if inpainting_size is not None:   # the plugin's resize / composite legs around the network, for the whole group
            from . import plugins as P

            out.copy_(P.inpaint_pages(self.lama, pages_u8, mask, int(inpainting_size), None, self.lama_mb, precision=precision))
            return
        kw = {} if precision == "fp32" else {"precision": precision}
        for i in range(0, pages_u8.shape[0], self.lama_mb):
            j = min(pages_u8.shape[0], i + self.lama_mb)
            out[i:j].copy_(self.lama.forward(pages_u8[i:j], mask[i:j], **kw))

    def _run_pipelined(self, pages_u8, max_seq_length, suppress_eos, prob_threshold, inject, group, req) -> CoupledResult:
        B, H, W, _ = pages_u8.shape
        spans = [(i, min(B, i + group)) for i in range(0, B, group)]
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        sec = {"detect+boxes+refine_mask": 0.0, "ocr": 0.0, "textline_merge+mask_refinement": 0.0, "inpaint (enqueue)": 0.0}
        mask = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        # (a DBNet engine's raw masks have a size of their own, per page once a request replaces some: they are gathered at the end)
        mask_raw_all = None if self.dbnet else torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        raws = [None] * len(spans)
        inpainted = torch.empty_like(pages_u8)
        caller = torch.cuda.current_stream()
        # One stream per stage thread (``stage_streams``, MIT_COUPLED_STAGE_STREAMS=1): a stage's read-backs wait for ITS kernels only, and
        # the kernels of the stages overlap on the GPU.  The streams start behind everything the caller queued, and the caller's stream
        # continues behind them at the end.  Same results; measured 25.4 vs 26.1 pages/s for the default (every stage thread launches
        # into the caller's stream, only the mask stage has its side stream): with 35 ms of kernels per page the GPU is the bound, and
        # the latency-bound OCR decode is the stage that loses when it has to share the CUs with LaMa.
        if self.stage_streams:
            st = self._stage_stream_set()
            start = caller.record_event()
            for x in st.values():
                x.wait_event(start)
        else:
            st = {"det": caller, "ocr": caller, "tail": caller}

        def timed(key, fn, *a):
            torch.cuda.set_device(dev_index)
            with torch.no_grad(), torch.cuda.stream(st[_STAGE_OF[key]]):
                t = time.perf_counter()
                r = fn(*a)
                sec[key] += time.perf_counter() - t           # one thread per key: no race
                return r

        def st_detect(a, b):
            inj = None if inject is None else {k: v[a:b] for k, v in inject.items()}
            return timed("detect+boxes+refine_mask", lambda: self._requested(*self.detect(pages_u8[a:b], inj, req["det"]), req, a, b, (H, W)))

        def st_ocr(a, b, f_det):
            tl, mraw = f_det.result()
            return timed("ocr", self.recognize, pages_u8[a:b], tl, max_seq_length, suppress_eos, prob_threshold), mraw

        def st_tail(a, b, f_ocr):
            tl, mraw = f_ocr.result()
            given = None if req["mask"] is None else req["mask"][a:b]
            regions, m = timed("textline_merge+mask_refinement", self.merge_and_refine, pages_u8[a:b], tl, mraw, given, req["offset"], req["kernel"], req["ignore_bubble"])
            with torch.cuda.stream(st["tail"]):
                mask[a:b] = m
                if mask_raw_all is not None:
                    mask_raw_all[a:b] = mraw
                else:
                    raws[a // group] = mraw
            timed("inpaint (enqueue)", self._inpaint, pages_u8[a:b], mask[a:b], inpainted[a:b], req["inpainting_size"], req["precision"])
            return tl, regions

        with cf.ThreadPoolExecutor(1, "mit-st-det") as e1, cf.ThreadPoolExecutor(1, "mit-st-ocr") as e2, cf.ThreadPoolExecutor(1, "mit-st-tail") as e3:
            f1 = [e1.submit(st_detect, a, b) for a, b in spans]
            f2 = [e2.submit(st_ocr, a, b, f) for (a, b), f in zip(spans, f1)]
            f3 = [e3.submit(st_tail, a, b, f) for (a, b), f in zip(spans, f2)]
            done = [f.result() for f in f3]
        for x in st.values():
            if x is not caller:
                caller.wait_stream(x)
        textlines = [t for tl, _ in done for t in tl]
        regions = [r for _, rg in done for r in rg]
        if mask_raw_all is None:   # one tensor while every group kept the detector's size, else the per-page list
            same = all(isinstance(r, torch.Tensor) and r.shape[1:] == raws[0].shape[1:] for r in raws)
            mask_raw_all = torch.cat(raws) if same else RawMasks(m for r in raws for m in r)
        return CoupledResult(textlines, regions, mask, inpainted, sec, mask_raw_all)
