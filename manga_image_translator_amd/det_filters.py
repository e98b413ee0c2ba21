"""The page filters of ``CommonDetector.detect`` (detection/common.py:12-64): what the reference puts around every detector.

Before the network (:18-35), in this order: ``rotate`` (``np.rot90(image, k=-1)``), a zero border up to a square of at least 400 px —
added BY DEFAULT when the shorter side is under 400 px, no option set —, ``invert`` (``cv2.bitwise_not``) and ``gamma_correct``
(gray mean -> ``gamma = log(127.5) / log(mean)`` -> ``np.power(image, gamma).clip(0, 255).astype(np.uint8)``).  After it (:45-64) the
border and the rotation are taken off the text lines and both masks, and with ``auto_rotate`` the detection runs a second time, turned
the other way, when horizontal lines are in the majority.

``apply_host`` / ``undo_host`` are the numpy statements of ``_add_rotation``, ``_add_border``, ``_add_inversion``,
``_add_gamma_correction``, ``_remove_border`` and ``_remove_rotation``: the statement of record and the oracle of the GPU tests.
``apply`` / ``undo`` are the device forms over ``mit_det_filter_gray_sum``, ``mit_det_filter_apply`` and ``mit_det_unrotate_u8``
(csrc/det_filters.hip), byte for byte the same.  ``detect`` is the control flow of ``CommonDetector.detect`` around either pair.

The reference is reproduced as it is, quirks included:
  * ``_remove_border`` crops the masks with the UNROTATED ``img_h, img_w`` and clips the points to them even when the bordered frame
    was rotated: a 96 x 160 page with ``rotate`` comes back with masks of shape (160, 96) and line ordinates such as -64.
  * ``_remove_border`` drops a line only when ``xyxy[0] >= old_w and xyxy[1] >= old_h`` and clips the points of the others in place.
  * its ``cv2.resize(mask, (new_w, new_h), INTER_LINEAR)`` is the identity when the masks are already at the filtered page's size, as
    the ctd plugin's are; any other size — the DBNet plugins return the mask at the network's page size (default.py:89-95) — goes
    through ``imgproc.resize_u8``, the project's INTER_LINEAR.  Without a border nothing is resized, there as here.
  * ``mask`` may be None (the DBNet plugins).
The gray value is the project's fixed-point restatement of ``cv2.COLOR_BGR2GRAY`` (hostglue.py, csrc/ctd_refine.hip): an OpenCV
primitive that stays restated and unpinned.
"""
from __future__ import annotations

import ctypes as C
import inspect
from collections import Counter
from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np

MINIMUM_IMAGE_SIZE = 400   # detection/common.py:21


class Plan(NamedTuple):
    """What ``detect`` does to a page of ``h`` x ``w``: whether the border is added, its ``side`` (0 without one) and the filtered frame."""
    border: bool
    side: int
    fh: int
    fw: int


def plan(h: int, w: int, rotate: bool) -> Plan:
    """The border decision (``min(img_w, img_h) < 400``, strict: common.py:23), ``side = max(fw, fh, 400)`` (:73) and the filtered
    frame: (w, h) when rotated, else (h, w); side x side with the border."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError(f"det_filters.plan: a page of {h} x {w}")
    fh, fw = (w, h) if rotate else (h, w)
    if min(w, h) < MINIMUM_IMAGE_SIZE:
        side = max(fw, fh, MINIMUM_IMAGE_SIZE)
        return Plan(True, side, side, side)
    return Plan(False, 0, fh, fw)


def gray_u8(image: np.ndarray) -> np.ndarray:
    """``cv2.cvtColor(image, cv2.COLOR_BGR2GRAY)`` on u8 [...,3] in the fixed-point form the project uses everywhere."""
    t = image.astype(np.int64)
    return ((t[..., 0] * 1868 + t[..., 1] * 9617 + t[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def gamma_lut(gray_sum: int, n_pixels: int) -> np.ndarray:
    """The 256 bytes ``_add_gamma_correction`` (common.py:118-124) maps the byte values to, for a filtered page whose gray image sums
    to ``gray_sum`` over ``n_pixels`` pixels (border included).  ``np.float64(gray_sum) / n_pixels`` is what ``np.mean`` of the u8 gray
    image returns (integer partial sums are exact in float64 at these sizes); the rest is the reference's own statement evaluated on
    ``np.arange(256, dtype=np.uint8)`` — nothing inside ``np.power`` is restated, so the table is the reference's bytes whichever numpy
    is installed.  The degenerate means follow on their own: 0 -> gamma -0.0 -> every entry 1; 1 -> gamma inf -> [0, 1, 255, 255, ...].

    For the device form this costs one synchronisation a call: the 8-byte sum of each page comes to the host and 256 bytes go back."""
    values = np.arange(256, dtype=np.uint8)
    with np.errstate(all="ignore"):
        mean = np.float64(gray_sum) / n_pixels
        mid = 0.5
        gamma = np.log(mid * 255) / np.log(mean)
        return np.power(values, gamma).clip(0, 255).astype(np.uint8)


def apply_host(image: np.ndarray, rotate: bool, invert: bool, gamma_correct: bool) -> np.ndarray:
    """The filters of common.py:24-35 on a host page u8 [H,W,3], statement by statement."""
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"expected uint8 [H,W,3], got {image.dtype} {image.shape}")
    img_h, img_w = image.shape[:2]
    if rotate:                                        # _add_rotation (:101-102)
        image = np.rot90(image, k=-1)
    if min(img_w, img_h) < MINIMUM_IMAGE_SIZE:        # _add_border (:71-79)
        old_h, old_w = image.shape[:2]
        new_w = new_h = max(old_w, old_h, MINIMUM_IMAGE_SIZE)
        new_image = np.zeros([new_h, new_w, 3]).astype(np.uint8)
        new_image[0:old_h, 0:old_w] = image
        image = new_image
    if invert:                                        # _add_inversion (:115-116)
        image = np.bitwise_not(image)
    if gamma_correct:                                 # _add_gamma_correction (:118-124)
        with np.errstate(all="ignore"):
            gray = gray_u8(image)
            mid = 0.5
            mean = np.mean(gray)
            gamma = np.log(mid * 255) / np.log(mean)
            image = np.power(image, gamma).clip(0, 255).astype(np.uint8)
    return image


def _rebuild(line, pts):
    return type(line)(pts, line.text, line.prob)


def remove_border_lines(textlines: List, old_w: int, old_h: int) -> List:
    """The text-line half of ``_remove_border`` (common.py:89-99): a line is dropped only when its box starts at or beyond BOTH
    ``old_w`` and ``old_h``; the points of the others are clipped in place and the line is built again from them."""
    out = []
    for txtln in textlines:
        if txtln.xyxy[0] >= old_w and txtln.xyxy[1] >= old_h:
            continue
        points = txtln.pts
        points[:, 0] = np.clip(points[:, 0], 0, old_w)
        points[:, 1] = np.clip(points[:, 1], 0, old_h)
        out.append(_rebuild(txtln, points))
    return out


def remove_rotation_lines(textlines: List, img_h: int) -> List:
    """The text-line half of ``_remove_rotation`` (common.py:109-112): (x, y) -> (y, img_h - x)."""
    out = []
    for txtln in textlines:
        rotated_pts = txtln.pts[:, [1, 0]]
        rotated_pts[:, 1] = -rotated_pts[:, 1] + img_h
        out.append(_rebuild(txtln, rotated_pts))
    return out


def _to_frame_host(m: np.ndarray, fh: int, fw: int) -> np.ndarray:
    """``cv2.resize(m, (fw, fh), INTER_LINEAR)`` (common.py:83,86): the identity at the frame's size, ``imgproc.resize_u8`` otherwise."""
    if m.shape[:2] == (fh, fw):
        return m
    import torch

    from . import imgproc

    return imgproc.resize_u8(torch.from_numpy(np.ascontiguousarray(m)).cuda()[None], (fw, fh))[0].cpu().numpy()


def undo_masks_host(raw_mask, mask, img_h: int, img_w: int, rotate: bool):
    """The mask halves of ``_remove_border`` (:82-87, cropping with the unrotated ``img_h, img_w``) and ``_remove_rotation`` (:105-107)."""
    p = plan(img_h, img_w, rotate)
    out = []
    for m in (raw_mask, mask):
        if m is not None:
            if p.border:
                m = _to_frame_host(m, p.fh, p.fw)[:img_h, :img_w]
            if rotate:
                m = np.ascontiguousarray(np.rot90(m))
        out.append(m)
    if rotate and out[1] is not None:
        out[1] = np.ascontiguousarray(out[1].astype(np.uint8))
    return out[0], out[1]


def undo_host(textlines: List, raw_mask, mask, img_h: int, img_w: int, rotate: bool):
    """``_remove_border`` then ``_remove_rotation`` (common.py:48-49,61-62) on the lines and both masks of a page of ``img_h`` x
    ``img_w`` -> (textlines, raw_mask, mask)."""
    if plan(img_h, img_w, rotate).border:
        textlines = remove_border_lines(textlines, img_w, img_h)
    if rotate:
        textlines = remove_rotation_lines(textlines, img_h)
    return (textlines,) + undo_masks_host(raw_mask, mask, img_h, img_w, rotate)


# ---- the device forms ------------------------------------------------------------------------------------------------------------

def _check_pages(pages):
    import torch

    if not torch.is_tensor(pages) or pages.dtype != torch.uint8 or pages.dim() not in (3, 4) or pages.shape[-1] != 3:
        raise ValueError("det_filters: expected a uint8 device tensor [B,H,W,3] or [H,W,3]")
    if not pages.is_cuda:
        raise ValueError("det_filters.apply runs on device tensors (apply_host is the numpy statement for host arrays)")
    if not pages.is_contiguous():
        raise ValueError("det_filters: the pages must be contiguous")


def gray_sums(pages, invert: bool) -> List[int]:
    """The exact sum of the gray image of every filtered, pre-gamma page of u8 [B,H,W,3] on the device (``mit_det_filter_gray_sum``),
    as Python integers.  Synchronises: the sums come to the host."""
    import torch

    from . import lib as _lib, ops

    _check_pages(pages)
    s = pages if pages.dim() == 4 else pages[None]
    B, H, W, _ = s.shape
    p = plan(H, W, False)
    sums = torch.empty(B, dtype=torch.int64, device=s.device)
    _lib.check(_lib.load().mit_det_filter_gray_sum(s.data_ptr(), B, H, W, p.side, int(bool(invert)), sums.data_ptr(),
                                                   C.c_void_p(ops.current_stream())), "mit_det_filter_gray_sum")
    return [int(v) for v in sums.cpu().numpy().view(np.uint64)]


def apply(pages, rotate: bool, invert: bool, gamma_correct: bool):
    """``apply_host`` for pages u8 [B,H,W,3] (or [H,W,3]) on the device -> [B,fh,fw,3] ([fh,fw,3]) there, the same bytes.  One pass
    from the source page to the filtered page; with ``gamma_correct`` one pass before it for the gray sums, which come to the host
    (8 bytes a page) for ``gamma_lut`` and go back as 256 bytes a page — the one synchronisation of this function.  A page that no
    filter touches is returned as it is."""
    import torch

    from . import lib as _lib, ops

    _check_pages(pages)
    squeeze = pages.dim() == 3
    s = pages[None] if squeeze else pages
    B, H, W, _ = s.shape
    p = plan(H, W, rotate)
    if not (rotate or p.border or invert or gamma_correct):
        return pages
    lut = None
    if gamma_correct:
        tables = np.stack([gamma_lut(v, p.fh * p.fw) for v in gray_sums(s, invert)])
        lut = torch.from_numpy(tables).to(s.device)
    out = torch.empty(B, p.fh, p.fw, 3, dtype=torch.uint8, device=s.device)
    _lib.check(_lib.load().mit_det_filter_apply(s.data_ptr(), B, H, W, int(bool(rotate)), p.side, int(bool(invert)),
                                                None if lut is None else lut.data_ptr(), out.data_ptr(),
                                                C.c_void_p(ops.current_stream())), "mit_det_filter_apply")
    return out[0] if squeeze else out


def unrotate_u8(maps, ch: int, cw: int):
    """``np.rot90(m[:ch, :cw])`` for u8 maps [B,h,w] (or [h,w]) on the device -> [B,cw,ch] ([cw,ch]) (``mit_det_unrotate_u8``)."""
    import torch

    from . import lib as _lib, ops

    if not torch.is_tensor(maps) or maps.dtype != torch.uint8 or maps.dim() not in (2, 3) or not maps.is_cuda:
        raise ValueError("det_filters.unrotate_u8 expects a uint8 device tensor [B,h,w] or [h,w]")
    squeeze = maps.dim() == 2
    s = (maps[None] if squeeze else maps).contiguous()
    B, h, w = s.shape
    out = torch.empty(B, int(cw), int(ch), dtype=torch.uint8, device=s.device)
    _lib.check(_lib.load().mit_det_unrotate_u8(s.data_ptr(), B, h, w, int(ch), int(cw), out.data_ptr(), C.c_void_p(ops.current_stream())),
               "mit_det_unrotate_u8")
    return out[0] if squeeze else out


def undo(raw_mask, mask, img_h: int, img_w: int, rotate: bool):
    """``undo_masks_host`` for u8 masks [h,w] on the device (None stays None): the crop alone is a slice, a rotation is one launch
    with the crop fused in."""
    from . import imgproc

    p = plan(img_h, img_w, rotate)
    out = []
    for m in (raw_mask, mask):
        if m is not None:
            if p.border and tuple(m.shape[:2]) != (p.fh, p.fw):
                m = imgproc.resize_u8(m[None].contiguous(), (p.fw, p.fh))[0]
            ch, cw = (min(img_h, m.shape[0]), min(img_w, m.shape[1])) if p.border else (m.shape[0], m.shape[1])
            m = unrotate_u8(m, ch, cw) if rotate else m[:ch, :cw]
        out.append(m)
    return out[0], out[1]


# ---- CommonDetector.detect -------------------------------------------------------------------------------------------------------

async def detect(infer_fn: Callable, image, detect_size: int, text_threshold: float, box_threshold: float, unclip_ratio: float,
                 invert: bool, gamma_correct: bool, rotate: bool, auto_rotate: bool = False, verbose: bool = False, *,
                 apply_fn: Callable = apply_host, undo_masks_fn: Callable = undo_masks_host, on_rerun: Optional[Callable] = None):
    """The control flow of ``CommonDetector.detect`` (common.py:12-64) around ``infer_fn(filtered_page, detect_size, text_threshold,
    box_threshold, unclip_ratio, verbose) -> (textlines, raw_mask, mask)`` (plain or a coroutine function).  ``image`` is the page
    [H,W,3] — a host array with ``apply_host`` / ``undo_masks_host`` (the default), a device tensor with ``apply`` / ``undo`` —
    and the masks come back where ``infer_fn`` left them.

    The ``area > 1`` filter on the lines (:45); the border taken off the lines (:48-49); the auto-rotate vote (:50-60): 'h' when
    ``aspect_ratio > 1``, no lines count as 'h', and a majority of 'h' runs the ORIGINAL page again with ``rotate`` flipped and
    ``auto_rotate`` off; the rotation taken off (:61-62).  The masks of a first run that is run again are discarded like the
    reference's, so they are undone only for the run that is returned."""
    img_h, img_w = int(image.shape[0]), int(image.shape[1])
    p = plan(img_h, img_w, rotate)
    filtered = apply_fn(image, rotate, invert, gamma_correct)
    res = infer_fn(filtered, detect_size, text_threshold, box_threshold, unclip_ratio, verbose)
    if inspect.isawaitable(res):
        res = await res
    textlines, raw_mask, mask = res
    textlines = list(filter(lambda x: x.area > 1, textlines))
    if p.border:
        textlines = remove_border_lines(textlines, img_w, img_h)
    if auto_rotate:
        if len(textlines) > 0:
            orientations = ["h" if txtln.aspect_ratio > 1 else "v" for txtln in textlines]
            majority_orientation = Counter(orientations).most_common(1)[0][0]
        else:
            majority_orientation = "h"
        if majority_orientation == "h":
            if on_rerun is not None:
                on_rerun()
            return await detect(infer_fn, image, detect_size, text_threshold, box_threshold, unclip_ratio, invert, gamma_correct,
                                rotate=(not rotate), auto_rotate=False, verbose=verbose, apply_fn=apply_fn, undo_masks_fn=undo_masks_fn,
                                on_rerun=on_rerun)
    if rotate:
        textlines = remove_rotation_lines(textlines, img_h)
    raw_mask, mask = undo_masks_fn(raw_mask, mask, img_h, img_w, rotate)
    return textlines, raw_mask, mask
