"""Tall / wide page tiling for the detectors ("rearrange"): what the reference's ``det_rearrange_forward`` does
(/root/reference/manga_translator/utils/generic.py:876-997, called from detection/ctd.py:137 and detection/default.py:60).

A webtoon strip letterboxed to the detect size would lose its text, so when ``long side / tgt_size > 2.5`` and the aspect ratio
exceeds 3 the reference cuts the strip into overlapping bands of ``pw_num`` strip-widths each, lays ``pw_num`` bands side by
side into a square, pads / shrinks that square to ``tgt_size`` (``square_pad_resize``, :848-874), runs the detector network on
batches of at most four squares, and stitches the output maps back (bands averaged where consecutive ones overlap).

This module re-derives that geometry once (``plan``) and applies it in two vectorised passes (``squares`` before the network,
``stitch`` after it); the network itself is whatever batched callable the plugin hands in (the HIP engine).  The arithmetic of the
stitch (accumulate, halve the overlap of every band after the first) is kept in float32 numpy in the reference's order, so the
stitched maps are bit-identical to the reference's for the same network output (tests/golden/rearrange.npz pins that against the
reference function itself, with a deterministic stand-in for the network).

``squares_gpu`` / ``stitch_gpu`` / ``forward_gpu`` are the same two passes with the page and the maps on the device
(csrc/rearrange.hip): the plan and the band starts still come from here, the stitch replays the same accumulation per output element
and gives the same bits (tests/test_rearrange_gpu.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np


@dataclass
class Plan:
    transpose: bool      # the strip is wide, not tall: work on the transposed page
    h: int               # strip length (after the transpose)
    w: int               # strip width
    pw_num: int          # bands laid side by side in one square
    patch: int           # band length = square side before padding = pw_num * w
    ph_num: int          # number of bands
    ph_step: int         # band pitch along the strip (consecutive bands overlap by patch - ph_step)
    rel_steps: List[float]  # band start / strip length
    p_num: int           # number of squares
    pad_num: int         # empty bands appended to fill the last square


def plan(height: int, width: int, tgt_size: int) -> Optional[Plan]:
    """The tiling of an [height, width] page for a detector running at ``tgt_size``, or None when the page is processed whole
    (generic.py:941-949: rearrange only when long/tgt > 2.5 and long/short > 3)."""
    transpose = height < width
    h, w = (width, height) if transpose else (height, width)
    if not (h / tgt_size > 2.5 and h / w > 3):
        return None
    pw_num = max(int(np.floor(2 * tgt_size / w)), 2)
    patch = pw_num * w
    ph_num = int(np.ceil(h / patch))
    ph_step = int((h - patch) / (ph_num - 1)) if ph_num > 1 else 0
    rel = [(i * ph_step) / h for i in range(ph_num)]
    p_num = int(np.ceil(ph_num / pw_num))
    return Plan(transpose, h, w, pw_num, patch, ph_num, ph_step, rel, p_num, p_num * pw_num - ph_num)


def squares(img: np.ndarray, pl: Plan, tgt_size: int, resize: Optional[Callable[[np.ndarray, Tuple[int, int]], np.ndarray]] = None):
    """u8 page [H,W,3] -> (squares u8 [p_num, tgt, tgt, 3], pad_size): bands of ``patch`` rows cut at pitch ph_step (the last one
    ends at or before the strip end by construction of ph_step; empty bands fill the last square), ``pw_num`` bands side by side
    per square, zero padding at the bottom / right up to ``tgt_size`` or — for squares larger than ``tgt_size`` —
    an INTER_LINEAR shrink (``resize(img, (w, h))``; with ``resize=None`` the squares are returned unshrunk, [p_num, side, side, 3],
    for a caller that shrinks them on the GPU)."""
    strip = np.transpose(img, (1, 0, 2)) if pl.transpose else img
    C = strip.shape[2]
    side = pl.patch
    out = []
    pad_size = None
    for s in range(pl.p_num):
        sq = np.zeros((side, side, C), dtype=strip.dtype)
        for j in range(pl.pw_num):
            b = s * pl.pw_num + j
            if b >= pl.ph_num:
                break
            t = b * pl.ph_step
            band = strip[t:t + side]
            assert band.shape[0] == side, "ph_step keeps every band inside the strip"
            if pl.transpose:   # '(p pw_num) ph pw c -> p (pw_num pw) ph c': bands stacked along rows, each one transposed
                sq[j * pl.w:(j + 1) * pl.w, :, :] = np.transpose(band, (1, 0, 2))
            else:              # '(p pw_num) ph pw c -> p ph (pw_num pw) c': bands side by side
                sq[:, j * pl.w:(j + 1) * pl.w, :] = band
        pad = max(tgt_size - side, 0)   # square_pad_resize: the input is already square, so pad_h == pad_w == tgt - side
        if pad:
            sq = np.pad(sq, ((0, pad), (0, pad), (0, 0)))
        if sq.shape[0] > tgt_size and resize is not None:
            sq = resize(sq, (tgt_size, tgt_size))
        if pad_size is None:
            pad_size = pad
        out.append(sq)
    return np.stack(out), int(pad_size)


def stitch_geometry(pl: Plan, psize: int) -> Tuple[int, int, int, List[int]]:
    """(step, pw, hh, starts) of the stitched map for network output squares of side ``psize`` (generic.py:892-895,904): the band
    pitch and the band width in map pixels, the map's length along the strip, and the row every band starts at.  ``stitch`` and
    ``stitch_gpu`` both take their geometry from here (``round`` is Python's, so the starts are computed on the host for both)."""
    step = int(pl.ph_step * psize / pl.patch)
    pw = int(psize / pl.pw_num)
    hh = int(pw / pl.w * pl.h)
    return step, pw, hh, [int(round(pl.rel_steps[p] * hh)) for p in range(pl.ph_num)]


def stitch(maps: Sequence[np.ndarray], pl: Plan, channel: int) -> np.ndarray:
    """Network output squares [c, s, s] (already cropped of the padding) -> the strip's map [1, c, H', W'] (float32).

    Every band is added at its relative position; from the second band on, the rows it shares with its predecessor (the first
    ``s - step`` rows of the band) are halved after the add — the reference's running average (generic.py:897-916)."""
    psize = maps[0].shape[-1]
    step, pw, hh, starts = stitch_geometry(pl, psize)
    tgt = np.zeros((channel, hh, pw), dtype=np.float32)
    last = len(maps) * pl.pw_num - pl.pad_num - 1
    done = False
    for ii, p in enumerate(maps):
        if done:
            break
        if pl.transpose:
            p = np.transpose(p, (0, 2, 1))
        for jj in range(pl.pw_num):
            pidx = ii * pl.pw_num + jj
            t = starts[pidx]
            b = min(t + psize, hh)
            tgt[..., t:b, :] += p[..., :b - t, jj * pw:(jj + 1) * pw]
            if pidx > 0:
                tgt[..., t:t + (psize - step), :] /= 2.0
            if pidx >= last:
                done = True
                break
    if pl.transpose:
        tgt = np.transpose(tgt, (0, 2, 1))
    return tgt[None]


def forward(img: np.ndarray, batch_forward: Callable[[np.ndarray], Tuple[np.ndarray, np.ndarray]], tgt_size: int,
            resize: Optional[Callable[[np.ndarray, Tuple[int, int]], np.ndarray]] = None, max_batch_size: int = 4):
    """det_rearrange_forward: (db [1,2,H',W'], mask [1,1,H'',W'']) or (None, None) when the page needs no tiling.
    ``batch_forward(u8 [n<=4, s, s, 3]) -> (db [n,2,m,m], mask [n,1,m',m'])`` float32 numpy, s = tgt_size (or the unshrunk
    square side when ``resize`` is None and the squares exceed tgt_size: the callable then shrinks them itself)."""
    pl = plan(img.shape[0], img.shape[1], tgt_size)
    if pl is None:
        return None, None
    sq, pad_size = squares(img, pl, tgt_size, resize)
    dbs, masks = [], []
    for i in range(0, len(sq), max_batch_size):
        db, mask = batch_forward(sq[i:i + max_batch_size])
        for d, m in zip(db, mask):
            if pad_size > 0:
                pd, pm = int(db.shape[-1] / tgt_size * pad_size), int(mask.shape[-1] / tgt_size * pad_size)
                d, m = d[..., :-pd, :-pd], m[..., :-pm, :-pm]
            dbs.append(d)
            masks.append(m)
    return stitch(dbs, pl, 2), stitch(masks, pl, 1)


# ---- the same tiling with the page and the maps on the device (csrc/rearrange.hip) ---------------------------------------------

def squares_gpu(page_dev, pl: Plan, tgt_size: int):
    """``squares`` on the device: u8 page [H,W,3] (device) -> u8 [p_num, tgt, tgt, 3]: the band gather (``mit_rearrange_squares``) and
    square_pad_resize's INTER_LINEAR shrink (``imgproc.resize_u8``).  Every plan of ``plan()`` has ``patch > tgt_size`` (for
    w <= tgt, patch = floor(2 tgt / w) w > 2 tgt - w >= tgt; else patch = 2 w > 2 tgt), so the padding branch of square_pad_resize
    does not exist here: a plan with ``patch <= tgt_size`` is refused."""
    import ctypes as C

    import torch

    from . import imgproc, lib as _lib, ops

    if pl.patch <= tgt_size:
        raise ValueError(f"squares_gpu: squares of side {pl.patch} would be padded to {tgt_size}; plan() makes no such plan (use squares)")
    if page_dev.dtype != torch.uint8 or page_dev.dim() != 3 or page_dev.shape[2] != 3 or not page_dev.is_cuda:
        raise ValueError(f"squares_gpu expects a uint8 device page [H,W,3], got {page_dev.dtype} {tuple(page_dev.shape)} on {page_dev.device}")
    H, W = int(page_dev.shape[0]), int(page_dev.shape[1])
    if (pl.h, pl.w) != ((W, H) if pl.transpose else (H, W)):
        raise ValueError(f"squares_gpu: the plan is for a {pl.h} x {pl.w} strip, the page is {H} x {W}")
    page_dev = page_dev.contiguous()
    sq = torch.empty(pl.p_num, pl.patch, pl.patch, 3, dtype=torch.uint8, device=page_dev.device)
    _lib.check(_lib.load().mit_rearrange_squares(page_dev.data_ptr(), H, W, int(pl.transpose), pl.w, pl.pw_num, pl.ph_num, pl.ph_step, pl.p_num,
                                                 sq.data_ptr(), C.c_void_p(ops.current_stream())), "mit_rearrange_squares")
    return imgproc.resize_u8(sq, (tgt_size, tgt_size))


def stitch_gpu(maps_dev, pl: Plan, u8: bool = False):
    """``stitch`` on the device (``mit_rearrange_stitch``): the network's output squares f32 [n, C, m, m] (or [n, m, m]: one channel),
    any strides — an engine's workspace view as it is — -> the strip's map f32 [1, C, H', W'], bit-identical to ``stitch``.  With
    ``u8`` it returns ``(map, (map * 255).astype(uint8))``: the second is ctd's postprocess_mask (ctd.py:41-44) of the stitched mask."""
    import ctypes as C

    import torch

    from . import lib as _lib, ops

    if maps_dev.dim() == 3:
        maps_dev = maps_dev[:, None]
    if maps_dev.dtype != torch.float32 or maps_dev.dim() != 4 or maps_dev.shape[2] != maps_dev.shape[3] or not maps_dev.is_cuda:
        raise ValueError(f"stitch_gpu expects float32 device squares [n,C,m,m], got {maps_dev.dtype} {tuple(maps_dev.shape)} on {maps_dev.device}")
    n, ch, m, _ = (int(v) for v in maps_dev.shape)
    if n != pl.p_num:
        raise ValueError(f"stitch_gpu: {n} squares for a plan of {pl.p_num}")
    step, pw, hh, starts = stitch_geometry(pl, m)
    if any(b < a for a, b in zip(starts, starts[1:])) or starts[0] < 0:
        raise ValueError("stitch_gpu: band starts must not decrease")
    dev = maps_dev.device
    starts_dev = torch.tensor(starts, dtype=torch.int32).to(dev)
    shape = (1, ch, pw, hh) if pl.transpose else (1, ch, hh, pw)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    out_u8 = torch.empty(shape, dtype=torch.uint8, device=dev) if u8 else None
    sn, sc, sy, sx = (int(v) for v in maps_dev.stride())
    _lib.check(_lib.load().mit_rearrange_stitch(maps_dev.data_ptr(), n, ch, m, sn, sc, sy, sx, int(pl.transpose), pl.pw_num, pl.ph_num, step, pw,
                                                hh, starts_dev.data_ptr(), out.data_ptr(), out_u8.data_ptr() if u8 else None, int(u8),
                                                C.c_void_p(ops.current_stream())), "mit_rearrange_stitch")
    return (out, out_u8) if u8 else out


def forward_gpu(page_dev, batch_forward_dev: Callable, tgt_size: int, max_batch_size: int = 4, mask_u8: bool = False):
    """``forward`` with the page on the device: -> (db [1,2,H',W'], mask [1,1,H'',W'']) device tensors, or (None, None) when the page
    needs no tiling.  ``batch_forward_dev(u8 [n<=max_batch_size, tgt, tgt, 3] device) -> (db [n,2,m,m], mask [n,1,m',m'] or [n,m',m'])``
    float32 device tensors of any strides; they may be views of a workspace that the next call overwrites (a strip of more than
    ``max_batch_size`` squares collects them in a buffer of its own, a smaller one stitches the views as they are).  ``mask_u8``: the
    mask comes back as ``(mask, mask_u8)`` (``stitch_gpu(..., u8=True)``)."""
    import torch

    pl = plan(int(page_dev.shape[0]), int(page_dev.shape[1]), tgt_size)
    if pl is None:
        return None, None
    sq = squares_gpu(page_dev, pl, tgt_size)
    if pl.p_num <= max_batch_size:
        db, mask = batch_forward_dev(sq)
    else:
        db = mask = None
        for i in range(0, pl.p_num, max_batch_size):
            d, m = batch_forward_dev(sq[i:i + max_batch_size])
            if db is None:
                db = torch.empty((pl.p_num,) + tuple(d.shape[1:]), dtype=d.dtype, device=d.device)
                mask = torch.empty((pl.p_num,) + tuple(m.shape[1:]), dtype=m.dtype, device=m.device)
            db[i:i + max_batch_size] = d
            mask[i:i + max_batch_size] = m
    return stitch_gpu(db, pl), stitch_gpu(mask, pl, u8=mask_u8)
