"""ESRGAN 4x upscaler (``--upscaler 4xultrasharp``: RRDBNet with the ``4x-UltraSharp`` weights) on the gfx950 engine.

Same network as ``RRDBNet(3, 3, nf=64, nb=23, upscale=4)`` of the reference
(/root/reference/manga_translator/upscaling/esrgan_pytorch.py:28-167) and the tensor part of
``ESRGANUpscalerPytorch._infer`` (:537-546).  MI355X layout:

* fp32 NHWC; every dense block works in ONE ``[B,H,W,192]`` buffer ``[x | x1 | x2 | x3 | x4]``: conv_k reads the first
  64+32(k-1) channels and writes its 32 outputs into the next slice, so the four torch.cat of
  ``ResidualDenseBlock_5C.forward`` (:152-166) cost nothing; conv5's epilogue does ``* 0.2 + x`` and writes the next block's x;
* nearest-x2 + 3x3 conv (upconv_block :317-324) as four 2x2 parity convolutions on the low-resolution tensor
  (ops.UpsampleConv2d): no 4x / 16x sized upsampled intermediates, 2.25x fewer MACs;
* the BGR flip of :541/:545 lives in the first conv's input-channel order and the last conv's output-channel order; the
  3-channel output conv runs on the VALU small-Cout kernel; clip + x255 truncation to uint8 on the GPU.

``precision="bf16"`` (opt-in; fp32 is the default and its code path is the one above, untouched): the dense blocks run on
``mit_rdb_conv3x3_bf16`` (csrc/rdb_bf16.hip) with the ``[x | x1 | x2 | x3 | x4]`` buffers held as bf16, while the residual trunk — every
dense block's 64-channel x, the RRDB input, ``fea`` — stays fp32: conv5 reads it as ``post`` and writes the next x both as fp32 (the
master copy) and as bf16 (the next block's operand).  Only convolution operands are ever rounded, so rounding does not accumulate
along the 69 blocks (torch.autocast also rounds every layer output and adds the residuals in bf16).  The RRDB's outer
``* 0.2 + rrdb_in`` rides in the third conv5's epilogue.  trunk / up1 / up2 / hr0 take the one-product bf16 tiles of ``mit_conv_gemm``
(``nprod = 1``); ``fea`` (Cin 4) and the 3-channel output convolution stay fp32.

``upscale`` adds what surrounds the network in the reference, still on the device: Pillow's BILINEAR resize by ratio / 4 after every
pass (:546), the pass loop of ``CommonUpscaler.upscale`` (upscaling/common.py:10-33) and its BICUBIC correction (:32), through
``imgproc.pil_resize_u8`` (csrc/pil_resample.hip, byte-identical to Pillow).  Only the final page leaves the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import lib as _lib
from . import ops
from .ops import ACT_LEAKY, ACT_NONE, PAD_ZERO

NF, GC = 64, 32
VALID_UPSCALE_RATIOS = (2, 3, 4)   # ESRGANUpscalerPytorch._VALID_UPSCALE_RATIOS (esrgan_pytorch.py:519)


def pass_size(w: int, h: int, ratio: float) -> Tuple[int, int]:
    """(w, h) one ``_infer(…, ratio)`` returns for a (w, h) page: the 4x output resized by ratio / 4 (esrgan_pytorch.py:539,546)."""
    r = ratio / 4
    return int(round(4 * w * r)), int(round(4 * h * r))


def upscale_plan(w: int, h: int, upscale_ratio: float, valid: Sequence[float] = VALID_UPSCALE_RATIOS):
    """The size arithmetic of ``CommonUpscaler.upscale`` (upscaling/common.py:10-33) for a (w, h) page: ([(pass ratio, (w, h) after the
    pass)], correction (w, h) or None).  Passes are taken while ``ratio_left > 0``, each the smallest valid ratio that covers what is left
    (the largest when none does); a negative rest is corrected by a resize by (ratio + ratio_left) / ratio, its sides TRUNCATED (:32)."""
    if upscale_ratio == 1:
        return [], None
    valid = sorted(valid)
    assert valid[0] > 1
    passes: List[Tuple[float, Tuple[int, int]]] = []
    ratio_left = upscale_ratio
    ratio = valid[-1]
    while ratio_left > 0:
        ratio = valid[-1]
        for v in valid:
            if ratio_left <= v:
                ratio = v
                break
        ratio_left -= ratio
        w, h = pass_size(w, h, ratio)
        passes.append((ratio, (w, h)))
    correction: Optional[Tuple[int, int]] = None
    if ratio_left < 0:
        d = (ratio + ratio_left) / ratio
        correction = (int(w * d), int(h * d))
    return passes, correction


class _RDB:
    def __init__(self, sd, p, device):
        self.convs = [ops.Conv2d(sd[f"{p}.conv{k}.0.weight"], sd[f"{p}.conv{k}.0.bias"], padding=1, act=ACT_LEAKY, alpha=0.2,
                                 device=device) for k in range(1, 5)]
        # x5 * 0.2 + x: the 0.2 rides in the epilogue scale (bias pre-multiplied), x comes in as ``post``
        self.conv5 = ops.Conv2d(sd[f"{p}.conv5.0.weight"], sd[f"{p}.conv5.0.bias"], padding=1, device=device,
                                out_scale=torch.full((NF,), 0.2))


class _RDBbf16:
    """The five convolutions of a dense block as ``ops.RdbConv3x3`` (bf16 weight packs [9 * Cin, N])."""

    def __init__(self, sd, p, device):
        self.convs = [ops.RdbConv3x3(sd[f"{p}.conv{k}.0.weight"], sd[f"{p}.conv{k}.0.bias"], act=ACT_LEAKY, alpha=0.2, device=device)
                      for k in range(1, 5)]
        self.conv5 = ops.RdbConv3x3(sd[f"{p}.conv5.0.weight"], sd[f"{p}.conv5.0.bias"], device=device, out_scale=torch.full((NF,), 0.2))


PRECISIONS = ("fp32", "bf16")


def _check_precision(precision: str, who: str) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"{who}: precision must be 'fp32' or 'bf16' (got {precision!r})")
    return precision


class EsrganEngine(ops.Engine):
    """Batched 4x upscaler: u8 RGB pages [B,H,W,3] -> u8 RGB [B,4H,4W,3] (device tensors).  ``precision``: "fp32" (default) or "bf16",
    the precision of ``forward`` / ``upscale`` calls that name none."""

    def __init__(self, sd: Dict[str, torch.Tensor], nb: int = 23, device="cuda", precision: str = "fp32"):
        super().__init__(device)
        dev = self.device
        self.nb = nb
        self.precision = _check_precision(precision, "EsrganEngine")
        # the dense blocks' bf16 packs: built now for a bf16 engine, else at the first bf16 call (an fp32 user pays no memory for them)
        self._rdb_sd = {k: v for k, v in sd.items() if ".RDB" in k}
        self.blocks_bf16: Optional[List[List[_RDBbf16]]] = None
        if precision == "bf16":
            self._ensure_bf16()
        w0 = sd["model.0.weight"].detach().float().flip(1)  # network input is BGR (:541): flip the input channels instead
        self.fea = ops.Conv2d(w0, sd["model.0.bias"], padding=1, device=dev)
        self.blocks = [[_RDB(sd, f"model.1.sub.{i}.RDB{r}", dev) for r in (1, 2, 3)] for i in range(nb)]
        self.trunk = ops.Conv2d(sd[f"model.1.sub.{nb}.weight"], sd[f"model.1.sub.{nb}.bias"], padding=1, device=dev)
        self.up1 = ops.UpsampleConv2d(sd["model.3.weight"], sd["model.3.bias"], act=ACT_LEAKY, alpha=0.2, device=dev)
        self.up2 = ops.UpsampleConv2d(sd["model.6.weight"], sd["model.6.bias"], act=ACT_LEAKY, alpha=0.2, device=dev)
        self.hr0 = ops.Conv2d(sd["model.8.weight"], sd["model.8.bias"], padding=1, act=ACT_LEAKY, alpha=0.2, device=dev)
        # output is BGR (:545 flips back): emit RGB directly by flipping the output channels
        self.hr1 = ops.ConvSmallCout(sd["model.10.weight"].detach().float().flip(0), sd["model.10.bias"].detach().float().flip(0),
                                     pad_mode=PAD_ZERO, device=dev)

    def _ensure_bf16(self) -> None:
        if self.blocks_bf16 is None:
            self.blocks_bf16 = [[_RDBbf16(self._rdb_sd, f"model.1.sub.{i}.RDB{r}", self.device) for r in (1, 2, 3)] for i in range(self.nb)]
            self._rdb_sd = None

    @torch.no_grad()
    def forward(self, img_u8: torch.Tensor, taps=None, precision: Optional[str] = None) -> torch.Tensor:
        """``precision``: "fp32" | "bf16"; None = the engine's."""
        precision = self.precision if precision is None else _check_precision(precision, "EsrganEngine.forward")
        if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[-1] != 3:
            raise ValueError(f"EsrganEngine.forward expects u8 [B,H,W,3], got {img_u8.dtype} {tuple(img_u8.shape)}")
        if precision == "bf16":
            return self._forward_bf16(img_u8.contiguous(), taps)
        img_u8 = img_u8.contiguous()
        B, H, W, _ = img_u8.shape
        lib = _lib.load()
        st = C.c_void_p(ops.current_stream())
        x4 = self._buf("in4", B, H, W, 4)
        zero_mask = self._buf("zmask", B, H, W, dtype=torch.uint8)
        zero_mask.zero_()
        # (rgb / 255 * (1 - 0), 0): the LaMa prep kernel with an all-zero mask is exactly ``float() / 255`` (:541)
        _lib.check(lib.mit_lama_prep(img_u8.data_ptr(), zero_mask.data_ptr(), x4.data_ptr(), B, H, W, st), "mit_lama_prep")
        fea = self._buf("fea", B, H, W, NF)
        self.fea(x4, out=fea)
        cat = [self._buf(f"cat{j}", B, H, W, NF + 4 * GC) for j in range(2)]  # ping-pong dense-block buffers
        t = self._buf("trunk_in", B, H, W, NF)   # RRDB input (kept for the outer residual)
        n = B * H * W * NF
        cur = 0
        cat[0][..., :NF].copy_(fea)
        src = fea
        for i, rrdb in enumerate(self.blocks):
            for r, rdb in enumerate(rrdb):
                buf = cat[cur]
                for k, conv in enumerate(rdb.convs):
                    conv(buf[..., :NF + k * GC], out=buf[..., NF + k * GC:NF + (k + 1) * GC])
                if r < 2:  # next dense block's x goes straight into the other buffer's first slice
                    rdb.conv5(buf, out=cat[cur ^ 1][..., :NF], post=buf[..., :NF])
                    cur ^= 1
                else:     # RRDB output: (x5 * 0.2 + x) * 0.2 + rrdb_in
                    o3 = self._buf("rdb3_out", B, H, W, NF)
                    rdb.conv5(buf, out=o3, post=buf[..., :NF])
                    dst = t if i + 1 == self.nb else self._buf(f"rrdb_out{i & 1}", B, H, W, NF)
                    _lib.check(lib.mit_axpy(dst.data_ptr(), 0.2, o3.data_ptr(), src.data_ptr(), n, st), "mit_axpy")
                    src = dst
                    if i + 1 < self.nb:
                        cat[cur ^ 1][..., :NF].copy_(dst)
                        cur ^= 1
        lr = self._buf("lr", B, H, W, NF)
        self.trunk(src, out=lr, post=fea)  # ShortcutBlock: fea + LR_conv(trunk)
        if taps is not None:
            taps["lr"] = lr.clone()
        u1 = self._buf("u1", B, 2 * H, 2 * W, NF)
        self.up1(lr, out=u1)
        u2 = self._buf("u2", B, 4 * H, 4 * W, NF)
        self.up2(u1, out=u2)
        h0 = self._buf("h0", B, 4 * H, 4 * W, NF)
        self.hr0(u2, out=h0)
        y = self._buf("y", B, 4 * H, 4 * W, 3)
        self.hr1(h0, out=y)
        if taps is not None:
            taps["out_float"] = y.clone()
        out = torch.empty(B, 4 * H, 4 * W, 3, dtype=torch.uint8, device=self.device)
        _lib.check(lib.mit_map_to_u8(y.data_ptr(), out.data_ptr(), y.numel(), 2, 0.0, st), "mit_map_to_u8")
        return out

    def _prep(self, img_u8: torch.Tensor, st) -> torch.Tensor:
        """u8 RGB [B,H,W,3] -> ``fea`` [B,H,W,64] fp32 (the engine's first convolution on rgb / 255)."""
        B, H, W, _ = img_u8.shape
        lib = _lib.load()
        x4 = self._buf("in4", B, H, W, 4)
        zero_mask = self._buf("zmask", B, H, W, dtype=torch.uint8)
        zero_mask.zero_()
        _lib.check(lib.mit_lama_prep(img_u8.data_ptr(), zero_mask.data_ptr(), x4.data_ptr(), B, H, W, st), "mit_lama_prep")
        fea = self._buf("fea", B, H, W, NF)
        self.fea(x4, out=fea)
        return fea

    @staticmethod
    def _p1(x: torch.Tensor) -> int:
        """nprod for a ``mit_conv_gemm`` layer of the bf16 precision reading ``x``: 1 while one image of ``x`` stays below the 2^31
        elements the one-product tiles address, else 0 (that layer in fp32: hr0 of a page above 2 M low-resolution pixels)."""
        return 1 if x.shape[1] * x.stride(1) < 2 ** 31 else 0

    def _forward_bf16(self, img_u8: torch.Tensor, taps=None) -> torch.Tensor:
        self._ensure_bf16()
        B, H, W, _ = img_u8.shape
        lib = _lib.load()
        st = C.c_void_p(ops.current_stream())
        fea = self._prep(img_u8, st)
        cat = [self._buf(f"cat{j}", B, H, W, NF + 4 * GC, dtype=torch.bfloat16) for j in range(2)]
        xa, xb = self._buf("rdb_x0", B, H, W, NF), self._buf("rdb_x1", B, H, W, NF)   # fp32 master copies of the dense blocks' x
        t = self._buf("trunk_in", B, H, W, NF)
        cur = 0
        ops.cast_bf16(fea, cat[0][..., :NF])
        src = fea
        for i, rrdb in enumerate(self.blocks_bf16):
            x = src
            for r, rdb in enumerate(rrdb):
                buf, nxt = cat[cur], cat[cur ^ 1][..., :NF]
                for k, conv in enumerate(rdb.convs):
                    conv(buf[..., :NF + k * GC], out_bf16=buf[..., NF + k * GC:NF + (k + 1) * GC])
                if r < 2:    # x5 * 0.2 + x: fp32 master and the next block's bf16 operand in one launch
                    xn = xb if r else xa
                    rdb.conv5(buf, post=x, out_f32=xn, out_bf16=nxt)
                    x = xn
                else:        # RRDB output (x5 * 0.2 + x) * 0.2 + rrdb_in, in the same epilogue
                    last = i + 1 == self.nb
                    dst = t if last else self._buf(f"rrdb_out{i & 1}", B, H, W, NF)
                    rdb.conv5(buf, post=x, post2=src, s2=0.2, out_f32=dst, out_bf16=None if last else nxt)
                    src = dst
                cur ^= 1
        lr = self._buf("lr", B, H, W, NF)
        self.trunk(src, out=lr, post=fea, nprod=self._p1(src))
        if taps is not None:
            taps["lr"] = lr.clone()
        u1 = self._buf("u1", B, 2 * H, 2 * W, NF)
        self.up1(lr, out=u1, nprod=self._p1(lr))
        u2 = self._buf("u2", B, 4 * H, 4 * W, NF)
        self.up2(u1, out=u2, nprod=self._p1(u1))
        h0 = self._buf("h0", B, 4 * H, 4 * W, NF)
        self.hr0(u2, out=h0, nprod=self._p1(u2))
        y = self._buf("y", B, 4 * H, 4 * W, 3)
        self.hr1(h0, out=y)
        if taps is not None:
            taps["out_float"] = y.clone()
        out = torch.empty(B, 4 * H, 4 * W, 3, dtype=torch.uint8, device=self.device)
        _lib.check(lib.mit_map_to_u8(y.data_ptr(), out.data_ptr(), y.numel(), 2, 0.0, st), "mit_map_to_u8")
        return out

    @torch.no_grad()
    def upscale(self, pages_u8: torch.Tensor, upscale_ratio: float, precision: Optional[str] = None) -> torch.Tensor:
        """``CommonUpscaler.upscale`` around ``_infer`` for u8 RGB pages [B,H,W,3] of one size, on the device: per pass ``forward`` and
        Pillow's BILINEAR resize to ``pass_size``; a BICUBIC correction when the ratios overshoot; ratio 1 returns the input.
        ``precision`` goes to every pass (None = the engine's)."""
        from . import imgproc

        precision = self.precision if precision is None else _check_precision(precision, "EsrganEngine.upscale")
        if upscale_ratio == 1:
            return pages_u8
        if pages_u8.dim() != 4:
            raise ValueError(f"EsrganEngine.upscale expects u8 [B,H,W,3], got {tuple(pages_u8.shape)}")
        passes, correction = upscale_plan(int(pages_u8.shape[2]), int(pages_u8.shape[1]), upscale_ratio)
        x = pages_u8
        for _, size in passes:
            x = imgproc.pil_resize_u8(self.forward(x, precision=precision), size, "bilinear")
        if correction is not None:
            x = imgproc.pil_resize_u8(x, correction, "bicubic")
        return x

    def flops_per_input_pixel(self) -> float:
        """Executed MACs x 2 per low-resolution pixel (the up-convs counted at their merged 2x2 form)."""
        rdb = 9 * (sum((NF + k * GC) * GC for k in range(4)) + (NF + 4 * GC) * NF)
        lr = 9 * 3 * NF + self.nb * 3 * rdb + 9 * NF * NF
        hr = 4 * 4 * NF * NF + 16 * 4 * NF * NF + 16 * 9 * NF * NF + 16 * 9 * NF * 3
        return 2.0 * (lr + hr)
