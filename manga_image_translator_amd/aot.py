"""AOT inpainter (the reference's ``Inpainter.default``) on the gfx950 engine.

Same network as ``AOTGenerator`` of the reference (manga_translator/inpainting/inpainting_aot.py:240-274) with the tensor
pre/post of the plugin path it inherits (inpainting_lama_mpe.py:_infer :82-117), laid out for MI355X:

* activations fp32 NHWC;
* scaled weight standardisation (:53-118) is folded into the weights once, at load;
* every gated layer (:120-146) is ONE ``mit_conv_gemm`` launch over the signal and gate weights concatenated along N
  (2 Cout columns), followed by ``mit_aot_gate`` (signal * sigmoid(gate) * 1.8, + relu_nf);
* reflect padding is the GEMM's own padding mode; the four dilated branches of an AOTBlock (:170-193) are four launches with
  taps (ky*r - r, kx*r - r), each writing its 32-channel slice of the 128-channel concatenation (no torch.cat);
* tail[0] / tail[2] (3x3, stride 1, 128 channels) run as Winograd F(4x4, 3x3), as LaMa's blocks do; the blocks' fuse / gate
  stay direct by default (see ``AotEngine.__init__``);
* my_layer_norm's plane statistics (``mit_aot_plane_stats``) and the blend (``mit_aot_blend``) are their own memory-bound
  kernels; the last gated layer, clip, u8 conversion and composite are one (``mit_aot_post``);
* uint8 pages in, uint8 pages out.

Precision "bf16" (opt-in; the reference's GPU path runs this generator under ``torch.autocast(bfloat16)``,
inpainting_lama_mpe.py:97-107): the four dilated branches of each of the ten blocks are ONE ``mit_aot_conv3x3_bf16`` launch
(csrc/aot_bf16.hip) that reads a bf16 copy of X and writes the concatenation, while X, the residual trunk that the blend reads and
writes, the plane statistics and the blend stay fp32: only convolution operands are rounded.  fuse and gate (128 -> 128, rate 1) take
the one-product bf16 tiles of ``mit_conv_gemm`` (``nprod=1``), which were measured faster for that shape than the new kernel
(``AotEngine.BF16_NATIVE``), as do head.2 / head.4 and tail.0 .. tail.6 (tail.0 / tail.2 in the direct form, not Winograd,
as LaMa's bf16 precision does); head.0 (4 input channels) and tail.8 (6 output columns) stay fp32.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import aot_schema, ops, synth
from . import lib as _lib
from .ops import ACT_RELU, PAD_REFLECT

PRECISIONS = ("fp32", "bf16")
MIN_SIDE = 72   # ReflectionPad2d(16) needs a 1/4-resolution side > 16; with the pad-to-8 resize that is 72


def fold_ws(weight: torch.Tensor, gain: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
    """ScaledWSConv2d.get_weight / ScaledWSTransposeConv2d.get_weight (:68-75, :104-111) in the reference's own fp32 torch
    arithmetic, so the folded weights are bit-identical to the reference's.  Statistics over dims (1, 2, 3): per output channel
    for [Cout, Cin, kh, kw], per INPUT channel for a transposed layer's [Cin, Cout, kh, kw]."""
    w = weight.detach().to(torch.float32).cpu()
    fan_in = np.prod(w.shape[1:])
    var, mean = torch.var_mean(w, dim=(1, 2, 3), keepdim=True)
    scale = torch.rsqrt(torch.max(var * fan_in, torch.tensor(eps).to(var.device))) * gain.detach().to(torch.float32).cpu().view_as(var)
    shift = mean * scale
    return w * scale - shift


def _check_precision(precision: str, who: str) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"{who}: precision must be 'fp32' or 'bf16' (got {precision!r})")
    return precision


class _Gated:
    """One gated layer: the signal and gate convolutions as one launch of 2 Cout columns."""

    def __init__(self, sd, p: str, k: int, stride: int, transposed: bool, winograd: bool, device):
        w = fold_ws(sd[p + ".conv.weight"], sd[p + ".conv.gain"])
        wg = fold_ws(sd[p + ".conv_gate.weight"], sd[p + ".conv_gate.gain"])
        b = torch.cat([sd[p + ".conv.bias"], sd[p + ".conv_gate.bias"]]).to(torch.float32)
        self.transposed, self.wino = transposed, False
        if transposed:   # GatedWSTransposeConvPadded: zero padding (k - 1) // 2, output padding 0 (:135-146)
            self.cout = w.shape[1]
            self.conv = ops.ConvTranspose2d(torch.cat([w, wg], 1), b, stride=stride, padding=(k - 1) // 2, device=device)
        else:            # GatedWSConvPadded: ReflectionPad2d((k - 1) // 2) + the convolution (:120-133)
            self.cout = w.shape[0]
            wc = torch.cat([w, wg], 0)
            if winograd and k == 3 and stride == 1 and wc.shape[1] % 4 == 0 and wc.shape[1] >= 64:
                self.wino = True
                self.conv = ops.WinogradConv3x3(wc, b, pad_mode=PAD_REFLECT, device=device)
            else:
                self.conv = ops.Conv2d(wc, b, stride=stride, padding=(k - 1) // 2, pad_mode=PAD_REFLECT, device=device)


class AotEngine(ops.Engine):
    """Batched AOT generator. ``forward(img_u8[B,H,W,3], mask_u8[B,H,W]) -> u8 [B,H,W,3]`` (device tensors), pages run in
    micro-batches of ``mb``."""

    # The convolutions of a block that the bf16 precision runs on ``mit_aot_conv3x3_bf16``; one left out runs on the one-product tiles
    # of ``mit_conv_gemm`` instead (DESIGN.md has the measurements behind the choice).  Never a function of the batch size.
    BF16_NATIVE = frozenset({"branches"})

    def __init__(self, sd: Dict[str, torch.Tensor], device="cuda", winograd: bool = True, mb: int = 4, block_winograd: bool = False,
                 precision: str = "fp32"):
        """``winograd``: the 3x3 stride-1 128-channel layers as Winograd F(4x4, 3x3) — tail[0] / tail[2] always, the blocks' fuse /
        gate only with ``block_winograd`` too.  Off by default in the blocks: the blend's sigmoid(5 * (2 z - 1)) amplifies rounding
        from block to block, and Winograd's larger rounding there doubled the distance to a float64 oracle after ten blocks
        (1.5e-4 -> 2.5e-4 at 256 x 184 in the split mode).
        ``precision``: "fp32" (default) or "bf16", the precision of ``forward`` calls that name none.  The bf16 weight packs are
        built now for a bf16 engine, else at the first bf16 call (an fp32 user pays no memory for them)."""
        synth.check_state_dict(sd, aot_schema.aot_generator_schema(), "AOT generator")
        super().__init__(device)
        self.mb = int(mb)
        if self.mb < 1:
            raise ValueError("AotEngine: mb must be >= 1")
        self.precision = _check_precision(precision, "AotEngine")
        dev = self.device
        self._winograd = bool(winograd)
        self._bf16_sd = {k: v for k, v in sd.items() if k.startswith(("body_conv.", "tail.0.", "tail.2."))}   # references, until packed
        self.blocks_bf16 = None    # [(branches, fuse, gate) as ops.AotConv3x3, then (fuse, gate) as direct ops.Conv2d for nprod = 1]
        self.tail_bf16 = None      # tail.0 / tail.2 in the direct form
        self.head = [_Gated(sd, "head.0", 3, 1, False, winograd, dev), _Gated(sd, "head.2", 4, 2, False, winograd, dev),
                     _Gated(sd, "head.4", 4, 2, False, winograd, dev)]
        C4 = 4 * aot_schema.CH
        self.blocks = []
        for i in range(aot_schema.N_BLOCKS):
            p = f"body_conv.{i}"
            br = [ops.Conv2d(sd[f"{p}.block{j:02d}.1.weight"], sd[f"{p}.block{j:02d}.1.bias"], padding=r, dilation=r, pad_mode=PAD_REFLECT,
                             act=ACT_RELU, device=dev) for j, r in enumerate(aot_schema.RATES)]
            if winograd and block_winograd:
                fuse = ops.WinogradConv3x3(sd[p + ".fuse.1.weight"], sd[p + ".fuse.1.bias"], pad_mode=PAD_REFLECT, device=dev)
                gate = ops.WinogradConv3x3(sd[p + ".gate.1.weight"], sd[p + ".gate.1.bias"], pad_mode=PAD_REFLECT, device=dev)
            else:
                fuse = ops.Conv2d(sd[p + ".fuse.1.weight"], sd[p + ".fuse.1.bias"], padding=1, pad_mode=PAD_REFLECT, device=dev)
                gate = ops.Conv2d(sd[p + ".gate.1.weight"], sd[p + ".gate.1.bias"], padding=1, pad_mode=PAD_REFLECT, device=dev)
            self.blocks.append((br, fuse, gate))
        self.C = C4
        self.tail = [_Gated(sd, "tail.0", 3, 1, False, winograd, dev), _Gated(sd, "tail.2", 3, 1, False, winograd, dev),
                     _Gated(sd, "tail.4", 4, 2, True, winograd, dev), _Gated(sd, "tail.6", 4, 2, True, winograd, dev),
                     _Gated(sd, "tail.8", 3, 1, False, winograd, dev)]
        if self.precision == "bf16":
            self._ensure_bf16()

    def _ensure_bf16(self) -> None:
        if self.blocks_bf16 is not None:
            return
        sd, dev = self._bf16_sd, self.device
        blocks = []
        for i in range(aot_schema.N_BLOCKS):
            p = f"body_conv.{i}"
            names = [f"{p}.block{j:02d}.1" for j in range(len(aot_schema.RATES))]
            br = ops.AotConv3x3([sd[n + ".weight"] for n in names], [sd[n + ".bias"] for n in names], aot_schema.RATES, act=ACT_RELU,
                                device=dev)
            fuse, gate = (ops.AotConv3x3([sd[f"{p}.{nm}.1.weight"]], [sd[f"{p}.{nm}.1.bias"]], [1], device=dev)
                          if nm in self.BF16_NATIVE else None for nm in ("fuse", "gate"))   # packed only where the engine launches them
            # the same two on the one-product tiles: the engine's own direct layers, or direct ones packed here beside Winograd ones
            p1 = tuple(l if isinstance(l, ops.Conv2d) else ops.Conv2d(sd[f"{p}.{nm}.1.weight"], sd[f"{p}.{nm}.1.bias"], padding=1,
                                                                      pad_mode=PAD_REFLECT, device=dev)
                       for nm, l in zip(("fuse", "gate"), self.blocks[i][1:]))
            blocks.append((br, fuse, gate) + p1)
        # tail.0 / tail.2: the direct 9-tap form (a Winograd engine packs it here; a direct engine's own layers serve)
        self.tail_bf16 = [_Gated(sd, "tail.0", 3, 1, False, False, dev), _Gated(sd, "tail.2", 3, 1, False, False, dev)] if self._winograd \
            else self.tail[:2]
        self.blocks_bf16 = blocks
        self._bf16_sd = None

    # -- pieces ------------------------------------------------------------------------------------------------------------------
    def _conv(self, layer, x: torch.Tensor, out: torch.Tensor):
        """Plain or Winograd 3x3 launch(es) of ``layer`` from x into out."""
        if isinstance(layer, ops.WinogradConv3x3):
            B, H, W, Cx = x.shape
            T = layer.tiles(B, H, W)
            layer(x, out=out, v=self._buf("wino_v", 36, T, Cx), m=self._buf("wino_m", 36, T, layer.Cout))
        else:
            layer(x, out=out)

    def _gated(self, g: _Gated, x: torch.Tensor, out: torch.Tensor, relu_nf: bool, pair_name: str, nprod: int = 0):
        """x -> (signal | gate) pair [B,Ho,Wo,2C] -> out [B,Ho,Wo,C].  ``nprod`` = 1: the convolution on the one-product bf16 tiles
        (a direct or transposed layer)."""
        B, Ho, Wo, Co = out.shape
        pair = self._buf(pair_name, B, Ho, Wo, 2 * Co)
        if nprod:
            g.conv(x, out=pair, nprod=nprod)
        else:
            self._conv(g.conv, x, pair)
        _lib.check(_lib.load().mit_aot_gate(pair.data_ptr(), 2 * Co, out.data_ptr(), out.stride(2), B * Ho * Wo, Co, int(relu_nf),
                                            C.c_void_p(ops.current_stream())), "mit_aot_gate")

    def plane_stats(self, g: torch.Tensor, mean: torch.Tensor, istd: torch.Tensor):
        """mit_aot_plane_stats of a pixel-dense NHWC [B,h,w,C] tensor into mean / istd [B, C]."""
        B, h, w, Cc = g.shape
        if g.stride(2) != Cc or g.stride(1) != w * Cc:
            raise ValueError("plane_stats: pixel-dense NHWC input expected")
        nbytes = int(_lib.load().mit_aot_plane_stats_ws(B, h * w, Cc))
        ws = self._buf("stats_ws", (nbytes + 7) // 8, dtype=torch.float64)
        _lib.check(_lib.load().mit_aot_plane_stats(g.data_ptr(), g.stride(0), Cc, B, h * w, Cc, ws.data_ptr(), ws.numel() * 8,
                                                   mean.data_ptr(), istd.data_ptr(), C.c_void_p(ops.current_stream())),
                   "mit_aot_plane_stats")

    def _block(self, blk, X: torch.Tensor):
        """AOTBlock.forward (:187-193), in place over X."""
        br, fuse, gate = blk
        B, h, w, Cc = X.shape
        cat = self._buf("cat", B, h, w, Cc)
        q = Cc // len(br)
        for j, conv in enumerate(br):
            conv(X, out=cat[..., j * q:(j + 1) * q])
        F_ = self._buf("fuse", B, h, w, Cc)
        G = self._buf("gate", B, h, w, Cc)
        self._conv(fuse, cat, F_)
        self._conv(gate, X, G)
        mean, istd = self._buf("ln_mean", B, Cc), self._buf("ln_istd", B, Cc)
        self.plane_stats(G, mean, istd)
        _lib.check(_lib.load().mit_aot_blend(X.data_ptr(), X.stride(0), X.stride(2), F_.data_ptr(), F_.stride(0), F_.stride(2), G.data_ptr(),
                                             G.stride(0), G.stride(2), mean.data_ptr(), istd.data_ptr(), B, h * w, Cc,
                                             C.c_void_p(ops.current_stream())), "mit_aot_blend")

    def _block_bf16(self, i: int, X: torch.Tensor):
        """AOTBlock.forward (:187-193) in the bf16 precision, in place over the fp32 X: the convolutions read bf16 copies of their
        operands (X, the concatenation), everything else is ``_block``'s."""
        br, fuse, gate, fuse32, gate32 = self.blocks_bf16[i]
        br32 = self.blocks[i][0]
        native = self.BF16_NATIVE
        B, h, w, Cc = X.shape
        F_ = self._buf("fuse", B, h, w, Cc)
        G = self._buf("gate", B, h, w, Cc)
        Xb = catb = cat = None
        if "branches" in native or "gate" in native:
            Xb = ops.cast_bf16(X, self._buf("X_bf16", B, h, w, Cc, dtype=torch.bfloat16))
        if "fuse" in native:
            catb = self._buf("cat_bf16", B, h, w, Cc, dtype=torch.bfloat16)
        if "fuse" not in native or "branches" not in native:
            cat = self._buf("cat", B, h, w, Cc)
        if "branches" in native:
            br(Xb, out_bf16=catb, out_f32=None if "fuse" in native else cat)
        else:
            q = Cc // len(br32)
            for j, conv in enumerate(br32):
                conv(X, out=cat[..., j * q:(j + 1) * q], nprod=1)
            if catb is not None:
                ops.cast_bf16(cat, catb)
        if "fuse" in native:
            fuse(catb, out_f32=F_)
        else:
            fuse32(cat, out=F_, nprod=1)
        if "gate" in native:
            gate(Xb, out_f32=G)
        else:
            gate32(X, out=G, nprod=1)
        mean, istd = self._buf("ln_mean", B, Cc), self._buf("ln_istd", B, Cc)
        self.plane_stats(G, mean, istd)
        _lib.check(_lib.load().mit_aot_blend(X.data_ptr(), X.stride(0), X.stride(2), F_.data_ptr(), F_.stride(0), F_.stride(2), G.data_ptr(),
                                             G.stride(0), G.stride(2), mean.data_ptr(), istd.data_ptr(), B, h * w, Cc,
                                             C.c_void_p(ops.current_stream())), "mit_aot_blend")

    # -- full generator ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, img_u8: torch.Tensor, mask_u8: torch.Tensor, taps: Optional[dict] = None, composite: bool = True,
                precision: Optional[str] = None) -> torch.Tensor:
        """AOTGenerator.forward (:265-274) + the tensor pre/post of _infer (:82-117) for pages whose H, W are multiples of 8 and at
        least 72.  img_u8 [B,H,W,3] u8, mask_u8 [B,H,W] u8 (device) -> u8 [B,H,W,3].  ``composite=False`` returns
        ``img_inpainted`` (:114, the network's bytes everywhere) instead of the composite of :117.  ``taps``: filled with NHWC
        copies of 'head', 'block{i}' and 'preclip' (diagnostics).  ``precision``: "fp32" | "bf16"; None = the engine's.  A page's
        bytes in either precision do not depend on the pages that travel with it."""
        if precision is not None:
            _check_precision(precision, "AotEngine.forward")
        if img_u8.dtype != torch.uint8 or mask_u8.dtype != torch.uint8:
            raise ValueError("AotEngine.forward expects uint8 page and mask tensors")
        if img_u8.dim() != 4 or img_u8.shape[-1] != 3 or tuple(mask_u8.shape) != tuple(img_u8.shape[:3]):
            raise ValueError(f"bad shapes: page {tuple(img_u8.shape)}, mask {tuple(mask_u8.shape)}")
        B, H, W, _ = img_u8.shape
        if H % 8 or W % 8:
            raise ValueError("AotEngine.forward: H and W must be multiples of 8 (the plugin resizes first, inpainting_lama_mpe.py:67-79)")
        if H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"AotEngine.forward: H and W must be at least {MIN_SIDE} (ReflectionPad2d(16) at 1/4 resolution, "
                             f"inpainting_aot.py:180); got {H} x {W}")
        precision = self.precision if precision is None else precision
        img_u8, mask_u8 = img_u8.contiguous(), mask_u8.contiguous()
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=self.device)
        parts = [] if taps is not None else None
        for b0 in range(0, B, self.mb):
            b1 = min(B, b0 + self.mb)
            t = {} if taps is not None else None
            self._forward_mb(img_u8[b0:b1], mask_u8[b0:b1], out[b0:b1], t, composite, precision == "bf16")
            if t is not None:
                parts.append(t)
        if taps is not None:
            for k in parts[0]:
                taps[k] = torch.cat([p[k] for p in parts]) if len(parts) > 1 else parts[0][k]
        return out

    def _forward_mb(self, img_u8, mask_u8, out, taps, composite, bf16: bool = False):
        B, H, W, _ = img_u8.shape
        if bf16:
            self._ensure_bf16()
        p1 = 1 if bf16 else 0                                   # head.0 and tail.8 stay fp32 in either precision
        tail01 = self.tail_bf16 if bf16 else self.tail[:2]
        lib = _lib.load()
        st = C.c_void_p(ops.current_stream())
        ch = aot_schema.CH
        x4 = self._buf("in4", B, H, W, 4)
        _lib.check(lib.mit_aot_prep(img_u8.data_ptr(), mask_u8.data_ptr(), x4.data_ptr(), B, H, W, st), "mit_aot_prep")
        f1 = self._buf("full", B, H, W, ch)
        self._gated(self.head[0], x4, f1, True, "pair_full")
        f2 = self._buf("half", B, H // 2, W // 2, 2 * ch)
        self._gated(self.head[1], f1, f2, True, "pair_half", p1)
        h, w = H // 4, W // 4
        X = self._buf("X", B, h, w, 4 * ch)
        self._gated(self.head[2], f2, X, False, "pair_q", p1)
        if taps is not None:
            taps["head"] = X.clone()
        for i, blk in enumerate(self.blocks):
            if bf16:
                self._block_bf16(i, X)
            else:
                self._block(blk, X)
            if taps is not None:
                taps[f"block{i}"] = X.clone()
        t1 = self._buf("cat", B, h, w, 4 * ch)
        self._gated(tail01[0], X, t1, True, "pair_q", p1)
        t2 = self._buf("fuse", B, h, w, 4 * ch)
        self._gated(tail01[1], t1, t2, True, "pair_q", p1)
        u1 = self._buf("half", B, H // 2, W // 2, 2 * ch)
        self._gated(self.tail[2], t2, u1, True, "pair_half", p1)
        u2 = self._buf("full", B, H, W, ch)
        self._gated(self.tail[3], u1, u2, True, "pair_full", p1)
        pre = self._buf("pre8", B, H, W, 8)
        self._conv(self.tail[4].conv, u2, pre[..., :6])
        preclip = self._buf("preclip", B, H, W, 3) if taps is not None else None
        _lib.check(lib.mit_aot_post(pre.data_ptr(), 8, img_u8.data_ptr(), mask_u8.data_ptr(), out.data_ptr(),
                                    None if preclip is None else preclip.data_ptr(), B, H, W, int(composite), st), "mit_aot_post")
        if taps is not None:
            taps["preclip"] = preclip.clone()

    # algorithmic FLOPs of one page: 2 * MACs of every convolution (gated layers count both halves)
    @staticmethod
    def flops_per_page(H: int, W: int) -> float:
        px, ch = H * W, aot_schema.CH
        f = 2.0 * px * 9 * 4 * 2 * ch                                   # head.0
        f += 2.0 * (px / 4) * 16 * ch * 4 * ch + 2.0 * (px / 16) * 16 * 2 * ch * 8 * ch   # head.2, head.4
        blk = 2.0 * (px / 16) * 9 * (4 * 128 * 32 + 128 * 128 + 128 * 128)
        f += aot_schema.N_BLOCKS * blk
        f += 2 * 2.0 * (px / 16) * 9 * 128 * 256                        # tail.0, tail.2
        f += 2.0 * (px / 4) * 4 * 128 * 128 + 2.0 * px * 4 * 64 * 64     # tail.4, tail.6 (4 taps per output pixel)
        f += 2.0 * px * 9 * 32 * 6                                       # tail.8
        return f
