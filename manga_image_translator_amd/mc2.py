"""The mc2 colorizer (the reference's ``Colorizer.mc2``, manga-colorization-v2) on the gfx950 engine.

Same computation as ``MangaColorizationV2._infer`` (manga_translator/colorization/manga_colorization_v2.py:42-74): FFDNet denoising
(denoising/denoiser.py), ``resize_pad`` (utils/utils.py) and ``Generator`` (networks/models.py, networks/extractor.py), laid out for
MI355X:

* activations fp32 NHWC; BatchNorm folded into per-channel epilogue scale / bias;
* dense convolutions on ``mit_conv_gemm`` (``ops.Conv2d``); the grouped 3x3 convolutions of the ResNeXt blocks on
  ``mit_grouped_conv3x3``; squeeze-and-excitation as ``mit_se_squeeze`` / ``mit_se_excite`` / ``mit_se_apply`` (the residual add and the
  encoder's ReLU inside the apply);
* every ``torch.cat`` is a buffer whose channel slices the producers write (the encoder layers and the tunnels' ``PixelShuffle``
  outputs land in the next tunnel's input directly);
* ``conv -> PixelShuffle(2) -> LeakyReLU`` is two GEMM launches, one per output row parity, whose weight columns are permuted so that
  a launch's 2C columns are the two horizontally adjacent output pixels (a column-split output map when the target is a slice);
* ``to4``, ``tunnel1`` and ``deconv_for_decoder`` never reach the reference's output and are not built; the four hint channels of
  ``to0.0``'s input are zero (``_infer`` passes no hints), so their weight columns are dropped;
* INTER_AREA resizes on ``mit_resize_u8`` mode 3; FFDNet's input / output and the generator's input / output are
  ``mit_mc2_ffd_pack`` / ``_ffd_unpack`` / ``_gen_in`` / ``_post``;
* uint8 pages in, uint8 images out.

``precision="bf16"`` (opt-in; fp32 is the default and its code path is the one above, untouched):

* FFDNet keeps its activations in HBM as bf16.  ``mit_mc2_ffd_pack``'s 16 fp32 channels are cast into a zeroed 32-channel bf16 buffer;
  layer 0 (its weight rows for c >= 15 zero, ``ffd_layer0_weight``) and the ten 96 -> 96 layers (folded BN as scale / bias, ReLU) run on
  ``mit_conv3x3_bf16`` between two bf16 buffers; the last of them also writes fp32, which the 96 -> 12 output layer reads as it does in
  fp32.  FFDNet is a plain chain without a residual trunk, so the resident bf16 rounds exactly what rounding the convolution operands
  would round.
* In the generator every dense convolution with K = Cin kh kw >= 64 and N >= 16 (``one_product``) runs on the one-product bf16 tiles of
  ``mit_conv_gemm`` (``nprod = 1``), the two launches of each ``_PixelShuffleConv`` included; ``encoder.conv1`` (K = 49), ``to0.0``
  (K = 9) and ``exit.2`` (N = 3) stay fp32, and so do the grouped convolutions, squeeze-and-excitation, the resizes, the glue kernels
  and every activation buffer.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import imgproc, mc2_schema as S, ops, synth
from . import lib as _lib
from .ops import ACT_LEAKY, ACT_NONE, ACT_RELU, bn_params

LEAK = 0.2
FFD_CAP = 1200
PRECISIONS = ("fp32", "bf16")
FFD_CIN_BF16 = 32      # FFDNet's 15 (+ 1 pad) input channels in the bf16 precision: one 32-channel chunk of mit_conv3x3_bf16
# The layers of the bf16 FFDNet as one launch of 96 columns (None) or as launches of these column counts: the same bits either way
# (tests/test_conv3x3_bf16_gpu.py).  Measured on the 96 -> 96 layer of four 1200 x 853 pages (profiles/README.md, r30a): 440 us in one
# launch (83 KB of LDS, one workgroup a CU), 283 us as 64 + 32 (two workgroups a CU), 346 us on mit_conv_gemm with nprod = 1.
FFD_SPLIT_BF16 = (64, 32)


def _check_precision(precision: str, who: str) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"{who}: precision must be 'fp32' or 'bf16' (got {precision!r})")
    return precision


def one_product(cin: int, kh: int, kw: int, n: int) -> bool:
    """Whether a dense convolution of the generator runs with ``nprod = 1`` in the bf16 precision: K = cin kh kw >= 64 and n >= 16
    (``cin`` = the input channels the layer really has: 1 for ``encoder.conv1`` and the sliced ``to0.0``)."""
    return cin * kh * kw >= 64 and n >= 16


def generator_dense_convs():
    """(key, cout, cin, k) of every dense convolution the engine builds from the generator's schema — the grouped ``conv2`` /
    ``conv_conv``, the squeeze-and-excitation 1x1s and the layers that never reach the output (``to4``, ``tunnel1``,
    ``deconv_for_decoder``) left out; ``to0.0`` with the one input channel it keeps."""
    out = []
    for key, shape, kind in S.generator_schema():
        if not key.endswith(".weight") or len(shape) != 4 or kind == "convT":
            continue
        name = key[:-len(".weight")]
        if ".selayer." in name or name.endswith(".conv_conv") or (name.startswith("encoder.layer") and name.endswith(".conv2")):
            continue
        if name.startswith(("to4.", "tunnel1.", "deconv_for_decoder.")):
            continue
        cout, cin, k, _ = shape
        out.append((name, cout, 1 if name == "to0.0" else cin, k))
    return out


def ffd_layer0_weight(fsd) -> torch.Tensor:
    """FFDNet's first weight [96, 15, 3, 3] as the bf16 precision's layer 0 takes it: [96, 32, 3, 3], input channels 15 .. 31 zero."""
    return ops.pad_cin_weight(fsd["intermediate_dncnn.itermediate_dncnn.0.weight"], FFD_CIN_BF16)


def _st():
    return C.c_void_p(ops.current_stream())


class _Grouped:
    """A grouped 3x3 convolution (stride / dilation = padding), optional folded BN, activation."""

    def __init__(self, w, C_, stride, dil, act, bn=None, device="cuda"):
        self.w = w.detach().to(torch.float32).contiguous().to(device)
        self.C, self.cpg = C_, w.shape[1]
        self.stride, self.dil, self.act = stride, dil, act
        self.scale = self.bias = None
        if bn is not None:
            sc, bi = ops.fold_bn(*bn)
            self.scale, self.bias = sc.to(device).contiguous(), bi.to(device).contiguous()

    def __call__(self, x, out):
        B, H, W, Cx = x.shape
        _lib.check(_lib.load().mit_grouped_conv3x3(x.data_ptr(), x.stride(0), x.stride(2), B, H, W, self.C, self.cpg, self.stride, self.dil,
                                                   self.w.data_ptr(), None if self.scale is None else self.scale.data_ptr(),
                                                   None if self.bias is None else self.bias.data_ptr(), self.act, LEAK, out.data_ptr(),
                                                   out.stride(0), out.stride(2), _st()), "mit_grouped_conv3x3")


class _SE:
    def __init__(self, sd, p, device):
        c = sd[p + ".conv2.weight"].shape[0]
        self.C = c
        self.w1 = sd[p + ".conv1.weight"].reshape(c // 16, c).to(torch.float32).contiguous().to(device)
        self.b1 = sd[p + ".conv1.bias"].to(torch.float32).contiguous().to(device)
        self.w2 = sd[p + ".conv2.weight"].reshape(c, c // 16).to(torch.float32).contiguous().to(device)
        self.b2 = sd[p + ".conv2.bias"].to(torch.float32).contiguous().to(device)


class _PixelShuffleConv:
    """Conv2d(C, 4 Cp, 3, padding=1) -> PixelShuffle(2) -> LeakyReLU(0.2) as two launches, one per output row parity i: columns
    j * Cp + c of launch i are the conv's channel c * 4 + i * 2 + j, i.e. output pixel (2y + i, 2x + j), channel c."""

    def __init__(self, w, b, device):
        self.Cp = w.shape[0] // 4
        self.convs = []
        for i in range(2):
            sel = [c * 4 + i * 2 + j for j in range(2) for c in range(self.Cp)]
            self.convs.append(ops.Conv2d(w[sel], b[sel], padding=1, act=ACT_LEAKY, alpha=LEAK, device=device))

    def __call__(self, x, out, nprod=0):
        """out: [B, 2H, 2W, Cp] (a channel slice of a wider buffer allowed)."""
        B, H, W, _ = x.shape
        P = out.stride(2)
        for i, conv in enumerate(self.convs):
            v = out.as_strided((B, H, W, 2 * self.Cp), (out.stride(0), 2 * out.stride(1), 2 * P, 1), out.storage_offset() + i * out.stride(1))
            d = conv.desc(x, v, nprod=nprod)
            if P != self.Cp:
                d.c = ops.tensor_map(v, nsplit=self.Cp, nhi=P)
            ops.launch_conv_gemm(d)


class Mc2Engine(ops.Engine):
    """``denoise`` (FFDNet), ``colorize`` (the generator) and ``forward`` (the whole ``_infer``) for B pages of one size.
    ``precision``: "fp32" (default) or "bf16", the precision of calls that name none.  The bf16 weight packs are built at the first
    bf16 call (an fp32 user pays no memory for them), or here for an engine created with ``precision="bf16"``."""

    def __init__(self, generator_sd: Dict[str, torch.Tensor], denoiser_sd: Optional[Dict[str, torch.Tensor]] = None, device="cuda",
                 precision: str = "fp32"):
        self.precision = _check_precision(precision, "Mc2Engine")
        synth.check_state_dict(generator_sd, S.generator_schema(), "mc2 generator")
        super().__init__(device)
        dev = self.device
        g = generator_sd
        # encoder
        self.conv1 = ops.Conv2d(g["encoder.conv1.weight"], stride=2, padding=3, bn=bn_params(g, "encoder.bn1"), act=ACT_RELU, device=dev)
        self.layers = []
        inplanes = 64
        for layer, planes, blocks, stride in S.ENCODER:
            blks = []
            for i in range(blocks):
                p = f"encoder.layer{layer}.{i}"
                s = stride if i == 0 else 1
                mid, out = 2 * planes, 4 * planes
                blk = dict(c1=ops.Conv2d(g[p + ".conv1.weight"], bn=bn_params(g, p + ".bn1"), act=ACT_RELU, device=dev),
                           c2=_Grouped(g[p + ".conv2.weight"], mid, s, 1, ACT_RELU, bn=bn_params(g, p + ".bn2"), device=dev),
                           c3=ops.Conv2d(g[p + ".conv3.weight"], bn=bn_params(g, p + ".bn3"), device=dev),
                           se=_SE(g, p + ".selayer", dev), stride=s, mid=mid, out=out)
                if i == 0:
                    blk["ds"] = ops.Conv2d(g[p + ".downsample.0.weight"], stride=s, bn=bn_params(g, p + ".downsample.1"), device=dev)
                blks.append(blk)
                inplanes = out
            self.layers.append(blks)
        # aux path to0..to3 (to4 unused); to0.0 keeps the sketch column only (the hint channels are zero)
        w0 = g["to0.0.weight"][:, :1]
        self.aux = [(ops.Conv2d(w0, g["to0.0.bias"], padding=1, act=ACT_LEAKY, alpha=LEAK, device=dev),
                     ops.Conv2d(g["to0.2.weight"], g["to0.2.bias"], padding=1, act=ACT_LEAKY, alpha=LEAK, device=dev))]
        # to2.2 and to3.0 read 92 channels, and the one-product tiles take multiples of 16: the bf16 precision runs them on 96 (``_wide``)
        self._wide: Dict[int, ops.Conv2d] = {}
        self._wide_sd = {(k, j): (g[f"{name}.{2 * j}.weight"], g[f"{name}.{2 * j}.bias"], st if j == 0 else 1)
                         for k, (name, _cin, _cout, st) in enumerate(S.AUX[1:4]) for j in (0, 1)
                         if g[f"{name}.{2 * j}.weight"].shape[1] % 16}
        for name, _cin, _cout, st in S.AUX[1:4]:
            self.aux.append((ops.Conv2d(g[name + ".0.weight"], g[name + ".0.bias"], stride=st, padding=1, act=ACT_LEAKY, alpha=LEAK, device=dev),
                             ops.Conv2d(g[name + ".2.weight"], g[name + ".2.bias"], padding=1, act=ACT_LEAKY, alpha=LEAK, device=dev)))
        # tunnels 4, 3, 2 (tunnel1 unused)
        self.tunnels = []
        for name, _cin, width, dils, card in S.TUNNELS[:3]:
            D = width // 2
            head = ops.Conv2d(g[name + ".0.weight"], g[name + ".0.bias"], padding=1, act=ACT_LEAKY, alpha=LEAK, device=dev)
            blks = []
            for i, d in enumerate(dils):
                p = f"{name}.2.{i}"
                blks.append(dict(r=ops.Conv2d(g[p + ".conv_reduce.weight"], act=ACT_LEAKY, alpha=LEAK, device=dev),
                                 g=_Grouped(g[p + ".conv_conv.weight"], D, 1, d, ACT_LEAKY, device=dev),
                                 e=ops.Conv2d(g[p + ".conv_expand.weight"], device=dev), se=_SE(g, p + ".selayer", dev)))
            tail = _PixelShuffleConv(g[name + ".3.weight"], g[name + ".3.bias"], dev)
            self.tunnels.append((name, width, head, blks, tail))
        self.exit0 = ops.Conv2d(g["exit.0.weight"], g["exit.0.bias"], padding=1, act=ACT_LEAKY, alpha=LEAK, device=dev)
        self.exit2 = ops.Conv2d(g["exit.2.weight"], g["exit.2.bias"], device=dev)
        # FFDNet
        self.ffd = None
        self.ffd16 = None      # the bf16 precision's layers 0 .. 10 (``_ensure_bf16``)
        self._ffd_sd = None
        if denoiser_sd is not None:
            f = synth.check_state_dict(S.strip_dataparallel(denoiser_sd), S.ffdnet_schema(), "mc2 FFDNet")
            p = "intermediate_dncnn.itermediate_dncnn"
            self.ffd = [ops.Conv2d(f[f"{p}.0.weight"], padding=1, act=ACT_RELU, device=dev)]
            for k in range(S.FFD_LAYERS - 2):
                self.ffd.append(ops.Conv2d(f[f"{p}.{2 + 3 * k}.weight"], padding=1, bn=bn_params(f, f"{p}.{3 + 3 * k}"), act=ACT_RELU, device=dev))
            self.ffd.append(ops.Conv2d(f[f"{p}.{2 + 3 * (S.FFD_LAYERS - 2)}.weight"], padding=1, device=dev))
            self._ffd_sd = {k: v for k, v in f.items() if not k.startswith(f"{p}.{2 + 3 * (S.FFD_LAYERS - 2)}.")}
        if precision == "bf16":
            self._ensure_bf16()

    def _ensure_bf16(self) -> None:
        """The bf16 packs of FFDNet's layers 0 .. 10 and the one-product planes of the generator's ``one_product`` layers."""
        if self.ffd is not None and self.ffd16 is None:
            f, p, dev = self._ffd_sd, "intermediate_dncnn.itermediate_dncnn", self.device
            layers = [ops.Conv3x3Bf16(ffd_layer0_weight(f), act=ACT_RELU, split=FFD_SPLIT_BF16, device=dev)]
            for k in range(S.FFD_LAYERS - 2):
                layers.append(ops.Conv3x3Bf16(f[f"{p}.{2 + 3 * k}.weight"], bn=bn_params(f, f"{p}.{3 + 3 * k}"), act=ACT_RELU,
                                              split=FFD_SPLIT_BF16, device=dev))
            self.ffd16, self._ffd_sd = layers, None
        if not getattr(self, "_p1_ready", False):
            for (k, j), (w, b, st) in self._wide_sd.items():   # the same layer with zero weight rows up to the next multiple of 16 channels
                wide = torch.zeros(w.shape[0], (w.shape[1] + 15) // 16 * 16, 3, 3)
                wide[:, :w.shape[1]] = w.detach().to(torch.float32)
                self._wide[id(self.aux[1 + k][j])] = ops.Conv2d(wide, b, stride=st, padding=1, act=ACT_LEAKY, alpha=LEAK, device=self.device)
            self._wide_sd = {}
            for conv in self._dense_convs() + list(self._wide.values()):
                if self._p1(conv, True):
                    ops.ensure_split(conv.w)
            self._p1_ready = True

    def _dense_convs(self):
        """Every ``ops.Conv2d`` of the generator."""
        out = [self.conv1, self.exit0, self.exit2]
        for blks in self.layers:
            for blk in blks:
                out += [blk["c1"], blk["c3"]] + ([blk["ds"]] if "ds" in blk else [])
        for c0, c1 in self.aux:
            out += [c0, c1]
        for _name, _width, head, blks, tail in self.tunnels:
            out += [head] + tail.convs
            for blk in blks:
                out += [blk["r"], blk["e"]]
        return out

    @staticmethod
    def _p1(conv: ops.Conv2d, bf16: bool) -> int:
        """``nprod`` of a dense convolution: 1 in the bf16 precision where ``one_product`` says so, else 0."""
        return 1 if bf16 and one_product(conv.Cin_raw, conv.kh, conv.kw, conv.Cout) else 0

    # -- squeeze-and-excitation --------------------------------------------------------------------------------------------------
    def se(self, se: _SE, t: torch.Tensor, res: torch.Tensor, out: torch.Tensor, act: int):
        """out = act(t * SE(t) + res); t dense [B,h,w,C], res / out NHWC views (may alias)."""
        B, h, w, Cc = t.shape
        lib = _lib.load()
        nbytes = int(lib.mit_se_squeeze_ws(B, h * w, Cc))
        ws = self._buf("se_ws", (nbytes + 7) // 8, dtype=torch.float64)
        _lib.check(lib.mit_se_squeeze(t.data_ptr(), t.stride(0), t.stride(2), B, h * w, Cc, ws.data_ptr(), ws.numel() * 8, _st()), "mit_se_squeeze")
        s = self._buf("se_s", B, Cc)
        _lib.check(lib.mit_se_excite(ws.data_ptr(), B, h * w, Cc, se.w1.data_ptr(), se.b1.data_ptr(), se.w2.data_ptr(), se.b2.data_ptr(),
                                     s.data_ptr(), _st()), "mit_se_excite")
        _lib.check(lib.mit_se_apply(t.data_ptr(), t.stride(0), t.stride(2), s.data_ptr(), res.data_ptr(), res.stride(0), res.stride(2),
                                    out.data_ptr(), out.stride(0), out.stride(2), B, h * w, Cc, act, _st()), "mit_se_apply")

    # -- FFDNet ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def denoise(self, page: torch.Tensor, sigma: float, bgr: bool = False, precision: Optional[str] = None, taps: Optional[dict] = None):
        """get_denoised_image (denoiser.py:51-118) of u8 RGB(A) pages [B,H,W,3|4] -> the B plane u8 [B,h,w] of the BGR result
        (with ``bgr``: also the whole BGR page [B,h,w,3]).  Pages whose long side exceeds 1200 are first INTER_AREA-resized to it.
        ``precision``: "fp32" | "bf16"; None = the engine's.  ``taps``: a copy of the noise estimate [B,h2,w2,12] as 'ffd_noise'."""
        precision = self.precision if precision is None else _check_precision(precision, "Mc2Engine.denoise")
        if self.ffd is None:
            raise RuntimeError("Mc2Engine: no denoiser weights")
        if page.dtype != torch.uint8 or page.dim() != 4 or page.shape[-1] not in (3, 4):
            raise ValueError(f"denoise expects u8 [B,H,W,3|4], got {page.dtype} {tuple(page.shape)}")
        B, H, W, Cin = page.shape
        img = page.contiguous()
        if max(H, W) > FFD_CAP:
            r = max(H, W) / FFD_CAP
            img = imgproc.resize_u8(page[..., :3].contiguous(), (int(W / r), int(H / r)), area=True)
            B, H, W, Cin = img.shape
        lib = _lib.load()
        h2, w2 = (H + 1) // 2, (W + 1) // 2
        pmax = self._buf("ffd_max", B, dtype=torch.int32)
        x = self._buf("ffd_in", B, h2, w2, 16)
        _lib.check(lib.mit_mc2_ffd_pack(img.data_ptr(), B, H, W, Cin, float(np.float32(sigma / 255)), pmax.data_ptr(), x.data_ptr(), _st()),
                   "mit_mc2_ffd_pack")
        if precision == "bf16":
            a = self._ffd_bf16(x)
        else:
            a, b = self._buf("ffd_a", B, h2, w2, S.FFD_FEATURES), self._buf("ffd_b", B, h2, w2, S.FFD_FEATURES)
            self.ffd[0](x, out=a)
            for conv in self.ffd[1:-1]:
                conv(a, out=b)
                a, b = b, a
        noise = self._buf("ffd_noise", B, h2, w2, 12)
        self.ffd[-1](a, out=noise)
        if taps is not None:
            taps["ffd_noise"] = noise.clone()
        plane = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        full = torch.empty(B, H, W, 3, dtype=torch.uint8, device=self.device) if bgr else None
        _lib.check(lib.mit_mc2_ffd_unpack(img.data_ptr(), B, H, W, Cin, pmax.data_ptr(), noise.data_ptr(), 12, plane.data_ptr(),
                                          None if full is None else full.data_ptr(), _st()), "mit_mc2_ffd_unpack")
        return (plane, full) if bgr else plane

    def _ffd_bf16(self, x: torch.Tensor) -> torch.Tensor:
        """Layers 0 .. 10 of FFDNet on bf16-resident activations: x [B,h2,w2,16] fp32 -> the last hidden tensor [B,h2,w2,96] fp32."""
        self._ensure_bf16()
        B, h2, w2, _ = x.shape
        x16 = self._buf("ffd_in16", B, h2, w2, FFD_CIN_BF16, dtype=torch.bfloat16)
        x16.zero_()
        ops.cast_bf16(x, x16[..., :16])
        a = self._buf("ffd_a16", B, h2, w2, S.FFD_FEATURES, dtype=torch.bfloat16)
        b = self._buf("ffd_b16", B, h2, w2, S.FFD_FEATURES, dtype=torch.bfloat16)
        last = self._buf("ffd_a", B, h2, w2, S.FFD_FEATURES)
        self.ffd16[0](x16, out_bf16=a)
        for conv in self.ffd16[1:-1]:
            conv(a, out_bf16=b)
            a, b = b, a
        self.ffd16[-1](a, out_f32=last)
        return last

    # -- generator ---------------------------------------------------------------------------------------------------------------
    def _encoder_layer(self, blks, x, Y, bf16=False):
        """One SE-ResNeXt layer from x into Y (both NHWC views); Y is the layer's residual stream."""
        for i, blk in enumerate(blks):
            src = x if i == 0 else Y
            B, H, W, _ = src.shape
            t1 = self._buf("e_t1", B, H, W, blk["mid"])
            blk["c1"](src, out=t1, nprod=self._p1(blk["c1"], bf16))
            Ho, Wo = Y.shape[1:3]
            t2 = self._buf("e_t2", B, Ho, Wo, blk["mid"])
            blk["c2"](t1, t2)
            t3 = self._buf("e_t3", B, Ho, Wo, blk["out"])
            blk["c3"](t2, out=t3, nprod=self._p1(blk["c3"], bf16))
            if "ds" in blk:
                blk["ds"](src, out=Y, nprod=self._p1(blk["ds"], bf16))
            self.se(blk["se"], t3, Y, Y, ACT_RELU)

    def _tunnel_blocks(self, blks, X, bf16=False):
        B, h, w, Cc = X.shape
        for blk in blks:
            t1 = self._buf("t_t1", B, h, w, Cc // 2)
            blk["r"](X, out=t1, nprod=self._p1(blk["r"], bf16))
            t2 = self._buf("t_t2", B, h, w, Cc // 2)
            blk["g"](t1, t2)
            t3 = self._buf("t_t3", B, h, w, Cc)
            blk["e"](t2, out=t3, nprod=self._p1(blk["e"], bf16))
            self.se(blk["se"], t3, X, X, ACT_NONE)

    @torch.no_grad()
    def colorize(self, plane: torch.Tensor, taps: Optional[dict] = None, precision: Optional[str] = None) -> torch.Tensor:
        """resize_pad's padding + ToTensor + Generator + the output glue of _infer (:54-74) for u8 planes [B,h,w] (already
        resized: one side of size, the other its scaled length) -> u8 RGB [B,h,w,3].  ``taps``: NHWC copies of x1..x4,
        tunnel4 / 3 / 2 and 'pre' (before the tanh).  ``precision``: "fp32" | "bf16"; None = the engine's."""
        precision = self.precision if precision is None else _check_precision(precision, "Mc2Engine.colorize")
        bf16 = precision == "bf16"
        if bf16:
            self._ensure_bf16()
        p1 = self._p1
        if plane.dtype != torch.uint8 or plane.dim() != 3:
            raise ValueError(f"colorize expects a u8 plane [B,h,w], got {plane.dtype} {tuple(plane.shape)}")
        B, h, w = plane.shape
        if h >= w:   # resize_pad pads the long side with 32 - side % 32 (32 when already divisible)
            Hp, Wp = h + 32 - h % 32, w
        else:
            Hp, Wp = h, w + 32 - w % 32
        if Hp % 8 or Wp % 8:
            raise ValueError(f"colorize: the unpadded side must be a multiple of 8 (got {h} x {w})")
        plane = plane.contiguous()
        lib = _lib.load()
        x = self._buf("g_in", B, Hp, Wp, 4)
        _lib.check(lib.mit_mc2_gen_in(plane.data_ptr(), B, h, w, x.data_ptr(), Hp, Wp, _st()), "mit_mc2_gen_in")
        H2, W2, H4, W4, H8, W8 = Hp // 2, Wp // 2, Hp // 4, Wp // 4, Hp // 8, Wp // 8
        E = self._buf("cat_exit", B, Hp, Wp, 96)            # (tunnel2 out 64 | x0 32)
        T2 = self._buf("cat_t2", B, H2, W2, 448)            # (tunnel3 out 128 | x2 256 | x1 64)
        T3 = self._buf("cat_t3", B, H4, W4, 768)            # (tunnel4 out 256 | x3 512)
        T4 = self._buf("cat_t4", B, H8, W8, 1152)           # (x4 1024 | aux 128)
        # aux path
        a = self._buf("aux0", B, Hp, Wp, 32)
        self.aux[0][0](x, out=a, nprod=p1(self.aux[0][0], bf16))
        self.aux[0][1](a, out=E[..., 64:96], nprod=p1(self.aux[0][1], bf16))
        cur = E[..., 64:96]
        wide = (lambda conv: self._wide.get(id(conv), conv)) if bf16 else (lambda conv: conv)

        def padded(name, hh, ww, cout, cin):
            """A [B,hh,ww,cout] buffer; with cin > cout (its reader takes zero channels up to cin) the view of a wider one, pad zeroed."""
            if cin == cout:
                return self._buf(name, B, hh, ww, cout)
            full = self._buf(name + "_w", B, hh, ww, cin)
            full[..., cout:].zero_()
            return full

        for k, (c0, c1) in enumerate(self.aux[1:]):
            hh, ww = c0.out_hw(cur.shape[1], cur.shape[2])
            c0, c1 = wide(c0), wide(c1)
            nxt = wide(self.aux[k + 2][0]) if k < 2 else None
            t = padded("aux_a", hh, ww, c0.Cout, c1.Cin)
            c0(cur, out=t[..., :c0.Cout], nprod=p1(c0, bf16))
            o = T4[..., 1024:1152] if k == 2 else padded(f"aux_b{k}", hh, ww, c1.Cout, nxt.Cin)
            c1(t, out=o[..., :c1.Cout], nprod=p1(c1, bf16))
            cur = o
        # encoder
        x1 = T2[..., 384:448]
        self.conv1(x, out=x1, nprod=p1(self.conv1, bf16))
        self._encoder_layer(self.layers[0], x1, T2[..., 128:384], bf16)
        self._encoder_layer(self.layers[1], T2[..., 128:384], T3[..., 256:768], bf16)
        self._encoder_layer(self.layers[2], T3[..., 256:768], T4[..., 0:1024], bf16)
        if taps is not None:
            taps.update(x1=x1.clone(), x2=T2[..., 128:384].clone(), x3=T3[..., 256:768].clone(), x4=T4[..., 0:1024].clone())
        # tunnels
        for (name, width, head, blks, tail), src, dst in zip(self.tunnels, (T4, T3, T2), (T3[..., 0:256], T2[..., 0:128], E[..., 0:64])):
            X = self._buf("tun_" + name, B, src.shape[1], src.shape[2], width)
            head(src, out=X, nprod=p1(head, bf16))
            self._tunnel_blocks(blks, X, bf16)
            tail(X, dst, nprod=p1(tail.convs[0], bf16))
            if taps is not None:
                taps[name] = dst.clone()
        t = self._buf("exit_t", B, Hp, Wp, 32)
        self.exit0(E, out=t, nprod=p1(self.exit0, bf16))
        pre = self._buf("exit_pre", B, Hp, Wp, 4)
        self.exit2(t, out=pre[..., :3], nprod=p1(self.exit2, bf16))
        if taps is not None:
            taps["pre"] = pre[..., :3].clone()
        out = torch.empty(B, h, w, 3, dtype=torch.uint8, device=self.device)
        _lib.check(lib.mit_mc2_post(pre.data_ptr(), 4, B, Hp, Wp, out.data_ptr(), h, w, _st()), "mit_mc2_post")
        return out

    # -- the whole _infer --------------------------------------------------------------------------------------------------------
    @staticmethod
    def plan(H: int, W: int, colorization_size: int, denoise_sigma: float):
        """(size, denoiser input (h, w) or None, plane (h, w)) of _infer (:44-56) for an H x W page."""
        m = min(H, W)
        m -= m % 32
        size = min(m, colorization_size - colorization_size % 32) if colorization_size > 0 else min(m, 576)
        if size <= 0:
            raise ValueError(f"mc2: page {H} x {W} is smaller than 32 pixels on its short side")
        dn = None
        h, w = H, W
        if 0 <= denoise_sigma <= 255:
            if max(H, W) > FFD_CAP:
                r = max(H, W) / FFD_CAP
                h, w = int(H / r), int(W / r)
            dn = (h, w)
        if h < w:
            ratio = h / (size * 1.5)
            ph, pw = int(size * 1.5), int(np.ceil(w / ratio))
        else:
            ratio = w / size
            ph, pw = int(np.ceil(h / ratio)), size
        return size, dn, (ph, pw)

    @torch.no_grad()
    def forward(self, page: torch.Tensor, colorization_size: int, denoise_sigma: float = 25, taps: Optional[dict] = None,
                precision: Optional[str] = None) -> torch.Tensor:
        """_infer (:42-74) for B u8 RGB(A) pages [B,H,W,3|4] of one size -> u8 RGB [B,h,w,3] at the network's size.
        ``precision``: "fp32" | "bf16"; None = the engine's.  A page's bytes in either precision do not depend on the pages that
        travel with it."""
        precision = self.precision if precision is None else _check_precision(precision, "Mc2Engine.forward")
        if page.dtype != torch.uint8 or page.dim() != 4 or page.shape[-1] not in (3, 4):
            raise ValueError(f"forward expects u8 [B,H,W,3|4], got {page.dtype} {tuple(page.shape)}")
        B, H, W, _ = page.shape
        _size, dn, (ph, pw) = self.plan(H, W, colorization_size, denoise_sigma)
        if dn is not None:
            src = self.denoise(page, denoise_sigma, precision=precision)   # B of the BGR page
        else:
            src = page[..., 0].contiguous()                         # R of the page
        if tuple(src.shape[1:]) != (ph, pw):
            src = imgproc.resize_u8(src, (pw, ph), area=True)
        if taps is not None:
            taps["plane"] = src.clone()
        return self.colorize(src, taps, precision=precision)

    @staticmethod
    def flops_per_page(H: int, W: int) -> float:
        """Algorithmic FLOPs (2 x MACs) of the generator's used layers at a padded input H x W."""
        px = H * W
        res = {0: px / 4, 1: px / 4, 2: px / 16, 3: px / 64}
        f = 2.0 * (px / 4) * 49 * 1 * 64
        inplanes = 64
        for layer, planes, blocks, _stride in S.ENCODER:
            for i in range(blocks):
                s_out = res[layer]
                s_in = res[layer - 1] if i == 0 else s_out
                mid, out = 2 * planes, 4 * planes
                f += 2.0 * (s_in * inplanes * mid + s_out * 9 * mid * (mid // S.CARDINALITY) + s_out * mid * out)
                if i == 0:
                    f += 2.0 * s_out * inplanes * out
                inplanes = out
        f += 2.0 * 9 * (px * (32 + 32 * 32) + (px / 4) * (32 * 64 + 64 * 64) + (px / 16) * (64 * 92 + 92 * 92)
                        + (px / 64) * (92 * 128 + 128 * 128))
        for (_name, cin, width, dils, card), s in zip(S.TUNNELS[:3], (px / 64, px / 16, px / 4)):
            D = width // 2
            f += 2.0 * s * 9 * (cin * width + width * 2 * width)
            f += len(dils) * 2.0 * s * (width * D + 9 * D * (D // card) + D * width)
        return f + 2.0 * px * (9 * 96 * 32 + 32 * 3)

    @staticmethod
    def ffd_flops(H: int, W: int) -> float:
        """Algorithmic FLOPs of FFDNet on an H x W page (after the 1200 cap)."""
        px = ((H + 1) // 2) * ((W + 1) // 2)
        return 2.0 * px * 9 * (15 * 96 + (S.FFD_LAYERS - 2) * 96 * 96 + 96 * 12)
