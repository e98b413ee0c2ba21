"""``--detector dbconvnext`` network (DBNet on ConvNeXt) on the gfx950 engine.

Same graph as ``DBNetConvNext.forward`` (manga_translator/detection/dbnet_convnext.py:474-491 of the reference) + ``DBHead`` (:382-408)
+ the tensor part of ``det_batch_forward_default`` (:499-509), which is the ``default`` detector's, second sigmoid on the threshold plane
included.

Layout: fp32 NHWC; each U-Net concat ``cat([up, skip])`` is a pre-allocated buffer whose two channel slices are written by the
producing layers.  A ConvNeXt block is three launches: depthwise 7x7 + LayerNorm (``mit_dwconv7_ln_nhwc``, measured 3x faster than
``mit_dwconv_nhwc`` then ``mit_layernorm_rows`` at every backbone width, profiles/r23a_dbconvnext.json), fc1 as a 1x1 convolution with the GELU in its epilogue, fc2 as
a 1x1 convolution whose epilogue scales by ``gamma`` and adds the block input.  The up-blocks' 7x7 is dense (out_chs < in_chs, :100) and
runs on the implicit GEMM; their 1x1 shortcut enters fc2's epilogue the same way.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import lib as _lib
from . import ops
from .dbconvnext_schema import DEPTHS, DIMS, LN_EPS, UPCONVS
from .ops import ACT_GELU, ACT_SIGMOID, ACT_SILU


def _f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous().to(dev)


class _Norm:
    """LayerNorm over the channels of NHWC pixels (timm LayerNorm / LayerNorm2d, eps 1e-6)."""

    def __init__(self, sd, p, dev):
        self.w, self.b = _f32(sd[p + ".weight"], dev), _f32(sd[p + ".bias"], dev)
        self.C = self.w.numel()

    def __call__(self, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        B, H, W, Cx = x.shape
        if Cx != self.C or tuple(out.shape) != tuple(x.shape) or not (_pixel_uniform(x) and _pixel_uniform(out)):
            raise ValueError(f"LayerNorm({self.C}): bad operands {tuple(x.shape)} -> {tuple(out.shape)}")
        _lib.check(_lib.load().mit_layernorm_rows(x.data_ptr(), x.stride(2), self.w.data_ptr(), self.b.data_ptr(), out.data_ptr(), out.stride(2),
                                                  B * H * W, self.C, LN_EPS, C.c_void_p(ops.current_stream())), "mit_layernorm_rows")
        return out


def _pixel_uniform(t: torch.Tensor) -> bool:
    """Pixel p = (b H + y) W + x of the NHWC view lies at p * stride(2): a dense tensor or a channel slice of one."""
    B, H, W, _ = t.shape
    return t.stride(3) == 1 and t.stride(1) == W * t.stride(2) and t.stride(0) == H * t.stride(1)


class _Mlp:
    """timm Mlp (fc1 -> GELU -> fc2) on pixels, layer scale and residual in fc2's epilogue (:121-126)."""

    def __init__(self, sd, p, dev):
        self.fc1 = ops.Conv2d(sd[p + ".mlp.fc1.weight"][:, :, None, None], sd[p + ".mlp.fc1.bias"], act=ACT_GELU, device=dev)
        self.fc2 = ops.Conv2d(sd[p + ".mlp.fc2.weight"][:, :, None, None], sd[p + ".mlp.fc2.bias"], out_scale=sd[p + ".gamma"], device=dev)


class _Block:
    """ConvNeXtBlock with in_chs == out_chs (:42-127): depthwise 7x7, identity shortcut."""

    def __init__(self, sd, p, dev):
        w = sd[p + ".conv_dw.weight"]                          # [C, 1, 7, 7]
        self.C = w.shape[0]
        self.dw_w = _f32(w.reshape(self.C, 49).t(), dev)       # [49][C]
        self.dw_b = _f32(sd[p + ".conv_dw.bias"], dev)
        self.norm = _Norm(sd, p + ".norm", dev)
        self.mlp = _Mlp(sd, p, dev)


class _UpBlock:
    """UpconvSkip (:359-380): a ConvNeXtBlock with out_chs < in_chs — dense 7x7, 1x1 shortcut — and ConvTranspose2d k2 s2."""

    def __init__(self, sd, p, dev):
        q = p + ".conv"
        self.dw = ops.Conv2d(sd[q + ".conv_dw.weight"], sd[q + ".conv_dw.bias"], padding=3, device=dev)
        self.norm = _Norm(sd, q + ".norm", dev)
        self.mlp = _Mlp(sd, q, dev)
        self.shortcut = ops.Conv2d(sd[q + ".shortcut.conv.weight"], sd.get(q + ".shortcut.conv.bias"), device=dev)
        self.up = ops.ConvTranspose2d(sd[p + ".upconv.weight"], sd[p + ".upconv.bias"], stride=2, device=dev)
        self.Cout = self.dw.Cout


class _Stage:
    """ConvNeXtStage (:130-193): LayerNorm2d + 2x2 stride-2 convolution (none in the backbone's stage 0), then the blocks."""

    def __init__(self, sd, p, depth, downsample, dev):
        self.norm = self.down = None
        if downsample:
            self.norm = _Norm(sd, p + ".downsample.0", dev)
            self.down = ops.Conv2d(sd[p + ".downsample.1.weight"], sd[p + ".downsample.1.bias"], stride=2, device=dev)
        self.blocks = [_Block(sd, f"{p}.blocks.{j}", dev) for j in range(depth)]
        self.C = self.blocks[0].C


def check_page_batch(img_u8: torch.Tensor) -> None:
    """What ``DbconvnextEngine.forward`` accepts: u8 [B, H, W, 3] with H and W multiples of 128 (h128 is H / 128 x W / 128 and every
    2x2 stride-2 convolution on the way down needs even sides)."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[-1] != 3:
        raise ValueError(f"DbconvnextEngine.forward expects u8 [B,H,W,3], got {img_u8.dtype} {tuple(img_u8.shape)}")
    _, H, W, _ = img_u8.shape
    if H <= 0 or W <= 0 or H % 128 or W % 128:
        raise ValueError(f"DbconvnextEngine.forward: H and W must be multiples of 128 (got {H} x {W})")


class DbconvnextEngine(ops.Engine):
    """Batched dbconvnext network: u8 pages (H, W multiples of 128) -> (db [B,2,H,W] after sigmoid, mask [B,H/2,W/2])."""

    def __init__(self, sd: Dict[str, torch.Tensor], device="cuda"):
        super().__init__(device)
        dev = self.device
        self.stem = ops.Conv2d(sd["backbone.stem.0.weight"], sd["backbone.stem.0.bias"], stride=4, device=dev)
        self.stem_norm = _Norm(sd, "backbone.stem.1", dev)
        self.stages = [_Stage(sd, f"backbone.stages.{i}", DEPTHS[i], i > 0, dev) for i in range(4)]
        self.stages += [_Stage(sd, f"down_conv{j}", 2, True, dev) for j in (1, 2)]
        self.ups = [_UpBlock(sd, name, dev) for name, *_ in UPCONVS]
        missing = [c for c in DIMS if not _lib.load().mit_dwconv7_ln_supported(c)]
        if missing:   # every backbone width is measured faster in the one-pass form (profiles/r23a_dbconvnext.json); no second path is kept
            raise RuntimeError(f"DbconvnextEngine: libmit_hip.so has no one-pass depthwise + LayerNorm kernel for C = {missing}")

        def branch(q, first_bias):
            c0 = ops.Conv2d(sd[q + ".0.weight"], sd[q + ".0.bias"] if first_bias else None, padding=1, act=ACT_SILU, device=dev)
            t1 = ops.ConvTranspose2d(sd[q + ".2.weight"], sd[q + ".2.bias"], stride=2, padding=1, act=ACT_SILU, device=dev)
            t2 = ops.ConvTranspose2d(sd[q + ".4.weight"], sd[q + ".4.bias"], stride=2, padding=1, act=ACT_SIGMOID, device=dev)
            return c0, t1, t2
        # det_batch_forward_default applies sigmoid to BOTH planes (:507): logits -> sigmoid; the threshold map, which DBHead already
        # passed through a sigmoid (:430), gets a second one (done in place after its own), as in dbnet.py
        self.binarize = branch("conv_db.binarize", True)
        self.thresh = branch("conv_db.thresh", False)
        self.mask_convs = [ops.Conv2d(sd[f"conv_mask.{i}.weight"], sd[f"conv_mask.{i}.bias"], padding=1, act=ACT_SILU, device=dev) for i in (0, 2)]
        self.mask_out = ops.Conv2d(sd["conv_mask.4.weight"], sd["conv_mask.4.bias"], act=ACT_SIGMOID, device=dev)

    def _dwln(self, blk: _Block, x, t, lib, st):
        """t = LayerNorm(dwconv7(x) + b) in one launch."""
        B, H, W, Cc = x.shape
        _lib.check(lib.mit_dwconv7_ln_nhwc(x.data_ptr(), x.stride(2), blk.dw_w.data_ptr(), blk.dw_b.data_ptr(), blk.norm.w.data_ptr(),
                                           blk.norm.b.data_ptr(), LN_EPS, t.data_ptr(), t.stride(2), B, H, W, Cc, st), "mit_dwconv7_ln_nhwc")
        return t

    def _block(self, blk: _Block, x, out, tag, lib, st):
        """out = x + gamma * fc2(gelu(fc1(LayerNorm(dwconv7(x)))))"""
        B, H, W, Cc = x.shape
        t = self._dwln(blk, x, self._buf(tag + ".t", B, H, W, Cc), lib, st)
        h = self._buf(tag + ".h", B, H, W, 4 * Cc)
        blk.mlp.fc1(t, out=h)
        return blk.mlp.fc2(h, out=out, post=x)

    def _stage(self, stg: _Stage, x, out, tag, lib, st):
        """One ConvNeXtStage from ``x`` into ``out`` (a dense buffer or the skip slice of a concat buffer)."""
        B, H, W, Cin = x.shape
        if stg.down is not None:
            n = self._buf(tag + ".n", B, H, W, Cin)
            stg.norm(x, n)
            H, W = H // 2, W // 2
            x = stg.down(n, out=self._buf(tag + ".x2", B, H, W, stg.C))
        for j, blk in enumerate(stg.blocks):
            last = j == len(stg.blocks) - 1
            x = self._block(blk, x, out if last else self._buf(f"{tag}.x{j & 1}", B, H, W, stg.C), tag, lib, st)
        return x

    def _up(self, ub: _UpBlock, x, out, tag):
        """UpconvSkip from ``x`` (a whole concat buffer) into ``out`` (the `up` slice of the next one, twice the size)."""
        B, H, W, _ = x.shape
        d = self._buf(tag + ".d", B, H, W, ub.Cout)
        ub.dw(x, out=d)
        t = self._buf(tag + ".t", B, H, W, ub.Cout)
        ub.norm(d, t)
        h = self._buf(tag + ".h", B, H, W, 4 * ub.Cout)
        ub.mlp.fc1(t, out=h)
        sc = self._buf(tag + ".sc", B, H, W, ub.Cout)
        ub.shortcut(x, out=sc)
        ub.mlp.fc2(h, out=d, post=sc)   # d has been consumed by the norm
        return ub.up(d, out=out)

    @torch.no_grad()
    def forward(self, img_u8: torch.Tensor, taps: Optional[dict] = None):
        check_page_batch(img_u8)
        B, H, W, _ = img_u8.shape
        img_u8 = img_u8.contiguous()
        lib = _lib.load()
        st = C.c_void_p(ops.current_stream())
        x = self._buf("in4", B, H, W, 4)
        _lib.check(lib.mit_u8_to_f32_nhwc4(img_u8.data_ptr(), x.data_ptr(), B * H * W, 1, st), "mit_u8_to_f32_nhwc4")
        h, w = H // 4, W // 4
        s0 = self._buf("stem", B, h, w, DIMS[0])
        self.stem(x, out=s0)
        s1 = self._buf("stem.n", B, h, w, DIMS[0])
        self.stem_norm(s0, s1)
        # concat buffers [up | skip] of the decoder (:485-489); the backbone and the two downs write their skips into them
        cat4 = self._buf("cat4", B, h, w, 256)                    # [up8 128 | h4 128]
        cat8 = self._buf("cat8", B, h // 2, w // 2, 384)          # [up16 128 | h8 256]
        cat16 = self._buf("cat16", B, h // 4, w // 4, 640)        # [up32 128 | h16 512]
        cat32 = self._buf("cat32", B, h // 8, w // 8, 1152)       # [up64 128 | h32 1024]
        cat64 = self._buf("cat64", B, h // 16, w // 16, 1152)     # [up128 128 | h64 1024]
        h128 = self._buf("h128", B, h // 32, w // 32, 1024)
        outs = [cat4[..., 128:], cat8[..., 128:], cat16[..., 128:], cat32[..., 128:], cat64[..., 128:], h128]
        cur = s1
        for i, stg in enumerate(self.stages):
            cur = self._stage(stg, cur, outs[i], f"s{i}", lib, st)
        h4, h32 = outs[0], outs[3]
        up4 = self._buf("up4", B, 2 * h, 2 * w, 64)
        srcs = [h128, cat64, cat32, cat16, cat8, cat4]
        dsts = [cat64[..., :128], cat32[..., :128], cat16[..., :128], cat8[..., :128], cat4[..., :128], up4]
        for i, ub in enumerate(self.ups):
            self._up(ub, srcs[i], dsts[i], f"u{i}")
        up8 = cat4[..., :128]
        # DBHead on up8 (1/4 resolution) -> full-resolution planes (:400-408) + db.sigmoid() (:507)
        db = self._buf("db", B, 2, H, W)
        for plane, (c0, t1, t2) in ((0, self.binarize), (1, self.thresh)):
            b0 = self._buf("db.b0", B, h, w, 32)
            c0(up8, out=b0)
            b1 = self._buf("db.b1", B, 2 * h, 2 * w, 32)
            t1(b0, out=b1)
            t2(b1, out=db[:, plane].unsqueeze(-1))
        for b in range(B):  # the second sigmoid on the (already sigmoided) threshold plane
            _lib.check(lib.mit_sigmoid_inplace(db[b, 1].data_ptr(), H * W, st), "mit_sigmoid_inplace")
        # conv_mask on up4 (1/2 resolution) (:455-460)
        m = up4
        for i, conv in enumerate(self.mask_convs):
            m = conv(m, out=self._buf(f"mask{i}", B, 2 * h, 2 * w, conv.Cout))
        mask = self._buf("mask", B, 2 * h, 2 * w, 1)
        self.mask_out(m, out=mask)
        if taps is not None:
            taps.update(h4=h4.clone(), h32=h32.clone(), h128=h128.clone(), up8=up8.clone(), up4=up4.clone())
        return db, mask[..., 0]
