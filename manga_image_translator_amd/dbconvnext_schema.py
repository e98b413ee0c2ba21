"""State-dict layout of the reference ``dbconvnext`` detector (``dbnet_convnext.ckpt`` = ``DBNetConvNext``).

manga_translator/detection/dbnet_convnext.py:450-472 of the reference: a ConvNeXt backbone with depths (3, 3, 27, 3) and dims
(128, 256, 512, 1024) (:196-319), two further 1024-wide ``ConvNeXtStage`` downs, six ``UpconvSkip`` blocks (:359-380), ``DBHead(128)``
(:382-445) and ``conv_mask``.  timm is not installed anywhere we can run, so the names its layers give their tensors
(``LayerNorm`` / ``LayerNorm2d``: weight, bias; ``Mlp``: fc1, fc2; ``create_conv2d``: a plain ``nn.Conv2d``) are restated from its
documented layout; the reference module's own names are pinned by a strict ``load_state_dict`` (tests/test_dbconvnext_cpu.py).
Entries are in the module's ``state_dict()`` order (a module's own parameters — ``gamma`` — before its children's).
"""
from __future__ import annotations

from .synth import Schema

DEPTHS = (3, 3, 27, 3)
DIMS = (128, 256, 512, 1024)
# (name, channels of the `up` slice, channels of the skip, out channels) of the six UpconvSkip blocks (:465-470)
UPCONVS = (("upconv1", 0, 1024, 128), ("upconv2", 128, 1024, 128), ("upconv3", 128, 1024, 128), ("upconv4", 128, 512, 128),
           ("upconv5", 128, 256, 128), ("upconv6", 128, 128, 64))
LN_EPS = 1e-6  # timm's LayerNorm / LayerNorm2d default
# Layer scale of the seeded weights: uniform in (0.1, 0.5) times this (a trained backbone starts from 1e-6, the other blocks from 1.0;
# seeded weights need every block to contribute without the 40-block trunk growing out of range, tests/_dbconvnext_oracle.py)
GAMMA = "gamma*1.0"


def _ln(p: str, c: int) -> Schema:
    return [(p + ".weight", (c,), "ln_w"), (p + ".bias", (c,), "bn_b")]


def _block(p: str, cin: int, cout: int) -> Schema:
    """ConvNeXtBlock (:42-127).  ``conv_dw`` is depthwise when out_chs >= in_chs, else a dense 7x7 (:100); a block that changes the
    channel count carries a 1x1 ``shortcut.conv`` (Downsample at stride 1, :25-35)."""
    s: Schema = [(p + ".gamma", (cout,), GAMMA),
                 (p + ".conv_dw.weight", (cout, 1 if cout >= cin else cin, 7, 7), "conv"), (p + ".conv_dw.bias", (cout,), "bias")]
    s += _ln(p + ".norm", cout)
    s += [(p + ".mlp.fc1.weight", (4 * cout, cout), "linear"), (p + ".mlp.fc1.bias", (4 * cout,), "bias"),
          (p + ".mlp.fc2.weight", (cout, 4 * cout), "linear"), (p + ".mlp.fc2.bias", (cout,), "bias")]
    if cin != cout:
        s += [(p + ".shortcut.conv.weight", (cout, cin, 1, 1), "conv"), (p + ".shortcut.conv.bias", (cout,), "bias")]
    return s


def _stage(p: str, cin: int, cout: int, depth: int, downsample: bool) -> Schema:
    """ConvNeXtStage (:130-193): LayerNorm2d + 2x2 stride-2 conv (absent in the backbone's stage 0), then ``depth`` blocks."""
    s: Schema = []
    if downsample:
        s += _ln(p + ".downsample.0", cin) + [(p + ".downsample.1.weight", (cout, cin, 2, 2), "conv"), (p + ".downsample.1.bias", (cout,), "bias")]
    for j in range(depth):
        s += _block(f"{p}.blocks.{j}", cout, cout)
    return s


def dbnet_convnext_schema() -> Schema:
    s: Schema = [("backbone.stem.0.weight", (DIMS[0], 3, 4, 4), "conv"), ("backbone.stem.0.bias", (DIMS[0],), "bias")] + _ln("backbone.stem.1", DIMS[0])
    prev = DIMS[0]
    for i, (depth, dim) in enumerate(zip(DEPTHS, DIMS)):
        s += _stage(f"backbone.stages.{i}", prev, dim, depth, downsample=i > 0)
        prev = dim
    s += [("conv_mask.0.weight", (64, 64, 3, 3), "conv"), ("conv_mask.0.bias", (64,), "bias"),
          ("conv_mask.2.weight", (32, 64, 3, 3), "conv"), ("conv_mask.2.bias", (32,), "bias"),
          ("conv_mask.4.weight", (1, 32, 1, 1), "conv*4.0"), ("conv_mask.4.bias", (1,), "bias")]
    for j in (1, 2):
        s += _stage(f"down_conv{j}", 1024, 1024, 2, downsample=True)
    for name, up, skip, out in UPCONVS:
        s += _block(name + ".conv", up + skip, out)
        s += [(name + ".upconv.weight", (out, out, 2, 2), "convT"), (name + ".upconv.bias", (out,), "bias")]
    # DBHead(128) (:382-445): binarize has biases throughout; thresh.0 is built with bias=False, its two ConvTranspose2d come from
    # _init_upsample (:433-445), which does not pass ``bias`` on, so they keep nn.ConvTranspose2d's default bias
    s += [("conv_db.binarize.0.weight", (32, 128, 3, 3), "conv"), ("conv_db.binarize.0.bias", (32,), "bias"),
          ("conv_db.binarize.2.weight", (32, 32, 4, 4), "convT"), ("conv_db.binarize.2.bias", (32,), "bias"),
          ("conv_db.binarize.4.weight", (32, 1, 4, 4), "convT*3.0"), ("conv_db.binarize.4.bias", (1,), "bias"),
          ("conv_db.thresh.0.weight", (32, 128, 3, 3), "conv"),
          ("conv_db.thresh.2.weight", (32, 32, 4, 4), "convT"), ("conv_db.thresh.2.bias", (32,), "bias"),
          ("conv_db.thresh.4.weight", (32, 1, 4, 4), "convT*3.0"), ("conv_db.thresh.4.bias", (1,), "bias")]
    return s
