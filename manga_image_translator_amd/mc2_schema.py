"""State-dict layouts of the reference colorizer ``Colorizer.mc2`` (manga-colorization-v2): ``generator.zip`` = ``Generator()``
(manga_translator/colorization/manga_colorization_v2_utils/networks/models.py:209-300, encoder networks/extractor.py) and
``net_rgb.pth`` = ``FFDNet(3)`` (denoising/models.py).

Generator keys: the SE-ResNeXt encoder ``encoder.{conv1, bn1, layer1..3}`` (``BottleneckX_Origin`` blocks with ``conv1..3``,
``bn1..3``, ``selayer.conv{1,2}`` and, in block 0, ``downsample.{0,1}``), the aux path ``to0..to4``, the unused guide decoder
``deconv_for_decoder.{0,2,4,6}``, the tunnels ``tunnel{4,3,2,1}.{0,2.<i>,3}`` (``ResNeXtBottleneck``: ``conv_reduce``, grouped
``conv_conv``, ``conv_expand``, ``selayer``) and ``exit.{0,2}``.  ``to4``, ``tunnel1`` and ``deconv_for_decoder`` are built by the
reference but never reach its output; the schema lists them (a checkpoint carries them) and the engine never reads them.  FFDNet keys
keep the reference's own spelling ``intermediate_dncnn.itermediate_dncnn.<n>``.  tests/test_mc2_cpu.py pins both layouts against the
reference modules' ``state_dict()``.

The seeded weights are chosen so that a synthetic page really exercises the network: every residual branch is scaled down (the
encoder's ``bn3`` gain by 0.25, the tunnels' ``conv_expand`` by 0.3), so the 17 encoder and 36 tunnel blocks neither blow up nor
vanish, and ``exit.2`` is scaled so that the tanh output spreads over most of [-1, 1] without saturating (at least half of a page's
bytes lie in [16, 239]; the three channels differ).  FFDNet's last convolution is scaled by 0.5: a noise estimate of a few hundredths.
"""
from __future__ import annotations

from .synth import Schema, bn_entries

# encoder: (layer, planes, blocks, stride); BottleneckX_Origin(inplanes, planes, 32, stride): mid = 2 planes, out = 4 planes
ENCODER = ((1, 64, 3, 1), (2, 128, 4, 2), (3, 256, 6, 2))
CARDINALITY = 32
# tunnels: (name, cin of the head conv, width, dilations of the blocks, cardinality)
TUNNELS = (("tunnel4", 1024 + 128, 512, (1,) * 20, 32),
           ("tunnel3", 512 + 256, 256, (1, 1, 2, 2, 4, 4, 2, 1), 32),
           ("tunnel2", 128 + 256 + 64, 128, (1, 1, 2, 2, 4, 4, 2, 1), 32),
           ("tunnel1", 64 + 32, 64, (1, 2, 4, 2, 1), 16))
# aux path: (name, cin, cout, first conv stride)
AUX = (("to0", 5, 32, 1), ("to1", 32, 64, 2), ("to2", 64, 92, 2), ("to3", 92, 128, 2), ("to4", 128, 256, 2))
FFD_FEATURES, FFD_LAYERS = 96, 12


def _conv(name: str, cout: int, cin: int, k: int, bias: bool = True, kind: str = "conv") -> Schema:
    s: Schema = [(name + ".weight", (cout, cin, k, k), kind)]
    if bias:
        s.append((name + ".bias", (cout,), "bias"))
    return s


def _se(prefix: str, c: int) -> Schema:
    return _conv(prefix + ".conv1", c // 16, c, 1) + _conv(prefix + ".conv2", c, c // 16, 1)


def generator_schema() -> Schema:
    s: Schema = _conv("encoder.conv1", 64, 1, 7, bias=False) + bn_entries("encoder.bn1", 64)
    inplanes = 64
    for layer, planes, blocks, _stride in ENCODER:
        for i in range(blocks):
            p = f"encoder.layer{layer}.{i}"
            mid, out = 2 * planes, 4 * planes
            s += _conv(p + ".conv1", mid, inplanes, 1, bias=False) + bn_entries(p + ".bn1", mid)
            s += _conv(p + ".conv2", mid, mid // CARDINALITY, 3, bias=False) + bn_entries(p + ".bn2", mid)
            s += _conv(p + ".conv3", out, mid, 1, bias=False) + bn_entries(p + ".bn3", out, "*0.25")
            s += _se(p + ".selayer", out)
            if i == 0:
                s += _conv(p + ".downsample.0", out, inplanes, 1, bias=False) + bn_entries(p + ".downsample.1", out)
            inplanes = out
    for name, cin, cout, _st in AUX:
        s += _conv(name + ".0", cout, cin, 3) + _conv(name + ".2", cout, cout, 3)
    for i, (cin, cout) in enumerate(((256, 128), (128, 64), (64, 32), (32, 3))):
        s += [(f"deconv_for_decoder.{2 * i}.weight", (cin, cout, 3, 3), "convT"), (f"deconv_for_decoder.{2 * i}.bias", (cout,), "bias")]
    for name, cin, width, dils, card in TUNNELS:
        s += _conv(name + ".0", width, cin, 3)
        D = width // 2
        for i in range(len(dils)):
            p = f"{name}.2.{i}"
            s += _conv(p + ".conv_reduce", D, width, 1, bias=False)
            s += _conv(p + ".conv_conv", D, D // card, 3, bias=False)
            s += _conv(p + ".conv_expand", width, D, 1, bias=False, kind="conv*0.3")
            s += _se(p + ".selayer", width)
        s += _conv(name + ".3", 2 * width, width, 3)
    s += _conv("exit.0", 32, 64 + 32, 3) + _conv("exit.2", 3, 32, 1, kind="conv*2.0")
    return s


def ffdnet_schema() -> Schema:
    p = "intermediate_dncnn.itermediate_dncnn"
    s: Schema = _conv(f"{p}.0", FFD_FEATURES, 15, 3, bias=False)
    for k in range(FFD_LAYERS - 2):
        s += _conv(f"{p}.{2 + 3 * k}", FFD_FEATURES, FFD_FEATURES, 3, bias=False) + bn_entries(f"{p}.{3 + 3 * k}", FFD_FEATURES)
    s += _conv(f"{p}.{2 + 3 * (FFD_LAYERS - 2)}", 12, FFD_FEATURES, 3, bias=False, kind="conv*0.5")
    return s


def strip_dataparallel(sd):
    """net_rgb.pth as saved from nn.DataParallel carries a ``module.`` prefix on every key (denoising/utils.py:39-52)."""
    if sd and all(k.startswith("module.") for k in sd):
        return {k[len("module."):]: v for k, v in sd.items()}
    return sd
