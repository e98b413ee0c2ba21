"""The mc2 colorizer's bf16 precision, the parts that need no GPU: the argument checks of ``mit_conv3x3_bf16`` (before any HIP call:
fake pointers that are never dereferenced), its descriptor from strided views, the zero-padded layer-0 weight of FFDNet, how the
engine's and the plugin's ``precision`` resolve, which generator layers the bf16 precision runs with one product, and the yardstick's
own check.

The yardstick (tests/_mc2_bf16_cases.py): on the inputs of tests/test_mc2_bf16_gpu.py, an emulation in float64 that rounds the two
operands of every dense convolution with K >= 64 and N >= 16 to bf16 — what the engine's bf16 precision does, minus its fp32
accumulation — against the float64 truth, beside the same oracle under ``torch.autocast("cpu", bfloat16)``.  Measured here (error of
the emulation / error of autocast):
    FFDNet noise estimate, pages 0 and 1:   mean 0.55, 0.57    max 0.66, 0.48
    generator before the tanh, 64x48, 96x64: mean 0.54, 0.54    max 0.57, 0.52
The mean is below autocast's with a wide margin; the max stays below 0.8 of autocast's on every case, so the GPU test asserts the
max as well as the mean (an engine whose max came close to autocast's would not be this computation)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mc2_bf16_cases as K
import _mc2_oracle as O

FAKE = 1 << 20      # 16-byte aligned, never dereferenced: every call below is refused by the argument checks


def _desc(lib, **kw):
    """A descriptor the checks accept (a 96 -> 96 FFDNet layer between two [1, 16, 40, 96] buffers), then ``kw`` on top."""
    d = lib.MitConv3x3Bf16()
    d.B, d.H, d.W, d.Cin, d.N = 1, 16, 40, 96, 96
    d.in_bs, d.in_ys, d.in_xs = 16 * 40 * 96, 40 * 96, 96
    setattr(d, "in", FAKE)
    d.w = FAKE + (1 << 24)
    d.out_bf16 = FAKE + (1 << 26)
    d.ob_bs, d.ob_ys, d.ob_xs = d.in_bs, d.in_ys, d.in_xs
    d.act = lib.ACT_RELU
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, L, what, **kw):
    rc = L.mit_conv3x3_bf16(C.byref(_desc(lib, **kw)), None)
    msg = L.mit_last_error()
    assert rc != 0 and what in msg, (kw, rc, msg)


def test_conv3x3_bf16_refuses_bad_arguments_before_any_hip_call():
    from manga_image_translator_amd import lib

    L = lib.load()
    assert lib.MIT_ABI_VERSION == 26 and L.mit_abi_version() == 26          # the entry is additive
    assert lib.MIT_CONV3X3_TILE_H > 0 and lib.MIT_CONV3X3_TILE_W > 0
    assert L.mit_conv3x3_bf16(None, None) != 0 and b"null descriptor" in L.mit_last_error()
    _refused(lib, L, b"null pointer", **{"in": None})
    _refused(lib, L, b"null pointer", w=None)
    _refused(lib, L, b"no output", out_bf16=None)
    for cin in (0, 16, 48, 224, -32):
        _refused(lib, L, b"Cin must be", Cin=cin)
    for n in (0, 16, 48, 128):
        _refused(lib, L, b"N must be", N=n)
    for k in ("B", "H", "W"):
        for v in (0, -1):
            _refused(lib, L, b"must be positive", **{k: v})
    for act in (lib.ACT_SILU, lib.ACT_GELU, 77, lib.ACT_RELU | lib.ACT_POST_FIRST):
        _refused(lib, L, b"act must be", act=act)
    _refused(lib, L, b"input strides: x stride smaller", in_xs=88)
    _refused(lib, L, b"input strides: y stride smaller", in_ys=88)
    _refused(lib, L, b"input strides: y stride smaller", in_bs=-8)
    _refused(lib, L, b"out_bf16 strides: x stride smaller", ob_xs=95)
    _refused(lib, L, b"out_bf16 strides: y stride smaller", ob_ys=95)
    _refused(lib, L, b"out_f32 strides: x stride smaller", out_f32=FAKE + (1 << 27), of_xs=95, of_ys=40 * 96, of_bs=0)
    _refused(lib, L, b"16-byte aligned", **{"in": FAKE + 2})
    _refused(lib, L, b"16-byte aligned", w=FAKE + (1 << 24) + 8)
    _refused(lib, L, b"multiples of 8", in_xs=100, in_ys=40 * 100, in_bs=16 * 40 * 100)
    # the addressing refuses what it cannot reach instead of wrapping
    _refused(lib, L, b"2^31 elements", H=1 << 15, W=1 << 10, in_ys=96 << 10, in_bs=96 << 25, ob_ys=96 << 10, ob_bs=96 << 25)
    _refused(lib, L, b"65535", H=8 * 65536, W=1, in_ys=96, ob_ys=96)
    _refused(lib, L, b"65535", B=65536, in_bs=0, ob_bs=0)
    # the bf16 output inside the input's own buffer: channel ranges [0, Cin) and [off, off + N) must be disjoint
    for off in (0, 32, 95, -95):
        _refused(lib, L, b"overlaps the input channels", out_bf16=FAKE + 2 * off, in_xs=192, in_ys=40 * 192, in_bs=16 * 40 * 192,
                 ob_xs=192, ob_ys=40 * 192, ob_bs=16 * 40 * 192)
    # another pixel grid over the same memory: refused when the extents touch
    _refused(lib, L, b"overlaps the input channels", out_bf16=FAKE + 2 * 1000)
    _refused(lib, L, b"overlaps the input channels", out_bf16=FAKE + 2 * 1000, ob_xs=128, ob_ys=40 * 128, ob_bs=16 * 40 * 128)


def test_descriptor_from_strided_views():
    from manga_image_translator_amd import lib, ops

    w = torch.randn(96, 96, 3, 3, generator=torch.Generator().manual_seed(3))
    layer = ops.Conv3x3Bf16(w, act=ops.ACT_RELU, device="cpu")
    assert layer.scale is None and layer.bias is None and len(layer.w) == 1
    assert torch.equal(layer.w[0].view(torch.int16), ops.pack_rdb_weight(w).view(torch.int16))
    # padded strides on the input, channel slices of wider buffers on the outputs
    xbase = torch.zeros(2, 5, 8, 104, dtype=torch.bfloat16)
    obase = torch.zeros(2, 5, 7, 200, dtype=torch.bfloat16)
    fbase = torch.zeros(2, 5, 7, 100)
    x = xbase[:, :, :7, :96]
    d, = layer.descs(x, out_bf16=obase[..., 100:196], out_f32=fbase[..., 4:])
    assert (d.B, d.H, d.W, d.Cin, d.N, d.act) == (2, 5, 7, 96, 96, lib.ACT_RELU)
    assert (d.in_bs, d.in_ys, d.in_xs) == (5 * 8 * 104, 8 * 104, 104)
    assert (d.ob_bs, d.ob_ys, d.ob_xs) == (5 * 7 * 200, 7 * 200, 200) and d.out_bf16 == obase.data_ptr() + 2 * 100
    assert (d.of_bs, d.of_ys, d.of_xs) == (5 * 7 * 100, 7 * 100, 100) and d.out_f32 == fbase.data_ptr() + 4 * 4
    assert getattr(d, "in") == xbase.data_ptr() and d.w == layer.w[0].data_ptr() and not d.scale and not d.bias
    # the 64 + 32 form: two descriptors over the same input, each with its own weight, its slice of scale / bias and of the outputs
    bn = (torch.rand(96) + 0.5, torch.randn(96), torch.randn(96), torch.rand(96) + 0.5, 1e-5)
    split = ops.Conv3x3Bf16(w, bn=bn, act=ops.ACT_RELU, split=(64, 32), device="cpu")
    sc, bi = ops.fold_bn(*bn)
    assert torch.equal(split.scale, sc) and torch.equal(split.bias, bi)
    d0, d1 = split.descs(x, out_bf16=obase[..., 100:196])
    assert (d0.N, d1.N) == (64, 32) and getattr(d0, "in") == getattr(d1, "in") == xbase.data_ptr()
    assert d0.out_bf16 == obase.data_ptr() + 2 * 100 and d1.out_bf16 == obase.data_ptr() + 2 * 164 and d1.ob_xs == 200
    assert d0.scale == split.scale.data_ptr() and d1.scale == split.scale.data_ptr() + 4 * 64 and d1.bias == split.bias.data_ptr() + 4 * 64
    assert torch.equal(split.w[0].view(torch.int16), ops.pack_rdb_weight(w[:64]).view(torch.int16))
    assert torch.equal(split.w[1].view(torch.int16), ops.pack_rdb_weight(w[64:]).view(torch.int16))
    assert not d0.out_f32 and not d1.out_f32
    with pytest.raises(ValueError):
        layer.descs(xbase[:, :, :7, :64], out_bf16=obase[..., :96])            # channel count of the layer
    with pytest.raises(ValueError):
        layer.descs(x, out_f32=torch.zeros(2, 5, 7, 96, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.Conv3x3Bf16(w, split=(64, 16), device="cpu")


def test_layer0_weight_is_zero_padded_to_one_chunk():
    from manga_image_translator_amd import mc2, ops

    _, f = O.weights()
    w0 = f["intermediate_dncnn.itermediate_dncnn.0.weight"]
    assert tuple(w0.shape) == (96, 15, 3, 3)
    wp = mc2.ffd_layer0_weight(f)
    assert tuple(wp.shape) == (96, mc2.FFD_CIN_BF16, 3, 3) and mc2.FFD_CIN_BF16 == 32
    packed = ops.pack_rdb_weight(wp).view(9, 32, 96)                          # [tap][c][n]
    assert bool((packed[:, 15:].float() == 0).all())                          # rows for c >= 15: exact zeros
    want = w0.permute(2, 3, 1, 0).reshape(9, 15, 96).to(torch.bfloat16)
    assert torch.equal(packed[:, :15].contiguous().view(torch.int16), want.contiguous().view(torch.int16))
    assert not torch.equal(want.float(), w0.permute(2, 3, 1, 0).reshape(9, 15, 96))     # it did round


@pytest.fixture(scope="module")
def cpu_engine():
    from manga_image_translator_amd import mc2

    g, f = O.weights()
    return mc2.Mc2Engine(g, f, device="cpu")


def test_engine_precision_resolution(cpu_engine):
    from manga_image_translator_amd import mc2

    g, f = O.weights()
    assert cpu_engine.precision == "fp32" and cpu_engine.ffd16 is None        # fp32 by default, no bf16 packs
    for bad in ("fp16", "half", "", "BF16", None):
        with pytest.raises(ValueError, match="precision"):
            mc2.Mc2Engine(g, f, device="cpu", precision=bad)                  # refused before any weight is packed
    page = torch.zeros(1, 64, 64, 3, dtype=torch.uint8)
    for call in (lambda: cpu_engine.forward(page, 64, 30, precision="fp16"), lambda: cpu_engine.denoise(page, 30, precision="fp16"),
                 lambda: cpu_engine.colorize(page[..., 0], precision="fp16")):
        with pytest.raises(ValueError, match="precision must be 'fp32' or 'bf16'"):
            call()
    assert cpu_engine.ffd16 is None
    cpu_engine._ensure_bf16()                                                 # what the first bf16 call does
    assert len(cpu_engine.ffd16) == 11 and [l.Cin for l in cpu_engine.ffd16] == [32] + [96] * 10
    assert all(l.Cout == 96 and l.act == mc2.ACT_RELU for l in cpu_engine.ffd16)
    assert cpu_engine.ffd16[0].scale is None and all(l.scale is not None and l.bias is not None for l in cpu_engine.ffd16[1:])
    assert cpu_engine._ffd_sd is None                                         # the fp32 copies of the packed weights are let go


def test_plugin_precision_from_argument_and_environment(monkeypatch):
    from manga_image_translator_amd import plugins as P

    monkeypatch.delenv("MIT_MC2_PRECISION", raising=False)
    assert P.mc2_precision_default() == "fp32"
    assert P.HipMangaColorizer(weights={}).precision == "fp32"
    for v in ("bf16", "fp32"):
        monkeypatch.setenv("MIT_MC2_PRECISION", v)
        assert P.mc2_precision_default() == v
        assert P.HipMangaColorizer(weights={}).precision == v
        assert P.HipMangaColorizer(weights={}, precision="fp32").precision == "fp32"     # an argument wins over the environment
        assert P.HipMangaColorizer(weights={}, precision="bf16").precision == "bf16"
    monkeypatch.setenv("MIT_MC2_PRECISION", "half")
    with pytest.raises(ValueError, match="MIT_MC2_PRECISION"):
        P.mc2_precision_default()
    with pytest.raises(ValueError):
        P.HipMangaColorizer(weights={})                                       # at construction, not at the first page
    monkeypatch.delenv("MIT_MC2_PRECISION")
    with pytest.raises(ValueError, match="mc2 precision"):
        P.HipMangaColorizer(weights={}, precision="fp16")


def test_which_generator_layers_take_one_product(cpu_engine):
    from manga_image_translator_amd import mc2

    layers = mc2.generator_dense_convs()
    fp32 = [name for name, cout, cin, k in layers if not mc2.one_product(cin, k, k, cout)]
    assert fp32 == ["encoder.conv1", "to0.0", "exit.2"]                       # K = 49, K = 9, N = 3
    assert len(layers) == 118 and {"to0.2", "tunnel4.0", "tunnel2.3", "exit.0", "encoder.layer3.5.conv3"} <= {n for n, *_ in layers}
    assert not any(".selayer." in n or n.endswith((".conv2", ".conv_conv")) or n.startswith(("to4", "tunnel1", "deconv")) for n, *_ in layers)
    # the engine applies the same rule to the layers it built: every ops.Conv2d of the generator, the two launches of a
    # _PixelShuffleConv counted once each
    convs = cpu_engine._dense_convs()
    assert len(convs) == len(layers) + 3                                      # three tunnels' .3 are two Conv2d each
    assert [c for c in convs if not cpu_engine._p1(c, True)] == [cpu_engine.conv1, cpu_engine.exit2, cpu_engine.aux[0][0]]
    assert all(cpu_engine._p1(c, False) == 0 for c in convs)                  # fp32 launches carry nprod = 0, as before
    # the one-product tiles take input channels in multiples of 16: the two layers that read to2's 92 channels run, in the bf16
    # precision, as the same layers over 96 channels whose last four weight rows are zero (exact zeros in the sums)
    cpu_engine._ensure_bf16()
    odd = [c for c in convs if c.Cin % 16 and cpu_engine._p1(c, True)]
    assert odd == [cpu_engine.aux[2][1], cpu_engine.aux[3][0]] and all(c.Cin == 92 for c in odd)
    assert set(cpu_engine._wide) == {id(c) for c in odd}
    for c in odd:
        w = cpu_engine._wide[id(c)]
        assert (w.Cin, w.Cout, w.sy, w.act) == (96, c.Cout, c.sy, c.act) and cpu_engine._p1(w, True) == 1
        wk, ck = w.w[:9 * 96, :c.Cout].view(9, 96, c.Cout), c.w[:9 * 92, :c.Cout].view(9, 92, c.Cout)
        assert torch.equal(wk[:, :92], ck) and bool((wk[:, 92:] == 0).all()) and torch.equal(w.bias, c.bias)
    assert mc2.one_product(16, 2, 2, 16) and not mc2.one_product(7, 3, 3, 16) and not mc2.one_product(64, 3, 3, 15)


def _ratios(results, key):
    truth = results["f64"][key]
    (em, ex), (am, ax) = K.errors(results["emul"][key], truth), K.errors(results["autocast"][key], truth)
    return em / am, ex / ax, em


def test_the_yardstick_operand_rounding_is_below_autocast_on_the_gpu_tests_inputs():
    g, f = O.weights()
    pages = K.ffd_pages()
    for b in range(len(pages)):
        r = {m: K.ffd_oracle(f, pages[b], m) for m in ("f64", "f32", "autocast", "emul")}
        mean, mx, em = _ratios(r, "noise")
        print(f"FFDNet page {b}: emulation / autocast  mean {mean:.3f}  max {mx:.3f}")
        assert em > 1e-6 and mean < 1.0 and mx < 0.8, (b, mean, mx)
        moved = lambda m: int(np.abs(r[m]["bgr"].astype(np.int64) - r["f32"]["bgr"]).max())   # noqa: E731
        assert moved("emul") <= moved("autocast") and moved("autocast") >= 1
    for tag, *_ in K.GEN_CASES:
        planes = K.gen_planes(tag)
        r = {m: K.gen_oracle(g, planes, m) for m in ("f64", "f32", "autocast", "emul")}
        mean, mx, em = _ratios(r, "pre")
        print(f"generator {tag}: emulation / autocast  mean {mean:.3f}  max {mx:.3f}")
        assert em > 1e-6 and mean < 1.0 and mx < 0.8, (tag, mean, mx)
        moved = lambda m: int(np.abs(r[m]["out"].astype(np.int64) - r["f32"]["out"]).max())   # noqa: E731
        assert moved("emul") <= moved("autocast") and moved("autocast") >= 1
