"""The upscaler's bf16 precision, the parts that need no GPU: the argument checks of ``mit_rdb_conv3x3_bf16`` and ``mit_cast_f32_bf16``
(before any HIP call: fake pointers that are never dereferenced), the host weight packer, how the plugin's ``precision`` resolves and
the ``nprod`` argument of ``ops.UpsampleConv2d``."""
import ctypes as C

import pytest
import torch

FAKE = 1 << 20      # 16-byte aligned, never dereferenced: every call below is refused by the argument checks


def _desc(lib, **kw):
    """A descriptor the checks accept (conv1 of a dense block in its own [1, 16, 40, 192] buffer), then ``kw`` on top."""
    d = lib.MitRdbConv()
    d.B, d.H, d.W, d.Cin, d.N = 1, 16, 40, 64, 32
    d.in_bs, d.in_ys, d.in_xs = 16 * 40 * 192, 40 * 192, 192
    setattr(d, "in", FAKE)
    d.w = FAKE + (1 << 24)
    d.out_bf16 = FAKE + 2 * 64
    d.ob_bs, d.ob_ys, d.ob_xs = d.in_bs, d.in_ys, d.in_xs
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, L, what, **kw):
    rc = L.mit_rdb_conv3x3_bf16(C.byref(_desc(lib, **kw)), None)
    msg = L.mit_last_error()
    assert rc != 0 and what in msg, (kw, rc, msg)


def test_rdb_conv_refuses_bad_arguments_before_any_hip_call():
    from manga_image_translator_amd import lib

    L = lib.load()
    assert lib.MIT_RDB_TILE_H > 0 and lib.MIT_RDB_TILE_W > 0
    assert L.mit_rdb_conv3x3_bf16(None, None) != 0 and b"null descriptor" in L.mit_last_error()
    _refused(lib, L, b"null pointer", **{"in": None})
    _refused(lib, L, b"null pointer", w=None)
    _refused(lib, L, b"null pointer", out_bf16=None)                     # no output at all
    for cin in (0, 32, 48, 80, 224, -64):
        _refused(lib, L, b"Cin must be", Cin=cin)
    for n in (0, 16, 48, 96, 128):
        _refused(lib, L, b"N must be", N=n)
    for k in ("B", "H", "W"):
        for v in (0, -1):
            _refused(lib, L, b"must be positive", **{k: v})
    _refused(lib, L, b"act must be", act=lib.ACT_RELU)
    _refused(lib, L, b"input strides: x stride smaller", in_xs=56)
    _refused(lib, L, b"input strides: y stride smaller", in_ys=184)
    _refused(lib, L, b"input strides: y stride smaller", in_bs=-8)
    _refused(lib, L, b"out_bf16 strides: x stride smaller", ob_xs=31)
    _refused(lib, L, b"out_f32 strides: x stride smaller", out_f32=FAKE + (1 << 26), of_xs=31, of_ys=40 * 32, of_bs=0)
    _refused(lib, L, b"post strides: x stride smaller", post=FAKE + (1 << 26), post_xs=16, post_ys=40 * 32)
    _refused(lib, L, b"post2 strides: y stride smaller", post2=FAKE + (1 << 26), post2_xs=32, post2_ys=16)
    _refused(lib, L, b"16-byte aligned", **{"in": FAKE + 2})
    _refused(lib, L, b"16-byte aligned", in_xs=196, in_ys=40 * 196, in_bs=16 * 40 * 196, ob_xs=196, ob_ys=40 * 196, ob_bs=16 * 40 * 196)
    # the addressing refuses what it cannot reach instead of wrapping: one image of 2^31 elements or more, too many tile rows or images
    _refused(lib, L, b"2^31 elements", H=1 << 15, W=1 << 10, in_ys=192 << 10, in_bs=192 << 25, ob_ys=192 << 10, ob_bs=192 << 25)
    _refused(lib, L, b"65535", H=8 * 65536, W=1, in_ys=192, ob_ys=192)
    _refused(lib, L, b"65535", B=65536, in_bs=0, ob_bs=0, out_bf16=FAKE + (1 << 26), ob_xs=32, ob_ys=40 * 32)
    # the bf16 output inside the input's own buffer: channel ranges [0, Cin) and [off, off + N) must be disjoint
    for off in (0, 32, 63, -31):
        _refused(lib, L, b"overlaps the input channels", out_bf16=FAKE + 2 * off)
    _refused(lib, L, b"overlaps the input channels", Cin=96)             # conv2 reads [0, 96) and would write [64, 96)
    # another pixel grid over the same memory: refused when the extents touch
    _refused(lib, L, b"overlaps the input channels", out_bf16=FAKE + 2 * 1000, ob_xs=32, ob_ys=40 * 32, ob_bs=16 * 40 * 32)


def test_cast_refuses_bad_arguments_before_any_hip_call():
    from manga_image_translator_amd import lib

    L = lib.load()
    ok = dict(s=(16 * 40 * 64, 40 * 64, 64), d=(16 * 40 * 192, 40 * 192, 192), size=(1, 16, 40, 64))

    def call(src=FAKE, dst=FAKE + (1 << 24), s=ok["s"], d=ok["d"], size=ok["size"]):
        return L.mit_cast_f32_bf16(src, *s, dst, *d, *size, None)

    assert call(src=None) != 0 and b"null pointer" in L.mit_last_error()
    assert call(dst=None) != 0 and b"null pointer" in L.mit_last_error()
    for i in range(4):
        for v in (0, -3):
            size = list(ok["size"])
            size[i] = v
            assert call(size=size) != 0 and b"must be positive" in L.mit_last_error(), size
    assert call(s=(16 * 40 * 64, 40 * 64, 63)) != 0 and b"x stride smaller" in L.mit_last_error()
    assert call(d=(16 * 40 * 192, 40 * 192, 48)) != 0 and b"x stride smaller" in L.mit_last_error()
    assert call(s=(16 * 40 * 64, 32, 64)) != 0 and b"y stride smaller" in L.mit_last_error()
    assert call(d=(-1, 40 * 192, 192)) != 0 and b"negative batch stride" in L.mit_last_error()


def test_weight_packer_is_its_definition():
    from manga_image_translator_amd import ops

    g = torch.Generator().manual_seed(7)
    N, Cin = 32, 64
    w = torch.randn(N, Cin, 3, 3, generator=g) * torch.logspace(-3, 2, N).view(N, 1, 1, 1)
    p = ops.pack_rdb_weight(w)
    assert p.dtype == torch.bfloat16 and tuple(p.shape) == (9 * Cin, N) and p.is_contiguous()
    want = torch.empty(9 * Cin, N, dtype=torch.bfloat16)
    for ky in range(3):
        for kx in range(3):
            for c in range(0, Cin, 7):
                want[(ky * 3 + kx) * Cin + c] = w[:, c, ky, kx].to(torch.bfloat16)     # RNE
    rows = [(ky * 3 + kx) * Cin + c for ky in range(3) for kx in range(3) for c in range(0, Cin, 7)]
    assert torch.equal(p[rows].view(torch.int16), want[rows].view(torch.int16))
    assert not torch.equal(p.float(), w.permute(2, 3, 1, 0).reshape(9 * Cin, N))     # it did round
    layer = ops.RdbConv3x3(w, torch.arange(N, dtype=torch.float32), out_scale=torch.full((N,), 0.2), device="cpu")
    assert torch.equal(layer.w.view(torch.int16), p.view(torch.int16))
    assert torch.equal(layer.bias, torch.arange(N, dtype=torch.float32) * 0.2) and torch.equal(layer.scale, torch.full((N,), 0.2))
    with pytest.raises(ValueError):
        ops.pack_rdb_weight(torch.zeros(32, 64, 1, 1))


def test_rdb_descriptor_from_views():
    from manga_image_translator_amd import lib, ops

    buf = torch.zeros(2, 5, 7, 192, dtype=torch.bfloat16)
    layer = ops.RdbConv3x3(torch.zeros(32, 96, 3, 3), torch.zeros(32), act=ops.ACT_LEAKY, alpha=0.2, device="cpu")
    d = layer.desc(buf[..., :96], out_bf16=buf[..., 96:128])
    assert (d.B, d.H, d.W, d.Cin, d.N, d.act) == (2, 5, 7, 96, 32, lib.ACT_LEAKY)
    assert (d.in_bs, d.in_ys, d.in_xs) == (5 * 7 * 192, 7 * 192, 192) == (d.ob_bs, d.ob_ys, d.ob_xs)
    assert d.out_bf16 - getattr(d, "in") == 2 * 96 and not d.out_f32 and not d.post and not d.post2
    with pytest.raises(ValueError):
        layer.desc(buf[..., :64], out_bf16=buf[..., 96:128])             # channel count of the layer
    with pytest.raises(ValueError):
        layer.desc(buf[..., :96], out_f32=torch.zeros(2, 5, 7, 32, dtype=torch.bfloat16))


def test_precision_default_from_environment(monkeypatch):
    from manga_image_translator_amd import plugins as P

    monkeypatch.delenv("MIT_ESRGAN_PRECISION", raising=False)
    assert P.esrgan_precision_default() == "fp32"
    assert P.HipESRGANUpscaler(weights={}).precision == "fp32"
    for v in ("bf16", "fp32"):
        monkeypatch.setenv("MIT_ESRGAN_PRECISION", v)
        assert P.esrgan_precision_default() == v
        assert P.HipESRGANUpscaler(weights={}).precision == v
        assert P.HipESRGANUpscaler(weights={}, precision="fp32").precision == "fp32"     # an argument wins over the environment
        assert P.HipESRGANUpscaler(weights={}, precision="bf16").precision == "bf16"
    monkeypatch.setenv("MIT_ESRGAN_PRECISION", "half")
    with pytest.raises(ValueError):
        P.esrgan_precision_default()
    with pytest.raises(ValueError):
        P.HipESRGANUpscaler(weights={})
    monkeypatch.delenv("MIT_ESRGAN_PRECISION")
    with pytest.raises(ValueError):
        P.HipESRGANUpscaler(weights={}, precision="fp16")


def test_engine_refuses_an_unknown_precision():
    from manga_image_translator_amd import esrgan

    with pytest.raises(ValueError, match="precision"):
        esrgan._check_precision("fp16", "EsrganEngine")
    assert esrgan._check_precision("bf16", "EsrganEngine") == "bf16"


def test_upsample_conv_descs_carry_nprod():
    from manga_image_translator_amd import ops

    layer = ops.UpsampleConv2d(torch.randn(8, 16, 3, 3), torch.zeros(8), device="cpu")
    x, out = torch.zeros(1, 3, 5, 16), torch.zeros(1, 6, 10, 8)
    ds = layer.descs(x, out)
    assert len(ds) == 4 and all(d.nprod == 0 for d in ds)
    ds = layer.descs(x, out, nprod=1)
    assert len(ds) == 4 and all(d.nprod == 1 for d in ds)
