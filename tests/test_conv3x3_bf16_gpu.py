"""``mit_conv3x3_bf16`` on the GPU against a float64 convolution of the same bf16-rounded operands.

Tolerance of the fp32 output (derived, not measured; the argument is the one in tests/test_rdb_bf16_gpu.py): products of two bf16
numbers are exact in fp32, so only the fp32 summation of the K = 9 * Cin products and the at most three rounded operations of the
epilogue (scale, bias, LeakyReLU — no FMA) contribute:
    |got - ref| <= (9 * Cin + 8) * 2^-24 * mag,    mag = |scale| * sum |a * w| + |bias|
The bf16 output must be the round-to-nearest-even of the fp32 output, bit for bit.

Shapes: one pixel past a tile in both directions (every tile kind: full, right edge, bottom edge, corner) with two images that differ
1000x in magnitude, and a 1 x 1 image.  Outputs are channel slices of wider, sentinel-filled buffers with padded x and y strides:
anything stored outside the addressed channels and pixels shows.  At N = 96 the wide store has 24 lane groups of four channels — 48
lanes carry two pixels an iteration and the other 16 must idle; a lane that did not would write the pixel after its iteration's, past
the tile's last column, which is where the sentinels of the right-edge tiles and of the 1 x 1 image sit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from manga_image_translator_amd import lib, ops

from _conv3x3_bf16_cases import SENT_BF16, SENT_F32, _activations, _bits, _bits32, _check_f32, _weight

pytestmark = pytest.mark.gpu

TH, TW = lib.MIT_CONV3X3_TILE_H, lib.MIT_CONV3X3_TILE_W
CINS, NS = [32, 96, 192], [32, 64, 96]
ACTS = {"none": (ops.ACT_NONE, 0.0), "relu": (ops.ACT_RELU, 0.0), "leaky": (ops.ACT_LEAKY, 0.2)}


def _case(B, H, W, Cin, N, seed, affine=True):
    g = torch.Generator().manual_seed(seed)
    a, w = _activations(g, B, H, W, Cin), _weight(g, N, Cin)
    bn = None
    if affine:   # (gamma, beta, mean, var, eps): folds to a scale of either sign and a bias
        bn = (torch.randn(N, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g) * 0.1, torch.rand(N, generator=g) + 0.5, 1e-5)
    return a, w, bn


def _reference(a, layer, w, act):
    """float64 form of the launch on the rounded operands; (ref, mag) as [B, H, W, N]."""
    Cin, N = w.shape[1], w.shape[0]
    wq = ops.pack_rdb_weight(w).double().view(3, 3, Cin, N).permute(3, 2, 0, 1)
    x = a.double().permute(0, 3, 1, 2)
    acc = F.conv2d(x, wq, padding=1).permute(0, 2, 3, 1)
    S = F.conv2d(x.abs(), wq.abs(), padding=1).permute(0, 2, 3, 1)
    sc = torch.ones(N, dtype=torch.float64) if layer.scale is None else layer.scale.cpu().double()
    bi = torch.zeros(N, dtype=torch.float64) if layer.bias is None else layer.bias.cpu().double()
    v, mag = acc * sc + bi, S * sc.abs() + bi.abs()
    code, alpha = ACTS[act]
    if code == ops.ACT_RELU:
        v = v.clamp_min(0)
    elif code == ops.ACT_LEAKY:
        v = torch.where(v >= 0, v, v * float(np.float32(alpha)))
    return v, mag


def _launch(layer, a_dev, N, cuda, *, f32=True, b16=True, c0=4, pad=8):
    """The layer into channels c0 .. c0 + N of sentinel-filled [B, H, W + 1, N + pad] buffers; returns the whole buffers on the CPU."""
    B, H, W, _ = a_dev.shape
    fbase = torch.full((B, H, W + 1, N + pad), SENT_F32, device=cuda)
    obase = torch.full((B, H, W + 1, N + pad), SENT_BF16, dtype=torch.bfloat16, device=cuda)
    layer(a_dev, out_f32=fbase[:, :, :W, c0:c0 + N] if f32 else None, out_bf16=obase[:, :, :W, c0:c0 + N] if b16 else None)
    torch.cuda.synchronize()
    return fbase.cpu(), obase.cpu()


def _untouched(base, W, c0, N, sent):
    return bool((base[:, :, W:] == sent).all()) and bool((base[..., :c0] == sent).all()) and bool((base[..., c0 + N:] == sent).all())


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Cin", CINS)
def test_every_tile_kind_both_store_forms_and_the_split_launch(cuda, Cin, N):
    B, H, W = 2, TH + 1, TW + 1
    a, w, bn = _case(B, H, W, Cin, N, 1000 + Cin + N)
    layer = ops.Conv3x3Bf16(w, bn=bn, act=ops.ACT_RELU, device=cuda)
    ref, mag = _reference(a, layer, w, "relu")
    # the input as a channel slice with padded strides as well (multiples of 8 elements: 16-byte loads)
    abase = torch.full((B, H, W + 1, Cin + 8), SENT_BF16, dtype=torch.bfloat16, device=cuda)
    a_dev = abase[:, :, :W, :Cin]
    a_dev.copy_(a)
    fb, ob = _launch(layer, a_dev, N, cuda)                               # wide stores: bases and strides multiples of four elements
    got = fb[:, :, :W, 4:4 + N]
    _check_f32(got, ref, mag, Cin, f"Cin {Cin} N {N}")
    assert torch.equal(_bits(ob[:, :, :W, 4:4 + N]), _bits(got.to(torch.bfloat16)))         # RNE of the fp32 value, bit for bit
    assert _untouched(fb, W, 4, N, SENT_F32) and _untouched(ob, W, 4, N, SENT_BF16)
    assert bool((got[..., :] >= 0).all()) and bool((got == 0).any()) and bool((got > 0).any())   # the ReLU cut something, not everything
    # each output alone: the same bits, and the other buffer keeps its sentinels
    f1, o1 = _launch(layer, a_dev, N, cuda, b16=False)
    assert torch.equal(_bits32(f1), _bits32(fb)) and bool((o1 == SENT_BF16).all())
    f2, o2 = _launch(layer, a_dev, N, cuda, f32=False)
    assert torch.equal(_bits(o2), _bits(ob)) and bool((f2 == SENT_F32).all())
    # outputs one element off the alignment: the narrow stores, with the same bits and the sentinels kept
    fn, on = _launch(layer, a_dev, N, cuda, c0=1, pad=5)
    assert torch.equal(_bits32(fn[:, :, :W, 1:1 + N]), _bits32(got)) and torch.equal(_bits(on[:, :, :W, 1:1 + N]), _bits(ob[:, :, :W, 4:4 + N]))
    assert _untouched(fn, W, 1, N, SENT_F32) and _untouched(on, W, 1, N, SENT_BF16)
    # each image alone: the same bytes
    for i in range(B):
        fi, oi = _launch(layer, a_dev[i:i + 1], N, cuda)
        assert torch.equal(_bits32(fi[0]), _bits32(fb[i])) and torch.equal(_bits(oi[0]), _bits(ob[i])), i
    # the columns as two launches into channel slices (64 + 32 at N = 96): the one launch's bits
    if N > 32:
        split = ops.Conv3x3Bf16(w, bn=bn, act=ops.ACT_RELU, split=(N - 32, 32), device=cuda)
        assert [d.N for d in split.descs(a_dev, out_bf16=torch.empty(B, H, W, N, dtype=torch.bfloat16, device=cuda))] == [N - 32, 32]
        fs, os_ = _launch(split, a_dev, N, cuda)
        assert torch.equal(_bits32(fs), _bits32(fb)) and torch.equal(_bits(os_), _bits(ob))
    assert bool((abase[:, :, W:] == SENT_BF16).all()) and bool((abase[..., Cin:] == SENT_BF16).all())


@pytest.mark.parametrize("N", NS)
def test_one_pixel_image(cuda, N):
    Cin = 96
    a, w, bn = _case(1, 1, 1, Cin, N, 2000 + N)
    layer = ops.Conv3x3Bf16(w, bn=bn, act=ops.ACT_NONE, device=cuda)
    ref, mag = _reference(a, layer, w, "none")
    a_dev = a.to(cuda)
    res = []
    for c0, pad in ((4, 8), (1, 5)):
        fb, ob = _launch(layer, a_dev, N, cuda, c0=c0, pad=pad)
        got = fb[:, :, :1, c0:c0 + N]
        _check_f32(got, ref, mag, Cin, f"1x1 N {N} c0 {c0}")
        assert torch.equal(_bits(ob[:, :, :1, c0:c0 + N]), _bits(got.to(torch.bfloat16)))
        assert _untouched(fb, 1, c0, N, SENT_F32) and _untouched(ob, 1, c0, N, SENT_BF16)
        res.append(got.contiguous())
    assert torch.equal(_bits32(res[0]), _bits32(res[1]))


@pytest.mark.parametrize("affine", [True, False], ids=["scale-bias", "null"])
@pytest.mark.parametrize("act", list(ACTS))
def test_each_activation_with_and_without_scale_and_bias(cuda, act, affine):
    B, H, W, Cin, N = 2, TH + 1, TW + 1, 96, 96
    a, w, bn = _case(B, H, W, Cin, N, 3000 + len(act) + affine, affine)
    code, alpha = ACTS[act]
    layer = ops.Conv3x3Bf16(w, bn=bn, act=code, alpha=alpha, device=cuda)
    assert (layer.scale is None) == (not affine) and (layer.bias is None) == (not affine)
    ref, mag = _reference(a, layer, w, act)
    fb, ob = _launch(layer, a.to(cuda), N, cuda)
    got = fb[:, :, :W, 4:4 + N]
    _check_f32(got, ref, mag, Cin, f"act {act} affine {affine}")
    assert torch.equal(_bits(ob[:, :, :W, 4:4 + N]), _bits(got.to(torch.bfloat16)))
    assert _untouched(fb, W, 4, N, SENT_F32) and _untouched(ob, W, 4, N, SENT_BF16)
    assert bool((got < 0).any()) == (act != "relu")
