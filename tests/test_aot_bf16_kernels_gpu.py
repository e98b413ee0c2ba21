"""``mit_aot_conv3x3_bf16`` on the GPU against a float64 convolution of the same bf16-rounded operands.

Tolerance of the fp32 output (derived, not measured; the argument of tests/test_rdb_bf16_gpu.py): products of two bf16 numbers are
exact in fp32, so only the fp32 summation of the K = 9 * Cin products (any order: at most K roundings, each relative to a partial sum
bounded by S = sum |a * w|) and the rounded operations of the epilogue (bias; ReLU is exact) contribute:
    |got - ref| <= (9 * Cin + 8) * 2^-24 * (S + |bias|)
per element.  The bf16 output must be the round-to-nearest-even of the fp32 output, bit for bit.

Shapes are the smallest that can still go wrong: 18 x 20 (rate 16 at the smallest legal sides: nearly every pixel reflects on both
sides), 19 x 45 (partial tiles on both axes, two tiles wide, three tile rows) and 41 x 18 (six tile rows, a 18-pixel partial tile)."""
import pytest
import torch
import torch.nn.functional as F

from manga_image_translator_amd import lib, ops

from _conv3x3_bf16_cases import SENT_BF16, SENT_F32, _activations, _bits, _bits32, _check_f32, _padded, _weight

pytestmark = pytest.mark.gpu

SHAPES = [(2, 18, 20), (1, 19, 45), (1, 41, 18)]
RATES = [1, 2, 4, 8, 16]


def _case(B, H, W, Cin, N, G, seed):
    """Operands (CPU): bf16 activations whose images differ in magnitude by 1000x, G weights and biases."""
    g = torch.Generator().manual_seed(seed)
    a = _activations(g, B, H, W, Cin)
    ws = [_weight(g, N, Cin) for _ in range(G)]
    bs = [torch.randn(N, generator=g) for _ in range(G)]
    return a, ws, bs


def _reference(a, w, bias, rate, relu):
    """float64 form of one group on the rounded operands; (ref, mag) as [B, H, W, N]."""
    N, Cin = w.shape[:2]
    wq = ops.pack_rdb_weight(w).double().view(3, 3, Cin, N).permute(3, 2, 0, 1)      # the bf16 values, [N, Cin, 3, 3]
    x = F.pad(a.double().permute(0, 3, 1, 2), [rate] * 4, mode="reflect")
    acc = F.conv2d(x, wq, dilation=rate).permute(0, 2, 3, 1)
    S = F.conv2d(x.abs(), wq.abs(), dilation=rate).permute(0, 2, 3, 1)
    v = acc + bias.double()
    if relu:
        v = v.clamp_min(0.0)
    return v, S + bias.double().abs()


def test_exported_extents():
    assert (lib.MIT_AOT_TILE_H, lib.MIT_AOT_TILE_W) == (8, 32)      # what the shapes above are chosen around


@pytest.mark.parametrize("Cin", [128, 32])
@pytest.mark.parametrize("N", [32, 128])
@pytest.mark.parametrize("B,H,W", SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in SHAPES])
def test_one_group_every_rate(cuda, B, H, W, N, Cin):
    """A launch of one group at every rate: fp32 and bf16 outputs into padded buffers of their own."""
    relu = N == 32                                                    # the branches carry the ReLU, fuse / gate none
    a, ws, bs = _case(B, H, W, Cin, N, len(RATES), 1000 + 7 * H + N + Cin)
    a_dev = a.to(cuda)
    for i, rate in enumerate(RATES):
        layer = ops.AotConv3x3([ws[i]], [bs[i]], [rate], act=ops.ACT_RELU if relu else ops.ACT_NONE, device=cuda)
        ref, mag = _reference(a, ws[i], bs[i], rate, relu)

        def launch(x, f32=True, b16=True):
            b = x.shape[0]
            _, xin = _padded(b, H, W, Cin, Cin + 8, torch.bfloat16, SENT_BF16, cuda)
            xin.copy_(x)
            fbase, fv = _padded(b, H, W, N, N + 8, torch.float32, SENT_F32, cuda)
            obase, ov = _padded(b, H, W, N, N + 8, torch.bfloat16, SENT_BF16, cuda)
            layer(xin, out_f32=fv if f32 else None, out_bf16=ov if b16 else None)
            torch.cuda.synchronize()
            return fbase.cpu(), obase.cpu()

        fb, ob = launch(a_dev)
        got = fb[:, :, :W, :N]
        _check_f32(got, ref, mag, Cin, f"{B}x{H}x{W} Cin {Cin} N {N} rate {rate}")
        assert torch.equal(_bits(ob[:, :, :W, :N]), _bits(got.to(torch.bfloat16)))          # RNE of the fp32 value, bit for bit
        assert bool((fb[:, :, W:] == SENT_F32).all()) and bool((fb[..., N:] == SENT_F32).all())
        assert bool((ob[:, :, W:] == SENT_BF16).all()) and bool((ob[..., N:] == SENT_BF16).all())
        if relu:
            assert bool((got >= 0).all()) and bool((got == 0).any())
        if rate in (1, 16):                                           # one output only: the same bytes, the other buffer untouched
            f1, o1 = launch(a_dev, b16=False)
            assert torch.equal(_bits32(f1), _bits32(fb)) and bool((o1 == SENT_BF16).all())
            f2, o2 = launch(a_dev, f32=False)
            assert torch.equal(_bits(o2), _bits(ob)) and bool((f2 == SENT_F32).all())
        if B == 2:                                                    # each image alone: the same bytes
            for k in range(B):
                f1, o1 = launch(a_dev[k:k + 1])
                assert torch.equal(_bits32(f1[0]), _bits32(fb[k])), (rate, k)
                assert torch.equal(_bits(o1[0]), _bits(ob[k])), (rate, k)


@pytest.mark.parametrize("B,H,W", SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in SHAPES])
def test_four_branches_as_one_launch(cuda, B, H, W):
    """The four dilated branches of a block: one launch of four groups into four slices of one bf16 buffer — the bytes of four
    launches of one group, sentinels kept outside every slice and outside W."""
    Cin, N, rates, LD, C0 = 128, 32, (2, 4, 8, 16), 144, 8
    a, ws, bs = _case(B, H, W, Cin, N, 4, 2000 + H)
    a_dev = a.to(cuda)
    _, xin = _padded(B, H, W, Cin, Cin, torch.bfloat16, SENT_BF16, cuda)
    xin.copy_(a_dev)
    grouped = ops.AotConv3x3(ws, bs, rates, act=ops.ACT_RELU, device=cuda)
    cbase, cat = _padded(B, H, W, 4 * N, LD, torch.bfloat16, SENT_BF16, cuda, c0=C0)     # slices at channels 8 .. 136 of 144
    fbase, f32 = _padded(B, H, W, 4 * N, LD, torch.float32, SENT_F32, cuda, c0=C0)
    grouped(xin, out_bf16=cat, out_f32=f32)
    sbase, scat = _padded(B, H, W, 4 * N, LD, torch.bfloat16, SENT_BF16, cuda, c0=C0)
    for g in range(4):
        one = ops.AotConv3x3([ws[g]], [bs[g]], [rates[g]], act=ops.ACT_RELU, device=cuda)
        one(xin, out_bf16=scat[..., g * N:(g + 1) * N])
    torch.cuda.synchronize()
    cb, sb, fb = cbase.cpu(), sbase.cpu(), fbase.cpu()
    assert torch.equal(_bits(cb), _bits(sb))                          # slices and sentinels alike
    for t, sent in ((cb, SENT_BF16), (fb, SENT_F32)):
        assert bool((t[:, :, W:] == sent).all()) and bool((t[..., :C0] == sent).all()) and bool((t[..., C0 + 4 * N:] == sent).all())
    assert torch.equal(_bits(cb[:, :, :W, C0:C0 + 4 * N]), _bits(fb[:, :, :W, C0:C0 + 4 * N].to(torch.bfloat16)))
    for g in range(4):
        ref, mag = _reference(a, ws[g], bs[g], rates[g], True)
        _check_f32(fb[:, :, :W, C0 + g * N:C0 + (g + 1) * N], ref, mag, Cin, f"grouped {B}x{H}x{W} rate {rates[g]}")
    # bf16 only, as the engine launches it: the same bytes
    c2base, cat2 = _padded(B, H, W, 4 * N, LD, torch.bfloat16, SENT_BF16, cuda, c0=C0)
    grouped(xin, out_bf16=cat2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(c2base.cpu()), _bits(cb))


def test_two_wide_groups_as_one_launch(cuda):
    """N = 128 with two groups (rates 1 and 3, a rate the network does not use) into the halves of a 256-channel fp32 buffer."""
    B, H, W, Cin, N, rates = 1, 19, 45, 32, 128, (1, 3)
    a, ws, bs = _case(B, H, W, Cin, N, 2, 2500)
    layer = ops.AotConv3x3(ws, [bs[0], None], rates, device=cuda)
    fbase, f32 = _padded(B, H, W, 2 * N, 2 * N + 4, torch.float32, SENT_F32, cuda)
    layer(a.to(cuda), out_f32=f32)
    torch.cuda.synchronize()
    fb = fbase.cpu()
    for g in range(2):
        bias = bs[g] if g == 0 else torch.zeros(N)
        ref, mag = _reference(a, ws[g], bias, rates[g], False)
        _check_f32(fb[:, :, :W, g * N:(g + 1) * N], ref, mag, Cin, f"two wide groups, rate {rates[g]}")
    assert bool((fb[:, :, W:] == SENT_F32).all()) and bool((fb[..., 2 * N:] == SENT_F32).all())


@pytest.mark.parametrize("N", [32, 128])
def test_unaligned_outputs_take_the_narrow_stores_and_give_the_same_bits(cuda, N):
    """Outputs whose strides or bases are not multiples of four elements cannot take the 16- / 8-byte stores: the launch falls to one
    channel a lane, with the same expression sequence — the bytes of the aligned launch, and sentinels kept around them."""
    B, H, W, Cin, rate = 2, 19, 45, 128, 2
    a, ws, bs = _case(B, H, W, Cin, N, 1, 3000 + N)
    layer = ops.AotConv3x3(ws, bs, [rate], act=ops.ACT_RELU, device=cuda)
    x = a.to(cuda)
    res = []
    for f_ld, o_ld, c0 in ((N + 8, N + 8, 4), (N + 3, N + 5, 1)):
        fbase = torch.full((B, H, W + 1, f_ld), SENT_F32, device=cuda)
        obase = torch.full((B, H, W + 1, o_ld), SENT_BF16, dtype=torch.bfloat16, device=cuda)
        layer(x, out_f32=fbase[:, :, :W, c0:c0 + N], out_bf16=obase[:, :, :W, c0:c0 + N])
        torch.cuda.synchronize()
        fb, ob = fbase.cpu(), obase.cpu()
        for t, sent in ((fb, SENT_F32), (ob, SENT_BF16)):
            assert bool((t[:, :, W:] == sent).all()) and bool((t[..., :c0] == sent).all()) and bool((t[..., c0 + N:] == sent).all())
        res.append((fb[:, :, :W, c0:c0 + N].contiguous(), ob[:, :, :W, c0:c0 + N].contiguous()))
    assert torch.equal(_bits32(res[0][0]), _bits32(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
    assert torch.equal(_bits(res[1][1]), _bits(res[1][0].to(torch.bfloat16)))
    ref, mag = _reference(a, ws[0], bs[0], rate, True)
    _check_f32(res[1][0], ref, mag, Cin, f"narrow stores N {N}")
