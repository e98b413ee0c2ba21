"""``mit_rdb_conv3x3_bf16`` and ``mit_cast_f32_bf16`` on the GPU against a float64 convolution of the same bf16-rounded operands.

Tolerance of the fp32 output (derived, not measured): products of two bf16 numbers are exact in fp32, so only the fp32 summation of
the K = 9 * Cin products (any order: at most K roundings, each relative to a partial sum bounded by S = sum |a * w|) and the at most
six rounded operations of the epilogue (scale, bias, LeakyReLU, post, s2, post2 — no FMA) contribute:
    |got - ref| <= (9 * Cin + 8) * 2^-24 * mag,    mag = (|scale| * S + |bias| + |post|) * |s2| + |post2|
which is the bound  (9 * Cin + 8) * 2^-24 * (S + |bias| + |post| + |post2|)  with the epilogue's scales (both <= 1 here) applied
to the terms they multiply — never looser than it.  The bf16 output must be the round-to-nearest-even of the fp32 output, bit for bit.

Shapes sit around the exported tile sides: one pixel, a few pixels, exactly one tile, one pixel past a tile in both directions (four
workgroups), and two tile rows less one with a short last column block."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from manga_image_translator_amd import lib, ops

from _conv3x3_bf16_cases import SENT_BF16, SENT_F32, _activations, _bits, _check_f32, _padded, _weight

pytestmark = pytest.mark.gpu

TH, TW = lib.MIT_RDB_TILE_H, lib.MIT_RDB_TILE_W
SHAPES = [(1, 1, 1), (2, 3, 5), (1, TH, TW), (2, TH + 1, TW + 1), (1, 2 * TH - 1, TW - 1)]
CINS = [64, 96, 128, 160, 192]
LD = 200                      # channels of the dense-block buffer: 192 + 8 of padding that must keep the sentinel


def _case(B, H, W, Cin, N, seed):
    """Operands (CPU): bf16 activations whose images differ in magnitude by 1000x, a weight, bias, post tensors."""
    g = torch.Generator().manual_seed(seed)
    a, w = _activations(g, B, H, W, Cin), _weight(g, N, Cin)
    bias = torch.randn(N, generator=g)
    post = torch.randn(B, H, W, N, generator=g) * 3.0
    post2 = torch.randn(B, H, W, N, generator=g) * 5.0
    return a, w, bias, post, post2


def _reference(a, wq, scale, bias_eff, alpha, post, s2, post2):
    """float64 form of the launch on the rounded operands; (ref, mag) as [B, H, W, N]."""
    x = a.double().permute(0, 3, 1, 2)
    wd = wq.double()                                   # [N, Cin, 3, 3], already the bf16 values
    acc = F.conv2d(x, wd, padding=1).permute(0, 2, 3, 1)
    S = F.conv2d(x.abs(), wd.abs(), padding=1).permute(0, 2, 3, 1)
    sc = torch.ones(wd.shape[0], dtype=torch.float64) if scale is None else scale.double()
    v = acc * sc + bias_eff.double()
    mag = S * sc.abs() + bias_eff.double().abs()
    if alpha is not None:
        v = torch.where(v >= 0, v, v * float(np.float32(alpha)))
    if post is not None:
        v, mag = v + post.double(), mag + post.double().abs()
    if post2 is not None:
        s2d = float(np.float32(s2))
        v, mag = v * s2d + post2.double(), mag * abs(s2d) + post2.double().abs()
    return v, mag


@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("B,H,W", SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in SHAPES])
def test_conv_n32_leaky_into_the_inputs_own_buffer(cuda, B, H, W, Cin):
    """conv1..4 of a dense block: N = 32, LeakyReLU, bf16 result into the next channel slice of the buffer the input lives in."""
    N = 32
    a, w, bias, _, _ = _case(B, H, W, Cin, N, 100 + Cin + H)
    layer = ops.RdbConv3x3(w, bias, act=ops.ACT_LEAKY, alpha=0.2, device=cuda)
    wq = ops.pack_rdb_weight(w).float().view(3, 3, Cin, N).permute(3, 2, 0, 1)
    ref, mag = _reference(a, wq, None, bias, 0.2, None, 0.0, None)

    def launch(a_dev, both):
        b = a_dev.shape[0]
        base, buf = _padded(b, H, W, LD, LD, torch.bfloat16, SENT_BF16, cuda)
        buf[..., :Cin] = a_dev
        fbase, f32 = _padded(b, H, W, N, N + 8, torch.float32, SENT_F32, cuda)
        layer(buf[..., :Cin], out_bf16=buf[..., Cin:Cin + N] if Cin + N <= 192 else None, out_f32=f32 if both or Cin + N > 192 else None)
        torch.cuda.synchronize()
        return base.cpu(), fbase.cpu()

    a_dev = a.to(cuda)
    if Cin + N <= 192:
        base, fbase = launch(a_dev, both=False)        # bf16 only, in place
        assert bool((fbase == SENT_F32).all())
        base2, fbase2 = launch(a_dev, both=True)
        assert torch.equal(_bits(base), _bits(base2))  # the bf16 result does not depend on whether fp32 is written too
    else:                                              # Cin = 192 fills the buffer: the fp32 output, and bf16 into a buffer of its own
        base2, fbase2 = launch(a_dev, both=True)
        obase, obuf = _padded(B, H, W, N, N + 8, torch.bfloat16, SENT_BF16, cuda)
        _, buf = _padded(B, H, W, LD, LD, torch.bfloat16, SENT_BF16, cuda)
        buf[..., :Cin] = a_dev
        layer(buf[..., :Cin], out_bf16=obuf)
        torch.cuda.synchronize()
        assert torch.equal(_bits(obase.cpu()[:, :, :W, :N]), _bits(fbase2[:, :, :W, :N].to(torch.bfloat16)))
        assert bool((obase.cpu()[:, :, W:] == SENT_BF16).all()) and bool((obase.cpu()[..., N:] == SENT_BF16).all())
        base = None
    got = fbase2[:, :, :W, :N]
    _check_f32(got, ref, mag, Cin, f"n32 {B}x{H}x{W} Cin {Cin}")
    # sentinels: fp32 padding; in the block buffer everything but the output slice is what it was
    assert bool((fbase2[:, :, W:] == SENT_F32).all()) and bool((fbase2[..., N:] == SENT_F32).all())
    if base is not None:
        assert torch.equal(_bits(base[:, :, :W, Cin:Cin + N]), _bits(got.to(torch.bfloat16)))          # RNE of the fp32 value, bit for bit
        assert torch.equal(_bits(base[:, :, :W, :Cin]), _bits(a))
        assert bool((base[:, :, :W, Cin + N:] == SENT_BF16).all()) and bool((base[:, :, W:] == SENT_BF16).all())
    if B == 2:                                         # each image alone: the same bytes
        for i in range(B):
            b1, f1 = launch(a_dev[i:i + 1], both=True)
            assert torch.equal(f1[0].view(torch.int32), fbase2[i].view(torch.int32)), i
            assert torch.equal(_bits(b1[0]), _bits(base2[i])), i


@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("B,H,W", SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in SHAPES])
def test_conv_n64_scale_post_and_outer_residual_into_another_buffer(cuda, B, H, W, Cin):
    """conv5 of a dense block: N = 64, the 0.2 scale, ``post``, then ``* s2 + post2``; fp32 and bf16 outputs in other buffers."""
    N = 64
    a, w, bias, post, post2 = _case(B, H, W, Cin, N, 200 + Cin + W)
    scale = torch.full((N,), 0.2)
    layer = ops.RdbConv3x3(w, bias, out_scale=scale, device=cuda)
    wq = ops.pack_rdb_weight(w).float().view(3, 3, Cin, N).permute(3, 2, 0, 1)
    ref, mag = _reference(a, wq, layer.scale.cpu(), layer.bias.cpu(), None, post, 0.2, post2)
    ref1, mag1 = _reference(a, wq, layer.scale.cpu(), layer.bias.cpu(), None, post, 0.0, None)

    def launch(sl, outer):
        b = sl.stop - sl.start
        _, buf = _padded(b, H, W, Cin, LD, torch.bfloat16, SENT_BF16, cuda)
        buf.copy_(a[sl])
        _, p1 = _padded(b, H, W, N, N + 4, torch.float32, 0.0, cuda)
        _, p2 = _padded(b, H, W, N, N, torch.float32, 0.0, cuda)
        p1.copy_(post[sl])
        p2.copy_(post2[sl])
        fbase, f32 = _padded(b, H, W, N, N + 8, torch.float32, SENT_F32, cuda)
        obase, o16 = _padded(b, H, W, N, LD, torch.bfloat16, SENT_BF16, cuda)    # the first 64 channels of the OTHER block buffer
        kw = dict(post2=p2, s2=0.2) if outer else {}
        layer(buf, post=p1, out_f32=f32, out_bf16=o16, **kw)
        torch.cuda.synchronize()
        return fbase.cpu(), obase.cpu()

    full = slice(0, B)
    for outer, (r, m) in ((True, (ref, mag)), (False, (ref1, mag1))):
        fbase, obase = launch(full, outer)
        got = fbase[:, :, :W, :N]
        _check_f32(got, r, m, Cin, f"n64 {B}x{H}x{W} Cin {Cin} outer {outer}")
        assert torch.equal(_bits(obase[:, :, :W, :N]), _bits(got.to(torch.bfloat16)))
        assert bool((fbase[:, :, W:] == SENT_F32).all()) and bool((fbase[..., N:] == SENT_F32).all())
        assert bool((obase[:, :, W:] == SENT_BF16).all()) and bool((obase[..., N:] == SENT_BF16).all())
        if B == 2 and outer:
            for i in range(B):
                f1, o1 = launch(slice(i, i + 1), outer)
                assert torch.equal(f1[0].view(torch.int32), fbase[i].view(torch.int32)), i
                assert torch.equal(_bits(o1[0]), _bits(obase[i])), i


@pytest.mark.parametrize("N", [32, 64])
def test_unaligned_epilogue_tensors_take_the_narrow_stores_and_give_the_same_bits(cuda, N):
    """Epilogue tensors whose strides or bases are not multiples of four elements cannot take the 16-byte accesses: the launch falls
    to one channel a lane, with the same expression sequence — the bytes of the aligned launch, and sentinels kept around them."""
    B, H, W, Cin = 2, TH + 1, TW + 1, 96
    a, w, bias, post, post2 = _case(B, H, W, Cin, N, 300 + N)
    layer = ops.RdbConv3x3(w, bias, act=ops.ACT_LEAKY, alpha=0.2, out_scale=torch.full((N,), 0.2), device=cuda)
    _, buf = _padded(B, H, W, Cin, LD, torch.bfloat16, SENT_BF16, cuda)
    buf.copy_(a)
    res = []
    for p_ld, f_ld, o_ld, c0 in ((N + 4, N + 8, N + 8, 4), (N + 1, N + 3, N + 5, 1)):
        _, p1 = _padded(B, H, W, N, p_ld, torch.float32, 0.0, cuda)
        _, p2 = _padded(B, H, W, N, p_ld, torch.float32, 0.0, cuda)
        p1.copy_(post)
        p2.copy_(post2)
        fbase = torch.full((B, H, W + 1, f_ld), SENT_F32, device=cuda)
        obase = torch.full((B, H, W + 1, o_ld), SENT_BF16, dtype=torch.bfloat16, device=cuda)
        f32, o16 = fbase[:, :, :W, c0:c0 + N], obase[:, :, :W, c0:c0 + N]
        layer(buf, post=p1, post2=p2, s2=0.2, out_f32=f32, out_bf16=o16)
        torch.cuda.synchronize()
        fb, ob = fbase.cpu(), obase.cpu()
        for t, sent in ((fb, SENT_F32), (ob, SENT_BF16)):
            assert bool((t[:, :, W:] == sent).all()) and bool((t[..., :c0] == sent).all()) and bool((t[..., c0 + N:] == sent).all())
        res.append((fb[:, :, :W, c0:c0 + N].contiguous(), ob[:, :, :W, c0:c0 + N].contiguous()))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
    assert torch.equal(_bits(res[1][1]), _bits(res[1][0].to(torch.bfloat16)))


def test_one_full_size_launch_past_32_bit_byte_offsets(cuda):
    """The upscaler's largest supported page (2048 x 1440 low-resolution pixels), Cin = 192, N = 64, B = 4: the input alone is 4.5 GB, so
    byte offsets pass 2^32 and element offsets of the later images 2^31.  Corner pixels of every image and 4096 seeded random pixels
    against the float64 form; the CPU sees those pixels only."""
    B, H, W, Cin, N = 4, 1440, 2048, 192, 64
    g = torch.Generator(device=cuda).manual_seed(5)
    buf = torch.empty(B, H, W, Cin, dtype=torch.bfloat16, device=cuda)
    post = torch.empty(B, H, W, N, dtype=torch.float32, device=cuda)
    for b in range(B):
        buf[b].normal_(generator=g)
        post[b].normal_(generator=g)
    assert buf.numel() * 2 > 2 ** 32 and buf[3].data_ptr() - buf.data_ptr() > 2 ** 31
    cg = torch.Generator().manual_seed(6)
    w = torch.randn(N, Cin, 3, 3, generator=cg) / (3.0 * Cin ** 0.5)
    bias = torch.randn(N, generator=cg)
    layer = ops.RdbConv3x3(w, bias, out_scale=torch.full((N,), 0.2), device=cuda)
    f32 = torch.empty(B, H, W, N, dtype=torch.float32, device=cuda)
    o16 = torch.empty(B, H, W, N, dtype=torch.bfloat16, device=cuda)
    layer(buf, post=post, post2=post, s2=0.2, out_f32=f32, out_bf16=o16)
    torch.cuda.synchronize()
    wk = ops.pack_rdb_weight(w).double().view(9, Cin, N)                    # [tap, c, n]
    sc, bi = layer.scale.cpu().double(), layer.bias.cpu().double()
    s2 = float(np.float32(0.2))
    n_rand = 4096 // B
    for b in range(B):
        ys = torch.cat([torch.tensor([0, 0, H - 1, H - 1]), torch.randint(0, H, (n_rand,), generator=cg)]).to(cuda)
        xs = torch.cat([torch.tensor([0, W - 1, 0, W - 1]), torch.randint(0, W, (n_rand,), generator=cg)]).to(cuda)
        win = torch.zeros(len(ys), 9, Cin, dtype=torch.float64)
        for t in range(9):
            yy, xx = ys + (t // 3 - 1), xs + (t % 3 - 1)
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = buf[b][yy.clamp(0, H - 1), xx.clamp(0, W - 1)].double() * ok.view(-1, 1)
            win[:, t] = v.cpu()
        acc = torch.einsum("ptc,tcn->pn", win, wk)
        S = torch.einsum("ptc,tcn->pn", win.abs(), wk.abs())
        p = post[b][ys, xs].cpu().double()
        ref = (acc * sc + bi + p) * s2 + p
        mag = (S * sc.abs() + bi.abs() + p.abs()) * s2 + p.abs()
        got = f32[b][ys, xs].cpu()
        _check_f32(got, ref, mag, Cin, f"full size image {b}")
        assert torch.equal(_bits(o16[b][ys, xs].cpu()), _bits(got.to(torch.bfloat16)))


def _tie_values(shape, seed):
    """fp32 values whose low 16 bits sit on, just above and just below the bf16 rounding tie, with even and odd kept bits: rounds up,
    down and to even; plus zeros, infinities and values that carry into the exponent."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    hi = torch.randint(0, 1 << 16, (n,), generator=g, dtype=torch.int64)
    hi = torch.where(((hi >> 7) & 0xff) == 0xff, hi & ~(1 << 14), hi)               # no NaN / inf exponents from the random part
    lo = torch.tensor([0x8000, 0x8001, 0x7fff, 0x0000, 0xffff, 0x0001, 0xc000, 0x4000])[torch.randint(0, 8, (n,), generator=g)]
    bits = (hi << 16) | lo
    special = torch.tensor([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x3f7fffff, 0x7f7fffff, 0x3f808000, 0x3f818000], dtype=torch.int64)
    bits[:len(special)] = special[:min(n, len(special))][:n]
    bits = torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32).view(*shape)


@pytest.mark.parametrize("Cn,src_c0,src_ld,dst_c0", [(64, 0, 64, 0), (64, 0, 72, 0), (70, 0, 72, 4), (13, 1, 72, 3), (3, 2, 8, 1), (4, 4, 8, 8)],
                         ids=["dense64", "slice64", "vec-tail70", "scalar13", "scalar3", "vec4"])
def test_cast_f32_bf16_is_torch_s_rounding(cuda, Cn, src_c0, src_ld, dst_c0):
    B, H, W = 2, 5, 7
    src_base = _tie_values((B, H, W + 1, src_ld), 40 + Cn).to(cuda)
    src = src_base[:, :, :W, src_c0:src_c0 + Cn]
    dst_base, _ = _padded(B, H, W, LD, LD, torch.bfloat16, SENT_BF16, cuda)
    dst = dst_base[:, :, :W, dst_c0:dst_c0 + Cn]
    ops.cast_bf16(src, dst)
    torch.cuda.synchronize()
    want = dst_base.cpu().clone().fill_(SENT_BF16)
    want[:, :, :W, dst_c0:dst_c0 + Cn] = src.cpu().to(torch.bfloat16)
    assert torch.equal(_bits(dst_base.cpu()), _bits(want))
    kept = src.cpu().view(torch.int32)
    up = (_bits(want[:, :, :W, dst_c0:dst_c0 + Cn]).int() & 0xffff) != ((kept >> 16) & 0xffff)
    assert bool(up.any()) and bool((~up).any())        # the data did round both ways
