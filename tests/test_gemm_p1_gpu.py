"""The one-product tiles of mit_conv_gemm (MitConvGemm.nprod = 1, "p1": both operands rounded to bf16, fp32 accumulation) at the layer
level, through the layer classes the LaMa engine uses.

What is checked, and why it is sharp: with operands that ARE bf16 numbers every product is exact in fp32, so a p1 tile and an fp32 tile
differ only in the order of the fp32 accumulation.  The fp32 MFMA tile is fed the pre-rounded operands and its error against float64
taken (e32); the p1 tile, fed the UNROUNDED operands, must land within the bound tests/test_gemm_split_gpu.py holds the 6- and 9-pair
tiles to (4 * e32 + 2e-6 of the output's max).  Every p1 tile, buffer-load twins and the automatic choice included, gives the same bits
on the same problem: a page's result depends neither on the tile nor on the launch size."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

K32 = ("split128x128x32p1o", "split128x128x32p1u", "split128x64x32p1o", "split128x64x32p1u", "split128x192x32p1o", "split128x192x32p1u",
       "split64x64x32p1o", "split64x64x32p1u")
K16 = ("split64x64x16p1o", "split64x64x16p1u")


def _cfg(name):
    from manga_image_translator_amd import lib
    L = lib.load()
    i = 0
    while True:
        n = L.mit_conv_gemm_config_name(i)
        if n is None:
            raise KeyError(name)
        if n.decode() == name:
            return i
        i += 1


def _rel(a, b, ymax):
    return float((a.double() - b.double()).abs().max()) / ymax


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


CASES = [
    # B, Cin, Cout, H, W, k, stride, pad mode, act, fp32 tile, p1 tiles
    (2, 128, 128, 40, 56, 3, 1, "reflect", 1, "fast128x128x16w4c", K32 + K16),      # LaMa-like 3x3, reflect; 192-column tile with a ragged tile
    (4, 64, 64, 64, 48, 3, 2, "zero", 0, "fast128x64x16w5c", K32 + K16),            # stride 2
    (1, 320, 1280, 12, 200, 1, 1, "zero", 5, "fast128x128x16w4c", K32),             # 1x1, long N
    (1, 64, 200, 9, 13, 3, 1, "reflect", 2, "fast128x128x16w4c", K32 + K16),        # ragged M and N
    (2, 384, 192, 16, 23, 1, 1, "zero", 1, "fast128x128x16w4c", K32),               # N = 192: LaMa spectral conv1
    (1, 192, 384, 16, 23, 1, 1, "zero", 1, "fast128x128x16w4c", K32),               # N = 384: two 192-column tiles
    (1, 48, 200, 25, 40, 3, 1, "zero", 2, "fast128x128x16w4c", K16),                # K = 432 is not a multiple of the 32-wide K-tile: 16-wide form
    (1, 16, 40, 9, 11, 1, 1, "zero", 0, "fast128x64x16w5c", K16),                   # one 16-wide K-tile, tiny problem
    (1, 32, 96, 20, 24, 1, 1, "zero", 1, "fast128x64x16w5c", K32 + K16),            # one 32-wide K-tile
    (1, 96, 128, 20, 24, 1, 1, "zero", 0, "fast128x128x16w4c", K32 + K16),          # three K-tiles: every peeled iteration kind
    (2, 128, 512, 27, 41, 3, 2, "zero", 1, "fast128x128x16w4c", K32),               # long K, stride 2, odd M
]


@pytest.mark.parametrize("mode", [6, 0], ids=["split6", "fp32mfma"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[1]}to{c[2]}k{c[5]}s{c[6]}")
def test_conv2d_p1_tiles(case, mode):
    from manga_image_translator_amd import ops

    B, Cin, Cout, H, W, k, s, pmode, act, ref_tile, tiles = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Cin, H, W, generator=g)
    x[:, ::7] *= 4.0
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.1
    pad = k // 2
    kw = dict(stride=s, padding=pad, pad_mode=ops.PAD_REFLECT if pmode == "reflect" else ops.PAD_ZERO, act=act, alpha=0.1, device="cuda")
    with ops.gemm_mode(mode):           # the tiles are taken whatever the GEMM mode is, and whatever it was when the weight was packed
        layer = ops.Conv2d(w, b, **kw)
        layer_r = ops.Conv2d(_bf(w), b, **kw)                                         # pre-rounded operands for the fp32 tile
        xd = x.permute(0, 2, 3, 1).contiguous().cuda()
        xr = _bf(x)
        xp = F.pad(xr.double(), (pad, pad, pad, pad), mode="reflect" if pmode == "reflect" else "constant") if pad else xr.double()
        want = F.conv2d(xp, _bf(w).double(), b.double(), stride=s)
        want = {0: lambda t: t, 1: torch.relu, 2: lambda t: F.leaky_relu(t, 0.1), 5: F.gelu}[act](want).permute(0, 2, 3, 1)
        ymax = float(want.abs().max())
        y32 = layer_r(xr.permute(0, 2, 3, 1).contiguous().cuda(), cfg=_cfg(ref_tile)).cpu()
        e32 = _rel(y32, want, ymax)
        first = layer(xd, nprod=1).cpu()                                              # the automatic choice
        assert torch.isfinite(first).all()
        err = _rel(first, want, ymax)
        print(f"{Cin}->{Cout} k{k} s{s} mode {mode}: e32 {e32:.2e}, p1 {err:.2e} (bound {4 * e32 + 2e-6:.2e})")
        assert err <= 4 * e32 + 2e-6, ("auto", err, e32)
        for t in tiles:
            y = layer(xd, cfg=_cfg(t), nprod=1).cpu()
            assert torch.equal(y, first), f"{t} differs bitwise from the automatic choice: a page's result would depend on the tile"
        # the rounding is really there: against the float64 result of the UNROUNDED operands the p1 tile is a bf16 product
        xp0 = F.pad(x.double(), (pad, pad, pad, pad), mode="reflect" if pmode == "reflect" else "constant") if pad else x.double()
        full = F.conv2d(xp0, w.double(), b.double(), stride=s)
        full = {0: lambda t: t, 1: torch.relu, 2: lambda t: F.leaky_relu(t, 0.1), 5: F.gelu}[act](full).permute(0, 2, 3, 1)
        assert 1e-5 < _rel(first, full, ymax) < 2e-2


def test_batched_p1_tiles():
    """Z = 36 slices with their own planes (ws_zs0) and slice bases (a_zs0): the batched GEMM of WinogradConv3x3 as a carrier."""
    from manga_image_translator_amd import ops

    g = torch.Generator().manual_seed(3)
    w = torch.randn(192, 128, 3, 3, generator=g) * 0.05
    layer = ops.WinogradConv3x3(w, None, pad_mode=ops.PAD_REFLECT, device="cuda")
    assert ops.register_split(layer.u, force=True) is not None
    ref = ops.WinogradConv3x3(w, None, pad_mode=ops.PAD_REFLECT, device="cuda")
    ref.u.copy_(_bf(ref.u))
    T = 1500
    v = torch.randn(36, T, 128, generator=g).cuda()
    vr = _bf(v)
    m32 = torch.empty(36, T, 192, device="cuda")
    ms = torch.empty_like(m32)
    ops.launch_conv_gemm(ref.gemm_desc(vr, m32), _cfg("fast128x64x16w5c"))
    want = torch.einsum("ztc,zcn->ztn", vr.double().cpu(), ref.u.double().cpu()[:, :128, :192])
    ymax = float(want.abs().max())
    e32 = _rel(m32.cpu(), want, ymax)
    first = None
    for t in (None,) + K32 + K16:
        ms.fill_(float("nan"))
        d = layer.gemm_desc(v, ms)
        d.nprod = 1
        ops.launch_conv_gemm(d, -1 if t is None else _cfg(t))
        assert _rel(ms.cpu(), want, ymax) <= 4 * e32 + 2e-6, t
        first = ms.clone() if first is None else first
        assert torch.equal(ms, first), t


def _plain_desc(ops, x, w, out, nprod):
    return ops.conv_gemm_desc(a=x, NB=1, Hi=x.shape[1], Wi=x.shape[2], Cin=x.shape[3], a_strides=(x.stride(0), x.stride(1), x.stride(2)),
                              Ho=x.shape[1], Wo=x.shape[2], sy=1, sx=1, taps=[(0, 0, 0)], pad_mode=ops.PAD_ZERO, w=w, ldw=w.shape[1],
                              Kw=w.shape[0], Nw=w.shape[1], N=w.shape[1], c=ops.tensor_map(out), nprod=nprod)


def test_p1_refusals():
    from manga_image_translator_amd import ops

    x = torch.randn(1, 8, 8, 32, device="cuda")
    out = torch.empty(1, 8, 8, 64, device="cuda")
    w = torch.randn(32, 64, device="cuda")                   # a bare weight: no planes attached
    with pytest.raises(RuntimeError, match="w_split"):
        ops.launch_conv_gemm(_plain_desc(ops, x, w, out, 1))
    ops.register_split(w, force=True)
    ops.launch_conv_gemm(_plain_desc(ops, x, w, out, 1))      # with planes the same launch runs
    for bad in (2, 6, -1):
        d = _plain_desc(ops, x, w, out, 0)
        d.nprod = bad
        with pytest.raises(RuntimeError, match="nprod"):
            ops.launch_conv_gemm(d)
    # a launch that misses the split tiles' preconditions (Cin % 16 != 0) is refused, not run in fp32
    x8 = torch.randn(1, 8, 8, 8, device="cuda")
    w8 = torch.randn(16, 64, device="cuda")
    ops.register_split(w8, force=True)
    with pytest.raises(RuntimeError, match="nprod = 1"):
        ops.launch_conv_gemm(_plain_desc(ops, x8, w8, out, 1))
    with pytest.raises(RuntimeError, match="not a one-product tile"):
        ops.launch_conv_gemm(_plain_desc(ops, x, w, out, 1), _cfg("split128x64x16p6o"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode,tile", [(6, "split128x128x16p6u"), (0, "fast128x128x16w4c")], ids=["split6", "fp32mfma"])
def test_nprod0_is_the_default_path(mode, tile):
    """nprod = 0 launches give the bytes of the default path — the tile the GEMM mode picks — before and after a one-product launch of
    the same layer; and planes attached for a one-product launch to a weight packed in mode 0 are not handed to other launches."""
    from manga_image_translator_amd import ops

    g = torch.Generator().manual_seed(5)
    with ops.gemm_mode(mode):
        layer = ops.Conv2d(torch.randn(128, 32, 1, 1, generator=g) * 0.1, torch.randn(128, generator=g), act=1, device="cuda")
        x = torch.randn(2, 200, 208, 32, generator=g).cuda()       # 650 row tiles x 2: past every under-filled-launch threshold
        want = layer(x, cfg=_cfg(tile))
        a = layer(x)
        b = layer(x, nprod=0)
        p1 = layer(x, nprod=1)
        c = layer(x)
        assert torch.equal(a, want) and torch.equal(b, want) and torch.equal(c, want)
        assert not torch.equal(p1, want)
        d = layer.desc(x, a)
        assert bool(d.w_split) == (mode == 6) and d.nprod == 0
        assert layer.desc(x, a, nprod=1).w_split
    if mode == 0:
        with ops.gemm_mode(6):      # the weight was packed without planes: it stays on the fp32 tiles in every mode
            assert not layer.desc(x, a).w_split
            assert torch.equal(layer(x), want)
