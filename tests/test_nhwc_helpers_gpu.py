"""The small memory-bound NHWC helpers (csrc/ctd_kernels.hip, the helper section of csrc/ocr_kernels.hip), each through the C-ABI against
a plain CPU reference at the shapes the engines never show them: images smaller than the window, odd sizes, several windows and
strides, channel slices of wider buffers.

Layout rules of every test whose entry takes pixel strides: the input is the channel slice [lead, lead + C) of a buffer whose pixels
are C + 12 floats apart (1e30 around the slice: a read outside it wrecks the result), the output a slice of another such buffer
pre-filled with a sentinel that must survive everywhere outside the slice, and one dense call must give the slice's bits.  Leads are 4
or 8 floats, so every pointer is 16-byte aligned.  The entries without stride arguments (mit_maxpool2d_nhwc, mit_avgpool_nhwc,
mit_dwconv_nhwc) run dense, with a sentinel tail behind the output.

Bounds (u = 2^-24, the unit roundoff of fp32; every reference is float64 on the fp32 inputs):
  max pools, copy             bitwise: max and copy are exact.
  mit_avgpool2_nhwc           3 adds and one exact x 0.25:                 |err| <= 3 u sum|x| / 4
  mit_avgpool_nhwc            taps adds, one product with the rounded 1 / (kh kw):  |err| <= (taps + 1) u sum|x| / (kh kw)
  mit_affine_act_nhwc, axpy   one product, one sum (or one fma):           |err| <= 2 u (|x s| + |b|)
  mit_dwconv_nhwc             the elementwise bound of test_conv_gemm_gpu.py: 2e-6 mag + 1e-6, mag = the expression on absolute values
  mit_layernorm               2e-5 absolute on unit-scale rows (derivation: test_dbconvnext_kernels_gpu.py)
  mit_sigmoid_inplace         one expf, one add, one divide, ~5 ulp worst case, headroom for a non-IEEE divide: |err| <= 8 u |ref|
  mit_gelu_inplace            a <= 2 ulp erff of magnitude <= 1, one add, two products, ~4 u |x|; twice that:   |err| <= 8 u |x|
  mit_xpos_rotate             cos sc and sin sc rounded, then two products and a sum:  |err| <= 4 u (|x| + |y|) |sc|
Each toleranced test prints its largest err / bound."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXTRA = 12          # floats between the channel slices of neighbouring pixels
BIG, SENT = 1e30, -7.0


def _L():
    from manga_image_translator_amd import lib, ops

    return lib, lib.load(), C.c_void_p(ops.current_stream())


def _gen(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def _wide_in(x, lead, cuda):
    """x [..., C] on the CPU -> (buffer, slice view) on the device; the buffer is [..., C + EXTRA], 1e30 outside the slice."""
    Cc = x.shape[-1]
    buf = torch.full((*x.shape[:-1], Cc + EXTRA), BIG, device=cuda)
    buf[..., lead:lead + Cc] = x.to(cuda)
    return buf, buf[..., lead:lead + Cc]


def _wide_out(shape, lead, cuda, extra=EXTRA):
    Cc = shape[-1]
    buf = torch.full((*shape[:-1], Cc + extra), SENT, device=cuda)
    return buf, buf[..., lead:lead + Cc]


def _untouched_outside(buf, lead, Cc):
    got = buf.cpu()
    return bool((got[..., :lead] == SENT).all()) and bool((got[..., lead + Cc:] == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _with_neg_inf(x, seed):
    g = torch.Generator().manual_seed(seed)
    x = x.clone()
    x[torch.rand(x.shape, generator=g) < 0.15] = float("-inf")
    return x


def _ratio(name, err, bound):
    """Largest err / bound (0 / 0 counts as 0), printed, returned."""
    r = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(r.max())
    print(f"{name}: max err/bound {worst:.3f}")
    return worst


# ---- mit_maxpool_nhwc: k x k, stride 1, pad k / 2 --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("B,H,W,Cc", [(2, 1, 1, 4), (1, 2, 7, 8), (1, 5, 3, 12), (1, 9, 11, 64)])
def test_maxpool_same(cuda, k, B, H, W, Cc):
    lib, L, st = _L()
    x = _with_neg_inf(_gen(B, H, W, Cc, seed=100 * k + H + W), seed=k + Cc)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), k, 1, k // 2).permute(0, 2, 3, 1)
    ibuf, iv = _wide_in(x, 4, cuda)
    obuf, ov = _wide_out((B, H, W, Cc), 8, cuda)
    lib.check(L.mit_maxpool_nhwc(iv.data_ptr(), iv.stride(2), ov.data_ptr(), ov.stride(2), B, H, W, Cc, k, st), "mit_maxpool_nhwc")
    assert _same_bits(ov, ref)
    assert _untouched_outside(obuf, 8, Cc)
    dense = torch.full((B, H, W, Cc), SENT, device=cuda)
    xdev = x.to(cuda)
    lib.check(L.mit_maxpool_nhwc(xdev.data_ptr(), Cc, dense.data_ptr(), Cc, B, H, W, Cc, k, st), "mit_maxpool_nhwc")
    assert _same_bits(dense, ov)


# ---- mit_maxpool2d_nhwc: k x k, stride s, pad p, floor mode ----------------------------------------------------------------------
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), (3, 1, 1), (5, 3, 2)])
@pytest.mark.parametrize("H,W", [(1, 1), (7, 10), (8, 8), (9, 5)])
@pytest.mark.parametrize("Cc", [4, 64])
def test_maxpool2d(cuda, k, s, p, H, W, Cc):
    lib, L, st = _L()
    B = 2
    if H == 1 and p == 0:   # a 2 x 2 window does not fit a 1 x 1 image: torch refuses it, and so must the entry (before any launch)
        assert L.mit_maxpool2d_nhwc(4096, 8192, B, H, W, Cc, k, s, p, st) != 0
        assert b"empty output" in L.mit_last_error()
        return
    x = _with_neg_inf(_gen(B, H, W, Cc, seed=1000 * k + 10 * H + W), seed=s + Cc)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = ref.shape[1:3]
    n = ref.numel()
    out = torch.full((n + 64,), SENT, device=cuda)
    xdev = x.to(cuda)
    lib.check(L.mit_maxpool2d_nhwc(xdev.data_ptr(), out.data_ptr(), B, H, W, Cc, k, s, p, st), "mit_maxpool2d_nhwc")
    assert _same_bits(out[:n].view(B, Ho, Wo, Cc), ref)
    assert bool((out[n:] == SENT).all())


# ---- mit_avgpool2_nhwc: 2 x 2, stride 2 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ho,Wo", [(1, 1), (3, 5), (8, 2)])
@pytest.mark.parametrize("Cc", [4, 40])
def test_avgpool2(cuda, Ho, Wo, Cc):
    lib, L, st = _L()
    B = 2
    x = _gen(B, 2 * Ho, 2 * Wo, Cc, seed=Ho * 10 + Wo + Cc, scale=1.3, shift=0.4)
    xd = x.double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(xd, 2, 2).permute(0, 2, 3, 1)
    bound = 3 * U * F.avg_pool2d(xd.abs(), 2, 2).permute(0, 2, 3, 1)      # 3 u sum|x| / 4
    ibuf, iv = _wide_in(x, 8, cuda)
    obuf, ov = _wide_out((B, Ho, Wo, Cc), 4, cuda)
    lib.check(L.mit_avgpool2_nhwc(iv.data_ptr(), iv.stride(2), ov.data_ptr(), ov.stride(2), B, Ho, Wo, Cc, st), "mit_avgpool2_nhwc")
    err = (ov.cpu().double() - ref).abs()
    _ratio(f"avgpool2 {Ho}x{Wo} C={Cc}", err, bound)
    assert bool((err <= bound).all()), float((err - bound).max())
    assert _untouched_outside(obuf, 4, Cc)
    dense = torch.full((B, Ho, Wo, Cc), SENT, device=cuda)
    xdev = x.to(cuda)
    lib.check(L.mit_avgpool2_nhwc(xdev.data_ptr(), Cc, dense.data_ptr(), Cc, B, Ho, Wo, Cc, st), "mit_avgpool2_nhwc")
    assert _same_bits(dense, ov)


# ---- mit_avgpool_nhwc: general window, count_include_pad -------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2, 2, 2, 1, 0, 1), (2, 2, 2, 2, 0, 0), (3, 3, 1, 1, 1, 1), (3, 2, 2, 1, 1, 0)], ids=lambda g: "k%dx%d-s%dx%d-p%dx%d" % g)
@pytest.mark.parametrize("H,W", [(2, 1), (6, 33), (7, 5)])
def test_avgpool_general(cuda, geom, H, W):
    lib, L, st = _L()
    kh, kw, sh, sw, ph, pw = geom
    B, Cc = 2, 8
    if H + 2 * ph < kh or W + 2 * pw < kw:   # the window does not fit: torch refuses it, and so must the entry (before any launch)
        assert L.mit_avgpool_nhwc(4096, 8192, B, H, W, Cc, kh, kw, sh, sw, ph, pw, st) != 0
        assert b"empty output" in L.mit_last_error()
        return
    x = _gen(B, H, W, Cc, seed=H * 100 + W + kh * 7 + sw, scale=1.3, shift=0.4)
    xd = x.double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(xd, (kh, kw), (sh, sw), (ph, pw), count_include_pad=True).permute(0, 2, 3, 1).contiguous()
    bound = (kh * kw + 1) * U * F.avg_pool2d(xd.abs(), (kh, kw), (sh, sw), (ph, pw), count_include_pad=True).permute(0, 2, 3, 1)
    Ho, Wo = ref.shape[1:3]
    n = ref.numel()
    out = torch.full((n + 64,), SENT, device=cuda)
    xdev = x.to(cuda)
    lib.check(L.mit_avgpool_nhwc(xdev.data_ptr(), out.data_ptr(), B, H, W, Cc, kh, kw, sh, sw, ph, pw, st), "mit_avgpool_nhwc")
    err = (out[:n].view(B, Ho, Wo, Cc).cpu().double() - ref).abs()
    _ratio(f"avgpool {geom} {H}x{W}", err, bound)
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((out[n:] == SENT).all())


# ---- mit_copy_channels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [1, 37])
@pytest.mark.parametrize("Cc", [4, 128])
def test_copy_channels(cuda, npix, Cc):
    lib, L, st = _L()
    x = _gen(npix, Cc, seed=npix + Cc)
    ibuf, iv = _wide_in(x, 4, cuda)                          # pixel stride C + 12
    obuf, ov = _wide_out((npix, Cc), 8, cuda, extra=20)      # pixel stride C + 20
    lib.check(L.mit_copy_channels(iv.data_ptr(), iv.stride(0), ov.data_ptr(), ov.stride(0), npix, Cc, st), "mit_copy_channels")
    assert _same_bits(ov, x)
    assert _untouched_outside(obuf, 8, Cc)
    dense = torch.full((npix, Cc), SENT, device=cuda)
    xdev = x.to(cuda)
    lib.check(L.mit_copy_channels(xdev.data_ptr(), Cc, dense.data_ptr(), Cc, npix, Cc, st), "mit_copy_channels")
    assert _same_bits(dense, ov)


# ---- mit_affine_act_nhwc ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("npix", [1, 37])
@pytest.mark.parametrize("Cc", [4, 64])
def test_affine_act(cuda, relu, npix, Cc):
    lib, L, st = _L()
    x = _gen(npix, Cc, seed=npix + Cc + relu, scale=1.5)
    s, b = _gen(Cc, seed=3, scale=0.4, shift=1.0), _gen(Cc, seed=4, scale=0.8)
    ref = x.double() * s.double() + b.double()
    bound = 2 * U * ((x.double() * s.double()).abs() + b.double().abs())
    if relu:
        ref = ref.clamp_min(0.0)                             # 1-Lipschitz: the bound carries over
    sd, bd = s.to(cuda), b.to(cuda)
    ibuf, iv = _wide_in(x, 8, cuda)
    obuf, ov = _wide_out((npix, Cc), 4, cuda)
    lib.check(L.mit_affine_act_nhwc(iv.data_ptr(), iv.stride(0), sd.data_ptr(), bd.data_ptr(), ov.data_ptr(), ov.stride(0), npix, Cc, relu, st),
              "mit_affine_act_nhwc")
    got = ov.cpu()
    err = (got.double() - ref).abs()
    _ratio(f"affine_act relu={relu} npix={npix} C={Cc}", err, bound)
    assert bool((err <= bound).all()), float((err - bound).max())
    if relu:
        assert bool((got >= 0).all())
    assert _untouched_outside(obuf, 4, Cc)
    dense = torch.full((npix, Cc), SENT, device=cuda)
    xdev = x.to(cuda)
    lib.check(L.mit_affine_act_nhwc(xdev.data_ptr(), Cc, sd.data_ptr(), bd.data_ptr(), dense.data_ptr(), Cc, npix, Cc, relu, st), "mit_affine_act_nhwc")
    assert _same_bits(dense, ov)


# ---- mit_axpy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028])
@pytest.mark.parametrize("a", [0.2, -1.0])
def test_axpy(cuda, n, a):
    lib, L, st = _L()
    x, y = _gen(n, seed=n, scale=1.5), _gen(n, seed=n + 1, scale=0.8, shift=0.1)
    a32 = float(np.float32(a))                               # what the float argument carries
    ref = a32 * x.double() + y.double()
    bound = 2 * U * ((a32 * x.double()).abs() + y.double().abs())
    out = torch.full((n + 16,), SENT, device=cuda)
    xd, yd = x.to(cuda), y.to(cuda)
    lib.check(L.mit_axpy(out.data_ptr(), a, xd.data_ptr(), yd.data_ptr(), n, st), "mit_axpy")
    err = (out[:n].cpu().double() - ref).abs()
    _ratio(f"axpy n={n} a={a}", err, bound)
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((out[n:] == SENT).all())


# ---- mit_dwconv_nhwc (dense form) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("B,H,W,Cc", [(1, 1, 2, 4), (2, 3, 9, 16), (1, 8, 5, 80)])
def test_dwconv_dense(cuda, k, B, H, W, Cc):
    lib, L, st = _L()
    x = _gen(B, H, W, Cc, seed=k * 100 + H + W, scale=1.3, shift=0.2)
    w = _gen(Cc, 1, k, k, seed=k, scale=1.0 / k)
    sc, bi = _gen(Cc, seed=5, scale=0.3, shift=1.0), _gen(Cc, seed=6, scale=0.5)
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    cv = lambda a, b: F.conv2d(a, b, None, padding=k // 2, groups=Cc).permute(0, 2, 3, 1)
    ref = cv(xd, wd) * sc.double() + bi.double()
    mag = cv(xd.abs(), wd.abs()) * sc.double().abs() + bi.double().abs()
    bound = 2e-6 * mag + 1e-6
    wk = w.reshape(Cc, k * k).t().contiguous().to(cuda)       # [k*k][C]
    n = B * H * W * Cc
    out = torch.full((n + 64,), SENT, device=cuda)
    xdev, scd, bid = x.to(cuda), sc.to(cuda), bi.to(cuda)
    lib.check(L.mit_dwconv_nhwc(xdev.data_ptr(), wk.data_ptr(), scd.data_ptr(), bid.data_ptr(), out.data_ptr(), B, H, W, Cc, k, st), "mit_dwconv_nhwc")
    err = (out[:n].view(B, H, W, Cc).cpu().double() - ref).abs()
    _ratio(f"dwconv k={k} {B}x{H}x{W}x{Cc}", err, bound)
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((out[n:] == SENT).all())


# ---- mit_layernorm: one wave per row, 4 rows per workgroup (5 and 9 rows leave a ragged last group) -------------------------------
@pytest.mark.parametrize("D", [8, 40, 64, 65, 300, 320, 512])
@pytest.mark.parametrize("rows", [1, 5, 9])
def test_layernorm(cuda, D, rows):
    lib, L, st = _L()
    lead, tail, eps = 8, 12, 1e-5
    src = _gen(rows, lead + D + tail, seed=D + rows, scale=1.7, shift=0.3)
    w, b = _gen(D, seed=1, scale=0.2, shift=1.0), _gen(D, seed=2, scale=0.1)
    ref = F.layer_norm(src[:, lead:lead + D].double(), (D,), w.double(), b.double(), eps)
    xin = src.to(cuda)
    out = torch.full((rows, tail + D + lead), SENT, device=cuda)
    wd, bd = w.to(cuda), b.to(cuda)
    lib.check(L.mit_layernorm(xin[:, lead:].data_ptr(), xin.stride(0), wd.data_ptr(), bd.data_ptr(), out[:, tail:].data_ptr(), out.stride(0), rows, D, eps, st),
              "mit_layernorm")
    got = out.cpu()
    err = float((got[:, tail:tail + D].double() - ref).abs().max())
    print(f"layernorm D={D} rows={rows}: max err {err:.3g}, err/bound {err / 2e-5:.3f}")
    assert err <= 2e-5, err
    assert bool((got[:, :tail] == SENT).all()) and bool((got[:, tail + D:] == SENT).all())
    dense_in, dense_out = xin[:, lead:lead + D].contiguous(), torch.empty(rows, D, device=cuda)
    lib.check(L.mit_layernorm(dense_in.data_ptr(), D, wd.data_ptr(), bd.data_ptr(), dense_out.data_ptr(), D, rows, D, eps, st), "mit_layernorm")
    assert _same_bits(dense_out, got[:, tail:tail + D])


# ---- mit_sigmoid_inplace / mit_gelu_inplace --------------------------------------------------------------------------------------
def test_sigmoid(cuda):
    lib, L, st = _L()
    inf = float("inf")
    x = torch.cat([torch.linspace(-80.0, 80.0, 4096), torch.tensor([0.0, -0.0, inf, -inf])])
    n = x.numel()
    ref = 1.0 / (1.0 + torch.exp(-x.double()))
    buf = torch.full((n + 16,), SENT, device=cuda)
    buf[:n] = x.to(cuda)
    lib.check(L.mit_sigmoid_inplace(buf.data_ptr(), n, st), "mit_sigmoid_inplace")
    got = buf.cpu()
    err, bound = (got[:n].double() - ref).abs(), 8 * U * ref.abs()
    worst = _ratio("sigmoid", err, bound)
    assert bool((err <= bound).all()), worst
    assert got[n - 2].item() == 1.0 and got[n - 1].item() == 0.0          # +inf, -inf: exactly 1 and 0
    assert got[n - 4].item() == 0.5 and got[n - 3].item() == 0.5          # 0, -0
    assert bool((got[n:] == SENT).all())


def test_gelu(cuda):
    lib, L, st = _L()
    x = torch.cat([torch.linspace(-12.0, 12.0, 4096), torch.tensor([0.0, 1e4, -1e4])])
    n = x.numel()
    xd = x.double()
    ref = 0.5 * xd * (1.0 + torch.erf(xd / 2.0 ** 0.5))
    buf = torch.full((n + 16,), SENT, device=cuda)
    buf[:n] = x.to(cuda)
    lib.check(L.mit_gelu_inplace(buf.data_ptr(), n, st), "mit_gelu_inplace")
    got = buf.cpu()
    err, bound = (got[:n].double() - ref).abs(), 8 * U * xd.abs()
    worst = _ratio("gelu", err, bound)
    assert bool((err <= bound).all()), worst
    assert got[n - 3].item() == 0.0 and got[n - 2].item() == 1e4 and got[n - 1].item() == 0.0
    assert bool((got[n:] == SENT).all())


# ---- mit_xpos_rotate -------------------------------------------------------------------------------------------------------------
_XPOS = {}


def _xpos(cuda):
    """Tables from a random scale vector, filled into a MitXposTables as Ocr48Engine.__init__ does (no engine needed)."""
    if not _XPOS:
        from manga_image_translator_amd import lib, ocr48

        sv = torch.rand(40, generator=torch.Generator().manual_seed(11)) * 0.7 + 0.3
        tables = ocr48.xpos_tables(sv, cuda)
        tb = lib.MitXposTables()
        tb.cos_t, tb.sin_t = tables["cos"].data_ptr(), tables["sin"].data_ptr()
        tb.scale_t, tb.iscale_t = tables["scale"].data_ptr(), tables["iscale"].data_ptr()
        tb.imax, tb.pmax = ocr48.XPOS_IMAX, ocr48.XPOS_PMAX
        _XPOS.update(dev=tables, tb=tb, cpu={k: v.cpu().double() for k, v in tables.items()}, imax=ocr48.XPOS_IMAX, pmax=ocr48.XPOS_PMAX)
        assert tables["cos"].shape == (ocr48.XPOS_IMAX, 40) and tables["scale"].shape == (2 * ocr48.XPOS_PMAX, 40)
    return _XPOS


def _xpos_check(cuda, R, T, i0, p0, downscale):
    lib, L, st = _L()
    X = _xpos(cuda)
    qkv = _gen(R, T, 960, seed=R * 1000 + T + i0, scale=1.2)                # q | k | v as the encoder's fused projection leaves them
    x = qkv[..., :320].double().reshape(R, T, 4, 40, 2)                     # 4 heads x 40 (x, y) pairs
    t = torch.arange(T)
    cos, sin = X["cpu"]["cos"][i0 + t], X["cpu"]["sin"][i0 + t]             # [T, 40], the fp32 entries in float64
    sc = X["cpu"]["iscale" if downscale else "scale"][p0 + t + X["pmax"]]
    c, s = (cos * sc)[None, :, None, :], (sin * sc)[None, :, None, :]
    xx, yy = x[..., 0], x[..., 1]
    ref = torch.stack([xx * c - yy * s, yy * c + xx * s], -1).reshape(R, T, 320)
    mag = (xx.abs() + yy.abs()) * sc.abs()[None, :, None, :]
    bound = (4 * U * mag)[..., None].expand(R, T, 4, 40, 2).reshape(R, T, 320)
    src = qkv.to(cuda)
    obuf, ov = _wide_out((R, T, 320), 4, cuda)
    lib.check(L.mit_xpos_rotate(src.data_ptr(), src.stride(0), src.stride(1), ov.data_ptr(), ov.stride(0), ov.stride(1), R, T, i0, p0, int(downscale),
                                C.byref(X["tb"]), st), "mit_xpos_rotate")
    err = (ov.cpu().double() - ref).abs()
    _ratio(f"xpos R={R} T={T} i0={i0} p0={p0} down={downscale}", err, bound)
    assert bool((err <= bound).all()), float((err - bound).max())
    assert _untouched_outside(obuf, 4, 320)
    dense_in, dense = src[..., :320].contiguous(), torch.full((R, T, 320), SENT, device=cuda)
    lib.check(L.mit_xpos_rotate(dense_in.data_ptr(), T * 320, 320, dense.data_ptr(), T * 320, 320, R, T, i0, p0, int(downscale), C.byref(X["tb"]), st),
              "mit_xpos_rotate")
    assert _same_bits(dense, ov)


@pytest.mark.parametrize("downscale", [False, True])
@pytest.mark.parametrize("engine_positions", [True, False])
@pytest.mark.parametrize("T", [1, 7, 70])
@pytest.mark.parametrize("R", [1, 3])
def test_xpos_rotate(cuda, R, T, engine_positions, downscale):
    i0, p0 = (0, -T // 2) if engine_positions else (5, -3)
    _xpos_check(cuda, R, T, i0, p0, downscale)


@pytest.mark.parametrize("edge", ["i0+T==imax", "p0==-pmax", "p0+T-1==pmax-1"])
@pytest.mark.parametrize("downscale", [False, True])
def test_xpos_rotate_on_the_table_edges(cuda, edge, downscale):
    """The last cos / sin row, the first and the last scale row: accepted, and as accurate as any other."""
    X = _xpos(cuda)
    T = 7
    i0, p0 = {"i0+T==imax": (X["imax"] - T, -3), "p0==-pmax": (0, -X["pmax"]), "p0+T-1==pmax-1": (0, X["pmax"] - T)}[edge]
    _xpos_check(cuda, 2, T, i0, p0, downscale)


# ---- the grid cap ----------------------------------------------------------------------------------------------------------------
def test_grid_cap_stride_loop(cuda):
    """grid_for caps a launch at 4096 workgroups of 256 threads; the kernels loop over the rest.  With 4096 * 256 + 77 work items the last
    77 are reached only by the second trip of that loop."""
    lib, L, st = _L()
    n = 4096 * 256 + 77
    g = torch.Generator().manual_seed(5)
    v = torch.rand(n, generator=g) * 1.2 - 0.1                             # some below 0, some above 1: mode 2 clips
    ref = (np.clip(v.numpy(), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.int32).astype(np.uint8)
    out = torch.full((n + 64,), 7, dtype=torch.uint8, device=cuda)
    vd = v.to(cuda)
    lib.check(L.mit_map_to_u8(vd.data_ptr(), out.data_ptr(), n, 2, 0.0, st), "mit_map_to_u8")
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], ref), int((got[:n] != ref).sum())
    assert len(set(ref[-77:].tolist())) > 8 and (got[n:] == 7).all()
    del vd, out
    x = torch.randn(n, 4, generator=g)
    xd = x.to(cuda)
    dst = torch.full((n + 16, 4), SENT, device=cuda)
    lib.check(L.mit_copy_channels(xd.data_ptr(), 4, dst.data_ptr(), 4, n, 4, st), "mit_copy_channels")
    assert torch.equal(dst[:n], xd) and bool((dst[n:] == SENT).all())
    assert _same_bits(dst[n - 77:n], x[n - 77:])
