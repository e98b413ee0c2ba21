"""The two kernels the dbconvnext detector adds (csrc/dbconvnext_kernels.hip), through the C-ABI, against torch on the CPU in float64.

Bounds: ``mit_layernorm_rows`` — the output of a LayerNorm is O(|g| + |b|) ~ a few units, float32 has 6e-8 relative precision and the two
D-term sums add at most ~log2(D) roundings in a pairwise order, so 2e-5 absolute on unit-scale rows leaves two orders of headroom over
the rounding and is far below any indexing or stride mistake (which is O(1)).  ``mit_dwconv7_ln_nhwc`` — at most 4x the error of torch's own
float32 ``F.conv2d(groups=C)`` + ``F.layer_norm`` on the same data, plus 1e-6."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WIDTHS = (128, 256, 512, 1024)
SHAPES = [(2, 1, 1), (1, 2, 3), (1, 7, 7), (1, 9, 11), (2, 17, 5), (1, 8, 64)]
EPS = 1e-6


def _L():
    from manga_image_translator_amd import lib, ops

    return lib, lib.load(), C.c_void_p(ops.current_stream())


def _gen(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


# ---- mit_layernorm_rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128, 512, 1024])
@pytest.mark.parametrize("rows", [1, 7, 300])
def test_layernorm_rows(cuda, D, rows):
    lib, L, st = _L()
    lead, tail = 8, 12                                    # the row is a channel slice [lead, lead + D) of a wider buffer, in and out
    src = _gen(rows, lead + D + tail, seed=D + rows, scale=1.7, shift=0.3)
    w, b = _gen(D, seed=1, scale=0.2, shift=1.0), _gen(D, seed=2, scale=0.1)
    ref = F.layer_norm(src[:, lead:lead + D].double(), (D,), w.double(), b.double(), EPS)
    xin = src.to(cuda)
    out = torch.full((rows, tail + D + lead), -7.0, device=cuda)
    wd, bd = w.to(cuda), b.to(cuda)
    lib.check(L.mit_layernorm_rows(xin[:, lead:].data_ptr(), xin.stride(0), wd.data_ptr(), bd.data_ptr(), out[:, tail:].data_ptr(), out.stride(0),
                                   rows, D, EPS, st), "mit_layernorm_rows")
    got = out.cpu()
    err = float((got[:, tail:tail + D].double() - ref).abs().max())
    print(f"layernorm_rows D={D} rows={rows}: max err {err:.3g}")
    assert err <= 2e-5, err
    assert bool((got[:, :tail] == -7.0).all()) and bool((got[:, tail + D:] == -7.0).all())   # nothing outside the slice is written
    # dense rows give the same bits as the slice
    dense_in, dense_out = xin[:, lead:lead + D].contiguous(), torch.empty(rows, D, device=cuda)
    lib.check(L.mit_layernorm_rows(dense_in.data_ptr(), D, wd.data_ptr(), bd.data_ptr(), dense_out.data_ptr(), D, rows, D, EPS, st), "mit_layernorm_rows")
    assert torch.equal(dense_out.cpu(), got[:, tail:tail + D])


def test_layernorm_rows_rejects_unsupported_widths(cuda):
    lib, L, st = _L()
    x = torch.zeros(4, 1032, device=cuda)
    for D in (1028, 1026, 62, 0):
        assert L.mit_layernorm_rows(x.data_ptr(), 1032, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1032, 4, D, EPS, st) != 0, D
        assert b"mit_layernorm_rows" in L.mit_last_error()
    assert L.mit_layernorm_rows(x.data_ptr(), 1030, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1032, 4, 64, EPS, st) != 0


# ---- mit_dwconv7_ln_nhwc ---------------------------------------------------------------------------------------------------------------
def _dw_case(Cc, B, H, W, seed):
    x = _gen(B, H, W, Cc, seed=seed, scale=1.3, shift=0.2)
    w = _gen(Cc, 1, 7, 7, seed=seed + 1, scale=1.0 / 7.0)
    bdw, g, b = _gen(Cc, seed=seed + 2, scale=0.05), _gen(Cc, seed=seed + 3, scale=0.2, shift=1.0), _gen(Cc, seed=seed + 4, scale=0.1)
    return x, w, bdw, g, b


def _dw_ref(x, w, bdw, g, b, dtype):
    y = F.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), bdw.to(dtype), padding=3, groups=x.shape[-1]).permute(0, 2, 3, 1)
    return F.layer_norm(y, (x.shape[-1],), g.to(dtype), b.to(dtype), EPS)


def _dw_fused(cuda, x_dev, w, bdw, g, b, out_dev):
    """x_dev / out_dev: NHWC views on the device whose pixels are uniformly strided (dense, or a channel slice)."""
    lib, L, st = _L()
    B, H, W, Cc = x_dev.shape
    wk = w.reshape(Cc, 49).t().contiguous().to(cuda)
    ops_ = [t.to(cuda) for t in (bdw, g, b)]
    lib.check(L.mit_dwconv7_ln_nhwc(x_dev.data_ptr(), x_dev.stride(2), wk.data_ptr(), ops_[0].data_ptr(), ops_[1].data_ptr(), ops_[2].data_ptr(), EPS,
                                    out_dev.data_ptr(), out_dev.stride(2), B, H, W, Cc, st), "mit_dwconv7_ln_nhwc")
    return out_dev


def _dw_two_launch(cuda, x_dev, w, bdw, g, b):
    lib, L, st = _L()
    B, H, W, Cc = x_dev.shape
    wk = w.reshape(Cc, 49).t().contiguous().to(cuda)
    one, bd, gd, be = torch.ones(Cc, device=cuda), bdw.to(cuda), g.to(cuda), b.to(cuda)
    mid, out = torch.empty(B, H, W, Cc, device=cuda), torch.empty(B, H, W, Cc, device=cuda)
    lib.check(L.mit_dwconv_nhwc(x_dev.data_ptr(), wk.data_ptr(), one.data_ptr(), bd.data_ptr(), mid.data_ptr(), B, H, W, Cc, 7, st), "mit_dwconv_nhwc")
    lib.check(L.mit_layernorm_rows(mid.data_ptr(), Cc, gd.data_ptr(), be.data_ptr(), out.data_ptr(), Cc, B * H * W, Cc, EPS, st), "mit_layernorm_rows")
    return out


@pytest.mark.parametrize("Cc", WIDTHS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_dwconv7_ln(cuda, Cc, B, H, W):
    x, w, bdw, g, b = _dw_case(Cc, B, H, W, seed=Cc + 31 * H + W)
    ref64 = _dw_ref(x, w, bdw, g, b, torch.float64)
    bound = 4.0 * float((_dw_ref(x, w, bdw, g, b, torch.float32).double() - ref64).abs().max()) + 1e-6
    xd = x.to(cuda)
    got = _dw_fused(cuda, xd, w, bdw, g, b, torch.empty(B, H, W, Cc, device=cuda))
    err = float((got.cpu().double() - ref64).abs().max())
    print(f"dwconv7_ln C={Cc} {B}x{H}x{W}: err {err:.3g} bound {bound:.3g}")
    assert err <= bound, (err, bound)
    # an image's result does not depend on the batch it is in
    last = _dw_fused(cuda, xd[B - 1:].contiguous(), w, bdw, g, b, torch.empty(1, H, W, Cc, device=cuda))
    assert torch.equal(last[0], got[B - 1])
    # the one-pass form against the two launches it replaces, under the same bound
    _, L, _ = _L()
    two = _dw_two_launch(cuda, xd, w, bdw, g, b)
    err2 = float((two.cpu().double() - ref64).abs().max())
    print(f"   two-launch err {err2:.3g}; fused at this width: {bool(L.mit_dwconv7_ln_supported(Cc))}")
    assert err2 <= bound, (err2, bound)


def test_dwconv7_ln_reads_and_writes_channel_slices(cuda):
    """C = 128 as the upper half of a 256-wide input buffer, written into the lower half of a 256-wide output buffer."""
    B, H, W, Cc = 1, 9, 11, 128
    x, w, bdw, g, b = _dw_case(Cc, B, H, W, seed=77)
    ref64 = _dw_ref(x, w, bdw, g, b, torch.float64)
    bound = 4.0 * float((_dw_ref(x, w, bdw, g, b, torch.float32).double() - ref64).abs().max()) + 1e-6
    wide_in = torch.full((B, H, W, 256), 1e30, device=cuda)     # a read outside the slice would wreck the result
    wide_in[..., 128:] = x.to(cuda)
    wide_out = torch.full((B, H, W, 256), -7.0, device=cuda)
    _dw_fused(cuda, wide_in[..., 128:], w, bdw, g, b, wide_out[..., :128])
    got = wide_out.cpu()
    err = float((got[..., :128].double() - ref64).abs().max())
    assert err <= bound, (err, bound)
    assert bool((got[..., 128:] == -7.0).all())
    dense = _dw_fused(cuda, x.to(cuda), w, bdw, g, b, torch.empty(B, H, W, Cc, device=cuda))
    assert torch.equal(dense.cpu(), got[..., :128])


def test_dwconv7_ln_rejects_other_widths(cuda):
    _, L, st = _L()
    x = torch.zeros(1, 4, 4, 96, device=cuda)
    assert L.mit_dwconv7_ln_supported(96) == 0 and L.mit_dwconv7_ln_supported(80) == 0
    assert L.mit_dwconv7_ln_nhwc(x.data_ptr(), 96, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), EPS, x.data_ptr(), 96, 1, 4, 4, 96, st) != 0
    assert b"128, 256, 512 or 1024" in L.mit_last_error()
    assert L.mit_dwconv7_ln_nhwc(x.data_ptr(), 64, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), EPS, x.data_ptr(), 128, 1, 4, 4, 128, st) != 0
