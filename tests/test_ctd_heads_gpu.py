"""``mit_convt_cout1`` (ConvTranspose2d(Cin -> 1, stride 2) in one pass, over a given output extent) against the four parity launches
of ``ops.ConvTranspose2d`` — bit for bit — and ``CtdEngine()`` against ``CtdEngine(fused_heads=False)``.

The shapes are the smallest at which the kernel can go wrong: every border case of the 2 x 2 neighbourhood, extents that cut a 2 x 2
output block, more than one strip of input positions with a partial last strip, more than one row block, strided views."""
import ctypes as C

import numpy as np
import pytest
import torch

from manga_image_translator_amd import lib as L

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
STRIP = {4: L.MIT_CONVT_COUT1_STRIP_K4, 2: L.MIT_CONVT_COUT1_STRIP_K2}    # input positions per workgroup along a row (include/mit_hip.h)
ROWS = {4: 16, 2: 8}        # rows of input positions a workgroup walks (csrc/convt_cout1.hip)


def make_layer(cuda, k, seed, bias=False, act=None):
    from manga_image_translator_amd import ops

    cin, pad = (64, 1) if k == 4 else (16, 0)
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cin, 1, k, k, generator=g) / (cin * k * k / 4) ** 0.5
    b = torch.randn(1, generator=g) * 0.1 if bias else None
    layer = ops.ConvTranspose2d(w, b, stride=2, padding=pad, act=ops.ACT_SIGMOID if act is None else act, device=cuda)
    assert layer.one_pass
    return layer, w, b, g


def check(layer, x, out_view_of, out_h=None, out_w=None):
    """``out_view_of(B, Ho, Wo)`` -> (buffer, [B, Ho, Wo, 1] view of it).  The four-launch form fills one such view completely; the
    single pass must give the same bits inside the extent and leave everything else of its (sentinel-filled) buffer alone."""
    B, H, W, _ = x.shape
    ref_buf, ref = out_view_of(B, 2 * H, 2 * W)
    layer(x, out=ref)
    got_buf, got = out_view_of(B, 2 * H, 2 * W)
    layer.single_pass(x, got, out_h, out_w)
    torch.cuda.synchronize()
    h, w = 2 * H if out_h is None else out_h, 2 * W if out_w is None else out_w
    assert torch.equal(got[:, :h, :w], ref[:, :h, :w])
    assert not torch.any(ref[:, :h, :w] == SENTINEL)
    inside = torch.zeros_like(got_buf, dtype=torch.bool)
    inside_view = inside.as_strided(got.shape, got.stride(), got.storage_offset() - got_buf.storage_offset())
    inside_view[:, :h, :w] = True
    assert torch.all(got_buf[~inside] == SENTINEL), "wrote outside the extent"


def dense_out(cuda):
    def make(B, Ho, Wo):
        buf = torch.full((B, Ho, Wo, 1), SENTINEL, device=cuda)
        return buf, buf
    return make


def test_k4_full_extent_every_border(cuda):
    layer, _, _, g = make_layer(cuda, 4, 1)
    check(layer, torch.randn(2, 5, 7, 64, generator=g).to(cuda), dense_out(cuda))


def test_k4_odd_extent_cuts_a_block(cuda):
    layer, _, _, g = make_layer(cuda, 4, 2)
    check(layer, torch.randn(2, 5, 7, 64, generator=g).to(cuda), dense_out(cuda), 7, 9)


def test_k2_bias_sigmoid_extent(cuda):
    layer, _, _, g = make_layer(cuda, 2, 3, bias=True)
    check(layer, torch.randn(2, 6, 5, 16, generator=g).to(cuda), dense_out(cuda), 11, 7)


@pytest.mark.parametrize("k", [4, 2])
@pytest.mark.parametrize("cut", [False, True])
def test_strip_boundary_and_partial_last_strip(cuda, k, cut):
    layer, _, _, g = make_layer(cuda, k, 4 + k, bias=True)
    W = STRIP[k] + 3
    x = torch.randn(1, 3, W, 64 if k == 4 else 16, generator=g).to(cuda)
    check(layer, x, dense_out(cuda), *((5, 2 * STRIP[k] + 1) if cut else (None, None)))


@pytest.mark.parametrize("k", [4, 2])
def test_row_block_boundary(cuda, k):
    """More rows than one workgroup walks: the row carried in registers and the row requested ahead cross a block boundary."""
    layer, _, _, g = make_layer(cuda, k, 8 + k)
    H = ROWS[k] + 2
    check(layer, torch.randn(1, H, 3, 64 if k == 4 else 16, generator=g).to(cuda), dense_out(cuda), 2 * H - 1, 5)


@pytest.mark.parametrize("k", [4, 2])
def test_strided_views(cuda, k):
    """x as a channel slice of a wider buffer, out as plane 1 of [B, 2, H, W] (what ``lines[:, plane]`` is)."""
    layer, _, _, g = make_layer(cuda, k, 12 + k, bias=True)
    cin = 64 if k == 4 else 16
    wide = torch.randn(2, 6, 5, cin + 32, generator=g).to(cuda)
    x = wide[..., 16:16 + cin]
    assert not x.is_contiguous()

    def planes(B, Ho, Wo):
        buf = torch.full((B, 2, Ho, Wo), SENTINEL, device=cuda)
        return buf, buf[:, 1].unsqueeze(-1)

    check(layer, x, planes, 11, 9)


def test_against_torch_on_the_cpu(cuda):
    """One case against torch.nn.functional.conv_transpose2d in float64, with the bound of the ConvTranspose2d comparison in
    tests/test_conv_gemm_gpu.py (2e-6 of the magnitude sum + 1e-6)."""
    import torch.nn.functional as F

    from manga_image_translator_amd import ops

    for k in (4, 2):
        layer, w, b, g = make_layer(cuda, k, 20 + k, bias=True, act=ops.ACT_NONE)
        x = torch.randn(2, 64 if k == 4 else 16, 6, 9, generator=g)
        out = torch.full((2, 12, 18, 1), SENTINEL, device=cuda)
        layer.single_pass(x.permute(0, 2, 3, 1).contiguous().to(cuda), out)
        torch.cuda.synchronize()
        pad = 1 if k == 4 else 0
        ref = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=pad)
        mag = F.conv_transpose2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=pad)
        got = out.cpu().permute(0, 3, 1, 2).double()
        assert got.shape == ref.shape
        worst = ((got - ref).abs() / (2e-6 * mag + 1e-6)).max().item()
        assert worst <= 1.0, f"k{k}: max err/bound = {worst:.3f}"


def test_other_forms_are_refused(cuda):
    from manga_image_translator_amd import lib as L, ops

    w3 = ops.ConvTranspose2d(torch.randn(16, 1, 3, 3), None, stride=2, padding=1, output_padding=1, device=cuda)
    assert not w3.one_pass and not ops.ConvTranspose2d(torch.randn(32, 1, 4, 4), None, stride=2, padding=1, device=cuda).one_pass
    with pytest.raises(ValueError):
        w3.single_pass(torch.zeros(1, 4, 4, 16, device=cuda), torch.zeros(1, 8, 8, 1, device=cuda))
    lib = L.load()
    x, w, o = torch.zeros(1, 4, 4, 32, device=cuda), torch.zeros(32, 1, 4, 4, device=cuda), torch.zeros(1, 8, 8, 1, device=cuda)
    args = lambda cin, k, s, p, oh: (x.data_ptr(), 512, 128, 32, 1, 4, 4, cin, w.data_ptr(), k, s, p, None, None, 0, 0.0, o.data_ptr(), 64, 8, 1, oh, 8, None)
    assert lib.mit_convt_cout1(*args(32, 4, 2, 1, 8)) != 0 and b"only k4 s2 p1" in lib.mit_last_error()
    assert lib.mit_convt_cout1(*args(64, 4, 2, 0, 8)) != 0 and b"only k4 s2 p1" in lib.mit_last_error()
    assert lib.mit_convt_cout1(*args(64, 4, 2, 1, 9)) != 0 and b"not inside" in lib.mit_last_error()


# ---- engine level ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engines(cuda, shipped_mode):
    from manga_image_translator_amd import ctd, ctd_schema as S, synth

    g = S.CTD_GAIN
    sds = [synth.synth_state_dict(sch, seed=0, gain=g) for sch in (S.yolo_schema(), S.unet_head_schema(), S.db_head_schema())]
    with shipped_mode():
        return ctd.CtdEngine(*sds, device=cuda), ctd.CtdEngine(*sds, device=cuda, fused_heads=False)


def gemv_launches(fn):
    """Run ``fn`` under the launch probe -> (its result, launches on the gemv tiles, launches of convt_cout1_kernel)."""
    from manga_image_translator_amd import lib as L

    lib = L.load()
    L.check(lib.mit_prof_enable(1), "mit_prof_enable")
    try:
        res = fn()
        torch.cuda.synchronize()
        stats, n = (L.MitProfStat * 64)(), C.c_int(0)
        L.check(lib.mit_prof_read(stats, 64, C.byref(n)), "mit_prof_read")
        kst, nk = (L.MitProfKernelStat * 64)(), C.c_int(0)
        L.check(lib.mit_prof_kernels_read(kst, 64, C.byref(nk)), "mit_prof_kernels_read")
    finally:
        L.check(lib.mit_prof_enable(0), "mit_prof_enable")
    gemv = sum(stats[i].launches for i in range(n.value) if lib.mit_conv_gemm_config_name(i).decode().startswith("gemv"))
    one = sum(kst[i].launches for i in range(nk.value) if kst[i].name == b"convt_cout1_kernel")
    return res, gemv, one


@pytest.mark.parametrize("H,W,B", [(96, 64, 2), (80, 80, 1)], ids=["portrait", "square"])
def test_engine_matches_the_four_launch_form(cuda, gemm_mode, engines, H, W, B):
    from manga_image_translator_amd import synth

    new, old = engines
    pages = torch.from_numpy(np.stack([synth.synth_page(i, H, W, n_boxes=4)[0] for i in range(B)])).to(cuda)
    (m_ref, l_ref, pad_ref), gemv_old, one_old = gemv_launches(lambda: old.forward(pages))
    m_ref, l_ref, f_ref = m_ref.clone(), l_ref.clone(), old.last_mask_f32.clone()
    # poison the new engine's workspace outputs through a first forward's views: stale values must not reach the valid region
    m0, l0, _ = new.forward(pages)
    m0.fill_(3)
    l0.fill_(SENTINEL)
    new.last_mask_f32.fill_(SENTINEL)
    (m, l, pad), gemv_new, one_new = gemv_launches(lambda: new.forward(pages))
    dw, dh = pad
    assert pad == pad_ref and ((dw > 0) if H > W else (dw == 0 and dh == 0))
    hv, wv = 1024 - dh, 1024 - dw
    assert tuple(m.shape) == (B, hv, wv) == tuple(m_ref.shape) and tuple(l.shape) == (B, 2, hv, wv)
    assert torch.equal(m, m_ref) and torch.equal(l, l_ref)
    assert tuple(new.last_mask_f32.shape) == (B, hv, wv) and torch.equal(new.last_mask_f32, f_ref[:, :hv, :wv])
    assert gemv_old == 12 and one_old == 0, (gemv_old, one_old)
    assert gemv_new == 0 and one_new == 3, (gemv_new, one_new)
