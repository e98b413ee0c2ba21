"""The memory-bound kernels of the AOT inpainter (aot_kernels.hip) called through the C ABI, each against the numpy restatement in
tests/_glue_cases.py of the reference line its comment cites (manga_translator/inpainting/inpainting_aot.py and the plugin path,
inpainting_lama_mpe.py:_infer):

  mit_aot_gate         signal * sigmoid(gate) * 1.8 (+ relu_nf)                          inpainting_aot.py:128-133, :35-36
  mit_aot_plane_stats  mean, 1 / (unbiased std + 1e-9)                                   :163-165
  mit_aot_blend        x (1 - m) + fuse m, m = sigmoid(5 (2 (g - mean) istd - 1))        :166-167, :189-192
  mit_aot_post         tail[8] -> clip -> ((v + 1) * 127.5) truncated -> composite       :133, :274; inpainting_lama_mpe.py:114, :57-61, :117
  mit_aot_prep         past the grid cap only (tests/test_page_io_gpu.py has the rest)   inpainting_lama_mpe.py:84-92

BIT / BYTE equality where the expression has no transcendental or has it only where it is exact (gates 30 / 0 / -200: sigmoid is
exactly 1 / 0.5 / 0); elsewhere the kernel's error against float64 must stay within 4 x the error of the float32 restatement
(printed: run with -s to see the figures).  Outputs sit inside sentinel-filled buffers.  The refusal and workspace-size tests are
not marked gpu: every refusal happens before any HIP call, so they run on the build machine with fake pointers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _glue_cases as G  # noqa: E402

gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SENT = float(G.SENT)


def _L():
    from manga_image_translator_amd import lib, ops

    return lib, lib.load(), C.c_void_p(ops.current_stream())


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _judge(name, got, r32, r64):
    e32, bar, ek = G.errors(r32, r64, got)
    print(f"{name}: float32 restatement {e32:.3e}, bar {bar:.3e}, kernel {ek:.3e}")
    assert ek <= bar, (name, e32, bar, ek)


# ---- mit_aot_gate ----------------------------------------------------------------------------------------------------------------
def _run_gate(cuda, C_, npix, in_ps, relu_nf, seed=0):
    lib, L, st = _L()
    c = G.gate_case(C_, npix, in_ps, seed)
    out_ps, off = C_ + 12, 4                                                        # a channel slice [4, 4 + C) of a wider tensor
    ind = _dev(c["buf"], cuda)
    out = torch.full((npix * out_ps + 8,), SENT, device=cuda)
    lib.check(L.mit_aot_gate(ind.data_ptr(), in_ps, out.data_ptr() + 4 * off, out_ps, npix, C_, relu_nf, st), "mit_aot_gate")
    buf = out.cpu().numpy()
    assert G.untouched_outside(buf, 1, npix, C_, npix * out_ps, out_ps, lead=off)
    got = G.view(buf, 1, npix, C_, npix * out_ps, out_ps, lead=off)[0]
    r32, r64 = G.gate_ref(c["s"], c["g"], relu_nf, f32), G.gate_ref(c["s"], c["g"], relu_nf, f64)
    _judge(f"aot_gate C={C_} npix={npix} ps={in_ps} relu_nf={relu_nf}", got, r32, r64)
    ex = c["exact"]
    if relu_nf:   # fmaxf(-0.0, 0) may return either zero (numpy's maximum keeps -0.0): the sign of a zero is not asked here
        assert (got >= 0).all() and (got[r64 < 0] == 0).all()
        assert G.bits_equal(got[ex] + f32(0.0), r32[ex] + f32(0.0))
    else:
        assert G.bits_equal(got[ex], r32[ex])


@gpu
@pytest.mark.parametrize("relu_nf", [0, 1])
@pytest.mark.parametrize("wide", [0, 8])
@pytest.mark.parametrize("npix", [1, 255, 1000])
@pytest.mark.parametrize("C_", [4, 32, 128])
def test_aot_gate(cuda, C_, npix, wide, relu_nf):
    _run_gate(cuda, C_, npix, 2 * C_ + wide, relu_nf, seed=C_ + npix)


@gpu
def test_aot_gate_past_the_grid_cap(cuda):
    _run_gate(cuda, 4, G.OVER_CAP, 8, 1)


# ---- mit_aot_prep past the grid cap ----------------------------------------------------------------------------------------------
@gpu
def test_aot_prep_past_the_grid_cap(cuda):
    lib, L, st = _L()
    n = G.OVER_CAP
    img = G.all_bytes_image(n)
    mask = ((np.arange(n) * 37) % 256).astype(np.uint8)
    out = torch.full((n + 4, 4), SENT, device=cuda)
    imgd, maskd = _dev(img, cuda), _dev(mask, cuda)
    lib.check(L.mit_aot_prep(imgd.data_ptr(), maskd.data_ptr(), out.data_ptr(), 1, 1, n, st), "mit_aot_prep")
    got = out.cpu().numpy()
    assert (got[n:] == SENT).all()
    m = (mask.astype(f32) / f32(255.0) >= f32(0.5)).astype(f32)                      # inpainting_lama_mpe.py:85-87
    rgb = (img.astype(f32) / f32(127.5) - f32(1.0)) * (f32(1.0) - m)[:, None]        # :84, :92
    assert G.bits_equal(got[:n], np.concatenate([m[:, None], rgb], -1))


# ---- mit_aot_post ----------------------------------------------------------------------------------------------------------------
def _run_post(cuda, pre, img, mask, composite, want_preclip):
    lib, L, st = _L()
    B, H, W, ps = pre.shape
    n = B * H * W
    out = torch.full((n * 3 + 16,), 7, dtype=torch.uint8, device=cuda)
    pc = torch.full((n * 3 + 4,), SENT, device=cuda)
    pred, imgd, maskd = _dev(pre, cuda), _dev(img, cuda), _dev(mask, cuda)
    lib.check(L.mit_aot_post(pred.data_ptr(), ps, imgd.data_ptr(), maskd.data_ptr(), out.data_ptr(),
                             pc.data_ptr() if want_preclip else None, B, H, W, composite, st), "mit_aot_post")
    got, gpc = out.cpu().numpy(), pc.cpu().numpy()
    assert (got[n * 3:] == 7).all() and (gpc[n * 3:] == SENT).all()
    if not want_preclip:
        assert (gpc == SENT).all()
    return got[:n * 3].reshape(B, H, W, 3), gpc[:n * 3].reshape(B, H, W, 3)


@gpu
@pytest.mark.parametrize("composite", [0, 1])
@pytest.mark.parametrize("pixstride", [6, 8])
def test_aot_post_at_exact_gates(cuda, pixstride, composite):
    c = G.aot_post_case(pixstride)
    ref, ref_pc = G.aot_post_ref(c["pre"], c["img"], c["mask"], composite)
    got, pc = _run_post(cuda, c["pre"], c["img"], c["mask"], composite, True)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    assert G.bits_equal(pc, ref_pc)                                                  # also where the composite hands back the page
    plain, _ = _run_post(cuda, c["pre"], c["img"], c["mask"], composite, False)
    assert np.array_equal(plain, got)
    band = c["band"]
    rows = {mk: slice(r * band, (r + 1) * band) for r, mk in enumerate(G.MASK_ROWS)}
    net = G.aot_post_ref(c["pre"], c["img"], c["mask"], 0)[0]
    for mk in G.MASK_ROWS:   # row 126 is the last the composite hands back, row 127 the first that keeps the network's byte
        want = c["img"] if composite and mk < 127 else net
        assert np.array_equal(got[0, rows[mk]], want[0, rows[mk]]), mk
    assert not np.array_equal(net[0, rows[126]], c["img"][0, rows[126]])


@gpu
def test_aot_post_past_the_grid_cap(cuda):
    n = G.OVER_CAP
    s, g = G.aot_post_pairs()
    e = np.arange(n * 3) % s.size
    pre = np.empty((1, 1, n, 6), f32)
    pre[0, 0, :, :3], pre[0, 0, :, 3:] = s[e].reshape(n, 3), g[e].reshape(n, 3)
    mask = np.asarray(G.MASK_ROWS, np.uint8)[np.arange(n) % 5].reshape(1, 1, n)
    img = ((np.arange(n * 3) * 11) % 256).astype(np.uint8).reshape(1, 1, n, 3)
    ref, ref_pc = G.aot_post_ref(pre, img, mask, 1)
    got, pc = _run_post(cuda, pre, img, mask, 1, True)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    assert G.bits_equal(pc, ref_pc)


# ---- mit_aot_blend ---------------------------------------------------------------------------------------------------------------
def _run_blend(cuda, B, hw, C_, seed=0):
    lib, L, st = _L()
    c = G.blend_case(B, hw, C_, seed)
    ps = dict(x=C_, fuse=C_ + 4, gate=C_ + 64)
    bs = {k: hw * p + 8 for k, p in ps.items()}                                      # batch strides larger than hw * ps
    bufs = {k: G.strided(c[k], bs[k], ps[k]) for k in ps}
    d = {k: _dev(v, cuda) for k, v in bufs.items()}
    mean, istd = _dev(c["mean"], cuda), _dev(c["istd"], cuda)
    lib.check(L.mit_aot_blend(d["x"].data_ptr(), bs["x"], ps["x"], d["fuse"].data_ptr(), bs["fuse"], ps["fuse"], d["gate"].data_ptr(),
                              bs["gate"], ps["gate"], mean.data_ptr(), istd.data_ptr(), B, hw, C_, st), "mit_aot_blend")
    buf = d["x"].cpu().numpy()
    assert G.untouched_outside(buf, B, hw, C_, bs["x"], ps["x"])
    for k in ("fuse", "gate"):
        assert np.array_equal(d[k].cpu().numpy().view(np.int32), bufs[k].view(np.int32))
    got = G.view(buf, B, hw, C_, bs["x"], ps["x"])
    (r32, _), (r64, _) = G.blend_ref(c, f32), G.blend_ref(c, f64)
    _judge(f"aot_blend B={B} hw={hw} C={C_}", got, r32, r64)
    # istd = 1e9: one ulp of the gate saturates the sigmoid, to fuse above the mean and to x below it (gate == mean, m = sigmoid(-5),
    # is in the comparison above)
    k, g1 = c["kind"], got[..., 1]
    assert G.bits_equal(g1[k == 1], c["fuse"][..., 1][k == 1]) and G.bits_equal(g1[k == 2], c["x"][..., 1][k == 2])


@gpu
@pytest.mark.parametrize("C_", [4, 128])
@pytest.mark.parametrize("hw", [1, 37, 513])
def test_aot_blend(cuda, hw, C_):
    _run_blend(cuda, 3, hw, C_, seed=hw + C_)


@gpu
def test_aot_blend_past_the_grid_cap(cuda):
    _run_blend(cuda, 1, G.OVER_CAP, 4)


# ---- mit_aot_plane_stats ---------------------------------------------------------------------------------------------------------
def _plane_stats(cuda, buf_dev, lead, bs, ps, B, hw, C_):
    """mean, istd [B, C] of the planes at buf_dev + lead, each result inside a sentinel-filled buffer; the workspace is exactly the
    size mit_aot_plane_stats_ws asks for, with guard bytes behind it."""
    lib, L, st = _L()
    need = L.mit_aot_plane_stats_ws(B, hw, C_)
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=cuda)
    mean, istd = torch.full((B * C_ + 4,), SENT, device=cuda), torch.full((B * C_ + 4,), SENT, device=cuda)
    lib.check(L.mit_aot_plane_stats(buf_dev.data_ptr() + 4 * lead, bs, ps, B, hw, C_, ws.data_ptr(), need, mean.data_ptr(), istd.data_ptr(),
                                    st), "mit_aot_plane_stats")
    m, i, w = mean.cpu().numpy(), istd.cpu().numpy(), ws.cpu().numpy()
    assert (m[B * C_:] == SENT).all() and (i[B * C_:] == SENT).all() and (w[need:] == 0xA5).all()
    return m[:B * C_].reshape(B, C_), i[:B * C_].reshape(B, C_)


@gpu
@pytest.mark.parametrize("C_,hw", G.STATS_SHAPES)
def test_aot_plane_stats_against_float64(cuda, C_, hw):
    B, ps = 3, C_ + 4
    bs = hw * ps + 16
    x = G.stats_case(B, hw, C_, seed=C_ + hw)
    buf = G.strided(x, bs, ps)
    d = _dev(buf, cuda)
    mean, istd = _plane_stats(cuda, d, 0, bs, ps, B, hw, C_)
    assert np.array_equal(d.cpu().numpy().view(np.int32), buf.view(np.int32))
    rm, ri = G.stats_ref(x)
    em = float((np.abs(mean - rm) / np.maximum(np.abs(rm), 1.0)).max())
    ei = float((np.abs(istd - ri) / ri).max())
    print(f"aot_plane_stats C={C_} hw={hw}: mean error {em:.3e} (bar 1e-6), istd error {ei:.3e} (bar 1e-5)")
    assert em < 1e-6 and ei < 1e-5
    for b in range(B):   # a plane's statistics do not depend on the batch it is in
        m1, i1 = _plane_stats(cuda, d, b * bs, bs, ps, 1, hw, C_)
        assert G.bits_equal(m1[0], mean[b]) and G.bits_equal(i1[0], istd[b])


@gpu
@pytest.mark.parametrize("C_,hw", G.STATS_SHAPES)
def test_aot_plane_stats_on_constant_planes(cuda, C_, hw):
    """n copies of one fp32 value sum exactly in double, the second pass sums zeros: mean == c and istd == 1 / (0 + 1e-9f), bit for bit."""
    B, ps = 3, C_ + 4
    bs = hw * ps + 16
    x, cst = G.stats_constant_case(B, hw, C_)
    d = _dev(G.strided(x, bs, ps), cuda)
    mean, istd = _plane_stats(cuda, d, 0, bs, ps, B, hw, C_)
    assert G.bits_equal(mean, cst)
    assert G.bits_equal(istd, np.full((B, C_), f32(1.0) / (f32(0.0) + f32(1e-9)), f32))


# ---- not marked gpu: workspace sizes and refusals --------------------------------------------------------------------------------
def test_aot_plane_stats_ws_bytes():
    from manga_image_translator_amd import lib

    L = lib.load()
    for B in (1, 3):
        for C_ in (4, 128, 1024):
            for hw, chunks in ((1, 1), (511, 1), (512, 1), (513, 2), (1024, 2), (1025, 3)):
                assert L.mit_aot_plane_stats_ws(B, hw, C_) == B * chunks * C_ * 16
    for B, hw, C_ in ((0, 512, 4), (1, 0, 4), (1, 512, 0), (-1, 512, 4), (1, -512, 4), (1, 512, -4)):
        assert L.mit_aot_plane_stats_ws(B, hw, C_) == 0


P_IN, P_OUT, P_A, P_B, P_C = 4096, 8192, 12288, 16384, 20480     # fake, non-null, 16-byte aligned: never dereferenced


def _refused(L, rc, text):
    assert rc != 0, text
    assert text.encode() in L.mit_last_error(), (text, L.mit_last_error())


def test_aot_kernels_refuse_what_their_error_paths_name():
    """One violated precondition per call; every one is rejected before any launch, so this needs no GPU."""
    from manga_image_translator_amd import lib

    L = lib.load()
    # mit_aot_gate(in, in_ps, out, out_ps, npix, C, relu_nf, stream)
    _refused(L, L.mit_aot_gate(None, 8, P_OUT, 4, 16, 4, 0, None), "mit_aot_gate: null pointer")
    _refused(L, L.mit_aot_gate(P_IN, 8, None, 4, 16, 4, 0, None), "mit_aot_gate: null pointer")
    _refused(L, L.mit_aot_gate(P_IN, 16, P_OUT, 8, 16, 6, 0, None), "mit_aot_gate: C must be a positive multiple of 4 (got 6)")
    _refused(L, L.mit_aot_gate(P_IN, 16, P_OUT, 8, 16, 0, 0, None), "mit_aot_gate: C must be a positive multiple of 4")
    for ips, ops_ in ((4, 4), (8, 0), (10, 4), (8, 6)):           # in < 2C, out < C, in % 4, out % 4
        _refused(L, L.mit_aot_gate(P_IN, ips, P_OUT, ops_, 16, 4, 0, None), "mit_aot_gate: pixel strides must be multiples of 4")
    _refused(L, L.mit_aot_gate(P_IN + 4, 8, P_OUT, 4, 16, 4, 0, None), "mit_aot_gate: operands must be 16-byte aligned")
    _refused(L, L.mit_aot_gate(P_IN, 8, P_OUT + 8, 4, 16, 4, 0, None), "mit_aot_gate: operands must be 16-byte aligned")

    # mit_aot_plane_stats(x, bs, ps, B, hw, C, ws, ws_bytes, mean, istd, stream)
    def stats(x=P_IN, bs=64, ps=8, B=1, hw=8, C_=8, ws=P_A, wsb=1 << 20, mean=P_B, istd=P_C):
        return L.mit_aot_plane_stats(x, bs, ps, B, hw, C_, ws, wsb, mean, istd, None)

    for kw in (dict(x=None), dict(ws=None), dict(mean=None), dict(istd=None)):
        _refused(L, stats(**kw), "mit_aot_plane_stats: null pointer")
    _refused(L, stats(hw=1, bs=8), "mit_aot_plane_stats: need B >= 1 and at least 2 pixels per plane")
    _refused(L, stats(B=0), "mit_aot_plane_stats: need B >= 1 and at least 2 pixels per plane")
    for C_ in (12, 2, 2048):                                      # not a power of two, below 4, above 1024
        _refused(L, stats(C_=C_, ps=2048, bs=8 * 2048), f"mit_aot_plane_stats: C must be a power of two in [4, 1024] (got {C_})")
    for kw in (dict(ps=4), dict(ps=10, bs=80), dict(bs=66), dict(bs=60)):   # ps < C, ps % 4, bs % 4, bs < hw * ps
        _refused(L, stats(**kw), "mit_aot_plane_stats: bad strides")
    for kw in (dict(x=P_IN + 4), dict(mean=P_B + 8), dict(ws=P_A + 4)):
        _refused(L, stats(**kw), "mit_aot_plane_stats: misaligned operand")
    need = L.mit_aot_plane_stats_ws(1, 8, 8)
    _refused(L, stats(wsb=need - 1), "mit_aot_plane_stats: workspace too small")
    _refused(L, stats(B=65536, wsb=1 << 40), "mit_aot_plane_stats: B too large")

    # mit_aot_blend(x, x_bs, x_ps, fuse, f_bs, f_ps, gate, g_bs, g_ps, mean, istd, B, hw, C, stream)
    def blend(x=P_IN, xs=(64, 8), f=P_OUT, fs=(64, 8), g=P_A, gs=(64, 8), mean=P_B, istd=P_C, C_=8):
        return L.mit_aot_blend(x, *xs, f, *fs, g, *gs, mean, istd, 1, 8, C_, None)

    for kw in (dict(x=None), dict(f=None), dict(g=None), dict(mean=None), dict(istd=None)):
        _refused(L, blend(**kw), "mit_aot_blend: null pointer")
    _refused(L, blend(C_=6), "mit_aot_blend: C must be a positive multiple of 4")
    for kw in (dict(xs=(66, 8)), dict(xs=(64, 10)), dict(fs=(62, 8)), dict(fs=(64, 9)), dict(gs=(65, 8)), dict(gs=(64, 11))):
        _refused(L, blend(**kw), "mit_aot_blend: strides must be multiples of 4")
    for kw in (dict(xs=(64, 4)), dict(fs=(64, 4)), dict(gs=(64, 4))):
        _refused(L, blend(**kw), "mit_aot_blend: pixel strides must hold C channels")
    for kw in (dict(x=P_IN + 4), dict(f=P_OUT + 8), dict(g=P_A + 12), dict(mean=P_B + 4), dict(istd=P_C + 4)):
        _refused(L, blend(**kw), "mit_aot_blend: operands must be 16-byte aligned")

    # mit_aot_post(pre, pre_ps, img, mask, out, preclip, B, H, W, composite, stream)
    def post(pre=P_IN, ps=6, img=P_A, mask=P_B, out=P_OUT, H=4):
        return L.mit_aot_post(pre, ps, img, mask, out, None, 1, H, 4, 1, None)

    for kw in (dict(pre=None), dict(img=None), dict(mask=None), dict(out=None)):
        _refused(L, post(**kw), "mit_aot_post: null pointer")
    _refused(L, post(H=0), "mit_aot_post: empty page")
    _refused(L, post(ps=5), "mit_aot_post: the input holds 3 signal + 3 gate channels per pixel")
