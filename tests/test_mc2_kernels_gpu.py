"""The glue kernels of the mc2 colorizer (mc2_kernels.hip) called through the C ABI, each against the numpy restatement in
tests/_glue_cases.py of the reference line its comment cites (manga_translator/colorization/manga_colorization_v2_utils/...):

  mit_mc2_ffd_pack     np.float32(x / 255.) only when the page max exceeds 1.2; (sigma x 3, 3 + c*4 + (i*2 + j), 0)
                                                                                  denoising/denoiser.py:79-103, functions.py:16-56
  mit_mc2_ffd_unpack   clamp(x - noise, 0, 1) * 255 truncated, BGR                functions.py:58-83, denoiser.py:107-118, utils.py:17-33
  mit_mc2_gen_in       np.pad(.., 'maximum') then ToTensor                        utils/utils.py:27-38, manga_colorization_v2.py:58-59
  mit_mc2_post         (tanh(y) * 0.5 + 0.5) * 255 truncated, cropped             manga_colorization_v2.py:61-74
  mit_se_squeeze / excite / apply   x * sigmoid(conv2(relu(conv1(avgpool(x)))))   networks/models.py:88-106, extractor.py:8-26, :64-67

pack, unpack and gen_in are asked BIT / BYTE equality.  mit_mc2_post is asked floor(float64) where float64 is at least 0.2499 from
a truncation boundary, +-1 on the boundaries themselves.  The squeeze partials are asked the worst-case bound of a double sum, the
excite / apply pair tests/_mc2_oracle.py's ``_se`` in float64 at tests/test_mc2_gpu.py's 1e-5.  Outputs sit inside sentinel-filled
buffers.  The refusal and workspace-size tests are not marked gpu: every refusal happens before any HIP call.

test_mc2_post_specials[9.0] is why the exit kernel evaluates in double: float64 gives (tanh(9) * 0.5 + 0.5) * 255 = 254.99999612,
byte 254, 3.9e-6 below a truncation boundary, while float32 resolves 1.5e-5 there.  In float32 tanh(9) = 1 - 2^-24, tanh * 0.5 + 0.5
ties to 1.0 and the byte is 255: a float32 kernel measured 255 on the MI355X, as numpy float32 gives (tests/test_glue_cases.py)."""
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


def _rel(got, ref):
    return float(np.abs(np.asarray(got, f64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


# ---- mit_mc2_ffd_pack ------------------------------------------------------------------------------------------------------------
def _run_pack(cuda, img):
    lib, L, st = _L()
    B, H, W, Cin = img.shape
    n = B * ((H + 1) // 2) * ((W + 1) // 2) * 16
    out = torch.full((n + 16,), SENT, device=cuda)
    pmax = torch.full((B + 2,), 12345, dtype=torch.int32, device=cuda)
    imgd = _dev(img, cuda)
    lib.check(L.mit_mc2_ffd_pack(imgd.data_ptr(), B, H, W, Cin, G.SIGMA, pmax.data_ptr(), out.data_ptr(), st), "mit_mc2_ffd_pack")
    got, pm = out.cpu().numpy(), pmax.cpu().numpy()
    assert (got[n:] == SENT).all() and (pm[B:] == 12345).all()
    return pm[:B].astype(np.uint32), got[:n].reshape(B, (H + 1) // 2, (W + 1) // 2, 16)


def _check_pack(cuda, img):
    rpm, ref = G.ffd_pack_ref(img)
    pm, got = _run_pack(cuda, img)
    assert np.array_equal(pm, rpm), (pm, rpm)                                        # the per-page RGB max itself
    assert G.bits_equal(got, ref), np.argwhere(got.view(np.int32) != ref.view(np.int32))[:8]


@gpu
@pytest.mark.parametrize("Cin", [3, 4])
@pytest.mark.parametrize("H,W", G.FFD_SIDES)
def test_ffd_pack_switches_per_page(cuda, H, W, Cin):
    """B = 3: pages of max 0 and 1 stay as they are, the page of max 2 is divided by 255; alpha = 255 (Cin = 4) changes nothing."""
    _check_pack(cuda, G.ffd_pages(H, W, Cin))


@gpu
@pytest.mark.parametrize("Cin", [3, 4])
def test_ffd_pack_every_byte_value(cuda, Cin):
    _check_pack(cuda, G.ffd_all_bytes_page(Cin))


@gpu
def test_ffd_pack_dim_rgba_page_stays_unnormalised(cuda):
    img = G.ffd_dim_rgba_page()
    _check_pack(cuda, img)
    pm, got = _run_pack(cuda, img)
    assert pm.tolist() == [1] and got[..., 3:15].max() == 1.0


@gpu
def test_ffd_pack_past_the_grid_cap(cuda):
    W = 2 * G.OVER_CAP - 1                                                           # odd: the last column is repeated
    _check_pack(cuda, G.all_bytes_image(W).reshape(1, 1, W, 3))


# ---- mit_mc2_ffd_unpack ----------------------------------------------------------------------------------------------------------
def _run_unpack(cuda, img, pmax, noise, plane=True, bgr=True):
    lib, L, st = _L()
    B, H, W, Cin = img.shape
    n = B * H * W
    pl = torch.full((n + 16,), 7, dtype=torch.uint8, device=cuda)
    bg = torch.full((n * 3 + 16,), 7, dtype=torch.uint8, device=cuda)
    imgd, pmd, nd = _dev(img, cuda), _dev(pmax.astype(np.int32), cuda), _dev(noise, cuda)
    lib.check(L.mit_mc2_ffd_unpack(imgd.data_ptr(), B, H, W, Cin, pmd.data_ptr(), nd.data_ptr(), noise.shape[-1],
                                   pl.data_ptr() if plane else None, bg.data_ptr() if bgr else None, st), "mit_mc2_ffd_unpack")
    gp, gb = pl.cpu().numpy(), bg.cpu().numpy()
    assert (gp[n:] == 7).all() and (gb[n * 3:] == 7).all()
    assert plane or (gp == 7).all()
    assert bgr or (gb == 7).all()
    return gp[:n].reshape(B, H, W), gb[:n * 3].reshape(B, H, W, 3)


def _check_unpack(cuda, img, noise):
    pm = G.ffd_pmax(img)
    ref = G.ffd_unpack_ref(img, pm, noise)
    plane, bgr = _run_unpack(cuda, img, pm, noise)
    assert np.array_equal(bgr, ref), np.argwhere(bgr != ref)[:8]
    assert np.array_equal(plane, ref[..., 0])                                        # the plane holds B
    return ref


@gpu
@pytest.mark.parametrize("Cin,ps", [(3, 12), (4, 12), (3, 16), (4, 16)])
def test_ffd_unpack_at_every_byte_boundary(cuda, Cin, ps):
    img, noise = G.ffd_unpack_boundary_case(Cin, ps)
    ref = _check_unpack(cuda, img, noise)
    assert set(ref[0].ravel().tolist()) == set(range(256))
    pm = G.ffd_pmax(img)
    only_plane, none_bgr = _run_unpack(cuda, img, pm, noise, bgr=False)              # either output may be NULL
    none_plane, only_bgr = _run_unpack(cuda, img, pm, noise, plane=False)
    assert np.array_equal(only_plane, ref[..., 0]) and np.array_equal(only_bgr, ref)


@gpu
@pytest.mark.parametrize("Cin,ps", [(3, 12), (4, 16)])
def test_ffd_unpack_unnormalised_page(cuda, Cin, ps):
    img, noise = G.ffd_unpack_unnormalised_case(Cin, ps)
    ref = _check_unpack(cuda, img, noise)
    assert {0, 255} <= set(ref.ravel().tolist()) and len(set(ref.ravel().tolist())) > 100


@gpu
@pytest.mark.parametrize("Cin,ps", [(3, 12), (4, 16)])
def test_ffd_unpack_depth_to_space_index(cuda, Cin, ps):
    """The noise encodes its own (c, idx) slot: a swapped i / j or channel changes bytes (tests/test_glue_cases.py shows it does)."""
    _check_unpack(cuda, *G.ffd_unpack_position_case(Cin, ps))


@gpu
def test_ffd_unpack_past_the_grid_cap(cuda):
    W = G.OVER_CAP
    img = G.all_bytes_image(W).reshape(1, 1, W, 3)
    rnd = np.random.default_rng(11).uniform(-0.2, 1.2, (1, 1, W, 3)).astype(f32)
    _check_unpack(cuda, img, G.ffd_noise(1, 1, W, 12, lambda b, y, x, c: rnd[b, y, x, c]))


# ---- mit_mc2_gen_in --------------------------------------------------------------------------------------------------------------
def _check_gen_in(cuda, plane, Hp, Wp):
    lib, L, st = _L()
    B, h, w = plane.shape
    n = B * Hp * Wp
    out = torch.full((n + 4, 4), SENT, device=cuda)
    pd = _dev(plane, cuda)
    lib.check(L.mit_mc2_gen_in(pd.data_ptr(), B, h, w, out.data_ptr(), Hp, Wp, st), "mit_mc2_gen_in")
    got = out.cpu().numpy()
    assert (got[n:] == SENT).all()
    ref = G.gen_in_ref(plane, Hp, Wp)
    assert G.bits_equal(got[:n].reshape(B, Hp, Wp, 4), ref)                          # channels 1-3: +0.0 exactly


@gpu
@pytest.mark.parametrize("h,w,Hp,Wp", G.GEN_IN_SHAPES)
def test_gen_in(cuda, h, w, Hp, Wp):
    _check_gen_in(cuda, G.gen_in_case(h, w), Hp, Wp)


@gpu
def test_gen_in_past_the_grid_cap(cuda):
    assert G.OVER_CAP % 3 == 0
    w = G.OVER_CAP // 3                                                              # Hp * Wp = 3 w: two padded rows of column maxima
    _check_gen_in(cuda, G.all_bytes_image(w)[:, 0].reshape(1, 1, w).copy(), 3, w)


# ---- mit_mc2_post ----------------------------------------------------------------------------------------------------------------
def _run_mc2_post(cuda, pre, h, w):
    lib, L, st = _L()
    B, Hp, Wp, ps = pre.shape
    n = B * h * w * 3
    out = torch.full((n + 16,), 7, dtype=torch.uint8, device=cuda)
    pd = _dev(pre, cuda)
    lib.check(L.mit_mc2_post(pd.data_ptr(), ps, B, Hp, Wp, out.data_ptr(), h, w, st), "mit_mc2_post")
    got = out.cpu().numpy()
    assert (got[n:] == 7).all()
    return got[:n].reshape(B, h, w, 3)


@gpu
@pytest.mark.parametrize("ps", [3, 4])
@pytest.mark.parametrize("h,w", [(8, 40), (5, 33)])
def test_mc2_post_away_from_boundaries(cuda, h, w, ps):
    x, _k = G.post_margin_inputs()
    pre = G.post_case(x, 2, 8, 40, h, w, ps)
    got = _run_mc2_post(cuda, pre, h, w)
    ref = G.post_ref64(pre[:, :h, :w, :3])
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    assert set(ref.ravel().tolist()) == set(range(255))


@gpu
@pytest.mark.parametrize("ps", [3, 4])
@pytest.mark.parametrize("h,w", [(8, 40), (5, 33)])
def test_mc2_post_on_boundaries(cuda, h, w, ps):
    pre = G.post_case(G.post_boundary_inputs(), 2, 8, 40, h, w, ps)
    got = _run_mc2_post(cuda, pre, h, w)
    ref = G.post_ref64(pre[:, :h, :w, :3])
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    print(f"mc2_post on boundaries: {int((d != 0).sum())} of {d.size} bytes differ from floor(float64), max {int(d.max())}")
    assert d.max() <= 1


@gpu
@pytest.mark.parametrize("v", G.POST_SPECIALS, ids=[repr(float(v)) for v in G.POST_SPECIALS])
def test_mc2_post_specials(cuda, v):
    """floor(float64) exactly.  [9.0]: float64 254.99999612 -> 254, where any float32 evaluation gives 255 because
    tanh(9) * 0.5 + 0.5 rounds to 1.0 in float32 (module docstring): the kernel evaluates in double."""
    pre = G.post_case(np.array([v], f32), 1, 2, 3, 2, 3, 3)
    got = _run_mc2_post(cuda, pre, 2, 3)
    ref = G.post_ref64(pre)
    print(f"mc2_post({v}): kernel {int(got[0, 0, 0, 0])}, floor(float64) {int(ref[0, 0, 0, 0])} ({float(G.post_value64(v)):.8f}), "
          f"numpy float32 {int(G.post_ref32(pre)[0, 0, 0, 0])}")
    assert np.array_equal(got, ref)


@gpu
def test_mc2_post_past_the_grid_cap(cuda):
    x, _k = G.post_margin_inputs()
    w = G.OVER_CAP
    pre = G.post_case(x, 1, 1, w, 1, w, 3)
    got = _run_mc2_post(cuda, pre, 1, w)
    assert np.array_equal(got, G.post_ref64(pre))


# ---- mit_se_squeeze --------------------------------------------------------------------------------------------------------------
def _squeeze(cuda, xd, bs, ps, B, hw, C_):
    """The partial sums [B, nchunks, C] (double) in a workspace of exactly mit_se_squeeze_ws bytes with guard bytes behind it."""
    lib, L, st = _L()
    need = L.mit_se_squeeze_ws(B, hw, C_)
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=cuda)
    lib.check(L.mit_se_squeeze(xd.data_ptr(), bs, ps, B, hw, C_, ws.data_ptr(), need, st), "mit_se_squeeze")
    assert bool((ws[need:] == 0xA5).all())
    return ws


@gpu
@pytest.mark.parametrize("hw", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("C_", [4, 16, 64, 1024])
def test_se_squeeze_partials(cuda, C_, hw):
    B, ps = 2, C_ + 4
    bs = hw * ps + 8
    rng = np.random.default_rng(C_ + hw)
    x = (rng.standard_normal((B, hw, C_)) * 3 + 1).astype(f32)
    buf = G.strided(x, bs, ps, fill=f32(1e30))                                       # a stride slip would add 1e30
    ws = _squeeze(cuda, _dev(buf, cuda), bs, ps, B, hw, C_)
    n = (hw + 255) // 256
    got = ws.cpu().numpy()[:B * n * C_ * 8].view(f64).reshape(B, n, C_)
    s, a = G.se_chunk_sums(x)
    err = np.abs(got.astype(np.longdouble) - s)
    bound = hw * 2.0 ** -53 * a                                                      # worst case of a double sum of that many terms
    print(f"se_squeeze C={C_} hw={hw}: worst error / bound {float((err / bound).max()):.3e}")
    assert (err <= bound).all()


# ---- mit_se_excite, mit_se_apply -------------------------------------------------------------------------------------------------
def _se64(x, w):
    """s [B, C] in float64 (networks/models.py:88-106)."""
    w1, b1, w2, b2 = (v.astype(f64) for v in w)
    h = np.maximum(x.astype(f64).mean(1) @ w1.T + b1, 0.0)
    return h, G.sigmoid64(h @ w2.T + b2)


def _run_se(cuda, C_, hw, act, alias, dead=False):
    import torch.nn.functional as F

    import _mc2_oracle as O

    lib, L, st = _L()
    B = 2
    rng = np.random.default_rng(C_ * 7 + hw + act)
    x, r = rng.standard_normal((B, hw, C_)).astype(f32), rng.standard_normal((B, hw, C_)).astype(f32)
    w = G.se_weights(C_, seed=C_ + hw, dead=dead)
    xs, rs = (hw * (C_ + 4) + 8, C_ + 4), (hw * (C_ + 8) + 16, C_ + 8)               # each operand has its own strides
    xbuf, rbuf = G.strided(x, *xs), G.strided(r, *rs)
    xd, rd = _dev(xbuf, cuda), _dev(rbuf, cuda)
    ws = _squeeze(cuda, xd, *xs, B, hw, C_)
    sd = torch.full((B * C_ + 4,), SENT, device=cuda)
    wd = [_dev(v, cuda) for v in w]
    lib.check(L.mit_se_excite(ws.data_ptr(), B, hw, C_, *[v.data_ptr() for v in wd], sd.data_ptr(), st), "mit_se_excite")
    out, os_ = (xd, xs) if alias == "x" else (rd, rs)
    lib.check(L.mit_se_apply(xd.data_ptr(), *xs, sd.data_ptr(), rd.data_ptr(), *rs, out.data_ptr(), *os_, B, hw, C_, act, st), "mit_se_apply")
    s = sd.cpu().numpy()
    assert (s[B * C_:] == SENT).all()
    s = s[:B * C_].reshape(B, C_)
    h64, s64 = _se64(x, w)
    obuf = out.cpu().numpy()
    assert G.untouched_outside(obuf, B, hw, C_, *os_)
    other, obuf0 = (rd, rbuf) if alias == "x" else (xd, xbuf)
    assert np.array_equal(other.cpu().numpy().view(np.int32), obuf0.view(np.int32))   # the operand that is not the output is intact
    got = G.view(obuf, B, hw, C_, *os_)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()                 # noqa: E731
    osd = {"p.conv1.weight": t(w[0])[:, :, None, None], "p.conv1.bias": t(w[1]), "p.conv2.weight": t(w[2])[:, :, None, None],
           "p.conv2.bias": t(w[3])}
    ref = O._se(osd, "p", t(x).permute(0, 2, 1)[..., None]) + t(r).permute(0, 2, 1)[..., None]
    ref = (F.relu(ref) if act else ref)[..., 0].permute(0, 2, 1).numpy()
    es, eo = _rel(s, s64), _rel(got, ref)
    print(f"se C={C_} hw={hw} act={act} out={alias} dead={dead}: s error {es:.3e}, output error {eo:.3e} (bar 1e-5)")
    assert es <= 1e-5 and eo <= 1e-5
    if dead:   # every hidden unit is negative before the ReLU: h = 0, and s = sigmoid(0 + b2)
        assert (h64 == 0).all()
        ex = np.isin(w[3], np.asarray(G.EXACT_GATES, f32))
        assert ex.sum() >= C_ // 2
        assert G.bits_equal(s[:, ex], np.broadcast_to(G.sigmoid32(w[3])[ex], (B, int(ex.sum()))))   # exact where the sigmoid is
        assert G.bits_equal(s[0], s[1])                                              # and nothing of x reaches s


@gpu
@pytest.mark.parametrize("alias", ["x", "res"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("hw", [1, 257])
@pytest.mark.parametrize("C_", [16, 64])
def test_se_excite_and_apply(cuda, C_, hw, act, alias):
    _run_se(cuda, C_, hw, act, alias)


@gpu
@pytest.mark.parametrize("C_", [16, 64])
def test_se_excite_with_every_hidden_unit_dead(cuda, C_):
    _run_se(cuda, C_, 257, 0, "res", dead=True)


@gpu
def test_se_apply_past_the_grid_cap(cuda):
    lib, L, st = _L()
    hw, C_ = G.OVER_CAP, 4
    rng = np.random.default_rng(3)
    x, r = rng.standard_normal((1, hw, C_)).astype(f32), rng.standard_normal((1, hw, C_)).astype(f32)
    s = np.array([[0.25, 0.9, 0.0, 1.0]], f32)
    xd, rd, sd = _dev(x, cuda), _dev(r, cuda), _dev(s, cuda)
    out = torch.full((hw * C_ + 8,), SENT, device=cuda)
    lib.check(L.mit_se_apply(xd.data_ptr(), hw * C_, C_, sd.data_ptr(), rd.data_ptr(), hw * C_, C_, out.data_ptr(), hw * C_, C_, 1, hw, C_, 1, st),
              "mit_se_apply")
    got = out.cpu().numpy()
    assert (got[hw * C_:] == SENT).all()
    ref = np.maximum(x.astype(f64) * s.astype(f64)[:, None] + r, 0.0)
    assert _rel(got[:hw * C_].reshape(1, hw, C_), ref) <= 1e-5


# ---- not marked gpu: workspace sizes and refusals --------------------------------------------------------------------------------
def test_se_squeeze_ws_bytes():
    from manga_image_translator_amd import lib

    L = lib.load()
    for B in (1, 2):
        for C_ in (4, 64, 1024):
            for hw, chunks in ((1, 1), (255, 1), (256, 1), (257, 2), (512, 2), (513, 3)):
                assert L.mit_se_squeeze_ws(B, hw, C_) == B * chunks * C_ * 8


P_IN, P_OUT, P_A, P_B, P_C, P_D = 4096, 8192, 12288, 16384, 20480, 24576     # fake, non-null, 16-byte aligned: never dereferenced


def _refused(L, rc, text):
    assert rc != 0, text
    assert text.encode() in L.mit_last_error(), (text, L.mit_last_error())


def test_mc2_kernels_refuse_what_their_error_paths_name():
    """One violated precondition per call; every one is rejected before any HIP call, so this needs no GPU."""
    from manga_image_translator_amd import lib

    L = lib.load()

    # mit_se_squeeze(x, bs, ps, B, hw, C, ws, ws_bytes, stream)
    def squeeze(x=P_IN, bs=64, ps=8, C_=8, ws=P_A, wsb=1 << 20):
        return L.mit_se_squeeze(x, bs, ps, 1, 8, C_, ws, wsb, None)

    _refused(L, squeeze(x=None), "mit_se_squeeze: null pointer")
    _refused(L, squeeze(ws=None), "mit_se_squeeze: null pointer")
    for C_ in (12, 2, 2048):
        _refused(L, squeeze(C_=C_), "mit_se_squeeze: C must be a power of two in [4, 1024]")
    for kw in (dict(ps=10), dict(bs=66), dict(x=P_IN + 4)):
        _refused(L, squeeze(**kw), "mit_se_squeeze: strides must be multiples of 4 floats, x 16-byte aligned")
    _refused(L, squeeze(wsb=L.mit_se_squeeze_ws(1, 8, 8) - 1), "mit_se_squeeze: workspace too small")

    # mit_se_excite(ws, B, hw, C, w1, b1, w2, b2, s, stream)
    ptrs = [P_A, P_IN, P_B, P_C, P_D, P_OUT]
    for i in range(6):
        p = list(ptrs)
        p[i] = None
        _refused(L, L.mit_se_excite(p[0], 1, 8, 16, p[1], p[2], p[3], p[4], p[5], None), "mit_se_excite: null pointer")
    for C_ in (8, 24, 1040):
        _refused(L, L.mit_se_excite(P_A, 1, 8, C_, P_IN, P_B, P_C, P_D, P_OUT, None), "mit_se_excite: C must be a multiple of 16 in [16, 1024]")

    # mit_se_apply(x, x_bs, x_ps, s, res, r_bs, r_ps, out, o_bs, o_ps, B, hw, C, act, stream)
    def apply(x=P_IN, xs=(64, 8), s=P_A, r=P_B, rs=(64, 8), o=P_OUT, os_=(64, 8), C_=8, act=0):
        return L.mit_se_apply(x, *xs, s, r, *rs, o, *os_, 1, 8, C_, act, None)

    for kw in (dict(x=None), dict(s=None), dict(r=None), dict(o=None)):
        _refused(L, apply(**kw), "mit_se_apply: null pointer")
    _refused(L, apply(C_=6), "mit_se_apply: C must be a multiple of 4")
    for kw in (dict(xs=(64, 10)), dict(rs=(64, 9)), dict(os_=(64, 11)), dict(xs=(66, 8)), dict(rs=(62, 8)), dict(os_=(65, 8)),
               dict(x=P_IN + 4), dict(r=P_B + 8), dict(o=P_OUT + 12)):
        _refused(L, apply(**kw), "mit_se_apply: strides must be multiples of 4 floats, operands 16-byte aligned")
    for act in (lib.ACT_LEAKY, lib.ACT_SIGMOID, -1):
        _refused(L, apply(act=act), "mit_se_apply: act none | relu")

    # mit_mc2_ffd_pack(img, B, H, W, Cin, sigma, pmax, out, stream)
    for img, pm, out in ((None, P_A, P_OUT), (P_IN, None, P_OUT), (P_IN, P_A, None)):
        _refused(L, L.mit_mc2_ffd_pack(img, 1, 4, 4, 3, 0.1, pm, out, None), "mit_mc2_ffd_pack: null pointer")
    for Cin in (1, 2, 5):
        _refused(L, L.mit_mc2_ffd_pack(P_IN, 1, 4, 4, Cin, 0.1, P_A, P_OUT, None), "mit_mc2_ffd_pack: bad shape (Cin 3 | 4)")
    _refused(L, L.mit_mc2_ffd_pack(P_IN, 1, 0, 4, 3, 0.1, P_A, P_OUT, None), "mit_mc2_ffd_pack: bad shape (Cin 3 | 4)")
    _refused(L, L.mit_mc2_ffd_pack(P_IN, 1, 4, 4, 3, 0.1, P_A, P_OUT + 4, None), "mit_mc2_ffd_pack: output must be 16-byte aligned")

    # mit_mc2_ffd_unpack(img, B, H, W, Cin, pmax, noise, noise_ps, plane, bgr, stream)
    def unpack(img=P_IN, Cin=3, pm=P_A, noise=P_B, nps=12, plane=P_OUT, bgr=P_C):
        return L.mit_mc2_ffd_unpack(img, 1, 4, 4, Cin, pm, noise, nps, plane, bgr, None)

    for kw in (dict(img=None), dict(pm=None), dict(noise=None), dict(plane=None, bgr=None)):
        _refused(L, unpack(**kw), "mit_mc2_ffd_unpack: null pointer")
    for kw in (dict(Cin=2), dict(Cin=5), dict(nps=11), dict(nps=8)):
        _refused(L, unpack(**kw), "mit_mc2_ffd_unpack: bad shape")

    # mit_mc2_gen_in(plane, B, h, w, out, Hp, Wp, stream)
    _refused(L, L.mit_mc2_gen_in(None, 1, 4, 4, P_OUT, 4, 4, None), "mit_mc2_gen_in: null pointer")
    _refused(L, L.mit_mc2_gen_in(P_IN, 1, 4, 4, None, 4, 4, None), "mit_mc2_gen_in: null pointer")
    for Hp, Wp in ((8, 8), (3, 4), (4, 3)):                        # both sides padded; smaller than the plane
        _refused(L, L.mit_mc2_gen_in(P_IN, 1, 4, 4, P_OUT, Hp, Wp, None), "mit_mc2_gen_in: bad shape (one side padded)")
    _refused(L, L.mit_mc2_gen_in(P_IN, 1, 4, 4, P_OUT + 8, 4, 4, None), "mit_mc2_gen_in: output must be 16-byte aligned")

    # mit_mc2_post(pre, pre_ps, B, Hp, Wp, out, h, w, stream)
    _refused(L, L.mit_mc2_post(None, 3, 1, 4, 4, P_OUT, 4, 4, None), "mit_mc2_post: null pointer")
    _refused(L, L.mit_mc2_post(P_IN, 3, 1, 4, 4, None, 4, 4, None), "mit_mc2_post: null pointer")
    for ps, h, w in ((2, 4, 4), (3, 5, 4), (3, 4, 5), (3, 0, 4)):  # pre_pixstride < 3; crop larger than the padded map; empty
        _refused(L, L.mit_mc2_post(P_IN, ps, 1, 4, 4, P_OUT, h, w, None), "mit_mc2_post: bad shape")
