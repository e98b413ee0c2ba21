"""The mc2 colorizer on the MI355X: the grouped convolution, squeeze-and-excitation and INTER_AREA resize against float64 / the
host twin, the engine against the float64 CPU oracle (tests/_mc2_oracle.py) with taps, batch independence, and the plugin against
the reference's own _infer (tests/golden/mc2_infer.npz).  Engine tests run in both GEMM modes (the ``gemm_mode`` fixture)."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _mc2_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(cuda, mode):
    from manga_image_translator_amd import mc2

    if mode not in _ENGINES:
        g, f = O.weights()
        _ENGINES[mode] = mc2.Mc2Engine(g, f, device=cuda)
    return _ENGINES[mode]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _rel(got, ref):
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


# (channels, group width, stride, dilation, act) of every grouped convolution the model runs
_GC = [(128, 4, 1, 1, 1), (256, 8, 2, 1, 1), (256, 8, 1, 1, 1), (512, 16, 2, 1, 1), (512, 16, 1, 1, 1), (256, 8, 1, 1, 2),
       (128, 4, 1, 2, 2), (128, 4, 1, 4, 2), (64, 2, 1, 1, 2), (64, 2, 1, 2, 2), (64, 2, 1, 4, 2)]


@pytest.mark.parametrize("C,cpg,s,d,act", _GC)
@pytest.mark.parametrize("odd", [False, True])
def test_grouped_conv_against_float64(cuda, C, cpg, s, d, act, odd):
    from manga_image_translator_amd import mc2

    H, W = (37, 53) if odd else (24, 40)
    g = torch.Generator().manual_seed(C + cpg + s + d)
    x = torch.randn(3, C, H, W, generator=g)
    w = torch.randn(C, cpg, 3, 3, generator=g) / (3 * cpg ** 0.5)
    bn = (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1,
          torch.rand(C, generator=g) + 0.5, 1e-5) if act == 1 else None
    conv = mc2._Grouped(w, C, s, d, act, bn=bn, device=cuda)
    xin = torch.zeros(3, H, W, C + 16, device=cuda)
    xin[..., 8:8 + C] = x.permute(0, 2, 3, 1).to(cuda)                      # a strided channel view as the input
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    out = torch.full((3, Ho, Wo, C + 32), 7.0, device=cuda)
    conv(xin[..., 8:8 + C], out[..., 16:16 + C])                             # and as the output
    one = torch.empty(1, Ho, Wo, C, device=cuda)
    conv(xin[1:2, ..., 8:8 + C], one)
    again = torch.full_like(out, 7.0)
    conv(xin[..., 8:8 + C], again[..., 16:16 + C])
    torch.cuda.synchronize()
    ref = F.conv2d(x.double(), w.double(), stride=s, padding=d, dilation=d, groups=C // cpg)
    if bn is not None:
        ref = F.batch_norm(ref, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.0, 1e-5)
    ref = F.relu(ref) if act == 1 else F.leaky_relu(ref, 0.2)
    got = _nchw(out[..., 16:16 + C].cpu()).double()
    assert _rel(got, ref) <= 1e-5, _rel(got, ref)
    assert bool((out[..., :16] == 7.0).all()) and bool((out[..., 16 + C:] == 7.0).all()), "the launch wrote outside its slice"
    assert torch.equal(one[0], out[1, ..., 16:16 + C]), "B = 1 and B = 3 differ"
    assert torch.equal(again, out), "a repeat run differs"


@pytest.mark.parametrize("C,hw", [(128, (45, 31)), (512, (26, 18)), (1024, (13, 9))])
def test_se_against_float64(cuda, C, hw):
    from manga_image_translator_amd import mc2

    g = torch.Generator().manual_seed(C)
    sd = {"p.conv1.weight": torch.randn(C // 16, C, 1, 1, generator=g) / C ** 0.5, "p.conv1.bias": torch.randn(C // 16, generator=g) * 0.1,
          "p.conv2.weight": torch.randn(C, C // 16, 1, 1, generator=g) / (C // 16) ** 0.5, "p.conv2.bias": torch.randn(C, generator=g) * 0.1}
    eng = _engine(cuda, 6)
    se = mc2._SE(sd, "p", cuda)
    t = torch.randn(2, C, *hw, generator=g)
    r = torch.randn(2, C, *hw, generator=g)
    td = t.permute(0, 2, 3, 1).contiguous().to(cuda)
    rbuf = torch.zeros(2, *hw, C + 64, device=cuda)
    rbuf[..., 64:] = r.permute(0, 2, 3, 1).to(cuda)
    out = torch.empty(2, *hw, C, device=cuda)
    eng.se(se, td, rbuf[..., 64:], out, 1)
    eng.se(se, td, rbuf[..., 64:], rbuf[..., 64:], 0)                      # in place over a strided residual
    torch.cuda.synchronize()
    sdd = {k: v.double() for k, v in sd.items()}
    ref = O._se(sdd, "p", t.double())
    assert _rel(_nchw(out.cpu()).double(), F.relu(ref + r.double())) <= 1e-5
    assert _rel(_nchw(rbuf[..., 64:].cpu()).double(), ref + r.double()) <= 1e-5


@pytest.mark.parametrize("src,dst", [((2048, 1456), (853, 1200)), ((1200, 853), (811, 576)), ((150, 230), (192, 295)),
                                     ((37, 53), (80, 29)), ((300, 212), (272, 192))])
def test_resize_area_byte_equal_to_the_host_twin(cuda, src, dst):
    from manga_image_translator_amd import imgproc

    rng = np.random.default_rng(src[0] + dst[0])
    img = rng.integers(0, 256, size=(2,) + src + (3,), dtype=np.uint8)
    got = imgproc.resize_u8(torch.from_numpy(img).to(cuda), (dst[1], dst[0]), area=True).cpu().numpy()
    for b in range(2):
        assert np.array_equal(got[b], imgproc.resize_u8_host(img[b], (dst[1], dst[0]), area=True))


# ---- the engine on a full page against the float64 oracle --------------------------------------------------------------------
_TAPS = ("x1", "x2", "x3", "x4", "tunnel4", "tunnel3", "tunnel2", "pre")


def _oracle(oracle_memo, dtype):
    """The oracle on the engine's own page resizes (the INTER_AREA host twin, byte-equal to the device): the float64 restatement
    of the resize rounds a few exact .5 ties down, and one byte of input moves a u8 output by more than the rounding of the network."""
    from unittest import mock

    from manga_image_translator_amd import imgproc

    def run():
        g, f = O.weights()
        page = O.synth_color_page(7, 2048, 1456)
        taps = {}
        with mock.patch.object(O, "resize_area", lambda img, dsize: imgproc.resize_u8_host(img, dsize, area=True)):
            o = O.infer(g, f, page, 576, 30, dtype=dtype, taps=taps)
        o["taps"] = {k: v[0].permute(1, 2, 0).double() for k, v in taps.items()}
        return o
    return oracle_memo(("mc2_page", str(dtype)), run)


def _u8_rule(got, f64, bar):
    """u8 within 1 of the float64 truncation; a differing pixel only where the float64 value lies within ``bar`` (relative to the
    range 255) of a truncation boundary."""
    want = np.floor(f64).astype(np.int64)
    diff = got.astype(np.int64) - want
    assert np.abs(diff).max(initial=0) <= 1, (int((np.abs(diff) > 1).sum()), np.argwhere(np.abs(diff) > 1)[:4].tolist())
    frac = f64 - np.floor(f64)
    near = (frac < bar * 255) | (frac > 1 - bar * 255)
    assert not np.any((diff != 0) & ~near), int(((diff != 0) & ~near).sum())


def test_engine_taps_and_u8_against_float64(cuda, gemm_mode, oracle_memo):
    o64, o32 = _oracle(oracle_memo, torch.float64), _oracle(oracle_memo, torch.float32)
    eng = _engine(cuda, gemm_mode)
    page = O.synth_color_page(7, 2048, 1456)
    pt = torch.from_numpy(page).to(cuda)[None]
    plane, bgr = eng.denoise(pt, 30, bgr=True)
    taps = {}
    out = eng.forward(pt, 576, 30, taps=taps)
    torch.cuda.synchronize()
    _u8_rule(bgr[0].cpu().numpy(), np.asarray(o64["den_f"]), 2e-3)
    report = {}
    for k in _TAPS:
        ref, r32 = o64["taps"][k], o32["taps"][k]
        bar = max(2e-3, 4 * _rel(r32, ref))
        err = _rel(taps[k][0].cpu().double(), ref)
        report[k] = (err, bar)
    print("mc2 taps (rel err, bar):", {k: (f"{e:.2e}", f"{b:.2e}") for k, (e, b) in report.items()})
    for k, (err, bar) in report.items():
        assert err <= bar, (k, err, bar)
    assert tuple(out.shape) == (1, 811, 576, 3)
    _u8_rule(out[0].cpu().numpy(), o64["out_f"], report["pre"][1])


def test_batch_of_three_equals_three_single_runs(cuda, gemm_mode):
    eng = _engine(cuda, gemm_mode)
    pages = np.stack([O.synth_color_page(s, 420, 300) for s in (1, 2, 3)])
    pt = torch.from_numpy(pages).to(cuda)
    batch = eng.forward(pt, 256, 30)
    singles = [eng.forward(pt[i:i + 1], 256, 30) for i in range(3)]
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(batch[i], singles[i][0]), i


def test_plugin_against_the_reference_infer(cuda, gemm_mode):
    from PIL import Image

    from manga_image_translator_amd import plugins as P

    z = np.load(os.path.join(O.GOLDEN, "mc2_infer.npz"))
    g, f = O.weights()
    plug = P.HipMangaColorizer(weights={"generator": g, "denoiser": f})
    loop = asyncio.new_event_loop()
    loop.run_until_complete(plug.load("cuda"))
    for tag, *_ in O.INFER_CASES:
        page = z[f"page_{tag}"]
        res = loop.run_until_complete(plug.infer(Image.fromarray(page), int(z[f"size_{tag}"]), denoise_sigma=float(z[f"sigma_{tag}"]),
                                                 text_regions=None))
        got, want = np.asarray(res), z[f"out_{tag}"]
        assert got.shape == want.shape, (tag, got.shape, want.shape)
        o64 = O.infer(g, f, page, int(z[f"size_{tag}"]), float(z[f"sigma_{tag}"]), dtype=torch.float64)
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"mc2 plugin {tag}: max diff {diff.max()}, differing {(diff != 0).mean():.4f}")
        assert diff.max() <= 1 and (diff != 0).mean() <= 0.02, tag
        assert np.abs(got.astype(int) - np.floor(o64["out_f"]).astype(int)).max() <= 1, tag
    loop.run_until_complete(plug.unload())
