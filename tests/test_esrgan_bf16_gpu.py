"""The upscaler's opt-in bf16 precision on the GPU.

Yardstick: ``oracle.esrgan.rrdbnet_forward`` in fp32 is the truth, the same function under ``torch.autocast("cpu", bfloat16)`` is
the reference's own reduced-precision run.  The engine's bf16 precision rounds nothing but convolution operands (the residual trunk
stays fp32), so on ``taps["out_float"]`` its mean and its max absolute error against the truth must be no larger than the autocast
run's on the same input — the criterion of tests/test_lama_bf16_gpu.py.  No element-wise comparison with an emulation of the mode:
rounding to bf16 is chaotic (that file says why).

An emulation of the mode on the oracle (every convolution rounds its operands, nothing else is rounded) measured, against autocast:
nb = 2 mean 4.2e-4 vs 8.9e-4, max 4.0e-3 vs 6.2e-3; nb = 4 mean 5.9e-4 vs 1.1e-3, max 4.5e-3 vs 8.3e-3; nb = 23 mean 1.18e-2 vs
2.58e-2, max 0.128 vs 0.278 — a margin of about 2x on every case."""
import asyncio

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {"nb2": (2, 2, 24, 40), "nb4": (4, 1, 37, 51), "nb23": (23, 1, 32, 40)}
_MEMO = {}


def _setup(name, cuda):
    """Weights, pages, the oracle's fp32 and autocast outputs (RGB NHWC float, like taps["out_float"]) and an engine: once per case."""
    if name in _MEMO:
        return _MEMO[name]
    from manga_image_translator_amd import esrgan, esrgan_schema, synth
    from oracle import esrgan as OE

    nb, B, H, W = CASES[name]
    sd = synth.synth_state_dict(esrgan_schema.rrdbnet_schema(nb))
    pages = np.stack([synth.synth_page(20 + i, H, W, n_boxes=2)[0] for i in range(B)])
    x = torch.from_numpy(pages[..., ::-1].copy()).float().div(255.0).permute(0, 3, 1, 2)      # BGR planes
    with torch.no_grad():
        truth = OE.rrdbnet_forward(sd, x, nb)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ac = OE.rrdbnet_forward(sd, x, nb).float()
    to_rgb_nhwc = lambda t: t.flip(1).permute(0, 2, 3, 1).contiguous()
    eng = esrgan.EsrganEngine(sd, nb=nb, device=cuda)
    _MEMO[name] = dict(nb=nb, sd=sd, pages=pages, truth=to_rgb_nhwc(truth), autocast=to_rgb_nhwc(ac), eng=eng,
                       dev=torch.from_numpy(pages).to(cuda))
    return _MEMO[name]


def _u8(y):
    return (y.clip(0, 1).numpy() * 255.0).astype(np.uint8)


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_error_is_within_the_autocast_run_s(cuda, name):
    c = _setup(name, cuda)
    taps = {}
    out = c["eng"].forward(c["dev"], taps=taps, precision="bf16")
    torch.cuda.synchronize()
    got = taps["out_float"].cpu()
    assert got.shape == c["truth"].shape and bool(torch.isfinite(got).all())
    e, a = (got - c["truth"]).abs(), (c["autocast"] - c["truth"]).abs()
    print(f"{name}: engine bf16 mean {e.mean().item():.3e} max {e.max().item():.3e} | autocast mean {a.mean().item():.3e} max {a.max().item():.3e}")
    assert e.mean().item() <= a.mean().item() and e.max().item() <= a.max().item(), (e.mean().item(), a.mean().item(), e.max().item(), a.max().item())
    assert e.mean().item() > 1e-6                     # the reduced precision did run: this is not the fp32 engine under another name
    if name != "nb23":                                # (the seeded nb = 23 weights give an output range of +-19: float output only)
        out32 = c["eng"].forward(c["dev"]).cpu().numpy().astype(np.int32)
        lv_e = int(np.abs(out.cpu().numpy().astype(np.int32) - out32).max())
        lv_a = int(np.abs(_u8(c["autocast"]).astype(np.int32) - _u8(c["truth"]).astype(np.int32)).max())
        print(f"{name}: u8 levels vs fp32: engine {lv_e}, autocast oracle {lv_a}")
        assert lv_e <= lv_a, (lv_e, lv_a)


def test_fp32_is_untouched_and_bf16_is_deterministic(cuda):
    from manga_image_translator_amd import esrgan

    c = _setup("nb2", cuda)
    eng, x = c["eng"], c["dev"]
    a = eng.forward(x).cpu()
    b16 = eng.forward(x, precision="bf16").cpu()
    assert torch.equal(a, eng.forward(x, precision="fp32").cpu()) and torch.equal(a, eng.forward(x).cpu())   # also after a bf16 call
    assert torch.equal(a, esrgan.EsrganEngine(c["sd"], nb=c["nb"], device=cuda).forward(x).cpu())
    assert not torch.equal(a, b16)
    for i in range(x.shape[0]):                       # B = 2 equals the two pages run alone
        assert torch.equal(eng.forward(x[i:i + 1], precision="bf16").cpu()[0], b16[i]), i
    eng.release_workspace()
    assert torch.equal(eng.forward(x, precision="bf16").cpu(), b16)
    e16 = esrgan.EsrganEngine(c["sd"], nb=c["nb"], device=cuda, precision="bf16")        # the engine's own precision
    assert e16.blocks_bf16 is not None and eng.precision == "fp32"
    assert torch.equal(e16.forward(x).cpu(), b16) and torch.equal(e16.forward(x, precision="fp32").cpu(), a)
    with pytest.raises(ValueError):
        eng.forward(x, precision="fp16")
    with pytest.raises(ValueError):
        esrgan.EsrganEngine(c["sd"], nb=c["nb"], device=cuda, precision="half")


def test_bf16_packs_are_built_lazily_for_an_fp32_engine(cuda):
    from manga_image_translator_amd import esrgan

    c = _setup("nb2", cuda)
    eng = esrgan.EsrganEngine(c["sd"], nb=c["nb"], device=cuda)
    assert eng.blocks_bf16 is None
    eng.forward(c["dev"])
    assert eng.blocks_bf16 is None                    # an fp32 user pays no memory for them
    eng.forward(c["dev"], precision="bf16")
    assert eng.blocks_bf16 is not None and len(eng.blocks_bf16) == c["nb"]


def test_plugin_and_upscale_follow_the_precision(cuda, monkeypatch):
    from PIL import Image

    from manga_image_translator_amd import esrgan, imgproc, plugins as P

    run = lambda co: asyncio.new_event_loop().run_until_complete(co)
    c = _setup("nb2", cuda)
    page = c["pages"][0]
    h, w = page.shape[:2]
    x = c["dev"][:1]
    want16 = imgproc.pil_resize_u8(c["eng"].forward(x, precision="bf16"), (2 * w, 2 * h), "bilinear")[0].cpu().numpy()
    want32 = imgproc.pil_resize_u8(c["eng"].forward(x), (2 * w, 2 * h), "bilinear")[0].cpu().numpy()
    assert not np.array_equal(want16, want32)
    monkeypatch.delenv("MIT_ESRGAN_PRECISION", raising=False)
    by_arg = P.HipESRGANUpscaler(weights=c["sd"], precision="bf16")
    monkeypatch.setenv("MIT_ESRGAN_PRECISION", "bf16")
    by_env = P.HipESRGANUpscaler(weights=c["sd"])
    fp32_arg = P.HipESRGANUpscaler(weights=c["sd"], precision="fp32")
    monkeypatch.delenv("MIT_ESRGAN_PRECISION")
    for up, want in ((by_arg, want16), (by_env, want16), (fp32_arg, want32)):
        run(up.load("cuda"))
        outs = run(up.infer([Image.fromarray(page)], 2))
        assert len(outs) == 1 and outs[0].size == (2 * w, 2 * h)      # 4x then x0.5 through PIL (esrgan_pytorch.py:546)
        assert np.array_equal(np.asarray(outs[0]), want)
        run(up.unload())
    # upscale(): every pass in the engine's precision (ratio 3 is one pass of 3; ratio 6 is a pass of 4 and a pass of 2), or the call's
    e16 = esrgan.EsrganEngine(c["sd"], nb=c["nb"], device=cuda, precision="bf16")
    small = x[:, :8, :12].contiguous()
    for ratio in (3, 6):
        passes, correction = esrgan.upscale_plan(12, 8, ratio)
        assert len(passes) == (1 if ratio == 3 else 2) and correction is None
        want, want_fp32 = small, small
        for _, size in passes:
            want = imgproc.pil_resize_u8(c["eng"].forward(want, precision="bf16"), size, "bilinear")
            want_fp32 = imgproc.pil_resize_u8(c["eng"].forward(want_fp32), size, "bilinear")
        assert torch.equal(e16.upscale(small, ratio), want) and torch.equal(c["eng"].upscale(small, ratio, precision="bf16"), want)
        assert torch.equal(c["eng"].upscale(small, ratio), want_fp32) and not torch.equal(want, want_fp32)
