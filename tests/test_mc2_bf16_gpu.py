"""The mc2 colorizer's bf16 precision on the MI355X, with seeded weights (``_mc2_oracle.weights()``).

Accuracy, by the yardstick the LaMa, ESRGAN and AOT bf16 precisions merged against: FFDNet and the generator, each on a fixed input
(tests/_mc2_bf16_cases.py — two 37 x 51 pages; planes of 64 x 48 and 96 x 64, B = 2), against the float64 oracle; the mean error must
not exceed that of the same oracle under ``torch.autocast("cpu", bfloat16)``, and neither must the max: tests/test_mc2_precision.py
shows on these very inputs that rounding the convolution operands alone stays below 0.8 of autocast's max on every case (0.48 .. 0.66),
so the engine's fp32 accumulation has the remaining fifth to spend.  The error must also exceed 1e-6: the mode provably ran.
The u8 plane and the u8 image move against the fp32 engine by no more levels than the autocast oracle moves against the fp32 oracle.

Then what the other three engines' precisions promise: fp32 bytes untouched before and after a bf16 call, bf16 deterministic,
batch-independent and the same after ``release_workspace()``, packs built at the first bf16 call, the plugin's option and
``MIT_MC2_PRECISION``, ``ValueError`` on another value."""
import asyncio

import numpy as np
import pytest
import torch

import _mc2_bf16_cases as K
import _mc2_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def weights():
    return O.weights()


@pytest.fixture(scope="module")
def eng(weights):
    """An fp32 engine (the default) whose bf16 calls name the precision."""
    from manga_image_translator_amd import mc2, ops

    with ops.gemm_mode(6):
        return mc2.Mc2Engine(*weights, device=torch.device("cuda:0"))


def _moved(a, b):
    return int(np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)).max())


def _judge(what, got, r):
    truth = r["f64"]
    (gm, gx), (am, ax) = K.errors(got, truth), K.errors(r["autocast"], truth)
    print(f"{what}: engine mean {gm:.3e} max {gx:.3e}; autocast mean {am:.3e} max {ax:.3e}; ratios {gm / am:.3f} {gx / ax:.3f}")
    assert gm > 1e-6, (what, gm)
    assert gm <= am, (what, gm, am)
    assert gx <= ax, (what, gx, ax)


def test_ffdnet_error_is_below_the_autocast_oracle_s(cuda, eng, weights, oracle_memo):
    pages = K.ffd_pages()
    pt = torch.from_numpy(pages).to(cuda)
    taps = {}
    plane, bgr = eng.denoise(pt, K.SIGMA, bgr=True, precision="bf16", taps=taps)
    plane32, bgr32 = eng.denoise(pt, K.SIGMA, bgr=True, precision="fp32")
    torch.cuda.synchronize()
    assert tuple(taps["ffd_noise"].shape) == (2, 19, 26, 12) and torch.equal(plane, bgr[..., 0])
    for b in range(2):
        r = oracle_memo(("mc2_bf16_ffd", b), lambda: {m: K.ffd_oracle(weights[1], pages[b], m) for m in ("f64", "f32", "autocast")})
        _judge(f"FFDNet noise, page {b}", taps["ffd_noise"][b].cpu(), {m: v["noise"] for m, v in r.items()})
        allowed = _moved(r["autocast"]["bgr"], r["f32"]["bgr"])
        got = _moved(bgr[b].cpu().numpy(), bgr32[b].cpu().numpy())
        print(f"FFDNet u8, page {b}: bf16 engine moves {got} level(s) against the fp32 engine; autocast moves {allowed}")
        assert got <= allowed, (b, got, allowed)


@pytest.mark.parametrize("tag", [c[0] for c in K.GEN_CASES])
def test_generator_error_is_below_the_autocast_oracle_s(cuda, eng, weights, oracle_memo, tag):
    planes = K.gen_planes(tag)
    pt = torch.from_numpy(planes).to(cuda)
    taps = {}
    out = eng.colorize(pt, taps, precision="bf16")
    out32 = eng.colorize(pt, precision="fp32")
    torch.cuda.synchronize()
    r = oracle_memo(("mc2_bf16_gen", tag), lambda: {m: K.gen_oracle(weights[0], planes, m) for m in ("f64", "f32", "autocast")})
    assert tuple(taps["pre"].shape) == tuple(r["f64"]["pre"].shape)
    _judge(f"generator pre, {tag}", taps["pre"].cpu(), {m: v["pre"] for m, v in r.items()})
    allowed = _moved(r["autocast"]["out"], r["f32"]["out"])
    got = _moved(out.cpu().numpy(), out32.cpu().numpy())
    print(f"generator u8, {tag}: bf16 engine moves {got} level(s) against the fp32 engine; autocast moves {allowed}")
    assert got <= allowed, (tag, got, allowed)


def _pages():
    """Two pages of one size for ``forward`` (INFER_CASES' landscape geometry: 150 x 230 at size 128, sigma 30)."""
    return np.stack([O.synth_color_page(s, 150, 230) for s in (51, 52)])


def test_fp32_is_untouched_and_packs_are_lazy(cuda, eng, weights):
    from manga_image_translator_amd import mc2, ops

    pt = torch.from_numpy(_pages()).to(cuda)
    with ops.gemm_mode(6):
        fresh = mc2.Mc2Engine(*weights, device=cuda)
    assert fresh.precision == "fp32" and fresh.ffd16 is None                      # no bf16 packs for an fp32 user
    before = fresh.forward(pt, 128, 30).clone()
    assert fresh.ffd16 is None
    low = fresh.forward(pt, 128, 30, precision="bf16").clone()
    assert fresh.ffd16 is not None and len(fresh.ffd16) == 11                     # built by the first bf16 call
    after = fresh.forward(pt, 128, 30)
    other = eng.forward(pt, 128, 30, precision="fp32")
    torch.cuda.synchronize()
    assert torch.equal(before, after) and torch.equal(before, other)              # fp32 bytes: before, after, another engine
    assert not torch.equal(low, before)                                           # and the bf16 call was another computation
    assert torch.equal(low, eng.forward(pt, 128, 30, precision="bf16"))           # the same on both engines
    with ops.gemm_mode(6):
        born = mc2.Mc2Engine(*weights, device=cuda, precision="bf16")
    assert born.ffd16 is not None                                                 # at construction for a bf16 engine
    assert torch.equal(born.forward(pt, 128, 30), low)                            # None = the engine's own setting
    assert torch.equal(born.forward(pt, 128, 30, precision="fp32"), before)


def test_bf16_is_deterministic_batch_independent_and_survives_release(cuda, eng):
    pt = torch.from_numpy(_pages()).to(cuda)
    both = eng.forward(pt, 128, 30, precision="bf16").clone()
    again = eng.forward(pt, 128, 30, precision="bf16").clone()
    singles = [eng.forward(pt[i:i + 1], 128, 30, precision="bf16").clone() for i in range(2)]
    eng.release_workspace()
    released = eng.forward(pt, 128, 30, precision="bf16")
    torch.cuda.synchronize()
    assert torch.equal(both, again) and torch.equal(both, released)
    for i in range(2):
        assert torch.equal(both[i], singles[i][0]), i
    plane = eng.denoise(pt, 30, precision="bf16")
    for i in range(2):
        assert torch.equal(plane[i], eng.denoise(pt[i:i + 1], 30, precision="bf16")[0]), i


def test_plugin_follows_its_option_and_the_environment(cuda, eng, weights, monkeypatch):
    from PIL import Image

    from manga_image_translator_amd import plugins as P

    page = _pages()[0]
    pt = torch.from_numpy(np.concatenate([page, np.full(page.shape[:2] + (1,), 255, np.uint8)], -1)).to(cuda)[None]
    want = {p: eng.forward(pt, 128, 30, precision=p)[0].cpu().numpy() for p in ("fp32", "bf16")}
    assert not np.array_equal(want["fp32"], want["bf16"])
    loop = asyncio.new_event_loop()
    w = {"generator": weights[0], "denoiser": weights[1]}
    monkeypatch.delenv("MIT_MC2_PRECISION", raising=False)
    for kw, env, expect in (({"precision": "bf16"}, None, "bf16"), ({}, "bf16", "bf16"), ({"precision": "fp32"}, "bf16", "fp32")):
        if env is not None:
            monkeypatch.setenv("MIT_MC2_PRECISION", env)
        plug = P.HipMangaColorizer(weights=dict(w), **kw)
        loop.run_until_complete(plug.load("cuda"))
        assert plug.precision == expect and plug.engine.precision == expect
        got = np.asarray(loop.run_until_complete(plug.infer(Image.fromarray(page), 128, denoise_sigma=30, text_regions=None)))
        assert np.array_equal(got, want[expect]), (kw, env)


def test_another_precision_is_a_value_error(cuda, eng, weights):
    from manga_image_translator_amd import mc2

    pt = torch.from_numpy(_pages()).to(cuda)
    with pytest.raises(ValueError, match="precision"):
        eng.forward(pt, 128, 30, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        eng.denoise(pt, 30, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        eng.colorize(pt[..., 0], precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        mc2.Mc2Engine(*weights, device=cuda, precision="fp16")
