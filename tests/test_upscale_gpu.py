"""The upscaler end to end on the device: ``EsrganEngine.upscale`` (pass loop + Pillow-exact resizes on the GPU), the plugin's batched
``_infer`` and the serving worker's ``config["upscale"]``, each against the engine's own ``forward`` bytes pushed through the REAL
Pillow in the reference's order (upscaling/common.py:10-33, esrgan_pytorch.py:537-549, manga_translator.py:626-629) — byte for byte."""
import asyncio

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

NB = 2
VALID = [2, 3, 4]


@pytest.fixture(scope="module")
def weights():
    from manga_image_translator_amd import esrgan_schema, synth

    return synth.synth_state_dict(esrgan_schema.rrdbnet_schema(NB))


@pytest.fixture(scope="module")
def engine(cuda, weights):
    from manga_image_translator_amd import esrgan

    return esrgan.EsrganEngine(weights, nb=NB, device=cuda)


def _pages(h, w, n, first=40):
    from manga_image_translator_amd import synth

    return [synth.synth_page(first + i, h, w, n_boxes=2)[0] for i in range(n)]


def _reference_order(engine, page: np.ndarray, upscale_ratio) -> Image.Image:
    """CommonUpscaler.upscale + ESRGANUpscalerPytorch._infer written out, the network being ``engine.forward`` on this one page."""
    img = Image.fromarray(page)
    ratio_left = upscale_ratio
    while ratio_left > 0:
        ratio = VALID[-1]
        for v in VALID:
            if ratio_left <= v:
                ratio = v
                break
        ratio_left -= ratio
        up = Image.fromarray(engine.forward(torch.from_numpy(np.array(img)).to(engine.device)[None])[0].cpu().numpy())
        r = ratio / 4
        img = up.resize(size=(int(round(up.size[0] * r)), int(round(up.size[1] * r))), resample=Image.Resampling.BILINEAR)
    if ratio_left < 0:
        d = (ratio + ratio_left) / ratio
        img = img.resize((int(img.size[0] * d), int(img.size[1] * d)))      # Pillow's default filter: BICUBIC
    return img


# (w, h) the reference returns for a 48 x 32 and a 40 x 24 page — ratio 5 is 4, then 2, then the correction by 0.5 (common.py:17-32)
SHAPES = {2: {(32, 48): (96, 64), (24, 40): (80, 48)}, 3: {(32, 48): (144, 96), (24, 40): (120, 72)},
          4: {(32, 48): (192, 128), (24, 40): (160, 96)}, 5: {(32, 48): (192, 128), (24, 40): (160, 96)}}


@pytest.mark.parametrize("ratio", [2, 3, 4, 5])
@pytest.mark.parametrize("hw", [(32, 48), (24, 40)], ids=["32x48", "24x40"])
def test_engine_upscale_equals_forward_through_pillow(engine, ratio, hw):
    page = _pages(hw[0], hw[1], 1)[0]
    got = engine.upscale(torch.from_numpy(page).to(engine.device)[None], ratio)
    want = _reference_order(engine, page, ratio)
    assert got.dtype == torch.uint8 and got.is_cuda
    assert tuple(got.shape) == (1, want.size[1], want.size[0], 3) and want.size == SHAPES[ratio][hw]
    assert np.array_equal(got[0].cpu().numpy(), np.asarray(want))


def test_engine_upscale_ratio_one_returns_the_input(engine):
    t = torch.from_numpy(_pages(24, 40, 1)[0]).to(engine.device)[None]
    assert engine.upscale(t, 1) is t


def test_plugin_batches_equal_sizes_and_keeps_order(cuda, weights):
    from manga_image_translator_amd import plugins as P

    run = lambda c: asyncio.new_event_loop().run_until_complete(c)
    up = P.HipESRGANUpscaler(weights=weights)
    run(up.load("cuda"))
    (a, a2), (b,) = _pages(32, 48, 2), _pages(24, 40, 1, first=50)
    calls = []
    fwd = up.engine.forward
    up.engine.forward = lambda x, *k, **kw: (calls.append(tuple(x.shape)), fwd(x, *k, **kw))[1]
    outs = run(up.infer([Image.fromarray(a), Image.fromarray(b), Image.fromarray(a2)], 2))
    assert sorted(calls) == [(1, 24, 40, 3), (2, 32, 48, 3)]                   # a and a2 went through ONE forward
    assert len(outs) == 3 and all(isinstance(o, Image.Image) and o.mode == "RGB" for o in outs)
    assert [o.size for o in outs] == [(96, 64), (80, 48), (96, 64)]
    for page, o in zip((a, b, a2), outs):
        single = run(up.infer([Image.fromarray(page)], 2))[0]
        assert np.array_equal(np.asarray(o), np.asarray(single))
        ref = Image.fromarray(fwd(torch.from_numpy(page).to(cuda)[None])[0].cpu().numpy())
        ref = ref.resize(size=(int(round(ref.size[0] * 0.5)), int(round(ref.size[1] * 0.5))), resample=Image.Resampling.BILINEAR)
        assert np.array_equal(np.asarray(o), np.asarray(ref))
    # micro-batches: at most MAX_LR_PIXELS low-resolution pixels per forward
    del calls[:]
    up.MAX_LR_PIXELS = 32 * 48
    outs2 = run(up.infer([Image.fromarray(a), Image.fromarray(b), Image.fromarray(a2)], 2))
    assert sorted(calls) == [(1, 24, 40, 3), (1, 32, 48, 3), (1, 32, 48, 3)]
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(outs, outs2))
    run(up.unload())


# ---- the serving worker -------------------------------------------------------------------------------------------------------------
H, W, D = 256, 320, 128      # the smallest page of the worker tests (tests/test_serve_batch_gpu.py)


@pytest.fixture(scope="module")
def stages(cuda):
    from manga_image_translator_amd import serve

    eng = serve.DenseStages({"dict_size": D, "esrgan_blocks": NB})
    loop = asyncio.new_event_loop()
    loop.run_until_complete(eng._load())
    yield eng, loop
    loop.close()


def _request():
    """A page and, in the UPSCALED frame (2H x 2W), text lines and the mask to inpaint: seeded detector weights fire on nothing."""
    from manga_image_translator_amd import synth

    page = synth.synth_page(60, H, W, n_boxes=3, disjoint=True)[0]
    _, quads, mask = synth.synth_page(61, 2 * H, 2 * W, n_boxes=3, disjoint=True)
    cfg = {"textlines": np.asarray(quads).tolist(), "mask": mask, "ocr": {"max_seq_length": 8, "suppress_eos": True, "prob": 0.0},
           "inpainter": {"inpainting_size": 512}}
    return page, cfg


def test_worker_upscales_first_and_reverts(stages):
    eng, loop = stages
    page, cfg = _request()
    assert eng.up is None                                                      # loaded by the first request that asks for it
    r = loop.run_until_complete(eng.translate(page, {**cfg, "upscale": {"upscale_ratio": 2}}))
    assert eng.up is not None and eng.up.engine.nb == NB
    assert r["inpainted"].shape == (2 * H, 2 * W, 3) and r["mask"].shape == (2 * H, 2 * W) and r["mask_raw"].shape == (2 * H, 2 * W)
    assert r["inpainted"].dtype == np.uint8
    upscaled = eng.up.engine.upscale(torch.from_numpy(page).to(eng.up.engine.device)[None], 2)[0].cpu().numpy()
    assert not np.array_equal(r["inpainted"], upscaled) and np.array_equal(r["inpainted"][r["mask"] < 127], upscaled[r["mask"] < 127])
    back = loop.run_until_complete(eng.translate(page, {**cfg, "upscale": {"upscale_ratio": 2, "revert_upscaling": True}}))
    assert back["inpainted"].shape == (H, W, 3) and back["mask"].shape == (2 * H, 2 * W)
    assert np.array_equal(back["inpainted"], np.asarray(Image.fromarray(r["inpainted"]).resize((W, H))))


def test_worker_without_the_key_is_unchanged(stages):
    eng, loop = stages
    from manga_image_translator_amd import synth

    page, quads, mask = synth.synth_page(62, H, W, n_boxes=3, disjoint=True)
    cfg = {"textlines": np.asarray(quads).tolist(), "mask": mask, "ocr": {"max_seq_length": 8, "suppress_eos": True, "prob": 0.0},
           "inpainter": {"inpainting_size": 512}}
    plain = loop.run_until_complete(eng.translate(page, cfg))
    for empty in ({"upscale": {}}, {"upscale": {"upscale_ratio": 0, "revert_upscaling": True}}, {"upscale": None}):
        other = loop.run_until_complete(eng.translate(page, {**cfg, **empty}))
        assert set(other) == set(plain) and other["textlines"] == plain["textlines"]
        for k in ("inpainted", "mask", "mask_raw"):
            assert other[k].shape == plain[k].shape and np.array_equal(other[k], plain[k])
    assert plain["inpainted"].shape == (H, W, 3) and not np.array_equal(plain["inpainted"], page)


def test_batch_request_with_upscaling_takes_the_page_loop(stages):
    eng, loop = stages
    page, cfg = _request()
    cfg = {**cfg, "upscale": {"upscale_ratio": 2}}
    b0, l0 = eng.pages_batched, eng.pages_looped
    got = loop.run_until_complete(eng.translate_batch([page, page.copy()], cfg, batch_size=2))
    assert eng.pages_looped - l0 == 2 and eng.pages_batched - b0 == 0
    assert eng.last_batch_plan == [([0], "upscale"), ([1], "upscale")]
    assert len(got) == 2 and all(g["inpainted"].shape == (2 * H, 2 * W, 3) for g in got)
    assert np.array_equal(got[0]["inpainted"], got[1]["inpainted"])
