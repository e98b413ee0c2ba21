"""The coupled page path with a DBNet detector and an inpainter of either other kind (``CoupledPageEngine.from_engines`` over a
``DbnetEngine``, the 48px OCR and an 18-block ``lama_large`` or the AOT engine) against the same chain through the drop-in plugins one
page at a time: HipDefaultDetector -> HipModel48pxOCR -> text-line merge -> mask refinement -> HipLamaLargeInpainter / HipAotInpainter.
A trained head is stood in for on both sides by coupled.synthetic_head_outputs at the network's map size (tests/_dbnet_pages.py).

Two page shapes at detect_size 256: 320 x 200 (network page 256 x 160 padded to 256 x 256: ``pad_w`` = 96, the mask is cropped on the
right) and 200 x 320 (``pad_h`` = 96, cropped at the bottom).  The plugin chain is computed once per shape and shared."""
import asyncio
import warnings

import numpy as np
import pytest
import torch

from tests._dbnet_pages import head_maps, small_page

pytestmark = pytest.mark.gpu

T, D, SIZE = 6, 211, 256
DET = dict(detect_size=SIZE, text_threshold=0.5, box_threshold=0.7, unclip_ratio=1.5)   # (the head helper's shrink is solved for 1.5)


@pytest.fixture(scope="module")
def world(cuda):
    """The loaded plugins (seeded weights), and per page shape: pages, injected maps, and the plugin chain's results page by page."""
    from manga_image_translator_amd import aot_schema, dbnet_schema, lama_schema, mask_refinement as MR, ocr_schema, plugins as P, synth
    from manga_image_translator_amd import textline_merge as TM

    run = asyncio.new_event_loop().run_until_complete
    dictionary = ["<PAD>", "<S>", "</S>", "<SP>"] + [chr(0x4E00 + i) for i in range(D - 4)]
    det = P.HipDefaultDetector(weights=synth.synth_state_dict(dbnet_schema.text_detection_schema(), gain=1.2))
    ocr = P.HipModel48pxOCR(weights=synth.synth_state_dict(ocr_schema.ocr48_schema(D)), dictionary=dictionary)
    large = P.HipLamaLargeInpainter(weights={"lama.gen": synth.synth_state_dict(lama_schema.lama_generator_schema(18))})
    aot = P.HipAotInpainter(weights={"aot": synth.synth_state_dict(aot_schema.aot_generator_schema())})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for p in (det, ocr, large, aot):
            run(p.load("cuda"))
    plain = det.engine.forward
    cur = {}

    def fwd(pages_u8, taps=None):     # the plugin's network call with the stand-in maps laid over its outputs, as ``inject`` does
        db, _ = plain(pages_u8, taps)
        db[:, 0] = cur["prob"]
        return db, cur["mask"]

    class Cfg:
        prob = 0.0

    shapes = {}
    for name, (H, W) in (("pad_w", (320, 200)), ("pad_h", (200, 320))):
        gen = [small_page(60 + i, H, W) for i in range(3)]
        maps = [head_maps(p, q, SIZE) for p, q in gen]
        inj = {"prob": torch.from_numpy(np.stack([m[0] for m in maps])).to(cuda), "mask": torch.from_numpy(np.stack([m[1] for m in maps])).to(cuda)}
        chain = []
        det.engine.forward = fwd
        for k, (page, _) in enumerate(gen):
            cur["prob"], cur["mask"] = inj["prob"][k:k + 1], inj["mask"][k:k + 1]
            tls, raw, _ = run(det.infer(page, SIZE, 0.5, 0.7, 1.5))
            lines = [l for l in run(ocr.infer(page, tls, Cfg(), False, 0, T, True)) if l.text.strip()]
            regions = TM.dispatch_sync(lines, W, H)
            mask = MR.dispatch_sync(regions, page, raw, "fit_text", 20, 0, False, 3)
            chain.append(dict(lines=lines, regions=regions, raw=raw, mask=mask,
                              large=np.asarray(run(large.infer(page, mask, None, max(H, W)))).astype(np.uint8),
                              aot=np.asarray(run(aot.infer(page, mask, None, max(H, W)))).astype(np.uint8)))
        det.engine.forward = plain
        shapes[name] = dict(H=H, W=W, pages=[g[0] for g in gen], pages_dev=torch.from_numpy(np.stack([g[0] for g in gen])).to(cuda), inj=inj,
                            chain=chain)
    yield dict(det=det, ocr=ocr, large=large, aot=aot, dictionary=dictionary, shapes=shapes)
    for p in (det, ocr, large, aot):
        run(p.unload())


def _equals_chain(res, s, inpainter: str):
    for k, want in enumerate(s["chain"]):
        got = res.textlines[k]
        assert len(got) == len(want["lines"]) >= 1               # every page yields at least one line
        for a, b in zip(got, want["lines"]):
            assert np.array_equal(np.asarray(a.pts), np.asarray(b.pts)) and a.text == b.text and a.prob == pytest.approx(b.prob, rel=1e-6)
            assert (a.fg_r, a.fg_g, a.fg_b, a.bg_r, a.bg_g, a.bg_b) == (b.fg_r, b.fg_g, b.fg_b, b.bg_r, b.bg_g, b.bg_b)
        assert [r.text for r in res.regions[k]] == [r.text for r in want["regions"]]
        raw = res.mask_raw[k].cpu().numpy()
        assert raw.shape == want["raw"].shape and np.array_equal(raw, want["raw"]), int((raw != want["raw"]).sum())
        assert np.array_equal(res.mask[k].cpu().numpy(), want["mask"]), int((res.mask[k].cpu().numpy() != want["mask"]).sum())
        assert np.array_equal(res.inpainted[k].cpu().numpy(), want[inpainter])
        assert want["mask"].any() and not np.array_equal(want[inpainter], s["pages"][k])


def _same_run(a, b):
    assert torch.equal(a.mask, b.mask) and torch.equal(a.inpainted, b.inpainted) and torch.equal(a.mask_raw, b.mask_raw)
    assert [[(l.text, l.prob, np.asarray(l.pts).tolist()) for l in t] for t in a.textlines] == \
           [[(l.text, l.prob, np.asarray(l.pts).tolist()) for l in t] for t in b.textlines]


@pytest.mark.parametrize("shape", ["pad_w", "pad_h"])
def test_dbnet_and_lama_large_batch_equals_the_plugin_chain(world, shape):
    from manga_image_translator_amd import coupled

    s = world["shapes"][shape]
    H, W = s["H"], s["W"]
    eng = coupled.CoupledPageEngine.from_engines(world["det"].engine, world["ocr"].engine, world["large"].engine, world["dictionary"],
                                                 ctd_mb=2, lama_mb=2, host_workers=4)
    assert eng.dbnet and eng.takes_strips is False
    kw = dict(max_seq_length=T, suppress_eos=True, prob_threshold=0.0, inject=s["inj"], inpainting_size=max(H, W), **DET)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        res = eng.run(s["pages_dev"], **kw)
        torch.cuda.synchronize()
        piped = eng.run(s["pages_dev"], group=1, **kw)      # three pipeline slots of one page
        torch.cuda.synchronize()
        # the raw mask has the detector's own size: the 256 x 256 map less the padding on ONE side (default.py:91-94)
        assert tuple(res.mask_raw.shape) == ((3, 256, 160) if shape == "pad_w" else (3, 160, 256)) and res.mask_raw.dtype == torch.uint8
        _same_run(piped, res)
        _equals_chain(res, s, "large")
        # a request's page-sized raw mask for ONE page: that page starts from it, the others from the detector's, and the masks come
        # back per page
        given = np.zeros((H, W), np.uint8)
        q = s["chain"][0]["lines"][0].pts
        given[q[:, 1].min():q[:, 1].max(), q[:, 0].min():q[:, 0].max()] = 255
        for group in (None, 1):
            mixed = eng.run(s["pages_dev"], mask_raw=[given, None, None], group=group, **kw)
            torch.cuda.synchronize()
            assert isinstance(mixed.mask_raw, list) and [tuple(m.shape) for m in mixed.mask_raw] == [(H, W)] + [tuple(res.mask_raw.shape[1:])] * 2
            assert np.array_equal(mixed.mask_raw[0].cpu().numpy(), given)
            assert all(torch.equal(mixed.mask_raw[k], res.mask_raw[k]) and torch.equal(mixed.mask[k], res.mask[k]) for k in (1, 2))
            assert torch.equal(mixed.inpainted[1:], res.inpainted[1:]) and mixed.mask[0].any()
    eng.close()


def test_dbnet_and_the_aot_inpainter_batch_equals_the_plugin_chain(world):
    from manga_image_translator_amd import coupled

    s = world["shapes"]["pad_w"]
    eng = coupled.CoupledPageEngine.from_engines(world["det"].engine, world["ocr"].engine, world["aot"].engine, world["dictionary"],
                                                 ctd_mb=2, lama_mb=2, host_workers=4)
    kw = dict(max_seq_length=T, suppress_eos=True, prob_threshold=0.0, inject=s["inj"], inpainting_size=max(s["H"], s["W"]), **DET)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        res = eng.run(s["pages_dev"], **kw)
        torch.cuda.synchronize()
        piped = eng.run(s["pages_dev"], group=1, **kw)
        torch.cuda.synchronize()
    _same_run(piped, res)
    _equals_chain(res, s, "aot")
    eng.close()


def test_a_dbnet_strip_is_refused_not_mis_served(world):
    from manga_image_translator_amd import coupled

    eng = coupled.CoupledPageEngine.from_engines(world["det"].engine, world["ocr"].engine, world["large"].engine, world["dictionary"])
    strip = torch.zeros(1, 1200, 96, 3, dtype=torch.uint8, device=world["shapes"]["pad_w"]["pages_dev"].device)
    with pytest.raises(NotImplementedError, match="strips"):
        eng.run(strip, **DET)
    eng.close()
