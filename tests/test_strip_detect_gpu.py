"""Webtoon strips through the detectors with the tiling on the device (csrc/rearrange.hip): the plugins' strip branch and the coupled
engine's, against the host composition they replace (rearrange.forward -> host box extraction -> host mask glue), which stays the
branch of every injected callable.  Integers and bytes are exact; box scores are within the 1 ulp tests/test_ctd_boxes_gpu.py allows
between the device extraction and the host routine."""
import asyncio

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

run = lambda c: asyncio.new_event_loop().run_until_complete(c)   # noqa: E731
TALL, WIDE = (2600, 160), (160, 2600)
D, T = 211, 6
DICTIONARY = ["<PAD>", "<S>", "</S>", "<SP>"] + [chr(0x4E00 + i) for i in range(D - 4)]


def _ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max(initial=0)


def _same_boxes(got, want, what):
    (gb, gs), (wb, ws) = got, want
    assert gb.shape == wb.shape and gs.shape == ws.shape, (what, gb.shape, wb.shape)
    assert np.array_equal(gb, wb), what
    assert _ulp(gs, ws) <= 1, (what, float(np.abs(gs - ws).max()))


def _same_lines(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a.pts), np.asarray(b.pts)), what
        assert _ulp([a.prob], [b.prob]) <= 1, (what, a.prob, b.prob)


def _strip(seed, hw):
    """(page, quads) of a synthetic strip; the wide one is the tall one transposed, so both hold the same text boxes."""
    from manga_image_translator_amd import synth

    page, quads, _ = synth.synth_page(seed, *TALL, n_boxes=6, disjoint=True)
    if hw == WIDE:
        return np.ascontiguousarray(np.transpose(page, (1, 0, 2))), np.asarray(quads)[..., ::-1]
    return page, np.asarray(quads)


def _stitched_hw(hw):
    from manga_image_translator_amd import rearrange as RA

    pl = RA.plan(*hw, 1024)
    _, pw, hh, _ = RA.stitch_geometry(pl, 1024)
    return (pw, hh) if pl.transpose else (hh, pw)


@pytest.mark.parametrize("hw", [TALL, WIDE], ids=["tall", "wide"])
def test_box_extraction_at_the_stitched_shape(cuda, hw):
    """The device box extraction on a map of the stitched geometry (1381 x 85: far from the page-shaped maps it has met so far) with
    the page's size as destination equals the host routine, for both detectors' parameters."""
    from manga_image_translator_amd import coupled, hostglue as HG

    page, quads = _strip(31, hw)
    mh, mw = _stitched_hw(hw)
    assert (mh, mw) == ((1381, 85) if hw == TALL else (85, 1381))
    prob, _ = coupled.synthetic_head_outputs(page, quads, (mh, mw))
    lm = np.zeros((1, 2, mh, mw), np.float32)
    lm[0, 0] = prob
    dev = torch.from_numpy(lm).to(cuda)
    want = HG.ctd_boxes(lm, *hw)
    assert len(want[0]) >= 3
    _same_boxes(HG.ctd_boxes_gpu(dev, *hw)[0], want, "ctd")
    for tt, bt, ur in ((0.5, 0.7, 2.3), (0.3, 0.6, 1.5)):
        _same_boxes(HG.dbnet_boxes_gpu(dev, *hw, tt, bt, ur)[0], HG.dbnet_boxes(lm, *hw, tt, bt, ur), f"dbnet {tt} {bt} {ur}")


@pytest.fixture(scope="module")
def plugins_loaded(cuda):
    from manga_image_translator_amd import pipeline, plugins as P

    weights = pipeline.synthetic_weights(dict_size=D)
    det = P.HipComicTextDetector(weights=weights)
    ocr = P.HipModel48pxOCR(weights=weights["ocr48"], dictionary=DICTIONARY)
    inp = P.HipLamaMPEInpainter(weights=weights)
    for p in (det, ocr, inp):
        run(p.load("cuda"))
    yield det, ocr, inp
    for p in (det, ocr, inp):
        run(p.unload())


class TrainedHead:
    """Stand-in for trained weights on strips: wraps ``engine.forward`` so that, AFTER the network has run, every square's line map and
    mask are replaced by that square's part of a synthetic trained-head map of its page (``coupled.synthetic_head_outputs`` at page
    size, cut and shrunk exactly like the page: channel 0 the shrink map, channel 1 the mask).  Squares are recognised by their bytes,
    so the wrapper serves the plugin's calls (one page) and the coupled engine's (squares of several pages in one batch) alike."""

    def __init__(self, engine, pages_quads, device):
        from manga_image_translator_amd import coupled, imgproc, rearrange as RA

        self.engine, self.plain, self.table = engine, engine.forward, {}
        for page, quads in pages_quads:
            H, W = page.shape[:2]
            prob, mask = coupled.synthetic_head_outputs(page, quads, (H, W))
            head = np.stack([(prob * 255).astype(np.uint8), mask, np.zeros_like(mask)], axis=-1)
            pl = RA.plan(H, W, 1024)
            resize = lambda a, ds: imgproc.resize_u8_host(a, ds)   # noqa: E731
            sq = RA.squares(page, pl, 1024, resize)[0]
            hd = RA.squares(head, pl, 1024, resize)[0].astype(np.float32) / np.float32(255)
            for s, h in zip(sq, hd):
                self.table[int(s.astype(np.int64).sum())] = (torch.from_numpy(h[..., 0].copy()).to(device), torch.from_numpy(h[..., 1].copy()).to(device))
        engine.forward = self

    def __call__(self, squares_u8, taps=None):
        m8, lines, pad = self.plain(squares_u8, taps)
        maps = [self.table[int(s.sum(dtype=torch.int64))] for s in squares_u8]
        lines[:, 0] = torch.stack([m[0] for m in maps])
        self.engine.last_mask_f32 = torch.stack([m[1] for m in maps])
        return m8, lines, pad

    def remove(self):
        self.engine.forward = self.plain


def _host_composition(det, page):
    """The strip branch as it was before the tiling ran on the device."""
    from manga_image_translator_amd import hostglue as HG, plugins as P, rearrange as RA

    H, W = page.shape[:2]
    lines_map, mask_f = RA.forward(page, det._tiles_forward, 1024)
    boxes, scores = P._native_ctd_boxes(lines_map, H, W)
    keep = scores > 0.6
    tls = [P._RefQuadrilateral(pts.astype(int), "", float(s)) for pts, s in zip(boxes[keep], scores[keep])]
    mask_u8 = (mask_f.squeeze() * 255).astype(np.uint8)                        # postprocess_mask (ctd.py:41-44)
    return tls, HG.refine_mask(page, HG.resize_linear_u8(mask_u8, (W, H)), tls, None)


@pytest.mark.parametrize("hw", [TALL, WIDE], ids=["tall", "wide"])
@pytest.mark.parametrize("head", ["random-init", "trained-head"])
def test_ctd_plugin_strip_stays_on_the_device(cuda, plugins_loaded, monkeypatch, hw, head):
    from manga_image_translator_amd import rearrange as RA

    det = plugins_loaded[0]
    page, quads = _strip(32, hw)
    wrap = TrainedHead(det.engine, [(page, quads)], cuda) if head == "trained-head" else None
    try:
        want_tls, want_mask = _host_composition(det, page)

        def refuse(*a, **k):
            raise AssertionError("the host tiling was taken")

        monkeypatch.setattr(RA, "forward", refuse)
        monkeypatch.setattr(RA, "squares", refuse)
        monkeypatch.setattr(RA, "stitch", refuse)
        tls, mask, extra = run(det.infer(page, 1024, 0.5, 0.7, 2.3))
    finally:
        if wrap:
            wrap.remove()
    assert extra is None and mask.dtype == np.uint8 and mask.shape == hw
    _same_lines(tls, want_tls, head)
    assert np.array_equal(mask, want_mask)
    if head == "trained-head":
        assert len(tls) >= 3 and mask.any()


@pytest.fixture(scope="module")
def default_pair(cuda):
    """(the detector with the host extractor injected: its host branch, the detector with nothing injected) on the same seeded weights."""
    from manga_image_translator_amd import dbnet_schema, plugins as P, synth

    sd = synth.synth_state_dict(dbnet_schema.text_detection_schema(), gain=1.2)
    pair = [P.HipDefaultDetector(weights=sd, boxes_from_maps=P._native_dbnet_boxes), P.HipDefaultDetector(weights=sd)]
    for d in pair:
        run(d.load("cuda"))
    yield pair
    for d in pair:
        run(d.unload())


@pytest.mark.parametrize("H,W,size", [(1400, 150, 320), (130, 1000, 192), (1400, 150, 256), (130, 1000, 256)])
def test_default_plugin_strip_equals_its_host_branch(cuda, default_pair, monkeypatch, H, W, size):
    """``HipDefaultDetector`` on a strip: the device branch against the host branch (forced by injecting the host extractor itself).
    ``DbnetEngine`` — like the reference's network, whose skip concatenations need it — takes sides that are multiples of 256 only, so
    at detect sizes 320 and 192 both branches end in the engine's refusal, the device one after its squares were made; the two cases at
    256 are the ones that compute maps."""
    from manga_image_translator_amd import rearrange as RA, synth

    assert RA.plan(H, W, size) is not None
    page = synth.synth_page(33, H, W, n_boxes=5)[0]
    outcome = []
    for det in default_pair:
        try:
            outcome.append(run(det.infer(page, size, 0.5, 0.7, 2.3)))
        except ValueError as e:
            outcome.append(str(e))
        monkeypatch.setattr(RA, "forward", None)      # the second detector must not take the host tiling
    host, dev = outcome
    if isinstance(host, str):
        assert size % 256 and "multiples of 256" in host and dev == host
        return
    assert size % 256 == 0 and not isinstance(dev, str)
    _same_lines(dev[0], host[0], "default")
    assert dev[1].dtype == np.uint8 and dev[1].std() > 0 and np.array_equal(dev[1], host[1]) and dev[2] is None


@pytest.fixture(scope="module")
def two_strips():
    return [_strip(34, TALL), _strip(35, TALL)]


def test_coupled_detect_on_strips_equals_the_plugin(cuda, plugins_loaded, two_strips):
    """Two different strips as one batch, their squares in ONE network call (ctd_mb = 16 > the reference's four): text lines and
    refined mask of every page are the plugin's, with the network's own maps and with the trained-head stand-in."""
    from manga_image_translator_amd import coupled

    det, ocr, inp = plugins_loaded
    pages_dev = torch.from_numpy(np.stack([p for p, _ in two_strips])).to(cuda)
    for head in ("random-init", "trained-head"):
        wrap = TrainedHead(det.engine, two_strips, cuda) if head == "trained-head" else None
        eng = coupled.CoupledPageEngine.from_engines(det.engine, ocr.engine, inp.engine, DICTIONARY, ctd_mb=16, host_workers=4)
        try:
            tls, refined = eng.detect(pages_dev)
            refined = refined.cpu().numpy()
            for k, (page, _) in enumerate(two_strips):
                want_tls, want_mask, _ = run(det.infer(page, 1024, 0.5, 0.7, 2.3))
                _same_lines(tls[k], want_tls, (head, k))
                assert np.array_equal(refined[k], want_mask), (head, k)
                if wrap:
                    assert len(tls[k]) >= 3
        finally:
            eng.close()
            if wrap:
                wrap.remove()


def test_coupled_run_on_two_strips_equals_two_runs_of_one(cuda, plugins_loaded, two_strips):
    """OCR, merge, mask refinement and LaMa (inpainting_size 2048) behind the strip detection: a batch of two equals one page at a time."""
    from manga_image_translator_amd import coupled

    det, ocr, inp = plugins_loaded
    pages_dev = torch.from_numpy(np.stack([p for p, _ in two_strips])).to(cuda)
    wrap = TrainedHead(det.engine, two_strips, cuda)
    eng = coupled.CoupledPageEngine.from_engines(det.engine, ocr.engine, inp.engine, DICTIONARY, ctd_mb=16, host_workers=4)
    kw = dict(max_seq_length=T, suppress_eos=True, prob_threshold=0.0, inpainting_size=2048)
    try:
        both = eng.run(pages_dev, **kw)
        torch.cuda.synchronize()
        assert both.mask.any() and all(len(t) >= 3 for t in both.textlines)
        for k in range(2):
            one = eng.run(pages_dev[k:k + 1], **kw)
            torch.cuda.synchronize()
            assert [(l.text, l.prob, np.asarray(l.pts).tolist()) for l in one.textlines[0]] == \
                   [(l.text, l.prob, np.asarray(l.pts).tolist()) for l in both.textlines[k]]
            assert [r.text for r in one.regions[0]] == [r.text for r in both.regions[k]]
            assert torch.equal(one.mask_raw[0], both.mask_raw[k]) and torch.equal(one.mask[0], both.mask[k])
            assert torch.equal(one.inpainted[0], both.inpainted[k])
    finally:
        eng.close()
        wrap.remove()
