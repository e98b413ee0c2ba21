"""``dbconvnext`` detector parity: the HIP engine against the reference module's recorded outputs (tests/golden/dbconvnext.npz) and the CPU
restatement (tests/_dbconvnext_oracle.py), then the plugin round it.

Tolerance: post-sigmoid maps at 2e-4 absolute, the project's bar for its detector maps (test_dbnet_gpu.py); the thresholded bitmap
``db[:, 0] > 0.5`` must agree outside a 2e-4 margin of the threshold; taps at 1e-3 of each tap's own range.  The fixture's float32
reference is within 2.1e-6 of its float64 run (recorded in the fixture), so the bar measures the engine."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _dbconvnext_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

run = lambda c: asyncio.new_event_loop().run_until_complete(c)  # noqa: E731


@pytest.fixture(scope="module")
def sd():
    return O.weights()


@pytest.fixture(scope="module")
def golden():
    return np.load(O.FIXTURE)


@pytest.fixture(scope="module")
def engine(cuda, sd, shipped_mode):
    from manga_image_translator_amd import dbconvnext

    with shipped_mode():
        return dbconvnext.DbconvnextEngine(sd, device=cuda)


@pytest.fixture(scope="module")
def plugin(cuda, sd, shipped_mode):
    """One loaded plugin for the plugin tests (a load packs 140 M parameters); a test that injects steps sets them for its own duration."""
    from manga_image_translator_amd import plugins as P

    det = P.HipDBConvNextDetector(weights=sd)
    with shipped_mode():
        run(det.load("cuda"))
    yield det
    run(det.unload())


def _forward(engine, cuda, pages, taps=None):
    db, mask = engine.forward(torch.from_numpy(pages).to(cuda), taps)
    torch.cuda.synchronize()
    return db.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("tag", [t for t, *_ in O.CASES])
def test_engine_parity(cuda, engine, golden, gemm_mode, tag):
    pg = golden[f"page_{tag}"]
    taps = {}
    db, mask = _forward(engine, cuda, pg[None], taps)
    H, W = pg.shape[:2]
    assert db.shape == (1, 2, H, W) and mask.shape == (1, H // 2, W // 2)
    rdb, rmask = golden[f"db_{tag}"], golden[f"mask_{tag}"]
    e1, e2 = np.abs(db[:, :, ::2, ::2] - rdb).max(), np.abs(mask - rmask[:, 0]).max()
    print(f"dbconvnext parity [{tag}, mode {gemm_mode}]: db {e1:.3g} mask {e2:.3g}")
    assert e1 <= 2e-4 and e2 <= 2e-4, (e1, e2)
    near = np.abs(rdb[:, 0] - 0.5) < 2e-4
    assert near.mean() <= 0.01
    assert np.array_equal((db[:, 0, ::2, ::2] > 0.5)[~near], (rdb[:, 0] > 0.5)[~near])
    for k in O.TAPS:
        ref = golden[f"{k}_{tag}"]
        e = np.abs(O.sub_tap(k, taps[k].cpu().numpy()) - ref).max() / (ref.max() - ref.min())
        print(f"   tap {k}: {e:.3g} of its range")
        assert e <= 1e-3, (k, e)


def test_batch_independence(cuda, engine, sd, golden, oracle_memo):
    from manga_image_translator_amd import synth

    a = golden["page_a"]
    pages = np.stack([a, synth.synth_page(43, a.shape[0], a.shape[1], n_boxes=4)[0]])
    rdb, rmask = oracle_memo("dbconvnext.batch", lambda: O.det_batch_forward(sd, pages))
    db2, mask2 = _forward(engine, cuda, pages)
    e1, e2 = np.abs(db2 - rdb).max(), np.abs(mask2 - rmask[:, 0]).max()
    print(f"dbconvnext B=2 vs oracle: db {e1:.3g} mask {e2:.3g}")
    assert e1 <= 2e-4 and e2 <= 2e-4, (e1, e2)
    db1, mask1 = _forward(engine, cuda, pages[:1])
    assert np.array_equal(db1[0], db2[0]) and np.array_equal(mask1[0], mask2[0])


def test_rejects_bad_input(cuda, engine):
    with pytest.raises(ValueError):
        engine.forward(torch.zeros(1, 200, 256, 3, dtype=torch.uint8, device=cuda))


def test_plugin_with_injected_steps(cuda, plugin, sd, oracle_memo):
    from manga_image_translator_amd import synth

    page = synth.synth_page(8, 256, 200, n_boxes=3)[0]
    seen = {}

    def pre(image, detect_size):  # stands in for bilateralFilter + resize_aspect_ratio: pad 200 -> 256 columns
        canvas = np.zeros((256, 256, 3), np.uint8)
        canvas[:, :200] = image
        return canvas, 1.0, 56, 0

    def boxes(db, h, w, tt, bt, ur):
        seen["db"] = db
        return np.array([[[10, 10], [90, 10], [90, 40], [10, 40]]]), np.array([0.8])

    saved = plugin._pre, plugin._boxes, plugin._resize2x
    plugin._pre, plugin._boxes, plugin._resize2x = pre, boxes, lambda m: np.repeat(np.repeat(m, 2, 0), 2, 1)
    try:
        tls, raw_mask, extra = run(plugin.infer(page, 256, 0.5, 0.7, 2.3))
    finally:
        plugin._pre, plugin._boxes, plugin._resize2x = saved
    assert extra is None and len(tls) == 1 and raw_mask.dtype == np.uint8 and raw_mask.shape == (256, 200)
    canvas, *_ = pre(page, 256)
    rdb, rmask = oracle_memo("dbconvnext.plugin", lambda: O.det_batch_forward(sd, canvas[None]))
    e = np.abs(seen["db"] - rdb).max()
    print(f"dbconvnext plugin db vs oracle: {e:.3g}")
    assert e <= 2e-4, e
    ref_mask = np.clip(np.repeat(np.repeat(rmask[0, 0], 2, 0), 2, 1)[:, :-56] * 255, 0, 255).astype(np.uint8)
    assert np.abs(raw_mask.astype(int) - ref_mask.astype(int)).max() <= 1


def test_plugin_end_to_end(cuda, plugin):
    """Nothing injected: bilateral filter + resize_aspect_ratio, the network, SegDetectorRepresenter and the x2 mask resize are the
    project's own; the shapes are the default detector's at the same sizes (the preprocess pads to a multiple of 256)."""
    from manga_image_translator_amd import synth

    page = synth.synth_page(9, 300, 210, n_boxes=3)[0]
    tls, raw_mask, extra = run(plugin.infer(page, 256, 0.5, 0.7, 2.3))
    assert extra is None and raw_mask.dtype == np.uint8 and raw_mask.shape == (256, 179)
    assert all(np.asarray(q.pts).shape == (4, 2) for q in tls)


def test_plugin_webtoon_strip(cuda, plugin):
    """A tall strip takes det_rearrange_forward's path (rearrange.py): the squares go through the engine as one batch."""
    from manga_image_translator_amd import rearrange, synth

    page = synth.synth_page(10, 1536, 256, n_boxes=6)[0]
    pl = rearrange.plan(page.shape[0], page.shape[1], 256)
    assert pl is not None and pl.p_num == 2 and not pl.transpose
    tls, raw_mask, extra = run(plugin.infer(page, 256, 0.5, 0.7, 2.3))
    pw = 128 // pl.pw_num                      # rearrange.stitch on the 128 x 128 mask squares, then the x2 resize
    assert extra is None and raw_mask.dtype == np.uint8 and raw_mask.shape == (2 * int(pw / pl.w * pl.h), 2 * pw)
    assert raw_mask.std() > 0
    assert all(np.isfinite(np.asarray(q.pts, dtype=np.float64)).all() for q in tls)
