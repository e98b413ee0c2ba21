"""mit_dbnet_mask_tail (csrc/dbnet_tail.hip) against the numpy statement of the DBNet detectors' mask tail (detection/default.py:89-95):
``np.clip(plugins._resize2x_f32(m)[:oh, :ow] * 255, 0, 255).astype(np.uint8)``, byte for byte.  The shapes cover a one-element map, one
row / one column (both borders in one tap), odd sizes, crops to an odd height and to a width that is no multiple of 4 (every row
of such an output starts at another byte of its 32-bit word), more than one wave per row, and a source that is a strided view."""
import numpy as np
import pytest
import torch

SHAPES = [(1, 1, 2, 2), (1, 9, 2, 18), (7, 1, 14, 2), (5, 7, 10, 14), (5, 7, 7, 14), (6, 37, 12, 71), (128, 96, 256, 150)]


def _want(m: np.ndarray, oh: int, ow: int) -> np.ndarray:
    from manga_image_translator_amd import plugins as P

    return np.stack([np.clip(P._resize2x_f32(p)[:oh, :ow] * 255, 0, 255).astype(np.uint8) for p in m])


def _planes(kind: str, h: int, w: int) -> np.ndarray:
    """B = 2 planes f32 [2,h,w]."""
    rng = np.random.default_rng(h * 1000 + w)
    if kind == "uniform":     # [-0.1, 1.1]: both sides of the clip occur
        return rng.uniform(-0.1, 1.1, (2, h, w)).astype(np.float32)
    if kind == "k255":        # exact k / 255: products that land on or beside an integer
        return (rng.integers(0, 256, (2, h, w)).astype(np.float32) / np.float32(255)).astype(np.float32)
    yy, xx = np.mgrid[:h, :w]
    board = ((yy + xx) & 1).astype(np.float32)
    return np.stack([board, 1 - board])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "k255", "checkerboard"])
@pytest.mark.parametrize("h, w, oh, ow", SHAPES)
def test_tail_bytes_equal_the_numpy_expression(cuda, kind, h, w, oh, ow):
    from manga_image_translator_amd import imgproc

    m = _planes(kind, h, w)
    got = imgproc.dbnet_mask_tail(torch.from_numpy(m).to(cuda), oh, ow).cpu().numpy()
    want = _want(m, oh, ow)
    assert got.shape == want.shape == (2, oh, ow) and got.dtype == np.uint8
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    if kind == "uniform" and h * w >= 128 * 96:
        assert (want == 0).any() and (want == 255).any()          # both sides of the clip occurred


@pytest.mark.gpu
def test_tail_reads_a_strided_view_and_writes_nothing_outside_its_output(cuda):
    """The source is a window of a larger slab (row stride 53, batch stride of the slab); the output sits inside a guard band that must
    stay untouched, with rows that start at every byte offset of a word (ow = 71)."""
    from manga_image_translator_amd import imgproc, lib, ops
    import ctypes as C

    h, w, oh, ow = 6, 37, 11, 71
    slab = torch.from_numpy(np.random.default_rng(5).uniform(-0.1, 1.1, (2, 9, 53)).astype(np.float32)).to(cuda)
    view = slab[:, 2:2 + h, 11:11 + w]
    assert not view.is_contiguous()
    want = _want(view.cpu().numpy(), oh, ow)
    assert np.array_equal(imgproc.dbnet_mask_tail(view, oh, ow).cpu().numpy(), want)
    assert np.array_equal(imgproc.dbnet_mask_tail(view[1], oh, ow).cpu().numpy(), want[1])     # [h,w] -> [oh,ow]
    for lead in (1, 2, 3):      # an output that itself starts off a word boundary
        guard = torch.full((lead + 2 * oh * ow + 8,), 0xA5, dtype=torch.uint8, device=cuda)
        out = guard[lead:lead + 2 * oh * ow]
        lib.check(lib.load().mit_dbnet_mask_tail(view.data_ptr(), view.stride(0), view.stride(1), 2, h, w, out.data_ptr(), oh, ow,
                                                 C.c_void_p(ops.current_stream())), "mit_dbnet_mask_tail")
        g = guard.cpu().numpy()
        assert np.array_equal(g[lead:lead + 2 * oh * ow].reshape(2, oh, ow), want), lead
        assert (g[:lead] == 0xA5).all() and (g[lead + 2 * oh * ow:] == 0xA5).all(), lead


@pytest.mark.gpu
def test_default_detector_mask_is_the_host_tail_s_mask(cuda):
    """The plugin with nothing injected (device tail) and with ``resize2x=plugins._resize2x_f32`` injected (the numpy tail) return the same
    lines and the same mask bytes, for a page cropped on the right (pad_w) and one cropped at the bottom (pad_h)."""
    import asyncio

    from manga_image_translator_amd import dbnet_schema, plugins as P, synth

    run = asyncio.new_event_loop().run_until_complete
    sd = synth.synth_state_dict(dbnet_schema.text_detection_schema(), gain=1.2)
    dev_tail, host_tail = P.HipDefaultDetector(weights=sd), P.HipDefaultDetector(weights=sd, resize2x=P._resize2x_f32)
    for p in (dev_tail, host_tail):
        run(p.load("cuda"))
    for H, W in ((320, 200), (200, 320)):
        page = synth.synth_page(3, H, W, n_boxes=2, disjoint=True)[0]
        a, b = run(dev_tail.infer(page, 256, 0.5, 0.7, 2.3)), run(host_tail.infer(page, 256, 0.5, 0.7, 2.3))
        assert a[1].shape == ((256, 160) if H > W else (160, 256)) and a[1].dtype == np.uint8      # the 256 x 256 map less its padding
        assert np.array_equal(a[1], b[1])
        assert [np.asarray(q.pts).tolist() for q in a[0]] == [np.asarray(q.pts).tolist() for q in b[0]]
    for p in (dev_tail, host_tail):
        run(p.unload())
