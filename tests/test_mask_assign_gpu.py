"""Component labelling and line assignment of the mask refinement on the device (csrc/mask_assign.hip: ``mit_mask_assign_lines_dev`` +
``mit_mask_line_crops_dev``, ``GpuMaskBackend.assign_lines_device``) against the host routine on the same inputs
(``mit_mask_assign_lines`` + ``mit_mask_line_crops``, itself pinned to the reference by tests/test_mask_refinement.py and
tests/golden/mask_refinement.npz).  Equality everywhere: outlined mask, line rectangles, every crop, the final mask — no tolerance.
Every comparison also checks the backend's ``device_assigns`` counter, so a silent fall-back to the host routine cannot pass."""
import types

import numpy as np
import pytest
import torch

from manga_image_translator_amd import mask_refinement as MR
from manga_image_translator_amd.textline import Quadrilateral

pytestmark = pytest.mark.gpu


def _random_scene(rng, H, W, n_lines):
    """Blobs of every kind the assignment distinguishes: glyph-sized ones inside rotated line quads, strays near and far (nearest-line
    branch and its cut-off), specks of <= 9 pixels, diagonal chains, blobs larger than their line, blobs on the frame."""
    mask = np.zeros((H, W), np.uint8)
    quads = []
    for k in range(n_lines):
        cx, cy = rng.uniform(30, W - 30), rng.uniform(30, H - 30)
        hw, hh = rng.uniform(20, 70), rng.uniform(6, 14)
        if rng.random() < 0.4:
            hw, hh = hh, hw
        a = rng.uniform(-0.5, 0.5) if rng.random() < 0.5 else 0.0
        c, s_ = np.cos(a), np.sin(a)
        rot = np.array([[c, s_], [-s_, c]])
        pts = np.array([[-hw, -hh], [hw, -hh], [hw, hh], [-hw, hh]]) @ rot + [cx, cy]
        quads.append(Quadrilateral(pts.astype(np.float64), "", 0))
        for _ in range(int(rng.integers(2, 9))):   # glyphs along the line
            gx, gy = (np.array([rng.uniform(-0.9, 0.9) * hw, rng.uniform(-0.5, 0.5) * hh]) @ rot + [cx, cy]).astype(int)
            g = int(rng.integers(2, 7))
            mask[max(gy - g, 0):gy + g, max(gx - g, 0):gx + g] = 255
        if k % 5 == 4:   # a blob larger than its line
            mask[max(int(cy - hh - 20), 0):int(cy + hh + 20), max(int(cx - hw - 20), 0):int(cx + hw + 20)] = 255
    for _ in range(12):   # strays
        x, y, w, h = int(rng.integers(0, W - 4)), int(rng.integers(0, H - 4)), int(rng.integers(1, 30)), int(rng.integers(1, 30))
        mask[y:y + h, x:x + w] = 255
    for _ in range(40):   # specks and diagonal chains
        x, y = int(rng.integers(1, W - 12)), int(rng.integers(1, H - 12))
        for d in range(int(rng.integers(1, 12))):
            mask[y + d, x + d] = 255
    mask[0:3, 5:40] = mask[H - 2:, W // 2:W // 2 + 30] = 255   # on the frame
    mask[H // 3:H // 3 + 25, 0:2] = mask[H // 2:H // 2 + 12, W - 3:] = 255
    mask[rng.random((H, W)) < 0.002] = 255
    return mask, quads


def _jobs_for(rects, H, W):
    """Crop jobs (line, x, y, w, h) the way the tail makes them (the rectangle, extended), plus a second, shifted job for the first
    line that has a rectangle and one that hangs over the page's edge."""
    jobs = []
    for i, r in enumerate(rects):
        if r is None:
            continue
        x, y, w, h = MR._extend_rect(r[0], r[1], r[2] - r[0], r[3] - r[1], W, H, 3)
        if w > 0 and h > 0:
            jobs.append((i, x, y, w, h))
    if jobs:
        i, x, y, w, h = jobs[0]
        jobs.append((i, max(x - 5, 0), max(y - 2, 0), w + 3, h + 1))
        jobs.append((i, W - 4, H - 3, 9, 7))
    return jobs


def _compare_assignment(cuda, be, mask, quads, keep_threshold=1e-2):
    """Host routine vs device form on the same mask: outlined mask, rectangles, crops (host arrays and the packed device buffer)."""
    H, W = mask.shape
    m_host = mask.copy()
    rects_h, _, crops_h = MR._assign_components_native(m_host, quads, keep_threshold)
    m_dev = torch.from_numpy(mask.copy()).to(cuda)
    before = be.device_assigns
    rects_d, _, crops_d, packed = be.assign_lines_device(m_dev, quads, keep_threshold)
    assert be.device_assigns == before + 1
    assert np.array_equal(m_dev.cpu().numpy(), m_host), "outlined mask"
    assert rects_d == rects_h, (rects_d, rects_h)
    jobs = _jobs_for(rects_h, H, W)
    if jobs:
        a, b = crops_h(jobs), crops_d(jobs)
        assert len(a) == len(b) == len(jobs)
        for j, (ca, cb) in enumerate(zip(a, b)):
            assert ca.shape == cb.shape and np.array_equal(ca, cb), f"crop of job {jobs[j]}"
        flat, offs = packed(jobs)
        assert flat.is_cuda and flat.numel() == int(offs[-1]) and np.array_equal(flat.cpu().numpy(), np.concatenate([c.reshape(-1) for c in a]))
    return rects_h


def _compare_final(cuda, be, be_host, page, mask, quads, dilation_offset=20):
    """``dispatch_device`` with the device assignment vs the same backend kind with the host routine: the final mask's bytes."""
    regions = [types.SimpleNamespace(lines=[np.asarray(q.pts)]) for q in quads]
    pd, md = torch.from_numpy(page).to(cuda), torch.from_numpy(mask).to(cuda)
    before, before_h = be.device_assigns, be_host.device_assigns
    got = MR.dispatch_device(regions, pd, md.clone(), dilation_offset=dilation_offset, kernel_size=3, backend=be)
    want = MR.dispatch_device(regions, pd, md.clone(), dilation_offset=dilation_offset, kernel_size=3, backend=be_host)
    assert be.device_assigns == before + 1 and be_host.device_assigns == before_h == 0
    assert got.is_cuda and got.shape == mask.shape
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    return got


@pytest.fixture(scope="module")
def backends(cuda):
    return MR.GpuMaskBackend(cuda), MR.GpuMaskBackend(cuda, gpu_assign=False)


@pytest.mark.parametrize("seed", range(14))
def test_device_assignment_equals_the_host_routine(cuda, backends, seed):
    be, be_host = backends
    rng = np.random.default_rng(500 + seed)
    H, W = int(rng.integers(120, 260)), int(rng.integers(150, 330))
    mask, quads = _random_scene(rng, H, W, int(rng.integers(1, 9)))
    rects = _compare_assignment(cuda, be, mask, quads)
    assert any(r is not None for r in rects)    # the scene exercises the assignment, not only the rejections
    # the whole refinement: a page 1.5x as large, so that dispatch's working scale (2 / 3) is about the scene's size
    Hp, Wp = int(H * 1.5), int(W * 1.5)
    big, lines = _random_scene(rng, Hp, Wp, int(rng.integers(1, 9)))
    page = rng.integers(0, 256, (Hp, Wp, 3), dtype=np.uint8)
    _compare_final(cuda, be, be_host, page, big, lines, dilation_offset=int(seed % 3) * 10)


@pytest.mark.parametrize("seed", range(2))
def test_device_assignment_at_page_scale(cuda, backends, seed):
    """1365 x 970 (the working scale of a 2048 x 1456 page) with 40 lines; then the whole ``dispatch_device`` of that page."""
    be, be_host = backends
    rng = np.random.default_rng(900 + seed)
    mask, quads = _random_scene(rng, 1365, 970, 40)
    assert len(quads) >= 32
    rects = _compare_assignment(cuda, be, mask, quads)
    assert sum(r is not None for r in rects) >= 16
    big, bq = _random_scene(np.random.default_rng(950 + seed), 2048, 1456, 36)
    page = rng.integers(0, 256, (2048, 1456, 3), dtype=np.uint8)
    _compare_final(cuda, be, be_host, page, big, bq)


def _q(pts):
    return Quadrilateral(np.array(pts, np.float64), "", 0)


LINE = [[10, 10], [60, 10], [60, 30], [10, 30]]


@pytest.mark.parametrize("name,mask,quads", [
    ("empty", np.zeros((40, 80), np.uint8), [_q(LINE)]),
    ("full", np.full((40, 80), 255, np.uint8), [_q(LINE)]),
    ("no lines", np.full((40, 80), 255, np.uint8), []),
    ("one pixel wide", np.full((64, 1), 255, np.uint8), [_q(LINE)]),
    ("one pixel tall", np.full((1, 64), 255, np.uint8), [_q(LINE)]),
    ("outline off the page", np.full((40, 80), 255, np.uint8), [_q([[200, 300], [260, 300], [260, 330], [200, 330]]), _q([[-90, -80], [-50, -80], [-50, -60], [-90, -60]])]),
    ("zero-area line", None, [_q([[50, 20], [50, 20], [50, 20], [50, 20]]), _q(LINE), _q([[5, 33], [70, 33], [70, 33], [5, 33]])]),
    ("zero-area line alone", None, [_q([[30, 20], [30, 20], [30, 20], [30, 20]])]),
])
def test_device_assignment_edge_cases(cuda, backends, name, mask, quads):
    be, be_host = backends
    if mask is None:   # glyphs inside and beside the lines
        mask = np.zeros((40, 80), np.uint8)
        mask[14:26, 14:22] = mask[14:26, 30:38] = mask[16:24, 47:54] = mask[32:37, 20:30] = 255
    _compare_assignment(cuda, be, mask, quads)
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, mask.shape + (3,), dtype=np.uint8)).to(cuda)
    before = be.device_assigns
    got = MR.complete_mask(img, torch.from_numpy(mask.copy()).to(cuda), quads, backend=be, device_result=True)
    want = MR.complete_mask(img, mask.copy(), quads, backend=be_host, device_result=True)
    assert be.device_assigns == before + 1
    assert (got is None) == (want is None), name
    if got is not None:
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())


def test_two_crop_jobs_for_one_line(cuda, backends):
    be, _ = backends
    mask = np.zeros((60, 120), np.uint8)
    mask[14:26, 14:22] = mask[14:26, 30:38] = mask[16:24, 47:54] = 255
    quads = [_q(LINE), _q([[70, 40], [110, 40], [110, 55], [70, 55]])]
    mask[42:52, 75:85] = 255
    m_host = mask.copy()
    rects_h, _, crops_h = MR._assign_components_native(m_host, quads, 1e-2)
    before = be.device_assigns
    rects_d, _, crops_d, _ = be.assign_lines_device(torch.from_numpy(mask.copy()).to(cuda), quads, 1e-2)
    assert be.device_assigns == before + 1 and rects_d == rects_h and rects_h[0] is not None and rects_h[1] is not None
    jobs = [(0, 10, 10, 30, 20), (1, 70, 40, 40, 15), (0, 25, 12, 40, 18), (0, 0, 0, 120, 60)]
    for a, b in zip(crops_h(jobs), crops_d(jobs)):
        assert np.array_equal(a, b)
    assert crops_d(jobs)[3].any() and not crops_d(jobs)[3][40:].any()   # the page-sized job of line 0 holds line 0's components only


def test_more_than_100000_components(cuda, backends):
    """Isolated pixels on a stride-2 grid at 1365 x 970: every one a component of its own, all specks, nothing assigned — the per-root
    planes have no cap on the number of components."""
    be, _ = backends
    H, W = 1365, 970
    mask = np.zeros((H, W), np.uint8)
    mask[::2, ::2] = 255
    quads = [_q([[100, 100], [400, 100], [400, 160], [100, 160]]), _q([[500, 700], [900, 700], [900, 760], [500, 760]])]
    rects = _compare_assignment(cuda, be, mask, quads)
    assert rects == [None, None]
    n_assigned, n_big, n_comp, _ = be.last_assign_status
    assert n_comp > 100000 and n_big == 0 and n_assigned == 0
    outlined = mask.copy()
    MR._assign_components_native(outlined, quads, 1e-2)
    assert n_comp == int(np.count_nonzero(outlined))


def test_argument_checks_do_not_touch_the_device():
    """Null pointers, polygons other than quadrilaterals and a short workspace are refused before any HIP call (the pointers below
    are never dereferenced)."""
    from manga_image_translator_amd import lib

    L = lib.load()
    need = L.mit_mask_assign_workspace_bytes(40, 80)
    assert need >= 7 * 40 * 80 * 4 and L.mit_mask_assign_workspace_bytes(0, 80) < 0 and L.mit_mask_assign_workspace_bytes(1 << 16, 1 << 16) < 0
    fake = 4096
    assert L.mit_mask_assign_lines_dev(None, 40, 80, fake, fake, fake, 1, 4, 0.01, fake, need, fake, None) != 0
    assert b"null pointer" in L.mit_last_error()
    assert L.mit_mask_assign_lines_dev(fake, 40, 80, None, fake, fake, 1, 4, 0.01, fake, need, fake, None) != 0
    assert b"null pointer" in L.mit_last_error()
    assert L.mit_mask_assign_lines_dev(fake, 40, 80, fake, fake, fake, 1, 5, 0.01, fake, need, fake, None) != 0
    assert b"quadrilaterals only" in L.mit_last_error()
    assert L.mit_mask_assign_lines_dev(fake, 40, 80, fake, fake, fake, 1, 4, 0.01, fake, need - 1, fake, None) != 0
    assert b"workspace" in L.mit_last_error()
    assert L.mit_mask_assign_lines_dev(fake, 0, 80, fake, fake, fake, 1, 4, 0.01, fake, need, fake, None) != 0
    assert b"bad shape" in L.mit_last_error()
    assert L.mit_mask_line_crops_dev(None, need, 40, 80, fake, fake, 1, 16, fake, None) != 0 and b"null pointer" in L.mit_last_error()
    assert L.mit_mask_line_crops_dev(fake, need, 40, 80, None, fake, 1, 16, fake, None) != 0 and b"null pointer" in L.mit_last_error()
    assert L.mit_mask_line_crops_dev(fake, need - 1, 40, 80, fake, fake, 1, 16, fake, None) != 0 and b"workspace" in L.mit_last_error()
    assert L.mit_mask_line_crops_dev(fake, need, 40, 80, fake, fake, -1, 16, fake, None) != 0 and b"bad shape" in L.mit_last_error()
