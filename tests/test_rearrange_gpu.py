"""csrc/rearrange.hip against the host tiling it mirrors (rearrange.squares / stitch / forward, themselves pinned to the reference's
det_rearrange_forward by tests/golden/rearrange.npz): byte-equal squares, bit-identical stitched maps."""
import hashlib
import os

import numpy as np
import pytest
import torch

from manga_image_translator_amd import imgproc, rearrange as RA, synth
from oracle.make_golden import fake_detector

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rearrange.npz"))
HOST_RESIZE = lambda a, ds: imgproc.resize_u8_host(a, ds)   # noqa: E731


def _case(tag):
    """(page, tgt, fixture tag or None)"""
    if tag in ("tall", "wide", "shrink"):
        H, W = (int(v) for v in G[f"shape_{tag}"])
        return synth.synth_page(int(G[f"seed_{tag}"]), H, W, n_boxes=6)[0], int(G[f"tgt_{tag}"]), tag
    page = synth.synth_page(21, 6100, 100, n_boxes=6)[0]      # 31 bands, 16 squares, one empty band
    if tag == "wide31":
        page = np.ascontiguousarray(np.transpose(page, (1, 0, 2)))
    return page, 128, None


_HOST = {}


def host(tag):
    """The host path's squares, network maps and stitched maps of a case, computed once."""
    if tag not in _HOST:
        page, tgt, fx = _case(tag)
        pl = RA.plan(page.shape[0], page.shape[1], tgt)
        sq, pad = RA.squares(page, pl, tgt, HOST_RESIZE)
        assert pad == 0
        d, m = fake_detector(sq)
        _HOST[tag] = dict(page=page, tgt=tgt, fx=fx, pl=pl, sq=sq, db=d, mask=m, db_st=RA.stitch(list(d), pl, 2), mask_st=RA.stitch(list(m), pl, 1))
    return _HOST[tag]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


CASES = ["tall", "wide", "shrink", "tall31", "wide31"]


@pytest.mark.parametrize("tag", CASES)
def test_squares_gpu_equals_host_squares(cuda, tag):
    h = host(tag)
    got = RA.squares_gpu(torch.from_numpy(h["page"]).to(cuda), h["pl"], h["tgt"])
    assert got.dtype == torch.uint8 and tuple(got.shape) == h["sq"].shape
    assert np.array_equal(got.cpu().numpy(), h["sq"])


def test_squares_gpu_unshrunk_gather_and_refusals(cuda):
    """The gather alone (before the shrink) against the host's unshrunk squares, on a plan whose band rows are no multiple of 16 bytes;
    a plan that would need the padding branch is refused."""
    from manga_image_translator_amd import lib as L, ops
    import ctypes as C

    for page in (_case("tall31")[0], _case("wide31")[0]):
        pl = RA.plan(page.shape[0], page.shape[1], 128)
        want, _ = RA.squares(page, pl, 128)
        dev = torch.from_numpy(page).to(cuda)
        sq = torch.full(want.shape, 7, dtype=torch.uint8, device=cuda)
        L.check(L.load().mit_rearrange_squares(dev.data_ptr(), page.shape[0], page.shape[1], int(pl.transpose), pl.w, pl.pw_num, pl.ph_num,
                                               pl.ph_step, pl.p_num, sq.data_ptr(), C.c_void_p(ops.current_stream())))
        assert np.array_equal(sq.cpu().numpy(), want)
        last = sq[-1].cpu().numpy()
        assert pl.pad_num == 1 and not (last[pl.w:] if pl.transpose else last[:, pl.w:]).any()   # the empty band
    pl = RA.plan(6100, 100, 128)
    with pytest.raises(ValueError, match="padded"):
        RA.squares_gpu(torch.zeros(6100, 100, 3, dtype=torch.uint8, device=cuda), pl, 400)
    with pytest.raises(ValueError, match="strip"):
        RA.squares_gpu(torch.zeros(6000, 100, 3, dtype=torch.uint8, device=cuda), pl, 128)
    with pytest.raises(RuntimeError, match="beyond the strip"):
        L.check(L.load().mit_rearrange_squares(1, 400, 100, 0, 100, 2, 3, 150, 2, 1, None))


@pytest.mark.parametrize("tag", CASES)
def test_stitch_gpu_equals_host_stitch(cuda, tag):
    """C = 2 at full resolution and the half-resolution C = 1 map; u8=True is postprocess_mask of the stitched map."""
    h = host(tag)
    db = RA.stitch_gpu(torch.from_numpy(h["db"]).to(cuda), h["pl"])
    mask, mask_u8 = RA.stitch_gpu(torch.from_numpy(h["mask"]).to(cuda), h["pl"], u8=True)
    for got, key in ((db, "db"), (mask, "mask")):
        want = h[f"{key}_st"]
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
        assert got.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()
        if h["fx"]:
            assert sha(got.cpu().numpy()) == str(G[f"{key}_sha_{h['fx']}"])
    assert mask_u8.dtype == torch.uint8 and np.array_equal(mask_u8.cpu().numpy(), (h["mask_st"] * 255).astype(np.uint8))


@pytest.mark.parametrize("tag", ["tall", "wide", "tall31"])
def test_stitch_gpu_takes_strided_views(cuda, tag):
    """A channel slice of a larger tensor (other batch / channel strides), a [n, m, m] view with a padded row stride (the ctd engine's
    ``last_mask_f32``), and a view whose storage offset breaks the 16-byte alignment: all uncopied, all bit-identical."""
    h = host(tag)
    n, _, m, _ = h["db"].shape
    big = torch.full((n, 5, m, m), -3.0, device=cuda)
    big[:, 1:3] = torch.from_numpy(h["db"]).to(cuda)
    view = big[:, 1:3]
    assert view.stride(0) == 5 * m * m and view.data_ptr() != big.data_ptr()      # the slice's own batch stride and offset
    assert RA.stitch_gpu(view, h["pl"]).cpu().numpy().tobytes() == np.ascontiguousarray(h["db_st"]).tobytes()
    mm = h["mask"].shape[-1]
    slab = torch.full((n, mm + 3, mm + 5, 1), -3.0, device=cuda)
    slab[:, :mm, :mm, 0] = torch.from_numpy(h["mask"][:, 0]).to(cuda)
    got, got_u8 = RA.stitch_gpu(slab[:, :mm, :mm, 0], h["pl"], u8=True)
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(h["mask_st"]).tobytes()
    assert np.array_equal(got_u8.cpu().numpy(), (h["mask_st"] * 255).astype(np.uint8))
    flat = torch.zeros(h["db"].size + 1, device=cuda)
    flat[1:] = torch.from_numpy(h["db"]).to(cuda).reshape(-1)
    assert RA.stitch_gpu(flat[1:].view(h["db"].shape), h["pl"]).cpu().numpy().tobytes() == np.ascontiguousarray(h["db_st"]).tobytes()


@pytest.mark.parametrize("tag", CASES)
def test_forward_gpu_equals_host_forward(cuda, tag):
    h = host(tag)
    calls = []

    def net(sq):   # the stand-in network on the device's squares; its outputs live in one reused buffer, like an engine's workspace
        assert sq.is_cuda and sq.dtype == torch.uint8
        calls.append(tuple(sq.shape))
        d, m = fake_detector(sq.cpu().numpy())
        net.db[:len(d)] = torch.from_numpy(d).to(cuda)
        net.mask[:len(m)] = torch.from_numpy(m).to(cuda)
        return net.db[:len(d)], net.mask[:len(m)]

    t = h["tgt"]
    net.db, net.mask = torch.empty(4, 2, t, t, device=cuda), torch.empty(4, 1, t // 2, t // 2, device=cuda)
    db, mask = RA.forward_gpu(torch.from_numpy(h["page"]).to(cuda), net, t)
    assert calls and all(s[0] <= 4 and s[1:] == (t, t, 3) for s in calls) and sum(s[0] for s in calls) == h["pl"].p_num
    want_db, want_mask = RA.forward(h["page"], fake_detector, t, resize=HOST_RESIZE)
    assert db.cpu().numpy().tobytes() == np.ascontiguousarray(want_db).tobytes()
    assert mask.cpu().numpy().tobytes() == np.ascontiguousarray(want_mask).tobytes()
    assert RA.forward_gpu(torch.zeros(300, 200, 3, dtype=torch.uint8, device=cuda), None, 128) == (None, None)
