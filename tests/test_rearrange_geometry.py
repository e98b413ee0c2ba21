"""The per-element form of the strip stitch that csrc/rearrange.hip runs, on the CPU: with ``rearrange.stitch_geometry``'s numbers, every
output element replays the bands that cover its row in ascending order (add, then halve where the band overlaps its predecessor).  That
reproduces ``rearrange.stitch`` — and through tests/golden/rearrange.npz the reference's own det_rearrange_forward — bit for bit.  Also
the claim the device path's missing padding branch rests on: every plan of ``plan()`` has squares larger than the detect size."""
import hashlib
import os

import numpy as np
import pytest

from manga_image_translator_amd import imgproc, rearrange as RA, synth
from oracle.make_golden import fake_detector

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rearrange.npz"))


def network_squares(page, tgt):
    """What ``rearrange.forward`` hands to ``stitch``: the stand-in network's maps of every square, at most four squares per call."""
    pl = RA.plan(page.shape[0], page.shape[1], tgt)
    sq, pad = RA.squares(page, pl, tgt, lambda a, ds: imgproc.resize_u8_host(a, ds))
    assert pad == 0 and sq.shape == (pl.p_num, tgt, tgt, 3)
    dbs, masks = [], []
    for i in range(0, len(sq), 4):
        d, m = fake_detector(sq[i:i + 4])
        dbs += list(d)
        masks += list(m)
    return pl, dbs, masks


def replay(maps, pl):
    """Element (c, y, x) of the stitched map, all elements at once: ``v`` holds every element's running value, and band p touches the
    elements whose row it covers.  No slice assignment: the conditions are evaluated per element, as the kernel's threads do.
    -> (map [1, C, H', W'], the largest number of bands that cover one row)."""
    psize = maps[0].shape[-1]
    step, pw, hh, starts = RA.stitch_geometry(pl, psize)
    assert len(starts) == pl.ph_num and all(b >= a for a, b in zip(starts, starts[1:]))
    C = maps[0].shape[0]
    c, y, x = np.meshgrid(np.arange(C), np.arange(hh), np.arange(pw), indexing="ij")
    v = np.zeros((C, hh, pw), np.float32)
    cover = np.zeros(hh, np.int64)
    for p in range(pl.ph_num):
        t = starts[p]
        sq = maps[p // pl.pw_num]
        add = (t <= y) & (y < min(t + psize, hh))
        col = (p % pl.pw_num) * pw + x[add]
        src = sq[c[add], col, y[add] - t] if pl.transpose else sq[c[add], y[add] - t, col]
        v[add] = v[add] + src
        if p > 0:
            half = (t <= y) & (y < t + (psize - step))
            v[half] = v[half] * np.float32(0.5)
        cover[t:min(t + psize, hh)] += 1
    assert v.dtype == np.float32
    out = np.transpose(v, (0, 2, 1)) if pl.transpose else v
    return out[None], int(cover.max())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("tag", ["tall", "wide", "shrink"])
def test_per_element_replay_equals_stitch_and_the_reference(tag):
    H, W = (int(v) for v in G[f"shape_{tag}"])
    tgt = int(G[f"tgt_{tag}"])
    page = synth.synth_page(int(G[f"seed_{tag}"]), H, W, n_boxes=6)[0]
    pl, dbs, masks = network_squares(page, tgt)
    for maps, ch, key in ((dbs, 2, "db"), (masks, 1, "mask")):
        want = RA.stitch(maps, pl, ch)
        got, cover = replay(maps, pl)
        assert got.dtype == np.float32 and got.shape == want.shape == tuple(G[f"{key}_shape_{tag}"])
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()
        assert sha(got) == str(G[f"{key}_sha_{tag}"]) == sha(want)
        assert cover <= 2


def test_per_element_replay_many_bands():
    """6100 x 100 at 128: 31 overlapping bands in 16 squares, the last square half empty, four network batches."""
    page = synth.synth_page(21, 6100, 100, n_boxes=6)[0]
    pl, dbs, masks = network_squares(page, 128)
    assert (pl.ph_num, pl.p_num, pl.pad_num, pl.pw_num) == (31, 16, 1, 2) and pl.ph_step < pl.patch and not pl.transpose
    for maps, ch in ((dbs, 2), (masks, 1)):
        want = RA.stitch(maps, pl, ch)
        got, _ = replay(maps, pl)
        assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()
    wide = np.ascontiguousarray(np.transpose(page, (1, 0, 2)))
    plw, dbs, masks = network_squares(wide, 128)
    assert plw.transpose and plw.ph_num == 31
    for maps, ch in ((dbs, 2), (masks, 1)):
        want = RA.stitch(maps, plw, ch)
        got, _ = replay(maps, plw)
        assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()


def test_stitch_geometry_is_what_stitch_uses():
    pl = RA.plan(12000, 800, 1024)
    step, pw, hh, starts = RA.stitch_geometry(pl, 1024)
    assert (step, pw, hh) == (int(pl.ph_step * 1024 / 1600), 512, int(512 / 800 * 12000)) and len(starts) == 8 and starts[0] == 0
    assert starts == [int(round(r * hh)) for r in pl.rel_steps]
    assert RA.stitch([np.zeros((1, 1024, 1024), np.float32)] * 4, pl, 1).shape == (1, 1, hh, pw)


def test_every_plan_shrinks_its_squares():
    """``squares_gpu`` has no padding branch: for every plan, patch > tgt (so square_pad_resize always shrinks) and there are at least
    two bands.  For w <= tgt, patch = floor(2 tgt / w) w > 2 tgt - w >= tgt; else patch = 2 w > 2 tgt."""
    rng = np.random.default_rng(5)
    n = 0
    for _ in range(60000):
        tgt = int(rng.integers(32, 2049))
        short = int(rng.integers(1, 4 * tgt))
        long = int(short * rng.uniform(1.0, 40.0)) + int(rng.integers(0, 3))
        for h, w in ((long, short), (short, long)):
            pl = RA.plan(h, w, tgt)
            if pl is None:
                continue
            n += 1
            assert pl.patch > tgt and pl.ph_num >= 2 and pl.patch == pl.pw_num * pl.w
            assert (pl.ph_num - 1) * pl.ph_step + pl.patch <= pl.h and 0 <= pl.pad_num < pl.pw_num
    assert n > 20000
