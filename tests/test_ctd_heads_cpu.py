"""``ctd.head_extents``: the crops of ``u320`` / ``db1`` / ``db0`` that the detector's last layers read for an un-padded region
``(hv, wv)`` of the letterbox square, checked against the tap tables ``ops.ConvTranspose2d`` builds (no GPU: the tables are host data).

For every output index inside the region the parity classes' taps name the input indices that are read; the extent must cover all of
them that lie inside the image (taps outside it read zeros, not memory) and reach at most one row / column further."""
import itertools

import numpy as np
import pytest
import torch

S = 1024
SIZES = (1, 2, 3, 4, 5, 727, 728, 729, 1023, 1024)


@pytest.fixture(scope="module")
def layers():
    from manga_image_translator_amd import ops

    g = torch.Generator().manual_seed(0)
    k4 = ops.ConvTranspose2d(torch.randn(64, 1, 4, 4, generator=g), None, stride=2, padding=1, device="cpu")
    k2 = ops.ConvTranspose2d(torch.randn(16, 1, 2, 2, generator=g), None, stride=2, device="cpu")
    return k4, k2


def reads_1d(layer, axis: int, n_out: int, n_in: int) -> np.ndarray:
    """Input indices (inside the image) along ``axis`` (0 = rows, 1 = columns) that outputs ``< n_out`` read, from ``layer.sub``."""
    read = np.zeros(n_in, dtype=bool)
    for py, px, pk in layer.sub:
        par = (py, px)[axis]
        o = np.arange(par, n_out, layer.s)          # output indices of this parity class inside the extent
        sub = (o - par) // layer.s                  # their index in the class's sub-grid (the launch's oy / ox)
        for tap in pk.taps:
            idx = sub + tap[axis]
            read[idx[(idx >= 0) & (idx < n_in)]] = True
    return read


def needed(layer, axis, n_out, n_in) -> int:
    r = np.nonzero(reads_1d(layer, axis, n_out, n_in))[0]
    return int(r.max()) + 1 if r.size else 0


def test_tap_tables_are_the_forms_the_extents_assume(layers):
    k4, k2 = layers
    assert k4.one_pass and k2.one_pass
    assert sorted(t[:2] for _, _, pk in k2.sub for t in pk.taps) == [(0, 0)] * 4
    assert {(py, px): [t[:2] for t in pk.taps] for py, px, pk in k4.sub} == {
        (0, 0): [(0, 0), (0, -1), (-1, 0), (-1, -1)], (0, 1): [(0, 1), (0, 0), (-1, 1), (-1, 0)],
        (1, 0): [(1, 0), (1, -1), (0, 0), (0, -1)], (1, 1): [(1, 1), (1, 0), (0, 1), (0, 0)]}


@pytest.mark.parametrize("hv,wv", list(itertools.product(SIZES, SIZES)))
def test_extents_cover_what_the_taps_read(layers, hv, wv):
    from manga_image_translator_amd import ctd

    k4, k2 = layers
    u, b1, b0 = ctd.head_extents(hv, wv, S)
    for axis, n in ((0, hv), (1, wv)):
        # up6 (k4 s2 p1) reads u320 [512]; t2 (k2 s2) reads db1 [512]; t1 (k2 s2) reads db0 [256] for the db1 extent
        for name, got, layer, n_out, n_in in (("u320", u[axis], k4, n, S // 2), ("db1", b1[axis], k2, n, S // 2),
                                              ("db0", b0[axis], k2, b1[axis], S // 4)):
            need = needed(layer, axis, n_out, n_in)
            assert need <= got <= min(need + 1, n_in), (name, axis, n, need, got)
    # t1 writes db1[: 2 * db0 extent], which must hold what t2 reads; c0's 3 x 3 window reads db0 extent + 1 of the uncropped `dc`
    assert 2 * b0[0] >= b1[0] and 2 * b0[1] >= b1[1] and 2 * b0[0] <= S // 2 and 2 * b0[1] <= S // 2


def test_letterbox_of_the_benchmark_page():
    from manga_image_translator_amd import ctd

    nh, nw, dw, dh = ctd.CtdEngine.letterbox_geometry(2048, 1456, S)
    assert (nh, nw, dw, dh) == (1024, 728, 296, 0)
    assert ctd.head_extents(S - dh, S - dw, S) == ((512, 365), (512, 364), (256, 182))
