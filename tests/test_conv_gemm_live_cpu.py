"""The live-block list of mit_conv_gemm (MitConvGemm.live_blocks / live_start) through mit_conv_gemm_plan, and the need propagation of
LaMa's masked decoder tail in numpy — no GPU: the plan dereferences no pointer, the propagation is host arithmetic."""
import numpy as np
import pytest
import torch

from _conv_gemm_plan_cases import desc, plan

FAKE_LIST, FAKE_START = 65536, 131072


@pytest.fixture(scope="module")
def handle():
    from manga_image_translator_amd import lib

    h = lib.load(build_if_missing=True)
    mode, mt = h.mit_gemm_mode_get(), h.mit_gemm_split_min_tiles(-1)
    h.mit_gemm_split_min_tiles(0)
    yield h
    h.mit_gemm_mode_set(mode)
    h.mit_gemm_split_min_tiles(mt)


def with_list(d):
    d.live_blocks, d.live_start = FAKE_LIST, FAKE_START
    return d


# a parity class of an up-convolution: 4 taps, Cin 256 -> 128 on a 512 x 364 sub-grid (364 is no multiple of 8)
UP = dict(NB=4, Ho=512, Wo=364, Cin=256, taps=4, N=128)


def test_list_is_accepted_on_split_p1_and_fp32_tiles(handle):
    for mode, kw, family in ((6, dict(split=1), "split"), (9, dict(split=1), "split"), (6, dict(split=1, nprod=1), "p1"), (0, dict(), "fast")):
        assert handle.mit_gemm_mode_set(mode) == 0
        got = plan(handle, with_list(desc(**UP, **kw)))
        dense = plan(handle, desc(**UP, **kw))
        assert not got.startswith("refused"), got
        assert got == dense, "the list changes neither the tile family nor the cut"
        name = got.rsplit(":", 1)[0]
        assert name.startswith("split" if family != "fast" else "fast"), got
        assert ("p1" in name) == (family == "p1"), got


def test_list_is_refused_where_no_kernel_reads_it(handle):
    handle.mit_gemm_mode_set(6)
    got = plan(handle, with_list(desc(NB=1, Ho=32, Wo=32, Cin=64, taps=9, N=3)))  # gemv-shaped: N <= 4
    assert got.startswith("refused") and "live-block list" in got, got
    got = plan(handle, with_list(desc(NB=1, Ho=24, Wo=24, Cin=12, taps=9, N=64)))  # the generic kernel (Cin % 16 != 0)
    assert got.startswith("refused") and "live-block list" in got, got
    got = plan(handle, with_list(desc(**UP, Z=2)))
    assert got.startswith("refused") and "Z == 1" in got, got
    d = desc(**UP)
    d.live_blocks = FAKE_LIST  # one array without the other
    assert plan(handle, d).startswith("refused")
    d = desc(**UP)
    d.live_img0 = 1            # an image offset without a list
    assert plan(handle, d).startswith("refused")


def test_cut_batch_reports_its_run_with_a_list(handle):
    handle.mit_gemm_mode_set(6)
    kw = dict(NB=16, Ho=1024, Wo=728, Cin=128, taps=4, N=64, split=1)  # ups[2] at 16 pages: the A operand is 6.1 GB
    dense, got = plan(handle, desc(**kw)), plan(handle, with_list(desc(**kw)))
    assert got == dense and not got.startswith("refused"), got
    assert int(got.rsplit(":", 1)[1]) == 4, got


def _read_sets(layer, need_out):
    """Brute force from the layer's own tap tables: the input positions that the needed outputs read."""
    H2, W2 = need_out.shape
    H, W = H2 // 2, W2 // 2
    read = np.zeros((H, W), bool)
    for py, px, pk in layer.sub:
        for oy, ox in zip(*np.nonzero(need_out[py::2, px::2])):
            for dy, dx, _ in pk.taps:
                iy, ix = oy + dy, ox + dx
                if 0 <= iy < H and 0 <= ix < W:
                    read[iy, ix] = True
    return read


def test_need_propagation_is_a_superset_of_what_the_taps_read():
    from manga_image_translator_amd import ops
    from manga_image_translator_amd.lama import tail_need_numpy

    layer = ops.ConvTranspose2d(torch.zeros(4, 4, 3, 3), None, stride=2, padding=1, output_padding=1, device="cpu")
    assert sorted(len(pk.taps) for _, _, pk in layer.sub) == [1, 2, 2, 4]
    rng = np.random.default_rng(5)
    H, W = 8, 12
    masks = [np.zeros((H, W), np.uint8) for _ in range(4)]
    masks[1][:] = 255
    masks[2][0, 0], masks[2][7, 11], masks[2][3, 6] = 127, 128, 126
    masks[3][:] = (rng.random((H, W)) < 0.08) * 255
    mask = np.stack(masks)
    need = tail_need_numpy(mask)
    assert np.array_equal(need["cells"][:, :, 0], (mask >= 127).any(axis=(1, 2))[:, None])
    for b in range(mask.shape[0]):
        pred = mask[b] >= 127
        win = np.zeros_like(pred)  # the 7x7 window under reflect padding, brute force
        for y, x in zip(*np.nonzero(pred)):
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    yy, xx = y + dy, x + dx
                    yy = -yy if yy < 0 else (2 * H - 2 - yy if yy >= H else yy)
                    xx = -xx if xx < 0 else (2 * W - 2 - xx if xx >= W else xx)
                    win[yy, xx] = True
        assert not (win & ~need["need_out"][2][b]).any()
        for L in (2, 1):  # 8 x 12 <- 4 x 6 <- 2 x 3: which inputs does each needed output read
            read = _read_sets(layer, need["need_out"][L][b])
            assert not (read & ~need["need_out"][L - 1][b]).any(), (L, b)
    assert need["need_out"][2][2, :, :].sum() < H * W and need["need_out"][2][3].any(), "the cases are neither all empty nor all full"
    # every layer: the inputs read by its needed outputs are needed outputs of the layer before (the same masks enlarged to 32 x 48, so that all three layers have valid sizes)
    big = np.kron(mask, np.ones((4, 4), np.uint8))
    need = tail_need_numpy(big)
    for L in (2, 1):
        for b in range(big.shape[0]):
            read = _read_sets(layer, need["need_out"][L][b])
            assert not (read & ~need["need_out"][L - 1][b]).any(), (L, b)
            # and a needed output lies in a live block of its own layer's parity sub-grid
            sub = need["need_out"][L][b].reshape(read.shape[0], 2, read.shape[1], 2).any(axis=(1, 3))
            blk = np.kron(need["blocks"][L][b], np.ones((8, 8), bool))[:sub.shape[0], :sub.shape[1]]
            assert not (sub & ~blk).any()
    for L in range(3):
        assert need["start"][L][-1] == len(need["list"][L]) and np.all(np.diff(need["list"][L]) > 0)
    assert len(need["list"][2]) == 0 or need["start"][2][1] == 0  # the empty mask lists nothing
