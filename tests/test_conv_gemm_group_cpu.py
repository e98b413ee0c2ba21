"""mit_conv_gemm_group seen through mit_conv_gemm_group_plan (no GPU: the plan makes no HIP call and dereferences no operand pointer).
A grouped launch is the concatenation of its members' grids: the plan reports the tile, the launch each member rides in and its first
workgroup there.  The descriptors carry fake, aligned pointers, like those of test_conv_gemm_plan.py."""
import ctypes as C
import re

import pytest

from _conv_gemm_plan_cases import FAKE_A, FAKE_C, desc, plan

GROUP_MAX = 32


@pytest.fixture(scope="module")
def handle():
    from manga_image_translator_amd import lib

    h = lib.load(build_if_missing=True)
    mode, mt = h.mit_gemm_mode_get(), h.mit_gemm_split_min_tiles(-1)
    h.mit_gemm_split_min_tiles(0)
    yield h
    h.mit_gemm_mode_set(mode)
    h.mit_gemm_split_min_tiles(mt)


def _group(shapes, **layer):
    """The layer ``layer`` (arguments of ``desc``) over images of the sizes ``shapes`` = [(NB, Ho, Wo), ...], each at its own address."""
    descs = []
    for i, (nb, ho, wo) in enumerate(shapes):
        descs.append(desc(NB=nb, Ho=ho, Wo=wo, a=FAKE_A + (i << 24), c=FAKE_C + (i << 24) + (1 << 23), **layer))
    return descs


def _plan(descs):
    from manga_image_translator_amd import ops

    return ops.conv_gemm_group_plan(descs)


def _tile_dims(name):
    bm, bn, _ = map(int, re.search(r"(\d+)x(\d+)x(\d+)", name).groups())
    return bm, bn


def _check_prefix(shapes, N, tile, launch, first, ntiles):
    """Every tile of every member exactly once: member i owns [first[i], first[i] + ntiles[i]) of its launch's grid, the ranges are back
    to back from 0 in member order, and ntiles[i] is the member's own grid on the tile."""
    bm, bn = _tile_dims(tile)
    nxt = {}
    for i, (nb, ho, wo) in enumerate(shapes):
        assert launch[i] == i // GROUP_MAX
        assert ntiles[i] == -(-nb * ho * wo // bm) * -(-N // bn)
        assert first[i] == nxt.get(launch[i], 0)
        nxt[launch[i]] = first[i] + ntiles[i]


@pytest.mark.parametrize("mode", (6, 0))
def test_prefix_covers_every_tile_once_and_the_tile_is_that_of_the_total(handle, mode):
    handle.mit_gemm_mode_set(mode)
    layer = dict(Cin=80, taps=9, N=80, split=1)
    # M < BM, M an exact multiple of BM (128 and 64 divide 2 * 48 * 64), odd sizes, a single row
    shapes = [(1, 3, 7), (2, 48, 64), (5, 48, 33), (1, 1, 1), (3, 48, 100)]
    tile, launch, first, ntiles = _plan(_group(shapes, **layer))
    total = sum(nb * ho * wo for nb, ho, wo in shapes)
    assert f"{tile}:1" == plan(handle, desc(NB=1, Ho=1, Wo=total, **layer))
    _check_prefix(shapes, 80, tile, launch, first, ntiles)
    assert sum(ntiles) == first[-1] + ntiles[-1]


def test_one_member_and_more_than_the_by_value_capacity(handle):
    handle.mit_gemm_mode_set(6)
    layer = dict(Cin=160, taps=2, N=320, split=1)
    tile, launch, first, ntiles = _plan(_group([(4, 6, 50)], **layer))
    assert launch == [0] and first == [0] and ntiles[0] > 0
    shapes = [(1 + i % 3, 6, 20 + 3 * i) for i in range(GROUP_MAX + 3)]
    tile, launch, first, ntiles = _plan(_group(shapes, **layer))
    assert launch[GROUP_MAX - 1] == 0 and launch[GROUP_MAX] == 1 and first[GROUP_MAX] == 0   # a second launch, its prefix from 0
    _check_prefix(shapes, 320, tile, launch, first, ntiles)


@pytest.mark.parametrize("mode", (6, 0))
def test_the_ocr_backbone_layers_run_grouped(handle, mode):
    """The seven spatial convolutions of the 48px OCR backbone (Cin, taps, N) over a page group's chunks: each takes a tile that has a
    grouped twin, whatever the group's size."""
    handle.mit_gemm_mode_set(mode)
    layers = ((4, 49, 40), (40, 4, 80), (80, 9, 80), (80, 4, 160), (160, 2, 320), (320, 2, 320), (320, 3, 320))
    for n_chunks, lines in ((3, 1), (32, 4), (32, 16)):
        shapes = [(lines, 6, 16 + 5 * i) for i in range(n_chunks)]
        for cin, taps, n in layers:
            tile, launch, first, ntiles = _plan(_group(shapes, Cin=cin, taps=taps, N=n, split=int(cin % 16 == 0)))
            assert min(launch) == 0, (mode, n_chunks, lines, cin, taps, n, tile)
            _check_prefix(shapes, n, tile, launch, first, ntiles)


def test_groups_that_fall_back_are_reported(handle):
    handle.mit_gemm_mode_set(6)
    shapes = [(2, 6, 9), (1, 6, 16), (3, 6, 5)]
    ok = dict(Cin=80, taps=9, N=80, split=1)
    assert _plan(_group(shapes, **ok))[1] == [0, 0, 0]
    # a tile without a grouped twin (N <= 4: the gemv kernel)
    tile, launch, _, _ = _plan(_group(shapes, Cin=64, taps=9, N=3))
    assert tile.startswith("gemv") and launch == [-1, -1, -1]
    # Z > 1, a live-block list, the row lookup
    assert _plan(_group(shapes, Z=8, **ok))[1] == [-1, -1, -1]
    descs = _group(shapes, **ok)
    descs[0].live_blocks, descs[0].live_start = 4096, 8192
    assert _plan(descs)[1] == [-1, -1, -1]
    descs = _group(shapes, **ok)
    descs[0].lut_rows, descs[0].lut1, descs[0].lut2, descs[0].lut_ld = 4096, 4096, 4096, 80
    assert _plan(descs)[1] == [-1, -1, -1]
    # one member whose offsets do not fit the buffer-load tile the others take: the whole group goes member by member
    descs = _group(shapes, **ok)
    far = desc(NB=1, Ho=64, Wo=64, a=FAKE_A, c=FAKE_C, **ok)
    far.a_ys = 1 << 24   # the last row starts 63 * 2^24 elements in: below 2^31 elements, past 2^31 bytes (the pixel stride is the group's)
    assert _plan(descs + [far])[1] == [-1, -1, -1, -1]
    # a member whose batch would be cut into runs (activations past 2^31 elements)
    assert _plan(_group([(2, 6, 9), (16, 2048, 1456)], Cin=64, taps=9, N=64, split=1))[1] == [-1, -1]


def test_refusals(handle):
    from manga_image_translator_amd import lib

    handle.mit_gemm_mode_set(6)
    descs = _group([(2, 6, 9), (1, 6, 16)], Cin=80, taps=9, N=80, split=1)
    descs[0].post.base = 4096
    with pytest.raises(RuntimeError, match="pre / post"):
        _plan(descs)
    descs = _group([(2, 6, 9), (1, 6, 0)], Cin=80, taps=9, N=80, split=1)   # an empty member is refused like an empty launch
    with pytest.raises(RuntimeError, match="empty problem"):
        _plan(descs)
    mem = (lib.MitConvGemmMember * 1)()
    assert handle.mit_conv_gemm_group_plan(C.byref(descs[0]), mem, 0, None, None, None, None) != 0
    assert handle.mit_conv_gemm_group(None, mem, 1, None) != 0
