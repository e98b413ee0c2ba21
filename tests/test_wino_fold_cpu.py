"""The Winograd pre-operand of mit_conv_gemm (MitConvGemm.wino_m) on the host: a pure-Python mirror of the row <-> tile mapping the
epilogue relies on (the 16 rows a lane holds of one 32 x 32 accumulator block are, under the 8 x 8 block row order, one aligned 4 x 4
Winograd tile), and what the launcher refuses, through mit_conv_gemm_plan — no GPU."""
import pytest

from _conv_gemm_plan_cases import desc, plan

FAKE_LIST, FAKE_START, FAKE_M = 65536, 131072, 262144


# ---- mirrors of csrc/conv_gemm_kernels.h ----
def decode_row(m, blocks, Ho, Wo):
    """decode_row's list form for one run starting at image 0: row m -> (nb, oy, ox) or None for a dead row."""
    blk = m >> 6
    if blk >= len(blocks):
        return None
    bw = (Wo + 7) >> 3
    bpi = ((Ho + 7) >> 3) * bw
    nb, rem = divmod(blocks[blk], bpi)
    by, bx = divmod(rem, bw)
    oy, ox = by * 8 + ((m & 63) >> 3), bx * 8 + (m & 7)
    return (nb, oy, ox) if oy < Ho and ox < Wo else None


def lane_rows(wm0, mi, lh):
    """epilogue_store: the row (inside the workgroup's tile) behind accumulator element r of block mi, for the lanes of half lh."""
    return [wm0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh for r in range(16)]


def wino_tile(m0, wm0, mi, lh, blocks, Ho, Wo):
    """wino_pre_add: the tile a lane loads for block mi — decoded from its r = 0 row — or None when it loads nothing."""
    d = decode_row(m0 + wm0 + mi * 32 + 4 * lh, blocks, Ho, Wo)
    return None if d is None else (d[0], d[1] >> 2, d[2] >> 2)


# (BM, WAVES_M) of every fast / split tile shape in conv_gemm_cfgs.inc
TILINGS = ((128, 2), (128, 1), (128, 4), (64, 2), (192, 2))


@pytest.mark.parametrize("Wo", [16, 18, 20, 22], ids=lambda w: f"Wo%8={w % 8}")
@pytest.mark.parametrize("Ho", [8, 10, 13])
def test_a_lanes_rows_are_one_aligned_tile(Ho, Wo):
    NB = 2
    th, tw = (Ho + 3) // 4, (Wo + 3) // 4
    bpi = ((Ho + 7) // 8) * ((Wo + 7) // 8)
    blocks = list(range(NB * bpi))                     # a dense layer: every block listed
    M = len(blocks) * 64
    for BM, waves_m in TILINGS:
        WM = BM // waves_m
        seen = {}
        for m0 in range(0, M + BM, BM):                # one tile past the end: rows past the list
            for wm0 in range(0, BM, WM):
                for mi in range(WM // 32):
                    for lh in (0, 1):                  # (every lane of a half shares the rows: the lane index only picks the column)
                        tile = wino_tile(m0, wm0, mi, lh, blocks, Ho, Wo)
                        live = 0
                        for r, row in enumerate(lane_rows(wm0, mi, lh)):
                            d = decode_row(m0 + row, blocks, Ho, Wo)
                            if d is None:
                                continue               # a dead row: nothing is stored, whatever was added
                            live += 1
                            nb, oy, ox = d
                            assert tile is not None, "a live row whose lane loads no tile"
                            assert tile == (nb, oy >> 2, ox >> 2), "rows of two tiles in one lane"
                            assert (oy & 3, ox & 3) == (r >> 2, r & 3), "accumulator element r is not tile element (r >> 2, r & 3)"
                            assert (nb, oy, ox) not in seen
                            seen[(nb, oy, ox)] = tile
                        if tile is None:
                            assert live == 0
                        else:                          # what is loaded exists: the tile lies inside [NB][th][tw]
                            assert tile[0] < NB and tile[1] < th and tile[2] < tw
                            assert live >= 1           # its first position is a live row
        assert len(seen) == NB * Ho * Wo, "every output position is owned exactly once"


def test_second_tile_of_an_edge_block_past_tw_loads_nothing():
    Ho, Wo = 8, 12                                      # tw = 3: block column 1 holds tile column 2 only
    blocks = list(range(2))
    assert wino_tile(64, 0, 0, 0, blocks, Ho, Wo) == (0, 0, 2)
    assert wino_tile(64, 0, 0, 1, blocks, Ho, Wo) is None
    assert wino_tile(64, 0, 1, 1, blocks, Ho, Wo) is None


# ---- the launcher ----
@pytest.fixture(scope="module")
def handle():
    from manga_image_translator_amd import lib

    h = lib.load(build_if_missing=True)
    mode, mt = h.mit_gemm_mode_get(), h.mit_gemm_split_min_tiles(-1)
    h.mit_gemm_split_min_tiles(0)
    yield h
    h.mit_gemm_mode_set(mode)
    h.mit_gemm_split_min_tiles(mt)


ST_OUT = dict(NB=16, Ho=256, Wo=182, Cin=192, taps=1, N=384)   # LaMa's conv2 at 16 pages


def folded(**over):
    kw = dict(ST_OUT, **{k: v for k, v in over.items() if k in ("NB", "Ho", "Wo", "Cin", "taps", "N", "Z", "split")})
    d = desc(**kw)
    d.live_blocks, d.live_start = FAKE_LIST, FAKE_START
    th, tw = (d.Ho + 3) // 4, (d.Wo + 3) // 4
    d.wino_m, d.wino_zs, d.wino_n, d.wino_th, d.wino_tw = FAKE_M, d.NB * th * tw * d.N, d.N, th, tw
    return d


def test_fold_keeps_the_tile_of_the_plain_launch(handle):
    for mode, split, want in ((6, 1, "split128x128x16p6u"), (0, 0, "fast128x128x16w4c")):
        assert handle.mit_gemm_mode_set(mode) == 0
        got = plan(handle, folded(split=split))
        assert got == f"{want}:16", got
        assert got == plan(handle, desc(**ST_OUT, split=split))


def test_fold_is_refused_where_the_mapping_does_not_hold(handle):
    handle.mit_gemm_mode_set(6)

    def refused(d, text):
        got = plan(handle, d)
        assert got.startswith("refused") and text in got, got

    d = folded(split=1)
    d.live_blocks = d.live_start = None
    refused(d, "block row order")
    refused(folded(split=1, taps=4), "one tap")
    d = folded(split=1)
    d.sy = d.sx = 2
    refused(d, "stride")
    d = folded(split=1)
    d.pre.base = 4096
    refused(d, "pre operand")
    d = folded(split=1)
    d.c.nsplit, d.c.nhi = 192, 1 << 20
    refused(d, "column-split")
    d = folded(split=1)
    d.post.base, d.post.nsplit, d.post.nhi = 4096, 192, 1 << 20
    refused(d, "column-split")
    refused(folded(split=1, N=382), "N % 4")
    d = folded(split=1)
    d.wino_n = 388
    refused(d, "wino_n")
    d = folded(split=1)
    d.wino_tw += 1
    refused(d, "ceil")
    d = folded(split=1)
    d.wino_zs -= 4
    refused(d, "wino_zs")
    refused(folded(NB=1, Ho=24, Wo=24, Cin=12, N=64), "live-block list")   # the generic kernel reads neither
