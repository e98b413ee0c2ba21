"""mit_conv_gemm_group on the device: a layer over several images as ONE grid (the members' grids back to back) gives every image the
bits of mit_conv_gemm on that image alone — torch.equal throughout, in GEMM modes 6 and 0.  Shapes are the smallest that still cross the
interesting edges: members of 1, 2 and 3 images, widths that are no multiple of anything, a member smaller than one tile beside one of
several tiles."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NBS, H, WS = (2, 1, 3), 6, (9, 16, 5)   # the group shape of the layer tests


def _bn(c, g):
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5, 1e-5)


def _layers(cuda):
    """name -> (Conv2d, input channels of the activation): the four layer kinds of the 48px OCR backbone's spatial convolutions."""
    from manga_image_translator_amd import ops

    g = torch.Generator().manual_seed(3)
    w = lambda co, ci, kh, kw: torch.randn(co, ci, kh, kw, generator=g) / (ci * kh * kw) ** 0.5
    return {
        "7x7_pad3_3to40_bn_relu": (ops.Conv2d(w(40, 3, 7, 7), torch.randn(40, generator=g), padding=3, bn=_bn(40, g), act=ops.ACT_RELU, device=cuda), 4),
        "2x2_s2_40to80": (ops.Conv2d(w(80, 40, 2, 2), torch.randn(80, generator=g), stride=2, bn=_bn(80, g), act=ops.ACT_RELU, device=cuda), 40),
        "3x3_pad1_80to80": (ops.Conv2d(w(80, 80, 3, 3), torch.randn(80, generator=g), padding=1, bn=_bn(80, g), act=ops.ACT_RELU, device=cuda), 80),
        "2x1_s21_32to64": (ops.Conv2d(w(64, 32, 2, 1), torch.randn(64, generator=g), stride=(2, 1), bn=_bn(64, g), act=ops.ACT_RELU, device=cuda), 32),
    }


def _members(conv, cin, shapes, cuda, seed=0):
    g = torch.Generator(device=cuda).manual_seed(seed)
    xs = [torch.randn(nb, h, w, cin, generator=g, device=cuda) for nb, h, w in shapes]
    if cin == 4:
        for x in xs:
            x[..., 3] = 0   # the padded fourth channel of an RGB input
    outs = lambda: [torch.full((x.shape[0], *conv.out_hw(x.shape[1], x.shape[2]), conv.Cout), float("nan"), device=cuda) for x in xs]
    return xs, outs


def _run_both(conv, xs, outs, **desc_kw):
    """(grouped results, member-by-member results) of the same descriptors."""
    from manga_image_translator_amd import ops

    got, ref = outs(), outs()
    ops.launch_conv_gemm_group([conv.desc(x, o, **desc_kw) for x, o in zip(xs, got)])
    for x, o in zip(xs, ref):
        ops.launch_conv_gemm(conv.desc(x, o, **desc_kw))
    torch.cuda.synchronize()
    return got, ref


@pytest.mark.parametrize("name", ["7x7_pad3_3to40_bn_relu", "2x2_s2_40to80", "3x3_pad1_80to80", "2x1_s21_32to64"])
def test_grouped_launch_equals_member_by_member(cuda, gemm_mode, name):
    from manga_image_translator_amd import ops

    conv, cin = _layers(cuda)[name]
    shapes = [(nb, H, w) for nb, w in zip(NBS, WS)]
    xs, outs = _members(conv, cin, shapes, cuda)
    tile, launch, _, _ = ops.conv_gemm_group_plan([conv.desc(x, o) for x, o in zip(xs, outs())])
    assert launch == [0, 0, 0], (name, tile)   # the grouped kernel is what runs, not the fallback
    got, ref = _run_both(conv, xs, outs)
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and torch.isfinite(a).all() and a.abs().sum() > 0


# Launches large enough for the 128-row tiles (the choice takes the 64 x 64 tiles below one full round of them: 768 split / 1280 fp32
# tiles of 128 x 64): layer -> (Conv2d arguments, group shape, the tile in mode 6, the tile in mode 0)
LARGE = {
    "3x3_80to80": (dict(co=80, ci=80, kh=3, kw=3, padding=1), [(2, 48, 300), (1, 48, 290), (3, 48, 292)], "split128x96x16p6u", "fast128x128x16w4c"),
    "2x2_s2_80to160": (dict(co=160, ci=80, kh=2, kw=2, stride=2), [(2, 48, 760), (1, 48, 780), (3, 48, 768)], "split128x64x16p6u", "fast128x64x16w5c"),
    "2x1_s21_320to320": (dict(co=320, ci=320, kh=2, kw=1, stride=(2, 1)), [(2, 48, 230), (1, 48, 236), (3, 48, 232)], "split128x160x16p6u", "fast128x64x16w5c"),
}


@pytest.mark.parametrize("name", sorted(LARGE))
def test_full_size_tiles(cuda, gemm_mode, name):
    from manga_image_translator_amd import ops

    kw, shapes, tile6, tile0 = LARGE[name]
    kw = dict(kw)
    g = torch.Generator().manual_seed(7)
    co, ci, kh, kw_ = kw.pop("co"), kw.pop("ci"), kw.pop("kh"), kw.pop("kw")
    conv = ops.Conv2d(torch.randn(co, ci, kh, kw_, generator=g) / (ci * kh * kw_) ** 0.5, torch.randn(co, generator=g), bn=_bn(co, g),
                      act=ops.ACT_RELU, device=cuda, **kw)
    xs, outs = _members(conv, ci, shapes, cuda, seed=8)
    tile, launch, _, _ = ops.conv_gemm_group_plan([conv.desc(x, o) for x, o in zip(xs, outs())])
    assert launch == [0, 0, 0] and tile == (tile6 if gemm_mode == 6 else tile0)
    got, ref = _run_both(conv, xs, outs)
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and torch.isfinite(a).all() and a.abs().sum() > 0


def test_member_smaller_than_a_tile_beside_one_of_several_tiles(cuda, gemm_mode):
    conv, cin = _layers(cuda)["3x3_pad1_80to80"]
    xs, outs = _members(conv, cin, [(1, 2, 3), (3, 6, 40), (1, 1, 1)], cuda, seed=1)   # 6 rows, 720 rows, 1 row
    got, ref = _run_both(conv, xs, outs)
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and torch.isfinite(a).all()


def test_more_members_than_travel_in_one_launch(cuda, gemm_mode):
    from manga_image_translator_amd import ops

    conv, cin = _layers(cuda)["2x1_s21_32to64"]
    shapes = [(1 + i % 2, 4, 3 + i % 7) for i in range(35)]
    xs, outs = _members(conv, cin, shapes, cuda, seed=2)
    _, launch, _, _ = ops.conv_gemm_group_plan([conv.desc(x, o) for x, o in zip(xs, outs())])
    assert launch[31] == 0 and launch[32] == 1
    got, ref = _run_both(conv, xs, outs)
    for a, b in zip(got, ref):
        assert torch.equal(a, b) and torch.isfinite(a).all()


def test_descriptor_with_a_live_list_takes_the_fallback(cuda, gemm_mode):
    """A live-block list belongs to one image size: the group (members of one size, every block listed) runs member by member."""
    from manga_image_translator_amd import ops

    conv, cin = _layers(cuda)["3x3_pad1_80to80"]
    xs, outs = _members(conv, cin, [(2, 6, 9)] * 3, cuda, seed=4)
    live = ops.full_block_list(2, 6, 9, cuda)
    _, launch, _, _ = ops.conv_gemm_group_plan([conv.desc(x, o, live=live) for x, o in zip(xs, outs())])
    assert launch == [-1, -1, -1]
    got, ref = _run_both(conv, xs, outs, live=live)
    dense = outs()
    for x, o in zip(xs, dense):
        conv(x, out=o)
    torch.cuda.synchronize()
    for a, b, d in zip(got, ref, dense):
        assert torch.equal(a, b) and torch.equal(a, d)


def test_probe_files_a_grouped_launch_once_with_the_summed_flops(cuda, gemm_mode):
    from manga_image_translator_amd import lib as L, ops

    conv, cin = _layers(cuda)["3x3_pad1_80to80"]
    shapes = [(nb, H, w) for nb, w in zip(NBS, WS)]
    xs, outs = _members(conv, cin, shapes, cuda)
    res = outs()
    descs = [conv.desc(x, o) for x, o in zip(xs, res)]
    tile, launch, _, _ = ops.conv_gemm_group_plan(descs)
    assert launch == [0, 0, 0]
    lib = L.load()
    L.check(lib.mit_prof_enable(1), "mit_prof_enable")
    try:
        ops.launch_conv_gemm_group(descs)
        torch.cuda.synchronize()
        stats, n = (L.MitProfStat * 64)(), C.c_int(0)
        L.check(lib.mit_prof_read(stats, 64, C.byref(n)), "mit_prof_read")
    finally:
        L.check(lib.mit_prof_enable(0), "mit_prof_enable")
    by_name = {lib.mit_conv_gemm_config_name(i).decode(): stats[i] for i in range(n.value)}
    assert sum(s.launches for s in by_name.values()) == 1 and by_name[tile].launches == 1
    rows = sum(nb * H * w for nb, w in zip(NBS, WS))
    assert by_name[tile].exec_flops == 2.0 * rows * 80 * (9 * 80) and by_name[tile].alg_flops == by_name[tile].exec_flops


@pytest.fixture(scope="module")
def engine(cuda, shipped_mode):
    from manga_image_translator_amd import ocr48, ocr_schema, synth

    D = 300
    with shipped_mode():
        return ocr48.Ocr48Engine(synth.synth_state_dict(ocr_schema.ocr48_schema(D)), D, device=cuda)


def test_encode_group_equals_its_per_chunk_launches(cuda, gemm_mode, engine):
    """Three chunks of 5 / 3 / 1 lines, padded widths 32 / 68 / 100: the grouped stem / downsampling convs and the one-launch input
    conversion against ``grouped_convs = False`` — the pooled cross-attention keys and values are the same bits."""
    eng = engine
    rng = np.random.default_rng(5)
    regions = [torch.from_numpy(rng.integers(0, 256, size=(n, 48, wp, 3), dtype=np.uint8)).to(cuda) for n, wp in ((5, 32), (3, 68), (1, 100))]
    Ls = [eng.memory_len(r.shape[2]) for r in regions]
    klens = torch.tensor([eng.valid_len(r.shape[2] - 3 * i, L) for r, L in zip(regions, Ls) for i in range(r.shape[0])], dtype=torch.int32, device=cuda)
    assert eng.grouped_convs
    gk, gv, _ = eng.encode_group(regions, klens, max(Ls))
    gk, gv = gk.clone(), gv.clone()
    eng.grouped_convs = False
    try:
        pk, pv, _ = eng.encode_group(regions, klens, max(Ls))
    finally:
        eng.grouped_convs = True
    torch.cuda.synchronize()
    assert torch.equal(gk, pk) and torch.equal(gv, pv)
    assert torch.isfinite(gk).all() and gk.abs().sum() > 0
