"""``imgproc.pil_resize_u8`` (mit_resample_pil_u8, csrc/pil_resample.hip) against the REAL Pillow and against the numpy form, byte for
byte: the table of tests/test_pil_resample.py, two pages at once, one-pass resizes, the packed and the single-byte vertical path, the
sizes of the real workload scaled down, and an upscaling case whose border windows are shorter than ksize."""
import numpy as np
import pytest
import torch
from PIL import Image

from test_pil_resample import CASES, FILTERS, pillow, planted

pytestmark = pytest.mark.gpu


def _check(cuda, pages, dst_hw, f):
    """pages: list of [H,W,C] arrays of one size -> every page equals its own Pillow result and the numpy form; input untouched."""
    from manga_image_translator_amd import imgproc

    h, w = dst_hw
    t = torch.from_numpy(np.stack(pages)).to(cuda)
    keep = t.clone()
    out = imgproc.pil_resize_u8(t, (w, h), f)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(pages), h, w, pages[0].shape[2]) and out.is_contiguous()
    assert torch.equal(t, keep)
    got = out.cpu().numpy()
    for i, p in enumerate(pages):
        c1 = p.shape[2] == 1
        want = pillow(p, w, h, f)
        g = got[i, ..., 0] if c1 else got[i]
        assert np.array_equal(g, want), (i, int(np.abs(g.astype(np.int32) - want.astype(np.int32)).max()))
        assert np.array_equal(g, imgproc.pil_resize_u8_host(p[..., 0] if c1 else p, (w, h), f))


@pytest.mark.parametrize("src,dst,c,f", CASES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}-c{c}-{f}" for s, d, c, f in CASES])
def test_device_equals_pillow(cuda, src, dst, c, f):
    _check(cuda, [planted(src[0] * 131 + src[1], src[0], src[1], c)], dst, f)


@pytest.mark.parametrize("src,dst,c,f", CASES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}-c{c}-{f}" for s, d, c, f in CASES])
def test_two_pages_each_equal_their_own_pillow_result(cuda, src, dst, c, f):
    _check(cuda, [planted(7 + src[0], src[0], src[1], c), planted(1000 + src[1], src[0], src[1], c)], dst, f)


EXTRA = [
    ("width-only", (40, 97), (40, 31), 3, "bicubic"),          # horizontal pass alone
    ("height-only", (61, 24), (19, 24), 3, "bilinear"),        # vertical pass alone (W * C = 72: packed stores)
    ("height-only-c1-odd", (61, 25), (90, 25), 1, "bicubic"),  # vertical pass alone, single-byte stores, upscaling
    ("workload-half", (1024, 1536), (512, 768), 3, "bilinear"),
    ("bicubic-down", (512, 768), (211, 317), 3, "bicubic"),
    ("wc-not-multiple-of-4", (33, 97), (21, 73), 3, "bilinear"),   # 73 * 3 = 219
    ("wc-multiple-of-4", (33, 97), (21, 72), 3, "bicubic"),        # 72 * 3 = 216
    ("upscale-short-border-windows", (17, 23), (51, 40), 3, "bicubic"),
]


@pytest.mark.parametrize("name,src,dst,c,f", EXTRA, ids=[e[0] for e in EXTRA])
def test_further_cases(cuda, name, src, dst, c, f):
    _check(cuda, [planted(len(name), src[0], src[1], c)], dst, f)


def test_one_pass_runs_when_one_side_changes(cuda):
    """A width-only and a height-only resize launch exactly one resampling kernel each (the library's kernel probe counts them)."""
    import ctypes as C

    from manga_image_translator_amd import imgproc, lib as L

    lib = L.load()
    t = torch.from_numpy(planted(5, 40, 52, 3)[None]).to(cuda)
    for size, name in (((30, 40), b"pil_horiz_kernel"), ((52, 20), b"pil_vert_kernel")):
        L.check(lib.mit_prof_enable(1))
        try:
            imgproc.pil_resize_u8(t, size, "bilinear")
            torch.cuda.synchronize()
            stats = (L.MitProfKernelStat * 64)()
            n = C.c_int(0)
            L.check(lib.mit_prof_kernels_read(stats, 64, C.byref(n)))
        finally:
            L.check(lib.mit_prof_enable(0))
        seen = {stats[i].name: stats[i].launches for i in range(n.value) if stats[i].name.startswith(b"pil_")}
        assert seen == {name: 1}


def test_same_size_returns_a_copy_and_bad_operands_raise(cuda):
    from manga_image_translator_amd import imgproc

    t = torch.from_numpy(planted(2, 12, 20, 3)[None]).to(cuda)
    same = imgproc.pil_resize_u8(t, (20, 12), "bicubic")
    assert torch.equal(same, t) and same.data_ptr() != t.data_ptr()
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8(t, (10, 6), "lanczos")
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8(t.float(), (10, 6), "bilinear")
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8(t[0], (10, 6), "bilinear")
    with pytest.raises(ValueError):
        imgproc.pil_resize_u8(torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device=cuda), (4, 4), "bilinear")   # RGBA is out of scope
