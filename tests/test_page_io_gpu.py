"""The byte-level conversions at the ends of the engines: u8 page -> fp32 network input and fp32 map -> u8, with every byte value and every
k / 255 boundary enumerated.  These kernels claim the reference's exact fp32 expressions, so each test asserts BIT (fp32) or BYTE (u8)
equality with a numpy float32 restatement of the same expression, written out here beside the reference line the kernel's own comment
cites (manga_translator/...):

  mit_ocr_prep, mit_u8_to_f32_nhwc4 mode 0   (x - 127.5) / 127.5                           ocr/model_48px.py:115
  mit_u8_to_f32_nhwc4 mode 1                 x / 127.5 - 1                                 detection/default.py:19
  mit_u8_to_f32_nhwc4 mode 2                 x / 255
  mit_map_to_u8 mode 0                       (v * 255).astype(uint8): truncation           detection/ctd.py:41-44
  mit_map_to_u8 mode 1                       v > thr                                       ctd_utils/utils/db_utils.py:75
  mit_map_to_u8 mode 2                       (clip(v, 0, 1) * 255).astype(uint8)           upscaling/esrgan_pytorch.py:545
  mit_lama_prep(_padded)                     m = mask / 255 >= 0.5; (img / 255 * (1 - m), m)  inpainting/inpainting_lama_mpe.py:82-92, :604 (pad :560)
  mit_lama_post                              pred * m + (1 - m) * img, * 255 truncated, composited where mask >= 127   :726, :111, :59-60, :117
  mit_aot_prep                               (m, (img / 127.5 - 1) * (1 - m))              inpainting_lama_mpe.py:84-92, inpainting_aot.py:266

numpy's float32 arithmetic is IEEE, one rounding per operation: a build that turned `/ 127.5f` into a reciprocal multiply, or contracted
a product into a neighbouring sum where that changes a bit, fails here."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

f32 = np.float32
SENT = -7.0


def _L():
    from manga_image_translator_amd import lib, ops

    return lib, lib.load(), C.c_void_p(ops.current_stream())


def _bits_equal(got, ref):
    """fp32 arrays, compared as bit patterns (so -0.0 != 0.0)."""
    got, ref = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(ref, dtype=f32)
    return got.shape == ref.shape and np.array_equal(got.view(np.int32), ref.view(np.int32))


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- u8 -> fp32 NHWC4 ------------------------------------------------------------------------------------------------------------
def _all_bytes_image():
    """768 RGB pixels: every byte value 0..255 occurs in each of the three channel positions."""
    i = np.arange(768)
    img = np.stack([i % 256, (i + 85) % 256, (255 - i) % 256], -1).astype(np.uint8)
    for c in range(3):
        assert len(set(img[:, c].tolist())) == 256
    return img


def _u8_to_f32_ref(img, mode):
    x = img.astype(f32)
    if mode == 0:
        v = (x - f32(127.5)) / f32(127.5)
    elif mode == 1:
        v = x / f32(127.5) - f32(1.0)
    else:
        v = x / f32(255.0)
    assert v.dtype == f32
    return np.concatenate([v, np.zeros((*v.shape[:-1], 1), f32)], -1)


def _run_u8_to_f32(cuda, img, call):
    npix = img.shape[0]
    out = torch.full((npix + 4, 4), SENT, device=cuda)
    call(_dev(img, cuda), out)
    got = out.cpu().numpy()
    assert (got[npix:] == SENT).all()
    return got[:npix]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("npix", [1, 255, 768])
def test_u8_to_f32_nhwc4(cuda, mode, npix):
    lib, L, st = _L()
    img = _all_bytes_image()[:npix]
    got = _run_u8_to_f32(cuda, img, lambda i, o: lib.check(L.mit_u8_to_f32_nhwc4(i.data_ptr(), o.data_ptr(), npix, mode, st), "mit_u8_to_f32_nhwc4"))
    assert _bits_equal(got, _u8_to_f32_ref(img, mode))
    assert _bits_equal(got[:, 3], np.zeros(npix, f32))          # +0.0 exactly


def test_u8_to_f32_modes_0_and_1_round_differently(cuda):
    """(x - 127.5) / 127.5 and x / 127.5 - 1 are different roundings of one value: were the two outputs identical, the comparison above
    would not be seeing what it claims to see."""
    lib, L, st = _L()
    img = _all_bytes_image()
    got = [_run_u8_to_f32(cuda, img, lambda i, o, m=m: lib.check(L.mit_u8_to_f32_nhwc4(i.data_ptr(), o.data_ptr(), 768, m, st), "mit_u8_to_f32_nhwc4"))
           for m in (0, 1)]
    assert not _bits_equal(got[0], got[1])
    assert not _bits_equal(_u8_to_f32_ref(img, 0), _u8_to_f32_ref(img, 1))
    assert float(np.abs(got[0].astype(np.float64) - got[1].astype(np.float64)).max()) <= 2.0 ** -23   # ... of ONE value


@pytest.mark.parametrize("N,H,Wp", [(1, 1, 1), (1, 5, 51), (2, 48, 8)])      # 1, 255 and 768 pixels
def test_ocr_prep(cuda, N, H, Wp):
    lib, L, st = _L()
    npix = N * H * Wp
    img = _all_bytes_image()[:npix]
    got = _run_u8_to_f32(cuda, img, lambda i, o: lib.check(L.mit_ocr_prep(i.data_ptr(), o.data_ptr(), N, H, Wp, st), "mit_ocr_prep"))
    assert _bits_equal(got, _u8_to_f32_ref(img, 0))
    assert _bits_equal(got[:, 3], np.zeros(npix, f32))


# ---- fp32 -> u8 ------------------------------------------------------------------------------------------------------------------
def _around(vals):
    """Each value with its two fp32 neighbours."""
    vals = np.asarray(vals, f32)
    return np.concatenate([np.nextafter(vals, f32(-np.inf)), vals, np.nextafter(vals, f32(np.inf))]).astype(f32)


def _run_map_to_u8(cuda, v, mode, thr):
    lib, L, st = _L()
    n = v.size
    out = torch.full((n + 16,), 7, dtype=torch.uint8, device=cuda)
    vd = _dev(v, cuda)
    lib.check(L.mit_map_to_u8(vd.data_ptr(), out.data_ptr(), n, mode, float(thr), st), "mit_map_to_u8")
    got = out.cpu().numpy()
    assert (got[n:] == 7).all()
    return got[:n]


def _trunc_u8(v):
    p = v * f32(255.0)
    assert p.dtype == f32
    return p.astype(np.int32).astype(np.uint8)


def test_map_to_u8_truncation_at_every_boundary(cuda):
    """Mode 0: every k / 255 (fp32) and its neighbours, kept inside [0, 1] (outside it the cast is undefined in both implementations)."""
    v = _around(np.arange(256, dtype=f32) / f32(255.0))
    v = v[(v >= 0) & (v <= 1)]
    ref = _trunc_u8(v)
    assert set(ref.tolist()) == set(range(256)) and v.size == 3 * 256 - 2
    got = _run_map_to_u8(cuda, v, 0, 0.0)
    assert np.array_equal(got, ref), [(float(a), int(b), int(c)) for a, b, c in zip(v, got, ref) if b != c][:8]


def test_map_to_u8_clipped_truncation(cuda):
    """Mode 2: the same boundaries, and what the clip is for: -0.0, negatives, exactly 1, values above 1, 1 - 2^-24."""
    extra = np.array([-0.0, 0.0, -1e-30, -0.25, -3.0, -1e30, 1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 1.5, 2.0, 256.0, 1e30], f32)
    v = np.concatenate([_around(np.arange(256, dtype=f32) / f32(255.0)), extra])
    assert v[-len(extra) + 7] == f32(1.0) - f32(2.0 ** -24) and v[-len(extra) + 7] < 1
    ref = _trunc_u8(np.clip(v, f32(0.0), f32(1.0)))
    got = _run_map_to_u8(cuda, v, 2, 0.0)
    assert np.array_equal(got, ref), [(float(a), int(b), int(c)) for a, b, c in zip(v, got, ref) if b != c][:8]
    assert got[-1] == 255 and got[-len(extra) + 7] == 254 and (got[-len(extra):-len(extra) + 6] == 0).all()


@pytest.mark.parametrize("thr", [0.3, 0.7, 0.0])
def test_map_to_u8_threshold(cuda, thr):
    """Mode 1: strictly greater than thr."""
    t = f32(thr)
    v = np.array([t, np.nextafter(t, f32(-np.inf)), np.nextafter(t, f32(np.inf)), 0.0, -0.0, 1.0, -1.0], f32)
    ref = (v > t).astype(np.uint8)
    got = _run_map_to_u8(cuda, v, 1, t)
    assert np.array_equal(got, ref), (got, ref)
    assert got[0] == 0 and got[1] == 0 and got[2] == 1


# ---- LaMa / AOT prep -------------------------------------------------------------------------------------------------------------
def _enumerated_page(H=256, W=256):
    """mask[y, x] = y; pixel channels x, 255 - x, (7 x) & 255: at W = 256 every mask value meets every pixel value."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([x & 255, (255 - x) & 255, (x * 7) & 255], -1).astype(np.uint8)
    return img[None], (y & 255).astype(np.uint8)[None]


def _hole(mask):
    """m = (mask / 255 >= 0.5) as fp32 0 / 1   (inpainting_lama_mpe.py:85-87)"""
    return (mask.astype(f32) / f32(255.0) >= f32(0.5)).astype(f32)


def _lama_prep_ref(img, mask):
    m = _hole(mask)
    rgb = (img.astype(f32) / f32(255.0)) * (f32(1.0) - m)[..., None]
    return np.concatenate([rgb, m[..., None]], -1).astype(f32)


def _call_prep(cuda, name, img, mask):
    lib, L, st = _L()
    B, H, W = mask.shape
    out = torch.full((B * H * W + 4, 4), SENT, device=cuda)
    imgd, maskd = _dev(img, cuda), _dev(mask, cuda)
    lib.check(getattr(L, name)(imgd.data_ptr(), maskd.data_ptr(), out.data_ptr(), B, H, W, st), name)
    got = out.cpu().numpy()
    assert (got[B * H * W:] == SENT).all()
    return got[:B * H * W].reshape(B, H, W, 4)


def test_lama_prep_every_mask_value_meets_every_pixel_value(cuda):
    img, mask = _enumerated_page()
    got = _call_prep(cuda, "mit_lama_prep", img, mask)
    assert _bits_equal(got, _lama_prep_ref(img, mask))
    assert (got[0, :128, :, 3] == 0).all() and (got[0, 128:, :, 3] == 1).all()      # 127 / 255 < 0.5 <= 128 / 255
    assert (got[0, 128:, :, :3] == 0).all() and (got[0, 127, 1:, 0] > 0).all()


def test_aot_prep_every_mask_value_meets_every_pixel_value(cuda):
    img, mask = _enumerated_page()
    got = _call_prep(cuda, "mit_aot_prep", img, mask)
    m = _hole(mask)
    rgb = (img.astype(f32) / f32(127.5) - f32(1.0)) * (f32(1.0) - m)[..., None]
    assert rgb.dtype == f32
    assert _bits_equal(got, np.concatenate([m[..., None], rgb], -1))
    assert (got[0, :128, :, 0] == 0).all() and (got[0, 128:, :, 0] == 1).all()


@pytest.mark.parametrize("H,W,pad,Wp", [(4, 5, 3, 12), (6, 7, 1, 16), (5, 9, 0, 9), (8, 8, 3, 14)])
def test_lama_prep_padded_is_reflect_pad_of_lama_prep(cuda, H, W, pad, Wp):
    lib, L, st = _L()
    B = 2
    rng = np.random.default_rng(H * 100 + W * 10 + pad)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mask = rng.choice(np.array([0, 126, 127, 128, 129, 255], np.uint8), (B, H, W))
    prep = _call_prep(cuda, "mit_lama_prep", img, mask)
    assert _bits_equal(prep, _lama_prep_ref(img, mask))
    Hp, Wv = H + 2 * pad, W + 2 * pad
    out = torch.full((B * Hp * Wp + 4, 4), SENT, device=cuda)
    imgd, maskd = _dev(img, cuda), _dev(mask, cuda)
    lib.check(L.mit_lama_prep_padded(imgd.data_ptr(), maskd.data_ptr(), out.data_ptr(), B, H, W, pad, Wp, st), "mit_lama_prep_padded")
    got = out.cpu().numpy()
    assert (got[B * Hp * Wp:] == SENT).all()
    got = got[:B * Hp * Wp].reshape(B, Hp, Wp, 4)
    assert _bits_equal(got[:, :, :Wv], np.pad(prep, ((0, 0), (pad, pad), (pad, pad), (0, 0)), mode="reflect"))
    assert _bits_equal(got[:, :, Wv:], np.zeros((B, Hp, Wp - Wv, 4), f32))          # the surplus columns: +0.0 in all four channels


# ---- LaMa composite --------------------------------------------------------------------------------------------------------------
def _lama_post_ref(pred, img, mask, composite):
    m = _hole(mask)[..., None]
    im = (img.astype(f32) / f32(255.0)) * (f32(1.0) - m)
    v = pred * m + (f32(1.0) - m) * im                                              # :726 (m is 0 or 1: every product and the sum are exact)
    assert v.dtype == f32
    q = (v * f32(255.0)).astype(np.int32).astype(np.uint8)                         # :111
    keep = np.full(mask.shape, True) if not composite else mask >= 127              # :59-60, :117
    return np.where(keep[..., None], q, img)


@pytest.mark.parametrize("composite", [0, 1])
@pytest.mark.parametrize("pixstride", [3, 4])
def test_lama_post(cuda, composite, pixstride):
    lib, L, st = _L()
    H, W = 256, 64
    y, x = np.mgrid[0:H, 0:W]
    mask = y.astype(np.uint8)[None]
    img = np.stack([(3 * x + c + 192 * y) & 255 for c in range(3)], -1).astype(np.uint8)[None]
    vals = _around(np.arange(256, dtype=f32) / f32(255.0))                          # 768 values: k / 255 and its two neighbours
    pred = vals[np.arange(H * W * 3) % vals.size].reshape(1, H, W, 3)
    for r in (0, 100, 127, 128, 200):                                               # 4 rows hold all 768
        assert len(set(pred[0, r:r + 4].ravel().tolist())) == 768
    ref = _lama_post_ref(pred, img, mask, composite)
    buf = np.full((1, H, W, pixstride), 1e30, f32)
    buf[..., :3] = pred
    out = torch.full((H * W * 3 + 16,), 7, dtype=torch.uint8, device=cuda)
    predd, imgd, maskd = _dev(buf, cuda), _dev(img, cuda), _dev(mask, cuda)
    lib.check(L.mit_lama_post(predd.data_ptr(), pixstride, imgd.data_ptr(), maskd.data_ptr(), out.data_ptr(), 1, H, W,
                              composite, st), "mit_lama_post")
    got = out.cpu().numpy()
    assert (got[H * W * 3:] == 7).all()
    got = got[:H * W * 3].reshape(1, H, W, 3)
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    # the two rows that tell the two thresholds apart.  Row 127: below mask / 255 >= 0.5, so its value derives from the page,
    # (uint8)(img / 255 * 255), yet at or above the compositing threshold 127, so it is that derived value and not the page byte that
    # is kept ...
    page_derived = ((img.astype(f32) / f32(255.0)) * f32(255.0)).astype(np.int32).astype(np.uint8)
    assert np.array_equal(got[0, 127], page_derived[0, 127])
    # ... (for every byte the derived value IS the byte: fl(fl(x / 255) * 255) truncates to x for x = 0..255, so on row 127 the two
    # thresholds cannot disagree in the output; the assertion pins that fact, on which the composite relies)
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(((b.astype(f32) / f32(255.0)) * f32(255.0)).astype(np.int32).astype(np.uint8), b)
    # ... row 128 is the first that takes the prediction, with or without compositing; row 126 is the last the composite hands back
    assert np.array_equal(got[0, 128], _trunc_u8(pred[0, 128]))
    assert not np.array_equal(got[0, 128], img[0, 128])
    assert np.array_equal(got[0, 126], img[0, 126])
