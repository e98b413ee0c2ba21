"""Argument checks of the NHWC helper and page I/O entries (ctd_kernels.hip, the helper section of ocr_kernels.hip, the prep kernels of
lama_kernels.hip and aot_kernels.hip).  Every check runs before any HIP call, so a refusal is observable without a GPU
(test_capi.py::test_error_channel_without_gpu): the pointers below are fake, non-null and 16-byte aligned, and are never dereferenced
because every call here is refused first."""
import ctypes as C

import pytest

P_IN, P_OUT, P_A, P_B = 4096, 8192, 12288, 16384


@pytest.fixture(scope="module")
def L():
    from manga_image_translator_amd import lib

    return lib.load()


def _refused(L, rc, text):
    assert rc != 0, text
    assert text.encode() in L.mit_last_error(), (text, L.mit_last_error())


def test_map_to_u8_refuses_unknown_modes(L):
    """Anything outside 0 / 1 / 2 used to run silently as mode 2."""
    for mode in (3, -1, 255):
        _refused(L, L.mit_map_to_u8(P_IN, P_OUT, 16, mode, 0.0, None), "mit_map_to_u8: bad mode")
    _refused(L, L.mit_map_to_u8(None, P_OUT, 16, 0, 0.0, None), "mit_map_to_u8: null pointer")


def test_u8_to_f32_refuses_mode_3(L):
    _refused(L, L.mit_u8_to_f32_nhwc4(P_IN, P_OUT, 16, 3, None), "mit_u8_to_f32_nhwc4: bad mode 3")
    _refused(L, L.mit_u8_to_f32_nhwc4(P_IN, P_OUT, 16, -1, None), "mit_u8_to_f32_nhwc4: bad mode -1")


def _tables(lib, imax=2048, pmax=1024):
    tb = lib.MitXposTables()
    tb.cos_t, tb.sin_t, tb.scale_t, tb.iscale_t = P_A, P_A + 64, P_B, P_B + 64
    tb.imax, tb.pmax = imax, pmax
    return tb


def test_xpos_rotate_refuses_positions_outside_the_tables(L):
    from manga_image_translator_amd import lib

    tb = _tables(lib)
    imax, pmax, T = tb.imax, tb.pmax, 4

    def call(i0, p0):
        return L.mit_xpos_rotate(P_IN, 960 * T, 960, P_OUT, 320 * T, 320, 2, T, i0, p0, 0, C.byref(tb), None)

    # i0 < 0 used to pass: check_tables bounded only the upper end, the kernel would have read before the cos / sin tables
    for i0 in (-1, -T, -imax):
        _refused(L, call(i0, 0), "mit_xpos_rotate: XPOS position out of table range")
    _refused(L, call(imax + 1 - T, 0), "mit_xpos_rotate: XPOS position out of table range")      # i0 + T == imax + 1
    _refused(L, call(0, -pmax - 1), "mit_xpos_rotate: XPOS position out of table range")         # p0 == -pmax - 1
    _refused(L, call(0, pmax - T + 1), "mit_xpos_rotate: XPOS position out of table range")      # p0 + T - 1 == pmax
    _refused(L, L.mit_xpos_rotate(P_IN, 960 * T, 960, P_OUT, 320 * T, 320, 2, T, 0, 0, 0, None, None), "mit_xpos_rotate: null XPOS tables")
    empty = lib.MitXposTables()
    _refused(L, L.mit_xpos_rotate(P_IN, 960 * T, 960, P_OUT, 320 * T, 320, 2, T, 0, 0, 0, C.byref(empty), None), "mit_xpos_rotate: null XPOS tables")


def test_maxpool_refuses_nonpositive_and_even_k(L):
    """-1 is "odd": k < 1 used to pass the parity check."""
    text = "mit_maxpool_nhwc: C/strides % 4, odd k >= 1"     # the whole text: a launch that fails for want of a GPU also returns nonzero
    for k in (-1, 0, -3, 2, 4):
        _refused(L, L.mit_maxpool_nhwc(P_IN, 8, P_OUT, 8, 1, 4, 4, 8, k, None), text)
    _refused(L, L.mit_maxpool_nhwc(P_IN, 8, P_OUT, 8, 1, 4, 4, 6, 3, None), text)   # C % 4
    _refused(L, L.mit_maxpool_nhwc(P_IN, 10, P_OUT, 8, 1, 4, 4, 8, 3, None), text)  # stride % 4


def test_pixel_stride_below_C_is_refused(L):
    """A pixel stride smaller than C makes neighbouring pixels overlap: the stores of two threads race."""
    msg = "pixel stride smaller than C"
    for ips, ops_ in ((4, 8), (8, 4), (0, 8), (8, -8)):
        _refused(L, L.mit_maxpool_nhwc(P_IN, ips, P_OUT, ops_, 1, 4, 4, 8, 3, None), "mit_maxpool_nhwc: " + msg)
        _refused(L, L.mit_avgpool2_nhwc(P_IN, ips, P_OUT, ops_, 1, 2, 2, 8, None), "mit_avgpool2_nhwc: " + msg)
        _refused(L, L.mit_copy_channels(P_IN, ips, P_OUT, ops_, 16, 8, None), "mit_copy_channels: " + msg)
        _refused(L, L.mit_affine_act_nhwc(P_IN, ips, P_A, P_B, P_OUT, ops_, 16, 8, 1, None), "mit_affine_act_nhwc: " + msg)
    # the C % 4 / stride % 4 checks these four already had
    _refused(L, L.mit_avgpool2_nhwc(P_IN, 8, P_OUT, 10, 1, 2, 2, 8, None), "mit_avgpool2_nhwc: C/strides")
    _refused(L, L.mit_copy_channels(P_IN, 8, P_OUT, 8, 16, 6, None), "mit_copy_channels: C/strides")
    _refused(L, L.mit_affine_act_nhwc(P_IN, 10, P_A, P_B, P_OUT, 8, 16, 8, 1, None), "mit_affine_act_nhwc: C and pixel strides")


def test_axpy_refuses_ragged_length_and_misaligned_pointers(L):
    text = "mit_axpy: n % 4 == 0 and 16-byte aligned pointers required"
    _refused(L, L.mit_axpy(P_OUT, 0.2, P_IN, P_A, 1026, None), text)
    for out, x, y in ((P_OUT + 4, P_IN, P_A), (P_OUT, P_IN + 8, P_A), (P_OUT, P_IN, P_A + 12)):
        _refused(L, L.mit_axpy(out, 0.2, x, y, 1028, None), text)
    _refused(L, L.mit_axpy(P_OUT, 0.2, None, P_A, 1028, None), "mit_axpy: null pointer")


def test_aot_prep_refuses_misaligned_output(L):
    _refused(L, L.mit_aot_prep(P_IN, P_A, P_OUT + 4, 1, 4, 4, None), "mit_aot_prep: output must be 16-byte aligned")
    _refused(L, L.mit_aot_prep(P_IN, P_A, P_OUT, 1, 0, 4, None), "mit_aot_prep: empty page")


def test_layernorm_refuses_widths_a_lane_cannot_hold(L):
    for D in (0, 513, -8):
        _refused(L, L.mit_layernorm(P_IN, 520, P_A, P_B, P_OUT, 520, 4, D, 1e-5, None), "mit_layernorm: D out of range")


def test_strided_pools_refuse_bad_geometry(L):
    # 2 p > k
    _refused(L, L.mit_maxpool2d_nhwc(P_IN, P_OUT, 2, 8, 8, 4, 3, 2, 2, None), "mit_maxpool2d_nhwc: bad geometry")
    _refused(L, L.mit_avgpool_nhwc(P_IN, P_OUT, 2, 8, 8, 4, 3, 3, 1, 1, 2, 1, None), "mit_avgpool_nhwc: bad geometry")
    _refused(L, L.mit_avgpool_nhwc(P_IN, P_OUT, 2, 8, 8, 4, 2, 2, 2, 1, 0, 2, None), "mit_avgpool_nhwc: bad geometry")
    # C % 4
    _refused(L, L.mit_maxpool2d_nhwc(P_IN, P_OUT, 2, 8, 8, 6, 3, 2, 1, None), "mit_maxpool2d_nhwc: bad geometry")
    _refused(L, L.mit_avgpool_nhwc(P_IN, P_OUT, 2, 8, 8, 6, 2, 2, 2, 2, 0, 0, None), "mit_avgpool_nhwc: bad geometry")
    # no output pixel: the window does not fit (1 + 2 * 0 < 3), or no image
    _refused(L, L.mit_maxpool2d_nhwc(P_IN, P_OUT, 2, 1, 8, 4, 3, 2, 0, None), "mit_maxpool2d_nhwc: empty output")
    _refused(L, L.mit_maxpool2d_nhwc(P_IN, P_OUT, 0, 8, 8, 4, 3, 2, 1, None), "mit_maxpool2d_nhwc: empty output")
    _refused(L, L.mit_avgpool_nhwc(P_IN, P_OUT, 2, 8, 1, 4, 2, 2, 2, 2, 0, 0, None), "mit_avgpool_nhwc: empty output")
    _refused(L, L.mit_avgpool_nhwc(P_IN, P_OUT, 0, 8, 8, 4, 2, 2, 2, 2, 0, 0, None), "mit_avgpool_nhwc: empty output")


def test_lama_prep_padded_refuses_paddings_reflection_cannot_serve(L):
    text = "mit_lama_prep_padded: bad padding"
    _refused(L, L.mit_lama_prep_padded(P_IN, P_A, P_OUT, 2, 4, 9, 4, 32, None), text)    # pad >= H
    _refused(L, L.mit_lama_prep_padded(P_IN, P_A, P_OUT, 2, 9, 4, 4, 32, None), text)    # pad >= W
    _refused(L, L.mit_lama_prep_padded(P_IN, P_A, P_OUT, 2, 8, 8, 3, 13, None), text)    # Wp < W + 2 pad
    _refused(L, L.mit_lama_prep_padded(P_IN, P_A, P_OUT, 2, 8, 8, -1, 16, None), text)
    _refused(L, L.mit_lama_prep_padded(P_IN, P_A, P_OUT, 0, 8, 8, 3, 14, None), "mit_lama_prep_padded: empty page")
