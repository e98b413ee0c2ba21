"""The automatic tile choice of mit_conv_gemm, seen through mit_conv_gemm_plan (no GPU: the plan makes no HIP call and dereferences no
operand pointer).  Every tile of a family gives identical bits by design, so no equality test can see WHICH tile a launch takes; this
one can.  tests/golden/conv_gemm_plan.json was recorded once, from the tile choice as it stood before it was rewritten around tile
traits (the plan entry added on the untouched code), and is never regenerated: a changed expectation is a changed behaviour."""
import ctypes as C
import json
import os

import pytest

from _conv_gemm_plan_cases import GPU_CASES, desc, plan, sweep, tile_names

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_gemm_plan.json")
# reference forms the tests name explicitly; the automatic choice never takes them
TEST_ONLY = {"split128x128x16p6", "split128x128x16p9", "split128x128x16p3", "split128x64x16p6"}


@pytest.fixture(scope="module")
def handle():
    from manga_image_translator_amd import lib

    h = lib.load(build_if_missing=True)
    mode, mt = h.mit_gemm_mode_get(), h.mit_gemm_split_min_tiles(-1)
    yield h
    h.mit_gemm_mode_set(mode)
    h.mit_gemm_split_min_tiles(mt)


def test_automatic_choice_matches_the_recorded_plan(handle):
    golden = json.load(open(GOLDEN))
    strings, cases = golden["strings"], golden["cases"]
    swept = list(sweep())
    assert len(swept) == len(cases), "every case has an expectation"
    seen, refused, cut = set(), 0, 0
    for i, (mode, mt, kw) in enumerate(swept):
        assert handle.mit_gemm_mode_set(mode) == 0
        handle.mit_gemm_split_min_tiles(mt)
        got = plan(handle, desc(**kw))
        assert got == strings[cases[i]], f"case {i}: mode {mode}, min_tiles {mt}, {kw}"
        if got.startswith("refused"):
            refused += 1
        else:
            name, nb_run = got.rsplit(":", 1)
            seen.add(name)
            cut += int(nb_run) < kw["NB"]
    assert seen == set(tile_names(handle)) - TEST_ONLY
    assert refused and cut, "refusals and cut batches are among the cases"


def test_device_test_launches_take_the_recorded_tiles(handle):
    golden = json.load(open(GOLDEN))["gpu_cases"]
    assert set(golden) == set(GPU_CASES)
    handle.mit_gemm_split_min_tiles(0)
    for name, (mode, kw) in GPU_CASES.items():
        handle.mit_gemm_mode_set(mode)
        assert plan(handle, desc(**kw)) == golden[name], name


def _refused():
    """(descriptor or None, cfg) of launches mit_conv_gemm_cfg refuses before any HIP call."""
    base = dict(NB=1, Ho=16, Wo=16, Cin=16, taps=1, N=64)
    out = [(None, -1), (desc(**base, a=0), -1)]
    for change in (dict(Cin=6), dict(taps=0), dict(taps=65), dict(N=0), dict(a=4100), dict(Z=70000), dict(nprod=2), dict(nprod=1),
                   dict(nprod=1, split=1, Cin=4), dict(nprod=1, split=1, taps=17)):
        out.append((desc(**{**base, **change}), -1))
    for d_kw, cfg_name in ((dict(nprod=1, split=1), "split128x128x16p6o"), (dict(N=8), "gemv16"), (dict(Cin=4), "fast128x128x16w4c"),
                           (dict(), "split128x128x16p6o"), (dict(split=1), "split64x64x32p1o"), (dict(), 99)):
        out.append((desc(**{**base, **d_kw}), cfg_name))
    d = desc(**{**base, "Cin": 4})  # the row-lookup epilogue on a launch that takes the generic kernel
    d.lut_rows, d.lut1, d.lut2, d.lut_ld = 4096, 4096, 4096, 64
    out.append((d, -1))
    return out


def test_plan_and_launch_refuse_alike(handle):
    names = tile_names(handle)
    handle.mit_gemm_mode_set(6)
    handle.mit_gemm_split_min_tiles(0)
    tile, nb = C.c_int32(), C.c_int32()
    for d, cfg in _refused():
        cfg = names.index(cfg) if isinstance(cfg, str) else cfg
        ref = C.byref(d) if d is not None else None
        rc_plan = handle.mit_conv_gemm_plan(ref, cfg, C.byref(tile), C.byref(nb))
        msg_plan = handle.mit_last_error()
        assert rc_plan != 0 and msg_plan, (cfg, msg_plan)  # (only then is the launch below refused before any HIP call)
        assert handle.mit_conv_gemm_cfg(ref, cfg, None) == rc_plan and handle.mit_last_error() == msg_plan, (cfg, msg_plan)
