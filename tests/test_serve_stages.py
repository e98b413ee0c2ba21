"""Which stages a serving worker runs for a request (serve.stage_keys, ``DenseStages(params={"stages": ...})``), without a GPU: the key
mapping and its refusals, the fixed mode, the batch planning of the config mode on the stub stages (tests/_serve_batch_stub.py), and
the argument checks of ``mit_dbnet_mask_tail`` that come before any HIP call."""
import asyncio
import types

import numpy as np
import pytest

from manga_image_translator_amd import serve


def test_stage_keys_defaults_are_the_reference_s():
    assert serve.stage_keys({}) == serve.stage_keys(None) == ("default", "48px", "lama_large")
    # a reference-default Config as a front server posts it (config.py:272-344), sections as dicts or as objects with enum members
    ref = {"detector": {"detector": "default", "detection_size": 2048, "text_threshold": 0.5, "det_rotate": False, "det_auto_rotate": False,
                        "det_invert": False, "det_gamma_correct": False, "box_threshold": 0.7, "unclip_ratio": 2.3},
           "inpainter": {"inpainter": "lama_large", "inpainting_size": 2048, "inpainting_precision": "bf16"},
           "ocr": {"use_mocr_merge": False, "ocr": "48px", "min_text_length": 0, "ignore_bubble": 0, "prob": None}, "kernel_size": 3,
           "mask_dilation_offset": 20}
    assert serve.stage_keys(ref) == ("default", "48px", "lama_large")
    enum = lambda v: types.SimpleNamespace(value=v)   # noqa: E731
    obj = types.SimpleNamespace(detector=types.SimpleNamespace(detector=enum("ctd"), det_rotate=False),
                                ocr=types.SimpleNamespace(ocr=enum("32px")), inpainter=types.SimpleNamespace(inpainter=enum("default")))
    assert serve.stage_keys(obj) == ("ctd", "32px", "default")
    assert serve.stage_keys({"detector": {}, "ocr": None}) == ("default", "48px", "lama_large")


@pytest.mark.parametrize("section, name, keys", [("detector", "detector", ("default", "dbconvnext", "ctd")), ("ocr", "ocr", ("48px", "48px_ctc", "32px")),
                                                 ("inpainter", "inpainter", ("lama_large", "lama_mpe", "default"))])
def test_stage_keys_maps_every_supported_key(section, name, keys):
    pos = ("detector", "ocr", "inpainter").index(section)
    for k in keys:
        got = serve.stage_keys({section: {name: k}})
        assert got[pos] == k and [g for i, g in enumerate(got) if i != pos] == [d for i, d in enumerate(("default", "48px", "lama_large")) if i != pos]


@pytest.mark.parametrize("section, name, key", [("detector", "detector", "craft"), ("detector", "detector", "paddle"), ("detector", "detector", "none"),
                                                ("ocr", "ocr", "mocr"), ("inpainter", "inpainter", "sd"), ("inpainter", "inpainter", "original"),
                                                ("inpainter", "inpainter", "none")])
def test_stage_keys_refuses_what_it_has_no_plugin_for(section, name, key):
    with pytest.raises(ValueError) as e:
        serve.stage_keys({section: {name: key}})
    msg = str(e.value)
    assert f"{section}.{name}" in msg and repr(key) in msg
    assert all(k in msg for k in serve.SUPPORTED_STAGE_KEYS[(section, name)])      # the supported set is named


@pytest.mark.parametrize("opt", ["det_rotate", "det_auto_rotate", "det_invert", "det_gamma_correct"])
def test_stage_keys_refuses_a_detector_filter_option_that_is_set(opt):
    assert serve.stage_keys({"detector": {opt: False}})[0] == "default"
    with pytest.raises(ValueError, match=f"detector.{opt} is set"):
        serve.stage_keys({"detector": {"detector": "ctd", opt: True}})


def test_bad_mode_is_refused(monkeypatch):
    with pytest.raises(ValueError, match="stages must be one of"):
        serve.DenseStages({"stages": "auto"})
    monkeypatch.setenv("MIT_SERVE_STAGES", "config")
    assert serve.DenseStages().stages == "config" and serve.DenseStages({"stages": "fixed"}).stages == "fixed"
    monkeypatch.delenv("MIT_SERVE_STAGES")
    assert serve.DenseStages().stages == "fixed"


def _stub(monkeypatch, params):
    monkeypatch.setenv("MIT_SERVE_ENGINE", "tests._serve_batch_stub:make")
    return serve._make_engine(params)


def _page(h, w, v):
    return np.full((h, w, 3), v, np.uint8)


def test_fixed_mode_serves_its_three_stages_whatever_the_config_says(monkeypatch):
    st = _stub(monkeypatch, {})
    assert st.stages == "fixed"
    cfg = {"detector": {"detector": "craft", "det_rotate": True}, "ocr": {"ocr": "32px"}, "inpainter": {"inpainter": "sd"}}
    assert st._select(cfg) == ("ctd", "48px", "lama_mpe")
    asyncio.run(st.translate_batch([_page(32, 32, 1), _page(32, 32, 2)], cfg, batch_size=2))
    assert st.last_stage_keys == ("ctd", "48px", "lama_mpe") and st.last_batch_plan == [([0, 1], "")]
    (_, kw), = st.fake.calls
    assert "detect_size" not in kw              # the run of the fixed mode is called as it always was


def test_config_mode_plans_by_the_stages_the_request_names(monkeypatch):
    st = _stub(monkeypatch, {"stages": "config"})
    pages = [_page(32, 32, 1), _page(32, 32, 2), _page(32, 32, 3)]
    # the 32px and ctc OCRs are not in the coupled engine: the page loop, with the reason
    for key in ("32px", "48px_ctc"):
        asyncio.run(st.translate_batch(pages, {"ocr": {"ocr": key}}, batch_size=4))
        assert st.last_stage_keys == ("default", key, "lama_large")
        assert st.last_batch_plan == [([i], f"ocr.ocr = {key} is not in the coupled engine") for i in range(3)]
    assert not st.fake.calls and st.pages_looped == 6
    # default + lama_large on equal pages: one coupled run, and the detector's parameters reach it
    cfg = {"detector": {"detector": "default", "detection_size": 1536, "text_threshold": 0.4, "unclip_ratio": 2.0}, "inpainter": {"inpainter": "lama_large"}}
    asyncio.run(st.translate_batch(pages, cfg, batch_size=4))
    assert st.last_stage_keys == ("default", "48px", "lama_large") and st.last_batch_plan == [([0, 1, 2], "")] and st.pages_batched == 3
    (shape, kw), = st.fake.calls
    assert shape == (3, 32, 32, 3)
    assert (kw["detect_size"], kw["text_threshold"], kw["box_threshold"], kw["unclip_ratio"]) == (1536, 0.4, 0.7, 2.0)
    assert kw["inpainting_size"] == 2048
    # absent fields: the reference's defaults
    asyncio.run(st.translate_batch(pages, None, batch_size=4))
    kw = st.fake.calls[-1][1]
    assert (kw["detect_size"], kw["text_threshold"], kw["box_threshold"], kw["unclip_ratio"]) == (2048, 0.5, 0.7, 2.3)
    # a request the worker cannot honour is an error, not another model
    with pytest.raises(ValueError, match="detector.detector = 'craft'"):
        asyncio.run(st.translate_batch(pages, {"detector": {"detector": "craft"}}, batch_size=4))


def test_config_mode_sends_dbnet_strips_through_the_loop(monkeypatch):
    """A strip is one at the size its detector tiles at; the stub's coupled engine has no ``takes_strips``, like a coupled engine over a
    DBNet detector."""
    st = _stub(monkeypatch, {"stages": "config"})
    strip = _page(4000, 300, 7)
    asyncio.run(st.translate_batch([strip, strip.copy()], {"detector": {"detection_size": 1024}}, batch_size=2))
    assert all("DBNet strips are not batched" in why for _, why in st.last_batch_plan) and st.pages_looped == 2
    asyncio.run(st.translate_batch([strip, strip.copy()], {"detector": {"detector": "ctd"}}, batch_size=2))
    assert [why for _, why in st.last_batch_plan] == ["webtoon strip (rearranged detection)"] * 2


def test_the_coupled_engine_over_a_dbnet_detector_declares_no_strips():
    from manga_image_translator_amd import coupled

    assert coupled.is_dbnet_engine(object()) is False
    assert coupled.CoupledPageEngine.takes_strips is True       # the class (ctd) keeps its attribute; from_engines clears it per instance


def test_mask_tail_refuses_bad_arguments_before_any_hip_call():
    from manga_image_translator_amd import lib

    L = lib.load()
    fake = 4096      # never dereferenced: every call below is refused by the argument checks
    assert L.mit_dbnet_mask_tail(None, 0, 8, 1, 4, 8, fake, 8, 16, None) != 0 and b"null pointer" in L.mit_last_error()
    assert L.mit_dbnet_mask_tail(fake, 0, 8, 1, 4, 8, None, 8, 16, None) != 0 and b"null pointer" in L.mit_last_error()
    assert L.mit_dbnet_mask_tail(fake, 32, 8, 1, 4, 8, fake, 9, 16, None) != 0 and b"inside the 2x map" in L.mit_last_error()
    assert L.mit_dbnet_mask_tail(fake, 32, 8, 1, 4, 8, fake, 8, 17, None) != 0 and b"inside the 2x map" in L.mit_last_error()
    for bad in ((0, 4, 8, 8, 16), (1, 0, 8, 8, 16), (1, 4, -1, 8, 16), (1, 4, 8, 0, 16), (1, 4, 8, 8, 0)):
        B, h, w, oh, ow = bad
        assert L.mit_dbnet_mask_tail(fake, 32, 8, B, h, w, fake, oh, ow, None) != 0 and b"must be positive" in L.mit_last_error(), bad
    assert L.mit_dbnet_mask_tail(fake, 32, 7, 1, 4, 8, fake, 8, 16, None) != 0 and b"strides" in L.mit_last_error()
