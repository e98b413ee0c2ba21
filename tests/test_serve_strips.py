"""Webtoon strips in ``DenseStages.translate_batch`` without a GPU: strips of equal size form one coupled run when the coupled engine
says it has the rearranged detection (``takes_strips``), and keep taking the page loop when it does not (the stand-ins of
tests/_serve_batch_stub.py, whose fake engine has no such attribute)."""
import asyncio

import numpy as np

from manga_image_translator_amd import rearrange, serve
from tests._serve_batch_stub import FakeCoupled, StubStages

STRIP = (2600, 160)


class StripCoupled(FakeCoupled):
    takes_strips = True


class CountingStages(StubStages):
    """Counts how often the planning asks for the coupled engine."""

    def __init__(self, fake):
        super().__init__({})
        self.fake, self.asked = fake, 0

    def _coupled_engine(self):
        self.asked += 1
        return self.fake


def _pages():
    assert rearrange.plan(*STRIP, 1024) is not None and rearrange.plan(64, 48, 1024) is None
    return [np.full(STRIP + (3,), 10, np.uint8), np.full(STRIP + (3,), 20, np.uint8), np.full((64, 48, 3), 30, np.uint8),
            np.full((64, 48, 3), 40, np.uint8)]


def test_equal_strips_are_one_coupled_run_when_the_engine_takes_strips():
    st = CountingStages(StripCoupled())
    out = asyncio.run(st.translate_batch(_pages(), {}, batch_size=4))
    assert st.last_batch_plan == [([0, 1], ""), ([2, 3], "")]
    assert [c[0] for c in st.fake.calls] == [(2,) + STRIP + (3,), (2, 64, 48, 3)] and not st.loop_calls
    assert [int(r["inpainted"][0, 0, 0]) for r in out] == [11, 21, 31, 41]      # the coupled stand-in adds 1
    assert st.pages_batched == 4 and st.pages_looped == 0
    assert st._loop_reason(_pages()[0], {}) is None
    # a strip is still held back by what holds any page back
    assert st._loop_reason(_pages()[0], {"ocr": {"ignore_bubble": 5}}) == "ocr.ignore_bubble is not implemented by the coupled engine"


def test_the_engine_is_asked_only_for_strips():
    st = CountingStages(StripCoupled())
    assert st._loop_reason(_pages()[2], {}) is None and st.asked == 0
    assert st._loop_reason(_pages()[0], {}) is None and st.asked == 1


def test_strips_take_the_loop_without_the_attribute():
    st = CountingStages(FakeCoupled())
    out = asyncio.run(st.translate_batch(_pages(), {}, batch_size=4))
    why = "webtoon strip (rearranged detection)"
    assert st.last_batch_plan == [([0], why), ([1], why), ([2, 3], "")]
    assert [c[0] for c in st.fake.calls] == [(2, 64, 48, 3)] and [c[0] for c in st.loop_calls] == [STRIP + (3,)] * 2
    assert [int(r["inpainted"][0, 0, 0]) for r in out] == [12, 22, 31, 41]      # the loop stand-in adds 2
    assert st.pages_batched == 2 and st.pages_looped == 2


def test_the_coupled_engine_declares_it():
    from manga_image_translator_amd import coupled

    assert coupled.CoupledPageEngine.takes_strips is True
