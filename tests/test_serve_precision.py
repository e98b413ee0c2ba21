"""A batch served by ``DenseStages.translate_batch`` runs the inpainter in what the page loop's ``self.inp.infer(page, mask, None, ...)``
runs in: the plugin's ``precision`` option reaches ``CoupledPageEngine.run`` as its ``precision`` keyword (MIT_SERVE_ENGINE stub:
tests/_serve_batch_stub.py records the keywords).  No GPU."""
import asyncio

import numpy as np
import pytest

from manga_image_translator_amd import plugins as P, serve


@pytest.fixture
def stages(monkeypatch):
    monkeypatch.setenv("MIT_SERVE_ENGINE", "tests._serve_batch_stub:make")
    monkeypatch.delenv("MIT_LAMA_PRECISION", raising=False)
    return serve._make_engine({})


def _batch(stages):
    pages = [np.full((32, 32, 3), v, np.uint8) for v in (1, 2)]
    asyncio.run(stages.translate_batch(pages, {}, batch_size=2))
    return stages.fake.calls[-1][1]


@pytest.mark.parametrize("setting,want", [("bf16", "bf16"), ("fp32", "fp32"), ("config", "fp32")])
def test_served_batch_follows_the_plugin_precision(stages, setting, want):
    # "config": serve.py hands the plugins no config (page loop and batch alike), so it resolves to fp32 there
    stages.inp = P.HipLamaMPEInpainter(weights={}, precision=setting)
    assert _batch(stages)["precision"] == want


def test_served_batch_follows_the_environment_default(stages, monkeypatch):
    monkeypatch.setenv("MIT_LAMA_PRECISION", "bf16")
    stages.inp = P.HipLamaMPEInpainter(weights={})
    assert _batch(stages)["precision"] == "bf16"


def test_served_batch_without_the_option_is_fp32(stages):
    assert _batch(stages)["precision"] == "fp32"        # an inpainter without precision_for (the stub has none)
    stages.inp = P.HipAotInpainter(weights={}, precision="bf16")
    assert _batch(stages)["precision"] == "fp32"        # the AOT engine stays fp32
