"""``DenseStages`` with the GPU taken out (MIT_SERVE_ENGINE=tests._serve_batch_stub:make): ``translate`` and the coupled engine are
recording stand-ins, so the batch planning of ``translate_batch`` — grouping, order, the ``per_page`` overlay, the counters — runs
as it is, on the CPU."""
import types

import numpy as np
import torch

from manga_image_translator_amd import serve


class FakeCoupled:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def run(self, pages, **kw):
        self.calls.append((tuple(pages.shape), kw))
        B, H, W, _ = pages.shape
        raw = torch.zeros(B, H, W, dtype=torch.uint8)
        for k, m in enumerate(kw["mask_raw"]):
            if m is not None:
                raw[k] = torch.from_numpy(np.asarray(m, dtype=np.uint8))
        return types.SimpleNamespace(textlines=[[] for _ in range(B)], mask_raw=raw, mask=raw.clone(), inpainted=pages + 1, seconds={"ocr": 0.0})


class StubStages(serve.DenseStages):
    def __init__(self, params=None):
        super().__init__(params)
        self.fake = FakeCoupled()
        self.loop_calls = []
        self.device_name = "stub"

    async def _load(self):
        self._loaded = True

    def _coupled_engine(self):
        return self.fake

    async def translate(self, image, config=None):
        page = np.asarray(image)
        self.loop_calls.append((page.shape, config))
        return {"textlines": [], "mask_raw": np.zeros(page.shape[:2], np.uint8), "mask": np.zeros(page.shape[:2], np.uint8),
                "inpainted": page + 2, "device": "stub", "visible_devices": None}


def make(params):
    return StubStages(params)
