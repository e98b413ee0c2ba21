"""The cases of tests/golden/det_filters.npz and the stand-in network, shared by the det_filters tests: scripts/make_det_filters_golden.py
loaded by path (the script that wrote the fixture defines the seeded pages, the quads and the stub, so the tests cannot drift from it)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_make_det_filters_golden", os.path.join(ROOT, "scripts", "make_det_filters_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLDEN = os.path.join(ROOT, "tests", "golden", "det_filters.npz")


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
