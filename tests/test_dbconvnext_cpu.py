"""The dbconvnext detector (DBNet on ConvNeXt) without a GPU: the restated oracle against the committed fixture of the reference
module, the fixture's own conditions, the schema, the plugin's place in the reference's registry and the engine's shape check.
Checks that need the reference tree skip where it is absent."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _dbconvnext_oracle as O  # noqa: E402
from manga_image_translator_amd import dbconvnext, dbconvnext_schema  # noqa: E402

HAVE_REF = os.path.isdir("/root/reference/manga_translator")
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="the reference checkout is only present in the build container")


@pytest.fixture(scope="module")
def sd():
    return O.weights()


@pytest.fixture(scope="module")
def golden():
    return np.load(O.FIXTURE)


@pytest.mark.parametrize("tag", [t for t, *_ in O.CASES])
def test_oracle_reproduces_the_fixture(sd, golden, tag):
    """The restated forward against the reference module's recorded outputs: 1e-5 on the post-sigmoid maps (the order of the other
    restated oracles), 1e-4 of each tap's range on the taps."""
    assert int(golden["seed"]) == O.SEED and float(golden["gain"]) == O.GAIN
    pg = golden[f"page_{tag}"]
    assert np.array_equal(pg, O.page(tag))
    taps = {}
    db, mask = O.det_batch_forward(sd, pg[None], taps)
    e_db, e_mask = np.abs(db[:, :, ::2, ::2] - golden[f"db_{tag}"]).max(), np.abs(mask - golden[f"mask_{tag}"]).max()
    print(f"oracle vs fixture [{tag}]: db {e_db:.3g} mask {e_mask:.3g}")
    assert e_db <= 1e-5 and e_mask <= 1e-5, (e_db, e_mask)
    for k in O.TAPS:
        ref = golden[f"{k}_{tag}"]
        e = np.abs(O.sub_tap(k, taps[k]) - ref).max() / (ref.max() - ref.min())
        assert e <= 1e-4, (k, e)


def test_fixture_meets_its_conditions(golden):
    """The seeded weights exercise the network (no dead or exploding trunk), float32 is far inside the 2e-4 parity bar, and few pixels sit
    within that bar of the 0.5 threshold — measured when the fixture was written, recorded in it."""
    O.check_conditions(golden)


@needs_ref
def test_fixture_regenerates(sd, golden):
    new = O.fixture(sd, stats=False)
    for k, v in new.items():
        v = np.asarray(v)
        if v.dtype.kind == "f" and v.ndim:
            np.testing.assert_allclose(golden[k], v, rtol=0, atol=1e-6, err_msg=k)
        else:
            assert np.array_equal(golden[k], v), k


def test_schema_equals_the_fixture_names_and_shapes(golden):
    ref = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(golden["names"], golden["shapes"])}
    ours = {n: tuple(s) for n, s, _ in dbconvnext_schema.dbnet_convnext_schema()}
    assert ours == ref
    assert [n for n, _, _ in dbconvnext_schema.dbnet_convnext_schema()] == [str(n) for n in golden["names"]]   # state_dict order
    assert abs(sum(int(np.prod(s)) for s in ours.values()) / 1e6 - 159.63) < 0.01


def test_engine_rejects_bad_pages_before_any_launch():
    eng = dbconvnext.DbconvnextEngine.__new__(dbconvnext.DbconvnextEngine)
    with pytest.raises(ValueError, match="multiples of 128"):
        eng.forward(torch.zeros(1, 200, 256, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="multiples of 128"):
        eng.forward(torch.zeros(1, 256, 192, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="u8"):
        eng.forward(torch.zeros(1, 256, 256, 3))
    dbconvnext.check_page_batch(torch.zeros(2, 128, 384, 3, dtype=torch.uint8))


_REGISTER = r"""
import os, sys, tempfile
sys.path.insert(0, {root!r})
sys.dont_write_bytecode = True
from oracle import ref_boundary as RB
RB.install(model_dir=tempfile.mkdtemp(prefix="mit_models_"))
import manga_translator.detection as RD
from manga_translator.detection.common import OfflineDetector
from manga_translator.detection.dbnet_convnext import DBConvNextDetector
from manga_translator.detection.default import DefaultDetector
from manga_image_translator_amd import plugins as P
P.register()
assert RD.DETECTORS["dbconvnext_hip"] is P.HipDBConvNextDetector
assert issubclass(P.HipDBConvNextDetector, OfflineDetector) and issubclass(P.HipDBConvNextDetector, P.HipDefaultDetector)
assert P.HipDBConvNextDetector._MODEL_MAPPING == DBConvNextDetector._MODEL_MAPPING
assert P.HipDBConvNextDetector._infer is P.HipDefaultDetector._infer
import inspect
strip = lambda f: inspect.getsource(f).split("verbose: bool = False):", 1)[1]
assert strip(DBConvNextDetector._infer).split("# if verbose")[0].split() == strip(DefaultDetector._infer).split("# if verbose")[0].split()
inst = RD.get_detector("dbconvnext_hip")
assert isinstance(inst, P.HipDBConvNextDetector) and RD.get_detector("dbconvnext_hip") is inst and not inst.is_loaded()
print("DBCONVNEXT REGISTERED")
"""


@needs_ref
def test_register_adds_the_dbconvnext_detector(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", _REGISTER.format(root=ROOT)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path),
                         env=env)
    assert out.returncode == 0 and "DBCONVNEXT REGISTERED" in out.stdout, out.stdout[-3000:] + "\n" + out.stderr[-3000:]
