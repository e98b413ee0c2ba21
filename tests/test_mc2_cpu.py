"""The mc2 colorizer without a GPU: the oracle (tests/_mc2_oracle.py) against the reference modules and fixtures, the state-dict
schemas, the checkpoint loader, registration, the INTER_AREA host twin and the seeded weights."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _mc2_oracle as O  # noqa: E402
from manga_image_translator_amd import imgproc, mc2_schema as S  # noqa: E402
from oracle import lama as OL, ref_import as R  # noqa: E402

needs_ref = pytest.mark.skipif(not R.available(), reason="the reference tree is not on this machine")


@pytest.fixture(scope="module")
def sd():
    return O.weights()


@needs_ref
def test_schemas_match_the_reference_modules():
    M = O.ref_modules()
    for mod, sch in ((M["models"].Generator(), S.generator_schema()), (M["dmodels"].FFDNet(3), S.ffdnet_schema())):
        ref = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
        assert ref == {n: tuple(s) for n, s, _ in sch}


def test_schema_names_the_unused_parts_and_the_reference_spelling():
    names = {n for n, _, _ in S.generator_schema()}
    assert {"tunnel1.2.4.conv_conv.weight", "deconv_for_decoder.6.bias", "to4.2.weight", "encoder.bn1.num_batches_tracked"} <= names
    assert "intermediate_dncnn.itermediate_dncnn.32.weight" in {n for n, _, _ in S.ffdnet_schema()}


@needs_ref
def test_oracle_matches_the_reference_modules(sd):
    gsd, fsd = sd
    M = O.ref_modules()
    g, f = O.ref_generator(gsd, M), O.ref_ffdnet(fsd, M)
    x = torch.rand(1, 1, 96, 64, generator=torch.Generator().manual_seed(0))
    xx = torch.cat([x, torch.zeros(1, 4, 96, 64)], 1)
    with torch.no_grad():
        y, _ = g(xx)
        xin = torch.rand(2, 3, 64, 48, generator=torch.Generator().manual_seed(1))
        n = f(xin, torch.FloatTensor([30 / 255, 30 / 255]))
    assert float((y - O.generator(gsd, xx)).abs().max()) <= 1e-5
    assert float((n - O.ffdnet(fsd, xin, float(np.float32(30 / 255)))).abs().max()) <= 1e-5


@needs_ref
def test_fixtures_regenerate(sd):
    gsd, fsd = sd
    z = np.load(os.path.join(O.GOLDEN, "mc2.npz"))
    for k, v in O.net_fixture(gsd, fsd).items():
        assert np.array_equal(z[k], v), k
    zi = np.load(os.path.join(O.GOLDEN, "mc2_infer.npz"))
    for k, v in O.infer_fixture(gsd, fsd).items():
        assert np.array_equal(zi[k], v), k


def test_oracle_against_the_fixtures(sd):
    gsd, fsd = sd
    z = np.load(os.path.join(O.GOLDEN, "mc2.npz"))
    for tag, H, W, _ in O.NET_CASES:
        sk = torch.from_numpy(z[f"sketch_{tag}"])
        y = O.generator(gsd, torch.cat([sk, torch.zeros(1, 4, H, W)], 1))
        assert float((y - torch.from_numpy(z[f"gen_{tag}"])).abs().max()) <= 1e-5
        n = O.ffdnet(fsd, torch.from_numpy(z[f"ffd_in_{tag}"]), float(np.float32(30 / 255)))
        assert float((n - torch.from_numpy(z[f"ffd_{tag}"])).abs().max()) <= 1e-5
    zi = np.load(os.path.join(O.GOLDEN, "mc2_infer.npz"))
    for tag, *_ in O.INFER_CASES:
        o = O.infer(gsd, fsd, zi[f"page_{tag}"], int(zi[f"size_{tag}"]), float(zi[f"sigma_{tag}"]))
        assert o["out"].shape == zi[f"out_{tag}"].shape
        assert np.array_equal(o["out"], zi[f"out_{tag}"]), tag


def test_checkpoint_loader_with_and_without_the_dataparallel_prefix(tmp_path, sd):
    from manga_image_translator_amd import plugins as P

    gsd, fsd = sd

    class Stub:
        def _get_file_path(self, name):
            return str(tmp_path / name)

    torch.save(gsd, tmp_path / "generator.zip")
    for d in (fsd, {"module." + k: v for k, v in fsd.items()}):
        torch.save(d, tmp_path / "net_rgb.pth")
        got = P._load_mc2_checkpoint(Stub())
        assert set(got["denoiser"]) == set(fsd) and all(torch.equal(got["denoiser"][k], fsd[k]) for k in fsd)
        assert set(got["generator"]) == set(gsd)
    bad = dict(fsd)
    del bad["intermediate_dncnn.itermediate_dncnn.0.weight"]
    torch.save(bad, tmp_path / "net_rgb.pth")
    with pytest.raises(ValueError, match="1 missing tensors"):
        P._load_mc2_checkpoint(Stub())


_REGISTER = r"""
import os, sys, tempfile
sys.path.insert(0, {root!r})
sys.dont_write_bytecode = True
from oracle import ref_boundary as RB
RB.install(model_dir=tempfile.mkdtemp(prefix="mit_models_"))
import manga_translator.colorization as RC
from manga_translator.colorization.manga_colorization_v2 import MangaColorizationV2
from manga_translator.colorization.common import OfflineColorizer
from manga_image_translator_amd import plugins as P
P.register()
assert RC.COLORIZERS["mc2_hip"] is P.HipMangaColorizer
assert issubclass(P.HipMangaColorizer, OfflineColorizer)
assert P.HipMangaColorizer._MODEL_MAPPING == MangaColorizationV2._MODEL_MAPPING
assert P.HipMangaColorizer._MODEL_SUB_DIR == MangaColorizationV2._MODEL_SUB_DIR
inst = RC.get_colorizer("mc2_hip")
assert isinstance(inst, P.HipMangaColorizer) and RC.get_colorizer("mc2_hip") is inst
print("MC2 REGISTERED")
"""


@needs_ref
def test_register_adds_the_colorizer(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", _REGISTER.format(root=ROOT)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path),
                         env=env)
    assert out.returncode == 0 and "MC2 REGISTERED" in out.stdout, out.stdout[-3000:] + "\n" + out.stderr[-3000:]


def test_standalone_plugin_mirrors_the_model_layout():
    from manga_image_translator_amd import plugins as P

    assert P.HipMangaColorizer._MODEL_SUB_DIR == os.path.join("colorization", "manga-colorization-v2")
    assert {m["file"] for m in P.HipMangaColorizer._MODEL_MAPPING.values()} == {"generator.zip", "net_rgb.pth"}


_SIZES = [((2048, 1456), (853, 1200)), ((1200, 853), (811, 576)), ((150, 230), (345, 225)), ((37, 53), (20, 17)), ((64, 48), (64, 48)),
          ((811, 576), (811, 576)), ((33, 31), (64, 29))]


@pytest.mark.parametrize("src,dst", _SIZES + [((int(a), int(b)), (int(c), int(d))) for a, b, c, d in
                                              np.random.default_rng(7).integers(8, 200, size=(8, 4))])
def test_area_host_twin_equals_the_oracle(src, dst):
    rng = np.random.default_rng(src[0] * 1000 + dst[1])
    img = rng.integers(0, 256, size=src + (3,), dtype=np.uint8)
    got = imgproc.resize_u8_host(img, (dst[1], dst[0]), area=True)
    ref = np.stack([OL.resize_area_u8(np.ascontiguousarray(img[..., c]), (dst[1], dst[0])) for c in range(3)], -1)
    assert got.shape == ref.shape
    # the twin rounds N / (H W) half up exactly; the float64 restatement may land just below an exact .5: only there may they differ
    ties = _exact_ties(img, dst)
    assert np.array_equal(got[~ties], ref[~ties])
    assert np.array_equal(got[ties].astype(int) - ref[ties].astype(int) >= 0, np.ones(int(ties.sum()), bool))
    assert (got[ties].astype(int) - ref[ties].astype(int)).max(initial=0) <= 1


def _exact_ties(img, dst):
    sh, sw = img.shape[:2]
    dh, dw = dst
    area = dh <= sh and dw <= sw
    yi, yc = imgproc.area_taps(sh, dh, area)
    xi, xc = imgproc.area_taps(sw, dw, area)
    t = img.astype(np.int64)
    rows = sum(t[:, np.minimum(xi + k, sw - 1)] * xc[None, :, k, None].astype(np.int64) for k in range(xc.shape[1]))
    N = sum(rows[np.minimum(yi + k, sh - 1)] * yc[:, k, None, None].astype(np.int64) for k in range(yc.shape[1]))
    return (2 * N + sh * sw) % (2 * sh * sw) == 0


def test_seeded_weights_do_not_saturate(sd):
    gsd, fsd = sd
    page = O.synth_color_page(3, 420, 300)
    u = O.infer(gsd, fsd, page, 256, 30)["out"]
    assert ((u >= 16) & (u <= 239)).mean() >= 0.5
    assert ((u[..., 0] != u[..., 1]) | (u[..., 1] != u[..., 2])).mean() >= 0.1


def test_plan_follows_infer():
    from manga_image_translator_amd.mc2 import Mc2Engine

    assert Mc2Engine.plan(2048, 1456, 576, 30) == (576, (1200, 853), (811, 576))
    assert Mc2Engine.plan(150, 230, 128, 30) == (128, (150, 230), (192, 295))
    assert Mc2Engine.plan(260, 200, 576, -1) == (192, None, (250, 192))
