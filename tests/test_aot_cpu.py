"""The AOT inpainter (the reference's ``Inpainter.default``) without a GPU: the restated oracle against the reference module and
its committed fixtures, the weight-standardisation fold, the schema, the checkpoint loader, the seeded weights' range, the
registration and the dilated ``ops.Conv2d`` descriptors.  Checks that need the reference tree skip where it is absent."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _aot_oracle as O  # noqa: E402
from manga_image_translator_amd import aot, aot_schema, ops, synth  # noqa: E402

HAVE_REF = os.path.isdir("/root/reference/manga_translator")
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="the reference checkout is only present in the build container")


def _rel(a, b):
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


@pytest.fixture(scope="module")
def sd():
    return O.weights()


@needs_ref
@pytest.mark.parametrize("H,W", [(96, 128), (72, 80)])
def test_oracle_matches_the_reference_generator(sd, H, W):
    m = O.ref_generator(sd)
    page, _, mask = synth.synth_page(21, H, W, n_boxes=3)
    img, mk = O.prep(page, mask)
    with torch.no_grad():
        ref = m(img, mk)
        ref_head = m.head(torch.cat([mk, img], 1))
    taps = {}
    got = O.generator(sd, img, mk, taps)
    assert _rel(got, ref) < 1e-5
    assert _rel(taps["head"], ref_head) < 1e-5


@needs_ref
def test_reference_rejects_a_quarter_side_of_16_and_accepts_72():
    m = O.ref_generator(O.weights())
    with torch.no_grad():
        m(torch.zeros(1, 3, 72, 80), torch.zeros(1, 1, 72, 80))
        with pytest.raises(RuntimeError):
            m(torch.zeros(1, 3, 64, 80), torch.zeros(1, 1, 64, 80))


@needs_ref
def test_fixtures_regenerate(sd):
    z = np.load(os.path.join(O.GOLDEN, "aot.npz"))
    new = O.gen_fixture(sd)
    for k, v in new.items():
        if v.dtype == np.uint8:
            assert np.array_equal(z[k], v), k
        else:
            np.testing.assert_allclose(z[k], v, rtol=0, atol=1e-6, err_msg=k)
    z = np.load(os.path.join(O.GOLDEN, "aot_resize.npz"))
    for k, v in O.resize_fixture(sd).items():
        assert np.array_equal(z[k], np.asarray(v)), k


@pytest.mark.parametrize("tag", [t for t, *_ in O.GEN_CASES])
def test_oracle_reproduces_the_fixture(sd, tag):
    z = np.load(os.path.join(O.GOLDEN, "aot.npz"))
    img, mk = O.prep(z[f"page_{tag}"], z[f"mask_{tag}"])
    got = O.generator(sd, img, mk)
    assert _rel(got, torch.from_numpy(z[f"out_{tag}"])) < 1e-5


@needs_ref
def test_folded_ws_weights_are_bit_equal_to_get_weight(sd):
    m = O.ref_generator(sd)
    for layer, p in ((m.head[2].conv_gate, "head.2.conv_gate"), (m.tail[4].conv, "tail.4.conv"), (m.tail[8].conv, "tail.8.conv")):
        with torch.no_grad():
            ref = layer.get_weight()
        got = aot.fold_ws(sd[p + ".weight"], sd[p + ".gain"])
        assert got.dtype == torch.float32 and torch.equal(got, ref), p


def test_fold_matches_the_oracle_statement(sd):
    for p in ("head.0.conv", "tail.6.conv_gate"):
        a, b = aot.fold_ws(sd[p + ".weight"], sd[p + ".gain"]), O.ws(sd[p + ".weight"], sd[p + ".gain"])
        assert _rel(a, b) < 1e-6, p


@needs_ref
def test_schema_equals_the_reference_state_dict():
    ref = {k: tuple(v.shape) for k, v in O.ref_module().AOTGenerator().state_dict().items()}
    ours = {n: tuple(s) for n, s, _ in aot_schema.aot_generator_schema()}
    assert ours == ref
    assert len(ours) == 168 and sum(int(np.prod(s)) for s in ours.values()) == sum(int(np.prod(s)) for s in ref.values())


def test_schema_counts():
    s = aot_schema.aot_generator_schema()
    assert len(s) == 168 and len({n for n, _, _ in s}) == 168
    assert abs(sum(int(np.prod(shape)) for _, shape, _ in s) / 1e6 - 5.68) < 0.01


def test_checkpoint_loader_accepts_both_layouts_and_rejects_a_wrong_one(tmp_path, sd):
    from manga_image_translator_amd import plugins as P

    class Stub:
        CKPT = "inpainting.ckpt"

        def _get_file_path(self, name):
            return str(tmp_path / name)

    for obj in ({"model": sd}, sd):
        torch.save(obj, tmp_path / "inpainting.ckpt")
        got = P._load_aot_checkpoint(Stub())["aot"]
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    bad = dict(sd)
    bad["body_conv.3.fuse.1.weight"] = torch.zeros(128, 64, 3, 3)
    del bad["tail.8.conv.gain"]
    torch.save({"model": bad}, tmp_path / "inpainting.ckpt")
    with pytest.raises(ValueError, match="1 missing tensors.*1 with another shape"):
        P._load_aot_checkpoint(Stub())


def test_seeded_weights_exercise_the_network(sd):
    page, _, mask = synth.synth_page(0, 256, 184, n_boxes=6)
    img, mk = O.prep(page, mask)
    taps = {}
    O.generator(sd, img, mk, taps)
    pre = taps["preclip"]
    clip = float((pre.abs() > 1).float().mean())
    assert 0.2 <= float(pre.std()) <= 1.0, float(pre.std())
    assert 0.005 <= clip <= 0.15, clip


_REGISTER = r"""
import os, sys, tempfile
sys.path.insert(0, {root!r})
sys.dont_write_bytecode = True
from oracle import ref_boundary as RB
RB.install(model_dir=tempfile.mkdtemp(prefix="mit_models_"))
import manga_translator.inpainting as RI
from manga_translator.inpainting.inpainting_aot import AotInpainter
from manga_translator.inpainting.inpainting_lama_mpe import LamaMPEInpainter
from manga_image_translator_amd import plugins as P
P.register()
assert RI.INPAINTERS["default_hip"] is P.HipAotInpainter
assert issubclass(P.HipAotInpainter, P.HipLamaMPEInpainter) and issubclass(AotInpainter, LamaMPEInpainter)
assert P.HipAotInpainter._MODEL_MAPPING == AotInpainter._MODEL_MAPPING
assert P.HipAotInpainter._infer is P.HipLamaMPEInpainter._infer
inst = RI.get_inpainter("default_hip")
assert isinstance(inst, P.HipAotInpainter) and RI.get_inpainter("default_hip") is inst
print("AOT REGISTERED")
"""


@needs_ref
def test_register_adds_the_aot_inpainter(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", _REGISTER.format(root=ROOT)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path),
                         env=env)
    assert out.returncode == 0 and "AOT REGISTERED" in out.stdout, out.stdout[-3000:] + "\n" + out.stderr[-3000:]


@pytest.mark.parametrize("d", [1, 2, 4, 8, 16])
def test_dilated_conv2d_taps_and_output_size(d):
    conv = ops.Conv2d(torch.randn(32, 128, 3, 3), None, padding=d, dilation=d, pad_mode=ops.PAD_REFLECT, device="cpu")
    assert conv.taps == [(ky * d - d, kx * d - d, 0) for ky in range(3) for kx in range(3)]
    assert conv.out_hw(18, 20) == (18, 20)
    x = torch.nn.functional.conv2d(torch.zeros(1, 1, 41, 57), torch.zeros(1, 1, 3, 3), padding=1, dilation=d, stride=2)
    conv2 = ops.Conv2d(torch.randn(4, 4, 3, 3), None, stride=2, padding=1, dilation=d, device="cpu")
    assert conv2.out_hw(41, 57) == tuple(x.shape[2:])


def test_dilation_one_compiles_to_the_same_taps():
    w = torch.randn(8, 8, 4, 4)
    a = ops.Conv2d(w, None, stride=2, padding=1, device="cpu")
    b = ops.Conv2d(w, None, stride=2, padding=1, dilation=1, device="cpu")
    assert a.taps == b.taps == [(ky - 1, kx - 1, 0) for ky in range(4) for kx in range(4)] and a.out_hw(96, 128) == (48, 64)
    with pytest.raises(ValueError):
        ops.Conv2d(w, None, dilation=0, device="cpu")


def test_engine_rejects_bad_pages_before_any_launch(sd):
    eng = aot.AotEngine.__new__(aot.AotEngine)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        eng.forward(torch.zeros(1, 72, 72, 3), u8(1, 72, 72))
    with pytest.raises(ValueError, match="multiples of 8"):
        eng.forward(u8(1, 76, 80, 3), u8(1, 76, 80))
    with pytest.raises(ValueError, match="at least 72"):
        eng.forward(u8(1, 64, 80, 3), u8(1, 64, 80))
    with pytest.raises(ValueError, match="bad shapes"):
        eng.forward(u8(1, 72, 80, 3), u8(1, 72, 88))
