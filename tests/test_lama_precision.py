"""LaMa's opt-in bf16 precision, the parts that need no GPU: how a plugin's ``precision`` setting and a call's config resolve, the
descriptor field behind it, and the pin of tests/golden/lama_bf16.npz (scripts/make_golden_lama_bf16.py): the reference module's
own fp32 output and its output under torch.autocast(bf16).

The pin shows, on the CPU, that the condition tests/test_lama_bf16_gpu.py imposes on the engine is one the arithmetic of the mode
satisfies: an emulation of the mode on ``oracle.lama`` (tests/_lama_bf16_emulation.py: operands of the convolutions rounded to bf16,
everything kept fp32) stays within the reference autocast run's own error against fp32, mean and max, on every fixture case."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import _lama_bf16_emulation as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lama_bf16.npz")


def test_precision_resolution():
    from manga_image_translator_amd import plugins as P

    cfg = lambda v: SimpleNamespace(inpainting_precision=v)
    assert P.resolve_lama_precision("config", cfg("bf16")) == "bf16"
    assert P.resolve_lama_precision("config", cfg("fp16")) == "bf16"       # the reference turns fp16 into bf16 (:102-104)
    assert P.resolve_lama_precision("config", cfg("fp32")) == "fp32"
    assert P.resolve_lama_precision("config", None) == "fp32"
    assert P.resolve_lama_precision("config", cfg(SimpleNamespace(value="bf16"))) == "bf16"   # an enum member
    assert P.resolve_lama_precision("bf16", cfg("fp32")) == "bf16"         # an explicit setting does not look at the config
    assert P.resolve_lama_precision("fp32", cfg("bf16")) == "fp32"
    with pytest.raises(ValueError):
        P.resolve_lama_precision("fp16", None)
    with pytest.raises(ValueError):
        P.resolve_lama_precision("config", cfg("int8"))


def test_precision_default_from_environment(monkeypatch):
    from manga_image_translator_amd import plugins as P

    monkeypatch.delenv("MIT_LAMA_PRECISION", raising=False)
    assert P.lama_precision_default() == "fp32"
    for cls in (P.HipLamaMPEInpainter, P.HipLamaLargeInpainter, P.HipAotInpainter):
        assert cls(weights={}).precision == "fp32"
    for v in ("bf16", "config", "fp32"):
        monkeypatch.setenv("MIT_LAMA_PRECISION", v)
        assert P.lama_precision_default() == v
        assert P.HipLamaMPEInpainter(weights={}).precision == v
        assert P.HipLamaMPEInpainter(weights={}, precision="fp32").precision == "fp32"   # an argument wins over the environment
    monkeypatch.setenv("MIT_LAMA_PRECISION", "half")
    with pytest.raises(ValueError):
        P.lama_precision_default()
    monkeypatch.delenv("MIT_LAMA_PRECISION")
    with pytest.raises(ValueError):
        P.HipLamaMPEInpainter(weights={}, precision="fp16")
    p = P.HipLamaLargeInpainter(weights={}, precision="config")
    assert p.precision_for(SimpleNamespace(inpainting_precision="fp16")) == "bf16" and p.precision_for(None) == "fp32"
    a = P.HipAotInpainter(weights={}, precision="config")                  # accepted; the AOT engine stays fp32
    assert a.precision_for(SimpleNamespace(inpainting_precision="bf16")) == "fp32"


def test_descriptor_has_nprod():
    import torch

    from manga_image_translator_amd import lib, ops

    assert "nprod" in [f[0] for f in lib.MitConvGemm._fields_]
    assert lib.MitConvGemm().nprod == 0
    w = torch.zeros(16, 8)
    mk = lambda **kw: ops.conv_gemm_desc(a=torch.zeros(1, 2, 2, 16), NB=1, Hi=2, Wi=2, Cin=16, a_strides=(64, 32, 16), Ho=2, Wo=2, sy=1, sx=1,
                                         taps=[(0, 0, 0)], pad_mode=ops.PAD_ZERO, w=w, ldw=8, Kw=16, Nw=8, N=8,
                                         c=ops.tensor_map(torch.zeros(1, 2, 2, 8)), **kw)
    assert mk().nprod == 0 and mk(nprod=1).nprod == 1


@pytest.mark.parametrize("name", E.CASES)
def test_fixture_pin(name):
    fx = np.load(GOLDEN)
    nb, mpe, page, mask = E.case_inputs(fx, name)
    sd, mpe_sd = E.weights(nb, mpe)
    ref32, ref_ac = fx[name + "/fp32"], fx[name + "/autocast"]
    ours32 = E.oracle_float(sd, mpe_sd, page, mask, nb)
    assert np.abs(ours32 - ref32).max() <= 1e-5                            # oracle.lama in fp32 is the stored reference fp32 output
    with E.emulated_bf16():
        emu = E.oracle_float(sd, mpe_sd, page, mask, nb)
    (em, ex), (am, ax) = E.masked_err(emu, ref32, mask), E.masked_err(ref_ac, ref32, mask)
    lv_e, lv_a = E.u8_levels(emu, ref32, mask), E.u8_levels(ref_ac, ref32, mask)
    print(f"{name}: emulation of the mode mean {em:.3e} max {ex:.3e} u8 {lv_e} | reference autocast mean {am:.3e} max {ax:.3e} u8 {lv_a}")
    assert em <= am and ex <= ax, (em, am, ex, ax)
    o_mean, _ = E.masked_err(ours32, ref32, mask)
    assert em > 10 * o_mean and em > 1e-5, (em, o_mean)                  # the patching took effect: not the fp32 run under another name
    assert lv_e <= lv_a, (lv_e, lv_a)
    outside = ~E.mask01(mask)
    assert np.array_equal(emu[0][:, outside], ours32[0][:, outside])       # outside the mask: the page
