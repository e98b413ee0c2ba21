"""The AOT inpainter's opt-in bf16 precision, the parts that need no GPU: how ``aot_precision`` / ``MIT_AOT_PRECISION`` and a call's
config resolve, what a served batch is told, the argument checks of ``mit_aot_conv3x3_bf16`` (before any HIP call: fake pointers that
are never dereferenced), and the pin of tests/golden/aot_bf16.npz (scripts/make_golden_aot_bf16.py): the reference module's own fp32
output and its output under torch.autocast(bf16).

The pin shows, on the CPU, that the condition tests/test_aot_bf16_gpu.py imposes on the engine is one the arithmetic of the mode
satisfies: an emulation of the mode on the oracle (tests/_aot_bf16_emulation.py) stays within the reference autocast run's own MEAN
error against the float64 oracle on both fixture cases.  The mean only: the blend's sigmoid(5 (2 z - 1)) turns a rounding difference
near its steep part into an O(1) difference of single values, so the maximum of either run is luck (on case b the emulation's is the
larger one)."""
import asyncio
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _aot_bf16_emulation as E  # noqa: E402
import _aot_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "aot_bf16.npz")
FAKE = 1 << 20      # 16-byte aligned, never dereferenced: every call below is refused by the argument checks


# ---- option resolution -------------------------------------------------------------------------------------------------------------
def test_aot_precision_resolution(monkeypatch):
    from manga_image_translator_amd import plugins as P

    monkeypatch.delenv("MIT_AOT_PRECISION", raising=False)
    monkeypatch.delenv("MIT_LAMA_PRECISION", raising=False)
    cfg = lambda v: SimpleNamespace(inpainting_precision=v)
    assert P.aot_precision_default() == "fp32"
    a = P.HipAotInpainter(weights={})
    assert a.aot_precision == "fp32" and a.precision_for(cfg("bf16")) == "fp32" and a.precision_for(None) == "fp32"
    a = P.HipAotInpainter(weights={}, aot_precision="bf16")
    assert a.precision_for(None) == "bf16" and a.precision_for(cfg("fp32")) == "bf16"     # an explicit setting does not look at the config
    a = P.HipAotInpainter(weights={}, aot_precision="config")
    assert a.precision_for(cfg("bf16")) == "bf16"
    assert a.precision_for(cfg("fp16")) == "bf16"                                         # the reference turns fp16 into bf16
    assert a.precision_for(cfg("fp32")) == "fp32"
    assert a.precision_for(cfg(SimpleNamespace(value="bf16"))) == "bf16"                  # an enum member
    assert a.precision_for(None) == "fp32"
    with pytest.raises(ValueError):
        a.precision_for(cfg("int8"))
    with pytest.raises(ValueError):
        P.HipAotInpainter(weights={}, aot_precision="fp16")
    with pytest.raises(ValueError):
        P.HipAotInpainter(weights={}, aot_precision="half")
    # the inherited LaMa option: still validated, still without effect on the AOT engine
    with pytest.raises(ValueError):
        P.HipAotInpainter(weights={}, precision="fp16")
    assert P.HipAotInpainter(weights={}, precision="bf16").precision_for(None) == "fp32"
    assert P.HipAotInpainter(weights={}, precision="fp32", aot_precision="bf16").precision_for(None) == "bf16"


def test_aot_precision_default_from_environment(monkeypatch):
    from manga_image_translator_amd import plugins as P

    monkeypatch.delenv("MIT_LAMA_PRECISION", raising=False)
    for v in ("bf16", "config", "fp32"):
        monkeypatch.setenv("MIT_AOT_PRECISION", v)
        assert P.aot_precision_default() == v
        assert P.HipAotInpainter(weights={}).aot_precision == v
        assert P.HipAotInpainter(weights={}, aot_precision="fp32").aot_precision == "fp32"   # an argument wins over the environment
        assert P.HipLamaMPEInpainter(weights={}).precision == "fp32"                         # LaMa does not listen to it
    monkeypatch.setenv("MIT_AOT_PRECISION", "bf16")
    assert P.HipAotInpainter(weights={}).precision_for(None) == "bf16"
    monkeypatch.setenv("MIT_AOT_PRECISION", "half")
    with pytest.raises(ValueError):
        P.aot_precision_default()
    with pytest.raises(ValueError):
        P.HipAotInpainter(weights={})
    monkeypatch.delenv("MIT_AOT_PRECISION")
    monkeypatch.setenv("MIT_LAMA_PRECISION", "bf16")                                         # LaMa's variable leaves AOT alone
    assert P.HipAotInpainter(weights={}).precision_for(None) == "fp32"


def test_engine_refuses_an_unknown_precision():
    from manga_image_translator_amd import aot

    with pytest.raises(ValueError, match="precision"):
        aot._check_precision("fp16", "AotEngine")
    assert aot._check_precision("bf16", "AotEngine") == "bf16" and aot._check_precision("fp32", "AotEngine") == "fp32"
    with pytest.raises(ValueError, match="precision"):
        aot.AotEngine(O.weights(), device="cpu", precision="fp16")


# ---- serving -----------------------------------------------------------------------------------------------------------------------
def test_served_batch_follows_aot_precision(monkeypatch):
    from manga_image_translator_amd import plugins as P, serve

    monkeypatch.setenv("MIT_SERVE_ENGINE", "tests._serve_batch_stub:make")
    monkeypatch.delenv("MIT_LAMA_PRECISION", raising=False)
    monkeypatch.delenv("MIT_AOT_PRECISION", raising=False)
    stages = serve._make_engine({})

    def batch():
        pages = [np.full((32, 32, 3), v, np.uint8) for v in (1, 2)]
        asyncio.run(stages.translate_batch(pages, {}, batch_size=2))
        return stages.fake.calls[-1][1]

    stages.inp = P.HipAotInpainter(weights={}, aot_precision="bf16")
    assert batch()["precision"] == "bf16"
    stages.inp = P.HipAotInpainter(weights={}, aot_precision="config")     # serve.py hands the plugins no config
    assert batch()["precision"] == "fp32"
    monkeypatch.setenv("MIT_AOT_PRECISION", "bf16")
    stages.inp = P.HipAotInpainter(weights={})
    assert batch()["precision"] == "bf16"


# ---- fixture pin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.CASES)
def test_fixture_pin(name):
    fx = np.load(GOLDEN)
    page, mask = E.case_inputs(fx, name)
    sd = O.weights()
    ref32, ref_ac = fx[name + "/fp32"], fx[name + "/autocast"]
    ours32 = E.oracle_preclip(sd, page, mask)
    assert np.abs(ours32 - ref32).max() <= 1e-5                            # the oracle in fp32 is the stored reference fp32 output
    truth = E.oracle_preclip(sd, page, mask, torch.float64)
    with E.emulated_bf16():
        emu = E.oracle_preclip(sd, page, mask)
    (em, ex), (am, ax), (om, _) = E.mean_max(emu, truth), E.mean_max(ref_ac, truth), E.mean_max(ours32, truth)
    print(f"{name}: emulation of the mode mean {em:.3e} max {ex:.3e} | reference autocast mean {am:.3e} max {ax:.3e} | fp32 oracle mean {om:.3e}")
    assert em <= am, (em, am)                                              # the mean only (module docstring)
    assert em > 10 * om, (em, om)                                          # the patching took effect: not the fp32 run under another name
    # outside the mask the composite (_aot_oracle.infer's last step) is the page, whatever the network's precision
    q =((np.clip(emu[0], -1, 1).transpose(1, 2, 0).astype(np.float32) + 1.0) * 127.5).astype(np.uint8)
    comp = np.where((mask >= 127)[..., None], q, page)
    assert np.array_equal(comp[mask < 127], page[mask < 127]) and not np.array_equal(comp, page)


# ---- kernel entry refusals ---------------------------------------------------------------------------------------------------------
def _desc(lib, **kw):
    """A descriptor the checks accept (the four branches of a block: [1, 20, 40, 128] bf16 -> the bf16 concatenation), then ``kw``."""
    d = lib.MitAotConv()
    d.B, d.H, d.W, d.Cin, d.N, d.groups, d.act = 1, 20, 40, 128, 32, 4, lib.ACT_RELU
    d.in_bs, d.in_ys, d.in_xs = 20 * 40 * 128, 40 * 128, 128
    setattr(d, "in", FAKE)
    for g, r in enumerate((2, 4, 8, 16)):
        d.rate[g], d.out_c0[g] = r, 32 * g
        d.w[g], d.bias[g] = FAKE + (1 << 24) + g * (1 << 20), FAKE + (1 << 28) + g * 4096
    d.out_bf16 = FAKE + (1 << 26)
    d.ob_bs, d.ob_ys, d.ob_xs = d.in_bs, d.in_ys, d.in_xs
    for k, v in kw.items():
        if isinstance(v, dict):                   # an array field: {index: value}
            for i, x in v.items():
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    return d


def _refused(lib, L, what, **kw):
    rc = L.mit_aot_conv3x3_bf16(C.byref(_desc(lib, **kw)), None)
    msg = L.mit_last_error()
    assert rc != 0 and what in msg, (kw, rc, msg)


def test_aot_conv_refuses_bad_arguments_before_any_hip_call():
    from manga_image_translator_amd import lib

    L = lib.load()
    assert (lib.MIT_AOT_TILE_H, lib.MIT_AOT_TILE_W, lib.MIT_AOT_MAX_GROUPS, lib.MIT_AOT_MAX_RATE) == (8, 32, 4, 16)
    assert lib.MIT_ABI_VERSION == 26                                       # the entry is additive
    assert L.mit_aot_conv3x3_bf16(None, None) != 0 and b"null descriptor" in L.mit_last_error()
    _refused(lib, L, b"null pointer", **{"in": None})
    _refused(lib, L, b"null pointer", out_bf16=None)                       # no output at all
    for g in range(4):
        _refused(lib, L, b"null pointer", w={g: None})
    for cin in (0, 16, 48, 100, 130, 544, -128):
        _refused(lib, L, b"Cin must be", Cin=cin)
    for n in (0, 16, 64, 96, 256):
        _refused(lib, L, b"N must be", N=n)
    for k in ("B", "H", "W"):
        for v in (0, -1):
            _refused(lib, L, b"must be positive", **{k: v})
    _refused(lib, L, b"act must be", act=lib.ACT_LEAKY)
    for r in (0, -1, 17, 32):
        _refused(lib, L, b"rate must be", rate={1: r})
    _refused(lib, L, b"H, W > rate", H=16)                                 # rate 16 needs sides of at least 17
    _refused(lib, L, b"H, W > rate", W=16)
    _refused(lib, L, b"H, W > rate", H=8, groups=3)                        # rate 8 of the third group
    for n in (0, 5, -1):
        _refused(lib, L, b"groups must be", groups=n)                      # more than four groups, or none
    # a slice that overruns its buffer: channels [c0, c0 + N) of a pixel must lie inside the x stride of every output
    _refused(lib, L, b"overruns its buffer", out_c0={3: 100})
    _refused(lib, L, b"overruns its buffer", ob_xs=96, ob_ys=40 * 96, ob_bs=20 * 40 * 96)
    _refused(lib, L, b"overruns its buffer", out_f32=FAKE + (1 << 27), of_xs=127, of_ys=40 * 128, of_bs=0)
    _refused(lib, L, b"negative output channel offset", out_c0={0: -32})
    _refused(lib, L, b"overlap", out_c0={1: 16})                           # two groups into the same channels
    _refused(lib, L, b"input strides: x stride smaller", in_xs=120)
    _refused(lib, L, b"input strides: y stride smaller", in_ys=64)
    _refused(lib, L, b"y stride smaller", ob_bs=-8)
    _refused(lib, L, b"16-byte aligned", **{"in": FAKE + 2})
    _refused(lib, L, b"16-byte aligned", w={2: FAKE + (1 << 24) + 6})
    _refused(lib, L, b"16-byte aligned", in_xs=132, in_ys=40 * 132, in_bs=20 * 40 * 132)
    _refused(lib, L, b"2^31 elements", H=1 << 15, W=1 << 10, in_ys=128 << 10, in_bs=128 << 25, ob_ys=128 << 10, ob_bs=128 << 25)
    _refused(lib, L, b"65535", H=8 * 65536, W=17, in_ys=17 * 128, ob_ys=17 * 128)
    _refused(lib, L, b"65535", B=16384, in_bs=0, ob_bs=0)                  # 16384 images x 4 groups
    _refused(lib, L, b"overlaps the input", out_bf16=FAKE + 2 * 1000)


def test_aot_conv_descriptor_from_views():
    from manga_image_translator_amd import lib, ops

    x = torch.zeros(2, 18, 20, 128, dtype=torch.bfloat16)
    cat = torch.zeros(2, 18, 20, 128, dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    ws_ = [torch.randn(32, 128, 3, 3, generator=g) for _ in range(4)]
    layer = ops.AotConv3x3(ws_, [torch.zeros(32)] * 3 + [None], (2, 4, 8, 16), act=ops.ACT_RELU, device="cpu")
    d = layer.desc(x, out_bf16=cat)
    assert (d.B, d.H, d.W, d.Cin, d.N, d.groups, d.act) == (2, 18, 20, 128, 32, 4, lib.ACT_RELU)
    assert list(d.rate) == [2, 4, 8, 16] and list(d.out_c0) == [0, 32, 64, 96]
    assert all(d.w[i] == layer.w[i].data_ptr() for i in range(4)) and d.bias[3] is None and d.bias[0] == layer.bias[0].data_ptr()
    assert (d.ob_bs, d.ob_ys, d.ob_xs) == (18 * 20 * 128, 20 * 128, 128) and not d.out_f32
    assert torch.equal(layer.w[1].view(torch.int16), ops.pack_rdb_weight(ws_[1]).view(torch.int16))
    with pytest.raises(ValueError):
        layer.desc(x[..., :64], out_bf16=cat)
    with pytest.raises(ValueError):
        layer.desc(x, out_f32=cat)                                         # dtype
    with pytest.raises(ValueError):
        ops.AotConv3x3(ws_ + ws_[:1], [None] * 5, (1, 2, 3, 4, 5), device="cpu")
