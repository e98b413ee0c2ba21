"""The AOT inpainter's opt-in bf16 precision on the GPU.

Yardstick (tests/golden/aot_bf16.npz, scripts/make_golden_aot_bf16.py): the float64 oracle (tests/_aot_oracle.py) is the truth, the
reference AOTGenerator's own run under ``torch.autocast("cpu", bfloat16)`` on the same input sets the allowance.  The engine's bf16
precision rounds nothing but convolution operands, so on ``taps["preclip"]`` (value range [-1, 1]) its MEAN absolute error against the
truth must be no larger than the autocast run's.  The mean only: the blend's sigmoid(5 (2 z - 1)) turns a rounding difference near
its steep part into an O(1) difference of single values, so the maximum of either run is luck — it is printed, not asserted
(tests/test_aot_precision.py has the CPU emulation's figures).  No element-wise comparison with an emulation: bf16 rounding is chaotic."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _aot_bf16_emulation as E  # noqa: E402
import _aot_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
_MEMO = {}


def _engine(cuda):
    from manga_image_translator_amd import aot

    if "eng" not in _MEMO:
        _MEMO["eng"] = aot.AotEngine(O.weights(), device=cuda)
    return _MEMO["eng"]


def _pages(cuda, n, H, W, seed0):
    from manga_image_translator_amd import synth

    pages, masks = zip(*[(p, m) for p, _, m in (synth.synth_page(seed0 + i, H, W, n_boxes=3) for i in range(n))])
    return torch.from_numpy(np.stack(pages)).to(cuda), torch.from_numpy(np.stack(masks)).to(cuda)


@pytest.mark.parametrize("name", E.CASES)
def test_bf16_mean_error_is_within_the_autocast_run_s(cuda, oracle_memo, name):
    from manga_image_translator_amd import synth

    fx = np.load(os.path.join(GOLDEN, "aot_bf16.npz"))
    page, mask = E.case_inputs(fx, name)
    H, W = mask.shape

    def run_truth():
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        return E.oracle_preclip(O.weights(), page, mask, torch.float64)

    truth = oracle_memo(("aot_bf16", name), run_truth)
    pages, masks = [page], [mask]
    if name == "b":                                    # B = 2: the fixture page with a stranger behind it
        pages.append(synth.synth_page(77, H, W, n_boxes=3)[0])
        masks.append(E.quarter_mask(H, W))
    taps = {}
    _engine(cuda).forward(torch.from_numpy(np.stack(pages)).to(cuda), torch.from_numpy(np.stack(masks)).to(cuda), taps=taps, precision="bf16")
    torch.cuda.synchronize()
    got = taps["preclip"][:1].permute(0, 3, 1, 2).cpu().numpy()
    assert got.shape == truth.shape and bool(np.isfinite(got).all())
    (em, ex), (am, ax) = E.mean_max(got, truth), E.mean_max(fx[name + "/autocast"], truth)
    print(f"{name}: engine bf16 mean {em:.3e} max {ex:.3e} | reference autocast mean {am:.3e} max {ax:.3e} (the max is informative only)")
    assert em <= am, (em, am)
    assert em > 1e-4, em                               # the reduced precision did run: this is not the fp32 engine under another name


def test_fp32_is_untouched_and_bf16_is_deterministic(cuda):
    from manga_image_translator_amd import aot

    eng = _engine(cuda)
    img, msk = _pages(cuda, 2, 72, 96, 60)
    fresh = aot.AotEngine(O.weights(), device=cuda)
    a = fresh.forward(img, msk).cpu()                  # an engine that has never run bf16
    assert fresh.blocks_bf16 is None
    t16 = {}
    b16 = eng.forward(img, msk, taps=t16, precision="bf16").cpu()
    assert eng.blocks_bf16 is not None
    assert torch.equal(a, eng.forward(img, msk).cpu()) and torch.equal(a, eng.forward(img, msk, precision="fp32").cpu())   # after a bf16 call
    assert not torch.equal(a, b16)
    again = {}
    assert torch.equal(b16, eng.forward(img, msk, taps=again, precision="bf16").cpu())
    assert torch.equal(t16["preclip"], again["preclip"]) and torch.equal(t16["block9"], again["block9"])
    eng.release_workspace()
    assert torch.equal(b16, eng.forward(img, msk, precision="bf16").cpu())
    for i in range(2):                                 # B = 2 equals the pages run alone
        t1 = {}
        o1 = eng.forward(img[i:i + 1], msk[i:i + 1], taps=t1, precision="bf16").cpu()
        assert torch.equal(o1[0], b16[i]), i
        assert torch.equal(t1["preclip"][0], t16["preclip"][i]) and torch.equal(t1["block9"][0], t16["block9"][i]), i
    with pytest.raises(ValueError, match="precision"):
        eng.forward(img, msk, precision="fp16")
    built16 = aot.AotEngine(O.weights(), device=cuda, precision="bf16")
    assert built16.blocks_bf16 is not None             # packed at construction
    assert torch.equal(built16.forward(img, msk).cpu(), b16)
    assert torch.equal(built16.forward(img, msk, precision="fp32").cpu(), a)


def test_micro_batches_of_the_engine_equal_one_batch(cuda):
    from manga_image_translator_amd import aot

    img, msk = _pages(cuda, 3, 72, 80, 64)
    eng2 = aot.AotEngine(O.weights(), device=cuda, mb=2, precision="bf16")
    assert torch.equal(eng2.forward(img, msk), _engine(cuda).forward(img, msk, precision="bf16"))


def test_plugin_end_to_end(cuda):
    """The 250 x 333 scene of RESIZE_CASES with inpainting_size 1024: the pad-to-8 resize on the way in and the resize back."""
    from manga_image_translator_amd import plugins as P

    run = lambda c: asyncio.new_event_loop().run_until_complete(c)
    g = np.load(os.path.join(GOLDEN, "aot_resize.npz"))
    page, mask, size = g["page_a"], g["mask_a"], int(g["size_a"])
    assert page.shape[:2] == (250, 333) and size == 1024
    outs = {}
    for prec in ("fp32", "bf16"):
        inp = P.HipAotInpainter(weights={"aot": O.weights()}, aot_precision=prec)
        run(inp.load("cuda"))
        assert inp.engine.precision == prec and inp.precision_for(None) == prec
        before = page.copy()
        outs[prec] = run(inp.infer(page, mask, None, size))
        assert np.array_equal(page, before)
        run(inp.unload())
    out = outs["bf16"]
    assert out.dtype == np.uint8 and out.shape == page.shape
    hole = mask >= 127
    assert np.array_equal(out[~hole], page[~hole])
    assert not np.array_equal(out[hole], outs["fp32"][hole])
    d = np.abs(outs["fp32"].astype(np.int32) - g["out_a"].astype(np.int32))     # the fp32 plugin is still the reference's bytes
    assert d.max() <= 1 and (d != 0).mean() < 2e-3
    # "config": the call's config decides, and the weights are packed at the first bf16 call
    from types import SimpleNamespace

    inp = P.HipAotInpainter(weights={"aot": O.weights()}, aot_precision="config")
    run(inp.load("cuda"))
    assert inp.engine.blocks_bf16 is None
    assert np.array_equal(run(inp.infer(page, mask, SimpleNamespace(inpainting_precision="fp32"), size)), outs["fp32"])
    assert np.array_equal(run(inp.infer(page, mask, SimpleNamespace(inpainting_precision="fp16"), size)), out)
    run(inp.unload())


def test_inpaint_pages_micro_batches_agree(cuda):
    """The coupled batch's path: ``inpaint_pages`` with one page at a time and with two gives the same bytes in bf16."""
    from manga_image_translator_amd import plugins as P

    eng = _engine(cuda)
    img, msk = _pages(cuda, 2, 100, 90, 68)            # resized to 104 x 96 and back
    one = P.inpaint_pages(eng, img, msk, 1024, None, micro_batch=1, precision="bf16")
    two = P.inpaint_pages(eng, img, msk, 1024, None, micro_batch=2, precision="bf16")
    assert torch.equal(one, two)
    assert not torch.equal(one, P.inpaint_pages(eng, img, msk, 1024, None, micro_batch=2))
    hole = (msk >= 127)
    assert torch.equal(one[~hole], img[~hole])
