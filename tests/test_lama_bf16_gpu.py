"""LaMa's opt-in bf16 precision (``LamaEngine.forward(precision="bf16")``, the plugins' ``precision`` option) at the network level.

The yardstick is the reference's own autocast run, stored with its fp32 run in tests/golden/lama_bf16.npz
(scripts/make_golden_lama_bf16.py); tests/test_lama_precision.py pins that fixture on the CPU.  With err(x) = |x - reference fp32|
over the masked pixels of the sigmoid output, the engine in bf16 must have mean err and max err no larger than the reference's
autocast run has — no margin: the mode rounds the operands of the convolutions as autocast does and does not round layer outputs,
so it does strictly less rounding — and its uint8 page may differ from the fp32 engine's by at most as many levels as the reference's
two runs differ.  Element-wise closeness of the whole network to an emulation is deliberately not tested: rounding to bf16 is chaotic
over 40-80 layers (layer-level sharpness is tests/test_gemm_p1_gpu.py).

Measured on MI355X (engine bf16 | reference autocast; mean / max err, uint8 levels): profiles/r17a_p1_lama_bf16_gpu.log (listed in profiles/README.md)."""
import asyncio
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _lama_bf16_emulation as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lama_bf16.npz")


def _engine(nb, mpe, cuda):
    from manga_image_translator_amd import lama

    sd, mpe_sd = E.weights(nb, mpe)
    return lama.LamaEngine(sd, mpe_sd, n_blocks=nb, device=cuda)


def _run(eng, pages, masks, precision):
    cuda = eng.device
    taps = {}
    out = eng.forward(torch.from_numpy(np.stack(pages)).to(cuda), torch.from_numpy(np.stack(masks)).to(cuda), taps=taps, precision=precision)
    torch.cuda.synchronize()
    return out.cpu().numpy(), taps["pred"].permute(0, 3, 1, 2).cpu().numpy()      # u8 [B,H,W,3], pred [B,3,H,W]


def _levels(a, b, inside):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32))[inside].max())


@pytest.mark.parametrize("name", E.CASES)
def test_bf16_against_the_reference_autocast_run(cuda, name):
    fx = np.load(GOLDEN)
    nb, mpe, page, mask = E.case_inputs(fx, name)
    ref32, ref_ac = fx[name + "/fp32"], fx[name + "/autocast"]
    eng = _engine(nb, mpe, cuda)
    u32, p32 = _run(eng, [page], [mask], "fp32")
    ub, pb = _run(eng, [page], [mask], "bf16")
    (fm, fxm), (bm, bx), (am, ax) = E.masked_err(p32, ref32, mask), E.masked_err(pb, ref32, mask), E.masked_err(ref_ac, ref32, mask)
    inside = E.mask01(mask)
    lv, lv_ref = _levels(ub[0], u32[0], inside), E.u8_levels(ref_ac, ref32, mask)
    print(f"{name}: engine fp32 mean {fm:.3e} max {fxm:.3e} | engine bf16 mean {bm:.3e} max {bx:.3e} | reference autocast mean {am:.3e} "
          f"max {ax:.3e} | u8 levels bf16 vs fp32 engine {lv}, reference autocast vs fp32 {lv_ref}")
    assert fxm <= 2e-4                                                     # the fp32 engine is the reference fp32 run (test_lama_gpu.py's tolerance)
    assert bm <= am, (bm, am)
    assert bx <= ax, (bx, ax)
    assert bm > 10 * fm                                                    # the precision did change: not the fp32 path under another name
    assert lv <= lv_ref, (lv, lv_ref)
    outside = mask < 127
    assert np.array_equal(ub[0][outside], page[outside])                   # outside the mask the bytes are the input page's


def test_bf16_is_deterministic_batch_independent_and_leaves_fp32_alone(cuda):
    from manga_image_translator_amd import synth

    eng = _engine(9, True, cuda)
    H, W = 128, 160
    gen = [synth.synth_page(30 + i, H, W, n_boxes=4) for i in range(3)]
    pages, masks = [g[0] for g in gen], [g[2] for g in gen]
    f0, pf0 = _run(eng, pages[1:2], masks[1:2], "fp32")
    b1, pb1 = _run(eng, pages[1:2], masks[1:2], "bf16")
    b1again, pb1again = _run(eng, pages[1:2], masks[1:2], "bf16")
    assert np.array_equal(b1, b1again) and np.array_equal(pb1, pb1again)   # two runs: equal bytes
    b3, pb3 = _run(eng, pages, masks, "bf16")
    assert np.array_equal(b3[1], b1[0]) and np.array_equal(pb3[1], pb1[0])  # B = 1 against the same page inside B = 3
    f1, pf1 = _run(eng, pages[1:2], masks[1:2], "fp32")
    assert np.array_equal(f1, f0) and np.array_equal(pf1, pf0)             # fp32 -> bf16 -> fp32: the fp32 bytes unchanged
    f3, _ = _run(eng, pages, masks, "fp32")
    assert np.array_equal(f3[1], f0[0])
    assert not np.array_equal(pb1, pf0)
    with pytest.raises(ValueError):
        _run(eng, pages[:1], masks[:1], "fp16")
    # an engine built without Winograd (direct-form FFC blocks from the start) gives the same bf16 bytes: the form, not the object
    from manga_image_translator_amd import lama
    sd, mpe_sd = E.weights(9, True)
    direct = lama.LamaEngine(sd, mpe_sd, n_blocks=9, device=cuda, winograd=False)
    bd, pbd = _run(direct, pages[1:2], masks[1:2], "bf16")
    assert np.array_equal(bd, b1) and np.array_equal(pbd, pb1)


def test_bf16_on_the_baseline_page(cuda):
    """2048 x 1456, 9 blocks + MPE, bf16 against the fp32 engine.  The cap of 2 levels is what the reference's own autocast run shows
    against its fp32 run on a page of this size (the emulation of the mode shows 1): a guard against a gross failure, not the accuracy
    claim, which the fixture cases carry."""
    from manga_image_translator_amd import synth

    eng = _engine(9, True, cuda)
    page, _, mask = synth.synth_page(3, 2048, 1456, n_boxes=4)
    u32, p32 = _run(eng, [page], [mask], "fp32")
    ub, pb = _run(eng, [page], [mask], "bf16")
    inside = E.mask01(mask)
    d = np.abs(pb.astype(np.float64) - p32)[0][:, inside]
    lv = np.abs(ub[0].astype(np.int32) - u32[0].astype(np.int32))
    hist = np.bincount(lv[inside].ravel(), minlength=4)
    print(f"BASELINE page bf16 vs fp32 engine: pred mean {d.mean():.3e} max {d.max():.3e} over {int(inside.sum())} masked pixels; "
          f"uint8 level histogram {hist.tolist()}")
    assert lv.max() <= 2
    outside = mask < 127
    assert np.array_equal(ub[0][outside], page[outside]) and np.array_equal(ub[0][outside], u32[0][outside])
    assert d.mean() > 0


def test_plugins_follow_the_precision_option(cuda):
    from manga_image_translator_amd import lama_schema, plugins as P, synth
    from _aot_oracle import weights as aot_weights

    run = asyncio.new_event_loop().run_until_complete
    sd, mpe_sd = E.weights(9, True)
    w = {"lama.gen": sd, "lama.mpe": mpe_sd}
    page, _, mask = synth.synth_page(41, 250, 333, n_boxes=4)             # goes through the resize legs (inpainting_size 160)
    cfg = lambda v: SimpleNamespace(inpainting_precision=v)
    plug = P.HipLamaMPEInpainter(weights=dict(w), precision="config")
    run(plug.load("cuda"))
    img0, msk0 = torch.from_numpy(page).to(cuda)[None], torch.from_numpy(mask).to(cuda)[None]
    want_bf = P.inpaint_pages(plug.engine, img0, msk0, 160, precision="bf16")[0].cpu().numpy()
    want_32 = P.inpaint_pages(plug.engine, img0, msk0, 160)[0].cpu().numpy()
    assert not np.array_equal(want_bf, want_32)
    assert np.array_equal(run(plug._infer(page, mask, cfg("bf16"), 160)), want_bf)
    assert np.array_equal(run(plug._infer(page, mask, cfg("fp16"), 160)), want_bf)
    assert np.array_equal(run(plug._infer(page, mask, cfg("fp32"), 160)), want_32)
    assert np.array_equal(run(plug._infer(page, mask, None, 160)), want_32)
    run(plug.unload())
    fixed = P.HipLamaMPEInpainter(weights=dict(w), precision="bf16")
    run(fixed.load("cuda"))
    assert np.array_equal(run(fixed._infer(page, mask, None, 160)), want_bf)
    run(fixed.unload())
    # lama_large inherits the option
    sd18, _ = E.weights(18, False)
    large = P.HipLamaLargeInpainter(weights={"lama.gen": sd18}, precision="config")
    run(large.load("cuda"))
    l32, lbf = run(large._infer(page, mask, None, 160)), run(large._infer(page, mask, cfg("bf16"), 160))
    assert not np.array_equal(l32, lbf)
    run(large.unload())
    # the AOT inpainter accepts the option and keeps running in fp32
    aw = {"aot": aot_weights()}
    a_cfg, a_32 = P.HipAotInpainter(weights=dict(aw), precision="config"), P.HipAotInpainter(weights=dict(aw))
    for a in (a_cfg, a_32):
        run(a.load("cuda"))
    assert np.array_equal(run(a_cfg._infer(page, mask, cfg("bf16"), 160)), run(a_32._infer(page, mask, None, 160)))
    for a in (a_cfg, a_32):
        run(a.unload())


def test_coupled_engine_passes_the_precision_on(cuda):
    from manga_image_translator_amd import coupled, ctd as CTD, pipeline, plugins as P, synth

    H, W, NB, T, D = 1024, 728, 4, 6, 211
    weights = pipeline.synthetic_weights(dict_size=D)
    dictionary = ["<PAD>", "<S>", "</S>", "<SP>"] + [chr(0x4E00 + i) for i in range(D - 4)]
    gen = [synth.synth_page(20 + i, H, W, n_boxes=NB, disjoint=True) for i in range(2)]
    pages, masks = [g[0] for g in gen], [g[2] for g in gen]
    nh, nw, dw, dh = CTD.CtdEngine.letterbox_geometry(H, W)
    heads = [coupled.synthetic_head_outputs(g[0], g[1], (CTD.INPUT_SIZE - dh, CTD.INPUT_SIZE - dw)) for g in gen]
    inj = {"prob": torch.from_numpy(np.stack([h[0] for h in heads])).to(cuda), "mask": torch.from_numpy(np.stack([h[1] for h in heads])).to(cuda)}
    pages_dev = torch.from_numpy(np.stack(pages)).to(cuda)
    run = asyncio.new_event_loop().run_until_complete
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        eng = coupled.CoupledPageEngine(weights, dictionary, device=cuda, ctd_mb=2, lama_mb=2, host_workers=4)
        kw = dict(max_seq_length=T, suppress_eos=True, prob_threshold=0.0, inject=inj, mask=masks, inpainting_size=max(H, W))
        rb = eng.run(pages_dev, precision="bf16", **kw)
        r32 = eng.run(pages_dev, **kw)
        piped = eng.run(pages_dev, precision="bf16", group=1, **kw)
        direct = eng.run(pages_dev, max_seq_length=T, suppress_eos=True, prob_threshold=0.0, inject=inj, mask=masks, precision="bf16")
        torch.cuda.synchronize()
        eng.close()
        with pytest.raises(ValueError):
            eng.run(pages_dev, precision="fp16", **kw)
    assert torch.equal(piped.inpainted, rb.inpainted) and not torch.equal(rb.inpainted, r32.inpainted)
    assert torch.equal(direct.inpainted, rb.inpainted)      # pages of a multiple-of-8 size: the resize legs are the identity
    inp = P.HipLamaMPEInpainter(weights=weights, precision="config")
    run(inp.load("cuda"))
    for k in range(2):
        want = run(inp._infer(pages[k], masks[k], SimpleNamespace(inpainting_precision="bf16"), max(H, W)))
        assert np.array_equal(rb.inpainted[k].cpu().numpy(), want)
        assert np.array_equal(r32.inpainted[k].cpu().numpy(), run(inp._infer(pages[k], masks[k], None, max(H, W))))
    run(inp.unload())
