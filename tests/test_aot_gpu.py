"""The AOT inpainter on the MI355X: the dilated reflect convolution and the plane statistics against float64 torch, the engine
against the CPU oracle (tests/_aot_oracle.py) with taps, batch independence, and the plugin against the reference's own _infer
(tests/golden/aot_resize.npz).  Every engine test runs in both GEMM modes (the ``gemm_mode`` fixture)."""
import asyncio
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _aot_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(cuda, mode):
    """One engine per GEMM mode (weights packed in that mode carry the split planes or not)."""
    from manga_image_translator_amd import aot

    if mode not in _ENGINES:
        _ENGINES[mode] = aot.AotEngine(O.weights(), device=cuda)
    return _ENGINES[mode]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("r", [2, 4, 8, 16])
@pytest.mark.parametrize("side", ["min", "page"])
def test_dilated_reflect_conv(cuda, gemm_mode, r, side):
    from manga_image_translator_amd import ops

    H, W = (r + 1, r + 3) if side == "min" else (37, 52)
    g = torch.Generator().manual_seed(r)
    x = torch.randn(2, 128, H, W, generator=g)
    w = torch.randn(32, 128, 3, 3, generator=g) / 34.0
    b = torch.randn(32, generator=g) * 0.1
    conv = ops.Conv2d(w, b, padding=r, dilation=r, pad_mode=ops.PAD_REFLECT, act=ops.ACT_RELU, device=cuda)
    out = torch.full((2, H, W, 128), 7.0, device=cuda)
    conv(x.permute(0, 2, 3, 1).contiguous().to(cuda), out=out[..., 64:96])   # a 32-channel slice of the concatenation
    torch.cuda.synchronize()
    ref = F.relu(F.conv2d(F.pad(x.double(), [r] * 4, mode="reflect"), w.double(), b.double(), dilation=r))
    got = _nchw(out[..., 64:96].cpu()).double()
    err = (got - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err
    rest = torch.cat([out[..., :64], out[..., 96:]], -1)
    assert bool((rest == 7.0).all()), "the launch wrote outside its slice"


def test_plane_stats_against_float64(cuda):
    from manga_image_translator_amd import aot, ops

    eng = aot.AotEngine.__new__(aot.AotEngine)
    eng._ws = ops.Workspace(cuda)
    g = torch.Generator().manual_seed(3)
    B, h, w, Cc = 3, 37, 29, 128
    x = torch.randn(B, h, w, Cc, generator=g) * 2.0 + 0.5
    x[:, :, :, 5] = 1e3 + 1e-2 * torch.randn(B, h, w, generator=g)   # |mean| >> std
    x[1, :, :, 9] = -40.0 + 1e-3 * torch.randn(h, w, generator=g)
    xd = x.to(cuda)
    mean, istd = torch.empty(B, Cc, device=cuda), torch.empty(B, Cc, device=cuda)
    eng.plane_stats(xd, mean, istd)
    torch.cuda.synchronize()
    x64 = x.double().reshape(B, h * w, Cc)
    rm, rs = x64.mean(1), x64.std(1)
    assert ((mean.cpu().double() - rm).abs() / rm.abs().clamp(min=1.0)).max().item() < 1e-6
    ri = 1.0 / (rs + 1e-9)
    assert ((istd.cpu().double() - ri).abs() / ri).max().item() < 1e-5
    for b in range(B):   # a plane's statistics do not depend on the batch it is in
        m1, i1 = torch.empty(1, Cc, device=cuda), torch.empty(1, Cc, device=cuda)
        eng.plane_stats(xd[b:b + 1].contiguous(), m1, i1)
        assert torch.equal(m1[0], mean[b]) and torch.equal(i1[0], istd[b])


def _u8_close(got, ref, ref_float):
    """Bytes equal except +-1 within 0.05 of a truncation boundary, on fewer than 1e-3 of them (tests/test_lama_gpu.py's rule)."""
    diff = got.astype(np.int32) - ref.astype(np.int32)
    bad = np.argwhere(diff != 0)
    if len(bad):
        assert np.abs(diff).max() <= 1
        v = (np.clip(ref_float, -1, 1) + 1.0) * 127.5
        frac = np.abs(v - np.round(v))
        assert all(frac[tuple(b)] < 0.05 for b in bad), "uint8 mismatch away from a truncation boundary"
        assert len(bad) < 1e-3 * diff.size
    return len(bad)


@pytest.mark.parametrize("H,W", [(72, 80), (96, 128), (256, 184), (2048, 1456)])
def test_engine_matches_the_oracle(cuda, gemm_mode, oracle_memo, H, W):
    from manga_image_translator_amd import synth

    eng = _engine(cuda, gemm_mode)
    page, _, mask = synth.synth_page(7, H, W, n_boxes=6 if H < 1000 else 32)
    mask[3, 5] = 127
    taps = {}
    out = eng.forward(torch.from_numpy(page[None]).to(cuda), torch.from_numpy(mask[None]).to(cuda), taps=taps)
    torch.cuda.synchronize()

    def run_oracle():   # in float64: the blend's sigmoid(5 * (2 z - 1)) amplifies float32 rounding from block to block, so the
        torch.set_num_threads(min(16, os.cpu_count() or 1))   # float32 oracle is itself ~1e-4 away from exact after ten blocks
        ot = {}
        r = O.infer(O.weights(), page, mask, ot, dtype=torch.float64)
        return r, {k: ot[k].float() for k in ["head", "block0", "block4", "block9", "preclip"]}

    ref, ot = oracle_memo(("aot", H, W), run_oracle)
    errs = {}
    for k in ["head", "block0", "block4", "block9", "preclip"]:
        got = _nchw(taps[k].cpu())
        errs[k] = (got - ot[k]).abs().max().item()
        # On the full page the float32 ORACLE itself lies 8.7e-5 (block4), 8.7e-4 (block9) and 4.3e-4 (pre-clip) from this float64
        # run (max |ref| 1.6 / 1.3 / 1.9): among 48 M values per tap, a few sit where the blend's sigmoid is steepest.  No float32
        # order meets 2e-4 there, so the deep taps of that page get 1.5e-3; the head, the first block and the bytes keep the bar.
        bar = 1.5e-3 if H * W > 1 << 20 and k in ("block4", "block9", "preclip") else 2e-4
        assert errs[k] < bar * max(1.0, ot[k].abs().max().item()), (k, errs[k])
    n = _u8_close(out[0].cpu().numpy(), ref, ot["preclip"][0].permute(1, 2, 0).numpy())
    keep = mask < 127
    assert np.array_equal(out[0].cpu().numpy()[keep], page[keep])
    print(f"aot {H}x{W} gemm mode {gemm_mode}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f", u8 diffs {n}")


def test_batch_independence(cuda, gemm_mode):
    from manga_image_translator_amd import synth

    eng = _engine(cuda, gemm_mode)
    pages, masks = zip(*[(p, m) for p, _, m in (synth.synth_page(40 + i, 96, 128, n_boxes=4) for i in range(3))])
    img, msk = torch.from_numpy(np.stack(pages)).to(cuda), torch.from_numpy(np.stack(masks)).to(cuda)
    t3 = {}
    out3 = eng.forward(img, msk, taps=t3)
    for i in range(3):
        t1 = {}
        out1 = eng.forward(img[i:i + 1], msk[i:i + 1], taps=t1)
        assert torch.equal(out1[0], out3[i]), i
        assert torch.equal(t1["preclip"][0], t3["preclip"][i]) and torch.equal(t1["block9"][0], t3["block9"][i]), i
    assert not torch.equal(out3[0], out3[1])


def test_micro_batches_equal_one_batch(cuda):
    from manga_image_translator_amd import aot, synth

    eng2 = aot.AotEngine(O.weights(), device=cuda, mb=2)
    eng = _engine(cuda, 6) if 6 in _ENGINES else aot.AotEngine(O.weights(), device=cuda)
    pages, masks = zip(*[(p, m) for p, _, m in (synth.synth_page(50 + i, 72, 96, n_boxes=3) for i in range(3))])
    img, msk = torch.from_numpy(np.stack(pages)).to(cuda), torch.from_numpy(np.stack(masks)).to(cuda)
    assert torch.equal(eng.forward(img, msk), eng2.forward(img, msk))


def test_plugin_against_the_reference_infer(cuda, gemm_mode):
    from manga_image_translator_amd import plugins as P

    run = lambda c: asyncio.new_event_loop().run_until_complete(c)
    g = np.load(os.path.join(ROOT, "tests", "golden", "aot_resize.npz"))
    inp = P.HipAotInpainter(weights={"aot": O.weights()})
    run(inp.load("cuda"))
    for tag in ("a", "b"):
        page, mask, size = g[f"page_{tag}"], g[f"mask_{tag}"], int(g[f"size_{tag}"])
        before, mbefore = page.copy(), mask.copy()
        out = run(inp.infer(page, mask, None, size))
        assert out.shape == page.shape and out.dtype == np.uint8
        assert np.array_equal(page, before) and np.array_equal(mask, mbefore)
        d = np.abs(out.astype(np.int32) - g[f"out_{tag}"].astype(np.int32))
        assert d.max() <= 1 and (d != 0).mean() < 2e-3, (tag, d.max(), (d != 0).mean())
        assert np.array_equal(out[mask < 127], page[mask < 127])
        print(f"aot plugin {page.shape[:2]} size {size} gemm mode {gemm_mode}: {int((d != 0).sum())} of {d.size} bytes differ by 1")
    with pytest.raises(ValueError):
        run(inp.infer(g["page_a"], g["mask_a"][:10], None, 1024))
    small = np.full((60, 200, 3), 200, np.uint8)   # resized to 64 x 200: below the 72 the dilated branches need
    with pytest.raises(ValueError, match="at least 72"):
        run(inp.infer(small, np.zeros((60, 200), np.uint8), None, 1024))
    run(inp.unload())


def test_kernels_refuse_bad_arguments(cuda):
    from manga_image_translator_amd import lib

    L = lib.load()
    x = torch.zeros(4, 8, device=cuda)
    assert L.mit_aot_gate(x.data_ptr(), 6, x.data_ptr(), 4, 4, 4, 0, None) != 0 and b"pixel strides" in L.mit_last_error()
    assert L.mit_aot_plane_stats(x.data_ptr(), 32, 8, 1, 4, 12, x.data_ptr(), 1 << 20, x.data_ptr(), x.data_ptr(), None) != 0
    assert b"power of two" in L.mit_last_error()
    assert L.mit_aot_plane_stats(x.data_ptr(), 32, 8, 1, 4, 8, x.data_ptr(), 8, x.data_ptr(), x.data_ptr(), None) != 0
    assert b"workspace too small" in L.mit_last_error()
