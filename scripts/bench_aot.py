"""AOT inpainter timing (the reference's ``Inpainter.default``; not the contract bench): AotEngine.forward on seeded
2048 x 1456 pages in micro-batches, lama_mpe on the same pages in the same process, one page through HipAotInpainter.infer,
and a parity check of one quarter page against the CPU oracle (tests/_aot_oracle.py).  Prints one JSON line.

    python scripts/bench_aot.py [--pages 16] [--mb 4] [--warmup 1] [--iters 3] [--precision fp32|bf16] [--layers]

``--precision bf16`` times the engine's and the plugin's bf16 precision (the parity figures are then the bf16 run's distance to the
fp32 oracle).  ``--layers`` adds, per convolution shape of a block at this page size and micro-batch (the four branch rates alone and
as the one grouped launch, fuse / gate), the median launch time of ``mit_aot_conv3x3_bf16`` beside ``mit_conv_gemm`` with nprod = 1
and with the engine's fp32 tiles.
"""
import argparse
import asyncio
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from manga_image_translator_amd import aot, lama, lama_schema, ops, plugins, synth  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def layer_medians(sd, dev, B, h, w, reps=20):
    """Median milliseconds of one launch per convolution shape of block 0 on [B, h, w, 128]: {"shape": {"aot_bf16", "gemm_p1", "gemm_fp32"}}."""
    from manga_image_translator_amd import aot_schema
    from manga_image_translator_amd.ops import ACT_RELU, PAD_REFLECT

    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn(B, h, w, 128, device=dev, generator=g)
    Xb = X.to(torch.bfloat16)
    out32, out16 = torch.empty(B, h, w, 128, device=dev), torch.empty(B, h, w, 128, dtype=torch.bfloat16, device=dev)
    p = "body_conv.0"

    def median(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return round(float(np.median(ts)), 4)

    res = {}
    names = [f"{p}.block{j:02d}.1" for j in range(len(aot_schema.RATES))]
    convs = []
    for n, r in zip(names, aot_schema.RATES):
        native = ops.AotConv3x3([sd[n + ".weight"]], [sd[n + ".bias"]], [r], act=ACT_RELU, device=dev)
        conv = ops.Conv2d(sd[n + ".weight"], sd[n + ".bias"], padding=r, dilation=r, pad_mode=PAD_REFLECT, act=ACT_RELU, device=dev)
        convs.append(conv)
        res[f"branch r{r} 128->32"] = {"aot_bf16": median(lambda: native(Xb, out_bf16=out16[..., :32])),
                                       "gemm_p1": median(lambda: conv(X, out=out32[..., :32], nprod=1)),
                                       "gemm_fp32": median(lambda: conv(X, out=out32[..., :32]))}
    grouped = ops.AotConv3x3([sd[n + ".weight"] for n in names], [sd[n + ".bias"] for n in names], aot_schema.RATES, act=ACT_RELU, device=dev)

    def four(nprod):
        for j, c in enumerate(convs):
            c(X, out=out32[..., 32 * j:32 * j + 32], nprod=nprod)

    res["four branches"] = {"aot_bf16": median(lambda: grouped(Xb, out_bf16=out16)), "gemm_p1": median(lambda: four(1)),
                            "gemm_fp32": median(lambda: four(0))}
    for nm in ("fuse", "gate"):
        wt, bi = sd[f"{p}.{nm}.1.weight"], sd[f"{p}.{nm}.1.bias"]
        native = ops.AotConv3x3([wt], [bi], [1], device=dev)
        conv = ops.Conv2d(wt, bi, padding=1, pad_mode=PAD_REFLECT, device=dev)
        res[f"{nm} r1 128->128"] = {"aot_bf16": median(lambda: native(Xb, out_f32=out32)), "gemm_p1": median(lambda: conv(X, out=out32, nprod=1)),
                                    "gemm_fp32": median(lambda: conv(X, out=out32))}
    res["cast X 128"] = {"aot_bf16": median(lambda: ops.cast_bf16(X, out16))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--mb", type=int, default=plugins.HipAotInpainter.MB)
    ap.add_argument("--lama-mb", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--H", type=int, default=2048)
    ap.add_argument("--W", type=int, default=1456)
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--no-lama", action="store_true", help="skip the lama_mpe comparison")
    ap.add_argument("--precision", choices=aot.PRECISIONS, default="fp32")
    ap.add_argument("--native", default=None, help="comma list out of branches,fuse,gate (or 'none'): the block convolutions the bf16 "
                    "precision runs on mit_aot_conv3x3_bf16 in this run (default: the engine's own choice, AotEngine.BF16_NATIVE)")
    ap.add_argument("--layers", action="store_true", help="per-layer medians: mit_aot_conv3x3_bf16 vs mit_conv_gemm nprod = 1 / fp32")
    args = ap.parse_args()
    import _aot_oracle as O

    if args.native is not None:
        aot.AotEngine.BF16_NATIVE = frozenset(x for x in args.native.split(",") if x and x != "none")
    dev = torch.device("cuda:0")
    H, W, N = args.H, args.W, args.pages
    sd = O.weights()
    eng = aot.AotEngine(sd, device=dev, mb=args.mb, precision=args.precision)
    lsd = synth.synth_state_dict(lama_schema.lama_generator_schema(9))
    lmpe = synth.synth_state_dict(lama_schema.lama_mpe_schema())
    leng = None if args.no_lama else lama.LamaEngine(lsd, lmpe, n_blocks=9, device=dev)
    pages, masks = zip(*[(p, m) for p, _, m in (synth.synth_page(i, H, W) for i in range(N))])
    img, msk = torch.from_numpy(np.stack(pages)).to(dev), torch.from_numpy(np.stack(masks)).to(dev)

    def run_aot():
        eng.forward(img, msk)   # the engine runs its own micro-batches of --mb pages

    def run_lama():
        for b0 in range(0, N, args.lama_mb):
            leng.forward(img[b0:b0 + args.lama_mb], msk[b0:b0 + args.lama_mb])

    for _ in range(args.warmup):
        run_aot()
        if leng is not None:
            run_lama()
    t_aot = timed(run_aot, args.iters)
    t_lama = timed(run_lama, args.iters) if leng is not None else float("nan")

    run = lambda c: asyncio.new_event_loop().run_until_complete(c)
    plug = plugins.HipAotInpainter(weights={"aot": sd}, aot_precision=args.precision)
    run(plug.load("cuda"))
    page0, mask0 = pages[0], masks[0]
    for _ in range(args.warmup):
        run(plug.infer(page0, mask0, None, max(H, W)))
    t0 = time.perf_counter()
    for _ in range(args.iters):
        run(plug.infer(page0, mask0, None, max(H, W)))
    t_plug = (time.perf_counter() - t0) / args.iters
    run(plug.unload())

    parity = None
    if not args.no_parity:   # one quarter page (both sides halved, still multiples of 8) against the float32 CPU oracle
        qh, qw = H // 2 // 8 * 8, W // 2 // 8 * 8
        qp, _, qm = synth.synth_page(99, qh, qw, n_boxes=8)
        taps = {}
        got = eng.forward(torch.from_numpy(qp[None]).to(dev), torch.from_numpy(qm[None]).to(dev), taps=taps)[0].cpu().numpy()
        ot = {}
        ref = O.infer(sd, qp, qm, ot)
        d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
        pre_err = (taps["preclip"].permute(0, 3, 1, 2).cpu() - ot["preclip"]).abs().max().item()
        parity = {"size": [qh, qw], "u8_max_diff": int(d.max()), "u8_frac_diff": float((d != 0).mean()), "preclip_max_err": pre_err}

    layers = layer_medians(sd, dev, min(args.mb, N), H // 4, W // 4) if args.layers else None
    fl = aot.AotEngine.flops_per_page(H, W)
    print(json.dumps({
        "metric": "aot_inpaint_ms_per_page", "precision": args.precision, "bf16_native": sorted(aot.AotEngine.BF16_NATIVE), "pages": N, "H": H, "W": W, "aot_mb": args.mb, "lama_mb": args.lama_mb,
        "gemm_mode": ops.split_mode(), "aot_ms_per_page": round(t_aot / N * 1e3, 3), "lama_mpe_ms_per_page": round(t_lama / N * 1e3, 3),
        "aot_alg_tflops": round(fl * N / t_aot / 1e12, 2), "plugin_infer_ms_one_page": round(t_plug * 1e3, 3),
        "max_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "parity_quarter_page": parity, "layers_ms": layers}))


if __name__ == "__main__":
    main()
