"""mc2 colorizer timing (the reference's ``Colorizer.mc2``; not the contract bench): ms per seeded 2048 x 1456 page at
colorization_size 576 and denoise_sigma 30, split into the denoiser (FFDNet, with its INTER_AREA cap) and the generator (resize_pad
+ Generator + output glue), plus one page through HipMangaColorizer.infer, and the grouped convolution's achieved bytes/s at the
tunnel shapes (algorithmic bytes: input read once, output written once).  Prints one JSON line.

    python scripts/bench_mc2.py [--pages 4] [--warmup 1] [--iters 3] [--precision fp32|bf16]
    python scripts/bench_mc2.py --alternate [--repeats 10]     fp32 and bf16 in one process, alternated: median and range of the
                                                               denoiser, the generator and the whole forward, ms per page
    python scripts/bench_mc2.py --layers                       the FFDNet 96 -> 96 layer (and exit.0) between HIP events: the bf16
                                                               kernel in one launch, as 64 + 32 columns, and mit_conv_gemm nprod = 1
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

from manga_image_translator_amd import imgproc, mc2, ops, plugins  # noqa: E402

HBM_PEAK = 8.0e12   # MI355X HBM3E, spec


def timed(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def grouped_rate(eng, dev, C, cpg, d, H, W, B, iters):
    conv = mc2._Grouped(torch.randn(C, cpg, 3, 3) * 0.1, C, 1, d, ops.ACT_LEAKY, device=dev)
    x = torch.randn(B, H, W, C, device=dev)
    y = torch.empty_like(x)
    for _ in range(3):
        conv(x, y)
    t = timed(lambda: conv(x, y), iters * 10)
    nbytes = 2 * 4.0 * B * H * W * C
    return {"C": C, "cpg": cpg, "dil": d, "HxW": [H, W], "B": B, "us": round(t * 1e6, 1), "GBps": round(nbytes / t / 1e9, 1),
            "frac_hbm_peak": round(nbytes / t / HBM_PEAK, 3)}


def event_ms(fn, launches, repeats):
    """Median, min and max ms per launch over ``repeats`` event pairs around ``launches`` back-to-back calls."""
    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / launches)
    return {"median_us": round(float(np.median(out)) * 1e3, 2), "min_us": round(min(out) * 1e3, 2), "max_us": round(max(out) * 1e3, 2)}


def layer_times(dev, dn, Hp, pw, N, launches=20, repeats=7):
    """Measurement B: one layer three ways on seeded operands at the benchmark's shapes."""
    g = torch.Generator().manual_seed(5)
    h2, w2 = (dn[0] + 1) // 2, (dn[1] + 1) // 2
    res = {"launches_per_event_pair": launches, "repeats": repeats}
    for name, (B, H, W, Cin, Cout) in (("ffdnet_96_96", (N, h2, w2, 96, 96)), ("exit0_96_32", (N, Hp, pw, 96, 32))):
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
        bias = torch.randn(Cout, generator=g)
        x32 = torch.randn(B, H, W, Cin, device=dev)
        x16 = x32.to(torch.bfloat16)
        o16 = torch.empty(B, H, W, Cout, dtype=torch.bfloat16, device=dev)
        o32 = torch.empty(B, H, W, Cout, device=dev)
        one = ops.Conv3x3Bf16(w, bias, act=ops.ACT_RELU, device=dev)
        gemm = ops.Conv2d(w, bias, padding=1, act=ops.ACT_RELU, device=dev)
        r = {"shape_BHWCinCout": [B, H, W, Cin, Cout], "bf16_one_launch": event_ms(lambda: one(x16, out_bf16=o16), launches, repeats)}
        if Cout == 96:
            two = ops.Conv3x3Bf16(w, bias, act=ops.ACT_RELU, split=(64, 32), device=dev)
            r["bf16_64_plus_32"] = event_ms(lambda: two(x16, out_bf16=o16), launches, repeats)
        else:   # exit.0 reads an fp32 buffer: the cast belongs to the bf16 kernel's cost, its output stays fp32
            r["bf16_one_launch_f32_out"] = event_ms(lambda: one(x16, out_f32=o32), launches, repeats)
            r["cast_f32_bf16"] = event_ms(lambda: ops.cast_bf16(x32, x16), launches, repeats)
        r["conv_gemm_nprod1"] = event_ms(lambda: gemm(x32, out=o32, nprod=1), launches, repeats)
        r["conv_gemm_fp32"] = event_ms(lambda: gemm(x32, out=o32), launches, repeats)
        res[name] = r
    return res


def alternate(eng, pages, args, ph, pw):
    """Measurement A: fp32 and bf16 alternated in one process; median and range, ms per page."""
    N = pages.shape[0]
    t = {p: {"denoiser": [], "generator": [], "forward": []} for p in mc2.PRECISIONS}
    planes = {}

    def legs(p):
        def den():
            planes[p] = eng.denoise(pages, args.sigma, precision=p)
        return (("denoiser", den), ("generator", lambda: eng.colorize(imgproc.resize_u8(planes[p], (pw, ph), area=True), precision=p)),
                ("forward", lambda: eng.forward(pages, args.size, args.sigma, precision=p)))

    for _ in range(max(args.warmup, 2)):
        for p in mc2.PRECISIONS:
            for _name, fn in legs(p):
                fn()
    for _ in range(args.repeats):
        for p in mc2.PRECISIONS:
            for name, fn in legs(p):
                t[p][name].append(timed(fn, args.iters) / N * 1e3)
    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}   # noqa: E731
    return {p: {k: stat(v) for k, v in t[p].items()} for p in t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=mc2.PRECISIONS, default="fp32")
    ap.add_argument("--alternate", action="store_true", help="fp32 and bf16 alternated in one process (measurement A)")
    ap.add_argument("--layers", action="store_true", help="per-layer event timings (measurement B)")
    ap.add_argument("--repeats", type=int, default=10, help="alternated repeats of --alternate")
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--size", type=int, default=576)
    ap.add_argument("--sigma", type=float, default=30)
    args = ap.parse_args()
    import _mc2_oracle as O

    dev = torch.device("cuda:0")
    H, W, N = 2048, 1456, args.pages
    g, f = O.weights()
    eng = mc2.Mc2Engine(g, f, device=dev, precision=args.precision)
    pages = torch.from_numpy(np.stack([O.synth_color_page(i, H, W) for i in range(N)])).to(dev)
    _size, dn, (ph, pw) = eng.plan(H, W, args.size, args.sigma)
    if args.alternate or args.layers:
        out = {"metric": "mc2_precision_ab", "pages": N, "H": H, "W": W, "size": args.size, "sigma": args.sigma, "gemm_mode": ops.split_mode(),
               "iters": args.iters}
        if args.alternate:
            out.update(repeats=args.repeats, ms_per_page=alternate(eng, pages, args, ph, pw))
        if args.layers:
            out["layers"] = layer_times(dev, dn, ph + 32 - ph % 32, pw, N)
        print(json.dumps(out))
        return
    planes = [None]

    def run_den():
        planes[0] = eng.denoise(pages, args.sigma)

    def run_gen():
        eng.colorize(imgproc.resize_u8(planes[0], (pw, ph), area=True))

    for _ in range(args.warmup):
        run_den()
        run_gen()
    t_den = timed(run_den, args.iters)
    t_gen = timed(run_gen, args.iters)

    run = lambda c: asyncio.new_event_loop().run_until_complete(c)
    from PIL import Image

    plug = plugins.HipMangaColorizer(weights={"generator": g, "denoiser": f}, precision=args.precision)
    run(plug.load("cuda"))
    im = Image.fromarray(pages[0].cpu().numpy())
    for _ in range(args.warmup):
        run(plug.infer(im, args.size, denoise_sigma=args.sigma))
    t0 = time.perf_counter()
    for _ in range(args.iters):
        run(plug.infer(im, args.size, denoise_sigma=args.sigma))
    t_plug = (time.perf_counter() - t0) / args.iters
    run(plug.unload())

    Hp = ph + 32 - ph % 32
    rates = [grouped_rate(eng, dev, 256, 8, 1, Hp // 8, pw // 8, 1, args.iters),     # tunnel4 (512-channel blocks, D = 256)
             grouped_rate(eng, dev, 64, 2, 4, Hp // 2, pw // 2, 1, args.iters),      # tunnel2 (128-channel blocks, D = 64)
             grouped_rate(eng, dev, 64, 2, 1, Hp // 2, pw // 2, 1, args.iters)]
    fl_g, fl_d = mc2.Mc2Engine.flops_per_page(Hp, pw), mc2.Mc2Engine.ffd_flops(*dn)
    print(json.dumps({
        "metric": "mc2_colorize_ms_per_page", "pages": N, "H": H, "W": W, "size": args.size, "sigma": args.sigma, "gemm_mode": ops.split_mode(),
        "precision": args.precision, "denoiser_ms_per_page": round(t_den / N * 1e3, 3), "generator_ms_per_page": round(t_gen / N * 1e3, 3),
        "denoiser_alg_tflops": round(fl_d * N / t_den / 1e12, 2), "generator_alg_tflops": round(fl_g * N / t_gen / 1e12, 2),
        "plugin_infer_ms_one_page": round(t_plug * 1e3, 3), "grouped_conv": rates,
        "max_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


if __name__ == "__main__":
    main()
