"""mc2 colorizer timing (the reference's ``Colorizer.mc2``; not the contract bench): ms per seeded 2048 x 1456 page at
colorization_size 576 and denoise_sigma 30, split into the denoiser (FFDNet, with its INTER_AREA cap) and the generator (resize_pad
+ Generator + output glue), plus one page through HipMangaColorizer.infer, and the grouped convolution's achieved bytes/s at the
tunnel shapes (algorithmic bytes: input read once, output written once).  Prints one JSON line.

    python scripts/bench_mc2.py [--pages 4] [--warmup 1] [--iters 3]
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


def main():
    ap = argparse.ArgumentParser()
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
    eng = mc2.Mc2Engine(g, f, device=dev)
    pages = torch.from_numpy(np.stack([O.synth_color_page(i, H, W) for i in range(N)])).to(dev)
    _size, dn, (ph, pw) = eng.plan(H, W, args.size, args.sigma)
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

    plug = plugins.HipMangaColorizer(weights={"generator": g, "denoiser": f})
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
        "denoiser_ms_per_page": round(t_den / N * 1e3, 3), "generator_ms_per_page": round(t_gen / N * 1e3, 3),
        "denoiser_alg_tflops": round(fl_d * N / t_den / 1e12, 2), "generator_alg_tflops": round(fl_g * N / t_gen / 1e12, 2),
        "plugin_infer_ms_one_page": round(t_plug * 1e3, 3), "grouped_conv": rates,
        "max_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))


if __name__ == "__main__":
    main()
