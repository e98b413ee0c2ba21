"""AOT inpainter timing (the reference's ``Inpainter.default``; not the contract bench): AotEngine.forward on seeded
2048 x 1456 pages in micro-batches, lama_mpe on the same pages in the same process, one page through HipAotInpainter.infer,
and a parity check of one quarter page against the CPU oracle (tests/_aot_oracle.py).  Prints one JSON line.

    python scripts/bench_aot.py [--pages 16] [--mb 4] [--warmup 1] [--iters 3]
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
    args = ap.parse_args()
    import _aot_oracle as O

    dev = torch.device("cuda:0")
    H, W, N = args.H, args.W, args.pages
    sd = O.weights()
    eng = aot.AotEngine(sd, device=dev, mb=args.mb)
    lsd = synth.synth_state_dict(lama_schema.lama_generator_schema(9))
    lmpe = synth.synth_state_dict(lama_schema.lama_mpe_schema())
    leng = lama.LamaEngine(lsd, lmpe, n_blocks=9, device=dev)
    pages, masks = zip(*[(p, m) for p, _, m in (synth.synth_page(i, H, W) for i in range(N))])
    img, msk = torch.from_numpy(np.stack(pages)).to(dev), torch.from_numpy(np.stack(masks)).to(dev)

    def run_aot():
        eng.forward(img, msk)   # the engine runs its own micro-batches of --mb pages

    def run_lama():
        for b0 in range(0, N, args.lama_mb):
            leng.forward(img[b0:b0 + args.lama_mb], msk[b0:b0 + args.lama_mb])

    for _ in range(args.warmup):
        run_aot()
        run_lama()
    t_aot = timed(run_aot, args.iters)
    t_lama = timed(run_lama, args.iters)

    run = lambda c: asyncio.new_event_loop().run_until_complete(c)
    plug = plugins.HipAotInpainter(weights={"aot": sd})
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

    fl = aot.AotEngine.flops_per_page(H, W)
    print(json.dumps({
        "metric": "aot_inpaint_ms_per_page", "pages": N, "H": H, "W": W, "aot_mb": args.mb, "lama_mb": args.lama_mb,
        "gemm_mode": ops.split_mode(), "aot_ms_per_page": round(t_aot / N * 1e3, 3), "lama_mpe_ms_per_page": round(t_lama / N * 1e3, 3),
        "aot_alg_tflops": round(fl * N / t_aot / 1e12, 2), "plugin_infer_ms_one_page": round(t_plug * 1e3, 3),
        "max_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "parity_quarter_page": parity}))


if __name__ == "__main__":
    main()
