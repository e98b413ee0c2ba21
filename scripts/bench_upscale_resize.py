"""The upscaler's page resize: host (Pillow, what the plugin did) against device (``imgproc.pil_resize_u8``), on one synthetic
2048 x 1440 page at ratio 2 — BASELINE config 5's shape.  Two legs alternated in one process after a warm-up:

  old   forward -> .cpu() of the 4x page -> Image.fromarray -> Pillow BILINEAR resize   (restated here: the plugin no longer does it)
  new   forward -> device resize -> .cpu() of the small page -> Image.fromarray        (``HipESRGANUpscaler._infer``)

Per leg: the resize step alone (everything after ``forward``) and the whole ``_infer``, wall clock around a device synchronisation.
Also: the two resample launches under HIP events with GB/s from the bytes they move, ``mit_resize_u8`` on the same page in the same
run, and the BICUBIC resize back to the input size.  The two legs must return identical bytes; the script exits non-zero otherwise.

    python scripts/bench_upscale_resize.py --out profiles/<tag>_upscale_resize.json
"""
import argparse
import asyncio
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
from PIL import Image

from manga_image_translator_amd import esrgan_schema, imgproc, plugins as P, synth


def _events(fn, iters):
    """Median milliseconds of ``fn`` over ``iters`` runs, one pair of device events around each."""
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1440)
    ap.add_argument("--ratio", type=float, default=2)
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W, ratio = a.height, a.width, a.ratio
    loop = asyncio.new_event_loop()
    up = P.HipESRGANUpscaler(weights=synth.synth_state_dict(esrgan_schema.rrdbnet_schema(a.blocks)))
    loop.run_until_complete(up.load("cuda"))
    eng, dev = up.engine, up.engine.device
    page = synth.synth_page(0, H, W, n_boxes=32)[0]
    pil_page = Image.fromarray(page)
    size = (int(round(4 * W * ratio / 4)), int(round(4 * H * ratio / 4)))
    sync = torch.cuda.synchronize

    def old_leg():
        t0 = time.perf_counter()
        big = eng.forward(torch.from_numpy(np.array(pil_page.convert("RGB"))).to(dev)[None])
        sync()
        t1 = time.perf_counter()
        host = big[0].cpu().numpy()
        t2 = time.perf_counter()
        im = Image.fromarray(host)
        t3 = time.perf_counter()
        out = im.resize(size=(int(round(im.size[0] * ratio / 4)), int(round(im.size[1] * ratio / 4))), resample=Image.Resampling.BILINEAR)
        t4 = time.perf_counter()
        return out, {"infer": t4 - t0, "forward": t1 - t0, "resize_step": t4 - t1, "download": t2 - t1, "fromarray": t3 - t2, "pillow_resize": t4 - t3}

    def new_leg():
        t0 = time.perf_counter()
        big = eng.forward(torch.from_numpy(np.array(pil_page.convert("RGB"))).to(dev)[None])
        sync()
        t1 = time.perf_counter()
        small = imgproc.pil_resize_u8(big, size, "bilinear")
        sync()
        t2 = time.perf_counter()
        host = small[0].cpu().numpy()
        t3 = time.perf_counter()
        out = Image.fromarray(host)
        t4 = time.perf_counter()
        return out, {"infer": t4 - t0, "forward": t1 - t0, "resize_step": t4 - t1, "device_resize": t2 - t1, "download": t3 - t2, "fromarray": t4 - t3}

    old_leg(), new_leg()                                            # warm-up: workspaces, tap tables, the host allocator
    runs = {"old": [], "new": []}
    for _ in range(a.repeats):
        o, to = old_leg()
        n, tn = new_leg()
        runs["old"].append(to)
        runs["new"].append(tn)
        same = o.size == n.size and o.mode == n.mode == "RGB" and np.array_equal(np.asarray(o), np.asarray(n))
        if not same:
            print("the device resize does NOT equal Pillow's bytes", file=sys.stderr)
            return 1
    t0 = time.perf_counter()
    plug = loop.run_until_complete(up.infer([pil_page], ratio))[0]   # the plugin itself: the new leg's code path
    plugin_infer = time.perf_counter() - t0
    if not np.array_equal(np.asarray(plug), np.asarray(n)):
        print("the plugin's page differs from the new leg's", file=sys.stderr)
        return 1

    med = lambda leg, k: statistics.median(r[k] for r in runs[leg])
    summary = {leg: {k: round(med(leg, k) * 1e3, 3) for k in runs[leg][0]} for leg in runs}

    # the launches alone, under device events
    big = eng.forward(torch.from_numpy(page).to(dev)[None])
    _, H4, W4, _ = big.shape
    mid = imgproc.pil_resize_u8(big, (size[0], H4), "bilinear")      # horizontal pass only
    kern = {}
    h_ms = _events(lambda: imgproc.pil_resize_u8(big, (size[0], H4), "bilinear"), a.kernel_iters)
    v_ms = _events(lambda: imgproc.pil_resize_u8(mid, size, "bilinear"), a.kernel_iters)
    both = _events(lambda: imgproc.pil_resize_u8(big, size, "bilinear"), a.kernel_iters)
    cv = _events(lambda: imgproc.resize_u8(big, size), a.kernel_iters)             # mit_resize_u8 (2x box mean at this ratio)
    cv_lin = _events(lambda: imgproc.resize_u8(big, (size[0] - 1, size[1] - 1)), a.kernel_iters)   # its two-tap linear mode
    back = imgproc.pil_resize_u8(big, size, "bilinear")
    rv = _events(lambda: imgproc.pil_resize_u8(back, (W, H), "bicubic"), a.kernel_iters)
    hb, vb = 3 * H4 * (W4 + size[0]), 3 * size[0] * (H4 + size[1])
    gbs = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e9, 1)
    kern["horizontal"] = {"ms": round(h_ms[0], 4), "min_ms": round(h_ms[1], 4), "bytes": hb, "GBps": gbs(hb, h_ms[0])}
    kern["vertical"] = {"ms": round(v_ms[0], 4), "min_ms": round(v_ms[1], 4), "bytes": vb, "GBps": gbs(vb, v_ms[0])}
    kern["both_passes"] = {"ms": round(both[0], 4), "bytes": hb + vb, "GBps": gbs(hb + vb, both[0])}
    ob = 3 * (H4 * W4 + size[0] * size[1])
    kern["mit_resize_u8_box2x"] = {"ms": round(cv[0], 4), "bytes": ob, "GBps": gbs(ob, cv[0])}
    kern["mit_resize_u8_linear"] = {"ms": round(cv_lin[0], 4), "bytes": ob, "GBps": gbs(ob, cv_lin[0])}
    rb = 3 * size[1] * (size[0] + W) + 3 * W * (size[1] + H)
    kern["revert_bicubic_both_passes"] = {"ms": round(rv[0], 4), "bytes": rb, "GBps": gbs(rb, rv[0])}
    ratio_to_cv = kern["both_passes"]["GBps"] / max(kern["mit_resize_u8_linear"]["GBps"], 1e-9)
    note = (f"resample passes at {ratio_to_cv:.2f} of mit_resize_u8's GB/s on the same page (both count algorithmic bytes; the two-pass form "
            "moves the 8-bit intermediate as well)")
    if ratio_to_cv < 0.5:
        note += ("; below half: the horizontal pass loads single bytes (C = 3 pixels are not 4-byte aligned), one load instruction per "
                 "source byte — the likely limit; a counter pass would have to confirm it")
    rec = {"page": [H, W], "ratio": ratio, "blocks": a.blocks, "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "pillow": __import__("PIL").__version__, "ms_median": summary, "runs_s": runs,
           "plugin_infer_ms": round(plugin_infer * 1e3, 3), "bytes_identical": True, "kernels": kern, "note": note,
           "resize_step_speedup": round(summary["old"]["resize_step"] / summary["new"]["resize_step"], 2)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    loop.run_until_complete(up.unload())
    return 0 if summary["new"]["resize_step"] < summary["old"]["resize_step"] else 2


if __name__ == "__main__":
    sys.exit(main())
