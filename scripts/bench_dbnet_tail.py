"""The DBNet detectors' mask tail (detection/default.py:89-95) on the device (csrc/dbnet_tail.hip) against the numpy tail it replaces.

1. the kernel alone under HIP events (20 back-to-back launches per event pair, so the figure includes the launch cadence of the Python
   wrapper) at the default detection size's map (1024 x 768 -> 2048 x 1536 bytes): median / min / max and TB/s over its algorithmic bytes (4 per source element read + 1 per output byte written), bytes compared with the numpy expression;
2. ``HipDefaultDetector.infer`` on one 2048 x 1456 page, ``detect_size`` 2048: the plugin as it is (device tail) against the same
   plugin with ``resize2x=plugins._resize2x_f32`` injected (the numpy tail: the float mask comes down, is resized and cast on the
   host), the two alternated in one process, lines and mask bytes compared on every repeat.

One JSON line; ``--out`` also writes it to a file."""
import argparse, asyncio, json, os, statistics, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from manga_image_translator_amd import dbnet_schema, imgproc, plugins as P, synth

warnings.simplefilter("ignore", RuntimeWarning)
ap = argparse.ArgumentParser()
ap.add_argument("--map-h", type=int, default=1024)
ap.add_argument("--map-w", type=int, default=768)
ap.add_argument("--batch", type=int, nargs="+", default=[1, 16], help="maps per launch: one page, and a coupled group's micro-batch")
ap.add_argument("--kernel-iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
run = asyncio.new_event_loop().run_until_complete


def spread(ts, scale=1.0, nd=3):
    return {"median_ms": round(scale * statistics.median(ts), nd), "min_ms": round(scale * min(ts), nd), "max_ms": round(scale * max(ts), nd), "n": len(ts)}


# ---- 1. the kernel alone ----
INNER = 20      # launches between one pair of events: a launch of a few microseconds is below what one pair resolves


def kernel_leg(B):
    h, w = a.map_h, a.map_w
    m = np.random.default_rng(B).uniform(-0.1, 1.1, (B, h, w)).astype(np.float32)
    src = torch.from_numpy(m).to(dev)
    out = torch.empty(B, 2 * h, 2 * w, dtype=torch.uint8, device=dev)
    for _ in range(5):
        imgproc.dbnet_mask_tail(src, 2 * h, 2 * w, out=out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.kernel_iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            imgproc.dbnet_mask_tail(src, 2 * h, 2 * w, out=out)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / INNER)
    t0 = time.perf_counter()
    want = np.clip(P._resize2x_f32(m[0]) * 255, 0, 255).astype(np.uint8)
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    nbytes = B * (4 * h * w + 4 * h * w)       # 4 bytes per source element read + 1 per output byte written (4 per source element)
    return {"map": [B, h, w], "out": [B, 2 * h, 2 * w], **spread(ts, nd=4), "algorithmic_bytes": nbytes,
            "TBps": round(nbytes / statistics.median(ts) / 1e9, 3), "first_map_bytes_equal_numpy": bool(np.array_equal(out[0].cpu().numpy(), want)),
            "numpy_expression_ms_per_map": round(numpy_ms, 1)}


res = {"kernel": [kernel_leg(B) for B in a.batch]}

# ---- 2. the plugin on one page: device tail / numpy tail, alternated ----
H, W, S = 2048, 1456, 2048
sd = synth.synth_state_dict(dbnet_schema.text_detection_schema(), gain=1.2)
legs = {"numpy_tail": P.HipDefaultDetector(weights=sd, resize2x=P._resize2x_f32), "device_tail": P.HipDefaultDetector(weights=sd)}
for p in legs.values():
    run(p.load("cuda"))
page = synth.synth_page(7, H, W, n_boxes=32, disjoint=True)[0]
times = {k: [] for k in legs}
same = True
for it in range(a.warmup + a.repeats):
    got = {}
    for name, det in legs.items():
        torch.cuda.synchronize()
        t = time.perf_counter()
        got[name] = run(det.infer(page, S, 0.5, 0.7, 2.3))
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[name].append(time.perf_counter() - t)
    (at, am, _), (bt, bm, _) = got["numpy_tail"], got["device_tail"]
    same = same and len(at) == len(bt) and all(np.array_equal(x.pts, y.pts) for x, y in zip(at, bt)) and np.array_equal(am, bm)
res["infer"] = {"page": [H, W], "detect_size": S, "mask": list(got["device_tail"][1].shape), "lines": len(got["device_tail"][0]),
                "numpy_tail": spread(times["numpy_tail"], 1e3), "device_tail": spread(times["device_tail"], 1e3),
                "lines_and_mask_bytes_identical_every_repeat": bool(same)}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
