"""The detector filters of ``CommonDetector.detect`` on the device (csrc/det_filters.hip) against the host form, alternated in one process.

One synthetic 2048 x 1456 page through ``HipDefaultDetector.detect`` with invert + gamma + rotate (seeded weights):
  * host leg: ``det_filters.detect`` with the numpy statements (``apply_host`` / ``undo_masks_host``) around the plugin's ``infer`` —
    the path a reference-importing install takes when the plugin inherits the reference's ``detect``;
  * device leg: the plugin's ``detect`` (upload once, ``mit_det_filter_gray_sum`` / ``mit_det_filter_apply`` before the network,
    ``mit_det_unrotate_u8`` after it, one download).
Each leg also without the network (filters applied and removed only), since the network is the same in both; and the kernels alone
between HIP events, 10 back-to-back calls per pair.  Bytes are compared on every repeat.  One JSON line; ``--out`` also writes it."""
import argparse, asyncio, json, os, statistics, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from manga_image_translator_amd import dbnet_schema, det_filters as DF, plugins as P, synth

warnings.simplefilter("ignore", RuntimeWarning)
ap = argparse.ArgumentParser()
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--detect-size", type=int, default=2048)
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
run = asyncio.new_event_loop().run_until_complete


def spread(ts, nd=3):
    return {"median_ms": round(1e3 * statistics.median(ts), nd), "min_ms": round(1e3 * min(ts), nd), "max_ms": round(1e3 * max(ts), nd), "n": len(ts)}


def timed(fn, sink, record):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    if record:
        sink.append(time.perf_counter() - t)
    return out


H, W = 2048, 1456
page = synth.synth_page(7, H, W, n_boxes=32)[0]
det = P.HipDefaultDetector(weights=synth.synth_state_dict(dbnet_schema.text_detection_schema(), gain=1.2))
run(det.load("cuda"))
ARGS = (a.detect_size, 0.5, 0.7, 2.3)
FLAGS = dict(invert=True, gamma_correct=True, rotate=True)


def same_result(got, want):
    ok = len(got[0]) == len(want[0]) and all(np.array_equal(x.pts, y.pts) for x, y in zip(got[0], want[0]))
    return ok and got[1].shape == want[1].shape and np.array_equal(got[1], want[1]) and got[2] is None and want[2] is None


def filters_host():
    f = DF.apply_host(page, FLAGS["rotate"], FLAGS["invert"], FLAGS["gamma_correct"])
    return f, DF.undo_masks_host(np.ascontiguousarray(f[..., 0]), None, H, W, True)[0]


def filters_device():
    f = DF.apply(torch.from_numpy(page).to(dev), FLAGS["rotate"], FLAGS["invert"], FLAGS["gamma_correct"])
    return f, DF.undo(f[..., 0].contiguous(), None, H, W, True)[0].cpu().numpy()


times = {k: [] for k in ("detect_host", "detect_device", "filters_host", "filters_device")}
same, same_filters, lines = True, True, 0
for it in range(a.warmup + a.repeats):
    rec = it >= a.warmup
    want = timed(lambda: run(DF.detect(det.infer, page, *ARGS, FLAGS["invert"], FLAGS["gamma_correct"], FLAGS["rotate"])), times["detect_host"], rec)
    got = timed(lambda: run(det.detect(page, *ARGS, FLAGS["invert"], FLAGS["gamma_correct"], FLAGS["rotate"])), times["detect_device"], rec)
    same = same and same_result(got, want)
    lines = len(want[0])
    fh, mh = timed(filters_host, times["filters_host"], rec)
    fd, md = timed(filters_device, times["filters_device"], rec)
    same_filters = same_filters and np.array_equal(fd.cpu().numpy(), fh) and np.array_equal(md, mh)

# the kernels alone between HIP events
page_dev = torch.from_numpy(page).to(dev)[None]
lut = torch.from_numpy(DF.gamma_lut(DF.gray_sums(page_dev, True)[0], H * W)[None].copy()).to(dev)
filtered = DF.apply(page_dev, True, True, True)
mask_dev = filtered[0, :, :, 0].contiguous()
from manga_image_translator_amd import lib as _lib, ops
import ctypes as C
L, out, sums = _lib.load(), torch.empty_like(filtered), torch.empty(1, dtype=torch.int64, device=dev)
stream = lambda: C.c_void_p(ops.current_stream())
kernels = {
    "mit_det_filter_gray_sum": lambda: L.mit_det_filter_gray_sum(page_dev.data_ptr(), 1, H, W, 0, 1, sums.data_ptr(), stream()),
    "mit_det_filter_apply_rotated": lambda: L.mit_det_filter_apply(page_dev.data_ptr(), 1, H, W, 1, 0, 1, lut.data_ptr(), out.data_ptr(), stream()),
    "mit_det_filter_apply_plain": lambda: L.mit_det_filter_apply(page_dev.data_ptr(), 1, H, W, 0, 0, 1, lut.data_ptr(), out.data_ptr(), stream()),
    "mit_det_unrotate_u8": lambda: DF.unrotate_u8(mask_dev, W, H),
}
events = {}
for name, fn in kernels.items():
    ev = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) / 10 / 1e3)
    events[name] = spread(ev[2:], 4)

res = {"page": [H, W], "filters": FLAGS, "detect_size": a.detect_size, "lines": lines, "detector": "default (seeded weights)",
       "detect_host_numpy_filters_around_infer": spread(times["detect_host"]), "detect_device": spread(times["detect_device"]),
       "filters_only_host_numpy": spread(times["filters_host"]), "filters_only_device_upload_and_download_included": spread(times["filters_device"]),
       "kernels_between_events_10_calls_per_pair": events,
       "bytes_identical_every_repeat": bool(same), "filters_only_bytes_identical_every_repeat": bool(same_filters),
       "device": torch.cuda.get_device_name(0)}
run(det.unload())
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
