"""The ``--ignore-bubble`` rules on the device (csrc/bubble.hip) against the host paths they replace, alternated in one process.

1. the bubble stage of the mask refinement on one synthetic 2048 x 1456 page with a 32-line mask that lives on the device, as mask
   refinement leaves it: the host leg downloads the mask and runs ``mask_refinement.bubble_filter`` (numpy + scipy: what
   ``dispatch_sync`` did), the device leg is ``GpuMaskBackend.bubble_filter`` (``mit_bubble_filter``) up to a stream synchronise, and
   once more with the download of its result, and between HIP events over 10 back-to-back calls;
2. the OCR crop test on one 70-line chunk u8 [70, 48, wp, 3]: the host leg is the ``reject`` loop of ``textline.rectified_chunks``
   (download the chunk, ``textline.is_ignore`` per crop, zero the rejected rows one by one), the device leg is
   ``textline.bubble_crop_flags`` (``mit_bubble_crop_flags``).

Bytes are compared on every repeat.  One JSON line; ``--out`` also writes it to a file."""
import argparse, json, os, statistics, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from manga_image_translator_amd import mask_refinement as MR, synth, textline as TL

warnings.simplefilter("ignore", RuntimeWarning)
ap = argparse.ArgumentParser()
ap.add_argument("--level", type=int, default=10, help="ignore_bubble")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")


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


# ---- 1. the mask stage ----
H, W = 2048, 1456
page, quads, mask = synth.synth_page(7, H, W, n_boxes=32, disjoint=True)
for q in quads[::4]:                                   # every fourth bubble carries colour: its contour goes
    x, y = int(q[0, 0]), int(q[0, 1])
    page[y + 2:y + 6, x + 2:x + 8] = (255, 0, 0)
be = MR.GpuMaskBackend(dev)
page_dev, mask_dev = torch.from_numpy(page).to(dev), torch.from_numpy(mask).to(dev)
times = {"host": [], "device": [], "device_with_download": []}
same = True
for it in range(a.warmup + a.repeats):
    rec = it >= a.warmup
    want = timed(lambda: MR.bubble_filter(mask_dev.cpu().numpy(), page, a.level), times["host"], rec)
    got = timed(lambda: be.bubble_filter(mask_dev, page_dev, a.level), times["device"], rec)
    got_host = timed(lambda: be.bubble_filter(mask_dev, page_dev, a.level).cpu().numpy(), times["device_with_download"], rec)
    same = same and np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_host, want)
# the device stage between HIP events, 10 back-to-back calls per pair (what the stream spends, Python's launch cadence aside)
ev = []
for _ in range(20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        be.bubble_filter(mask_dev, page_dev, a.level)
    e1.record()
    e1.synchronize()
    ev.append(e0.elapsed_time(e1) / 10 / 1e3)
from scipy import ndimage as nd
k = int(max(H, W) * 0.025)
labels, n = nd.label(nd.binary_fill_holes(MR.dilate(mask, np.ones((k, k), np.uint8)) > 0), structure=np.ones((3, 3)))
kept = int((np.asarray(nd.maximum(want, labels, index=np.arange(1, n + 1))) > 0).sum())
res = {"mask_stage": {"page": [H, W], "lines": len(quads), "ignore_bubble": a.level, "k": k, "contours": n, "erased": n - kept, "kept": kept,
                      "host_numpy_download_included": spread(times["host"]), "device": spread(times["device"]),
                      "device_with_download": spread(times["device_with_download"]),
                      "device_between_events_10_calls_per_pair": spread(ev),
                      "workspace_bytes": int(be._bubble_ws.numel()), "bytes_identical_every_repeat": bool(same)}}

# ---- 2. the crop test ----
n_lines, h = 70, 48
rng = np.random.default_rng(11)
widths = sorted(int(v) for v in rng.integers(40, 600, n_lines))
wp = max(widths) + 7 + 128                              # the 48px_ctc model's padding
region = np.zeros((n_lines, h, wp, 3), np.uint8)
for j, w in enumerate(widths):                          # bright writing on dark (kept), noise (rejected), a coloured bubble (rejected)
    crop = np.full((h, w, 3), 25, np.uint8)
    crop[8:40:4, 6:w - 6] = 240
    if j % 3 == 1:
        crop = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif j % 3 == 2:
        crop[10:14, 10:14] = (0, 0, 255)
    region[j, :, :w] = crop
region_dev = torch.from_numpy(region).to(dev)
rule = lambda crop: TL.is_ignore(crop, a.level)


def host_leg(chunk):
    host = chunk.cpu().numpy()
    for j, w_line in enumerate(widths):
        if rule(host[j, :, :w_line]):
            chunk[j] = 0
    return chunk


times = {"host": [], "device": []}
same, rejected = True, 0
for it in range(a.warmup + a.repeats):
    rec = it >= a.warmup
    c0, c1 = region_dev.clone(), region_dev.clone()
    want = timed(lambda: host_leg(c0), times["host"], rec)
    flags = timed(lambda: TL.bubble_crop_flags(c1, widths, a.level), times["device"], rec)
    same = same and torch.equal(c0, c1)
    rejected = int(flags.sum())
    same = same and rejected == sum(int(not want[j].any()) for j in range(n_lines))
ev = []
for _ in range(20):
    chunks = [region_dev.clone() for _ in range(10)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for c in chunks:
        TL.bubble_crop_flags(c, widths, a.level)
    e1.record()
    e1.synchronize()
    ev.append(e0.elapsed_time(e1) / 10 / 1e3)
res["crop_test"] = {"chunk": [n_lines, h, wp, 3], "ignore_bubble": a.level, "rejected": rejected, "kept": n_lines - rejected,
                    "host_reject_loop": spread(times["host"]), "device": spread(times["device"]),
                    "device_between_events_10_calls_per_pair": spread(ev), "bytes_identical_every_repeat": bool(same)}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
