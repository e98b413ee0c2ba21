"""Webtoon strips: the detector's strip branch with the tiling on the host (numpy bands / stitch, host box extraction: what an injected
``boxes_from_maps`` still selects) against the tiling on the device (csrc/rearrange.hip), legs alternated in one process.

1. one synthetic 12000 x 800 strip through ``HipComicTextDetector.infer``: warm-up, then ``--repeats`` alternations, median and spread
   per leg; the two legs' boxes and mask bytes are compared on every repeat;
2. the two kernels alone under HIP events, GB/s over their algorithmic bytes;
3. ``--pages`` strips through ``serve.DenseStages.translate_batch``: the page loop (``batch_size=1``) against one coupled run.

Seeded weights detect nothing, so the maps a trained ctd head would emit replace the network's own AFTER it has run (per square: the
page's ``coupled.synthetic_head_outputs`` cut and shrunk like the page).  One JSON line; ``--out`` also writes it to a file."""
import argparse, asyncio, ctypes as C, json, os, statistics, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from manga_image_translator_amd import coupled, imgproc, lib as L, ops, plugins as P, rearrange as RA, serve, synth

warnings.simplefilter("ignore", RuntimeWarning)
ap = argparse.ArgumentParser()
ap.add_argument("--height", type=int, default=12000)
ap.add_argument("--width", type=int, default=800)
ap.add_argument("--lines", type=int, default=48)
ap.add_argument("--pages", type=int, default=8)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--serve-repeats", type=int, default=10)
ap.add_argument("--kernel-iters", type=int, default=50)
ap.add_argument("--max-seq-length", type=int, default=32)
ap.add_argument("--dict-size", type=int, default=6004)
ap.add_argument("--out", default="")
a = ap.parse_args()
H, W, S = a.height, a.width, 1024
dev = torch.device("cuda:0")
loop = asyncio.new_event_loop()
run = loop.run_until_complete
eng = serve.DenseStages({"dict_size": a.dict_size})
run(eng._load())
det = eng.det
pl = RA.plan(H, W, S)
assert pl is not None
host_resize = lambda x, ds: imgproc.resize_u8_host(x, ds)   # noqa: E731

pages, table = [], {}
for i in range(a.pages):
    page, quads, _ = synth.synth_page(100 + i, H, W, n_boxes=a.lines, disjoint=True)
    prob, mask = coupled.synthetic_head_outputs(page, quads, (H, W))
    head = np.stack([(prob * 255).astype(np.uint8), mask, np.zeros_like(mask)], axis=-1)
    sq = RA.squares(page, pl, S, host_resize)[0]
    hd = RA.squares(head, pl, S, host_resize)[0].astype(np.float32) / np.float32(255)
    for s, h in zip(sq, hd):
        table[int(s.astype(np.int64).sum())] = (torch.from_numpy(h[..., 0].copy()).to(dev), torch.from_numpy(h[..., 1].copy()).to(dev))
    pages.append(page)
plain = det.engine.forward


def fwd(squares_u8, taps=None):   # squares are recognised by their bytes: one page's squares or several pages' arrive in one call
    m8, lines, pad = plain(squares_u8, taps)
    maps = [table[int(s.sum(dtype=torch.int64))] for s in squares_u8]
    lines[:, 0] = torch.stack([m[0] for m in maps])
    det.engine.last_mask_f32 = torch.stack([m[1] for m in maps])
    return m8, lines, pad


det.engine.forward = fwd


def spread(ts):
    return {"median_ms": round(1e3 * statistics.median(ts), 3), "min_ms": round(1e3 * min(ts), 3), "max_ms": round(1e3 * max(ts), 3), "n": len(ts)}


# ---- 1. the plugin on one strip: host leg (an injected extractor selects the host branch) / device leg, alternated ----
legs = {"host": P._native_ctd_boxes, "device": None}
times = {k: [] for k in legs}
same = True
for it in range(a.warmup + a.repeats):
    got = {}
    for name, boxes_fn in legs.items():
        det._boxes = boxes_fn
        torch.cuda.synchronize()
        t = time.perf_counter()
        got[name] = run(det.infer(pages[0], S, 0.5, 0.7, 2.3))
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[name].append(time.perf_counter() - t)
    det._boxes = None
    (ht, hm, _), (dt, dm, _) = got["host"], got["device"]
    same = same and len(ht) == len(dt) and all(np.array_equal(x.pts, y.pts) for x, y in zip(ht, dt)) and np.array_equal(hm, dm)
res = {"strip": [H, W], "squares": pl.p_num, "bands": pl.ph_num, "lines_detected": len(got["device"][0]),
       "infer_host": spread(times["host"]), "infer_device": spread(times["device"]), "legs_identical": bool(same)}


# ---- 2. the two kernels alone ----
def events(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


lib = L.load()
st = C.c_void_p(ops.current_stream())
page_dev = torch.from_numpy(pages[0]).to(dev)
sq_out = torch.empty(pl.p_num, pl.patch, pl.patch, 3, dtype=torch.uint8, device=dev)
ms = events(lambda: L.check(lib.mit_rearrange_squares(page_dev.data_ptr(), H, W, int(pl.transpose), pl.w, pl.pw_num, pl.ph_num, pl.ph_step,
                                                      pl.p_num, sq_out.data_ptr(), st)), a.kernel_iters)
nbytes = 2 * sq_out.numel()
kern = {"rearrange_squares": {"ms": round(ms[0], 4), "min_ms": round(ms[1], 4), "max_ms": round(ms[2], 4), "bytes": nbytes,
                              "GBps": round(nbytes / ms[0] / 1e6, 1)}}
step, pw, hh, starts = RA.stitch_geometry(pl, S)
starts_dev = torch.tensor(starts, dtype=torch.int32).to(dev)
rows_read = sum(min(t + S, hh) - t for t in starts)
for name, ch, u8 in (("rearrange_stitch_lines", 2, 0), ("rearrange_stitch_mask_u8", 1, 1)):
    src = torch.rand(pl.p_num, ch, S, S, device=dev)
    out = torch.empty(1, ch, hh, pw, device=dev)
    out8 = torch.empty(1, ch, hh, pw, dtype=torch.uint8, device=dev)
    sn, sc, sy, sx = src.stride()
    ms = events(lambda: L.check(lib.mit_rearrange_stitch(src.data_ptr(), pl.p_num, ch, S, sn, sc, sy, sx, int(pl.transpose), pl.pw_num, pl.ph_num,
                                                         step, pw, hh, starts_dev.data_ptr(), out.data_ptr(), out8.data_ptr(), u8, st)),
                a.kernel_iters)
    nbytes = ch * pw * (4 * rows_read + (4 + u8) * hh)
    kern[name] = {"ms": round(ms[0], 4), "min_ms": round(ms[1], 4), "max_ms": round(ms[2], 4), "bytes": nbytes, "GBps": round(nbytes / ms[0] / 1e6, 1)}
res["kernels"] = kern

# ---- 3. a batch of strips through the serving engine: the page loop / one coupled run, alternated ----
if a.pages > 1 and a.serve_repeats > 0:
    cfg = {"ocr": {"max_seq_length": a.max_seq_length, "suppress_eos": True, "prob": 0.0}, "inpainter": {"inpainting_size": 2048}}
    stimes = {"loop": [], "coupled": []}
    outs = {}
    for it in range(1 + a.serve_repeats):
        for name, bs in (("loop", 1), ("coupled", a.pages)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            outs[name] = run(eng.translate_batch(pages, cfg, batch_size=bs))
            torch.cuda.synchronize()
            if it >= 1:
                stimes[name].append(time.perf_counter() - t)
            if name == "coupled":
                plan = eng.last_batch_plan
    res["serve"] = {"pages": a.pages, "loop": spread(stimes["loop"]), "coupled": spread(stimes["coupled"]), "coupled_plan": [[i, w] for i, w in plan],
                    "pages_per_s_loop": round(a.pages / statistics.median(stimes["loop"]), 2),
                    "pages_per_s_coupled": round(a.pages / statistics.median(stimes["coupled"]), 2),
                    "lines_read": [sum(len(r["textlines"]) for r in outs[k]) for k in ("loop", "coupled")],
                    "masks_identical": bool(all(np.array_equal(x["mask"], y["mask"]) for x, y in zip(outs["loop"], outs["coupled"]))),
                    "inpainted_identical": bool(all(np.array_equal(x["inpainted"], y["inpainted"]) for x, y in zip(outs["loop"], outs["coupled"])))}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
