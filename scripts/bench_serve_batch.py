"""Rate of a batch request through the stand-alone worker's engine, in process (no HTTP): 16 synthetic 2048 x 1456 pages with 32
lines each, ``DenseStages.translate_batch(pages, cfg, batch_size=16)``, 2 warm-up + N timed calls, median and spread.

Seeded weights detect nothing, so the maps a trained detector head would emit for each page replace the network's own AFTER it has run
(``coupled.synthetic_head_outputs``, hung on the detector plugin's ``engine.forward`` the way scripts/prof_coupled_maskref.py does);
every stage downstream then has a page's worth of work.  Without ``--stages`` the script uses only what every revision of
``serve.DenseStages`` has, so the same file measures a revision where ``translate_batch`` loops over ``translate`` and one where it
runs coupled batches.

``--stages config --detector default --inpainter lama_large`` (any supported keys) makes the worker follow the request, and
``--alternate`` times the page loop (``batch_size=1``) and the batch in turns in one process, comparing their pages on every repeat."""
import argparse, asyncio, json, os, statistics, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from manga_image_translator_amd import coupled, ctd as CTD, serve, synth

warnings.simplefilter("ignore", RuntimeWarning)
ap = argparse.ArgumentParser()
ap.add_argument("--pages", type=int, default=16)
ap.add_argument("--lines", type=int, default=32)
ap.add_argument("--batch-size", type=int, default=16)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--max-seq-length", type=int, default=32)
ap.add_argument("--dict-size", type=int, default=6004)
ap.add_argument("--tag", default="")
ap.add_argument("--stages", default=None, help="fixed | config (serve.DenseStages' worker parameter; absent: the worker's default)")
ap.add_argument("--detector", default=None)
ap.add_argument("--ocr", default=None)
ap.add_argument("--inpainter", default=None)
ap.add_argument("--detection-size", type=int, default=2048, help="config mode with a DBNet detector: the request's detection_size")
ap.add_argument("--alternate", action="store_true", help="time batch_size=1 (the page loop) and --batch-size in turns, compare their pages")
ap.add_argument("--out", default="")
a = ap.parse_args()
H, W = 2048, 1456
loop = asyncio.new_event_loop()
cfg = {"ocr": {"max_seq_length": a.max_seq_length, "suppress_eos": True, "prob": 0.0}, "inpainter": {"inpainting_size": 2048}}
for section, key in (("detector", a.detector), ("ocr", a.ocr), ("inpainter", a.inpainter)):
    if key:
        cfg.setdefault(section, {})[section] = key
eng = serve.DenseStages({"dict_size": a.dict_size, **({"stages": a.stages} if a.stages else {})})
keys = eng._select(cfg) if hasattr(eng, "_select") else ("ctd", "48px", "lama_mpe")
dbnet = keys[0] != "ctd"
if dbnet:   # (the stand-in head's shrink is solved for an unclip ratio of 1.5)
    cfg.setdefault("detector", {}).update(detection_size=a.detection_size, unclip_ratio=1.5)
loop.run_until_complete(eng._load())
dev = torch.device("cuda:0")
if dbnet:   # the network's page: the long side at detection_size, zero-padded to a multiple of 256; the mask head works at half of it
    r = a.detection_size / max(H, W)
    th, tw = int(round(H * r)), int(round(W * r))
    nh, nw = th + (256 - th % 256) % 256, tw + (256 - tw % 256) % 256
else:
    _, _, dw, dh = CTD.CtdEngine.letterbox_geometry(H, W)
pages, probs, masks = [], [], []
for i in range(a.pages):
    page, quads, _ = synth.synth_page(i, H, W, n_boxes=a.lines, disjoint=True)
    if dbnet:
        prob, m = np.zeros((nh, nw), np.float32), np.zeros((nh // 2, nw // 2), np.float32)
        prob[:th, :tw] = coupled.synthetic_head_outputs(page, quads, (th, tw))[0]
        m[:th // 2, :tw // 2] = coupled.synthetic_head_outputs(page, quads, (th // 2, tw // 2))[1].astype(np.float32) / np.float32(255)
    else:
        prob, m = coupled.synthetic_head_outputs(page, quads, (CTD.INPUT_SIZE - dh, CTD.INPUT_SIZE - dw))
    pages.append(page), probs.append(prob), masks.append(m)
inj_prob, inj_mask = torch.from_numpy(np.stack(probs)).to(dev), torch.from_numpy(np.stack(masks)).to(dev)
plain = eng.det.engine.forward
cursor = [0]


def fwd(pages_u8, taps=None):   # the request's pages reach the detector in order, one at a time or a batch at a time
    idx = [(cursor[0] + k) % a.pages for k in range(pages_u8.shape[0])]
    cursor[0] = (cursor[0] + pages_u8.shape[0]) % a.pages
    if dbnet:
        db, _ = plain(pages_u8, taps)
        db[:, 0] = inj_prob[idx]
        return db, inj_mask[idx].contiguous()
    mm, lines, pad = plain(pages_u8, taps)
    lines[:, 0] = inj_prob[idx]
    return inj_mask[idx].contiguous(), lines, pad


eng.det.engine.forward = fwd
legs = [("loop", 1), ("batch", a.batch_size)] if a.alternate else [("batch", a.batch_size)]
times, outs, same = {k: [] for k, _ in legs}, {}, True
for it in range(a.warmup + a.calls):
    for name, bs in legs:
        cursor[0] = 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        outs[name] = loop.run_until_complete(eng.translate_batch(pages, cfg, batch_size=bs))
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[name].append(time.perf_counter() - t)
        if name == "batch":
            plan = getattr(eng, "last_batch_plan", None)
    if a.alternate:
        same = same and all(np.array_equal(x[k], y[k]) for x, y in zip(outs["loop"], outs["batch"]) for k in ("mask_raw", "mask", "inpainted")) \
            and all([t["pts"] for t in x["textlines"]] == [t["pts"] for t in y["textlines"]] and [t["text"] for t in x["textlines"]] ==
                    [t["text"] for t in y["textlines"]] for x, y in zip(outs["loop"], outs["batch"]))
out = outs["batch"]
med = statistics.median(times["batch"])
res = {"tag": a.tag, "pages": a.pages, "lines_per_page": a.lines, "batch_size": a.batch_size, "calls": len(times["batch"]),
       "seconds_median": round(med, 4), "seconds_min": round(min(times["batch"]), 4), "seconds_max": round(max(times["batch"]), 4),
       "pages_per_s": round(a.pages / med, 2), "lines_read": sum(len(r["textlines"]) for r in out),
       "mask_coverage": round(float(np.mean([(r["mask"] > 0).mean() for r in out])), 4),
       "pages_batched": getattr(eng, "pages_batched", None), "pages_looped": getattr(eng, "pages_looped", None),
       "coupled_seconds": getattr(eng, "last_coupled_seconds", None)}
if a.stages:
    res.update(stages=eng.stages, stage_keys=list(eng.last_stage_keys), batch_plan=[[i, w] for i, w in plan or []])
if a.alternate:
    lmed = statistics.median(times["loop"])
    res["loop"] = {"seconds_median": round(lmed, 4), "seconds_min": round(min(times["loop"]), 4), "seconds_max": round(max(times["loop"]), 4),
                   "pages_per_s": round(a.pages / lmed, 2), "lines_read": sum(len(r["textlines"]) for r in outs["loop"])}
    res["batch_over_loop"] = round(lmed / med, 3)
    res["pages_identical_every_repeat"] = bool(same)
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
