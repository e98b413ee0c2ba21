"""Rate of a batch request through the stand-alone worker's engine, in process (no HTTP): 16 synthetic 2048 x 1456 pages with 32
lines each, ``DenseStages.translate_batch(pages, cfg, batch_size=16)``, 2 warm-up + N timed calls, median and spread.

Seeded weights detect nothing, so the maps a trained ctd head would emit for each page replace the network's own AFTER it has run
(``coupled.synthetic_head_outputs``, hung on the detector plugin's ``engine.forward`` the way scripts/prof_coupled_maskref.py does);
every stage downstream then has a page's worth of work.  The script uses only what every revision of ``serve.DenseStages`` has, so
the same file measures a revision where ``translate_batch`` loops over ``translate`` and one where it runs coupled batches."""
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
a = ap.parse_args()
H, W = 2048, 1456
loop = asyncio.new_event_loop()
eng = serve.DenseStages({"dict_size": a.dict_size})
loop.run_until_complete(eng._load())
dev = torch.device("cuda:0")
nh, nw, dw, dh = CTD.CtdEngine.letterbox_geometry(H, W)
pages, probs, masks = [], [], []
for i in range(a.pages):
    page, quads, _ = synth.synth_page(i, H, W, n_boxes=a.lines, disjoint=True)
    prob, m = coupled.synthetic_head_outputs(page, quads, (CTD.INPUT_SIZE - dh, CTD.INPUT_SIZE - dw))
    pages.append(page), probs.append(prob), masks.append(m)
inj_prob, inj_mask = torch.from_numpy(np.stack(probs)).to(dev), torch.from_numpy(np.stack(masks)).to(dev)
plain = eng.det.engine.forward
cursor = [0]


def fwd(pages_u8, taps=None):   # the request's pages reach the detector in order, one at a time or a batch at a time
    mm, lines, pad = plain(pages_u8, taps)
    idx = [(cursor[0] + k) % a.pages for k in range(pages_u8.shape[0])]
    cursor[0] = (cursor[0] + pages_u8.shape[0]) % a.pages
    lines[:, 0] = inj_prob[idx]
    return inj_mask[idx].contiguous(), lines, pad


eng.det.engine.forward = fwd
cfg = {"ocr": {"max_seq_length": a.max_seq_length, "suppress_eos": True, "prob": 0.0}, "inpainter": {"inpainting_size": 2048}}
times, out = [], None
for it in range(a.warmup + a.calls):
    cursor[0] = 0
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = loop.run_until_complete(eng.translate_batch(pages, cfg, batch_size=a.batch_size))
    torch.cuda.synchronize()
    if it >= a.warmup:
        times.append(time.perf_counter() - t)
med = statistics.median(times)
res = {"tag": a.tag, "pages": a.pages, "lines_per_page": a.lines, "batch_size": a.batch_size, "calls": len(times),
       "seconds_median": round(med, 4), "seconds_min": round(min(times), 4), "seconds_max": round(max(times), 4),
       "pages_per_s": round(a.pages / med, 2), "lines_read": sum(len(r["textlines"]) for r in out),
       "mask_coverage": round(float(np.mean([(r["mask"] > 0).mean() for r in out])), 4),
       "pages_batched": getattr(eng, "pages_batched", None), "pages_looped": getattr(eng, "pages_looped", None),
       "coupled_seconds": getattr(eng, "last_coupled_seconds", None)}
print(json.dumps(res))
