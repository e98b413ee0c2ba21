"""32px OCR timing (the reference's ``Ocr.ocr32px``; not the contract bench): the 32 text lines of the synthetic 2048 x 1456 page
recognised by ``Ocr32Engine`` and, in the same process, by ``Ocr48Engine`` (same lines, 32 steps, synthetic weights, dictionary of
pipeline.DICT_SIZE entries) — ms per page for encode (rectification + backbone + encoder + memory K/V) and decode (the native beam
search) separately, from HIP events after a warm-up, with the steps run and the kernel launches of one decode step.  Prints one JSON line.

    python scripts/bench_ocr32.py [--warmup 2] [--iters 5] [--steps 32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from manga_image_translator_amd import ocr32, ocr32_schema, ocr48, ocr_schema, ops, pipeline, synth, textline as TL  # noqa: E402

# kernel launches of one decode step, from the loops of csrc/ocr32_decoder.hip and csrc/ocr_decoder.hip (few-row form with its fusions):
# 32px: 2 layers x (qkv, self-attention, out, norm1, q2, cross-attention, out2, norm2, ff1, ff2, norm3) + pred1 + pred + top-5 + beam
LAUNCHES_32 = 2 * 11 + 4
LAUNCHES_48 = 40


def events(fn, iters):
    """Mean milliseconds of fn() from HIP events around ``iters`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ocr32 needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    D, T = pipeline.DICT_SIZE, args.steps
    page_np, quads_np, _ = synth.synth_page(0, 2048, 1456, n_boxes=32)
    page = torch.from_numpy(page_np).to(dev)[None]
    quads = [TL.Quadrilateral(q) for q in quads_np]
    dirs = [q.direction for q in quads]

    e32 = ocr32.Ocr32Engine(synth.synth_state_dict(ocr32_schema.ocr32_schema(D)), D, device=dev)
    rec = TL.warp_plans(quads, dirs, 2048, 1456, 32)
    widths = np.where(rec["vertical"] != 0, rec["dh"], rec["dw"]).tolist()
    plan32 = TL.chunk_plan(widths)
    enc32 = [None]

    def encode32():
        enc32[0] = [e32.encode(TL.rectify(page, rec[idx], ocr32.TEXT_HEIGHT, wp), ws) for idx, ws, wp in plan32]

    out32 = [None]

    def decode32():
        out32[0] = e32.decode_chunks(enc32[0], T)

    e48 = ocr48.Ocr48Engine(synth.synth_state_dict(ocr_schema.ocr48_schema(D)), D, device=dev)
    plan48 = e48.upload_plan(e48.plan_pages([quads], 2048, 1456, [dirs]))
    mem48 = e48.alloc_memory(len(plan48["order"]), plan48["Lmax"])

    def encode48():
        e48.encode_planned(page, plan48, list(range(len(plan48["chunks"]))), *mem48)

    out48 = [None]

    def decode48():
        out48[0] = e48.decode(mem48[0], mem48[1], plan48["klen_dev"], T, suppress_eos=True)

    for _ in range(args.warmup):
        encode32(), decode32(), encode48(), decode48()
    res = {"metric": "ocr32_ms_per_page", "lines": len(quads), "steps": T, "dict": D, "gemm_mode": ops.split_mode(),
           "crop_widths_32px": [min(widths), max(widths)]}
    # the two engines alternate inside the timed window, so a drift of the machine lands on both
    t = {k: 0.0 for k in ("e32", "d32", "e48", "d48")}
    for _ in range(args.iters):
        t["e32"] += events(encode32, 1)
        t["d32"] += events(decode32, 1)
        t["e48"] += events(encode48, 1)
        t["d48"] += events(decode48, 1)
    n = args.iters
    res.update(ocr32_encode_ms=round(t["e32"] / n, 3), ocr32_decode_ms=round(t["d32"] / n, 3), ocr32_steps_run=int(out32[0]["steps_run"]),
               ocr32_decode_ms_per_step=round(t["d32"] / n / int(out32[0]["steps_run"]), 4), ocr32_launches_per_step=LAUNCHES_32,
               ocr48_encode_ms=round(t["e48"] / n, 3), ocr48_decode_ms=round(t["d48"] / n, 3), ocr48_steps_run=int(out48[0]["steps_run"]),
               ocr48_decode_ms_per_step=round(t["d48"] / n / int(out48[0]["steps_run"]), 4), ocr48_launches_per_step=LAUNCHES_48,
               ocr32_lengths=sorted(set(out32[0]["length"].cpu().tolist())), max_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
