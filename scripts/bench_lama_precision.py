"""LaMa stage alone in its two precisions: fp32 (GEMM mode 6, the default) and the opt-in bf16 (``LamaEngine.forward(precision="bf16")``).

Two workloads, the ones bench.py's stage times use: ``lama_mpe`` (9 blocks + MPE) on 16 resident 2048 x 1456 pages, and ``lama_large``
(18 blocks) on one 512 x 512 page (``--large-pages`` of them).  Per workload: warm-up of both precisions, then ``--rounds`` rounds that
alternate fp32 and bf16 calls in one process, device events around each call (median, min, max ms per page), a sha256 of each leg's
output bytes, the accuracy of the bf16 page against the fp32 page (uint8 level histogram inside the mask), and one HIP-event probe
pass per precision (mit_prof_*) for the time per tile — the p1 tiles next to their p6 twins.  One JSON line; ``--out`` also writes it.

A revision whose ``forward`` has no ``precision`` argument runs the fp32 leg alone, so the same file times the parent commit: its fp32
ms/page and output checksum are the proof that nothing existing got slower or different.  ``--parent-json FILE`` (the ``--out`` of such
a run on the same box) is merged in as ``parent_commit``: the parent's fp32 times and whether its output checksum equals this tree's."""
import argparse, ctypes as C, hashlib, inspect, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from manga_image_translator_amd import lama, lama_schema, lib as L, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--pages", type=int, default=16)
ap.add_argument("--large-pages", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--skip-large", action="store_true")
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="")
ap.add_argument("--parent-json", default="", help="--out of the same script run on the parent commit on the same box")
a = ap.parse_args()
dev = torch.device("cuda:0")
lib = L.load()
ops.set_split_mode(6)


def probe(fn):
    """One instrumented call: {tile: (launches, ms, executed GFLOP)} of its mit_conv_gemm launches."""
    torch.cuda.synchronize()
    L.check(lib.mit_prof_enable(1), "mit_prof_enable")
    fn()
    torch.cuda.synchronize()
    stats, n = (L.MitProfStat * 64)(), C.c_int(0)
    L.check(lib.mit_prof_read(stats, 64, C.byref(n)), "mit_prof_read")
    L.check(lib.mit_prof_enable(0), "mit_prof_enable")
    out = {}
    for i in range(n.value):
        if stats[i].launches:
            out[lib.mit_conv_gemm_config_name(i).decode()] = {"launches": int(stats[i].launches), "ms": round(stats[i].ms, 4),
                                                              "exec_tflops": round(stats[i].exec_flops / (stats[i].ms * 1e9), 1)}
    return out


def workload(name, nb, mpe, B, H, W):
    sd = synth.synth_state_dict(lama_schema.lama_generator_schema(nb))
    mpe_sd = synth.synth_state_dict(lama_schema.lama_mpe_schema()) if mpe else None
    eng = lama.LamaEngine(sd, mpe_sd, n_blocks=nb, device=dev)
    gen = [synth.synth_page(i, H, W, n_boxes=8) for i in range(B)]
    img = torch.from_numpy(np.stack([g[0] for g in gen])).to(dev)
    msk = torch.from_numpy(np.stack([g[2] for g in gen])).to(dev)
    legs = ["fp32"] + (["bf16"] if "precision" in inspect.signature(eng.forward).parameters else [])
    call = {"fp32": lambda: eng.forward(img, msk), "bf16": lambda: eng.forward(img, msk, precision="bf16")}
    outs, ms = {}, {p: [] for p in legs}
    for _ in range(a.warmup):
        for p in legs:
            outs[p] = call[p]()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for p in legs:      # alternating: both legs see the same box state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o = call[p]()
            e1.record()
            torch.cuda.synchronize()
            ms[p].append(e0.elapsed_time(e1) / B)
            assert torch.equal(o, outs[p]), f"{name} {p}: output changed between calls"
    res = {"pages": B, "H": H, "W": W, "n_blocks": nb, "alg_gflop_per_page": round(eng.flops_per_page(H, W) / 1e9, 1)}
    for p in legs:
        med = statistics.median(ms[p])
        res[p] = {"ms_per_page_median": round(med, 3), "ms_per_page_min": round(min(ms[p]), 3), "ms_per_page_max": round(max(ms[p]), 3),
                  "alg_tflops": round(eng.flops_per_page(H, W) / (med * 1e9), 1),
                  "output_sha256": hashlib.sha256(outs[p].cpu().numpy().tobytes()).hexdigest(), "tiles": probe(call[p])}
    if "bf16" in legs:
        res["speedup_bf16_over_fp32"] = round(res["fp32"]["ms_per_page_median"] / res["bf16"]["ms_per_page_median"], 3)
        inside = (msk >= 127).cpu().numpy()
        lv = np.abs(outs["bf16"].cpu().numpy().astype(np.int32) - outs["fp32"].cpu().numpy().astype(np.int32))
        res["u8_levels_bf16_vs_fp32_in_mask"] = np.bincount(lv[inside].ravel(), minlength=3).tolist()
        res["u8_differences_outside_mask"] = int((lv[~inside] != 0).sum())
    eng.release_workspace()
    return res


res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "gemm_mode": ops.split_mode(), "rounds": a.rounds, "warmup": a.warmup,
       "lama_mpe_2048x1456": workload("lama_mpe", 9, True, a.pages, 2048, 1456)}
if not a.skip_large:
    res["lama_large_512x512"] = workload("lama_large", 18, False, a.large_pages, 512, 512)
if a.parent_json:
    par = json.load(open(a.parent_json))
    res["parent_commit"] = {k: {"fp32_ms_per_page_median": par[k]["fp32"]["ms_per_page_median"], "fp32_ms_per_page_min": par[k]["fp32"]["ms_per_page_min"],
                                "fp32_ms_per_page_max": par[k]["fp32"]["ms_per_page_max"], "fp32_output_sha256": par[k]["fp32"]["output_sha256"],
                                "fp32_output_equal": par[k]["fp32"]["output_sha256"] == res[k]["fp32"]["output_sha256"]}
                            for k in ("lama_mpe_2048x1456", "lama_large_512x512") if k in par and k in res}
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
