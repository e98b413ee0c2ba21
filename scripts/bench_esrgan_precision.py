"""The ESRGAN upscaler in its two precisions: fp32 (GEMM mode 6, the default) and the opt-in bf16 (``EsrganEngine.forward(precision="bf16")``).

1. ``forward`` on one synthetic 2048 x 1440 page (the low-resolution size of BASELINE config 5), 23 blocks: warm-up of both precisions,
   then ``--rounds`` rounds that alternate fp32 and bf16 calls in one process, device events around each call: median, min and max ms.
   The bf16 leg must beat the fp32 leg by more than the run-to-run range of either (``bf16_faster_beyond_range``).
2. Per dense-block layer shape at that size (Cin = 64 .. 160 with N = 32, Cin = 192 with N = 64): ``mit_rdb_conv3x3_bf16`` on
   bf16-resident activations against the same layer on ``mit_conv_gemm`` with ``nprod = 1`` (fp32 activations, rounded while staged),
   ``--layer-reps`` launches each, alternated: median ms, executed bf16 TFLOP/s, the fraction of the 2.5 PFLOP/s peak, and the bytes
   each kernel REQUESTS from the memory system over the algorithmic bytes of the layer (input once + output once + weights once, in
   the kernel's own operand types).  The requested bytes follow from the kernels' structure (rdb: the 10 x 34 halo of an 8 x 32 tile
   and the weights once per workgroup; conv_gemm: every tap gathers its fp32 activations again); HBM bytes by counters are not
   measured here.
One JSON line; ``--out`` also writes it."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from manga_image_translator_amd import esrgan, esrgan_schema, lib as L, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--height", type=int, default=2048)
ap.add_argument("--width", type=int, default=1440)
ap.add_argument("--blocks", type=int, default=23)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layer-reps", type=int, default=9)
ap.add_argument("--skip-forward", action="store_true")
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
L.load()
ops.set_split_mode(6)
H, W = a.height, a.width
PEAK_BF16 = 2.5e15


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def forward_legs():
    sd = synth.synth_state_dict(esrgan_schema.rrdbnet_schema(a.blocks))
    eng = esrgan.EsrganEngine(sd, nb=a.blocks, device=dev)
    page = torch.from_numpy(synth.synth_page(3, H, W, n_boxes=8)[0][None]).to(dev)
    call = {"fp32": lambda: eng.forward(page), "bf16": lambda: eng.forward(page, precision="bf16")}
    outs, ms = {}, {"fp32": [], "bf16": []}
    for _ in range(a.warmup):
        for p in call:
            outs[p] = call[p]()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for p in call:          # alternating: both legs see the same box state
            t, o = timed(call[p])
            ms[p].append(t)
            assert torch.equal(o, outs[p]), f"{p}: output changed between calls"
    res = {"blocks": a.blocks, "alg_tflop_per_page": round(eng.flops_per_input_pixel() * H * W / 1e12, 1)}
    for p in call:
        res[p] = stats(ms[p])
        res[p]["alg_tflops"] = round(eng.flops_per_input_pixel() * H * W / (res[p]["ms_median"] * 1e9), 1)
    rng = max(res[p]["ms_max"] - res[p]["ms_min"] for p in call)
    res["speedup_bf16_over_fp32"] = round(res["fp32"]["ms_median"] / res["bf16"]["ms_median"], 3)
    res["run_to_run_range_ms"] = round(rng, 3)
    res["bf16_faster_beyond_range"] = bool(res["fp32"]["ms_median"] - res["bf16"]["ms_median"] > rng)
    lv = np.abs(outs["bf16"].cpu().numpy().astype(np.int16) - outs["fp32"].cpu().numpy().astype(np.int16))
    res["u8_levels_bf16_vs_fp32"] = np.bincount(lv.ravel(), minlength=3).tolist()
    eng.release_workspace()
    del eng
    torch.cuda.empty_cache()
    return res


def layer_legs():
    g = torch.Generator().manual_seed(1)
    cat32 = torch.randn(1, H, W, 192, device=dev)
    cat16 = cat32.to(torch.bfloat16)
    cat32 = cat16.float()                               # the same operand values on both sides
    out32 = torch.empty(1, H, W, 64, device=dev)
    out16 = torch.empty(1, H, W, 64, dtype=torch.bfloat16, device=dev)
    post = torch.randn(1, H, W, 64, device=dev)
    res = {}
    th, tw = L.MIT_RDB_TILE_H, L.MIT_RDB_TILE_W
    tiles = -(-H // th) * -(-W // tw)
    for Cin, N in ((64, 32), (96, 32), (128, 32), (160, 32), (192, 64)):
        w = torch.randn(N, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
        b = torch.randn(N, generator=g)
        last = N == 64
        kw = dict(out_scale=torch.full((N,), 0.2)) if last else dict(act=ops.ACT_LEAKY, alpha=0.2)
        rdb = ops.RdbConv3x3(w, b, device=dev, **kw)
        cg = ops.Conv2d(w, b, padding=1, device=dev, **kw)
        o32, o16 = out32[..., :N], out16[..., :N]
        if last:   # conv5: fp32 master and bf16 copy, post residual
            call = {"rdb_bf16": lambda: rdb(cat16[..., :Cin], post=post, out_f32=o32, out_bf16=o16),
                    "conv_gemm_p1": lambda: cg(cat32[..., :Cin], out=o32, post=post, nprod=1)}
        else:      # conv1..4: into the next slice of the block's own buffer
            call = {"rdb_bf16": lambda: rdb(cat16[..., :Cin], out_bf16=cat16[..., Cin:Cin + N]),
                    "conv_gemm_p1": lambda: cg(cat32[..., :Cin], out=cat32[..., Cin:Cin + N], nprod=1)}
        for p in call:
            call[p]()
        torch.cuda.synchronize()
        ms = {p: [] for p in call}
        for _ in range(a.layer_reps):
            for p in call:
                ms[p].append(timed(call[p])[0])
        flop = 2.0 * 9 * Cin * N * H * W
        px = float(H * W)
        alg = {"rdb_bf16": px * (2 * Cin + (2 * N if not last else 2 * N + 4 * N + 4 * N)) + 18.0 * Cin * N,
               "conv_gemm_p1": px * (4 * Cin + 4 * N + (4 * N if last else 0)) + 36.0 * Cin * N}
        req = {"rdb_bf16": tiles * ((th + 2) * (tw + 2) * 2.0 * Cin + 18.0 * Cin * N) + (alg["rdb_bf16"] - px * 2 * Cin - 18.0 * Cin * N),
               "conv_gemm_p1": px * 9 * 4.0 * Cin + (alg["conv_gemm_p1"] - px * 4 * Cin)}
        r = {}
        for p in call:
            s = stats(ms[p])
            s["exec_tflops"] = round(flop / (s["ms_median"] * 1e9), 1)
            s["fraction_of_bf16_peak"] = round(flop / (s["ms_median"] * 1e-3) / PEAK_BF16, 4)
            s["requested_over_algorithmic_bytes"] = round(req[p] / alg[p], 2)
            s["algorithmic_gbytes"] = round(alg[p] / 1e9, 3)
            r[p] = s
        r["speedup_rdb_over_p1"] = round(r["conv_gemm_p1"]["ms_median"] / r["rdb_bf16"]["ms_median"], 3)
        res[f"cin{Cin}_n{N}"] = r
    return res


res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "gemm_mode": ops.split_mode(), "H": H, "W": W, "rounds": a.rounds,
       "warmup": a.warmup, "layer_reps": a.layer_reps}
if not a.skip_forward:
    res["forward"] = forward_legs()
res["layers"] = layer_legs()
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
