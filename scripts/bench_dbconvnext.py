"""The dbconvnext detector (DBNet on ConvNeXt) on the GPU: its one new hot kernel against the two launches it replaces, and the engine.

1. ``mit_dwconv7_ln_nhwc`` against ``mit_dwconv_nhwc`` + ``mit_layernorm_rows`` for each backbone width at the stage's extent for a
   2048 x 2048 network input (C = 128 at 512^2, 256 at 256^2, 512 at 128^2, 1024 at 64^2): warm-up of both forms, then ``--rounds`` rounds
   that alternate them in one process, device events round ``--reps`` back-to-back launches of a form (median, min, max us per launch),
   the achieved share of the 8 TB/s HBM peak over the algorithmic bytes (activation read once, written once; the two-launch form moves
   twice that) and the run-to-run spread of each form (max - min over its rounds, relative to its median).  A width is ``fused_wins``
   when the one-pass median is below the two-launch median by more than the larger of the two spreads.
2. The engine at 2048 x 2048, B = 1 and B = 4: ms per page (same alternation, against the ``default`` detector's engine at the same
   input for scale) and a per-layer-class breakdown from one extra pass with device events round every layer call.

One JSON line; ``--out`` also writes it (profiles/<tag>_dbconvnext.json)."""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from manga_image_translator_amd import dbconvnext, dbconvnext_schema, dbnet, dbnet_schema, lib as L, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=2048)
ap.add_argument("--batches", default="1,4")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=20, help="back-to-back kernel launches inside one timed window")
ap.add_argument("--skip-engine", action="store_true")
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_dbconvnext: no GPU visible (nothing is measured on a CPU)")
dev = torch.device("cuda:0")
lib = L.load()
ops.set_split_mode(6)
HBM_PEAK = 8.0e12  # bytes / s, MI355X specification
EPS = dbconvnext_schema.LN_EPS


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(ms):
    med = statistics.median(ms)
    return {"median": med, "min": min(ms), "max": max(ms), "spread_rel": (max(ms) - min(ms)) / med}


def kernel_ab(Cc, side, B=1):
    st = C.c_void_p(ops.current_stream())
    g = torch.Generator().manual_seed(Cc)
    x = torch.randn(B, side, side, Cc, generator=g).to(dev)
    w = (torch.randn(49, Cc, generator=g) / 7).to(dev)
    bdw, gam, bet, one = (torch.randn(Cc, generator=g) * 0.05).to(dev), (torch.rand(Cc, generator=g) + 0.5).to(dev), (torch.randn(Cc, generator=g) * 0.1).to(dev), torch.ones(Cc, device=dev)
    mid, o1, o2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)

    def fused():
        L.check(lib.mit_dwconv7_ln_nhwc(x.data_ptr(), Cc, w.data_ptr(), bdw.data_ptr(), gam.data_ptr(), bet.data_ptr(), EPS, o1.data_ptr(), Cc, B, side, side, Cc, st), "mit_dwconv7_ln_nhwc")

    def two():
        L.check(lib.mit_dwconv_nhwc(x.data_ptr(), w.data_ptr(), one.data_ptr(), bdw.data_ptr(), mid.data_ptr(), B, side, side, Cc, 7, st), "mit_dwconv_nhwc")
        L.check(lib.mit_layernorm_rows(mid.data_ptr(), Cc, gam.data_ptr(), bet.data_ptr(), o2.data_ptr(), Cc, B * side * side, Cc, EPS, st), "mit_layernorm_rows")

    legs = {"fused": fused, "two_launch": two}
    for _ in range(a.warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, f in legs.items():   # alternating: both forms see the same box state
            ms[k].append(timed(f, a.reps))
    alg_bytes = 8.0 * B * side * side * Cc
    res = {"C": Cc, "B": B, "H": side, "W": side, "alg_MB": round(alg_bytes / 1e6, 2), "max_abs_diff": float((o1 - o2).abs().max())}
    for k in legs:
        s = summary(ms[k])
        res[k] = {"us_median": round(s["median"] * 1e3, 2), "us_min": round(s["min"] * 1e3, 2), "us_max": round(s["max"] * 1e3, 2),
                  "spread_rel": round(s["spread_rel"], 4), "hbm_share_of_peak_alg_bytes": round(alg_bytes / (s["median"] * 1e-3) / HBM_PEAK, 4)}
    spread = max(res["fused"]["spread_rel"], res["two_launch"]["spread_rel"])
    res["fused_over_two_launch"] = round(res["fused"]["us_median"] / res["two_launch"]["us_median"], 4)
    res["fused_wins"] = bool(res["fused_over_two_launch"] < 1.0 - spread)
    res["library_uses_fused"] = bool(lib.mit_dwconv7_ln_supported(Cc))
    return res


class Clock:
    """Device events round every call of the wrapped layers; ``read()`` sums them per class after one synchronise."""

    def __init__(self):
        self.ev = []

    def wrap(self, fn, cls):
        def timed_call(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            self.ev.append((cls, e0, e1))
            return r
        timed_call.Cout = getattr(fn, "Cout", None)   # the engine sizes a buffer by its mask convolutions' Cout
        return timed_call

    def read(self):
        torch.cuda.synchronize()
        out = {}
        for cls, e0, e1 in self.ev:
            out[cls] = out.get(cls, 0.0) + e0.elapsed_time(e1)
        self.ev = []
        return out


def breakdown(eng, pages):
    """ms per layer class of one forward (events round each call serialise nothing — one stream — but add their own cost, so the classes
    are read as shares; the ms per page above come from untouched calls)."""
    ck = Clock()
    saved = []

    def swap(obj, name, cls):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, ck.wrap(getattr(obj, name), cls))

    swap(eng, "_dwln", "dwconv_ln")
    swap(eng, "stem", "stem_down_convs")
    swap(eng, "stem_norm", "layernorm")
    for stg in eng.stages:
        if stg.down is not None:
            swap(stg, "down", "stem_down_convs")
            swap(stg, "norm", "layernorm")
        for blk in stg.blocks:
            swap(blk.mlp, "fc1", "pw_gemms")
            swap(blk.mlp, "fc2", "pw_gemms")
    for ub in eng.ups:
        swap(ub, "dw", "dense_7x7")
        swap(ub, "norm", "layernorm")
        swap(ub.mlp, "fc1", "up_block_pw_shortcut_convT")
        swap(ub.mlp, "fc2", "up_block_pw_shortcut_convT")
        swap(ub, "shortcut", "up_block_pw_shortcut_convT")
        swap(ub, "up", "up_block_pw_shortcut_convT")
    heads = eng.binarize, eng.thresh, eng.mask_convs
    eng.binarize = tuple(ck.wrap(f, "heads") for f in eng.binarize)
    eng.thresh = tuple(ck.wrap(f, "heads") for f in eng.thresh)
    eng.mask_convs = [ck.wrap(f, "heads") for f in eng.mask_convs]
    swap(eng, "mask_out", "heads")
    total = timed(lambda: eng.forward(pages))
    cls = ck.read()
    for obj, name, val in saved:
        setattr(obj, name, val)
    eng.binarize, eng.thresh, eng.mask_convs = heads
    B = pages.shape[0]
    return {"ms_per_page_with_events": round(total / B, 3), "ms_per_page_by_class": {k: round(v / B, 3) for k, v in sorted(cls.items(), key=lambda kv: -kv[1])}}


def engines():
    S = a.size
    res = {}
    conv = dbconvnext.DbconvnextEngine(synth.synth_state_dict(dbconvnext_schema.dbnet_convnext_schema()), device=dev)
    dflt = dbnet.DbnetEngine(synth.synth_state_dict(dbnet_schema.text_detection_schema(), gain=1.2), device=dev)
    for B in [int(b) for b in a.batches.split(",")]:
        pages = torch.from_numpy(np.stack([synth.synth_page(i, S, S, n_boxes=16)[0] for i in range(B)])).to(dev)
        legs = {"dbconvnext": lambda: conv.forward(pages), "default": lambda: dflt.forward(pages)}
        for _ in range(a.warmup):
            for f in legs.values():
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():
                ms[k].append(timed(f) / B)
        r = {"B": B, "H": S, "W": S}
        for k in legs:
            s = summary(ms[k])
            r[k] = {"ms_per_page_median": round(s["median"], 3), "ms_per_page_min": round(s["min"], 3), "ms_per_page_max": round(s["max"], 3)}
        r["dbconvnext_over_default"] = round(r["dbconvnext"]["ms_per_page_median"] / r["default"]["ms_per_page_median"], 2)
        r["dbconvnext_breakdown"] = breakdown(conv, pages)
        res[f"B{B}"] = r
    res["workspace_GB"] = {"dbconvnext": round(conv._ws.nbytes() / 1e9, 2), "default": round(dflt._ws.nbytes() / 1e9, 2)}
    return res


res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "gemm_mode": ops.split_mode(), "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
       "hbm_peak_TBps": HBM_PEAK / 1e12,
       "dwconv7_ln": [kernel_ab(c, a.size // 4 >> i) for i, c in enumerate(dbconvnext_schema.DIMS)]}
if not a.skip_engine:
    res["engine"] = engines()
line = json.dumps(res)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(line + "\n")
print(line)
