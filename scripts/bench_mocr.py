#!/usr/bin/env python3
"""Time the manga-ocr recogniser (``--ocr mocr``) on the HIP engine, per phase, on seeded weights.

    python scripts/bench_mocr.py [--config DIR_OR_JSON] [--lines 1 16] [--repeats 10] [--warmup 2] [--out profiles/mocr_bench.json]

Sizes and generation parameters come from ``--config`` (a model directory or a config.json); without it the sizes are the ones the
published manga-ocr-base checkpoint is REMEMBERED to have (224², patch 16, 768 / 12 heads / 12 + 12 layers, V = 6144, 4 beams,
no_repeat_ngram_size 3, length_penalty 2, early_stopping, max_length 300) and the result is marked ``"sizes": "assumed"``: nobody has
verified them against the checkpoint's files.  Reports, per number of lines: pre-processing, encoder and decode milliseconds (median and
range over the repeats), steps run, and the kernel launches of a step as COMPUTED from the decoder loop's structure (7 + 12 per layer; the
trace copies of tests and the done-counter read every fourth step are not in it).  Nothing here counts launches at run time.  When ``transformers`` imports, the
same weights run through ``VisionEncoderDecoderModel.generate`` in fp32 on the same device, alternating with the engine in the same
process, and the ratio is reported — the reference's own path on this hardware; otherwise the output says that no baseline was measured.
NOT measured here: the real checkpoint's weights, its real config.json, ``post_process`` against the ``manga_ocr`` package."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from manga_image_translator_amd import mocr, mocr_schema as S  # noqa: E402
from manga_image_translator_amd.synth import synth_state_dict  # noqa: E402


def assumed():
    cfg = S.tiny_config_dict(image_size=224, patch_size=16, hidden=768, heads=12, enc_layers=12, dec_layers=12, inter=3072, vocab=6144, max_pos=512)
    gen = S.GenerationParams(max_length=300, num_beams=4, no_repeat_ngram_size=3, length_penalty=2.0, early_stopping=True, eos_token_id=3,
                             pad_token_id=0, decoder_start_token_id=2)
    return cfg, gen, "assumed"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config")
    ap.add_argument("--lines", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hf-repeats", type=int, default=3)
    ap.add_argument("--eos-bias", type=float, default=0.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.config:
        d = a.config if os.path.isdir(a.config) else None
        if d:
            cfg, _, gen = S.load_model_dir(d, max_length=300)
        else:
            with open(a.config) as f:
                cfg = json.load(f)
            gen = S.generation_from_dicts({k: v for k, v in cfg.items() if k in S.GenerationParams.__dataclass_fields__}, max_length=300)
        sizes = "from " + a.config
    else:
        cfg, gen, sizes = assumed()
    c = S.config_from_dict(cfg)
    sd = synth_state_dict(S.mocr_schema(c), seed=0)
    b = sd["decoder.cls.predictions.bias"].clone()
    b[gen.eos_token_id] += a.eos_bias
    sd["decoder.cls.predictions.bias"] = sd["decoder.cls.predictions.decoder.bias"] = b
    dev = torch.device("cuda:0")
    eng = mocr.MocrEngine(sd, cfg, gen, device=dev)
    hf = None
    try:
        from transformers import GenerationConfig, VisionEncoderDecoderConfig, VisionEncoderDecoderModel

        hc = VisionEncoderDecoderConfig(**dict(cfg, decoder=dict(cfg["decoder"], tie_word_embeddings=False)))
        hc.tie_word_embeddings = False
        hf = VisionEncoderDecoderModel(hc).float().eval()
        hf.load_state_dict(sd, strict=True)
        hf = hf.to(dev)
        hg = GenerationConfig(max_length=gen.max_length, num_beams=gen.num_beams, no_repeat_ngram_size=gen.no_repeat_ngram_size,
                              length_penalty=gen.length_penalty, early_stopping=gen.early_stopping, eos_token_id=gen.eos_token_id,
                              pad_token_id=gen.pad_token_id, decoder_start_token_id=gen.decoder_start_token_id, do_sample=False)
    except ImportError:
        pass
    # computed, not counted: embed+LN | per layer 7 Linears, 2 attentions, 3 LayerNorms | LM head (3) | log-softmax/top-k, bookkeeping
    launches = 1 + 12 * c.dec_layers + 3 + 2
    res = {"sizes": sizes, "config": cfg, "generation": gen.__dict__, "device": torch.cuda.get_device_name(0), "kernel_launches_per_step_computed": launches,
           "repeats": a.repeats, "warmup": a.warmup, "runs": []}
    rng = np.random.default_rng(0)
    for N in a.lines:
        crops = [torch.from_numpy(rng.integers(0, 256, size=(40 + 7 * (i % 5), 120 + 31 * (i % 7), 3), dtype=np.uint8)).to(dev) for i in range(N)]
        pre, enc, dec, hf_ms, steps, same = [], [], [], [], None, None
        with torch.no_grad():
            for it in range(a.warmup + a.repeats):
                t0, imgs = timed(lambda: eng.preprocess(crops))
                t1, mem = timed(lambda: eng.encode(imgs))
                t2, out = timed(lambda: eng.decode(*mem))
                if it >= a.warmup:
                    pre.append(t0), enc.append(t1), dec.append(t2)
                steps = out["steps_run"]
                if hf is not None and it < 1 + a.hf_repeats:   # alternate in the same process; the first HuggingFace run is its warm-up
                    pv = ((imgs.float() * (1.0 / 255.0) - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
                    t3, seq = timed(lambda: hf.generate(pv, generation_config=hg))
                    if it >= 1:
                        hf_ms.append(t3)
                    n = min(seq.shape[1], out["tokens"].shape[1])
                    same = float((seq[:, :n].cpu() == out["tokens"][:, :n].cpu()).all(1).float().mean())
        run = {"lines": N, "steps_run": steps, "preprocess": stats(pre), "encode": stats(enc), "decode": stats(dec),
               "per_line_ms": {k: statistics.median(v) / N for k, v in (("preprocess", pre), ("encode", enc), ("decode", dec))}}
        ours = statistics.median(enc) + statistics.median(dec)
        if hf_ms:
            run["huggingface_generate_fp32"] = stats(hf_ms)
            run["huggingface_over_engine"] = statistics.median(hf_ms) / ours
            run["lines_with_equal_tokens"] = same
        else:
            run["huggingface_generate_fp32"] = "no baseline was measured (transformers does not import here)"
        res["runs"].append(run)
        print(json.dumps(run))
    res["not_measured"] = ["real checkpoint weights", "the real config.json", "post_process against the manga_ocr package"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
