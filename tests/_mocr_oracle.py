"""Plain-torch restatement of the manga-ocr recogniser (``--ocr mocr``): pre-processing, ViT / DeiT encoder, BERT decoder with
cross-attention and HuggingFace's beam search, in any dtype (the tests use float64).  No ``transformers`` import: the GPU tests use this
file and the GPU box may not have the package; tests/test_mocr_cpu.py checks it against HuggingFace's own modules and ``generate``.

State-dict names are those of ``VisionEncoderDecoderModel.state_dict()`` (manga_image_translator_amd/mocr_schema.py).

Fixture recipe (``make_case``).  Seeded weights alone never end a line: the EOS logit is one of V near-equal draws.  Each case therefore
  * draws the weights from ``mocr_schema`` with the given seed (the vocabulary Linear carries mocr_schema.HEAD_GAIN),
  * adds ``eos_bias`` to ``decoder.cls.predictions.bias[eos]`` (and its tied ``decoder.bias``): with the gain above, +12 ends lines within
    two steps, a negative value never ends them, +6 .. +9 give lines of one batch that end at different steps,
  * optionally scales the word embeddings (``embed_scale``) so that the input token matters more and n-grams repeat.
``CASES`` lists the (seed, eos_bias, embed_scale) triples the GPU tests use and what each one is for; tests/test_mocr_cpu.py::HF_MODELS the two
models every generation setting is run on against HuggingFace.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from manga_image_translator_amd.mocr_schema import GenerationParams, MocrConfig, config_from_dict, mocr_schema, tiny_config_dict
from manga_image_translator_amd.synth import synth_state_dict

EOS, PAD, START = 3, 1, 2


# ---- pre-processing ---------------------------------------------------------------------------------------------------------------
def gray_rgb(img: np.ndarray) -> np.ndarray:
    """Pillow's convert("L").convert("RGB") on u8 [..., 3]: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    v = img.astype(np.uint32)
    l = ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)
    return np.stack([l, l, l], -1)


def resize_bilinear(img: np.ndarray, size: int) -> np.ndarray:
    """Pillow BILINEAR (with its antialiasing support on reduction) to size x size: the host statement is Pillow itself."""
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((size, size), Image.BILINEAR))


def normalize(img_u8: np.ndarray) -> torch.Tensor:
    """ViTImageProcessor: rescale by 1 / 255, normalise with mean 0.5 and std 0.5 -> [3, S, S] float32."""
    x = torch.from_numpy(img_u8.astype(np.float32)) * np.float32(1.0 / 255.0)
    return ((x - 0.5) / 0.5).permute(2, 0, 1).contiguous()


def patch_rows(pixel_values: torch.Tensor, ps: int) -> torch.Tensor:
    """[N, 3, S, S] -> [N, (S / ps)^2, 3 ps ps], column = (c, py, px): the im2col of the patch convolution."""
    N, Cc, S, _ = pixel_values.shape
    G = S // ps
    return pixel_values.reshape(N, Cc, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(N, G * G, Cc * ps * ps)


def preprocess(crop_u8: np.ndarray, image_size: int) -> np.ndarray:
    """Line crop u8 [h, w, 3] -> u8 [S, S, 3] (byte-exact part of the pre-processing)."""
    return resize_bilinear(gray_rgb(crop_u8), image_size)


# ---- model ------------------------------------------------------------------------------------------------------------------------
def _ln(x, sd, p, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _lin(x, sd, p):
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"])


def _mha(q, k, v, heads, mask=None):
    B, Tq, E = q.shape
    hd = E // heads
    sp = lambda t: t.reshape(B, -1, heads, hd).transpose(1, 2)
    s = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(hd)
    if mask is not None:
        s = s + mask
    return (torch.softmax(s, -1) @ sp(v)).transpose(1, 2).reshape(B, Tq, E)


def cast(sd: Dict[str, torch.Tensor], dtype) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype) for k, v in sd.items()}


def encode(sd, c: MocrConfig, pixel_values: torch.Tensor) -> torch.Tensor:
    """pixel_values [N, 3, S, S] -> encoder_hidden_states [N, tokens, dec_hidden] as the decoder's cross-attention reads them
    (final layernorm, no pooler; enc_to_dec_proj where the hidden sizes differ)."""
    dt = sd["encoder.layernorm.weight"].dtype
    x = patch_rows(pixel_values.to(dt), c.patch_size)
    w = sd["encoder.embeddings.patch_embeddings.projection.weight"]
    x = x @ w.reshape(w.shape[0], -1).t() + sd["encoder.embeddings.patch_embeddings.projection.bias"]
    N = x.shape[0]
    toks = [sd["encoder.embeddings.cls_token"].expand(N, -1, -1)]
    if c.deit:
        toks.append(sd["encoder.embeddings.distillation_token"].expand(N, -1, -1))
    x = torch.cat(toks + [x], 1) + sd["encoder.embeddings.position_embeddings"]
    for i in range(c.enc_layers):
        p = f"encoder.layers.{i}"
        h = _ln(x, sd, p + ".layernorm_before", c.enc_eps)
        a = _mha(_lin(h, sd, p + ".attention.q_proj"), _lin(h, sd, p + ".attention.k_proj"), _lin(h, sd, p + ".attention.v_proj"), c.enc_heads)
        x = x + _lin(a, sd, p + ".attention.o_proj")
        h = _ln(x, sd, p + ".layernorm_after", c.enc_eps)
        x = x + _lin(F.gelu(_lin(h, sd, p + ".mlp.fc1")), sd, p + ".mlp.fc2")
    x = _ln(x, sd, "encoder.layernorm", c.enc_eps)
    if "enc_to_dec_proj.weight" in sd:
        x = _lin(x, sd, "enc_to_dec_proj")
    return x


def decoder_logits(sd, c: MocrConfig, tokens: torch.Tensor, memory: torch.Tensor) -> torch.Tensor:
    """Teacher-forced BertLMHeadModel: tokens [B, T] int64, memory [B, L, dec_hidden] -> logits [B, T, V] (causal self-attention)."""
    e = "decoder.bert.embeddings"
    B, T = tokens.shape
    x = sd[e + ".word_embeddings.weight"][tokens] + sd[e + ".token_type_embeddings.weight"][0] + sd[e + ".position_embeddings.weight"][:T]
    x = _ln(x, sd, e + ".LayerNorm", c.dec_eps)
    causal = torch.full((T, T), float("-inf"), dtype=x.dtype).triu(1)
    for i in range(c.dec_layers):
        p = f"decoder.bert.encoder.layer.{i}"
        a = _mha(_lin(x, sd, p + ".attention.self.query"), _lin(x, sd, p + ".attention.self.key"), _lin(x, sd, p + ".attention.self.value"),
                 c.dec_heads, causal)
        x = _ln(_lin(a, sd, p + ".attention.output.dense") + x, sd, p + ".attention.output.LayerNorm", c.dec_eps)
        a = _mha(_lin(x, sd, p + ".crossattention.self.query"), _lin(memory, sd, p + ".crossattention.self.key"),
                 _lin(memory, sd, p + ".crossattention.self.value"), c.dec_heads)
        x = _ln(_lin(a, sd, p + ".crossattention.output.dense") + x, sd, p + ".crossattention.output.LayerNorm", c.dec_eps)
        h = F.gelu(_lin(x, sd, p + ".intermediate.dense"))
        x = _ln(_lin(h, sd, p + ".output.dense") + x, sd, p + ".output.LayerNorm", c.dec_eps)
    h = "decoder.cls.predictions"
    x = _ln(F.gelu(_lin(x, sd, h + ".transform.dense")), sd, h + ".transform.LayerNorm", c.dec_eps)
    return _lin(x, sd, h + ".decoder")


# ---- beam search (transformers generation/utils.py::_beam_search, per line) -------------------------------------------------------------
def ban_ngrams(logp: torch.Tensor, hist: torch.Tensor, cur_len: int, n: int) -> torch.Tensor:
    """NoRepeatNGramLogitsProcessor on log-probabilities [R, V]; hist [R, >= cur_len]."""
    if n <= 0 or cur_len + 1 < n:
        return logp
    logp = logp.clone()
    for r in range(hist.shape[0]):
        seq = hist[r, :cur_len].tolist()
        tail = seq[cur_len - (n - 1):] if n > 1 else []
        for i in range(cur_len - n + 1):
            if seq[i:i + n - 1] == tail:
                logp[r, seq[i + n - 1]] = float("-inf")
    return logp


def beam_search(step_fn: Callable[[int, torch.Tensor], torch.Tensor], N: int, g: GenerationParams, steps: Optional[int] = None):
    """step_fn(step, hist [N * nb, step + 1] int64) -> log-probabilities [N * nb, V] (before the n-gram ban), any float dtype.
    Returns dict(tokens [N, T], length [N], score [N] float64, logp [steps, R, V] after the ban, hist [steps, R, T], done_step [N],
    steps_run).  A line that can no longer change (finished list full under early_stopping, or the early-stop heuristic satisfied) is
    frozen: its rows of ``hist`` keep their last state.  num_beams == 1 is greedy search: the line ends at its first EOS."""
    nb, T = g.num_beams, g.max_length
    K, R = 2 * nb, N * nb
    es = True if nb == 1 else g.early_stopping
    hist = torch.full((R, T), g.pad_token_id, dtype=torch.int64)
    hist[:, 0] = g.decoder_start_token_id
    run = [[0.0] * nb for _ in range(N)]
    fin: List[list] = [[] for _ in range(N)]   # (score, length, tokens), best first
    heur, done, done_step = [True] * N, [False] * N, [None] * N
    tr_logp, tr_hist = [], []
    n_steps = T - 1 if steps is None else steps
    steps_run = 0
    for step in range(n_steps):
        logp = ban_ngrams(step_fn(step, hist[:, :step + 1]).to(torch.float64), hist, step + 1, g.no_repeat_ngram_size)
        tr_logp.append(logp)
        new_hist = hist.clone()
        hit_all = step + 2 >= T
        len_pow = float(step + 1) ** g.length_penalty
        for n in range(N):
            if done[n]:
                continue
            cand = []
            for b in range(nb):
                base = -1.0e9 if (step == 0 and b > 0) else run[n][b]
                vals, idx = torch.sort(logp[n * nb + b], descending=True, stable=True)   # ties (banned tokens) to the lower token
                vals, idx = vals[:K], idx[:K]
                cand += [(base + float(v), b, int(t)) for v, t in zip(vals, idx)]
            cand.sort(key=lambda e: (-e[0], e[1], e[2]))
            top = cand[:K]
            hit = [hit_all or t == g.eos_token_id for _, _, t in top]
            keep = [q for q in range(K) if not hit[q]][:nb]
            keep += [q for q in range(K) if hit[q]][:nb - len(keep)]
            for q in range(nb):
                if not hit[q]:
                    continue
                key, b, t = top[q]
                sc = key / len_pow
                toks = hist[n * nb + b].clone()
                toks[step + 1] = t
                if len(fin[n]) == nb:
                    if not sc > fin[n][-1][0]:
                        continue
                    fin[n].pop()
                m = len(fin[n])
                while m > 0 and sc > fin[n][m - 1][0]:
                    m -= 1
                fin[n].insert(m, (sc, step + 2, toks))
            new_run = []
            for k, q in enumerate(keep):
                key, b, t = top[q]
                new_hist[n * nb + k] = hist[n * nb + b]
                new_hist[n * nb + k, step + 1] = t
                new_run.append(key + (-1.0e9 if hit[q] else 0.0))
            run[n] = new_run
            if len(fin[n]) == nb and not (new_run[0] / len_pow > fin[n][-1][0]):
                heur[n] = False
            if (len(fin[n]) == nb if es else not heur[n]) or hit_all:
                done[n], done_step[n] = True, step
        hist = new_hist
        tr_hist.append(hist.clone())
        steps_run = step + 1
        if all(done):
            break
    tokens = torch.full((N, T), g.pad_token_id, dtype=torch.int64)
    length = torch.zeros(N, dtype=torch.int64)
    score = torch.full((N,), -1.0e9, dtype=torch.float64)
    for n in range(N):
        if fin[n]:
            score[n], length[n], tokens[n] = fin[n][0][0], fin[n][0][1], fin[n][0][2]
    return dict(tokens=tokens, length=length, score=score, logp=torch.stack(tr_logp), hist=torch.stack(tr_hist), done_step=done_step,
                steps_run=steps_run)


def generate(sd, c: MocrConfig, memory: torch.Tensor, g: GenerationParams):
    """Beam search over the restated decoder; memory [N, L, dec_hidden]."""
    nb = g.num_beams
    mem = memory.repeat_interleave(nb, 0)

    def step_fn(step, hist):
        return torch.log_softmax(decoder_logits(sd, c, hist, mem)[:, -1], -1)

    return beam_search(step_fn, memory.shape[0], g)


def replay(tables: torch.Tensor, N: int, g: GenerationParams):
    """The bookkeeping alone on log-probability tables [steps, N * nb, V]."""
    return beam_search(lambda step, hist: tables[step], N, g, steps=tables.shape[0])


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def gen_params(num_beams=4, ngram=0, length_penalty=1.0, early_stopping=False, max_length=16) -> GenerationParams:
    return GenerationParams(max_length=max_length, num_beams=num_beams, no_repeat_ngram_size=ngram, length_penalty=length_penalty,
                            early_stopping=early_stopping, eos_token_id=EOS, pad_token_id=PAD, decoder_start_token_id=START)


def make_case(seed: int, eos_bias: float, embed_scale: float = 1.0, dtype=torch.float64, **cfg_kw):
    """(config dict, MocrConfig, state dict in ``dtype``) of one seeded model (see the recipe at the top)."""
    cfg = tiny_config_dict(**cfg_kw)
    c = config_from_dict(cfg)
    sd = synth_state_dict(mocr_schema(c), seed=seed)
    b = sd["decoder.cls.predictions.bias"].clone()
    b[EOS] += eos_bias
    sd["decoder.cls.predictions.bias"] = b
    sd["decoder.cls.predictions.decoder.bias"] = b
    sd["decoder.bert.embeddings.word_embeddings.weight"] = sd["decoder.bert.embeddings.word_embeddings.weight"] * embed_scale
    return cfg, c, cast(sd, dtype)


def make_crops(n: int, seed: int = 0, sizes=((40, 90), (23, 57), (64, 31), (17, 120), (48, 48))) -> List[np.ndarray]:
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(*sizes[i % len(sizes)], 3), dtype=np.uint8) for i in range(n)]


def pixel_values(crops: List[np.ndarray], image_size: int) -> torch.Tensor:
    return torch.stack([normalize(preprocess(cr, image_size)) for cr in crops])


# name -> (model keywords, seed, eos_bias, embed_scale, lines, generation keywords).  What each is for:
#   vit32    three lines ending at different steps, the n-gram ban active, early_stopping off (the heuristic ends lines)
#   vit48    image 48² (10 tokens), V = 97 (no multiple of 8: the vocabulary Linear takes the tiled form), N = 5, length_penalty 2,
#            early_stopping on
#   deit     the distillation token, decoder narrower than the encoder (enc_to_dec_proj), N = 1
#   greedy   num_beams = 1
#   early    a strong EOS bias: lines finish within the first two steps
#   tomax    EOS never wins: every line runs to max_length
#   wide     hidden 768 / 12 heads / 1 + 1 layers / FFN 3072 / V = 6144, 2 lines, 6 steps: the real row width
CASES = {
    "vit32": (dict(vocab=50, max_pos=40), 1, 9.5, 1.5, 3, dict(num_beams=4, ngram=3, length_penalty=1.0, early_stopping=False, max_length=16)),
    "vit48": (dict(image_size=48, vocab=97, max_pos=32), 0, 7.0, 1.0, 5, dict(num_beams=4, ngram=0, length_penalty=2.0, early_stopping=True, max_length=12)),
    "deit": (dict(deit=True, vocab=48, max_pos=32, dec_hidden=32), 2, 8.5, 1.0, 1, dict(num_beams=4, ngram=3, length_penalty=1.0, early_stopping=True, max_length=12)),
    "greedy": (dict(vocab=64, max_pos=32), 3, 4.5, 1.5, 3, dict(num_beams=1, ngram=3, length_penalty=1.0, early_stopping=False, max_length=14)),
    "early": (dict(vocab=50, max_pos=32), 0, 12.0, 1.0, 2, dict(num_beams=4, ngram=0, length_penalty=1.0, early_stopping=True, max_length=10)),
    "tomax": (dict(vocab=50, max_pos=32), 4, -4.0, 1.0, 2, dict(num_beams=4, ngram=0, length_penalty=2.0, early_stopping=False, max_length=9)),
    "wide": (dict(hidden=768, heads=12, enc_layers=1, dec_layers=1, inter=3072, vocab=6144, max_pos=16), 0, 6.0, 1.0, 2,
             dict(num_beams=4, ngram=3, length_penalty=2.0, early_stopping=True, max_length=7)),
}


def case(name: str, dtype=torch.float64):
    """(config dict, MocrConfig, state dict, crops, GenerationParams) of a named case."""
    kw, seed, eos_bias, embed_scale, lines, gkw = CASES[name]
    cfg, c, sd = make_case(seed, eos_bias, embed_scale, dtype, **kw)
    return cfg, c, sd, make_crops(lines, seed), gen_params(**gkw)


def run_case(name: str, dtype=torch.float64):
    """The oracle's own run of a case: dict(memory, **generate(...))."""
    _, c, sd, crops, g = case(name, dtype)
    with torch.no_grad():
        mem = encode(sd, c, pixel_values(crops, c.image_size))
        out = generate(sd, c, mem, g)
    out["memory"] = mem
    return out
