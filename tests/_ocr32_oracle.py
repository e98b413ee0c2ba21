"""Float32 / float64 CPU oracle of the 32px OCR (the reference's ``Ocr.ocr32px``), restated from its description:
``OCR.infer_beam_batch`` / ``next_token_batch`` (manga_translator/ocr/model_32px.py:415-465, :518-595) and the tensor path of
``Model32pxOCR._infer`` (:58-140).  Plain ``F.conv2d`` / matmuls; no reference code.  ``make_fixtures()`` writes
tests/golden/ocr32.npz from the reference's own ``OCR`` module (only where the reference tree is present)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from manga_image_translator_amd import ocr32_schema as S, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
E, H, HD = 320, 4, 80
BEAMS, START, END = 5, 1, 2
DICT = 97
# (tag, seed, widths, steps (max_seq_length), </S> bias added to pred.bias[2]) — the beam cases of the CPU and GPU tests
# plain: no line ends (the step limit); early: lines whose first token is </S> end at once while line 0 goes on; spread: lines done at
# steps 2, 8 and 10 beside one that never ends (four lengths); one: a line with ONE finished hypothesis at the step limit
CASES = (("plain", 0, (50, 77, 120, 121), 12, 0.0), ("early", 0, (50, 77, 120, 121), 12, 2.0),
         ("spread", 2, (40, 70, 100, 128), 12, 4.0), ("one", 2, (40, 70, 100, 128), 12, 3.5))


def weights(dict_size: int = DICT, seed: int = 0, eos_bias: float = 0.0):
    sd = synth.synth_state_dict(S.ocr32_schema(dict_size), seed=seed)
    if eos_bias:
        sd["pred.bias"] = sd["pred.bias"].clone()
        sd["pred.bias"][END] += eos_bias
    return sd


def lines_u8(widths, seed: int):
    """Seeded glyph-like line crops [32, w, 3] u8 and the chunk tensor the reference forms from them (:77-87)."""
    rng = np.random.default_rng(1000 + seed)
    imgs = []
    for w in widths:
        im = np.full((32, w, 3), 245, np.uint8)
        for x in range(2, w - 6, 9):
            if rng.random() < 0.8:
                g = int(rng.integers(3, 8))
                y = int(rng.integers(2, 32 - g - 2))
                im[y:y + g, x:x + g] = rng.integers(0, 60, size=3)
        imgs.append(im)
    return imgs


def make_region(imgs, widths=None):
    widths = [im.shape[1] for im in imgs] if widths is None else widths
    wp = 4 * (max(widths) + 7) // 4   # == max + 7 (:78)
    region = np.zeros((len(imgs), 32, wp, 3), np.uint8)
    for i, im in enumerate(imgs):
        region[i, :, :im.shape[1]] = im
    return region


def cast(sd, dt):
    return {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}


# ---- backbone (ResNet.forward :201-234, BasicBlock.forward :253-267) ---------------------------------------------------------
def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def backbone(sd, x):
    p = "backbone.ConvNet"
    c = lambda n, t, **kw: F.conv2d(t, sd[f"{p}.{n}.weight"], **kw)
    x = c("conv0_2", F.relu(_bn(sd, p + ".bn0_1", c("conv0_1", x, padding=1))), padding=1)
    pools = [dict(kernel_size=2, stride=2), dict(kernel_size=2, stride=2), dict(kernel_size=2, stride=(2, 1), padding=(0, 1)), None]
    for li, n in enumerate(S.LAYERS, start=1):
        if pools[li - 1] is not None:
            x = F.avg_pool2d(x, **pools[li - 1])
        for b in range(n):
            q = f"{p}.layer{li}.{b}"
            out = F.conv2d(F.relu(_bn(sd, q + ".bn1", x)), sd[q + ".conv1.weight"], padding=1)
            out = F.conv2d(F.relu(_bn(sd, q + ".bn2", out)), sd[q + ".conv2.weight"], padding=1)
            res = x
            if (q + ".downsample.1.weight") in sd:
                res = F.conv2d(_bn(sd, q + ".downsample.0", x), sd[q + ".downsample.1.weight"])
            x = out + res
        if li < 4:
            x = c(f"conv{li}", F.relu(_bn(sd, f"{p}.bn{li}", x)), padding=1)
    x = c("conv4_1", F.relu(_bn(sd, p + ".bn4_1", x)), stride=(2, 1), padding=(0, 1))
    x = c("conv4_2", F.relu(_bn(sd, p + ".bn4_2", x)))
    return _bn(sd, p + ".bn4_3", x)   # [N, 320, 1, T]


# ---- attention / layers ------------------------------------------------------------------------------------------------------
def mha(sd, p, q_in, kv_in, key_mask=None):
    """nn.MultiheadAttention (batch_first False): q_in [Lq, N, E], kv_in [Lk, N, E], key_mask [N, Lk] True = masked."""
    w, b = sd[p + ".in_proj_weight"], sd[p + ".in_proj_bias"]
    Lq, N, _ = q_in.shape
    Lk = kv_in.shape[0]
    q = (q_in @ w[:E].t() + b[:E]) * (HD ** -0.5)
    k = kv_in @ w[E:2 * E].t() + b[E:2 * E]
    v = kv_in @ w[2 * E:].t() + b[2 * E:]
    q = q.reshape(Lq, N, H, HD).permute(1, 2, 0, 3)
    k = k.reshape(Lk, N, H, HD).permute(1, 2, 0, 3)
    v = v.reshape(Lk, N, H, HD).permute(1, 2, 0, 3)
    att = q @ k.transpose(-1, -2)
    if key_mask is not None:
        att = att.masked_fill(key_mask[:, None, None, :], float("-inf"))
    o = torch.softmax(att, -1) @ v                                   # [N, H, Lq, HD]
    o = o.permute(2, 0, 1, 3).reshape(Lq, N, E)
    return o @ sd[p + ".out_proj.weight"].t() + sd[p + ".out_proj.bias"]


def _ln(sd, p, x):
    return F.layer_norm(x, (E,), sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def _ffn(sd, p, x):
    return F.relu(x @ sd[p + ".linear1.weight"].t() + sd[p + ".linear1.bias"]) @ sd[p + ".linear2.weight"].t() + sd[p + ".linear2.bias"]


def valid_len(w: int) -> int:
    return (w + 3) // 4 + 2


def encode(sd, region_u8: np.ndarray, widths, taps=None):
    """region u8 [N, 32, Wp, 3] -> (memory [T, N, E], mask [N, T] bool) (:519-528)."""
    dt = sd["pe.pe"].dtype
    x = (torch.from_numpy(region_u8).to(dt) - 127.5) / 127.5
    feats = backbone(sd, x.permute(0, 3, 1, 2))
    feats = feats[:, :, 0, :].permute(2, 0, 1)                       # 'n e h s -> s n e' (h == 1)
    T, N, _ = feats.shape
    if taps is not None:
        taps["backbone"] = feats.permute(1, 0, 2).clone()
    mask = torch.zeros(N, T, dtype=torch.bool)
    for i, w in enumerate(widths):
        mask[i, valid_len(w):] = True
    x = feats + sd["pe.pe"][:T]
    for i in range(S.N_ENC):
        p = f"encoders.layers.{i}"
        x = _ln(sd, p + ".norm1", x + mha(sd, p + ".self_attn", x, x, mask))
        x = _ln(sd, p + ".norm2", x + _ffn(sd, p, x))
    return x, mask


def next_token(sd, toks, pos, caches, memory, mem_mask):
    """next_token_batch (:415-465) for n hypotheses of equal length: toks [n], caches[l] [pos, n, E] (inputs of layer l at the earlier
    steps; caches[N_DEC] the outputs).  Returns (out [n, E], new caches)."""
    tgt = (sd["embd.weight"][toks] + sd["pe.pe"][pos, 0])[None]     # [1, n, E]
    new = []
    for l in range(S.N_DEC):
        p = f"decoders.layers.{l}"
        hist = torch.cat([caches[l], tgt], 0)
        new.append(hist)
        tgt = _ln(sd, p + ".norm1", tgt + mha(sd, p + ".self_attn", tgt, hist))
        tgt = _ln(sd, p + ".norm2", tgt + mha(sd, p + ".multihead_attn", tgt, memory, mem_mask))
        tgt = _ln(sd, p + ".norm3", tgt + _ffn(sd, p, tgt))
    new.append(torch.cat([caches[S.N_DEC], tgt], 0))
    return tgt[0], new


def logits_of(sd, dec):
    return F.relu(dec @ sd["pred1.0.weight"].t() + sd["pred1.0.bias"]) @ sd["pred.weight"].t() + sd["pred.bias"]


def color_heads(sd, dec):
    f = F.relu(dec @ sd["color_pred1.0.weight"].t() + sd["color_pred1.0.bias"])
    return torch.cat([f @ sd[h + ".weight"].t() + sd[h + ".bias"] for h in S.COLOR_HEADS], -1)   # [.., 6]


# ---- the Hypothesis bookkeeping alone (:529-585), on top-5 tables ---------------------------------------------------------------
class Hyp:
    __slots__ = ("line", "toks", "lps", "parent")

    def __init__(self, line, toks, lps, parent):
        self.line, self.toks, self.lps, self.parent = line, toks, lps, parent   # parent: index in the previous live list

    def key(self, ftype):
        return -float(np.asarray(self.lps, dtype=ftype).mean())

    def ended(self):
        return self.toks[-1] == END


class Beams:
    """first(): step 0; step(): one iteration of the loop; result(): the final pick.  ``live`` is the reference's ``hypos`` list."""

    def __init__(self, n_lines: int, max_finished: int = 2, ftype=np.float64):
        self.N, self.max_finished, self.ftype = n_lines, max_finished, ftype
        self.finished = {}
        self.live = []
        self.last = {}
        self.done_at = {}
        self.steps = 0

    def first(self, vals, idx):
        """vals / idx [N, 5]: the top-5 of each line's first row.  Nothing is tested for </S> here (:535-541)."""
        self.live = [Hyp(i, [START, int(idx[i][k])], [0.0, float(vals[i][k])], i) for i in range(self.N) for k in range(BEAMS)]
        self.steps = 1
        return self.live

    def step(self, vals, idx):
        """vals / idx [len(live), 5] (:549-572)."""
        per = {}
        for r, h in enumerate(self.live):
            for k in range(BEAMS):
                per.setdefault(h.line, []).append(Hyp(h.line, h.toks + [int(idx[r][k])], h.lps + [float(vals[r][k])], r))
        self.last = per
        live = []
        for i, cands in per.items():
            cur = sorted(cands, key=lambda a: a.key(self.ftype))[:BEAMS + 1]
            keep, done = [], False
            for h in cur:
                if h.ended():
                    self.finished.setdefault(i, []).append(h)
                    if len(self.finished[i]) >= self.max_finished:
                        done = True
                        self.done_at[i] = self.steps
                        break
                elif len(keep) < BEAMS:
                    keep.append(h)
            if not done:
                live += keep
        self.live = live
        self.steps += 1
        return live

    def result(self):
        out = []
        for i in range(self.N):
            if i not in self.finished:
                out.append(sorted(self.last[i], key=lambda a: a.key(self.ftype))[0])
            else:
                out.append(sorted(self.finished[i], key=lambda a: a.key(self.ftype))[0])
        return out


def replay(vals_steps, idx_steps, n_lines, max_finished=2, ftype=np.float64):
    """The bookkeeping over in-place tables [steps][N * 5][5] (row 5 n + j = line n's j-th kept hypothesis; step 0 reads row 5 n; rows of
    done lines are ignored) — the layout the native decoder uses.  Returns (Beams, kept-token trace per step {line: [5 token lists]})."""
    b = Beams(n_lines, max_finished, ftype)
    b.first([vals_steps[0][5 * i] for i in range(n_lines)], [idx_steps[0][5 * i] for i in range(n_lines)])
    trace = [_kept(b)]
    for s in range(1, len(vals_steps)):
        if not b.live:
            break
        rows = []
        seen = {}
        for h in b.live:
            j = seen.get(h.line, 0)
            seen[h.line] = j + 1
            rows.append(5 * h.line + j)
        b.step([vals_steps[s][r] for r in rows], [idx_steps[s][r] for r in rows])
        trace.append(_kept(b))
    return b, trace


def _kept(b):
    out = {}
    for h in b.live:
        out.setdefault(h.line, []).append(list(h.toks))
    return out


# ---- the whole beam search --------------------------------------------------------------------------------------------------
@torch.no_grad()
def beam_search(sd, memory, mask, max_seq_length: int, max_finished: int = 2, ftype=None):
    """infer_beam_batch after the encoder.  Returns dict(tokens, prob, mean, colors [len, 6] per line, trace)."""
    dt = memory.dtype
    ftype = ftype or (np.float32 if dt == torch.float32 else np.float64)
    N = memory.shape[1]
    b = Beams(N, max_finished, ftype)
    empty = [torch.zeros(0, N, E, dtype=dt) for _ in range(S.N_DEC + 1)]
    dec, caches = next_token(sd, torch.full((N,), START), 0, empty, memory, mask)
    lp = torch.log_softmax(logits_of(sd, dec), -1)
    trace = dict(logprobs=[lp.clone()], lines=[list(range(N))], kept=[], logits=[logits_of(sd, dec)])
    vals, idx = torch.topk(lp, BEAMS, dim=1)
    live = b.first(vals.tolist(), idx.tolist())
    trace["kept"].append(_kept(b))
    sel = torch.tensor([h.parent for h in live])
    caches = [c[:, sel] for c in caches]
    outputs = {}
    for _ in range(max_seq_length):
        lines = torch.tensor([h.line for h in live])
        toks = torch.tensor([h.toks[-1] for h in live])
        dec, caches = next_token(sd, toks, b.steps, caches, memory[:, lines], mask[lines])
        lg = logits_of(sd, dec)
        lp = torch.log_softmax(lg, -1)
        trace["logprobs"].append(lp.clone())
        trace["logits"].append(lg)
        trace["lines"].append(lines.tolist())
        vals, idx = torch.topk(lp, BEAMS, dim=1)
        prev_caches = caches
        live = b.step(vals.tolist(), idx.tolist())
        trace["kept"].append(_kept(b))
        # output histories of hypotheses that may be picked: every candidate's history is its parent's (:404-410)
        for i, fin in b.finished.items():
            for h in fin:
                if id(h) not in outputs:
                    outputs[id(h)] = prev_caches[S.N_DEC][:, h.parent].clone()
        outputs["last"] = (prev_caches[S.N_DEC], {i: c for i, c in b.last.items()})
        if not live:
            break
        sel = torch.tensor([h.parent for h in live])
        caches = [c[:, sel] for c in prev_caches]
    res = b.result()
    out = dict(tokens=[], prob=[], mean=[], colors=[], dec=[], trace=trace, beams=b)
    for i, h in enumerate(res):
        hist = outputs[id(h)] if id(h) in outputs else outputs["last"][0][:, h.parent]
        out["tokens"].append(list(h.toks))
        m = np.asarray(h.lps, dtype=ftype).mean()
        out["mean"].append(float(m))
        out["prob"].append(float(np.exp(m)))
        out["dec"].append(hist)
        out["colors"].append(color_heads(sd, hist))
    return out


@torch.no_grad()
def infer_chunk(sd, region_u8, widths, max_seq_length, dt=torch.float64, taps=None):
    sdc = cast(sd, dt)
    mem, mask = encode(sdc, region_u8, widths, taps)
    if taps is not None:
        taps["memory"] = mem.permute(1, 0, 2).clone()
    return beam_search(sdc, mem, mask, max_seq_length)


# ---- Model32pxOCR._infer's host rules (:58-140) ------------------------------------------------------------------------------------
def int_colors(col: torch.Tensor):
    """[len, 6] head outputs -> six ints (:104-109) and the float values mean * 255 they truncate."""
    f = col.clamp(0, 1).mean(0) * 255
    return [int(v) for v in f.to(torch.int64).tolist()], f.tolist()


def text_of(tokens, dictionary):
    seq = []
    for t in tokens:
        ch = dictionary[t]
        if ch == "<S>":
            continue
        if ch == "</S>":
            break
        seq.append(" " if ch == "<SP>" else ch)
    return "".join(seq)


def dictionary(n: int = DICT):
    return ["<PAD>", "<S>", "</S>", "<SP>"] + [chr(0x3041 + i) for i in range(n - 4)]


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def reference_model(sd, dict_size):
    """The reference's own OCR module (unmodified) holding ``sd``; None where the reference tree is absent."""
    from oracle import ref_import

    if not ref_import.available():
        return None
    ref_import._prepare()
    mod = ref_import._load("manga_translator.ocr.model_32px", "ocr/model_32px.py")
    m = mod.OCR(dictionary(dict_size), S.MAX_LEN)
    m.load_state_dict(sd)
    return m.eval()


@torch.no_grad()
def run_reference(model, region_u8, widths, max_seq_length):
    x = (torch.from_numpy(region_u8).float() - 127.5) / 127.5
    ret = model.infer_beam_batch(x.permute(0, 3, 1, 2).contiguous(), list(widths), beams_k=5, max_seq_length=max_seq_length)
    return [dict(tokens=r[0].tolist(), prob=float(r[1]), colors=torch.cat([c.reshape(-1, 1) for c in r[2:]], 1)) for r in ret]


@torch.no_grad()
def make_fixtures(path=None):
    path = path or os.path.join(GOLDEN, "ocr32.npz")
    out = {}
    for tag, seed, widths, steps, eos in CASES:
        sd = weights(DICT, seed, eos)
        model = reference_model(sd, DICT)
        if model is None:
            raise RuntimeError("the reference tree is needed to write fixtures")
        region = make_region(lines_u8(widths, seed))
        res = run_reference(model, region, widths, steps)
        if tag == CASES[0][0]:   # one backbone tap (the largest array of the file)
            feats = model.backbone((torch.from_numpy(region).float().permute(0, 3, 1, 2) - 127.5) / 127.5)
            out[f"{tag}.backbone"] = feats[:, :, 0, :].permute(0, 2, 1).numpy()
        out[f"{tag}.region"] = region
        out[f"{tag}.widths"] = np.asarray(widths, np.int32)
        out[f"{tag}.prob"] = np.asarray([r["prob"] for r in res], np.float64)
        for i, r in enumerate(res):
            out[f"{tag}.tokens{i}"] = np.asarray(r["tokens"], np.int32)
            out[f"{tag}.colors{i}"] = r["colors"].numpy()
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    print(make_fixtures())


# ---- crafted top-5 tables for the bookkeeping alone (CPU: replay(); GPU: mit_ocr32_beam_replay) ---------------------------------
def _tables(n_lines, steps):
    vals = np.tile(np.asarray([-1.0, -1.5, -2.0, -2.5, -3.0], np.float32), (steps, n_lines * 5, 1))
    idx = np.tile(np.asarray([10, 11, 12, 13, 14], np.int32), (steps, n_lines * 5, 1))
    return vals, idx


def crafted():
    """name -> dict(vals, idx [steps, N * 5, 5], N, T, tokens = the expected result per line, kept = expected kept hypotheses after the
    last step per live line (or None)).  Expectations are worked out by hand from the rules of model_32px.py:529-585."""
    out = {}
    # the first token </S> is not tested (:535-541): the hypothesis is extended like any other and stays the best
    v, i = _tables(1, 2)
    i[0, 0] = [END, 10, 11, 12, 13]
    v[0, 0] = [-0.1, -1.0, -2.0, -3.0, -4.0]
    v[1, 0] = [-0.1, -1.5, -2.0, -2.5, -3.0]
    out["first_eos"] = dict(vals=v, idx=i, N=1, T=1, tokens=[[START, END, 10]], kept=None)
    # exact ties: Python's sort is stable, so the order (hypothesis, rank) decides; all five kept come from hypothesis 0
    v, i = _tables(1, 2)
    v[:] = -1.0
    out["ties"] = dict(vals=v, idx=i, N=1, T=1, tokens=[[START, 10, 10]],
                       kept={0: [[START, 10, 10], [START, 10, 11], [START, 10, 12], [START, 10, 13], [START, 10, 14]]})
    # beams_k + 1 = 6 are looked at: with one </S> among them the SIXTH candidate is the fifth kept
    v, i = _tables(1, 2)
    v[0] = -1.0
    i[1, 0] = [END, 10, 11, 12, 13]
    v[1, 0] = [-0.1, -0.2, -0.3, -0.4, -0.5]
    v[1, 1] = [-0.6, -5.0, -5.0, -5.0, -5.0]
    v[1, 2:] = -9.0
    out["sixth"] = dict(vals=v, idx=i, N=1, T=1, tokens=[[START, 10, END]],
                        kept={0: [[START, 10, 10], [START, 10, 11], [START, 10, 12], [START, 10, 13], [START, 11, 10]]})
    # three lines, T = 3: line 0 is done at the first loop step by two </S> in its best six (candidates after the second are dropped) while
    # its neighbours go on; line 1 keeps ONE finished hypothesis (mean -0.4) and returns it although its live ones end higher (-0.22);
    # line 2 never finishes and returns the best of the last 25
    v, i = _tables(3, 4)
    i[1, 0] = [END, 10, 11, 12, 13]
    v[1, 0] = [-0.1, -0.2, -3.0, -3.0, -3.0]
    i[1, 1] = [END, 10, 11, 12, 13]
    v[1, 1] = [-0.1, -3.0, -3.0, -3.0, -3.0]
    i[1, 5] = [10, END, 11, 12, 13]
    v[1, 5] = [-0.1, -0.2, -0.3, -0.4, -0.5]
    v[2, 5] = [0.0, -1.5, -2.0, -2.5, -3.0]
    v[3, 5] = [0.0, -1.5, -2.0, -2.5, -3.0]
    out["dropout"] = dict(vals=v, idx=i, N=3, T=3, tokens=[[START, 10, END], [START, 10, END], [START, 10, 10, 10, 10]], kept=None)
    return out
