"""manga-ocr recogniser (``--ocr mocr``) on the gfx950 engine: ViT / DeiT encoder, BERT decoder with cross-attention, HuggingFace's
``generate`` as one native call.

Reference: ``ModelMangaOCR._infer`` (manga_translator/ocr/model_manga_ocr.py:132-295) takes each line's text from the ``manga_ocr``
package: ``img.convert("L").convert("RGB")`` -> ``ViTImageProcessor`` (Pillow BILINEAR to image_size², x / 255, mean 0.5, std 0.5) ->
``VisionEncoderDecoderModel.generate(x[None], max_length=300)``.  Every size and generation parameter comes from the model's config
(mocr_schema.load_model_dir); what is not implemented is refused by name.

MI355X layout
* pre-processing on the device from the uploaded page: per-line perspective warp (mit_ocr_warp_lines, each line at its own height) ->
  mit_mocr_gray -> Pillow-exact BILINEAR (imgproc.pil_resize_u8) -> mit_mocr_patches, which writes the normalised patch rows in the
  order of the projection weight's (c, py, px) axes, so the patch convolution is one Linear; byte-exact up to the resize;
* encoder: pre-LN layers on the tiled GEMM (q | k | v fused, the q columns scaled by head_dim ** -0.5 in the epilogue),
  mit_attention_heads over all tokens, mit_layernorm_wide (hidden 768 is beyond mit_layernorm), erf GELU in the fc1 epilogue;
* the cross-attention K | V of every decoder layer are projected once per line at encode time;
* decoder: mit_mocr_decode (csrc/mocr_decoder.hip) — the whole beam search, no host round trip per step.  Its workspace is dominated by
  the K / V history (layers x 2 x lines x beams x max_length x hidden floats), so recognize() / recognize_lines() decode a page's lines in
  chunks that keep it under ``max_workspace_bytes`` (a line's result does not depend on the other lines of its call).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import imgproc
from . import lib as _lib
from . import ops
from . import textline as TL
from .lib import MitMocrDecodeArgs, MitMocrDecoder, MitMocrLayer
from .mocr_schema import GenerationParams, MocrConfig, config_from_dict, mocr_schema
from .ocr48 import Linear
from .ops import ACT_GELU
from .synth import check_state_dict


def _fill_token(g: GenerationParams) -> int:
    """What results are padded with: ``pad_token_id``; HuggingFace's beam search fills with ``pad_token_id or eos_token_id``, so a pad
    token 0 (or none) gives the EOS token there."""
    if g.num_beams > 1:
        return g.pad_token_id or g.eos_token_id
    return g.eos_token_id if g.pad_token_id is None else g.pad_token_id


class MocrEngine(ops.Engine):
    """preprocess(): line crops -> u8 [N, S, S, 3]; encode(): -> cross-attention K / V; decode(): beam search; recognize(crops) and
    recognize_lines(page, quads, directions) chain them."""

    MAX_WORKSPACE_BYTES = 2 << 30   # decode workspace per call; more lines than fit are decoded in chunks

    def __init__(self, sd: Dict[str, torch.Tensor], config: Dict, generation: GenerationParams, device="cuda"):
        super().__init__(device)
        self.max_workspace_bytes = self.MAX_WORKSPACE_BYTES
        dev = self.device
        self.cfg: MocrConfig = config if isinstance(config, MocrConfig) else config_from_dict(config)
        c = self.cfg
        check_state_dict(sd, mocr_schema(c, pooler=False), "mocr state dict")
        self.generation = self._checked(generation)
        f = lambda k: sd[k].detach().float().to(dev).contiguous()
        ln = lambda p: (f(p + ".weight"), f(p + ".bias"))
        lin = lambda p: Linear(sd[p + ".weight"], sd[p + ".bias"], dev)

        def fused(names, hidden, heads, scaled=True):
            w = torch.cat([sd[n + ".weight"].float() for n in names], 0)
            b = torch.cat([sd[n + ".bias"].float() for n in names], 0)
            sc = None
            if scaled:   # the q columns carry head_dim ** -0.5 (bias included); k | v columns stay
                sc = torch.cat([torch.full((hidden,), (hidden // heads) ** -0.5), torch.ones(w.shape[0] - hidden)])
            return Linear(w, b, dev, sc)

        # -- encoder
        H = c.enc_hidden
        pw = sd["encoder.embeddings.patch_embeddings.projection.weight"]
        self.patch = Linear(pw.reshape(H, -1), sd["encoder.embeddings.patch_embeddings.projection.bias"], dev)
        pos = f("encoder.embeddings.position_embeddings")[0]                        # [tokens, H]
        extra = [f("encoder.embeddings.cls_token")[0]] + ([f("encoder.embeddings.distillation_token")[0]] if c.deit else [])
        self.n_extra = len(extra)
        self.extra_rows = (torch.cat(extra, 0) + pos[:self.n_extra]).contiguous()     # cls (+ distillation) token + its position
        self.patch_pos = pos[self.n_extra:].contiguous()                           # added to the projection in its epilogue
        self.enc = []
        for i in range(c.enc_layers):
            p = f"encoder.layers.{i}"
            self.enc.append(dict(qkv=fused([f"{p}.attention.{n}_proj" for n in "qkv"], H, c.enc_heads), out=lin(p + ".attention.o_proj"),
                                 ff1=lin(p + ".mlp.fc1"), ff2=lin(p + ".mlp.fc2"), ln1=ln(p + ".layernorm_before"), ln2=ln(p + ".layernorm_after")))
        self.enc_ln = ln("encoder.layernorm")
        self.enc_to_dec = lin("enc_to_dec_proj") if "enc_to_dec_proj.weight" in sd else None
        if (self.enc_to_dec is None) != (c.enc_hidden == c.dec_hidden):
            raise ValueError("mocr state dict: enc_to_dec_proj must be present exactly when the hidden sizes differ")

        # -- decoder
        D = c.dec_hidden
        self._keep: List = []
        layers = (MitMocrLayer * c.dec_layers)()
        self.mem_kv = []
        for l in range(c.dec_layers):
            p = f"decoder.bert.encoder.layer.{l}"
            lins = dict(q=fused([p + ".attention.self.query"], D, c.dec_heads),
                        kv=fused([p + ".attention.self.key", p + ".attention.self.value"], D, c.dec_heads, scaled=False),
                        out=lin(p + ".attention.output.dense"), q2=fused([p + ".crossattention.self.query"], D, c.dec_heads),
                        out2=lin(p + ".crossattention.output.dense"), ff1=lin(p + ".intermediate.dense"), ff2=lin(p + ".output.dense"))
            self._keep.append(lins)
            for k, v in lins.items():
                setattr(layers[l], k, v.c_struct())
            for i, name in ((1, ".attention.output.LayerNorm"), (2, ".crossattention.output.LayerNorm"), (3, ".output.LayerNorm")):
                wt, bt = ln(p + name)
                self._keep += [wt, bt]
                setattr(layers[l], f"ln{i}_w", wt.data_ptr())
                setattr(layers[l], f"ln{i}_b", bt.data_ptr())
            self.mem_kv.append(fused([p + ".crossattention.self.key", p + ".crossattention.self.value"], D, c.dec_heads, scaled=False))
        self._layers = layers
        e = "decoder.bert.embeddings"
        h = "decoder.cls.predictions"
        self.word, self.pos, self.type0 = f(e + ".word_embeddings.weight"), f(e + ".position_embeddings.weight"), f(e + ".token_type_embeddings.weight")[0].contiguous()
        self.emb_ln, self.head_ln = ln(e + ".LayerNorm"), ln(h + ".transform.LayerNorm")
        self.head_dense, self.head_out = lin(h + ".transform.dense"), lin(h + ".decoder")
        d = MitMocrDecoder()
        d.layers = C.cast(layers, C.c_void_p)
        d.n_layers, d.hidden, d.heads, d.inter, d.vocab, d.max_pos = c.dec_layers, D, c.dec_heads, c.dec_inter, c.vocab, c.max_pos
        d.word_emb, d.pos_emb, d.type_emb = self.word.data_ptr(), self.pos.data_ptr(), self.type0.data_ptr()
        d.emb_ln_w, d.emb_ln_b = (t.data_ptr() for t in self.emb_ln)
        d.head_ln_w, d.head_ln_b = (t.data_ptr() for t in self.head_ln)
        d.head_dense, d.head_out = self.head_dense.c_struct(), self.head_out.c_struct()
        d.ln_eps = c.dec_eps
        self.dec = d

    def _checked(self, g: GenerationParams) -> GenerationParams:
        c = self.cfg
        for name in ("eos_token_id", "decoder_start_token_id"):
            v = getattr(g, name)
            if v is None or not 0 <= v < c.vocab:
                raise ValueError(f"mocr generation: {name} = {v!r} must be a token of the vocabulary (0 .. {c.vocab - 1})")
        if g.pad_token_id is not None and not 0 <= g.pad_token_id < c.vocab:
            raise ValueError(f"mocr generation: pad_token_id = {g.pad_token_id!r} is outside the vocabulary")
        if g.max_length > c.max_pos:
            raise ValueError(f"mocr generation: max_length = {g.max_length} exceeds max_position_embeddings = {c.max_pos}")
        return g

    # -- pre-processing ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def preprocess(self, crops: Sequence[torch.Tensor]) -> torch.Tensor:
        """Line crops u8 [h, w, 3] (device) -> u8 [N, S, S, 3]: convert("L").convert("RGB"), then Pillow BILINEAR to image_size²."""
        S = self.cfg.image_size
        lib, st = _lib.load(), C.c_void_p(ops.current_stream())
        out = torch.empty(len(crops), S, S, 3, dtype=torch.uint8, device=self.device)
        for i, crop in enumerate(crops):
            if crop.dtype != torch.uint8 or crop.dim() != 3 or crop.shape[2] != 3 or crop.numel() == 0:
                raise ValueError(f"MocrEngine.preprocess expects u8 [h,w,3] crops, got {crop.dtype} {tuple(crop.shape)}")
            crop = crop.to(self.device).contiguous()
            gray = torch.empty_like(crop)
            _lib.check(lib.mit_mocr_gray(crop.data_ptr(), crop.shape[0] * crop.shape[1], gray.data_ptr(), st), "mit_mocr_gray")
            out[i] = imgproc.pil_resize_u8(gray[None], (S, S), "bilinear")[0]
        return out

    def patch_rows(self, images_u8: torch.Tensor) -> torch.Tensor:
        """u8 [N, S, S, 3] -> fp32 [N, (S / ps)², 3 ps ps] normalised patch rows (mit_mocr_patches)."""
        c = self.cfg
        S, ps = c.image_size, c.patch_size
        if images_u8.dtype != torch.uint8 or tuple(images_u8.shape[1:]) != (S, S, 3):
            raise ValueError(f"MocrEngine expects u8 [N,{S},{S},3], got {images_u8.dtype} {tuple(images_u8.shape)}")
        images_u8 = images_u8.contiguous()
        N, G = images_u8.shape[0], S // ps
        rows = torch.empty(N, G * G, 3 * ps * ps, device=self.device)
        _lib.check(_lib.load().mit_mocr_patches(images_u8.data_ptr(), N, S, ps, rows.data_ptr(), C.c_void_p(ops.current_stream())), "mit_mocr_patches")
        return rows

    # -- encoder ----------------------------------------------------------------------------------------------------------------------
    def _ln(self, src, wb, dst, eps):
        _lib.check(_lib.load().mit_layernorm_wide(src.data_ptr(), src.stride(0), wb[0].data_ptr(), wb[1].data_ptr(), dst.data_ptr(), dst.stride(0),
                                                  src.shape[0], src.shape[1], eps, C.c_void_p(ops.current_stream())), "mit_layernorm_wide")

    @torch.no_grad()
    def encode(self, images_u8: torch.Tensor, taps: Optional[dict] = None):
        """u8 [N, S, S, 3] -> (mem_k, mem_v) [dec_layers, N, tokens, dec_hidden]; ``taps['memory']``: the encoder states the decoder reads."""
        c = self.cfg
        rows = self.patch_rows(images_u8)
        N, P, _ = rows.shape
        H, L, nx = c.enc_hidden, c.tokens, self.n_extra
        lib, st = _lib.load(), C.c_void_p(ops.current_stream())
        x = self._buf("enc.x", N, L, H)
        x[:, :nx] = self.extra_rows
        for n in range(N):   # patch projection + position embedding (post operand) straight into the token rows
            self.patch(rows[n], x[n, nx:], post=self.patch_pos)
        M = N * L
        x = x.view(M, H)
        h, y = self._buf("enc.h", M, H), self._buf("enc.y", M, H)
        qkv, att, ffh = self._buf("enc.qkv", 3, M, H), self._buf("enc.att", M, H), self._buf("enc.ffh", M, c.enc_inter)
        LH = L * H
        for ly in self.enc:   # pre-LN: x += o(attn(ln1(x))); x += fc2(gelu(fc1(ln2(x))))
            self._ln(x, ly["ln1"], h, c.enc_eps)
            ly["qkv"](h, qkv[0], nsplit=H, nhi=M * H)
            _lib.check(lib.mit_attention_heads(qkv[0].data_ptr(), LH, H, qkv[1].data_ptr(), LH, H, qkv[2].data_ptr(), LH, H, att.data_ptr(), LH, H,
                                               None, N, L, L, 1, c.enc_heads, H // c.enc_heads, st), "mit_attention_heads")
            ly["out"](att, y, post=x)
            self._ln(y, ly["ln2"], h, c.enc_eps)
            ly["ff1"](h, ffh, act=ACT_GELU)
            ly["ff2"](ffh, x, post=y)
        self._ln(x, self.enc_ln, h, c.enc_eps)
        mem = h
        if self.enc_to_dec is not None:
            mem = self.enc_to_dec(h, self._buf("enc.proj", M, c.dec_hidden))
        if taps is not None:
            taps["memory"] = mem.reshape(N, L, c.dec_hidden).clone()
        D = c.dec_hidden
        mem_k = torch.empty(c.dec_layers, N, L, D, device=self.device)
        mem_v = torch.empty(c.dec_layers, N, L, D, device=self.device)
        for l in range(c.dec_layers):   # one GEMM: K columns land in mem_k[l], V columns in mem_v[l]
            self.mem_kv[l](mem, mem_k[l].view(M, D), nsplit=D, nhi=(mem_v[l].data_ptr() - mem_k[l].data_ptr()) // 4)
        return mem_k, mem_v

    # -- decoder ----------------------------------------------------------------------------------------------------------------------
    def _args(self, N: int, g: GenerationParams, hidden: int, inter: int, layers: int, vocab: Optional[int] = None):
        nbytes = _lib.load().mit_mocr_decode_workspace_bytes(N, g.num_beams, g.max_length, hidden, inter, self.cfg.vocab if vocab is None else vocab, layers)
        ws = self._buf("decode.ws", nbytes, dtype=torch.uint8)
        a = MitMocrDecodeArgs()
        a.N, a.num_beams, a.max_length = N, g.num_beams, g.max_length
        a.no_repeat_ngram_size, a.early_stopping, a.length_penalty = g.no_repeat_ngram_size, int(bool(g.early_stopping)), float(g.length_penalty)
        a.eos_token_id, a.pad_token_id, a.decoder_start_token_id = g.eos_token_id, _fill_token(g), g.decoder_start_token_id
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        dev = self.device
        out = dict(tokens=torch.zeros(N, g.max_length, dtype=torch.int32, device=dev), length=torch.zeros(N, dtype=torch.int32, device=dev),
                   score=torch.zeros(N, dtype=torch.float32, device=dev))
        a.res_tok, a.res_len, a.res_score = (out[k].data_ptr() for k in ("tokens", "length", "score"))
        return a, out

    @torch.no_grad()
    def decode(self, mem_k: torch.Tensor, mem_v: torch.Tensor, generation: Optional[GenerationParams] = None, trace: bool = False,
               tiled: bool = False):
        """``generate`` over N lines at once.  Returns device tensors tokens [N, max_length] (padded), length [N], score [N]
        (``sequences_scores``) (+ trace_logits [max_length - 1, N * beams, V]: log-probabilities after the logits processors, trace_hist
        [max_length - 1, N * beams, max_length] when ``trace``) and steps_run.  ``tiled``: every Linear of a step on the tiled GEMM
        (MitMocrDecodeArgs.form; tests compare the two)."""
        c = self.cfg
        g = self.generation if generation is None else self._checked(generation)
        _, N, L, _ = mem_k.shape
        a, out = self._args(N, g, c.dec_hidden, c.dec_inter, c.dec_layers)
        a.L, a.form = L, 1 if tiled else 0
        mem_k, mem_v = mem_k.contiguous(), mem_v.contiguous()
        a.mem_k, a.mem_v = mem_k.data_ptr(), mem_v.data_ptr()
        if trace:
            R = N * g.num_beams
            out["trace_logits"] = torch.zeros(g.max_length - 1, R, c.vocab, device=self.device)
            out["trace_hist"] = torch.zeros(g.max_length - 1, R, g.max_length, dtype=torch.int32, device=self.device)
            a.trace_logits, a.trace_hist = out["trace_logits"].data_ptr(), out["trace_hist"].data_ptr()
        _lib.check(_lib.load().mit_mocr_decode(C.byref(self.dec), C.byref(a), C.c_void_p(ops.current_stream())), "mit_mocr_decode")
        out["steps_run"], out["form_run"] = a.steps_run, a.form_run
        return out

    def lines_per_call(self, generation: Optional[GenerationParams] = None) -> int:
        """How many lines one decode call takes under ``max_workspace_bytes`` (at least one)."""
        c, g = self.cfg, self.generation if generation is None else generation
        size = lambda n: _lib.load().mit_mocr_decode_workspace_bytes(n, g.num_beams, g.max_length, c.dec_hidden, c.dec_inter, c.vocab, c.dec_layers)
        per_line = size(2) - size(1)
        return max(1, int((self.max_workspace_bytes - (size(1) - per_line)) // max(per_line, 1)))

    @torch.no_grad()
    def decode_chunked(self, mem_k: torch.Tensor, mem_v: torch.Tensor, generation: Optional[GenerationParams] = None):
        """decode() over any number of lines, ``lines_per_call`` at a time: tokens / length / score concatenated, steps_run the largest."""
        N, step = mem_k.shape[1], self.lines_per_call(generation)
        if N <= step:
            return self.decode(mem_k, mem_v, generation)
        parts = []
        for i in range(0, N, step):
            o = self.decode(mem_k[:, i:i + step], mem_v[:, i:i + step], generation)
            parts.append(o)
        out = {k: torch.cat([p[k] for p in parts]) for k in ("tokens", "length", "score")}
        out["steps_run"], out["form_run"], out["calls"] = max(p["steps_run"] for p in parts), parts[0]["form_run"], len(parts)
        return out

    @torch.no_grad()
    def beam_replay(self, logp: torch.Tensor, n_lines: int, generation: GenerationParams):
        """The decoder's bookkeeping kernels alone on log-probability tables [steps, n_lines * beams, V] (mit_mocr_beam_replay)."""
        g = generation
        steps, R, V = (int(s) for s in logp.shape)
        if R != n_lines * g.num_beams:
            raise ValueError(f"beam_replay expects [steps, {n_lines * g.num_beams}, V] tables, got {tuple(logp.shape)}")
        logp = logp.to(self.device, torch.float32).contiguous()
        a, out = self._args(n_lines, g, 0, 0, 0, vocab=V)
        out["trace_hist"] = torch.zeros(steps, R, g.max_length, dtype=torch.int32, device=self.device)
        a.trace_hist = out["trace_hist"].data_ptr()
        _lib.check(_lib.load().mit_mocr_beam_replay(logp.data_ptr(), steps, V, C.byref(a), C.c_void_p(ops.current_stream())), "mit_mocr_beam_replay")
        out["steps_run"] = a.steps_run
        return out

    # -- whole lines ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def recognize(self, crops: Sequence, generation: Optional[GenerationParams] = None):
        """Line crops u8 [h, w, 3] (numpy or tensors) -> decode()'s dict."""
        crops = [torch.from_numpy(np.ascontiguousarray(cr)) if isinstance(cr, np.ndarray) else cr for cr in crops]
        mem_k, mem_v = self.encode(self.preprocess(crops))
        return self.decode_chunked(mem_k, mem_v, generation)

    @torch.no_grad()
    def line_crops(self, page_u8: torch.Tensor, quads, directions) -> List[torch.Tensor]:
        """model_manga_ocr.py:153-160: every line is rectified in direction 'h' at text height = its box's own width ('h') or height
        ('v') — faithful to the reference, odd as it is."""
        if page_u8.dtype != torch.uint8 or page_u8.dim() != 4 or page_u8.shape[0] != 1 or page_u8.shape[-1] != 3:
            raise ValueError(f"recognize_lines expects u8 [1,H,W,3], got {page_u8.dtype} {tuple(page_u8.shape)}")
        page_u8 = page_u8.contiguous()
        H, W = int(page_u8.shape[1]), int(page_u8.shape[2])
        crops = []
        for q, d in zip(quads, directions):
            if d not in ("h", "v"):
                raise ValueError(f"direction must be 'h' or 'v', got {d!r}")
            keep = getattr(q, "assigned_direction", None)
            plan = TL.warp_plan(q, "h", H, W, textheight=q.aabb.w if d == "h" else q.aabb.h)
            q.assigned_direction = keep
            rec = np.zeros(1, dtype=TL.WARP_LINE_DTYPE)
            rec["minv"] = plan.minv.reshape(1, 9)
            rec["x1"], rec["y1"], rec["cw"], rec["ch"], rec["dw"], rec["dh"] = plan.x1, plan.y1, plan.cw, plan.ch, plan.dw, plan.dh
            crops.append(TL.rectify(page_u8, rec, plan.dh, plan.dw)[0])
        return crops

    @torch.no_grad()
    def recognize_lines(self, page_u8: torch.Tensor, quads, directions, generation: Optional[GenerationParams] = None):
        """page_u8 [1,H,W,3] u8 (device); quads = textline.Quadrilateral list, directions per quad -> decode()'s dict, row i = quad i."""
        if len(quads) == 0:
            return dict(tokens=None)
        mem_k, mem_v = self.encode(self.preprocess(self.line_crops(page_u8, quads, directions)))
        return self.decode_chunked(mem_k, mem_v, generation)
