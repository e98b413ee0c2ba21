"""32px OCR (``--ocr 32px``) on the gfx950 engine: FAN ResNet backbone, post-norm encoder, native beam decoder.

Same model as ``OCR`` of the reference (manga_translator/ocr/model_32px.py:467-595):
  backbone (:143-234, blocks [3, 6, 7, 5]) -> + pe -> 3 x nn.TransformerEncoderLayer (:474-476, key mask :523-528)
  -> beam search over 2 x nn.TransformerDecoderLayer (:415-465, :529-595).

MI355X layout
* the backbone is ``ocr_ctc.FanBackbone`` (the 48px_ctc model's blocks with other counts, input height 32 and 2 x 2 tail convs); the
  positional table is added to the features — residual stream included — in conv4_2's epilogue (``post`` map with batch stride 0);
* every padded key is masked in the encoder and in the cross-attention (the 48px_ctc model masks nothing), so a line's result does not
  depend on its chunk: chunks are encoded one by one (their padded widths differ), all lines of a page are decoded in one native loop
  (mit_ocr32_decode);
* q-scaling (head_dim ** -0.5) is a column scale of the projection's epilogue; BatchNorm folded into conv epilogues as in ocr_ctc.py.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import lib as _lib
from . import ops
from . import textline as TL
from .lib import MitOcr32DecodeArgs, MitOcr32Decoder
from .ocr48 import Linear
from .ocr_ctc import FanBackbone
from .ocr32_schema import COLOR_HEADS, LAYERS
from .ops import ACT_RELU

EMBD, HEADS, HEAD_DIM, FF = 320, 4, 80, 2048
N_ENC, N_DEC = 3, 2
TEXT_HEIGHT = 32


def _in_proj(sd, p, device, part: slice, scaled: bool):
    w, b = sd[p + ".in_proj_weight"].float()[part], sd[p + ".in_proj_bias"].float()[part]
    sc = None
    if scaled:   # F.multi_head_attention_forward scales q (bias included) by head_dim ** -0.5; k | v columns (if any) stay
        sc = torch.cat([torch.full((EMBD,), HEAD_DIM ** -0.5), torch.ones(w.shape[0] - EMBD)])
    return Linear(w, b, device, sc)


class Ocr32Engine(ops.Engine):
    """encode(): u8 line crops of one chunk -> cross-attention K / V of the encoder memory; decode(): beam search over any number of
    lines; recognize_lines(): a page's quads -> tokens / probabilities / colours in the reference's processing order."""

    def __init__(self, sd: Dict[str, torch.Tensor], dict_size: int, device="cuda"):
        super().__init__(device)
        dev = self.device
        self.dict_size = dict_size
        self.backbone = FanBackbone(sd, dev, LAYERS, 2)
        pe = sd["pe.pe"].detach().float().reshape(-1, EMBD)
        self.pe = pe.to(dev).contiguous()                                   # [768, 320]
        ln = lambda p: (sd[p + ".weight"].float().to(dev), sd[p + ".bias"].float().to(dev))
        lin = lambda p: Linear(sd[p + ".weight"], sd[p + ".bias"], dev)
        self.enc = []
        for i in range(N_ENC):
            q = f"encoders.layers.{i}"
            self.enc.append(dict(qkv=_in_proj(sd, q + ".self_attn", dev, slice(0, 3 * EMBD), True), out=lin(q + ".self_attn.out_proj"),
                                 ff1=lin(q + ".linear1"), ff2=lin(q + ".linear2"), ln=[ln(f"{q}.norm{j}") for j in (1, 2)]))
        self._keep: List = []
        d = MitOcr32Decoder()
        self.mem_kv = []
        for l in range(N_DEC):
            p = f"decoders.layers.{l}"
            lins = dict(qkv=_in_proj(sd, p + ".self_attn", dev, slice(0, 3 * EMBD), True), out=lin(p + ".self_attn.out_proj"),
                        q2=_in_proj(sd, p + ".multihead_attn", dev, slice(0, EMBD), True), out2=lin(p + ".multihead_attn.out_proj"),
                        ff1=lin(p + ".linear1"), ff2=lin(p + ".linear2"))
            self._keep.append(lins)
            ly = d.layers[l]
            for k, v in lins.items():
                setattr(ly, k, v.c_struct())
            for i in (1, 2, 3):
                wt, bt = ln(f"{p}.norm{i}")
                self._keep += [wt, bt]
                setattr(ly, f"ln{i}_w", wt.data_ptr())
                setattr(ly, f"ln{i}_b", bt.data_ptr())
            # cross-attention K | V projection of the encoder memory: once per line at encode time
            self.mem_kv.append(_in_proj(sd, p + ".multihead_attn", dev, slice(EMBD, 3 * EMBD), False))
        self.embd = sd["embd.weight"].detach().float().to(dev).contiguous()
        self.pred1 = lin("pred1.0")
        self.pred = lin("pred")
        self.color1 = lin("color_pred1.0")
        self.color_heads = Linear(torch.cat([sd[h + ".weight"] for h in COLOR_HEADS], 0), torch.cat([sd[h + ".bias"] for h in COLOR_HEADS], 0), dev)
        d.embd, d.pe = self.embd.data_ptr(), self.pe.data_ptr()
        d.pred1, d.pred = self.pred1.c_struct(), self.pred.c_struct()
        d.color1, d.color_heads = self.color1.c_struct(), self.color_heads.c_struct()
        d.dict_size, d.pe_len = dict_size, self.pe.shape[0]
        self.dec = d

    @staticmethod
    def valid_len(width: int, L: int) -> int:
        """Unmasked memory positions of a line (:523)."""
        return min((width + 3) // 4 + 2, L)

    def memory_len(self, Wp: int) -> int:
        return self.backbone.out_width(Wp)

    @torch.no_grad()
    def encode(self, region_u8: torch.Tensor, widths: Sequence[int], taps: Optional[dict] = None):
        """One reference chunk (:519-528): region_u8 [N,32,Wp,3] u8 (device), widths of the unpadded crops.
        Returns (mem_k [2,N,L,320], mem_v [2,N,L,320], mem_len [N] int32, L)."""
        if region_u8.dtype != torch.uint8 or region_u8.dim() != 4 or region_u8.shape[1] != TEXT_HEIGHT or region_u8.shape[3] != 3:
            raise ValueError(f"Ocr32Engine.encode expects u8 [N,32,Wp,3], got {region_u8.dtype} {tuple(region_u8.shape)}")
        region_u8 = region_u8.contiguous()
        N, _, Wp, _ = region_u8.shape
        lib = _lib.load()
        st = C.c_void_p(ops.current_stream())
        x = self._buf("in", N, TEXT_HEIGHT, Wp, 4)
        _lib.check(lib.mit_ocr_prep(region_u8.data_ptr(), x.data_ptr(), N, TEXT_HEIGHT, Wp, st), "mit_ocr_prep")
        L = self.memory_len(Wp)
        if L > self.pe.shape[0]:
            raise ValueError(f"line of {Wp} px gives {L} memory positions, the positional table has {self.pe.shape[0]}")
        if taps is not None:   # the features before the positional table (a second backbone run: tests only)
            taps["backbone"] = self.backbone(x, self._buf).reshape(N, L, EMBD).clone()
        # feats + pe[:T] (:527), added to conv4_2's output in its epilogue
        feat = self.backbone(x, self._buf, post=self.pe[:L].view(1, 1, L, EMBD).expand(N, 1, L, EMBD))
        if tuple(feat.shape) != (N, 1, L, EMBD):
            raise RuntimeError(f"backbone output {tuple(feat.shape)} != {(N, 1, L, EMBD)}")
        M = N * L
        mem = feat.reshape(M, EMBD)
        klen = torch.tensor([self.valid_len(w, L) for w in widths], dtype=torch.int32).to(self.device)
        qkv = self._buf("qkv", 3, M, EMBD)
        att = self._buf("att", M, EMBD)
        y = self._buf("y", M, EMBD)
        ffh = self._buf("ffh", M, FF)
        ln = lambda src, wb, dst: _lib.check(lib.mit_layernorm(src.data_ptr(), src.stride(0), wb[0].data_ptr(), wb[1].data_ptr(),
                                                               dst.data_ptr(), dst.stride(0), M, EMBD, 1e-5, st), "mit_layernorm")
        LE = L * EMBD
        for ly in self.enc:   # nn.TransformerEncoderLayer, norm_first False: x = norm1(x + sa(x)); x = norm2(x + ff(x))
            ly["qkv"](mem, qkv[0], nsplit=EMBD, nhi=M * EMBD)
            _lib.check(lib.mit_attention(qkv[0].data_ptr(), LE, EMBD, qkv[1].data_ptr(), LE, EMBD, qkv[2].data_ptr(), LE, EMBD,
                                         att.data_ptr(), LE, EMBD, klen.data_ptr(), N, L, L, 1, st), "mit_attention")
            ly["out"](att, y, post=mem)
            ln(y, ly["ln"][0], mem)
            ly["ff1"](mem, ffh, act=ACT_RELU)
            ly["ff2"](ffh, y, post=mem)
            ln(y, ly["ln"][1], mem)
        if taps is not None:
            taps["memory"] = mem.reshape(N, L, EMBD).clone()
        mem_k = torch.empty(N_DEC, N, L, EMBD, device=self.device)
        mem_v = torch.empty(N_DEC, N, L, EMBD, device=self.device)
        for l in range(N_DEC):   # one GEMM: K columns land in mem_k[l], V columns in mem_v[l] (column split with a plane offset)
            self.mem_kv[l](mem, mem_k[l].view(M, EMBD), nsplit=EMBD, nhi=(mem_v[l].data_ptr() - mem_k[l].data_ptr()) // 4)
        return mem_k, mem_v, klen, L

    @torch.no_grad()
    def decode(self, mem_k: torch.Tensor, mem_v: torch.Tensor, mem_len: torch.Tensor, max_seq_length: int = 255, trace: bool = False,
               max_finished: int = 2, tiled: bool = False):
        """Beam search (:529-595) over N lines at once.  mem_k / mem_v [2,N,L,320], mem_len [N] int32.
        Returns device tensors: tokens [N,T+2] int32, length [N], prob [N], colors [N,T+1,6] (length - 1 valid positions), src [N,T+1]
        (+ trace_logits [T+1,N*5,dict], trace_hist [T+1,N*5,T+2] when ``trace``) and steps_run.  ``tiled``: every Linear of a step on
        the tiled GEMM even where the few-row form applies (MitOcr32DecodeArgs.form; tests compare the two)."""
        _, N, L, _ = mem_k.shape
        T = int(max_seq_length)
        lib = _lib.load()
        dev = self.device
        a = self._args(N, T, max_finished)
        a.L, a.form = L, 1 if tiled else 0
        mem_k, mem_v = mem_k.contiguous(), mem_v.contiguous()
        a.mem_k, a.mem_v, a.mem_len = mem_k.data_ptr(), mem_v.data_ptr(), mem_len.data_ptr()
        out = self._results(a, N, T)
        colors = torch.zeros(N, T + 1, 8, dtype=torch.float32, device=dev)
        a.colors = colors.data_ptr()
        if trace:
            out["trace_logits"] = torch.zeros(T + 1, N * 5, self.dict_size, device=dev)
            out["trace_hist"] = torch.zeros(T + 1, N * 5, T + 2, dtype=torch.int32, device=dev)
            a.trace_logits, a.trace_hist = out["trace_logits"].data_ptr(), out["trace_hist"].data_ptr()
        _lib.check(lib.mit_ocr32_decode(C.byref(self.dec), C.byref(a), C.c_void_p(ops.current_stream())), "mit_ocr32_decode")
        out.update(colors=colors[..., :6], steps_run=a.steps_run)
        return out

    def _args(self, N: int, T: int, max_finished: int) -> MitOcr32DecodeArgs:
        nbytes = _lib.load().mit_ocr32_decode_workspace_bytes(N, T, self.dict_size)
        ws = self._buf("decode.ws", nbytes, dtype=torch.uint8)
        a = MitOcr32DecodeArgs()
        a.N, a.max_seq_length, a.start_tok, a.end_tok, a.max_finished = N, T, 1, 2, max_finished
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        return a

    def _results(self, a: MitOcr32DecodeArgs, N: int, T: int) -> dict:
        dev = self.device
        out = dict(tokens=torch.zeros(N, T + 2, dtype=torch.int32, device=dev), length=torch.zeros(N, dtype=torch.int32, device=dev),
                   prob=torch.zeros(N, dtype=torch.float32, device=dev), src=torch.zeros(N, T + 1, dtype=torch.int32, device=dev))
        a.res_tok, a.res_len, a.res_prob, a.res_src = (out[k].data_ptr() for k in ("tokens", "length", "prob", "src"))
        return out

    @torch.no_grad()
    def beam_replay(self, vals: torch.Tensor, idx: torch.Tensor, n_lines: int, max_seq_length: int, max_finished: int = 2):
        """The decoder's bookkeeping kernels alone on given top-5 tables vals / idx [steps, n_lines * 5, 5] (mit_ocr32_beam_replay)."""
        steps = int(vals.shape[0])
        T = int(max_seq_length)
        vals = vals.to(self.device, torch.float32).contiguous()
        idx = idx.to(self.device, torch.int32).contiguous()
        if tuple(vals.shape) != (steps, n_lines * 5, 5) or tuple(idx.shape) != tuple(vals.shape):
            raise ValueError(f"beam_replay expects [steps, {n_lines * 5}, 5] tables, got {tuple(vals.shape)} / {tuple(idx.shape)}")
        a = self._args(n_lines, T, max_finished)
        out = self._results(a, n_lines, T)
        out["trace_hist"] = torch.zeros(steps, n_lines * 5, T + 2, dtype=torch.int32, device=self.device)
        a.trace_hist = out["trace_hist"].data_ptr()
        _lib.check(_lib.load().mit_ocr32_beam_replay(vals.data_ptr(), idx.data_ptr(), steps, C.byref(a), C.c_void_p(ops.current_stream())),
                   "mit_ocr32_beam_replay")
        out["steps_run"] = a.steps_run
        return out

    # -- Model32pxOCR._infer's batching (:68-87) ---------------------------------------------------------------------
    make_chunks = staticmethod(functools.partial(TL.pack_chunks, height=TEXT_HEIGHT))   # max_w + 7 (:78); no + 128 here

    def decode_chunks(self, encoded, max_seq_length: int, trace: bool = False, tiled: bool = False):
        """Pool the (mem_k, mem_v, mem_len, L) of several chunks (zero-padded to the longest memory; the pad is masked) and decode once."""
        mem_k, mem_v = TL.pool_memories([e[0] for e in encoded]), TL.pool_memories([e[1] for e in encoded])
        return self.decode(mem_k, mem_v, torch.cat([e[2] for e in encoded]), max_seq_length, trace=trace, tiled=tiled)

    @torch.no_grad()
    def recognize(self, region_imgs: List[np.ndarray], max_seq_length: int = 255):
        """Host crops [32, w, 3] u8: per-chunk encode, one pooled decode.  ``order`` = crop index per result row."""
        order, enc = [], []
        for indices, widths, region in self.make_chunks(region_imgs):
            enc.append(self.encode(torch.from_numpy(region).to(self.device), widths))
            order += indices
        out = self.decode_chunks(enc, max_seq_length)
        out["order"] = order
        return out

    @torch.no_grad()
    def recognize_lines(self, page_u8: torch.Tensor, quads, directions, max_seq_length: int = 255, reject=None, ignore_bubble: int = 0):
        """page_u8 [1,H,W,3] u8 (device); quads = textline.Quadrilateral list, directions per quad.  Every line is rectified on the GPU
        at height 32 straight into its chunk tensor, chunks (sorted by crop width, 16 lines, padded to max + 7) are encoded one by one and
        all lines decoded in one pooled beam search.  ``reject(crop u8 [32, w, 3] ndarray) -> bool`` (optional): a rejected line's rows
        are zeroed before encoding and it is still decoded, as the reference's ``continue`` leaves it (:84-86).  ``ignore_bubble`` in
        1..50 (and no ``reject``): the reference's own rule, ``textline.is_ignore``, judged on the device without fetching a crop.
        Returns decode()'s dict plus ``order`` (quad index per result row)."""
        if page_u8.dtype != torch.uint8 or page_u8.dim() != 4 or page_u8.shape[0] != 1 or page_u8.shape[-1] != 3:
            raise ValueError(f"recognize_lines expects u8 [1,H,W,3], got {page_u8.dtype} {tuple(page_u8.shape)}")
        if len(quads) == 0:
            return dict(order=[], tokens=None)
        order, enc = [], []
        for idx, ws, region in TL.rectified_chunks(page_u8.contiguous(), quads, directions, TEXT_HEIGHT, reject=reject,
                                                      ignore_bubble=ignore_bubble):
            enc.append(self.encode(region, ws))
            order += list(idx)
        out = self.decode_chunks(enc, max_seq_length)
        out["order"] = order
        return out
