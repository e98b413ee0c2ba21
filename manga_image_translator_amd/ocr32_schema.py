"""State-dict layout of the reference ``32px`` OCR model (``ocr.ckpt``).

``OCR(dictionary, 768)`` of manga_translator/ocr/model_32px.py:467-489: the FAN pre-activation ResNet of the 48px_ctc
model with block counts [3, 6, 7, 5] and 2 x 2 ``conv4_1`` / ``conv4_2`` (:143-234, :284) -> 3 x ``nn.TransformerEncoderLayer(320, 4)``
-> 2 x ``nn.TransformerDecoderLayer(320, 4)`` (both post-norm, FFN 2048, ReLU); ``pe.pe`` is a registered buffer [768, 1, 320];
``pred.weight`` is tied to ``embd.weight``; ``color_pred1`` + six Linear(64, 1) colour heads.
tests/test_ocr32_cpu.py pins every name and shape against the reference module's own state_dict.
"""
from __future__ import annotations

from .ocr_ctc_schema import resnet_schema
from .synth import Schema

EMBD, FFN, HEADS, N_ENC, N_DEC, MAX_LEN = 320, 2048, 4, 3, 2, 768
LAYERS = [3, 6, 7, 5]
COLOR_HEADS = ("fg_r_pred", "fg_g_pred", "fg_b_pred", "bg_r_pred", "bg_g_pred", "bg_b_pred")
# Gains of the synthetic weights.  With unit gains the decode collapses: the post-norm layers hand `pred` a unit-variance vector and the tied
# embedding (rows of norm 1) turns it into logits of spread ~1, so every step is a near-uniform draw and no line ever ends.  The embedding
# gain makes the top-5 distinct (the precedent is ocr_ctc_schema.CTC_GAIN); the </S> bias is what tests raise to end lines early.
EMBD_GAIN = 4.0


def _mha(p: str) -> Schema:
    return [(p + ".in_proj_weight", (3 * EMBD, EMBD), "linear"), (p + ".in_proj_bias", (3 * EMBD,), "bias"),
            (p + ".out_proj.weight", (EMBD, EMBD), "linear"), (p + ".out_proj.bias", (EMBD,), "bias")]


def _ffn_norms(p: str, n_norms: int) -> Schema:
    s: Schema = [(p + ".linear1.weight", (FFN, EMBD), "linear"), (p + ".linear1.bias", (FFN,), "bias"),
                 (p + ".linear2.weight", (EMBD, FFN), "linear"), (p + ".linear2.bias", (EMBD,), "bias")]
    for j in range(1, n_norms + 1):
        s += [(f"{p}.norm{j}.weight", (EMBD,), "ln_w"), (f"{p}.norm{j}.bias", (EMBD,), "bn_b")]
    return s


def ocr32_schema(dict_size: int) -> Schema:
    s = resnet_schema(layers=LAYERS, tail_kernel=2)
    for i in range(N_ENC):
        p = f"encoders.layers.{i}"
        s += _mha(p + ".self_attn") + _ffn_norms(p, 2)
    for i in range(N_DEC):
        p = f"decoders.layers.{i}"
        s += _mha(p + ".self_attn") + _mha(p + ".multihead_attn") + _ffn_norms(p, 3)
    s += [("pe.pe", (MAX_LEN, 1, EMBD), "sinus_pe_t"),
          ("embd.weight", (dict_size, EMBD), f"embed*{EMBD_GAIN}"),
          ("pred1.0.weight", (EMBD, EMBD), "linear"), ("pred1.0.bias", (EMBD,), "bias"),
          ("pred.weight", (dict_size, EMBD), "tie:embd.weight"), ("pred.bias", (dict_size,), "bias"),
          ("color_pred1.0.weight", (64, EMBD), "linear"), ("color_pred1.0.bias", (64,), "bias")]
    for h in COLOR_HEADS:
        s += [(h + ".weight", (1, 64), "linear*0.3"), (h + ".bias", (1,), "bias*8.0")]
    return s
