"""State-dict layout and configuration of the manga-ocr recogniser (``--ocr mocr``).

The model is a HuggingFace ``VisionEncoderDecoderModel``: a ``ViTModel`` / ``DeiTModel`` encoder and a ``BertLMHeadModel`` decoder with
cross-attention (reference: manga_translator/ocr/model_manga_ocr.py:132-295, through the ``manga_ocr`` package).  The names below are the
ones ``VisionEncoderDecoderModel.state_dict()`` of the installed ``transformers`` produces (``encoder.layers.N.attention.q_proj...``,
``decoder.bert.encoder.layer.N.crossattention.self.query...``, ``decoder.cls.predictions.*``); tests/test_mocr_cpu.py pins every name and
shape against that module.  Every size comes from a config dict — the model directory's ``config.json`` — and the generation parameters
from ``generation_config.json`` / ``config.json``: nothing is taken from memory of the published checkpoint.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Any, Dict, Optional

from .synth import Schema

# Gains of the synthetic weights (the precedent is ocr32_schema.EMBD_GAIN): with unit gains the post-LN decoder hands the LM head a
# unit-variance vector and every step is a near-uniform draw over the vocabulary; the gain on the vocabulary Linear spreads the
# log-probabilities so that beams differ.  Tests bias the EOS logit on top of it to end lines (tests/_mocr_oracle.py records the recipe).
HEAD_GAIN = 4.0


@dataclass(frozen=True)
class MocrConfig:
    """Sizes of one model, read from a ``VisionEncoderDecoderConfig`` dict."""
    image_size: int
    patch_size: int
    enc_hidden: int
    enc_heads: int
    enc_layers: int
    enc_inter: int
    enc_eps: float
    deit: bool
    dec_hidden: int
    dec_heads: int
    dec_layers: int
    dec_inter: int
    dec_eps: float
    vocab: int
    max_pos: int
    type_vocab: int

    @property
    def tokens(self) -> int:
        return (self.image_size // self.patch_size) ** 2 + (2 if self.deit else 1)


def _need(d: Dict[str, Any], key: str, what: str):
    if key not in d:
        raise ValueError(f"mocr config: {what} has no {key!r}")
    return d[key]


def config_from_dict(cfg: Dict[str, Any]) -> MocrConfig:
    """``config.json`` of a VisionEncoderDecoderModel -> MocrConfig.  Refuses, by name, what the engine does not implement."""
    enc, dec = _need(cfg, "encoder", "config"), _need(cfg, "decoder", "config")
    et, dt = enc.get("model_type"), dec.get("model_type")
    if et not in ("vit", "deit"):
        raise ValueError(f"mocr config: encoder model_type {et!r} is not implemented (vit, deit)")
    if dt != "bert":
        raise ValueError(f"mocr config: decoder model_type {dt!r} is not implemented (bert)")
    for side, d in (("encoder", enc), ("decoder", dec)):
        if d.get("hidden_act", "gelu") != "gelu":
            raise ValueError(f"mocr config: {side} hidden_act {d.get('hidden_act')!r} is not implemented (gelu)")
    if not enc.get("qkv_bias", True):
        raise ValueError("mocr config: encoder qkv_bias = false is not implemented")
    if dec.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"mocr config: decoder position_embedding_type {dec.get('position_embedding_type')!r} is not implemented (absolute)")
    image_size, patch = _need(enc, "image_size", "encoder"), _need(enc, "patch_size", "encoder")
    if isinstance(image_size, (list, tuple)) or isinstance(patch, (list, tuple)):
        raise ValueError("mocr config: a non-square image_size / patch_size is not implemented")
    if image_size % patch:
        raise ValueError(f"mocr config: image_size {image_size} is no multiple of patch_size {patch}")
    return MocrConfig(
        image_size=int(image_size), patch_size=int(patch), enc_hidden=int(_need(enc, "hidden_size", "encoder")),
        enc_heads=int(_need(enc, "num_attention_heads", "encoder")), enc_layers=int(_need(enc, "num_hidden_layers", "encoder")),
        enc_inter=int(_need(enc, "intermediate_size", "encoder")), enc_eps=float(enc.get("layer_norm_eps", 1e-12)), deit=et == "deit",
        dec_hidden=int(_need(dec, "hidden_size", "decoder")), dec_heads=int(_need(dec, "num_attention_heads", "decoder")),
        dec_layers=int(_need(dec, "num_hidden_layers", "decoder")), dec_inter=int(_need(dec, "intermediate_size", "decoder")),
        dec_eps=float(dec.get("layer_norm_eps", 1e-12)), vocab=int(_need(dec, "vocab_size", "decoder")),
        max_pos=int(_need(dec, "max_position_embeddings", "decoder")), type_vocab=int(dec.get("type_vocab_size", 2)))


def tiny_config_dict(image_size: int = 32, patch_size: int = 16, hidden: int = 64, heads: int = 4, enc_layers: int = 2, dec_layers: int = 2,
                     inter: int = 128, vocab: int = 50, max_pos: int = 40, deit: bool = False, dec_hidden: Optional[int] = None) -> Dict[str, Any]:
    """A ``config.json`` dict of the given sizes (tests, the benchmark script)."""
    dh = hidden if dec_hidden is None else dec_hidden
    return {
        "model_type": "vision-encoder-decoder",
        "encoder": {"model_type": "deit" if deit else "vit", "image_size": image_size, "patch_size": patch_size, "hidden_size": hidden,
                    "num_hidden_layers": enc_layers, "num_attention_heads": heads, "intermediate_size": inter, "hidden_act": "gelu",
                    "layer_norm_eps": 1e-12, "qkv_bias": True, "num_channels": 3},
        "decoder": {"model_type": "bert", "vocab_size": vocab, "hidden_size": dh, "num_hidden_layers": dec_layers, "num_attention_heads": heads,
                    "intermediate_size": inter, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "max_position_embeddings": max_pos,
                    "type_vocab_size": 2, "is_decoder": True, "add_cross_attention": True, "position_embedding_type": "absolute"},
    }


# ---- generation parameters -------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class GenerationParams:
    """What ``generate`` is run with.  The defaults are HuggingFace's own (GenerationConfig): greedy, no ban, length_penalty 1."""
    max_length: int = 20
    num_beams: int = 1
    no_repeat_ngram_size: int = 0
    length_penalty: float = 1.0
    early_stopping: bool = False
    eos_token_id: Optional[int] = None
    pad_token_id: Optional[int] = None
    decoder_start_token_id: Optional[int] = None


# parameter -> the value(s) at which it is off; anything else is refused with an error that names the parameter
_UNSUPPORTED = {
    "do_sample": (False,), "num_beam_groups": (1,), "diversity_penalty": (0.0,), "penalty_alpha": (None,), "top_k": (None, 50), "top_p": (None, 1.0),
    "temperature": (None, 1.0), "typical_p": (None, 1.0), "epsilon_cutoff": (None, 0.0), "eta_cutoff": (None, 0.0), "min_p": (None,),
    "repetition_penalty": (None, 1.0), "encoder_repetition_penalty": (None, 1.0), "encoder_no_repeat_ngram_size": (None, 0),
    "bad_words_ids": (None,), "force_words_ids": (None,), "constraints": (None,), "min_length": (None, 0), "min_new_tokens": (None,),
    "max_new_tokens": (None,), "forced_bos_token_id": (None,), "forced_eos_token_id": (None,), "forced_decoder_ids": (None,),
    "suppress_tokens": (None,), "begin_suppress_tokens": (None,), "sequence_bias": (None,), "exponential_decay_length_penalty": (None,),
    "renormalize_logits": (False,), "remove_invalid_values": (None, False), "guidance_scale": (None, 1.0), "num_return_sequences": (None, 1),
    "prompt_lookup_num_tokens": (None,), "assistant_early_exit": (None,), "dola_layers": (None,), "low_memory": (None, False),
    "max_time": (None,), "stop_strings": (None,), "watermarking_config": (None,), "token_healing": (False,),
}


def generation_from_dicts(*dicts: Dict[str, Any], **overrides) -> GenerationParams:
    """Later dicts win (``config.json``'s decoder / top level, then ``generation_config.json``, then the caller's overrides, e.g. the
    ``max_length=300`` manga_ocr passes to ``generate``).  Sampling, beam groups, penalties, constraints, ``min_length > 0`` and
    ``forced_*`` are refused with a ValueError that names the parameter; so are ``early_stopping = "never"`` and a list of EOS tokens."""
    merged: Dict[str, Any] = {}
    for d in list(dicts) + [overrides]:
        merged.update({k: v for k, v in (d or {}).items() if v is not None})
    for name, off in _UNSUPPORTED.items():
        if name in merged and merged[name] not in off:
            raise ValueError(f"mocr generation: {name} = {merged[name]!r} is not implemented")
    es = merged.get("early_stopping", False)
    if es not in (True, False):
        raise ValueError(f"mocr generation: early_stopping = {es!r} is not implemented (true, false)")
    eos = merged.get("eos_token_id")
    if isinstance(eos, (list, tuple)):
        if len(eos) != 1:
            raise ValueError(f"mocr generation: eos_token_id = {eos!r} (several tokens) is not implemented")
        eos = eos[0]
    fields = {k: merged[k] for k in ("max_length", "num_beams", "no_repeat_ngram_size", "length_penalty", "pad_token_id",
                                     "decoder_start_token_id") if k in merged}
    p = GenerationParams(early_stopping=bool(es), eos_token_id=eos, **fields)
    if p.num_beams < 1 or p.num_beams > 8:
        raise ValueError(f"mocr generation: num_beams = {p.num_beams} is not implemented (1 .. 8)")
    if p.no_repeat_ngram_size < 0 or p.max_length < 2:
        raise ValueError(f"mocr generation: no_repeat_ngram_size = {p.no_repeat_ngram_size} / max_length = {p.max_length} out of range")
    return p


def load_model_dir(model_dir: str, **overrides):
    """(config dict, MocrConfig, GenerationParams) of a model directory: ``config.json`` (+ ``generation_config.json`` when present)."""
    with open(os.path.join(model_dir, "config.json")) as f:
        cfg = json.load(f)
    gen_file = os.path.join(model_dir, "generation_config.json")
    gen = {}
    if os.path.exists(gen_file):
        with open(gen_file) as f:
            gen = json.load(f)
    gen_keys = set(GenerationParams.__dataclass_fields__) | set(_UNSUPPORTED)
    pick = lambda d: {k: v for k, v in d.items() if k in gen_keys}
    # (older checkpoints keep generation parameters inside config.json, at the top level or in the decoder's section)
    return cfg, config_from_dict(cfg), generation_from_dicts(pick(cfg.get("decoder", {})), pick(cfg), pick(gen), **overrides)


# ---- state dict -------------------------------------------------------------------------------------------------------------------

def _lin(p: str, n_out: int, n_in: int, kind: str = "linear") -> Schema:
    return [(p + ".weight", (n_out, n_in), kind), (p + ".bias", (n_out,), "bias")]


def _ln(p: str, n: int) -> Schema:
    return [(p + ".weight", (n,), "ln_w"), (p + ".bias", (n,), "bn_b")]


def mocr_schema(c: MocrConfig, pooler: bool = True) -> Schema:
    H, ps = c.enc_hidden, c.patch_size
    s: Schema = [("encoder.embeddings.cls_token", (1, 1, H), "normal*0.5")]
    s += [("encoder.embeddings.position_embeddings", (1, c.tokens, H), "normal*0.5")]
    if c.deit:
        s += [("encoder.embeddings.distillation_token", (1, 1, H), "normal*0.5")]
    s += [("encoder.embeddings.patch_embeddings.projection.weight", (H, 3, ps, ps), "conv"),
          ("encoder.embeddings.patch_embeddings.projection.bias", (H,), "bias")]
    for i in range(c.enc_layers):
        p = f"encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            s += _lin(f"{p}.attention.{n}", H, H)
        s += _ln(p + ".layernorm_before", H) + _ln(p + ".layernorm_after", H)
        s += _lin(p + ".mlp.fc1", c.enc_inter, H) + _lin(p + ".mlp.fc2", H, c.enc_inter)
    s += _ln("encoder.layernorm", H)
    if pooler:   # unused by the recogniser (add_pooling_layer is irrelevant to last_hidden_state)
        s += _lin("encoder.pooler.dense", H, H)
    D = c.dec_hidden
    e = "decoder.bert.embeddings"
    s += [(e + ".word_embeddings.weight", (c.vocab, D), "normal*0.5"), (e + ".position_embeddings.weight", (c.max_pos, D), "normal*0.5"),
          (e + ".token_type_embeddings.weight", (c.type_vocab, D), "normal*0.5")] + _ln(e + ".LayerNorm", D)
    for i in range(c.dec_layers):
        p = f"decoder.bert.encoder.layer.{i}"
        for a in ("attention", "crossattention"):
            for n in ("query", "key", "value"):
                s += _lin(f"{p}.{a}.self.{n}", D, D)
            s += _lin(f"{p}.{a}.output.dense", D, D) + _ln(f"{p}.{a}.output.LayerNorm", D)
        s += _lin(p + ".intermediate.dense", c.dec_inter, D) + _lin(p + ".output.dense", D, c.dec_inter) + _ln(p + ".output.LayerNorm", D)
    h = "decoder.cls.predictions"
    s += [(h + ".bias", (c.vocab,), "bias")] + _lin(h + ".transform.dense", D, D) + _ln(h + ".transform.LayerNorm", D)
    s += [(h + ".decoder.weight", (c.vocab, D), f"linear*{HEAD_GAIN}"), (h + ".decoder.bias", (c.vocab,), f"tie:{h}.bias")]
    if D != H:
        s += _lin("enc_to_dec_proj", D, H)
    return s
