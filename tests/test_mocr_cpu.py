"""The restatement the manga-ocr GPU tests compare against (tests/_mocr_oracle.py) pinned to HuggingFace itself — ``transformers``'
VisionEncoderDecoderModel (ViT / DeiT + BertLMHeadModel), its ``generate`` and ViTImageProcessor — on seeded tiny models; the schema;
the refusals; the plugin's aggregation; the serving key.  No GPU."""
import asyncio
import dataclasses
import itertools
import types

import numpy as np
import pytest
import torch

import _mocr_oracle as O
from manga_image_translator_amd import mocr_schema as S

transformers = pytest.importorskip("transformers")

T_MAX = 16
# (seed, eos_bias, embed_scale) of the two models every generation setting runs on (the recipe: tests/_mocr_oracle.py)
HF_MODELS = {"a": (0, 7.0, 1.0), "b": (1, 8.0, 1.5)}


def _hf_model(cfg, sd):
    from transformers import VisionEncoderDecoderConfig, VisionEncoderDecoderModel

    cfg = dict(cfg, decoder=dict(cfg["decoder"], tie_word_embeddings=False))   # the seeded vocabulary Linear is its own tensor
    hc = VisionEncoderDecoderConfig(**cfg)
    hc.tie_word_embeddings = False
    m = VisionEncoderDecoderModel(hc).double().eval()
    m.load_state_dict(sd, strict=True)
    return m


@pytest.fixture(scope="module")
def hf_models():
    out = {}
    for tag, (seed, bias, scale) in HF_MODELS.items():
        cfg, c, sd = O.make_case(seed, bias, embed_scale=scale, vocab=50, max_pos=40)
        pv = O.pixel_values(O.make_crops(3, seed), c.image_size).double()
        with torch.no_grad():
            mem = O.encode(sd, c, pv)
        out[tag] = (_hf_model(cfg, sd), c, sd, pv, mem)
    return out


@pytest.mark.parametrize("kw", [dict(), dict(deit=True, dec_hidden=32), dict(image_size=48, vocab=97)], ids=["vit", "deit_proj", "vit48"])
def test_schema_is_the_state_dict_of_the_huggingface_model(kw):
    from transformers import VisionEncoderDecoderConfig, VisionEncoderDecoderModel

    cfg = S.tiny_config_dict(**kw)
    c = S.config_from_dict(cfg)
    hf = {k: tuple(v.shape) for k, v in VisionEncoderDecoderModel(VisionEncoderDecoderConfig(**cfg)).state_dict().items()}
    ours = {n: tuple(shape) for n, shape, _ in S.mocr_schema(c)}
    assert ours == hf
    assert c.tokens == hf["encoder.embeddings.position_embeddings"][1]
    optional = {n for n in ours if n.startswith("encoder.pooler.")}
    assert {n for n, _, _ in S.mocr_schema(c, pooler=False)} == set(ours) - optional and len(optional) == 2


@pytest.mark.parametrize("kw", [dict(vocab=50, max_pos=40), dict(deit=True, dec_hidden=32, vocab=48, max_pos=32)], ids=["vit", "deit_proj"])
def test_encoder_states_and_teacher_forced_logits(kw):
    cfg, c, sd = O.make_case(5, 2.0, **kw)
    m = _hf_model(cfg, sd)
    pv = O.pixel_values(O.make_crops(3, 5), c.image_size).double()
    toks = torch.randint(0, c.vocab, (3, 9), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want_enc = m.encoder(pixel_values=pv).last_hidden_state
        want_mem = m.enc_to_dec_proj(want_enc) if hasattr(m, "enc_to_dec_proj") and c.enc_hidden != c.dec_hidden else want_enc
        mem = O.encode(sd, c, pv)
        assert (mem - want_mem).abs().max().item() < 1e-10
        want = m.decoder(input_ids=toks, encoder_hidden_states=want_mem).logits
        assert (O.decoder_logits(sd, c, toks, mem) - want).abs().max().item() < 1e-10


SETTINGS = list(itertools.product((1, 4), (0, 3), (0.0, 1.0, 2.0), (True, False)))


@pytest.fixture(scope="module")
def hf_record(hf_models):
    """(model, num_beams, ngram, length_penalty, early_stopping) -> (oracle result, HuggingFace sequences padded, sequences_scores or
    None): every setting on both models, computed once for the tests below."""
    from transformers import GenerationConfig

    rec = {}
    for tag, (m, c, sd, pv, mem) in hf_models.items():
        for nb, ngram, lp, es in SETTINGS:
            got = O.generate(sd, c, mem, O.gen_params(nb, ngram, lp, es, max_length=T_MAX))
            hg = GenerationConfig(max_length=T_MAX, num_beams=nb, no_repeat_ngram_size=ngram, length_penalty=lp, early_stopping=es, eos_token_id=O.EOS,
                                  pad_token_id=O.PAD, decoder_start_token_id=O.START, do_sample=False, return_dict_in_generate=True, output_scores=True)
            with torch.no_grad():
                h = m.generate(pv, generation_config=hg)
            seq = torch.full((3, T_MAX), O.PAD)
            seq[:, :h.sequences.shape[1]] = h.sequences
            rec[(tag, nb, ngram, lp, es)] = (got, seq, h.sequences_scores.double() if nb > 1 else None)
    return rec


@pytest.mark.parametrize("nb, ngram, lp, es", SETTINGS)
def test_generate_agrees_with_huggingface(hf_record, nb, ngram, lp, es):
    """Tokens (padded) and ``sequences_scores`` (beam search; greedy search reports none) for every setting, on both models.  Scores:
    HuggingFace sums fp32 log-probabilities in fp32, the oracle in float64 — 16 terms of magnitude < 16 at 6e-8 relative give 2e-5."""
    for tag in HF_MODELS:
        got, seq, scores = hf_record[(tag, nb, ngram, lp, es)]
        assert torch.equal(seq, got["tokens"]), (tag, seq.tolist(), got["tokens"].tolist())
        if scores is not None:
            assert (scores - got["score"]).abs().max().item() < 2e-5


def test_the_fixture_conditions_hold(hf_record):
    """Over all settings: a line ends by EOS before max_length, one runs to max_length, two lines of one batch end at different steps,
    and the n-gram ban changes the tokens of a line."""
    assert len(hf_record) == 2 * len(SETTINGS)
    lens = {k: got["length"].tolist() for k, (got, _, _) in hf_record.items()}
    flat = [l for ls in lens.values() for l in ls]
    assert any(l < T_MAX for l in flat) and any(l == T_MAX for l in flat)
    assert any(len(set(ls)) > 1 for ls in lens.values())
    assert any(not torch.equal(hf_record[(tag, nb, 0, lp, es)][0]["tokens"], hf_record[(tag, nb, 3, lp, es)][0]["tokens"])
               for tag, nb, ng, lp, es in hf_record if ng == 0)


def test_a_pad_token_of_zero_is_filled_the_way_huggingface_fills_it(hf_models):
    """Beam search fills with ``pad_token_id or eos_token_id``: the engine passes that token down (mocr._fill_token)."""
    from transformers import GenerationConfig

    from manga_image_translator_amd import mocr

    m, c, sd, pv, mem = hf_models["a"]
    g = dataclasses.replace(O.gen_params(4, 0, 1.0, True, max_length=T_MAX), pad_token_id=0)
    assert mocr._fill_token(g) == O.EOS and mocr._fill_token(dataclasses.replace(g, num_beams=1)) == 0
    got = O.generate(sd, c, mem, dataclasses.replace(g, pad_token_id=mocr._fill_token(g)))
    with torch.no_grad():
        h = m.generate(pv, generation_config=GenerationConfig(max_length=T_MAX, num_beams=4, length_penalty=1.0, early_stopping=True, eos_token_id=O.EOS,
                                                              pad_token_id=0, decoder_start_token_id=O.START, do_sample=False))
    assert torch.equal(h, got["tokens"][:, :h.shape[1]]) and (got["length"] < T_MAX).any()


@pytest.mark.parametrize("name", list(O.CASES))
def test_gpu_cases_are_decisive(name):
    """The cases of tests/test_mocr_gpu.py give the same tokens and beam histories in float32 and float64."""
    a, b = O.run_case(name, torch.float64), O.run_case(name, torch.float32)
    assert torch.equal(a["tokens"], b["tokens"]) and a["hist"].shape == b["hist"].shape and torch.equal(a["hist"], b["hist"])
    assert a["done_step"] == b["done_step"]


def test_the_cases_cover_what_they_are_for():
    done = {n: O.run_case(n)["done_step"] for n in ("vit32", "early", "tomax", "greedy")}
    assert min(done["early"]) <= 1                                   # a line that finishes at step 1
    assert len(set(done["vit32"])) > 1 and len(set(done["greedy"])) > 1      # lines of one batch end at different steps
    kw, _, _, _, _, gkw = O.CASES["tomax"]
    assert all(d == gkw["max_length"] - 2 for d in done["tomax"])   # every line runs to max_length


@pytest.mark.parametrize("hw", [(2, 2), (17, 300), (300, 17), (224, 224), (40, 90)])
def test_preprocessing_against_pillow_and_the_image_processor(hw):
    from PIL import Image
    from transformers import ViTImageProcessor

    S_ = 48
    crop = np.random.default_rng(hw[1]).integers(0, 256, size=(*hw, 3), dtype=np.uint8)
    pil = Image.fromarray(crop).convert("L").convert("RGB")
    assert np.array_equal(O.gray_rgb(crop), np.asarray(pil))                      # byte for byte
    proc = ViTImageProcessor(size={"height": S_, "width": S_}, resample=Image.BILINEAR, image_mean=[0.5] * 3, image_std=[0.5] * 3)
    want = torch.as_tensor(np.asarray(proc(pil, return_tensors="pt").pixel_values))[0]
    u8 = O.preprocess(crop, S_)
    assert np.array_equal(u8, np.asarray(pil.resize((S_, S_), Image.BILINEAR)))  # byte for byte before the float step
    got = O.normalize(u8)
    assert got.shape == want.shape and (got - want.float()).abs().max().item() <= 2.4e-7     # 2 ulp of a value in [-1, 1]


# ---- configuration ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, value", [("do_sample", True), ("num_beam_groups", 2), ("repetition_penalty", 1.2), ("min_length", 3),
                                         ("forced_eos_token_id", 3), ("forced_bos_token_id", 2), ("bad_words_ids", [[5]]), ("temperature", 0.7),
                                         ("top_k", 10), ("top_p", 0.9), ("early_stopping", "never"), ("num_beams", 9), ("diversity_penalty", 0.5),
                                         ("encoder_no_repeat_ngram_size", 2), ("suppress_tokens", [4]), ("num_return_sequences", 2),
                                         ("eos_token_id", [3, 4]), ("min_new_tokens", 2), ("max_new_tokens", 8)])
def test_unsupported_generation_parameters_are_refused_by_name(name, value):
    base = dict(max_length=20, num_beams=4, eos_token_id=3, pad_token_id=0, decoder_start_token_id=2)
    assert S.generation_from_dicts(base).num_beams == 4
    with pytest.raises(ValueError, match=name):
        S.generation_from_dicts(base, {name: value})


def test_generation_parameters_come_from_the_config_files(tmp_path):
    import json

    cfg = S.tiny_config_dict()
    cfg["decoder"].update(num_beams=2, eos_token_id=3)                 # an older checkpoint: parameters inside config.json
    cfg.update(decoder_start_token_id=2, pad_token_id=0)
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    _, c, g = S.load_model_dir(str(tmp_path), max_length=30)
    assert (g.num_beams, g.eos_token_id, g.decoder_start_token_id, g.pad_token_id, g.max_length) == (2, 3, 2, 0, 30)
    assert (g.no_repeat_ngram_size, g.length_penalty, g.early_stopping) == (0, 1.0, False)       # HuggingFace's own defaults
    (tmp_path / "generation_config.json").write_text(json.dumps(dict(num_beams=4, no_repeat_ngram_size=3, length_penalty=2.0, early_stopping=True)))
    _, _, g = S.load_model_dir(str(tmp_path))
    assert (g.num_beams, g.no_repeat_ngram_size, g.length_penalty, g.early_stopping, g.max_length) == (4, 3, 2.0, True, 20)
    (tmp_path / "generation_config.json").write_text(json.dumps(dict(do_sample=True)))
    with pytest.raises(ValueError, match="do_sample"):
        S.load_model_dir(str(tmp_path))
    for key, val, word in (("model_type", "swin", "encoder model_type"), ("hidden_act", "relu", "hidden_act")):
        bad = S.tiny_config_dict()
        bad["encoder"][key] = val
        with pytest.raises(ValueError, match=word):
            S.config_from_dict(bad)


# ---- plugin -------------------------------------------------------------------------------------------------------------------------
def test_aggregation_is_the_reference_s_statements():
    """model_manga_ocr.py:239-275 restated literally on hand-made regions (one group of three lines of which one failed the 48px
    threshold, a single line, a group with nothing left)."""
    from manga_image_translator_amd import plugins as P

    mk = lambda prob, area, fg, bg: types.SimpleNamespace(prob=prob, area=area, fg_r=fg[0], fg_g=fg[1], fg_b=fg[2], bg_r=bg[0], bg_g=bg[1], bg_b=bg[2])
    out_regions = {0: mk(0.9, 1200.0, (10, 20, 31), (250, 251, 252)), 2: mk(0.35, 300.5, (13, 20, 30), (240, 250, 255)), 3: mk(0.5, 10.0, (1, 2, 3), (4, 5, 6))}
    merged_idx = [[0, 1, 2], [3], [4]]
    want = []
    for nodes in merged_idx:
        total_logprobs, total_area = 0, 0
        fg_r, fg_g, fg_b, bg_r, bg_g, bg_b = [], [], [], [], [], []
        for idx in nodes:
            if idx not in out_regions:
                continue
            region_out = out_regions[idx]
            total_logprobs += np.log(region_out.prob) * region_out.area
            total_area += region_out.area
            fg_r.append(region_out.fg_r); fg_g.append(region_out.fg_g); fg_b.append(region_out.fg_b)
            bg_r.append(region_out.bg_r); bg_g.append(region_out.bg_g); bg_b.append(region_out.bg_b)
        if total_area > 0:
            total_logprobs /= total_area
            prob = np.exp(total_logprobs)
        else:
            prob = 0.0
        rd = lambda v: round(np.mean(v)) if v else 0
        want.append((prob, (rd(fg_r), rd(fg_g), rd(fg_b)), (rd(bg_r), rd(bg_g), rd(bg_b))))
    got = P.mocr_aggregate(merged_idx, out_regions)
    assert [(g[1], g[2]) for g in got] == [(w[1], w[2]) for w in want]
    assert all(abs(g[0] - w[0]) <= 1e-15 for g, w in zip(got, want))
    assert got[2] == (0.0, (0, 0, 0), (0, 0, 0)) and got[0][1] == (12, 20, 30)


def test_tokens_to_text_and_post_processing():
    from manga_image_translator_amd import plugins as P

    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "あ", "##い", "…", "・", "A", "."]
    assert P.mocr_tokens_to_text([2, 5, 6, 9, 3, 0, 0], vocab, (3, 0, 2)) == "あい A"
    try:
        import manga_ocr  # noqa: F401
        pytest.skip("manga_ocr is installed: its own post_process is used")
    except ImportError:
        pass
    try:
        import jaconv  # noqa: F401
        wide = True
    except ImportError:
        wide = False
    got = P.mocr_post_process("あ い…\n・・・A.")
    assert got == ("あい......Ａ." if wide else "あい......A.")


def test_use_mocr_merge_is_refused():
    from manga_image_translator_amd import plugins as P

    p = P.HipModelMangaOCR(weights={"ocr48": {}, "mocr": {}}, dictionary=["a"], vocab=["[PAD]"], mocr_config={}, generation=object())
    assert p.is_downloaded()
    with pytest.raises(ValueError, match="use_mocr_merge"):
        asyncio.run(p._infer(np.zeros((8, 8, 3), np.uint8), [], types.SimpleNamespace(use_mocr_merge=True)))
    assert P.HipModelMangaOCR._KEY == "mocr_hip"


def test_the_serving_worker_accepts_mocr():
    """Every worker in "config" mode serves ``ocr.ocr = "mocr"``, with no option: ``DenseStages`` calls ``stage_keys(..., mocr=True)``."""
    from manga_image_translator_amd import serve

    st = serve.DenseStages({"stages": "config"})
    assert st._select({"ocr": {"ocr": "mocr"}}) == ("default", "mocr", "lama_large") and st.last_stage_keys[1] == "mocr"
    assert serve.stage_keys({"ocr": {"ocr": "mocr"}}, mocr=True) == ("default", "mocr", "lama_large")
    assert serve.OPTIONAL_STAGE_KEYS[("ocr", "ocr")] == ("mocr",)
    with pytest.raises(ValueError) as e:
        st._select({"ocr": {"ocr": "paddle"}})
    assert "ocr.ocr = 'paddle'" in str(e.value) and "48px, 48px_ctc, 32px, mocr" in str(e.value)
    assert serve.DenseStages({})._select({"ocr": {"ocr": "mocr"}}) == serve.FIXED_STAGE_KEYS      # fixed mode: whatever the request names
    assert not hasattr(st, "mocr") and "mocr" not in serve.DenseStages({"stages": "config", "mocr": False}).__dict__
