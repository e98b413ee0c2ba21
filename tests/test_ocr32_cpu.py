"""The 32px OCR without a GPU: the CPU oracle against the fixture written from the reference's own module (and against that module
live where the reference tree exists), the state-dict schema, the beam rules on crafted top-5 tables, the host rules of
``Model32pxOCR._infer`` (model_32px.py:58-140) and the plugin's lifecycle (the C struct layouts: tests/test_capi.py)."""
import asyncio
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _ocr32_oracle as O
from manga_image_translator_amd import lib, ocr32, ocr32_schema as S, plugins as P


def run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(O.GOLDEN, "ocr32.npz"))


@pytest.fixture(scope="module")
def oracle_runs():
    """Every beam case through the oracle in float64 and float32."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    runs = {}
    for tag, seed, widths, steps, eos in O.CASES:
        sd = O.weights(O.DICT, seed, eos)
        region = O.make_region(O.lines_u8(widths, seed))
        taps = {}
        runs[tag] = dict(region=region, sd=sd, f64=O.infer_chunk(sd, region, widths, steps, torch.float64, taps),
                         f32=O.infer_chunk(sd, region, widths, steps, torch.float32), taps=taps)
    return runs


def test_oracle_equals_fixture(golden, oracle_runs):
    """Tokens exact; probabilities and colour histories to float32 rounding (the fixture is the reference module's float32 run)."""
    for tag, seed, widths, steps, eos in O.CASES:
        r = oracle_runs[tag]
        assert np.array_equal(golden[f"{tag}.region"], r["region"]) and golden[f"{tag}.widths"].tolist() == list(widths)
        for i in range(len(widths)):
            assert golden[f"{tag}.tokens{i}"].tolist() == r["f64"]["tokens"][i] == r["f32"]["tokens"][i], (tag, i)
            ref_col = golden[f"{tag}.colors{i}"]
            assert ref_col.shape == (len(r["f64"]["tokens"][i]) - 1, 6)
            assert np.abs(ref_col - r["f64"]["colors"][i].numpy()).max() < 2e-5 * max(1.0, np.abs(ref_col).max()), (tag, i)
        assert np.allclose(golden[f"{tag}.prob"], r["f64"]["prob"], rtol=2e-6, atol=0)
    bb = golden["plain.backbone"]
    assert np.abs(bb - oracle_runs["plain"]["taps"]["backbone"].numpy()).max() < 1e-5 * np.abs(bb).max()


def test_cases_are_decisive_and_cover_the_paths(oracle_runs):
    """Conditions on the committed cases: float32 and float64 agree on every token (so exact tokens may be demanded of the GPU), and
    together the traces show a line done by two finished hypotheses while another line of the call is live, a line that reaches the step
    limit unfinished, a line returning its single finished hypothesis, and lines ending at >= 3 different lengths."""
    lengths, done_beside_live, unfinished, single = set(), False, False, False
    for tag, seed, widths, steps, eos in O.CASES:
        r = oracle_runs[tag]
        assert r["f64"]["tokens"] == r["f32"]["tokens"], tag
        assert np.allclose(r["f64"]["prob"], r["f32"]["prob"], rtol=1e-5)
        b = r["f64"]["beams"]
        lengths |= {len(t) for t in r["f64"]["tokens"]}
        n = len(widths)
        for line, at in b.done_at.items():
            others = [o for o in range(n) if o != line and b.done_at.get(o, steps + 1) > at]
            done_beside_live |= len(b.finished[line]) >= 2 and bool(others)
        unfinished |= any(i not in b.finished and len(r["f64"]["tokens"][i]) == steps + 2 for i in range(n))
        single |= any(len(f) == 1 for f in b.finished.values())
    assert done_beside_live and unfinished and single and len(lengths) >= 3, (done_beside_live, unfinished, single, lengths)


def test_oracle_equals_reference_live(oracle_runs):
    """Where the reference tree exists: the oracle (float32) == the reference's own OCR module, and the schema == its state_dict."""
    model = O.reference_model(O.weights(O.DICT, 0), O.DICT)
    if model is None:
        return   # no reference tree on this machine: the fixture test above is the pin
    ref_sd = model.state_dict()
    want = {n: tuple(s) for n, s, k in S.ocr32_schema(O.DICT)}
    assert {k: tuple(v.shape) for k, v in ref_sd.items()} == want
    assert ref_sd["pred.weight"].data_ptr() == ref_sd["embd.weight"].data_ptr()
    assert torch.equal(ref_sd["pe.pe"], O.weights(O.DICT, 0)["pe.pe"])
    tag, seed, widths, steps, eos = O.CASES[2]
    model = O.reference_model(O.weights(O.DICT, seed, eos), O.DICT)
    ref = O.run_reference(model, oracle_runs[tag]["region"], widths, steps)
    o32 = oracle_runs[tag]["f32"]
    for i, r in enumerate(ref):
        assert r["tokens"] == o32["tokens"][i]
        assert abs(r["prob"] - o32["prob"][i]) < 1e-6
        assert float((r["colors"] - o32["colors"][i]).abs().max()) < 2e-5


@pytest.mark.parametrize("name", sorted(O.crafted()))
def test_beam_rules_on_crafted_tables(name):
    c = O.crafted()[name]
    for ftype in (np.float64, np.float32):
        b, trace = O.replay(c["vals"].tolist(), c["idx"].tolist(), c["N"], ftype=ftype)
        assert [h.toks for h in b.result()] == c["tokens"]
        if c["kept"] is not None:
            assert trace[-1] == c["kept"]
    if name == "dropout":
        b, trace = O.replay(c["vals"].tolist(), c["idx"].tolist(), c["N"])
        assert b.done_at == {0: 1} and {k: len(v) for k, v in b.finished.items()} == {0: 2, 1: 1}
        assert [sorted(t) for t in trace[1:]] == [[1, 2]] * 3                      # line 0 has dropped out, its neighbours go on
        live_best = max(-h.key(np.float64) for h in b.live if h.line == 1)
        assert live_best > -b.finished[1][0].key(np.float64)                        # ... although a live hypothesis scores higher
        assert abs(-b.result()[2].key(np.float64) - (-4.0 / 5)) < 1e-12             # mean over len + 1 entries (the start token's 0.0)


def test_decode_32px_line():
    d = O.dictionary(20)
    col = np.asarray([[0.5, 1.5, -1.0, 0.2, 0.999, 0.0], [0.25, 0.5, 2.0, 0.2, 1.0, 0.0039215688]], np.float32)
    txt, fg, bg = P.decode_32px_line([1, 5, 3, 6, 2, 7], col, d)
    assert txt == d[5] + " " + d[6]                       # <S> skipped, <SP> -> blank, stops at </S>
    assert fg == (int(0.375 * 255), 191, 127) and bg == (51, 254, 0)   # clip, mean over ALL rows, * 255, truncate
    want_c, _ = O.int_colors(torch.from_numpy(col))
    assert list(fg + bg) == want_c
    assert P.decode_32px_line([1, 2], col[:1], d)[0] == ""


def test_chunks_have_no_extra_padding():
    """Model32pxOCR._infer pads a chunk to 4 * (max + 7) // 4 = max + 7 (:78) — the 48px_ctc model adds 128 more."""
    imgs = [np.full((32, w, 3), w % 251, np.uint8) for w in (90, 30, 64, 31) + tuple(range(100, 114))]
    chunks = list(ocr32.Ocr32Engine.make_chunks(imgs))
    assert [len(c[0]) for c in chunks] == [16, 2]
    idx, ws, region = chunks[0]
    assert ws == sorted(ws) and idx[:3] == [1, 3, 2] and region.shape == (16, 32, max(ws) + 7, 3)
    assert region[0, :, 30:].max() == 0 and (region[0, :, :30] == 30).all()
    assert chunks[1][2].shape == (2, 32, 113 + 7, 3)
    assert O.make_region(imgs[:4]).shape == (4, 32, 97, 3)
    assert [O.valid_len(w) for w in (1, 4, 5, 121)] == [3, 3, 4, 33]
    assert ocr32.Ocr32Engine.valid_len(121, 33) == 33 and ocr32.Ocr32Engine.valid_len(121, 30) == 30


def test_ignore_bubble_rule():
    """ignore_bubble outside 1..50 never rejects; inside, a crop with a half-dark frame is rejected (utils/bubble.py:28-84)."""
    from manga_image_translator_amd import textline as TL

    crop = np.full((32, 64, 3), 255, np.uint8)
    crop[:, :32] = 0
    assert TL.is_ignore(crop, 10) and not TL.is_ignore(crop, 0) and not TL.is_ignore(crop, 51)
    assert not TL.is_ignore(np.full((32, 64, 3), 255, np.uint8), 10)


def test_native_argument_checks_without_gpu():
    h = lib.load()
    assert h.mit_ocr32_decode(None, None, None) != 0 and b"null argument" in h.mit_last_error()
    assert h.mit_ocr32_decode_workspace_bytes(0, 4, 10) == 0 and h.mit_ocr32_decode_workspace_bytes(4, 12, 97) > 0
    a = lib.MitOcr32DecodeArgs()
    a.N, a.max_seq_length = 1, 4
    assert h.mit_ocr32_beam_replay(4096, 4096, 9, C.byref(a), None) != 0 and b"steps must be" in h.mit_last_error()


def test_schema_and_synthetic_weights():
    sch = S.ocr32_schema(O.DICT)
    names = [n for n, _, _ in sch]
    assert len(names) == len(set(names)) and names.index("embd.weight") < names.index("pred.weight")
    sd = O.weights(O.DICT, 0)
    assert sd["pred.weight"] is sd["embd.weight"] and tuple(sd["pe.pe"].shape) == (768, 1, 320)
    assert tuple(sd["backbone.ConvNet.conv4_1.weight"].shape) == (320, 320, 2, 2)
    assert sum(n.startswith("backbone.ConvNet.layer3.") and n.endswith("conv1.weight") for n in names) == 7
    bad = dict(sd)
    del bad["pe.pe"]
    from manga_image_translator_amd import synth
    with pytest.raises(ValueError, match="missing"):
        synth.check_state_dict(bad, sch, "ocr.ckpt")


def test_plugin_lifecycle_standalone(tmp_path):
    cls = P.HipModel32pxOCR
    assert cls._KEY == "32px_hip" and set(cls._MODEL_MAPPING["model"]["archive"]) == {"ocr.ckpt", "alphabet-all-v5.txt"}
    assert issubclass(cls, P.HipModel48pxOCR)
    p = cls()
    assert not p.is_loaded()
    with pytest.raises(Exception, match="without having loaded"):
        run(p.infer(np.zeros((8, 8, 3), np.uint8), []))
    p = cls(weights={}, dictionary=[])
    assert p.is_downloaded() and not p.is_loaded()
    with pytest.raises(RuntimeError, match="MI355X only"):
        run(p.load("cpu"))
    run(p.unload())
    # the checkpoint loader: {'model': sd} or bare, schema-checked, dictionary lines lose their newline
    d = O.dictionary(12)
    (tmp_path / "alphabet-all-v5.txt").write_text("".join(ch + "\n" for ch in d), encoding="utf-8")
    sd = O.weights(12, 0)

    class Stub:
        def _get_file_path(self, name):
            return str(tmp_path / name)

    torch.save({"model": sd}, tmp_path / "ocr.ckpt")
    got, dic = P._load_ocr32_checkpoint(Stub())
    assert dic == d and set(got) == set(sd)
    torch.save({k: v for k, v in sd.items() if k != "pred.bias"}, tmp_path / "ocr.ckpt")
    with pytest.raises(ValueError, match="pred.bias"):
        P._load_ocr32_checkpoint(Stub())


def test_page_case_is_decisive():
    """The page-sized GPU case (32 lines of the synthetic 2048 x 1456 page, dictionary pipeline.DICT_SIZE, 32 steps) qualifies too:
    float32 and float64 return the same tokens for every line."""
    from manga_image_translator_amd import pipeline, synth
    from oracle import textline as OT

    torch.set_num_threads(min(8, torch.get_num_threads()))
    sd = O.weights(pipeline.DICT_SIZE, 0)
    page, quads, _ = synth.synth_page(0, 2048, 1456, n_boxes=32)
    crops = []
    for pts in quads:
        sp, vert = OT.sort_pnts(pts)
        crops.append(OT.get_transformed_region(page, sp, "v" if vert else "h", 32))
    n = 0
    for indices, ws, region in ocr32.Ocr32Engine.make_chunks(crops):
        r64 = O.infer_chunk(sd, region, ws, 32, torch.float64)
        r32 = O.infer_chunk(sd, region, ws, 32, torch.float32)
        assert r64["tokens"] == r32["tokens"]
        n += len(ws)
    assert n == 32
