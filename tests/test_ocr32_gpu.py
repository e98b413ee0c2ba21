"""32px OCR stage parity: HIP engine vs the CPU oracle (tests/_ocr32_oracle.py, run in float64) of the reference model
(manga_translator/ocr/model_32px.py).

Bars (each an existing bar of this project for the same kind of quantity): backbone and encoder memory 3e-4 * max|ref|
(tests/test_ocr_ctc_gpu.py, the same FAN backbone); per-step log-probs 5e-4 absolute, prob 1e-3 relative, colour heads
2e-4 * max(1, max|ref|) (tests/test_ocr_gpu.py); tokens, lengths and kept hypotheses identical — every case is decisive (the oracle
returns the same tokens in float32 and float64, tests/test_ocr32_cpu.py)."""
import asyncio

import numpy as np
import pytest
import torch

import _ocr32_oracle as O

pytestmark = pytest.mark.gpu

PAGE_EOS_BIAS = 0.0   # the page-sized case runs every line to the step limit


def _engine(cuda, sd, D):
    from manga_image_translator_amd import ocr32

    return ocr32.Ocr32Engine(sd, D, device=cuda)


@pytest.fixture(scope="module")
def setup0(cuda, shipped_mode):
    sd = O.weights(O.DICT, 0)
    with shipped_mode():
        return sd, _engine(cuda, sd, O.DICT)


def test_backbone_and_memory_parity(cuda, gemm_mode, setup0, oracle_memo):
    """Chunks of different padded widths (T = 33 and 12) and a line whose valid length equals the padded length (w = 121 -> 33)."""
    sd, eng = setup0
    sd64 = O.cast(sd, torch.float64)
    for ci, widths in enumerate(((50, 77, 120, 121), (33, 40))):
        region = O.make_region(O.lines_u8(widths, 7 + ci))
        taps = {}
        mem_k, mem_v, klen, L = eng.encode(torch.from_numpy(region).to(cuda), widths, taps=taps)
        torch.cuda.synchronize()

        def run_oracle():
            t = {}
            with torch.no_grad():
                mem, mask = O.encode(sd64, region, widths, t)
            return t["backbone"], mem.permute(1, 0, 2), mask

        bb, mem, mask = oracle_memo(("ocr32-enc", ci), run_oracle)
        assert tuple(taps["backbone"].shape) == tuple(bb.shape) and L == bb.shape[1]
        assert klen.cpu().tolist() == [O.valid_len(w) for w in widths] and (ci != 0 or klen[-1].item() == L)
        e1 = (taps["backbone"].cpu().double() - bb).abs().max().item()
        print(f"gemm mode {gemm_mode} chunk {ci}: backbone err {e1:.3e} / max {bb.abs().max().item():.3f}")
        assert e1 < 3e-4 * bb.abs().max().item(), e1
        valid = ~mask
        e2 = ((taps["memory"].cpu().double() - mem).abs() * valid[..., None]).max().item()
        print(f"gemm mode {gemm_mode} chunk {ci}: memory err {e2:.3e} / max {mem.abs().max().item():.3f}")
        assert e2 < 3e-4 * mem.abs().max().item(), e2


def _check_beam(cuda, sd, D, eng, region, widths, T, memo):
    """One chunk through encode + decode(trace) against the float64 oracle.  Returns the worst per-step log-prob error."""
    enc = eng.encode(torch.from_numpy(region).to(cuda), widths)
    out = eng.decode(enc[0], enc[1], enc[2], max_seq_length=T, trace=True)
    torch.cuda.synchronize()
    ref = memo(lambda: O.infer_chunk(sd, region, widths, T, torch.float64))
    N = len(widths)
    tr = ref["trace"]
    assert out["steps_run"] >= len(tr["logprobs"])          # (the native loop tests for the early exit every four steps only)
    tl = out["trace_logits"].cpu().double()
    th = out["trace_hist"].cpu()
    worst = 0.0
    for s, (lp, lines) in enumerate(zip(tr["logprobs"], tr["lines"])):
        # row mapping: the oracle's live list is line-major; here line n's j-th hypothesis is always row 5 n + j (step 0: row 5 n)
        seen, rows = {}, []
        for ln in lines:
            j = seen.get(ln, 0)
            seen[ln] = j + 1
            rows.append(5 * ln + j)
        got = tl[s][rows].log_softmax(-1)
        err = (got - lp).abs().max().item()
        assert err < 5e-4, (s, err)
        worst = max(worst, err)
        for ln, kept in tr["kept"][s].items():
            for j, toks in enumerate(kept):
                assert th[s, 5 * ln + j, :len(toks)].tolist() == toks, (s, ln, j)
    toks, lens, probs = out["tokens"].cpu(), out["length"].cpu(), out["prob"].cpu()
    for n in range(N):
        want = ref["tokens"][n]
        assert lens[n].item() == len(want) and toks[n, :len(want)].tolist() == want, (n, toks[n].tolist(), want)
        assert not toks[n, len(want):].any()
        assert abs(probs[n].item() - ref["prob"][n]) < 1e-3 * ref["prob"][n], (n, probs[n].item(), ref["prob"][n])
        refc = ref["colors"][n]
        col = out["colors"][n, :len(want) - 1].cpu().double()
        cerr = (col - refc).abs().max().item()
        assert cerr < 2e-4 * max(1.0, refc.abs().max().item()), (n, cerr)
    return worst, out, ref


@pytest.mark.parametrize("case", O.CASES, ids=[c[0] for c in O.CASES])
def test_beam_search_parity(cuda, gemm_mode, oracle_memo, case):
    """4 lines, 12 steps: no line ends / lines end at once / lines end at different steps while others go on / a single finished one."""
    tag, seed, widths, T, eos = case
    sd = O.weights(O.DICT, seed, eos)
    eng = _engine(cuda, sd, O.DICT)
    region = O.make_region(O.lines_u8(widths, seed))
    worst, out, ref = _check_beam(cuda, sd, O.DICT, eng, region, widths, T, lambda fn: oracle_memo(("ocr32-beam", tag), fn))
    print(f"gemm mode {gemm_mode} case {tag}: lengths {[len(t) for t in ref['tokens']]}, steps run {out['steps_run']}, "
          f"worst per-step log-prob error {worst:.2e}")
    # integer colours of the plugin rule: equal unless the oracle's value lies within 255 * 2e-4 of an integer (then +-1)
    from manga_image_translator_amd import plugins as P

    for n, want in enumerate(ref["tokens"]):
        _, fg, bg = P.decode_32px_line(want, out["colors"][n, :len(want) - 1].cpu().numpy(), O.dictionary(O.DICT))
        ints, floats = O.int_colors(ref["colors"][n])
        for g, w, f in zip(fg + bg, ints, floats):
            near = abs(f - round(f)) < 255 * 2e-4
            assert g == w or (near and abs(g - w) <= 1), (n, g, w, f)


def _page_crops(height=32):
    from manga_image_translator_amd import synth
    from oracle import textline as OT

    page, quads, _ = synth.synth_page(0, 2048, 1456, n_boxes=32)
    crops = []
    for pts in quads:
        sp, vert = OT.sort_pnts(pts)
        crops.append(OT.get_transformed_region(page, sp, "v" if vert else "h", height))
    return page, quads, crops


def test_beam_search_parity_at_page_size(cuda, gemm_mode, oracle_memo):
    """The 32 text lines of the synthetic 2048 x 1456 page (two chunks of 16), dictionary of pipeline.DICT_SIZE entries, 32 steps."""
    from manga_image_translator_amd import ocr32, pipeline

    D = pipeline.DICT_SIZE
    sd = O.weights(D, 0, PAGE_EOS_BIAS)
    eng = _engine(cuda, sd, D)
    _, _, crops = _page_crops()
    assert len(crops) == 32
    for c, (indices, ws, region) in enumerate(ocr32.Ocr32Engine.make_chunks(crops)):
        worst, out, ref = _check_beam(cuda, sd, D, eng, region, ws, 32, lambda fn: oracle_memo(("ocr32-page", c), fn))
        print(f"gemm mode {gemm_mode} page chunk {c}: widths {ws[0]}..{ws[-1]}, lengths {sorted({len(t) for t in ref['tokens']})}, "
              f"steps run {out['steps_run']}, worst per-step log-prob error {worst:.2e}")



@pytest.mark.parametrize("name", sorted(O.crafted()))
def test_bookkeeping_kernel_on_crafted_tables(cuda, setup0, name):
    """mit_ocr32_beam_replay = the decoder's bookkeeping kernels alone, on the crafted tables of the CPU test: same expected outputs."""
    _, eng = setup0
    c = O.crafted()[name]
    out = eng.beam_replay(torch.from_numpy(c["vals"]), torch.from_numpy(c["idx"]), c["N"], c["T"])
    torch.cuda.synchronize()
    b, trace = O.replay(c["vals"].tolist(), c["idx"].tolist(), c["N"])
    res = b.result()
    toks, lens, probs, src = (out[k].cpu() for k in ("tokens", "length", "prob", "src"))
    for n, want in enumerate(c["tokens"]):
        assert toks[n, :lens[n]].tolist() == want == res[n].toks, (n, toks[n].tolist())
        assert abs(probs[n].item() - np.exp(-res[n].key(np.float64))) < 1e-6
        assert (src[n, :len(want) - 1] // 5 == n).all() and (src[n, len(want) - 1:] == -1).all()
    th = out["trace_hist"].cpu()
    for s, kept in enumerate(trace):
        for ln, hyps in kept.items():
            for j, t in enumerate(hyps):
                assert th[s, 5 * ln + j, :len(t)].tolist() == t, (s, ln, j)
    if c["kept"] is not None:
        for ln, hyps in c["kept"].items():
            assert [th[-1, 5 * ln + j, :len(t)].tolist() for j, t in enumerate(hyps)] == hyps


def test_pooled_decode_equals_per_chunk_and_repeats(cuda, gemm_mode):
    """Every padded key is masked, so a line's result does not depend on its chunk or on the lines decoded beside it: the pooled decode
    of 20 lines (two chunks, two memory lengths) == chunk-by-chunk decodes, bit for bit; and a second run repeats the first bit for bit."""
    sd = O.weights(O.DICT, 2, 4.0)
    eng = _engine(cuda, sd, O.DICT)
    crops = O.lines_u8([40 + 9 * i for i in range(20)], 5)
    pooled = eng.recognize(crops, max_seq_length=12)
    again = eng.recognize(crops, max_seq_length=12)
    torch.cuda.synchronize()
    for k in ("tokens", "length", "prob", "colors"):
        assert torch.equal(pooled[k], again[k]), k
    assert pooled["order"] == sorted(range(20), key=lambda i: crops[i].shape[1])
    assert len(set(pooled["length"].cpu().tolist())) >= 2
    pos = 0
    for indices, ws, region in eng.make_chunks(crops):
        mk, mv, kl, L = eng.encode(torch.from_numpy(region).to(cuda), ws)
        o = eng.decode(mk, mv, kl, max_seq_length=12)
        torch.cuda.synchronize()
        n = len(ws)
        for k in ("tokens", "length", "prob"):
            assert torch.equal(o[k], pooled[k][pos:pos + n]), k
        for j in range(n):
            m = int(o["length"][j]) - 1
            assert torch.equal(o["colors"][j, :m], pooled["colors"][pos + j, :m])
        pos += n


def test_few_row_form_equals_tiled_form(cuda):
    """The two forms of a decode step (MitOcr32DecodeArgs.form) in the shipped GEMM mode: same tokens, lengths and kept hypotheses; the
    per-step logits, probabilities and colours within 1e-5 (relative to 1) — the few-row FFN output Linear sums K in four parts, the
    only arithmetic that differs (the bar tests/test_ocr_gpu.py holds the 48px loop's two forms to).  Dictionary 96 lets ``pred`` take
    the planar form too (its width must be a multiple of 4)."""
    from manga_image_translator_amd import ops

    with ops.gemm_mode(6):
        for D, (tag, seed, widths, T, eos) in ((96, O.CASES[2]), (O.DICT, O.CASES[2]), (96, O.CASES[0])):
            sd = O.weights(D, seed, eos)
            eng = _engine(cuda, sd, D)
            region = O.make_region(O.lines_u8(widths, seed))
            enc = eng.encode(torch.from_numpy(region).to(cuda), widths)
            a = eng.decode(enc[0], enc[1], enc[2], max_seq_length=T, trace=True)
            b = eng.decode(enc[0], enc[1], enc[2], max_seq_length=T, trace=True, tiled=True)
            torch.cuda.synchronize()
            assert torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["length"], b["length"]) and a["steps_run"] == b["steps_run"]
            assert len(set(a["length"].cpu().tolist())) >= (3 if eos else 1)
            live = a["trace_hist"][:, :5]                  # line 0 never ends in these cases: its rows are live at every step
            assert torch.equal(live, b["trace_hist"][:, :5])
            n = a["steps_run"]
            dl = (a["trace_logits"][:n, :5] - b["trace_logits"][:n, :5]).abs().max().item()
            assert dl < 1e-5 * max(1.0, b["trace_logits"][:n, :5].abs().max().item()), dl
            assert (a["prob"] - b["prob"]).abs().max().item() < 1e-5
            for j in range(len(widths)):
                m = int(a["length"][j]) - 1
                assert (a["colors"][j, :m] - b["colors"][j, :m]).abs().max().item() < 1e-5 * max(1.0, b["colors"][j, :m].abs().max().item())


def test_plugin_end_to_end(cuda):
    """HipModel32pxOCR on the synthetic page: prob = 0.0 returns every line with text and colours equal to the engine's own results,
    prob = 1.1 returns [], ignore_bubble zeroes rejected crops (still decoded); register() where the reference package imports."""
    from manga_image_translator_amd import plugins as P, synth, textline as TL

    run = lambda coro: asyncio.new_event_loop().run_until_complete(coro)
    D = 64
    sd = O.weights(D, 0)   # no </S> bias: lines run on, so their text is not empty
    p = P.HipModel32pxOCR(weights=sd, dictionary=O.dictionary(D))
    with pytest.raises(Exception, match="without having loaded"):
        run(p.infer(np.zeros((8, 8, 3), np.uint8), []))
    run(p.load("cuda"))
    page, quads, _ = synth.synth_page(0, 1024, 728, n_boxes=8)

    class Cfg:
        def __init__(self, prob, ignore_bubble=0):
            self.prob, self.ignore_bubble = prob, ignore_bubble

    mk = lambda: [P._RefQuadrilateral(q.astype(int), "", 1.0) for q in quads]
    lines = mk()
    got = run(p.infer(page, lines, Cfg(0.0), max_seq_length=12) if not P.HAVE_REFERENCE else p._infer(page, lines, Cfg(0.0), max_seq_length=12))
    assert len(got) == 8 and all(isinstance(q.text, str) and 0.0 < q.prob <= 1.0 for q in got)
    assert all(0 <= v <= 255 for q in got for v in (q.fg_r, q.fg_g, q.fg_b, q.bg_r, q.bg_g, q.bg_b))
    assert any(q.text for q in got)
    # the same lines through the engine: the plugin returns them in processing order with the engine's numbers
    own = [P._own_quad(q) for q, _ in p._directions(mk())]
    dirs = [d for _, d in p._directions(mk())]
    r = p.engine.recognize_lines(torch.from_numpy(page).to(cuda)[None], own, dirs, max_seq_length=12)
    assert [float(v) for v in r["prob"].cpu()] == [q.prob for q in got]
    assert run(p._infer(page, mk(), Cfg(1.1), max_seq_length=12)) == []
    # ignore_bubble = 10: the plugin zeroes the rows of the crops textline.is_ignore rejects and still decodes them (:84-86) — the same
    # as the engine with that predicate; a rejected line's result is the one of its all-zero crop, the others are untouched
    rej = run(p._infer(page, mk(), Cfg(0.0, 10), max_seq_length=12))
    flags = []
    r3 = p.engine.recognize_lines(torch.from_numpy(page).to(cuda)[None], own, dirs, max_seq_length=12,
                                  reject=lambda crop: flags.append(TL.is_ignore(crop, 10)) or flags[-1])
    assert [float(v) for v in r3["prob"].cpu()] == [q.prob for q in rej] and r3["order"] == r["order"]
    seen = []
    r2 = p.engine.recognize_lines(torch.from_numpy(page).to(cuda)[None], own, dirs, max_seq_length=12, reject=lambda crop: seen.append(crop.shape) or True)
    assert len(seen) == 8 and all(s[0] == 32 and s[2] == 3 for s in seen)
    assert any(flags), "the page is expected to hold a crop the bubble filter rejects"
    for row, f in enumerate(flags):
        other = r2 if f else r
        assert torch.equal(r3["tokens"][row], other["tokens"][row]) and torch.equal(r3["prob"][row], other["prob"][row]), (row, f)
    run(p.unload())
    assert p.engine is None
    if P.HAVE_REFERENCE:
        P.register()
        from manga_translator.ocr import OCRS  # type: ignore

        assert any(v is P.HipModel32pxOCR for v in OCRS.values())
