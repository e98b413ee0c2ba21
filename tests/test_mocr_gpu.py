"""manga-ocr recogniser parity: HIP engine (mocr.MocrEngine, mit_mocr_decode) vs the float64 oracle tests/_mocr_oracle.py, which
tests/test_mocr_cpu.py pins to HuggingFace's own modules and ``generate``.

Bars (those of the 32px tests, tests/test_ocr32_gpu.py:55-97): encoder states 3e-4 * max|ref|; per-step log-probabilities 5e-4
absolute; tokens, lengths and beam histories identical; res_score 1e-3 relative.  Every case is decisive: the oracle gives the same
tokens and histories in float32 and float64 (asserted in tests/test_mocr_cpu.py).  The few-row and the tiled form of a step share every
product and its order (no K cut here), so their scores agree within 1e-5.
Pre-processing kernels: byte-exact against Pillow up to the resize; the normalised patch rows are one fp32 expression per value
(two roundings), compared at 1e-6."""
import numpy as np
import pytest
import torch

import _mocr_oracle as O

pytestmark = pytest.mark.gpu


def _engine(cuda, name):
    from manga_image_translator_amd import mocr

    cfg, c, sd, crops, g = O.case(name, torch.float32)
    return mocr.MocrEngine(sd, cfg, g, device=cuda), c, crops, g


def _check(cuda, name, memo, gemm_mode, tiled=False):
    eng, c, crops, g = _engine(cuda, name)
    ref = memo(("mocr-case", name), lambda: O.run_case(name))
    imgs = eng.preprocess([torch.from_numpy(cr).to(cuda) for cr in crops])
    want_imgs = np.stack([O.preprocess(cr, c.image_size) for cr in crops])
    assert np.array_equal(imgs.cpu().numpy(), want_imgs)
    taps = {}
    mem_k, mem_v = eng.encode(imgs, taps=taps)
    out = eng.decode(mem_k, mem_v, trace=True, tiled=tiled)
    torch.cuda.synchronize()
    mem = ref["memory"]
    e_mem = (taps["memory"].cpu().double() - mem).abs().max().item()
    print(f"{name} gemm mode {gemm_mode} tiled {tiled}: encoder err {e_mem:.3e} / max {mem.abs().max().item():.3f}")
    assert e_mem < 3e-4 * mem.abs().max().item(), e_mem
    nb, N = g.num_beams, len(crops)
    assert out["steps_run"] >= ref["steps_run"]          # (the native loop tests for the early exit every four steps only)
    tl, th = out["trace_logits"].cpu().double(), out["trace_hist"].cpu().long()
    worst = 0.0
    for s in range(ref["steps_run"]):
        for n in range(N):
            if ref["done_step"][n] is not None and s > ref["done_step"][n]:
                continue                                  # a line that is done keeps its rows; nothing reads them again
            rows = slice(n * nb, n * nb + (1 if s == 0 else nb))   # step 0: only the first beam of a line counts
            a, b = tl[s, rows], ref["logp"][s, rows]
            assert torch.equal(torch.isinf(a), torch.isinf(b)), (name, s, n)      # the same tokens are banned
            fin = ~torch.isinf(b)
            err = (a[fin] - b[fin]).abs().max().item()
            worst = max(worst, err)
            assert err < 5e-4, (name, s, n, err)
            assert torch.equal(th[s, n * nb:(n + 1) * nb], ref["hist"][s, n * nb:(n + 1) * nb]), (name, s, n)
    print(f"{name} gemm mode {gemm_mode} tiled {tiled}: worst per-step log-prob error {worst:.2e}, lengths {ref['length'].tolist()}, "
          f"steps run {out['steps_run']}")
    assert torch.equal(out["tokens"].cpu().long(), ref["tokens"]), (out["tokens"].cpu().tolist(), ref["tokens"].tolist())
    assert torch.equal(out["length"].cpu().long(), ref["length"])
    sc = out["score"].cpu().double()
    rel = ((sc - ref["score"]).abs() / ref["score"].abs()).max().item()
    print(f"{name}: score {sc.tolist()} vs {ref['score'].tolist()} (rel {rel:.2e})")
    assert rel < 1e-3, rel
    # which form ran: the few-row form needs a split GEMM mode (the weights then carry their planes) and is what ships there; the
    # vocabulary Linear joins it when V % 8 == 0
    want_form = 0 if tiled or gemm_mode not in (6, 9) else (2 if c.vocab % 8 == 0 else 1)
    assert out["form_run"] == want_form, (name, gemm_mode, tiled, out["form_run"])
    return out


@pytest.mark.parametrize("name", ["vit32", "vit48", "deit", "greedy", "early", "tomax"])
def test_generate_parity(cuda, gemm_mode, oracle_memo, name):
    """vit32: lines end at different steps, n-gram ban, heuristic stop; vit48: 10 tokens, V = 97, N = 5, length_penalty 2; deit: the
    distillation token + enc_to_dec_proj, N = 1; greedy; early: lines finished within the first two steps; tomax: no line ends."""
    _check(cuda, name, oracle_memo, gemm_mode)


def test_generate_parity_at_the_real_width(cuda, gemm_mode, oracle_memo):
    """hidden 768 / 12 heads / 1 + 1 layers / FFN 3072 / V = 6144, 2 lines, 6 steps: the LayerNorm at 768, K = 768 / 3072 Linears, the
    LM-head tile edges."""
    _check(cuda, "wide", oracle_memo, gemm_mode)


@pytest.mark.parametrize("name", ["vit32", "vit48"])
def test_few_row_form_against_tiled_form(cuda, oracle_memo, name):
    from manga_image_translator_amd import ops

    with ops.gemm_mode(6):
        a = _check(cuda, name, oracle_memo, 6, tiled=False)
        b = _check(cuda, name, oracle_memo, 6, tiled=True)
    assert a["form_run"] >= 1 and b["form_run"] == 0          # the two runs did take different forms
    assert torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["length"], b["length"])
    d = (a["score"] - b["score"]).abs().max().item()
    print(f"{name}: few-row vs tiled score difference {d:.2e}")
    assert d < 1e-5, d


# ---- bookkeeping alone --------------------------------------------------------------------------------------------------------------
def _tables(seed, steps, N, nb, V, eos_at=(), only_one=()):
    """Log-probability tables without ties: a random permutation of distinct, well separated values per row, normalised.  ``eos_at``:
    steps at which EOS is the best (odd beams) or second best (even beams) token of every row, so that it lands inside the top
    2 * beams; ``only_one``: steps at which all but one token are banned (-inf) in every row."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.empty(steps, N * nb, V, dtype=torch.float64)
    for s in range(steps):
        for r in range(N * nb):
            vals = -0.37 * torch.arange(V, dtype=torch.float64) - 0.011 * torch.rand(V, generator=gen, dtype=torch.float64) - 0.003 * r
            perm = torch.randperm(V, generator=gen)
            row = torch.empty(V, dtype=torch.float64)
            row[perm] = vals
            if s in eos_at:
                rank = 0 if r % 2 else 1
                j = perm[rank].item()
                row[j], row[O.EOS] = row[O.EOS].item(), row[j].item()
            if s in only_one:
                keep = perm[3].item() if perm[3].item() != O.EOS else perm[4].item()
                v = row[keep].item()
                row[:] = float("-inf")
                row[keep] = v
            t[s, r] = row
    return t.float()


@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("kind", ["eos", "banned", "plain"])
def test_beam_replay_against_the_oracle(cuda, nb, es, kind):
    """mit_mocr_beam_replay on hand-built tables against the oracle's bookkeeping, exact: EOS inside the top 2 * beams at chosen steps,
    all tokens banned but one, early_stopping both ways, num_beams 1 and 4, with the n-gram ban and length_penalty 2."""
    from manga_image_translator_amd import mocr

    N, V, T = 3, 48, 12
    eng, _, _, _ = _engine(cuda, "early")
    g = O.gen_params(num_beams=nb, ngram=2 if kind != "banned" else 0, length_penalty=2.0, early_stopping=es, max_length=T)
    tab = _tables(11 + nb, T - 1, N, nb, V, eos_at=(2, 3, 6) if kind == "eos" else (), only_one=(1, 4) if kind == "banned" else ())
    ref = O.replay(tab.double(), N, g)
    steps = ref["steps_run"]
    out = eng.beam_replay(tab[:steps], N, g)
    torch.cuda.synchronize()
    assert out["steps_run"] == steps
    assert torch.equal(out["trace_hist"].cpu().long(), ref["hist"]), kind
    assert torch.equal(out["tokens"].cpu().long(), ref["tokens"]) and torch.equal(out["length"].cpu().long(), ref["length"])
    have = ref["length"] > 0
    assert torch.allclose(out["score"].cpu().double()[have], ref["score"][have], rtol=1e-6, atol=0)
    print(f"replay nb {nb} es {es} {kind}: lengths {ref['length'].tolist()} done {ref['done_step']}")


def test_lines_are_decoded_in_chunks_under_the_workspace_limit(cuda):
    """N = 5 lines with a workspace limit that holds two: three calls, the same tokens, lengths and scores as one call."""
    eng, c, crops, g = _engine(cuda, "vit48")
    mem_k, mem_v = eng.encode(eng.preprocess([torch.from_numpy(cr).to(cuda) for cr in crops]))
    one = eng.decode(mem_k, mem_v)
    assert eng.lines_per_call() >= 5 and "calls" not in eng.decode_chunked(mem_k, mem_v)
    from manga_image_translator_amd import lib

    size = lambda n: lib.load().mit_mocr_decode_workspace_bytes(n, g.num_beams, g.max_length, c.dec_hidden, c.dec_inter, c.vocab, c.dec_layers)
    eng.max_workspace_bytes = size(2) + (size(3) - size(2)) // 2
    assert eng.lines_per_call() == 2
    got = eng.decode_chunked(mem_k, mem_v)
    torch.cuda.synchronize()
    assert got["calls"] == 3
    for k in ("tokens", "length", "score"):
        assert torch.equal(got[k], one[k]), k
    eng.max_workspace_bytes = 1                               # never fewer than one line a call
    assert eng.lines_per_call() == 1


def test_the_plugin_carries_the_48px_results_through(cuda):
    """HipModelMangaOCR._infer with a stand-in for the 48px plugin (the ``ocr48=`` argument) that accepts two of three lines with known
    probabilities and colours: accepted lines come out with exactly those (a group is one line, so exp(log(p) * area / area) = p), the
    rejected line with prob 0.0 and black, every line with the text of the manga-ocr engine, all in processing order."""
    import asyncio

    from manga_image_translator_amd import plugins as P
    from manga_image_translator_amd.textline import Quadrilateral
    kind = {}                                                 # id(line) -> 0 | 2 accepted with known values, 1 under the threshold

    class Stub48:
        dictionary = None

        def is_loaded(self):
            return True

        async def _infer(self, image, textlines, config, verbose, ignore_bubble, max_seq_length):
            assert config is None and ignore_bubble == 0 and max_seq_length == 255          # the reference's fixed call (:189)
            out = []
            for q in textlines:
                k = kind[id(q)]
                q.text = "discarded"
                if k != 1:                                    # "under 0.2": not returned, nothing written
                    q.prob, (q.fg_r, q.fg_g, q.fg_b), (q.bg_r, q.bg_g, q.bg_b) = 0.3 + 0.2 * k, (10 + k, 20, 30), (200, 210 + k, 220)
                    out.append(q)
            return out

    cfg, c, sd, _, g = O.case("vit32", torch.float32)
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [chr(0x3042 + i) for i in range(c.vocab - 5)]
    page = np.random.default_rng(5).integers(0, 256, size=(320, 200, 3), dtype=np.uint8)
    quads = [[[20, 20], [150, 20], [150, 50], [20, 50]], [[20, 80], [60, 80], [60, 250], [20, 250]], [[90, 100], [180, 100], [180, 130], [90, 130]],
             [[100, 150], [130, 150], [130, 300], [100, 300]]]
    lines = [Quadrilateral(np.asarray(p, dtype=np.int64), "", 1.0) for p in np.asarray(quads)]
    assert len(lines) == 4
    kind.update({id(q): i % 3 for i, q in enumerate(lines)})
    plug = P.HipModelMangaOCR(weights={"mocr": sd}, vocab=vocab, mocr_config=cfg, generation=g, ocr48=Stub48())
    assert plug.is_downloaded()
    loop = asyncio.new_event_loop()
    try:
        loop.run_until_complete(plug.load("cuda"))
        got = loop.run_until_complete(plug.infer(page, lines, None, False))
    finally:
        loop.close()
    assert len(got) == len(lines) and {id(q) for q in got} == {id(q) for q in lines}
    want_text = plug.engine.recognize_lines(plug._page_on_device(page), got, [q.assigned_direction for q in got])
    for row, q in enumerate(got):
        k = kind[id(q)]
        if k != 1:
            assert abs(q.prob - (0.3 + 0.2 * k)) < 1e-12 and (q.fg_r, q.fg_g, q.fg_b) == (10 + k, 20, 30) and (q.bg_r, q.bg_g, q.bg_b) == (200, 210 + k, 220)
        else:
            assert q.prob == 0.0 and (q.fg_r, q.fg_g, q.fg_b, q.bg_r, q.bg_g, q.bg_b) == (0,) * 6
        toks = want_text["tokens"][row, :int(want_text["length"][row])].cpu().numpy()
        assert q.text == P.mocr_post_process(P.mocr_tokens_to_text(toks, vocab, (g.eos_token_id, g.pad_token_id, g.decoder_start_token_id)))
        assert q.text != "discarded"
    print("48px stand-in:", [(kind[id(q)], q.text, q.prob) for q in got])


def test_decode_refuses_what_it_does_not_implement(cuda):
    import dataclasses

    eng, _, crops, g = _engine(cuda, "early")
    mem_k, mem_v = eng.encode(eng.preprocess([torch.from_numpy(cr).to(cuda) for cr in crops]))
    with pytest.raises(RuntimeError, match="num_beams"):
        eng.decode(mem_k, mem_v, dataclasses.replace(g, num_beams=9))
    with pytest.raises(ValueError, match="max_length"):
        eng.decode(mem_k, mem_v, dataclasses.replace(g, max_length=1000))


# ---- kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(2, 2), (17, 300), (300, 17), (224, 224)])
def test_preprocessing_kernels(cuda, hw):
    """convert("L").convert("RGB") and the resize byte-exact against Pillow; the patch rows against the host statement."""
    from PIL import Image

    eng, c, _, _ = _engine(cuda, "vit48")
    crop = np.random.default_rng(hw[0]).integers(0, 256, size=(*hw, 3), dtype=np.uint8)
    pil = Image.fromarray(crop).convert("L").convert("RGB")
    assert np.array_equal(O.gray_rgb(crop), np.asarray(pil))
    got = eng.preprocess([torch.from_numpy(crop).to(cuda)])
    want = np.asarray(pil.resize((c.image_size, c.image_size), Image.BILINEAR))
    assert np.array_equal(got[0].cpu().numpy(), want)
    rows = eng.patch_rows(got).cpu()
    ref = O.patch_rows(O.normalize(want)[None], c.patch_size)
    assert rows.shape == ref.shape and (rows - ref).abs().max().item() <= 1e-6


@pytest.mark.parametrize("rows,D", [(1, 768), (5, 768), (9, 100), (3, 8192)])
def test_layernorm_wide(cuda, rows, D):
    """Bound: the output is O(|g| + |b|) ~ a few units; fp32 sums over D terms in a butterfly of partial sums keep the relative error of
    mean and variance near sqrt(D) * 6e-8 < 6e-6, so 2e-5 absolute on unit-scale rows (the bar of mit_layernorm's own test)."""
    import ctypes as C

    from manga_image_translator_amd import lib

    gen = torch.Generator().manual_seed(D + rows)
    x = torch.randn(rows, D + 8, generator=gen)
    w, b = torch.rand(D, generator=gen) + 0.5, torch.randn(D, generator=gen) * 0.1
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    out = torch.full((rows, D + 4), 7.0, device=cuda)
    L = lib.load()
    lib.check(L.mit_layernorm_wide(xd.data_ptr(), D + 8, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), D + 4, rows, D, 1e-12, None), "mit_layernorm_wide")
    torch.cuda.synchronize()
    ref = torch.nn.functional.layer_norm(x[:, :D].double(), (D,), w.double(), b.double(), 1e-12)
    assert (out[:, :D].cpu().double() - ref).abs().max().item() < 2e-5
    assert (out[:, D:] == 7.0).all()                          # nothing written past a row
    assert L.mit_layernorm_wide(xd.data_ptr(), D + 8, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), D + 4, rows, 8193, 1e-12, None) != 0
    assert b"mit_layernorm_wide" in L.mit_last_error()
