"""48px OCR stage parity: HIP engine vs the CPU oracle restatement of the reference model.

Tolerances: encoder memory / raw logits ("OCR logits" = pred(pred1(decoded)), model_48px.py:713) at
2e-4 * max|ref| (fp32, ~150 layers deep; observed ~1e-5); token ids, lengths and the beam history must be
identical (integer results) as long as no two candidates are closer than the float tolerance.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocr_setup(cuda, shipped_mode):
    from manga_image_translator_amd import ocr48, ocr_schema, synth

    D = 300
    sd = synth.synth_state_dict(ocr_schema.ocr48_schema(D))
    with shipped_mode():
        return sd, D, ocr48.Ocr48Engine(sd, D, device=cuda)


def _crops(widths, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(48, w, 3), dtype=np.uint8) for w in widths]


def _pooled_memory(eng, crops, cuda):
    """The encoder memory of every chunk of ``crops`` pooled for one ``decode``: mem_k / mem_v [5, N, Lmax, 320] (zero-padded), mem_len [N]."""
    mks, mvs, lens = [], [], []
    for indices, ws, region in eng.make_chunks(crops):
        mk, mv, kl, _ = eng.encode(torch.from_numpy(region).to(cuda), ws)
        mks.append(mk.clone()); mvs.append(mv.clone()); lens.append(kl.clone())
    Lmax = max(m.shape[2] for m in mks)
    pad = lambda m: m if m.shape[2] == Lmax else torch.cat([m, m.new_zeros(5, m.shape[1], Lmax - m.shape[2], 320)], 2)
    return torch.cat([pad(m) for m in mks], 1).contiguous(), torch.cat([pad(m) for m in mvs], 1).contiguous(), torch.cat(lens)


def _forms(L):
    """The decode's kernel forms (MitOcr48DecodeArgs.forms_off / forms_run) under short names."""
    return L.MIT_OCR48_FORM_ROWS, L.MIT_OCR48_FORM_LN_FUSED, L.MIT_OCR48_FORM_Q2_FUSED, L.MIT_OCR48_FORM_FF2_SPLITK, L.MIT_OCR48_FORM_SELF_ROWS


def test_encoder_memory_parity(cuda, gemm_mode, ocr_setup):
    from oracle import ocr48 as OO

    sd, D, eng = ocr_setup
    crops = _crops([50, 77, 120, 121, 64])
    for indices, widths, region in eng.make_chunks(crops):
        taps = {}
        mem_k, mem_v, klen, L = eng.encode(torch.from_numpy(region).to(cuda), widths, taps=taps)
        torch.cuda.synchronize()
        img = ((torch.from_numpy(region).float() - 127.5) / 127.5).permute(0, 3, 1, 2)
        with torch.no_grad():
            bb = OO.backbone(sd, img).squeeze(2).permute(0, 2, 1)
            mem, mask = OO.encode_lines(sd, img, widths)
        assert bb.shape == taps["backbone"].shape
        e1 = (taps["backbone"].cpu() - bb).abs().max().item()
        assert e1 < 2e-4 * bb.abs().max().item(), e1
        valid = ~mask
        e2 = ((taps["memory"].cpu() - mem).abs() * valid[..., None]).max().item()
        assert e2 < 2e-4 * mem.abs().max().item(), e2
        assert klen.cpu().tolist() == [min((w + 3) // 4 + 2, L) for w in widths]


def _check_beam_parity(cuda, sd, D, eng, crops, T, suppress, memo=None):
    from oracle import ocr48 as OO

    chunks = list(eng.make_chunks(crops))
    assert len(chunks) == 1
    indices, ws, region = chunks[0]
    mem_k, mem_v, klen, L = eng.encode(torch.from_numpy(region).to(cuda), ws)
    out = eng.decode(mem_k, mem_v, klen, max_seq_length=T, suppress_eos=suppress, trace=True)
    torch.cuda.synchronize()
    img = ((torch.from_numpy(region).float() - 127.5) / 127.5).permute(0, 3, 1, 2)
    def run_oracle():
        tr = []
        with torch.no_grad():
            r = OO.infer_beam_batch_tensor(sd, img, ws, max_seq_length=T, trace=tr, suppress_eos=suppress)
        return r, tr

    ref, trace = memo[0](memo[1], run_oracle) if memo is not None else run_oracle()
    N = len(ws)
    tl = out["trace_logits"].cpu()
    worst = 0.0
    # step-wise "OCR logits": compare log-softmax of our raw logits with the oracle's log-probs while all samples are alive
    for st in trace:
        s = st["step"]
        if s >= out["steps_run"]:
            break
        ref_lp = st["logp"]
        if s == 0:
            got = tl[0].reshape(N, 5, D)[:, 0]
        else:
            if ref_lp.shape[0] != N * 5:
                break  # the oracle compacted finished samples away; row mapping no longer 1:1
            got = tl[s]
        got_lp = got.log_softmax(-1)
        if suppress:
            got_lp[:, 2] = float("-inf")
            finite = torch.isfinite(ref_lp)
            err = (got_lp[finite] - ref_lp[finite]).abs().max().item()
        else:
            err = (got_lp - ref_lp).abs().max().item()
        assert err < 5e-4, (s, err)
        worst = max(worst, err)
    toks, lens, probs = out["tokens"].cpu(), out["length"].cpu(), out["prob"].cpu()
    for n, (r_idx, r_prob, fg, bg, fgi, bgi) in enumerate(ref):
        got_tok = toks[n, 1:lens[n]].tolist()
        assert got_tok == r_idx.tolist(), (n, got_tok, r_idx.tolist())
        assert abs(probs[n].item() - r_prob) < 1e-3 * max(r_prob, 1e-6) + 1e-7, (probs[n].item(), r_prob)
        nt = len(got_tok)
        col = out["colors"][n, :nt].cpu()
        refc = torch.cat([fg[:nt], bg[:nt], fgi[:nt], bgi[:nt]], dim=-1)
        assert (col - refc).abs().max().item() < 2e-4 * max(1.0, refc.abs().max().item())
    return worst


@pytest.mark.parametrize("widths,T,suppress", [([50, 77, 120, 121], 12, False), ([200, 33, 90], 10, True)])
def test_beam_search_parity(cuda, gemm_mode, ocr_setup, widths, T, suppress):
    sd, D, eng = ocr_setup
    _check_beam_parity(cuda, sd, D, eng, _crops(widths, seed=3), T, suppress)


def test_beam_search_parity_at_bench_config(cuda, gemm_mode, oracle_memo):
    """The bench's OCR workload: the 32 text lines of a synthetic 2048x1456 page (two chunks of 16, crop widths 180..600 px),
    dictionary of 6004 entries, 32 decode steps with EOS suppressed — per-step log-probs within 5e-4 of the oracle, token ids,
    probabilities and colour heads identical / within tolerance (model_48px.py:678-801)."""
    from manga_image_translator_amd import ocr48, ocr_schema, pipeline, synth
    from oracle import textline as OT

    D = pipeline.DICT_SIZE
    sd = synth.synth_state_dict(ocr_schema.ocr48_schema(D))
    eng = ocr48.Ocr48Engine(sd, D, device=cuda)
    page, quads, _ = synth.synth_page(0, 2048, 1456, n_boxes=32)
    crops = []
    for pts in quads:
        sp, vert = OT.sort_pnts(pts)
        crops.append(OT.get_transformed_region(page, sp, "v" if vert else "h", 48))
    order = sorted(range(len(crops)), key=lambda i: crops[i].shape[1])
    assert len(crops) == 32 and crops[order[0]].shape[1] >= 150 and crops[order[-1]].shape[1] <= 640
    for c in range(0, 32, 16):
        worst = _check_beam_parity(cuda, sd, D, eng, [crops[i] for i in order[c:c + 16]], 32, True, memo=(oracle_memo, ("ocr-bench", c)))
        print(f"gemm mode {gemm_mode} bench-config chunk {c // 16}: widths {crops[order[c]].shape[1]}..{crops[order[c + 15]].shape[1]}, worst per-step log-prob error {worst:.2e}")


def test_pooled_decode_equals_per_chunk(cuda, ocr_setup):
    """Lines of several chunks decoded together give the same tokens as chunk-by-chunk decoding."""
    sd, D, eng = ocr_setup
    crops = _crops([40 + 9 * i for i in range(20)], seed=5)
    pooled = eng.recognize(crops, max_seq_length=8, suppress_eos=True)
    torch.cuda.synchronize()
    toks = pooled["tokens"].cpu()
    pos = 0
    for indices, ws, region in eng.make_chunks(crops):
        mk, mv, kl, L = eng.encode(torch.from_numpy(region).to(cuda), ws)
        o = eng.decode(mk, mv, kl, max_seq_length=8, suppress_eos=True)
        assert torch.equal(o["tokens"].cpu(), toks[pos:pos + len(ws)])
        pos += len(ws)
    assert pooled["order"] == sorted(range(20), key=lambda i: crops[i].shape[1])


def test_group_encode_equals_per_chunk(cuda, ocr_setup):
    """encode_group (row-wise ops over all chunks at once, ragged depthwise conv) is bitwise the per-chunk encode()."""
    sd, D, eng = ocr_setup
    crops = _crops([40 + 13 * i for i in range(21)], seed=9)  # 2 chunks: 16 + 5 lines, different padded widths
    chunks = list(eng.make_chunks(crops))
    regions = [torch.from_numpy(r).to(cuda) for _, _, r in chunks]
    Ls = [eng.memory_len(r.shape[2]) for r in regions]
    Lmax = max(Ls)
    klens = torch.tensor([eng.valid_len(w, L) for (_, ws, _), L in zip(chunks, Ls) for w in ws], dtype=torch.int32, device=cuda)
    gk, gv, _ = eng.encode_group(regions, klens, Lmax)
    gk, gv = gk.clone(), gv.clone()
    l0 = 0
    for (_, ws, _), reg, L in zip(chunks, regions, Ls):
        mk, mv, kl, L1 = eng.encode(reg, ws)
        torch.cuda.synchronize()
        n = len(ws)
        assert L1 == L and torch.equal(kl, klens[l0:l0 + n])
        assert torch.equal(gk[:, l0:l0 + n, :L], mk) and torch.equal(gv[:, l0:l0 + n, :L], mv)
        assert not gk[:, l0:l0 + n, L:].any() and not gv[:, l0:l0 + n, L:].any()  # zero padding up to Lmax
        l0 += n


def test_ragged_xpos_attention_equals_the_per_chunk_launches(cuda, ocr_setup):
    """mit_attention_lines_xpos / mit_memory_kv_lines (one launch per encoder layer / decoder layer for all lines of a group, XPOS
    rotation folded in) against the per-chunk form of the same engine (mit_xpos_rotate x 2 + mit_attention per chunk): bitwise."""
    sd, D, eng = ocr_setup
    crops = _crops([30 + 11 * i for i in range(37)], seed=4)  # 3 chunks of 16 + 16 + 5 lines, three memory lengths
    chunks = list(eng.make_chunks(crops))
    regions = [torch.from_numpy(r).to(cuda) for _, _, r in chunks]
    Ls = [eng.memory_len(r.shape[2]) for r in regions]
    assert len(set(Ls)) == 3
    klens = torch.tensor([eng.valid_len(w, L) for (_, ws, _), L in zip(chunks, Ls) for w in ws], dtype=torch.int32, device=cuda)
    assert not eng.per_chunk_attention
    gk, gv, _ = eng.encode_group(regions, klens, max(Ls))
    gk, gv = gk.clone(), gv.clone()
    eng.per_chunk_attention = True
    try:
        pk, pv, _ = eng.encode_group(regions, klens, max(Ls))
    finally:
        eng.per_chunk_attention = False
    torch.cuda.synchronize()
    assert torch.equal(gk, pk) and torch.equal(gv, pv)
    assert gk.abs().sum() > 0


def test_lines_longer_than_the_lds_form_take_the_per_chunk_path(cuda, ocr_setup):
    """Crops around 1230-1600 px wide (aspect ratio 26-33: long vertical lines) give memory lengths past what mit_attention_lines_xpos
    holds in LDS (mit_attention_lines_xpos_max_len, 308 at head_dim 80).  The engine must derive its guard from the library's limit and
    encode such a group chunk by chunk — same result as forcing that path — instead of failing the page group (ADVICE r04, ocr48.py:320);
    a group right at the limit still takes the one-launch form; the C entry itself refuses the oversize line with an error, no launch."""
    from manga_image_translator_amd import lib as L_

    sd, D, eng = ocr_setup
    lib = L_.load()
    lim = lib.mit_attention_lines_xpos_max_len(80)
    assert lim == eng.lines_attention_max_len == 308 and lib.mit_attention_lines_xpos_max_len(81) == 0
    for widths, over in (([1300, 90, 1500], True), ([1216, 64], False)):
        crops = _crops(widths, seed=11)
        chunks = list(eng.make_chunks(crops))
        regions = [torch.from_numpy(r).to(cuda) for _, _, r in chunks]
        Ls = [eng.memory_len(r.shape[2]) for r in regions]
        assert (max(Ls) > lim) == over, (Ls, lim)
        klens = torch.tensor([eng.valid_len(w, Lc) for (_, ws, _), Lc in zip(chunks, Ls) for w in ws], dtype=torch.int32, device=cuda)
        gk, gv, _ = eng.encode_group(regions, klens, max(Ls))       # raised "do not fit the LDS form" for the first group before the fix
        gk, gv = gk.clone(), gv.clone()
        eng.per_chunk_attention = True
        try:
            pk, pv, _ = eng.encode_group(regions, klens, max(Ls))
        finally:
            eng.per_chunk_attention = False
        torch.cuda.synchronize()
        assert torch.equal(gk, pk) and torch.equal(gv, pv) and torch.isfinite(gk).all() and gk.abs().sum() > 0
    q = torch.zeros(lim + 1, 320, device=cuda)
    tab = torch.tensor([[0, lim + 1]], dtype=torch.int32, device=cuda)
    kl = torch.tensor([lim + 1], dtype=torch.int32, device=cuda)
    import ctypes as C
    rc = lib.mit_attention_lines_xpos(q.data_ptr(), q.data_ptr(), q.data_ptr(), q.data_ptr(), 320, tab.data_ptr(), kl.data_ptr(), 1, lim + 1, 4, 80,
                                      C.byref(eng.xpos), None)
    assert rc != 0 and b"mit_attention_lines_xpos_max_len" in lib.mit_last_error()


@pytest.mark.parametrize("G,Tk,heads,hd", [(5, 70, 4, 80), (5, 200, 4, 80), (3, 64, 8, 40), (8, 129, 2, 16)])
def test_shared_kv_attention_bitwise_equals_per_row(cuda, G, Tk, heads, hd):
    """The beams of a line share the K / V block (kv_div = beams): the shared-K/V kernel must give bit for bit what the
    one-wave-per-row kernel gives on the same K / V repeated per row, and match a float64 softmax(q k^T) v."""
    import ctypes as C

    from manga_image_translator_amd import lib as L, ops

    lib = L.load()
    g = torch.Generator().manual_seed(3)
    NL, E = 7, heads * hd
    q = torch.randn(NL * G, E, generator=g).to(cuda)
    k = torch.randn(NL, Tk, E, generator=g).to(cuda)
    v = torch.randn(NL, Tk, E, generator=g).to(cuda)
    klen = torch.tensor([Tk, 1, Tk // 2, Tk - 1, 3, Tk, 17][:NL], dtype=torch.int32, device=cuda)
    out_a, out_b = torch.zeros_like(q), torch.zeros_like(q)
    st = C.c_void_p(ops.current_stream())
    L.check(lib.mit_attention_heads(q.data_ptr(), E, E, k.data_ptr(), Tk * E, E, v.data_ptr(), Tk * E, E, out_a.data_ptr(), E, E,
                                    klen.data_ptr(), NL * G, 1, Tk, G, heads, hd, st), "shared")
    kr, vr = k.repeat_interleave(G, 0).contiguous(), v.repeat_interleave(G, 0).contiguous()
    klr = klen.repeat_interleave(G).contiguous()
    L.check(lib.mit_attention_heads(q.data_ptr(), E, E, kr.data_ptr(), Tk * E, E, vr.data_ptr(), Tk * E, E, out_b.data_ptr(), E, E,
                                    klr.data_ptr(), NL * G, 1, Tk, 1, heads, hd, st), "per-row")
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b)
    qd = q.double().cpu().view(NL, G, heads, hd)
    kd, vd = k.double().cpu().view(NL, Tk, heads, hd), v.double().cpu().view(NL, Tk, heads, hd)
    sc = torch.einsum("nghd,nthd->nght", qd, kd)
    mask = torch.arange(Tk)[None, :] >= klen.cpu()[:, None]
    sc = sc.masked_fill(mask[:, None, None, :], float("-inf"))
    ref = torch.einsum("nght,nthd->nghd", sc.softmax(-1), vd).reshape(NL * G, E)
    assert (out_a.double().cpu() - ref).abs().max() < 2e-5


@pytest.mark.parametrize("T,heads,hd", [(70, 4, 80), (142, 4, 80), (33, 8, 40), (16, 2, 16), (150, 1, 128)])
def test_row_attention_bitwise_equals_per_query(cuda, T, heads, hd):
    """The encoder's self-attention (every query position of a row at once, keys / values staged in LDS once per (head, row):
    attention_rows_kernel) must give bit for bit what the one-wave-per-query kernel gives when it is called one query position at a
    time, and match a float64 softmax(q k^T) v; padded keys (klen) masked, padded queries still computed."""
    import ctypes as C

    from manga_image_translator_amd import lib as L, ops

    lib = L.load()
    g = torch.Generator().manual_seed(5)
    R, E = 6, heads * hd
    q = torch.randn(R, T, E, generator=g).to(cuda)
    k = torch.randn(R, T, E, generator=g).to(cuda)
    v = torch.randn(R, T, E, generator=g).to(cuda)
    klen = torch.tensor([T, 1, T // 2, T - 1, 3, 17][:R], dtype=torch.int32, device=cuda).clamp_(max=T)
    out_a, out_b = torch.full_like(q, float("nan")), torch.full_like(q, float("nan"))
    st = C.c_void_p(ops.current_stream())
    L.check(lib.mit_attention_heads(q.data_ptr(), T * E, E, k.data_ptr(), T * E, E, v.data_ptr(), T * E, E, out_a.data_ptr(), T * E, E,
                                    klen.data_ptr(), R, T, T, 1, heads, hd, st), "rows")
    for t in range(T):   # Tq = 1: the per-query kernel
        L.check(lib.mit_attention_heads(q[:, t].data_ptr(), T * E, E, k.data_ptr(), T * E, E, v.data_ptr(), T * E, E, out_b[:, t].data_ptr(),
                                        T * E, E, klen.data_ptr(), R, 1, T, 1, heads, hd, st), "per-query")
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b)
    qd, kd, vd = (x.double().cpu().view(R, T, heads, hd) for x in (q, k, v))
    sc = torch.einsum("nqhd,nthd->nhqt", qd, kd)
    mask = torch.arange(T)[None, :] >= klen.cpu()[:, None]
    sc = sc.masked_fill(mask[:, None, None, :], float("-inf"))
    ref = torch.einsum("nhqt,nthd->nqhd", sc.softmax(-1), vd).reshape(R, T, E)
    assert (out_a.double().cpu() - ref).abs().max() < 5e-5   # fp32 dot products of 80-128 N(0,1) terms, outputs of order 1


@pytest.mark.parametrize("k,C_,H,shapes", [(7, 80, 24, [(2, 37), (1, 64), (3, 9)]), (7, 160, 12, [(1, 150), (2, 5)]), (5, 320, 6, [(2, 33), (1, 70)]),
                                           (3, 320, 3, [(2, 40)]), (5, 16, 8, [(1, 3), (1, 4)])])
def test_dwconv_ragged_rows_equals_per_row_kernel(cuda, k, C_, H, shapes):
    """mit_dwconv_nhwc_ragged_rows (YT output rows per thread, weights in LDS) == mit_dwconv_nhwc_ragged bit for bit: same fmaf
    chain per output.  Covers YT = 4 (H = 24, 12, 8), YT = 2 (H = 6), the fallback (H = 3), ragged right edges and W < 4."""
    import ctypes as C

    from manga_image_translator_amd import lib as L, ops
    from manga_image_translator_amd.lib import MitRaggedSeg

    g = torch.Generator().manual_seed(k * 100 + H)
    segs = (MitRaggedSeg * len(shapes))()
    pix = grp = 0
    for i, (n, w) in enumerate(shapes):
        segs[i].pixel_start, segs[i].group_start, segs[i].B, segs[i].H, segs[i].W = pix, grp, n, H, w
        pix += n * H * w
        grp += n * H * ((w + 3) // 4)
    x = torch.randn(pix, C_, generator=g).to(cuda)
    wt = torch.randn(k * k, C_, generator=g).to(cuda)
    sc, bi = (torch.rand(C_, generator=g) + 0.5).to(cuda), torch.randn(C_, generator=g).to(cuda)
    tab = torch.frombuffer(bytearray(bytes(segs)), dtype=torch.uint8).to(cuda)
    a, b = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    st = C.c_void_p(ops.current_stream())
    Lh = L.load()
    L.check(Lh.mit_dwconv_nhwc_ragged(x.data_ptr(), wt.data_ptr(), sc.data_ptr(), bi.data_ptr(), a.data_ptr(), tab.data_ptr(), len(shapes), grp,
                                      C_, k, st), "mit_dwconv_nhwc_ragged")
    L.check(Lh.mit_dwconv_nhwc_ragged_rows(x.data_ptr(), wt.data_ptr(), sc.data_ptr(), bi.data_ptr(), b.data_ptr(), tab.data_ptr(), len(shapes),
                                           grp, C_, k, H, st), "mit_dwconv_nhwc_ragged_rows")
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a, b)
    # and against torch's depthwise conv on the first segment
    n0, w0 = shapes[0]
    ref = torch.nn.functional.conv2d(x[:n0 * H * w0].view(n0, H, w0, C_).permute(0, 3, 1, 2).cpu().double(),
                                     wt.cpu().double().t().reshape(C_, 1, k, k), padding=k // 2, groups=C_)
    ref = ref * sc.cpu().double().view(1, -1, 1, 1) + bi.cpu().double().view(1, -1, 1, 1)
    got = b[:n0 * H * w0].view(n0, H, w0, C_).permute(0, 3, 1, 2).cpu().double()
    assert (got - ref).abs().max() < 1e-4


@pytest.mark.parametrize("widths,T,suppress", [([50, 77, 120, 121, 64, 200], 14, True), ([90, 33], 9, False), ([40 + 5 * i for i in range(40)], 6, True)])
def test_few_row_decode_equals_the_tiled_form(cuda, ocr_setup, widths, T, suppress):
    """The few-row form of a decode step (MIT_OCR48_FORM_ROWS: every Linear one wave per 32 x 32 block on bf16-plane
    activations, LayerNorm / attention kernels producing the planes) against the tiled form the full batches take: the plane split,
    the MFMA pair order and the epilogue arithmetic are the same, so tokens, lengths, probabilities and colours must be identical."""
    from manga_image_translator_amd import lib as L, ops

    sd, D, eng = ocr_setup
    mem_k, mem_v, klen = _pooled_memory(eng, _crops(widths, seed=5), cuda)
    ROWS, LN, Q2, SK, SELF = _forms(L)
    assert L.MIT_OCR48_ROWS_MAX >= 5 * len(widths), "the few-row form must be the default at these sizes"
    outs = []
    for off in (ROWS, SK):   # SK off: the one-chain FFN kernel, the k-sequential sum of the tiles (the K-cut form has its own test)
        o = eng.decode(mem_k, mem_v, klen, max_seq_length=T, suppress_eos=suppress, forms_off=off)
        torch.cuda.synchronize()
        outs.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()})
    assert outs[0]["forms_run"] & (ROWS | LN | Q2 | SK) == 0
    assert outs[1]["forms_run"] == ROWS | LN | SELF | (Q2 if ops.split_mode() == 6 else 0)
    for o in outs[1:]:
        assert o["steps_run"] == outs[0]["steps_run"]
        for k in ("tokens", "length", "prob", "colors"):
            assert torch.equal(o[k], outs[0][k]), k


@pytest.mark.parametrize("rows", [33, 128, 1000, 40000])
def test_fused_convnext_mlp_matches_the_two_launch_form(cuda, ocr_setup, rows):
    """mit_convnext_mlp (pwconv1 -> GELU -> pwconv2 -> gamma -> + input in one launch, hidden activations in registers; model_48px.py:203-214)
    against the two GEMM launches it replaces and against a float64 evaluation of the block's formula.  The first contraction is the
    tiles' own arithmetic; the second adds the same products with an MFMA step's 16 values in other k slots: differences of a few fp32
    ulps of the sums at most.  Ragged row counts (not a multiple of the 32-pixel wave tile / 128-row workgroup) included."""
    from manga_image_translator_amd import ops

    sd, D, eng = ocr_setup
    blk = eng.stages[0][0]
    assert blk.dim == 80
    g = torch.Generator().manual_seed(rows)
    t = torch.randn(rows, 80, generator=g).to(cuda)
    x0 = torch.randn(rows, 80, generator=g).to(cuda)
    h = torch.empty(rows, 320, device=cuda)
    with ops.gemm_mode(6, min_tiles=1):
        x1 = x0.clone()
        blk.mlp(t, h, x1, rows)
        x2 = x0.clone()
        blk.mlp(t, h, x2, rows, fused=False)
        x1b = x0.clone()
        blk.mlp(t, h, x1b, rows)
    torch.cuda.synchronize()
    assert torch.equal(x1, x1b)                                   # run-to-run identical
    p = "backbone.block1.0"
    w1, b1 = sd[p + ".pwconv1.weight"].double().reshape(320, 80), sd[p + ".pwconv1.bias"].double()
    w2, b2 = sd[p + ".pwconv2.weight"].double().reshape(80, 320), sd[p + ".pwconv2.bias"].double()
    gamma = sd[p + ".gamma"].double().reshape(-1)
    hid = torch.nn.functional.gelu(t.cpu().double() @ w1.t() + b1)
    ref = x0.cpu().double() + gamma * (hid @ w2.t() + b2)
    ymax = float(ref.abs().max())
    e_fused, e_two = float((x1.cpu().double() - ref).abs().max()) / ymax, float((x2.cpu().double() - ref).abs().max()) / ymax
    assert e_fused < 4 * e_two + 2e-6, (e_fused, e_two)
    assert float((x1 - x2).abs().max()) / ymax < 2e-6


@pytest.mark.parametrize("widths,T", [([50, 77, 120, 121, 64, 200], 14), ([40 + 5 * i for i in range(40)], 9)])
def test_row_staged_self_attention_is_bitwise_the_per_head_kernel(cuda, ocr_setup, widths, T):
    """attention_self_kernel (the decoder's self-attention with a row's key history staged once for its four heads) against
    attention_kernel (one single-wave workgroup per head and row): the whole beam search — tokens, lengths, probabilities, colours —
    must come out bit for bit the same (6 lines: the few-row decoder form with planar outputs; 40 lines: likewise, pooled)."""
    from manga_image_translator_amd import lib as L, ops

    sd, D, eng = ocr_setup
    mem_k, mem_v, klen = _pooled_memory(eng, _crops(widths, seed=3), cuda)
    ROWS, LN, Q2, SK, SELF = _forms(L)
    outs = []
    for off in (0, SELF, 0):
        r = eng.decode(mem_k, mem_v, klen, max_seq_length=T, suppress_eos=True, forms_off=off)
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in r.items() if torch.is_tensor(v)})
        assert r["forms_run"] == (ROWS | LN | SK | SELF | (Q2 if ops.split_mode() == 6 else 0)) & ~off   # 0: everything that ships
    assert {"tokens", "length", "prob", "colors"} <= set(outs[0])
    for other in outs[1:]:
        for k, v in outs[0].items():
            assert torch.equal(v, other[k]), k


@pytest.mark.parametrize("R,D,suppress", [(7, 6004, 2), (160, 6004, -1), (5, 2047, 0), (3, 300, -1), (4, 7000, 5)])
def test_register_form_of_logsoftmax_top5_is_bitwise_the_loop_form(cuda, R, D, suppress):
    """logsoftmax_top5_kernel<NJ>: a thread's elements loaded once and every pass on registers (all loads in flight together) against the
    loop form (loop_form = 1: three passes over the row, loads serialised by the candidate insertion): same elements per thread in
    the same order, same pairing across threads — the five values and the five indices must be identical, with ties
    (lower index first), a suppressed token and rows of -inf padding."""
    import ctypes as C
    from manga_image_translator_amd import lib as L, ops

    lib = L.load()
    g = torch.Generator().manual_seed(R * 131 + D)
    Dp = (D + 3) // 4 * 4
    x = torch.randn(R, Dp, generator=g) * 4
    x[:, ::97] = x[:, 5:6]              # exact ties spread over the threads
    x[R // 2:, ::97] = 20.0             # ... and, on half of the rows, ties among the winners
    x[0, : min(D, 40)] = float("-inf")  # a run of -inf entries
    x = x.to(cuda)
    outs = []
    for loop_form in (1, 0):
        vals = torch.empty(R, 5, device=cuda)
        idx = torch.empty(R, 5, dtype=torch.int32, device=cuda)
        L.check(lib.mit_logsoftmax_top5(x.data_ptr(), Dp, R, D, suppress, vals.data_ptr(), idx.data_ptr(), loop_form,
                                        C.c_void_p(ops.current_stream())), "mit_logsoftmax_top5")
        torch.cuda.synchronize()
        outs.append((vals.clone(), idx.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # and against torch (values within fp32 rounding; indices exactly, ties to the lower index)
    ref = x[:, :D].clone()
    if suppress >= 0:
        ref[:, suppress] = float("-inf")
    lp = torch.log_softmax(ref.double(), 1)
    order = torch.argsort(-lp, dim=1, stable=True)[:, :5]
    assert torch.equal(outs[1][1].long().cpu(), order.cpu())
    assert (outs[1][0].double() - torch.gather(lp, 1, order)).abs().max() < 2e-5


@pytest.mark.parametrize("widths,T,suppress", [([50, 77, 120, 121, 64, 200], 14, True), ([90, 33], 9, False), ([40 + 5 * i for i in range(40)], 6, True)])
def test_layernorm_inside_the_few_row_gemm_is_bit_identical(cuda, ocr_setup, widths, T, suppress):
    """pgemm_rows_ln_kernel (the decoder's norm1 / norm2 / norm3 computed by the waves of the Linear that consumes them, same butterfly
    as layernorm_kernel) against the two-launch form (MIT_OCR48_FORM_LN_FUSED off) and against the tiled form of full batches: every
    result tensor identical; 6, 2 and 40 lines = 30, 10 and 200 rows (ragged last row block).  The K-cut FFN Linear is off throughout."""
    from manga_image_translator_amd import lib as L, ops

    sd, D, eng = ocr_setup
    mem_k, mem_v, klen = _pooled_memory(eng, _crops(widths, seed=23), cuda)
    ROWS, LN, Q2, SK, SELF = _forms(L)
    outs = []
    for off in (LN | SK, SK, ROWS):
        o = eng.decode(mem_k, mem_v, klen, max_seq_length=T, suppress_eos=suppress, forms_off=off)
        torch.cuda.synchronize()
        outs.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()})
    assert outs[0]["forms_run"] == ROWS | SELF                    # (the q projection inside the cross-attention needs the fused LayerNorm)
    assert outs[1]["forms_run"] == ROWS | LN | SELF | (Q2 if ops.split_mode() == 6 else 0)
    assert outs[2]["forms_run"] & (ROWS | LN | Q2 | SK) == 0
    for o in outs[1:]:
        assert o["steps_run"] == outs[0]["steps_run"]
        for k in ("tokens", "length", "prob", "colors"):
            assert torch.equal(o[k], outs[0][k]), k


@pytest.mark.parametrize("widths,T,suppress", [([50, 77, 120, 121, 64, 200], 14, True), ([90, 33], 9, False), ([40 + 5 * i for i in range(32)], 12, True)])
def test_k_cut_ffn_linear_of_the_few_row_decode(cuda, ocr_setup, widths, T, suppress):
    """pgemm_rows_splitk_kernel (the FFN's K = 2048 Linear with K cut across four waves, summed in a fixed order; the default up to 640
    rows) against the one-chain kernel (MIT_OCR48_FORM_FF2_SPLITK off): a different fp32 rounding of the same sums — tokens and lengths
    must be identical, probabilities within 1e-4 relative (the oracle bar on log-probabilities is 5e-4), colour heads within 1e-4; run to
    run the K-cut form is bit-reproducible ."""
    from manga_image_translator_amd import lib as L, ops

    sd, D, eng = ocr_setup
    mem_k, mem_v, klen = _pooled_memory(eng, _crops(widths, seed=31), cuda)
    ROWS, LN, Q2, SK, SELF = _forms(L)
    outs = []
    for off in (SK, 0, 0):
        o = eng.decode(mem_k, mem_v, klen, max_seq_length=T, suppress_eos=suppress, forms_off=off)
        torch.cuda.synchronize()
        outs.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()})
        assert o["forms_run"] == (ROWS | LN | SK | SELF | (Q2 if ops.split_mode() == 6 else 0)) & ~off   # 0: everything that ships
    for k in ("tokens", "length", "prob", "colors"):
        assert torch.equal(outs[1][k], outs[2][k]), k
    assert outs[1]["steps_run"] == outs[0]["steps_run"]
    assert torch.equal(outs[1]["tokens"], outs[0]["tokens"]) and torch.equal(outs[1]["length"], outs[0]["length"])
    assert ((outs[1]["prob"] - outs[0]["prob"]).abs() <= 1e-4 * outs[0]["prob"].abs() + 1e-12).all()
    assert (outs[1]["colors"] - outs[0]["colors"]).abs().max() < 1e-4
    assert not torch.equal(outs[1]["colors"], outs[0]["colors"]) or len(widths) < 3   # (the K-cut kernel really ran)


@pytest.mark.parametrize("widths,T,suppress", [([50, 77, 120, 121, 64, 200], 14, True), ([90, 33], 9, False), ([40 + 5 * i for i in range(40)], 6, True)])
def test_q_projection_inside_the_cross_attention_is_bit_identical(cuda, ocr_setup, widths, T, suppress):
    """attention_shared_kv_kernel<..., QF> (norm2 and multihead_attn's q projection computed inside the decoder's cross-attention kernel:
    one wave normalises the line's five beams with layernorm_kernel's butterfly, three waves run pgemm_rows_kernel's K loop on the head's
    columns) against the separate launches (MIT_OCR48_FORM_Q2_FUSED off): every result tensor identical."""
    from manga_image_translator_amd import lib as L, ops

    sd, D, eng = ocr_setup
    mem_k, mem_v, klen = _pooled_memory(eng, _crops(widths, seed=41), cuda)
    ROWS, LN, Q2, SK, SELF = _forms(L)
    outs = []
    for off in (Q2, 0):
        o = eng.decode(mem_k, mem_v, klen, max_seq_length=T, suppress_eos=suppress, forms_off=off)
        torch.cuda.synchronize()
        outs.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()})
        assert o["forms_run"] == (ROWS | LN | SK | SELF | (Q2 if ops.split_mode() == 6 else 0)) & ~off   # 0: everything that ships
    for o in outs[1:]:
        assert o["steps_run"] == outs[0]["steps_run"]
        for k in ("tokens", "length", "prob", "colors"):
            assert torch.equal(o[k], outs[0][k]), k


@pytest.mark.parametrize("n_lines,T", [(1, 8), (129, 5), (140, 5)])
def test_few_row_decode_at_the_edges_of_its_forms(cuda, ocr_setup, n_lines, T):
    """One line (5 rows: a single ragged row block), 129 lines (past the 128 the q-projecting cross-attention takes: separate launches) and
    140 lines (700 rows: past the 640 the K-cut FFN Linear takes: the one-chain K = 2048 kernel) against the tiled form, with the K-cut
    off — every result tensor identical.  Past 640 rows nothing switches the K-cut off but the row count: that leg is what ships."""
    from manga_image_translator_amd import lib as L, ops

    sd, D, eng = ocr_setup
    mem_k, mem_v, klen = _pooled_memory(eng, _crops([48 + (7 * i) % 90 for i in range(n_lines)], seed=53), cuda)
    ROWS, LN, Q2, SK, SELF = _forms(L)
    outs = []
    for off in (ROWS, SK if 5 * n_lines <= 640 else 0):
        o = eng.decode(mem_k, mem_v, klen, max_seq_length=T, suppress_eos=True, forms_off=off)
        torch.cuda.synchronize()
        outs.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()})
    assert outs[0]["forms_run"] & (ROWS | LN | Q2 | SK) == 0
    assert outs[1]["forms_run"] == ROWS | LN | SELF | (Q2 if ops.split_mode() == 6 and n_lines <= 128 else 0)
    for k in ("tokens", "length", "prob", "colors"):
        assert torch.equal(outs[1][k], outs[0][k]), k
