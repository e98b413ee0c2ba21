"""What tests/_glue_cases.py promises about its own inputs, asserted without a GPU: a wrong test input fails here, not silently on
the device.  Nothing below calls the library."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _glue_cases as G  # noqa: E402

f32, f64 = np.float32, np.float64


def _adjacent(a, b):
    return bool((np.nextafter(a, f32(np.inf)) == b).all() and (a < b).all())


def test_all_256_bytes_occur_in_each_channel():
    img = G.all_bytes_image()
    for c in range(3):
        assert set(img[:, c].tolist()) == set(range(256))
    for Cin in (3, 4):
        page = G.ffd_all_bytes_page(Cin)
        for c in range(Cin):
            assert set(page[0, ..., c].ravel().tolist()) == set(range(256))
        assert G.ffd_pmax(page)[0] == 255


def test_float32_sigmoid_is_exact_at_the_exact_gates():
    assert G.bits_equal(G.sigmoid32(np.asarray(G.EXACT_GATES, f32)), np.array([1.0, 0.5, 0.0], f32))
    # ... with room for an expf a few ulp off: 1 + e rounds to 1 for any e below 2^-24, and e^-30 is 9.4e-14; e^200 overflows fp32
    assert float(np.exp(f64(-30.0))) * 1.001 < 2.0 ** -24 and float(np.exp(f64(200.0))) > 1e3 * float(np.finfo(f32).max)


def test_aot_post_signal_pairs_straddle_every_byte_boundary():
    ks = np.arange(1, 256)
    for gate, sig in ((30.0, 1.0), (0.0, 0.5)):
        v = G.aot_post_signals(gate)
        a, b = v[:255], v[255:510]
        assert _adjacent(a, b)
        assert np.array_equal(G.aot_post_byte(a, sig), ks - 1) and np.array_equal(G.aot_post_byte(b, sig), ks)
    assert G.aot_post_signals(-200.0).size == 12
    extra = G.aot_post_signals(-200.0)
    assert np.signbit(extra[0]) and extra[0] == 0 and f32(1.0) / f32(1.8) in extra and f32(1e30) in extra and f32(-10) in extra


def test_aot_post_case_meets_every_pair_in_every_mask_band():
    s, g = G.aot_post_pairs()
    assert set(g.tolist()) == set(G.EXACT_GATES)
    for ps in (6, 8):
        c = G.aot_post_case(ps)
        assert sorted(set(c["mask"].ravel().tolist())) == list(G.MASK_ROWS)
        for r, mk in enumerate(G.MASK_ROWS):
            rows = slice(r * c["band"], (r + 1) * c["band"])
            assert (c["mask"][0, rows] == mk).all()
            got = set(zip(c["pre"][0, rows, :, :3].ravel().view(np.int32).tolist(), c["pre"][0, rows, :, 3:6].ravel().tolist()))
            assert got == set(zip(s.view(np.int32).tolist(), g.tolist()))
        # the page differs from the network's byte on most pixels, so handing back the wrong one shows
        ref0, _ = G.aot_post_ref(c["pre"], c["img"], c["mask"], 0)
        assert (ref0 != c["img"]).mean() > 0.9


def test_aot_post_float32_restatement_agrees_with_float64_at_the_exact_gates():
    """At gates 30 / 0 / -200 the float64 value of s * sigmoid(g) * 1.8 differs from the float32 one by rounding only, and the bisected
    signals are the float32 boundaries: away from them (every signal moved 4e-6 off its boundary, 5e-4 of a byte or more, where
    float32 loses about 5e-5 of one) the float64 bytes must agree."""
    s, g = G.aot_post_pairs()
    fin = np.abs(s) < 1e29
    for d in (-4e-6, 4e-6):
        sv = s[fin] + f32(d)
        q32 = G.aot_post_byte(sv, 1.0 * G.sigmoid32(g[fin]))
        v64 = np.clip(sv.astype(f64) * G.sigmoid64(g[fin]) * f64(f32(1.8)), -1, 1)
        q64 = np.floor((v64 + 1.0) * 127.5).astype(np.uint8)
        assert np.array_equal(q32, q64)
    pc = G.aot_post_ref(*[G.aot_post_case(6)[k] for k in ("pre", "img", "mask")], 1)[1]
    assert np.isfinite(pc).all() and np.signbit(pc[pc == 0]).any()


def test_gate_and_blend_cases_hold_what_they_claim():
    c = G.gate_case(4, 1000, 16)
    assert set(c["g"][c["exact"]].tolist()) == set(G.EXACT_GATES) and c["g"].min() < -19 and c["g"].max() > 19
    assert (c["buf"][:, 8:] == G.SENT).all()
    for relu in (0, 1):
        r32, r64 = G.gate_ref(c["s"], c["g"], relu, f32), G.gate_ref(c["s"], c["g"], relu, f64)
        e32, bar, _ = G.errors(r32, r64)
        assert 0 < e32 < 1e-6
        if relu:
            assert (r32 >= 0).all() and (r32[(c["s"] < 0) & (c["g"] > -80)] == 0).all()
    b = G.blend_case(3, 37, 4)
    k, g1, m1 = b["kind"], b["gate"][..., 1], b["mean"][:, None, 1]
    assert (b["istd"][:, 1] == f32(1e9)).all() and (np.abs(b["mean"][:, 1]) >= 0.5).all()
    assert (g1[k == 0] == np.broadcast_to(m1, k.shape)[k == 0]).all() and (g1[k == 1] > np.broadcast_to(m1, k.shape)[k == 1]).all()
    r32, m32 = G.blend_ref(b, f32)
    r64, m64 = G.blend_ref(b, f64)
    assert G.bits_equal(m32[..., 1][k == 0], np.full((k == 0).sum(), G.sigmoid32(-5.0), f32))
    assert G.bits_equal(r32[..., 1][k == 1], b["fuse"][..., 1][k == 1]) and G.bits_equal(r32[..., 1][k == 2], b["x"][..., 1][k == 2])
    z2 = np.abs(b["gate"][..., 2].astype(f64) - b["mean"][:, None, 2]) * b["istd"][:, None, 2]
    assert (np.abs(z2 - 0.5) < 0.03).all()
    assert len({tuple(r) for r in b["mean"].tolist()}) == 3                          # a wrong b * C offset reads other statistics
    assert G.errors(r32, r64)[0] < 1e-5


def test_plane_stats_cases():
    for C, hw in G.STATS_SHAPES:
        assert C & (C - 1) == 0 and hw >= 2
    assert {hw for _, hw in G.STATS_SHAPES} >= {511, 512, 513} and {C for C, _ in G.STATS_SHAPES} >= {4, 1024}
    x = G.stats_case(3, 513, 4)
    mean, istd = G.stats_ref(x)
    assert (np.abs(mean[:, 1]) * istd[:, 1] > 1e4).all()                             # |mean| >> std
    xc, cst = G.stats_constant_case(3, 5, 4)
    assert set(cst.ravel().view(np.int32).tolist()) == set(np.asarray(G.STATS_CONSTANTS, f32).view(np.int32).tolist())
    assert (xc == cst[:, None]).all()
    assert G.STATS_CONSTANTS[2] > f32(1e3) and f32(1.0) / (f32(0.0) + f32(1e-9)) == f32(1e9)
    # n copies of one fp32 value sum exactly in double for n <= 1073, so mean == c can be asked bit for bit
    for c in G.STATS_CONSTANTS:
        assert f32(sum([float(c)] * 1073) / 1073.0) == c


def test_ffd_cases():
    for H, W in G.FFD_SIDES:
        for Cin in (3, 4):
            img = G.ffd_pages(H, W, Cin)
            assert G.ffd_pmax(img).tolist() == [0, 1, 2] and (Cin == 3 or (img[..., 3] == 255).all())
            pm, out = G.ffd_pack_ref(img)
            assert out.shape == (3, (H + 1) // 2, (W + 1) // 2, 16) and (out[..., 15] == 0).all() and (out[..., :3] == f32(G.SIGMA)).all()
            assert set(out[1, ..., 3:15].ravel().tolist()) <= {0.0, 1.0} and out[1, ..., 3:15].max() == 1.0      # unnormalised
            assert out[2, ..., 3:15].max() == f32(2 / 255.)
    page = G.ffd_dim_rgba_page()
    assert G.ffd_pack_ref(page)[1][..., 3:15].max() == 1.0
    # float32(v / 255.) (double division, one rounding) against v * (1.f / 255.f): they differ, so the test can tell them apart
    v = np.arange(256)
    assert (np.float32(v / 255.) != v.astype(f32) * (f32(1.0) / f32(255.0))).any()
    assert np.array_equal(np.float32(v / 255.), v.astype(f32) / f32(255.0))          # ... but fp32 division is the same rounding


def test_ffd_unpack_noise_pairs_straddle_every_byte_boundary():
    ks = np.arange(1, 256)
    v = G.ffd_unpack_noise_values()
    a, b = v[:255], v[255:510]
    assert _adjacent(a, b)
    assert np.array_equal(G.ffd_unpack_byte(a), ks) and np.array_equal(G.ffd_unpack_byte(b), ks - 1)      # falls as the noise rises
    for d in (-4e-6, 4e-6):   # 1e-3 of a byte off the float32 boundaries, float64 yields the same bytes
        n = v[:510] + f32(d)
        q64 = np.floor(np.clip(1.0 - n.astype(f64), 0.0, 1.0) * 255.0).astype(np.uint8)
        assert np.array_equal(G.ffd_unpack_byte(n), q64)
    for Cin, ps in ((3, 12), (4, 16)):
        img, noise = G.ffd_unpack_boundary_case(Cin, ps)
        pm = G.ffd_pmax(img)
        assert pm.tolist() == [255, 1]
        ref = G.ffd_unpack_ref(img, pm, noise)
        assert set(ref[0].ravel().tolist()) == set(range(256))
        assert set(ref[1][img[1, ..., :3][..., ::-1] == 1].tolist()) == set(range(256))                  # the same on the unnormalised page
        assert ps == 12 or (noise[..., 12:] == f32(1e30)).all()
        # every value lands on some element of each page
        for b_ in range(2):
            up = np.stack([noise[b_, :, :, c * 4 + i * 2 + j] for c in range(3) for i in range(2) for j in range(2)])
            assert set(v.view(np.int32).tolist()) <= set(up.ravel().view(np.int32).tolist())
        img, noise = G.ffd_unpack_unnormalised_case(Cin, ps)
        assert G.ffd_pmax(img).tolist() == [1, 1] and noise[..., :12].min() < -0.9


def test_ffd_unpack_position_case_tells_slots_apart():
    for Cin, ps in ((3, 12), (4, 16)):
        img, noise = G.ffd_unpack_position_case(Cin, ps)
        pm = G.ffd_pmax(img)
        ref = G.ffd_unpack_ref(img, pm, noise)
        swapped = noise.copy()
        swapped[..., [1, 2, 5, 6, 9, 10]] = noise[..., [2, 1, 6, 5, 10, 9]]          # i and j exchanged
        other = G.ffd_unpack_ref(img, pm, swapped)
        odd = np.zeros(ref.shape[1:3], bool)
        odd[1::2, 0::2] = odd[0::2, 1::2] = True
        assert (ref[:, odd] != other[:, odd]).all()
        rolled = noise.copy()
        rolled[..., :12] = np.roll(noise[..., :12], 4, -1)                           # channels exchanged
        assert (G.ffd_unpack_ref(img, pm, rolled) != ref).all()


def test_gen_in_cases():
    for h, w, Hp, Wp in G.GEN_IN_SHAPES:
        assert Hp == h or Wp == w
        p = G.gen_in_case(h, w)
        ref = G.gen_in_ref(p, Hp, Wp)
        assert G.bits_equal(ref[:, :h, :w, 0], p.astype(f32) / f32(255.0)) and (ref[..., 1:] == 0).all()
        if Hp > h:
            assert np.array_equal(ref[:, h:, :, 0], np.broadcast_to((p.max(1).astype(f32) / f32(255.0))[:, None], (2, Hp - h, w)))
        if Wp > w:
            assert np.array_equal(ref[:, :, w:, 0], np.broadcast_to((p.max(2).astype(f32) / f32(255.0))[:, :, None], (2, h, Wp - w)))
        if h * w > 1:
            assert not np.array_equal(p[0].max(0), p[1].max(0)) and not np.array_equal(p[0].max(1), p[1].max(1))
        assert np.array_equal(ref.astype(f64)[..., 0], np.float32(np.pad(p, ((0, 0), (0, Hp - h), (0, Wp - w)), "maximum") / 255.))


def test_mc2_post_margins():
    x, k = G.post_margin_inputs()
    assert x.size == 765
    p64 = G.post_value64(x)
    assert (np.abs(p64 - np.round(p64)) >= 0.2499).all()                             # the float64 value is far from a boundary ...
    p32 = ((np.tanh(x) * f32(0.5) + f32(0.5)) * f32(255.0)).astype(f64)
    assert np.abs(p32 - p64).max() / 255.0 <= 1.8e-5                                 # ... next to what float32 loses
    assert np.array_equal(G.post_ref64(x), k) and np.array_equal(G.post_ref32(x), k)
    xb = G.post_boundary_inputs()
    assert xb.size == 3 * 254 and np.abs(G.post_ref32(xb).astype(int) - G.post_ref64(xb).astype(int)).max() <= 1
    assert G.post_ref64(np.asarray(G.POST_SPECIALS, f32)).tolist() == [127, 127, 254, 0, 255, 0, 255, 0, 255, 0]
    # x = 9 is the one special that float32 cannot place: 254.99999612 in float64, but tanh(9) * 0.5 + 0.5 rounds to 1.0 in float32
    assert G.post_ref32(np.asarray(G.POST_SPECIALS, f32)).tolist() == [127, 127, 255, 0, 255, 0, 255, 0, 255, 0]
    assert 255.0 - float(G.post_value64(9.0)) < 4e-6
    pre = G.post_case(x, 2, 8, 40, 5, 33, 4)
    assert set(x.view(np.int32).tolist()) <= set(pre[:, :5, :33, :3].ravel().view(np.int32).tolist()) and (pre[..., 3] == f32(1e30)).all()
