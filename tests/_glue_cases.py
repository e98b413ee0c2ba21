"""Inputs and numpy references for the direct tests of the AOT and mc2 glue kernels (tests/test_aot_kernels_gpu.py,
tests/test_mc2_kernels_gpu.py), and what tests/test_glue_cases.py asserts about those inputs on the CPU.

Every reference restates the expression of the reference line the kernel's own comment cites (manga_translator/...):

  mit_aot_gate         signal * sigmoid(gate) * 1.8, relu(x) * 1.7139588594436646        inpainting/inpainting_aot.py:128-133, :35-36
  mit_aot_plane_stats  mean, 1 / (std(unbiased) + 1e-9)                                   inpainting_aot.py:163-165
  mit_aot_blend        m = sigmoid(5 (2 (g - mean) istd - 1)); x (1 - m) + fuse m         inpainting_aot.py:166-167, :189-192
  mit_aot_post         s * sigmoid(g) * 1.8, clip(-1, 1), ((v + 1) * 127.5) truncated,    inpainting_aot.py:133, :274,
                       composited where mask >= 127                                       inpainting_lama_mpe.py:114, :57-61, :117
  mit_se_*             x * sigmoid(conv2(relu(conv1(mean(x)))))                           manga_colorization_v2_utils/networks/models.py:88-106
  mit_mc2_ffd_pack     np.float32(x / 255.) if x.max() > 1.2, space-to-depth + sigma      denoising/denoiser.py:79-103, functions.py:16-56
  mit_mc2_ffd_unpack   clamp(x - noise, 0, 1), (v * 255) truncated, RGB -> BGR            functions.py:58-83, denoiser.py:107-118, utils.py:17-33
  mit_mc2_gen_in       np.pad(.., 'maximum'), ToTensor                                    utils/utils.py:27-38, manga_colorization_v2.py:58-59
  mit_mc2_post         (tanh(y) * 0.5 + 0.5) * 255 truncated                              manga_colorization_v2.py:61-74

numpy float32 arithmetic is IEEE with one rounding per operation; the library is built with -ffp-contract=off, so a kernel whose
expression has no transcendental (or has one only where it is exact) must reproduce these bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64
SENT = f32(-7.0)
OVER_CAP = 256 * 4096 + 257            # work items: one full grid of the elementwise kernels, then a second trip with a ragged tail
EXACT_GATES = (30.0, 0.0, -200.0)      # fp32 1 / (1 + expf(-g)) is exactly 1, 0.5, 0 here
RELU_NF = 1.7139588594436646           # relu_nf, inpainting_aot.py:35-36
MASK_ROWS = (0, 126, 127, 128, 255)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def bits_equal(got, ref):
    """fp32 arrays compared as bit patterns (so -0.0 != 0.0)."""
    got, ref = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(ref, dtype=f32)
    return got.shape == ref.shape and np.array_equal(got.view(np.int32), ref.view(np.int32))


def trunc_u8(p):
    """astype(np.uint8) of a float array already inside [0, 256): truncation."""
    assert p.dtype == f32
    return p.astype(np.int32).astype(np.uint8)


def around(vals):
    """Each value with its two fp32 neighbours."""
    vals = np.asarray(vals, f32)
    return np.concatenate([np.nextafter(vals, f32(-np.inf)), vals, np.nextafter(vals, f32(np.inf))]).astype(f32)


def sigmoid32(g):
    g = np.asarray(g, f32)
    with np.errstate(over="ignore"):
        r = f32(1.0) / (f32(1.0) + np.exp(-g))
    assert r.dtype == f32
    return r


def sigmoid64(g):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(g, f64)))


def _key(v):
    """fp32 -> int64, monotone in the value (-0.0 -> -1, +0.0 -> 0)."""
    b = np.asarray(v, f32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF) - 1)


def _unkey(k):
    k = np.asarray(k, np.int64)
    b = np.where(k >= 0, k, (-(k + 1)) | 0x80000000).astype(np.uint32)
    return b.view(f32)


def bisect_f32(byte_fn, lo, hi):
    """For every k in 1..255: the two ADJACENT fp32 values (a < b) between which the monotone ``byte_fn`` (fp32 array -> u8 array)
    crosses k, found by bisection over bit patterns between lo and hi.  Returns (a [255], b [255])."""
    ks = np.arange(1, 256)
    lo, hi = _key(np.full(255, lo, f32)), _key(np.full(255, hi, f32))
    plo, phi = byte_fn(_unkey(lo)) >= ks, byte_fn(_unkey(hi)) >= ks
    assert (plo != phi).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        same = (byte_fn(_unkey(mid)) >= ks) == plo
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    return _unkey(lo), _unkey(hi)


def all_bytes_image(npix=768):
    """RGB pixels: in the first 768, every byte value 0..255 occurs in each of the three channel positions."""
    i = np.arange(npix)
    return np.stack([i % 256, (i + 85) % 256, (255 - i) % 256], -1).astype(np.uint8)


def strided(arr, bs, ps, fill=SENT, lead=0, tail=8):
    """arr [B, n, C] placed at batch / pixel strides (floats) inside a flat buffer filled with ``fill``."""
    B, n, C = arr.shape
    assert ps >= C and bs >= n * ps and lead % 4 == 0
    buf = np.full(lead + B * bs + tail, fill, f32)
    view(buf, B, n, C, bs, ps, lead)[...] = arr
    return buf


def view(buf, B, n, C, bs, ps, lead=0):
    return np.lib.stride_tricks.as_strided(buf[lead:], (B, n, C), (bs * 4, ps * 4, 4))


def untouched_outside(buf, B, n, C, bs, ps, lead=0, fill=SENT):
    """True when every float of ``buf`` outside the [B, n, C] view still holds ``fill``."""
    chk = buf.copy()
    view(chk, B, n, C, bs, ps, lead)[...] = fill
    return bool((chk == fill).all())


def errors(r32, r64, got=None):
    """(e32, bar, kernel error): max-abs errors of the float32 restatement and of the kernel against the float64 truth, relative to
    max |truth|; the kernel's bar is 4 * e32 (the factor tests/test_mc2_gpu.py uses for its taps)."""
    r64 = np.asarray(r64, f64)
    den = max(float(np.abs(r64).max()), 1e-30)
    e32 = float(np.abs(np.asarray(r32, f64) - r64).max()) / den
    ek = None if got is None else float(np.abs(np.asarray(got, f64) - r64).max()) / den
    return e32, 4.0 * e32, ek


# ---- mit_aot_gate ----------------------------------------------------------------------------------------------------------------
def gate_case(C, npix, in_ps, seed=0):
    """dict(buf [npix, in_ps] = (signal | gate | sentinel), s, g, exact): gates over [-20, 20], every 7th one of EXACT_GATES."""
    rng = np.random.default_rng(1000 + seed)
    s = rng.standard_normal((npix, C)).astype(f32)
    g = rng.uniform(-20, 20, (npix, C)).astype(f32)
    i = np.arange(npix * C).reshape(npix, C)
    exact = i % 7 == 0
    g[exact] = np.asarray(EXACT_GATES, f32)[(i[exact] // 7) % 3]
    buf = np.full((npix, in_ps), SENT, f32)
    buf[:, :C], buf[:, C:2 * C] = s, g
    return dict(buf=buf, s=s, g=g, exact=exact)


def gate_ref(s, g, relu_nf, dt):
    sg = sigmoid32(g) if dt is f32 else sigmoid64(g)
    v = s.astype(dt) * sg * dt(1.8)
    if relu_nf:
        v = np.maximum(v, dt(0.0)) * dt(RELU_NF)
    assert v.dtype == dt
    return v


# ---- mit_aot_post ----------------------------------------------------------------------------------------------------------------
def aot_post_byte(s, sig):
    v = s * f32(sig) * f32(1.8)
    v = np.minimum(np.maximum(v, f32(-1.0)), f32(1.0))
    return trunc_u8((v + f32(1.0)) * f32(127.5))


def aot_post_signals(gate):
    """The signals paired with ``gate`` (one of EXACT_GATES): for every k the adjacent pair where the byte turns k - 1 -> k, then
    -0.0, 0, +-1/1.8 with their neighbours, +-10, +-1e30."""
    extra = np.concatenate([np.array([-0.0, 0.0], f32), around([f32(1.0) / f32(1.8), -(f32(1.0) / f32(1.8))]),
                            np.array([10, -10, 1e30, -1e30], f32)])
    sig = float(sigmoid32(gate))
    if sig == 0.0:
        return extra
    a, b = bisect_f32(lambda s: aot_post_byte(s, sig), -4.0, 4.0)
    return np.concatenate([a, b, extra])


_POST_PAIRS = []


def aot_post_pairs():
    """[(signal, gate)]: every signal of aot_post_signals with its exact gate."""
    if not _POST_PAIRS:
        sv = [aot_post_signals(g) for g in EXACT_GATES]
        _POST_PAIRS.append((np.concatenate(sv), np.concatenate([np.full(v.size, g, f32) for v, g in zip(sv, EXACT_GATES)])))
    return _POST_PAIRS[0]


def aot_post_case(pixstride, H=45, W=64):
    """One page whose rows carry mask values MASK_ROWS in H / 5-row bands; the channel elements of a band cycle through
    aot_post_pairs from the band's start, so each band meets every pair (H * W * 3 / 5 >= the number of pairs)."""
    s, g = aot_post_pairs()
    band = H // len(MASK_ROWS)
    assert band * len(MASK_ROWS) == H and band * W * 3 >= s.size
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    e = (((y % band) * W + x) * 3 + c) % s.size
    pre = np.full((1, H, W, pixstride), 1e30, f32)
    pre[0, ..., :3], pre[0, ..., 3:6] = s[e], g[e]
    mask = np.repeat(np.asarray(MASK_ROWS, np.uint8), band)[None, :, None].repeat(W, 2)
    img = np.random.default_rng(5).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    return dict(pre=pre, img=img, mask=mask, band=band)


def aot_post_ref(pre, img, mask, composite):
    """(u8 [.., 3], the fp32 product before the clip).  Exact in float32 only at EXACT_GATES."""
    s, g = pre[..., :3], pre[..., 3:6]
    pc = s * sigmoid32(g) * f32(1.8)                                                 # inpainting_aot.py:133
    v = np.minimum(np.maximum(pc, f32(-1.0)), f32(1.0))                              # :274
    q = trunc_u8((v + f32(1.0)) * f32(127.5))                                        # inpainting_lama_mpe.py:114
    keep = np.full(mask.shape, True) if not composite else mask >= 127               # :57-61, :117
    return np.where(keep[..., None], q, img), pc


# ---- mit_aot_blend ---------------------------------------------------------------------------------------------------------------
def blend_case(B, hw, C, seed=0):
    """x, fuse, gate [B, hw, C], mean / istd [B, C] chosen per (b, c).  Channel 1 has istd = 1e9 and |mean| in [0.5, 1): its pixels
    cycle gate == mean, one ulp above, one ulp below.  Channel 2 sits at |gate - mean| * istd ~ 0.5, where the sigmoid is steepest."""
    rng = np.random.default_rng(2000 + seed)
    x, fuse = rng.standard_normal((B, hw, C)).astype(f32), rng.standard_normal((B, hw, C)).astype(f32)
    mean = rng.uniform(-1, 1, (B, C)).astype(f32)
    istd = rng.uniform(0.5, 2, (B, C)).astype(f32)
    z = rng.uniform(-1, 2, (B, hw, C))
    z[..., 2] = 0.5 + rng.uniform(-0.02, 0.02, (B, hw))
    gate = (mean[:, None] + z / istd[:, None]).astype(f32)
    mean[:, 1] = rng.uniform(0.5, 1, B).astype(f32) * np.where(np.arange(B) % 2, -1, 1).astype(f32)
    istd[:, 1] = f32(1e9)
    m1 = np.broadcast_to(mean[:, None, 1], (B, hw))
    kind = np.broadcast_to((np.arange(hw) + np.arange(B)[:, None]) % 3, (B, hw))
    gate[..., 1] = np.where(kind == 0, m1, np.where(kind == 1, np.nextafter(m1, f32(np.inf)), np.nextafter(m1, f32(-np.inf))))
    return dict(x=x, fuse=fuse, gate=gate, mean=mean, istd=istd, kind=kind)


def blend_ref(c, dt):
    x, f, g = (c[k].astype(dt) for k in ("x", "fuse", "gate"))
    mu, si = c["mean"].astype(dt)[:, None], c["istd"].astype(dt)[:, None]
    z = dt(5.0) * (dt(2.0) * (g - mu) * si - dt(1.0))                                # my_layer_norm :166-167, sigmoid :191
    m = sigmoid32(z) if dt is f32 else sigmoid64(z)
    r = x * (dt(1.0) - m) + f * m                                                    # :192
    assert r.dtype == dt
    return r, m


# ---- mit_aot_plane_stats ---------------------------------------------------------------------------------------------------------
STATS_SHAPES = [(C, hw) for C in (4, 16, 128, 1024) for hw in (2, 511, 512, 513, 1073)]
STATS_CONSTANTS = (f32(0.1), f32(-40.0), np.nextafter(f32(1e3), f32(np.inf)), f32(0.0))


def stats_case(B, hw, C, seed=0):
    """x [B, hw, C]; channel 1 has |mean| >> std (1e3 +- 1e-2), channel 2 of page 1 sits at -40 +- 1e-3."""
    rng = np.random.default_rng(3000 + seed)
    x = (rng.standard_normal((B, hw, C)) * 2.0 + 0.5).astype(f32)
    x[..., 1] = (1e3 + 1e-2 * rng.standard_normal((B, hw))).astype(f32)
    x[1, :, 2] = (-40.0 + 1e-3 * rng.standard_normal(hw)).astype(f32)
    return x


def stats_constant_case(B, hw, C):
    """Plane (b, c) is the constant STATS_CONSTANTS[(b + c) % 4]."""
    k = (np.arange(B)[:, None] + np.arange(C)) % 4
    cst = np.asarray(STATS_CONSTANTS, f32)[k]
    return np.broadcast_to(cst[:, None], (B, hw, C)).copy(), cst


def stats_ref(x):
    x64 = x.astype(f64)
    return x64.mean(1), 1.0 / (x64.std(1, ddof=1) + 1e-9)


# ---- mit_se_* --------------------------------------------------------------------------------------------------------------------
def se_chunk_sums(x, chunk=256):
    """x [B, hw, C] -> (sums [B, nchunks, C], sums of |x|) in extended precision."""
    B, hw, C = x.shape
    n = (hw + chunk - 1) // chunk
    xl = x.astype(np.longdouble)
    s = np.stack([xl[:, k * chunk:min(hw, (k + 1) * chunk)].sum(1) for k in range(n)], 1)
    a = np.stack([np.abs(xl[:, k * chunk:min(hw, (k + 1) * chunk)]).sum(1) for k in range(n)], 1)
    return s, a


def se_weights(C, seed=0, dead=False):
    """conv1 [C/16, C], conv2 [C, C/16] and biases.  dead: b1 = -100 makes every hidden unit negative before the ReLU, and b2 cycles
    through EXACT_GATES and general values."""
    rng = np.random.default_rng(4000 + seed)
    Ch = C // 16
    w1 = (rng.standard_normal((Ch, C)) / C ** 0.5).astype(f32)
    b1 = (rng.standard_normal(Ch) * 0.1).astype(f32)
    w2 = (rng.standard_normal((C, Ch)) / Ch ** 0.5).astype(f32)
    b2 = (rng.standard_normal(C) * 0.1).astype(f32)
    if dead:
        b1[:] = -100.0
        b2 = (rng.standard_normal(C) * 2).astype(f32)
        b2[::2] = np.asarray(EXACT_GATES, f32)[np.arange(b2[::2].size) % 3]
    return w1, b1, w2, b2


# ---- mit_mc2_ffd_pack / unpack ---------------------------------------------------------------------------------------------------
FFD_SIDES = [(1, 1), (2, 2), (5, 7), (6, 9)]
SIGMA = float(f32(30 / 255))


def ffd_pages(H, W, Cin, seed=0):
    """B = 3 pages whose RGB max is 0, 1 and 2 (the /255 switch is per page); alpha = 255 when Cin == 4."""
    rng = np.random.default_rng(5000 + seed)
    img = np.stack([rng.integers(0, m + 1, (H, W, Cin), dtype=np.uint8) for m in (0, 1, 2)])
    for b, m in enumerate((0, 1, 2)):
        img[b, H - 1, W - 1, (b + H) % 3] = m
    if Cin == 4:
        img[..., 3] = 255
    return img


def ffd_all_bytes_page(Cin, H=16, W=48):
    """One page in which every byte value occurs in each of R, G, B (alpha, when there, counts 0..255 too, out of step)."""
    img = all_bytes_image(H * W).reshape(1, H, W, 3)
    if Cin == 4:
        a = ((np.arange(H * W) * 5 + 3) % 256).astype(np.uint8).reshape(1, H, W, 1)
        img = np.concatenate([img, a], -1)
    return img


def ffd_dim_rgba_page(H=5, W=7):
    """A Cin = 4 page whose RGB values are all <= 1 under alpha = 255: it must stay unnormalised."""
    img = ffd_pages(H, W, 4, seed=9)[1:2].copy()
    assert img[..., :3].max() == 1 and (img[..., 3] == 255).all()
    return img


def ffd_pmax(img):
    return img[..., :3].reshape(img.shape[0], -1).max(1).astype(np.uint32)


def ffd_value(rgb, pmax):
    """The page FFDNet sees (denoiser.py:86-87)."""
    v = np.float32(rgb / 255.) if pmax > 1.2 else rgb.astype(f32)
    assert v.dtype == f32
    return v


def ffd_pack_ref(img, sigma=SIGMA):
    """(pmax [B] u32, out [B, ceil(H/2), ceil(W/2), 16] f32)."""
    B, H, W, _ = img.shape
    pm = ffd_pmax(img)
    out = np.zeros((B, (H + 1) // 2, (W + 1) // 2, 16), f32)
    out[..., :3] = f32(sigma)
    for b in range(B):
        x = np.pad(ffd_value(img[b, ..., :3], pm[b]), ((0, H % 2), (0, W % 2), (0, 0)), mode="edge")   # denoiser.py:79-84
        for c in range(3):
            for i in range(2):
                for j in range(2):
                    out[b, ..., 3 + c * 4 + i * 2 + j] = x[i::2, j::2, c]                              # functions.py:16-56
    return pm, out


def ffd_unpack_ref(img, pmax, noise):
    """BGR u8 [B, H, W, 3] from noise [B, h2, w2, >= 12]; the plane output is its channel 0 (B)."""
    B, H, W, _ = img.shape
    h2, w2 = noise.shape[1:3]
    out = np.zeros((B, H, W, 3), np.uint8)
    for b in range(B):
        n = np.zeros((2 * h2, 2 * w2, 3), f32)
        for c in range(3):
            for i in range(2):
                for j in range(2):
                    n[i::2, j::2, c] = noise[b, :, :, c * 4 + i * 2 + j]                                # functions.py:58-83
        v = np.minimum(np.maximum(ffd_value(img[b, ..., :3], pmax[b]) - n[:H, :W], f32(0.0)), f32(1.0))  # denoiser.py:107-110
        out[b] = trunc_u8(v * f32(255.0))[..., ::-1]                                                    # utils.py:17-33
    return out


def ffd_noise(B, H, W, ps, elem_fn):
    """noise [B, h2, w2, ps] whose depth-to-space image at (b, y, x, c) is elem_fn(b, y, x, c); 1e30 in the surplus channels and
    in the slots of the repeated last row / column that the crop drops."""
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    noise = np.full((B, h2, w2, ps), 1e30, f32)
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    noise[b, y >> 1, x >> 1, c * 4 + (y & 1) * 2 + (x & 1)] = elem_fn(b, y, x, c)
    return noise


def ffd_unpack_byte(n, x=f32(1.0)):
    v = np.minimum(np.maximum(x - n, f32(0.0)), f32(1.0))
    return trunc_u8(v * f32(255.0))


_UNPACK_VALS = []


def ffd_unpack_noise_values():
    """For the page value 1.0 (byte 255 normalised, byte 1 unnormalised): for every k the adjacent fp32 noise pair where the byte
    turns k -> k - 1 (it falls as the noise rises), then what the clamp is for."""
    if not _UNPACK_VALS:
        a, b = bisect_f32(ffd_unpack_byte, -1.0, 2.0)
        _UNPACK_VALS.append(np.concatenate([a, b, np.array([0.0, -0.0, 1.0, 2.0, -1.0, 0.5, 1e30, -1e30], f32)]))
    return _UNPACK_VALS[0]


def ffd_unpack_boundary_case(Cin, ps, H=15, W=13):
    """B = 2: page 0 all 255 (normalised to 1.0), page 1 all 1 (max <= 1: unnormalised 1.0) but for a few 0 pixels; the elements of
    each page cycle through ffd_unpack_noise_values."""
    vals = ffd_unpack_noise_values()
    assert H * W * 3 >= vals.size
    img = np.zeros((2, H, W, Cin), np.uint8)
    img[0, ..., :3], img[1, ..., :3] = 255, 1
    img[1, ::4, ::3, :3] = 0
    if Cin == 4:
        img[..., 3] = 255
    noise = ffd_noise(2, H, W, ps, lambda b, y, x, c: vals[((y * W + x) * 3 + c) % vals.size])
    return img, noise


def ffd_unpack_unnormalised_case(Cin, ps, H=9, W=10):
    """x in {0, 1} (page max 1) with noise over [-1, 2]."""
    rng = np.random.default_rng(6000 + Cin + ps)
    img = rng.integers(0, 2, (2, H, W, Cin), dtype=np.uint8)
    img[:, 0, 0, :3] = 1
    if Cin == 4:
        img[..., 3] = 255
    rnd = rng.uniform(-1, 2, (2, H, W, 3)).astype(f32)
    return img, ffd_noise(2, H, W, ps, lambda b, y, x, c: rnd[b, y, x, c])


def ffd_unpack_position_case(Cin, ps, H=6, W=9):
    """Pages of 255 under a noise tensor that encodes its own slot: noise[b, y2, x2, ch] = (20 ch + 2 ((y2 w2 + x2 + b) % 10)) / 256,
    so two slots of one pixel differ by at least 2 / 256 and their bytes by at least 1."""
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    img = np.full((2, H, W, Cin), 255, np.uint8)
    noise = np.full((2, h2, w2, ps), 1e30, f32)
    b, y2, x2, ch = np.meshgrid(np.arange(2), np.arange(h2), np.arange(w2), np.arange(12), indexing="ij")
    noise[..., :12] = ((20 * ch + 2 * ((y2 * w2 + x2 + b) % 10)) / 256.0).astype(f32)
    return img, noise


# ---- mit_mc2_gen_in --------------------------------------------------------------------------------------------------------------
GEN_IN_SHAPES = [(1, 1, 1, 1), (3, 5, 8, 5), (3, 5, 3, 8), (32, 31, 32, 32)]


def gen_in_case(h, w, B=2):
    """Planes whose row and column maxima differ from page to page: page b's row y peaks at 200 + 3 y + b, its column x at least at
    100 + x + 7 b."""
    rng = np.random.default_rng(7000 + h * 100 + w)
    p = rng.integers(0, 100, (B, h, w), dtype=np.uint8)
    for b in range(B):
        for x in range(w):
            p[b, (x + b) % h, x] = min(255, 100 + x + 7 * b)
        for y in range(h):
            p[b, y, (2 * y + b) % w] = min(255, 200 + 3 * y + b)
    return p


def gen_in_ref(plane, Hp, Wp):
    B, h, w = plane.shape
    out = np.zeros((B, Hp, Wp, 4), f32)
    for b in range(B):
        out[b, ..., 0] = np.pad(plane[b], ((0, Hp - h), (0, Wp - w)), "maximum").astype(f32) / f32(255.0)   # utils.py:27-38, ToTensor
    return out


# ---- mit_mc2_post ----------------------------------------------------------------------------------------------------------------
POST_SPECIALS = (0.0, -0.0, 9.0, -9.0, 20.0, -20.0, 88.0, -88.0, np.inf, -np.inf)


def post_margin_inputs():
    """atanh(2 (k + d) / 255 - 1) for k = 0..254 and d = 1/4, 1/2, 3/4, as fp32; and the k each must yield."""
    k = np.arange(255)
    x = np.concatenate([np.arctanh(2.0 * (k + d) / 255.0 - 1.0) for d in (0.25, 0.5, 0.75)]).astype(f32)
    return x, np.tile(k, 3).astype(np.uint8)


def post_boundary_inputs():
    """atanh(2 k / 255 - 1), k = 1..254, with their fp32 neighbours: on a truncation boundary, where +-1 is all that can be asked."""
    return around(np.arctanh(2.0 * np.arange(1, 255) / 255.0 - 1.0).astype(f32))


def post_value64(x):
    return (np.tanh(np.asarray(x, f64)) * 0.5 + 0.5) * 255.0


def post_ref64(x):
    return np.floor(np.clip(post_value64(x), 0.0, 255.0)).astype(np.uint8)


def post_ref32(x):
    v = (np.tanh(np.asarray(x, f32)) * f32(0.5) + f32(0.5)) * f32(255.0)
    return trunc_u8(np.minimum(np.maximum(v, f32(0.0)), f32(255.0)))


def post_case(vals, B, Hp, Wp, h, w, ps):
    """pre [B, Hp, Wp, ps]: the cropped elements cycle through ``vals``; 0.3 outside the crop, 1e30 in a fourth channel."""
    pre = np.full((B, Hp, Wp, ps), 1e30, f32)
    pre[..., :3] = 0.3
    n = B * h * w * 3
    pre[:, :h, :w, :3] = vals[np.arange(n) % vals.size].reshape(B, h, w, 3)
    return pre
