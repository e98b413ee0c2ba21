"""What tests/test_mc2_precision.py (CPU) and tests/test_mc2_bf16_gpu.py share: the fixed inputs of the mc2 bf16 accuracy check and
the CPU oracles they are judged against, all built on tests/_mc2_oracle.py with seeded weights.

The yardstick is the one the LaMa, ESRGAN and AOT bf16 precisions merged against: the error against the float64 truth must not exceed
that of the oracle under ``torch.autocast("cpu", bfloat16)`` on the same input.  FFDNet and the generator are judged separately, each on
a fixed input (never through ``forward``: the denoiser's u8 plane differs by a level between the modes, and the generator would then
see another input).

Modes of the oracles: "f64" (the truth), "f32", "autocast", and "emul" — float64 in which every dense convolution with
K = Cin kh kw >= 64 and N >= 16 rounds its two operands to bf16 and nothing else is rounded: what the engine's bf16 precision does,
without its fp32 accumulation error."""
import contextlib
import types

import numpy as np
import torch
import torch.nn.functional as F

import _mc2_oracle as O

SIGMA = 30
FFD_PAGE_HW = (37, 51)         # odd sides: FFDNet's edge padding to even is exercised
FFD_SEEDS = (41, 42)
GEN_CASES = tuple((tag, H, W, seed) for tag, H, W, seed in O.NET_CASES)     # (64, 48) and (96, 64)
MODES = ("f64", "f32", "autocast", "emul")


def ffd_pages() -> np.ndarray:
    """u8 RGB [2, 37, 51, 3]."""
    return np.stack([O.synth_color_page(s, *FFD_PAGE_HW) for s in FFD_SEEDS])


def gen_planes(tag: str) -> np.ndarray:
    """u8 [2, H, W]: the planes the generator sees before its padding."""
    _, H, W, seed = next(c for c in GEN_CASES if c[0] == tag)
    rng = np.random.default_rng(seed + 100)
    return np.stack([O.synth_color_page(seed + 7 * b, H, W)[..., 0] if b == 0 else rng.integers(0, 256, (H, W), dtype=np.uint8) for b in range(2)])


def _round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _emul_conv2d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
    dense = groups == 1 and tuple(x.shape[-2:]) != (1, 1)      # (a 1 x 1 input: the two 1x1s of a squeeze-and-excitation, kept fp32)
    if dense and w.shape[1] * w.shape[2] * w.shape[3] >= 64 and w.shape[0] >= 16:
        x, w = _round(x), _round(w)
    return F.conv2d(x, w, bias, stride, padding, dilation, groups)


@contextlib.contextmanager
def _mode(mode):
    """Inside: the oracle's functions run in ``mode``; yields the dtype its tensors take."""
    if mode == "autocast":
        with torch.autocast("cpu", dtype=torch.bfloat16):
            yield torch.float32
    elif mode == "emul":
        proxy = types.SimpleNamespace(**{k: getattr(F, k) for k in ("relu", "leaky_relu", "batch_norm", "pixel_shuffle")}, conv2d=_emul_conv2d)
        real, O.F = O.F, proxy
        try:
            yield torch.float64
        finally:
            O.F = real
    else:
        yield torch.float64 if mode == "f64" else torch.float32


def _cast(sd, dtype):
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


@torch.no_grad()
def ffd_oracle(fsd, page: np.ndarray, mode: str):
    """One u8 page [H,W,3] -> dict(noise = FFDNet's estimate [h2,w2,12] float64 in the engine's layout (channel c * 4 + i * 2 + j),
    den_f = the float BGR page before the truncation, 0 .. 255 scale, bgr = its u8)."""
    img = page[..., :3].transpose(2, 0, 1)
    x = np.float32(img / 255.)
    h, w = x.shape[1:]
    x = np.pad(x, ((0, 0), (0, h % 2), (0, w % 2)), mode="edge")
    with _mode(mode) as dtype:
        t = torch.from_numpy(x)[None].to(dtype)
        n = O.ffdnet(_cast(fsd, dtype), t, float(np.float32(SIGMA / 255))).to(dtype if mode != "autocast" else torch.float32)
    out = torch.clamp(t - n, 0., 1.)[0, :, :h, :w].double().numpy().transpose(1, 2, 0)[..., ::-1] * 255.
    n = n.double()[0]
    packed = torch.stack([n[c, i::2, j::2] for c in range(3) for (i, j) in ((0, 0), (0, 1), (1, 0), (1, 1))], -1)
    return dict(noise=packed, den_f=out, bgr=np.clip(out, 0, 255).astype(np.uint8))


@torch.no_grad()
def gen_oracle(gsd, planes: np.ndarray, mode: str):
    """u8 planes [B,h,w] -> dict(pre = the generator before the tanh on the padded input [B,Hp,Wp,3] float64, out = the u8 RGB images
    [B,h,w,3]): resize_pad's 'maximum' padding of the long side, ToTensor, Generator and the output glue of _infer."""
    B, h, w = planes.shape
    pad = ((0, 32 - h % 32), (0, 0)) if h >= w else ((0, 0), (0, 32 - w % 32))
    x = np.stack([np.pad(p, pad, "maximum") for p in planes]).astype(np.float32) / np.float32(255)
    with _mode(mode) as dtype:
        t = torch.from_numpy(x)[:, None].to(dtype)
        t = torch.cat([t, torch.zeros(B, 4, *t.shape[2:], dtype=dtype)], 1)
        taps = {}
        y = O.generator(_cast(gsd, dtype), t, taps)
    img = (y.double().permute(0, 2, 3, 1) * 0.5 + 0.5)[:, :h, :w].numpy() * 255
    return dict(pre=taps["pre"].double().permute(0, 2, 3, 1), out=img.astype(np.uint8))


def errors(got, truth):
    """(mean, max) absolute error."""
    e = (torch.as_tensor(got).double() - torch.as_tensor(truth).double()).abs()
    return float(e.mean()), float(e.max())
