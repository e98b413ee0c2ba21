"""Float32 / float64 CPU oracle of the mc2 colorizer (the reference's ``Colorizer.mc2``), restated from its description:
``MangaColorizationV2._infer`` (manga_translator/colorization/manga_colorization_v2.py:42-74) with FFDNet (denoising/) and
``Generator`` (networks/models.py, networks/extractor.py).  Plain ``F.conv2d(groups=, dilation=)``; no reference code.  The u8 glue
is built on ``oracle.lama.resize_area_u8`` per channel.  ``make_fixtures()`` writes tests/golden/mc2.npz and mc2_infer.npz from the
reference modules themselves (only where the reference tree is present)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from manga_image_translator_amd import mc2_schema as S, synth  # noqa: E402
from oracle import lama as OL  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# (tag, H, W, seed) of the network fixture (mc2.npz): generator input size and FFDNet input size
NET_CASES = (("a", 64, 48, 21), ("b", 96, 64, 22))
# (tag, (H, W), colorization_size, denoise_sigma, seed, dim) of the _infer fixture (mc2_infer.npz)
INFER_CASES = (("portrait", (300, 212), 192, 30, 31, False), ("landscape", (150, 230), 128, 30, 32, False),
               ("cap", (1232, 96), 64, 25, 33, False), ("nodenoise", (260, 200), 576, -1, 34, False),
               ("dim", (200, 160), 128, 30, 35, True))


def weights(seed: int = 0):
    return synth.synth_state_dict(S.generator_schema(), seed=seed), synth.synth_state_dict(S.ffdnet_schema(), seed=seed + 1)


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def _leaky(x):
    return F.leaky_relu(x, 0.2)


def _se(sd, p, x):
    m = x.mean((2, 3), keepdim=True)
    h = F.relu(F.conv2d(m, sd[p + ".conv1.weight"], sd[p + ".conv1.bias"]))
    return x * torch.sigmoid(F.conv2d(h, sd[p + ".conv2.weight"], sd[p + ".conv2.bias"]))


# ---- FFDNet ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def ffdnet(sd, x, sigma):
    """x [B,3,H,W] (H, W even), sigma (float) -> noise estimate [B,3,H,W]."""
    B, C, H, W = x.shape
    idx = ((0, 0), (0, 1), (1, 0), (1, 1))
    down = torch.zeros(B, 12, H // 2, W // 2, dtype=x.dtype)
    for k, (i, j) in enumerate(idx):
        down[:, k::4] = x[:, :, i::2, j::2]
    h = torch.cat([torch.full((B, 3, H // 2, W // 2), sigma, dtype=x.dtype), down], 1)
    p = "intermediate_dncnn.itermediate_dncnn"
    h = F.relu(F.conv2d(h, sd[f"{p}.0.weight"], padding=1))
    for k in range(S.FFD_LAYERS - 2):
        h = F.relu(_bn(sd, f"{p}.{3 + 3 * k}", F.conv2d(h, sd[f"{p}.{2 + 3 * k}.weight"], padding=1)))
    h = F.conv2d(h, sd[f"{p}.{2 + 3 * (S.FFD_LAYERS - 2)}.weight"], padding=1)
    out = torch.zeros(B, 3, H, W, dtype=x.dtype)
    for k, (i, j) in enumerate(idx):
        out[:, :, i::2, j::2] = h[:, k::4]
    return out


# ---- Generator ---------------------------------------------------------------------------------------------------------------
def _enc_block(sd, p, x, stride, first):
    out = F.relu(_bn(sd, p + ".bn1", F.conv2d(x, sd[p + ".conv1.weight"])))
    out = F.relu(_bn(sd, p + ".bn2", F.conv2d(out, sd[p + ".conv2.weight"], stride=stride, padding=1, groups=S.CARDINALITY)))
    out = _se(sd, p + ".selayer", _bn(sd, p + ".bn3", F.conv2d(out, sd[p + ".conv3.weight"])))
    res = _bn(sd, p + ".downsample.1", F.conv2d(x, sd[p + ".downsample.0.weight"], stride=stride)) if first else x
    return F.relu(out + res)


def _tunnel_block(sd, p, x, d, card):
    b = _leaky(F.conv2d(x, sd[p + ".conv_reduce.weight"]))
    b = _leaky(F.conv2d(b, sd[p + ".conv_conv.weight"], padding=d, dilation=d, groups=card))
    b = _se(sd, p + ".selayer", F.conv2d(b, sd[p + ".conv_expand.weight"]))
    return x + b


def _tunnel(sd, name, x, taps):
    _, _, width, dils, card = next(t for t in S.TUNNELS if t[0] == name)
    x = _leaky(F.conv2d(x, sd[name + ".0.weight"], sd[name + ".0.bias"], padding=1))
    for i, d in enumerate(dils):
        x = _tunnel_block(sd, f"{name}.2.{i}", x, d, card)
    x = _leaky(F.pixel_shuffle(F.conv2d(x, sd[name + ".3.weight"], sd[name + ".3.bias"], padding=1), 2))
    if taps is not None:
        taps[name] = x.clone()
    return x


def _aux(sd, name, x, stride):
    x = _leaky(F.conv2d(x, sd[name + ".0.weight"], sd[name + ".0.bias"], stride=stride, padding=1))
    return _leaky(F.conv2d(x, sd[name + ".2.weight"], sd[name + ".2.bias"], padding=1))


@torch.no_grad()
def generator(sd, x, taps=None):
    """Generator.forward on [B,5,H,W] -> tanh output [B,3,H,W].  ``taps``: x1..x4, tunnel4 / 3 / 2 and 'pre' (before the tanh)."""
    x0 = _aux(sd, "to0", x, 1)
    a = _aux(sd, "to3", _aux(sd, "to2", _aux(sd, "to1", x0, 2), 2), 2)
    e = F.relu(_bn(sd, "encoder.bn1", F.conv2d(x[:, 0:1], sd["encoder.conv1.weight"], stride=2, padding=3)))
    feats = [e]
    for layer, _planes, blocks, stride in S.ENCODER:
        for i in range(blocks):
            e = _enc_block(sd, f"encoder.layer{layer}.{i}", e, stride if i == 0 else 1, i == 0)
        feats.append(e)
    x1, x2, x3, x4 = feats
    if taps is not None:
        taps.update(x1=x1.clone(), x2=x2.clone(), x3=x3.clone(), x4=x4.clone())
    out = _tunnel(sd, "tunnel4", torch.cat([x4, a], 1), taps)
    y = _tunnel(sd, "tunnel3", torch.cat([out, x3], 1), taps)
    y = _tunnel(sd, "tunnel2", torch.cat([y, x2, x1], 1), taps)
    y = _leaky(F.conv2d(torch.cat([y, x0], 1), sd["exit.0.weight"], sd["exit.0.bias"], padding=1))
    y = F.conv2d(y, sd["exit.2.weight"], sd["exit.2.bias"])
    if taps is not None:
        taps["pre"] = y.clone()
    return torch.tanh(y)


# ---- the _infer glue ---------------------------------------------------------------------------------------------------------
def resize_area(img: np.ndarray, dsize):
    """cv2.resize(img, dsize, INTER_AREA) for u8 [H,W] or [H,W,C], channel by channel through oracle.lama.resize_area_u8."""
    if img.ndim == 2:
        return OL.resize_area_u8(img, dsize)
    return np.stack([OL.resize_area_u8(np.ascontiguousarray(img[..., c]), dsize) for c in range(img.shape[2])], -1)


def colorization_size(h: int, w: int, size: int) -> int:
    m = min(h, w)
    m -= m % 32
    return min(m, size - size % 32) if size > 0 else min(m, 576)


def denoise_input(page: np.ndarray):
    """The page FFDNet sees (denoiser.py:66-77) as u8: alpha dropped, INTER_AREA below a long side of 1200."""
    img = page[..., :3]
    if max(img.shape[:2]) > 1200:
        r = max(img.shape[:2]) / 1200
        img = resize_area(img, (int(img.shape[1] / r), int(img.shape[0] / r)))
    return img


@torch.no_grad()
def denoise(fsd, page: np.ndarray, sigma: float, dtype=torch.float32):
    """get_denoised_image (denoiser.py:51-118): returns (BGR u8 [h,w,3], the float before the truncation [h,w,3] BGR)."""
    img = denoise_input(page).transpose(2, 0, 1)
    x = np.float32(img / 255.) if img.max() > 1.2 else img.astype(np.float32)
    h, w = x.shape[1:]
    x = np.pad(x, ((0, 0), (0, h % 2), (0, w % 2)), mode="edge")
    t = torch.from_numpy(x)[None]
    sd = fsd
    if dtype != torch.float32:
        sd, t = {k: v.to(dtype) if v.is_floating_point() else v for k, v in fsd.items()}, t.to(dtype)
    noise = ffdnet(sd, t, float(np.float32(sigma / 255)))
    out = torch.clamp(t - noise, 0., 1.)[0, :, :h, :w].numpy().transpose(1, 2, 0)[..., ::-1]
    f = out * 255.
    return np.clip(f, 0, 255).astype(np.uint8), f


def resize_pad(img: np.ndarray, size: int):
    """utils/utils.py:resize_pad on u8 pages: INTER_AREA, pad the long side with np.pad 'maximum', keep channel 0."""
    if img.shape[2] == 4:
        img = img[..., :3]
    if img.shape[0] < img.shape[1]:
        ratio = img.shape[0] / (size * 1.5)
        width = int(np.ceil(img.shape[1] / ratio))
        img = resize_area(img, (width, int(size * 1.5)))
        pad = (0, width + (32 - width % 32) - width)
        img = np.pad(img, ((0, 0), (0, pad[1]), (0, 0)), "maximum")
    else:
        ratio = img.shape[1] / size
        height = int(np.ceil(img.shape[0] / ratio))
        img = resize_area(img, (size, height))
        pad = (height + (32 - height % 32) - height, 0)
        img = np.pad(img, ((0, pad[0]), (0, 0), (0, 0)), "maximum")
    return img[:, :, :1], pad


@torch.no_grad()
def infer(gsd, fsd, page: np.ndarray, size: int, sigma: float = 25, dtype=torch.float32, taps=None):
    """_infer (:42-74) on a u8 RGB(A) page -> dict(out = u8 RGB, out_f = the float before the truncation, plane = the u8 plane the
    generator sees before padding, den_f = FFDNet's float BGR before its truncation or None)."""
    sz = colorization_size(page.shape[0], page.shape[1], size)
    img, den_f = page, None
    if 0 <= sigma <= 255:
        img, den_f = denoise(fsd, page, sigma, dtype)
    plane, pad = resize_pad(img, sz)
    x = torch.from_numpy(plane[..., 0].astype(np.float32) / np.float32(255))[None, None]
    x = torch.cat([x, torch.zeros(1, 4, *x.shape[2:])], 1)
    sd = gsd
    if dtype != torch.float32:
        sd, x = {k: v.to(dtype) if v.is_floating_point() else v for k, v in gsd.items()}, x.to(dtype)
    y = generator(sd, x, taps)[0].permute(1, 2, 0) * 0.5 + 0.5
    if pad[0]:
        y = y[:-pad[0]]
    if pad[1]:
        y = y[:, :-pad[1]]
    f = y.numpy() * 255
    h, w = f.shape[:2]
    return dict(out=f.astype(np.uint8), out_f=f, plane=plane[:h, :w, 0] if pad[0] else plane[:, :w, 0], den_f=den_f)


def page_for(tag: str) -> np.ndarray:
    """The page of INFER_CASES entry ``tag`` (RGBA for the portrait case, as PIL hands an RGBA page to _infer)."""
    _, (H, W), _, _, seed, dim = next(c for c in INFER_CASES if c[0] == tag)
    return synth_color_page(seed, H, W, dim=dim, rgba=(tag == "portrait"))


def synth_color_page(seed: int, H: int, W: int, dim: bool = False, rgba: bool = False) -> np.ndarray:
    """A manga-like page (synth.synth_page) with coloured panels, so the three channels of the denoised page differ."""
    page, _, _ = synth.synth_page(seed, H, W, n_boxes=2)
    rng = np.random.default_rng(seed)
    page = page.astype(np.int32)
    for _ in range(3):
        y0, x0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
        page[y0:y0 + H // 3, x0:x0 + W // 3] -= rng.integers(0, 60, size=3)
    page = np.clip(page, 0, 255).astype(np.uint8)
    if dim:
        page = (page > 128).astype(np.uint8)   # a page of 0 / 1 bytes: FFDNet's max <= 1.2 rule skips the /255
    if rgba:
        page = np.concatenate([page, np.full(page.shape[:2] + (1,), 255, np.uint8)], -1)
    return page


# ---- fixtures from the reference's own modules ------------------------------------------------------------------------------
def ref_modules():
    from oracle import ref_import as R

    R._prepare()
    for p in ["manga_translator.colorization", "manga_translator.colorization.manga_colorization_v2_utils",
              "manga_translator.colorization.manga_colorization_v2_utils.networks",
              "manga_translator.colorization.manga_colorization_v2_utils.denoising",
              "manga_translator.colorization.manga_colorization_v2_utils.utils"]:
        R._pkg(p)
    base = "colorization/manga_colorization_v2_utils/"
    dotted = "manga_translator.colorization.manga_colorization_v2_utils."
    ext = R._load(dotted + "networks.extractor", base + "networks/extractor.py")
    mod = R._load(dotted + "networks.models", base + "networks/models.py")
    fun = R._load(dotted + "denoising.functions", base + "denoising/functions.py")
    dmod = R._load(dotted + "denoising.models", base + "denoising/models.py")
    dut = R._load(dotted + "denoising.utils", base + "denoising/utils.py")
    den = R._load(dotted + "denoising.denoiser", base + "denoising/denoiser.py")
    ut = R._load(dotted + "utils.utils", base + "utils/utils.py")
    return dict(extractor=ext, models=mod, functions=fun, dmodels=dmod, dutils=dut, denoiser=den, utils=ut)


class _Cv2:
    """The three OpenCV calls on the colorizer's path, restated (parity with the real library is unpinned)."""
    INTER_AREA, COLOR_RGB2BGR = 3, 4

    @staticmethod
    def resize(src, dsize, interpolation=3):
        assert interpolation == 3
        return resize_area(src, dsize)

    @staticmethod
    def cvtColor(src, code):
        assert code == 4
        return np.ascontiguousarray(src[..., ::-1])


def _to_tensor(img):
    """torchvision.transforms.ToTensor on a u8 [H,W,C] array."""
    return torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float().div(255)


def ref_generator(gsd, M=None):
    M = M or ref_modules()
    g = M["models"].Generator()
    g.load_state_dict(gsd, strict=True)
    return g.eval()


def ref_ffdnet(fsd, M=None):
    M = M or ref_modules()
    m = M["dmodels"].FFDNet(num_input_channels=3)
    m.load_state_dict(fsd, strict=True)
    return m.eval()


def net_fixture(gsd=None, fsd=None):
    M = ref_modules()
    if gsd is None:
        gsd, fsd = weights()
    g, f = ref_generator(gsd, M), ref_ffdnet(fsd, M)
    out = {}
    for tag, H, W, seed in NET_CASES:
        rng = np.random.default_rng(seed)
        sk = torch.from_numpy(rng.random((1, 1, H, W), dtype=np.float32))
        with torch.no_grad():
            y, _ = g(torch.cat([sk, torch.zeros(1, 4, H, W)], 1))
            xin = torch.from_numpy(rng.random((1, 3, H, W), dtype=np.float32))
            n = f(xin, torch.FloatTensor([np.float32(30 / 255)]))
        out.update({f"sketch_{tag}": sk.numpy(), f"gen_{tag}": y.numpy(), f"ffd_in_{tag}": xin.numpy(), f"ffd_{tag}": n.numpy()})
    return out


def infer_fixture(gsd=None, fsd=None):
    import asyncio
    from unittest import mock

    from oracle import ref_import as R
    from PIL import Image

    M = ref_modules()
    if gsd is None:
        gsd, fsd = weights()
    M["denoiser"].cv2 = M["dutils"].cv2 = M["utils"].cv2 = _Cv2
    R._pkg("manga_translator.colorization")
    common = type(sys)("manga_translator.colorization.common")
    common.OfflineColorizer = type("OfflineColorizer", (), {"_MODEL_SUB_DIR": "colorization"})
    sys.modules["manga_translator.colorization.common"] = common
    tv = type(sys)("torchvision.transforms")
    tv.ToTensor = lambda: _to_tensor
    sys.modules["torchvision.transforms"] = tv
    mc2 = R._load("manga_translator.colorization.manga_colorization_v2", "colorization/manga_colorization_v2.py")
    plug = mc2.MangaColorizationV2.__new__(mc2.MangaColorizationV2)
    plug.device, plug.logger = "cpu", mock.MagicMock()
    plug.colorizer = M["models"].Colorizer().eval()
    plug.colorizer.generator.load_state_dict(gsd, strict=True)
    den = M["denoiser"].FFDNetDenoiser.__new__(M["denoiser"].FFDNetDenoiser)
    den.sigma, den.channels, den.device, den.model = 25 / 255, 3, "cpu", ref_ffdnet(fsd, M)
    plug.denoiser = den
    out = {}
    for tag, (H, W), size, sigma, seed, dim in INFER_CASES:
        page = page_for(tag)
        res = asyncio.new_event_loop().run_until_complete(plug._infer(Image.fromarray(page), size, denoise_sigma=sigma))
        out.update({f"page_{tag}": page, f"size_{tag}": size, f"sigma_{tag}": sigma, f"out_{tag}": np.asarray(res).astype(np.uint8)})
    return out


def make_fixtures():
    np.savez_compressed(os.path.join(GOLDEN, "mc2.npz"), source="colorization/manga_colorization_v2_utils (Generator, FFDNet)", **net_fixture())
    np.savez_compressed(os.path.join(GOLDEN, "mc2_infer.npz"), source="colorization/manga_colorization_v2.py:42-74 (_infer)", **infer_fixture())


if __name__ == "__main__":
    make_fixtures()
