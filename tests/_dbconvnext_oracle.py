"""Float32 CPU oracle of the ``dbconvnext`` detector network (DBNet on ConvNeXt), restated from its description:
``DBNetConvNext.forward`` (manga_translator/detection/dbnet_convnext.py:474-491), ``ConvNeXtBlock`` (:112-127), ``ConvNeXtStage`` (:190-193),
``UpconvSkip`` (:377-380), ``DBHead`` (:400-408) and the tensor part of ``det_batch_forward_default`` (:499-509).  Plain ``F.conv2d`` /
``F.layer_norm`` / ``F.gelu`` / ``F.conv_transpose2d``; no reference code.

``make_fixtures()`` writes tests/golden/dbconvnext.npz from the reference module itself (only where the reference tree is present).
timm is not installed, so the module is imported over a small ``timm.layers`` stand-in restated from timm's documented behaviour
(below): what the fixture pins is the reference's own Python round those primitives and its state-dict names (``load_state_dict`` is
strict), not timm itself — the arrangement of the restated ResNet-34 behind the ``default`` detector.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from manga_image_translator_amd import dbconvnext_schema as S, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "dbconvnext.npz")
SEED, GAIN = 0, 1.0
# (tag, H, W, page seed): the two orientations of the smallest page with more than one h128 pixel
CASES = (("a", 128, 256, 41), ("b", 256, 128, 42))
TAPS = ("h4", "h32", "h128", "up8", "up4")
EPS = 1e-6


def weights(seed: int = SEED, gain: float = GAIN):
    return synth.synth_state_dict(S.dbnet_convnext_schema(), seed=seed, gain=gain)


def page(tag: str) -> np.ndarray:
    _, H, W, seed = next(c for c in CASES if c[0] == tag)
    return synth.synth_page(seed, H, W, n_boxes=4)[0]


# ---- the restated forward (NCHW) -----------------------------------------------------------------------------------------------------
def ln2d(sd, p, x):
    """LayerNorm over the channels of NCHW, eps 1e-6."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), sd[p + ".weight"], sd[p + ".bias"], EPS).permute(0, 3, 1, 2)


def block(sd, p, x):
    """7x7 convolution (depthwise when its weight has one input channel, else dense), LayerNorm over the channels, fc1, GELU, fc2, layer
    scale, plus the input — through a 1x1 convolution when the block changes the channel count."""
    w = sd[p + ".conv_dw.weight"]
    y = F.conv2d(x, w, sd[p + ".conv_dw.bias"], padding=3, groups=x.shape[1] if w.shape[1] == 1 and x.shape[1] > 1 else 1)
    y = y.permute(0, 2, 3, 1)
    y = F.layer_norm(y, (y.shape[-1],), sd[p + ".norm.weight"], sd[p + ".norm.bias"], EPS)
    y = F.linear(F.gelu(F.linear(y, sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"])), sd[p + ".mlp.fc2.weight"], sd[p + ".mlp.fc2.bias"])
    y = y.permute(0, 3, 1, 2) * sd[p + ".gamma"].reshape(1, -1, 1, 1)
    if (p + ".shortcut.conv.weight") in sd:
        x = F.conv2d(x, sd[p + ".shortcut.conv.weight"], sd.get(p + ".shortcut.conv.bias"))
    return y + x


def stage(sd, p, x, depth):
    if (p + ".downsample.1.weight") in sd:
        x = F.conv2d(ln2d(sd, p + ".downsample.0", x), sd[p + ".downsample.1.weight"], sd[p + ".downsample.1.bias"], stride=2)
    for j in range(depth):
        x = block(sd, f"{p}.blocks.{j}", x)
    return x


def upconv(sd, p, x):
    return F.conv_transpose2d(block(sd, p + ".conv", x), sd[p + ".upconv.weight"], sd[p + ".upconv.bias"], stride=2)


def head(sd, p, x):
    x = F.silu(F.conv2d(x, sd[p + ".0.weight"], sd.get(p + ".0.bias"), padding=1))
    x = F.silu(F.conv_transpose2d(x, sd[p + ".2.weight"], sd.get(p + ".2.bias"), stride=2, padding=1))
    return F.conv_transpose2d(x, sd[p + ".4.weight"], sd.get(p + ".4.bias"), stride=2, padding=1)


@torch.no_grad()
def network(sd, x, taps=None):
    """x [B,3,H,W] in [-1, 1] -> (db [B,2,H,W]: logits and the threshold map after its sigmoid, mask [B,1,H/2,W/2])."""
    x = ln2d(sd, "backbone.stem.1", F.conv2d(x, sd["backbone.stem.0.weight"], sd["backbone.stem.0.bias"], stride=4))
    hs = []
    for i, depth in enumerate(S.DEPTHS):
        x = stage(sd, f"backbone.stages.{i}", x, depth)
        hs.append(x)
    h4, h8, h16, h32 = hs
    h64 = stage(sd, "down_conv1", h32, 2)
    h128 = stage(sd, "down_conv2", h64, 2)
    up = upconv(sd, "upconv1", h128)
    for name, skip in (("upconv2", h64), ("upconv3", h32), ("upconv4", h16), ("upconv5", h8)):
        up = upconv(sd, name, torch.cat([up, skip], 1))
    up8 = up
    up4 = upconv(sd, "upconv6", torch.cat([up8, h4], 1))
    db = torch.cat([head(sd, "conv_db.binarize", up8), torch.sigmoid(head(sd, "conv_db.thresh", up8))], 1)
    m = F.silu(F.conv2d(up4, sd["conv_mask.0.weight"], sd["conv_mask.0.bias"], padding=1))
    m = F.silu(F.conv2d(m, sd["conv_mask.2.weight"], sd["conv_mask.2.bias"], padding=1))
    m = torch.sigmoid(F.conv2d(m, sd["conv_mask.4.weight"], sd["conv_mask.4.bias"]))
    if taps is not None:
        taps.update(h4=h4, h32=h32, h128=h128, up8=up8, up4=up4)
    return db, m


def prep(pages_u8: np.ndarray, dtype=torch.float32) -> torch.Tensor:
    """u8 [B,H,W,3] -> the model input of det_batch_forward_default (:503): x / 127.5 - 1 in float32, NCHW."""
    x = torch.from_numpy(pages_u8.astype(np.float32) / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()
    return x.to(dtype)


@torch.no_grad()
def det_batch_forward(sd, pages_u8: np.ndarray, taps=None, dtype=torch.float32):
    """det_batch_forward_default (:499-509): -> (db [B,2,H,W] after ``db.sigmoid()``, mask [B,1,H/2,W/2]) as float32 numpy.
    ``dtype=torch.float64`` runs the network in double precision on the float32 inputs and weights.  ``taps`` come back NHWC."""
    if dtype != torch.float32:
        sd = {k: v.to(dtype) for k, v in sd.items()}
    t = {} if taps is not None else None
    db, m = network(sd, prep(pages_u8, dtype), t)
    if taps is not None:
        taps.update({k: v.permute(0, 2, 3, 1).to(torch.float32).numpy() for k, v in t.items()})
    return torch.sigmoid(db).to(torch.float32).numpy(), m.to(torch.float32).numpy()


def sub_tap(name: str, t: np.ndarray) -> np.ndarray:
    """The part of an NHWC tap the fixture keeps: every pixel of the small ones, every fourth pixel and channel of up8 / up4 / h4."""
    return t if name in ("h32", "h128") else t[:, ::4, ::4, ::4]


# ---- the timm.layers stand-in: what the reference file imports from timm (:17-18), restated from timm's documented behaviour --------
def timm_layers_standin() -> types.ModuleType:
    m = types.ModuleType("timm.layers")

    class LayerNorm(nn.LayerNorm):
        """LayerNorm over the last dimension, eps 1e-6."""

        def __init__(self, num_channels, eps=1e-6, affine=True):
            super().__init__(num_channels, eps=eps, elementwise_affine=affine)

    class LayerNorm2d(nn.LayerNorm):
        """LayerNorm over the channels of an NCHW tensor, eps 1e-6."""

        def __init__(self, num_channels, eps=1e-6, affine=True):
            super().__init__(num_channels, eps=eps, elementwise_affine=affine)

        def forward(self, x):
            return F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)

    class Mlp(nn.Module):
        """fc1 -> act -> fc2 (Linear layers unless use_conv)."""

        def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, use_conv=False, **_):
            super().__init__()
            lin = (lambda i, o: nn.Conv2d(i, o, 1)) if use_conv else nn.Linear
            self.fc1 = lin(in_features, hidden_features or in_features)
            self.act = act_layer()
            self.fc2 = lin(hidden_features or in_features, out_features or in_features)

        def forward(self, x):
            return self.fc2(self.act(self.fc1(x)))

    def create_conv2d(in_channels, out_channels, kernel_size, **kwargs):
        """nn.Conv2d with symmetric padding ((stride - 1) + dilation * (k - 1)) // 2 unless one is given; groups = in_channels when
        depthwise."""
        depthwise = kwargs.pop("depthwise", False)
        groups = in_channels if depthwise else kwargs.pop("groups", 1)
        padding = kwargs.pop("padding", "")
        if isinstance(padding, str):
            padding = ((kwargs.get("stride", 1) - 1) + kwargs.get("dilation", 1) * (kernel_size - 1)) // 2
        return nn.Conv2d(in_channels, out_channels, kernel_size, padding=padding, groups=groups, **kwargs)

    def get_act_layer(name):
        return {"gelu": nn.GELU, "silu": nn.SiLU, "relu": nn.ReLU}[name] if isinstance(name, str) else name

    def to_ntuple(n):
        return lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x,) * n

    class _Unused(nn.Module):
        def __init__(self, *a, **k):
            raise NotImplementedError("not on DBNetConvNext's path")

    m.LayerNorm, m.LayerNorm2d, m.Mlp, m.create_conv2d, m.get_act_layer, m.to_ntuple = LayerNorm, LayerNorm2d, Mlp, create_conv2d, get_act_layer, to_ntuple
    m.trunc_normal_ = nn.init.trunc_normal_
    m.AvgPool2dSame = m.DropPath = m.GlobalResponseNormMlp = _Unused
    m.make_divisible = lambda v, *a, **k: v
    return m


def ref_module():
    """The reference's own dbnet_convnext.py, imported over the stand-in."""
    from unittest import mock

    from oracle import ref_import as R

    R._prepare()
    saved = {k: sys.modules.get(k) for k in ("timm", "timm.layers")}
    pk = types.ModuleType("timm")
    pk.__path__ = []
    pk.layers = timm_layers_standin()
    sys.modules["timm"], sys.modules["timm.layers"] = pk, pk.layers
    if "einops" not in sys.modules:
        try:
            import einops  # noqa: F401
        except Exception:
            sys.modules["einops"] = mock.MagicMock()
    du = R._pkg("manga_translator.detection.default_utils")
    for n in ("imgproc", "dbnet_utils", "craft_utils"):   # imported by the plugin half of the file; the network does not touch them
        if not hasattr(du, n):
            setattr(du, n, mock.MagicMock())
    try:
        return R._load("manga_translator.detection.dbnet_convnext", "detection/dbnet_convnext.py")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def ref_model(sd):
    m = ref_module().DBNetConvNext()
    m.load_state_dict(sd, strict=True)
    return m.eval()


@torch.no_grad()
def fixture(sd=None, stats: bool = True):
    """What tests/golden/dbconvnext.npz holds: per case the page, the reference's post-sigmoid ``db`` (every second pixel) and ``mask``, a few
    subsampled taps; the state-dict names and shapes; with ``stats`` the measured conditions of ``check_conditions``."""
    sd = weights() if sd is None else sd
    want_stats = stats
    m = ref_model(sd)
    out = {"seed": np.int64(SEED), "gain": np.float64(GAIN),
           "names": np.asarray([k for k in m.state_dict()]), "shapes": np.asarray([",".join(map(str, v.shape)) for v in m.state_dict().values()])}
    feats = {}
    hooks = [m.backbone.stages[0].register_forward_hook(lambda _m, _i, o: feats.__setitem__("h4", o)),
             m.backbone.stages[3].register_forward_hook(lambda _m, _i, o: feats.__setitem__("h32", o)),
             m.down_conv2.register_forward_hook(lambda _m, _i, o: feats.__setitem__("h128", o)),
             m.upconv5.register_forward_hook(lambda _m, _i, o: feats.__setitem__("up8", o)),
             m.upconv6.register_forward_hook(lambda _m, _i, o: feats.__setitem__("up4", o))]
    stats = {}
    for tag, *_ in CASES:
        pg = page(tag)
        db, mask = m(prep(pg[None]))
        db = db.sigmoid().numpy()   # det_batch_forward_default (:507)
        out.update({f"page_{tag}": pg, f"db_{tag}": db[:, :, ::2, ::2].copy(), f"mask_{tag}": mask.numpy()})
        for k in TAPS:
            out[f"{k}_{tag}"] = sub_tap(k, feats[k].permute(0, 2, 3, 1).numpy()).copy()
            stats[f"std_{k}_{tag}"] = float(feats[k].std())
        stats[f"std_db0_{tag}"], stats[f"std_mask_{tag}"] = float(db[:, 0].std()), float(mask.std())
        if not want_stats:
            continue
        # the conditions on the seeded weights, measured on the CPU when the fixture is made
        d32, m32 = det_batch_forward(sd, pg[None])
        d64, m64 = det_batch_forward(sd, pg[None], dtype=torch.float64)
        stats[f"f32_vs_f64_{tag}"] = float(max(np.abs(d32 - d64).max(), np.abs(m32 - m64).max()))
        stats[f"margin_share_{tag}"] = float((np.abs(d64[:, 0] - 0.5) < 2e-4).mean())
    for h in hooks:
        h.remove()
    if want_stats:
        out.update({k: np.float64(v) for k, v in stats.items()})
    return out


def check_conditions(fx) -> None:
    """The conditions the seeded weights must meet for the 2e-4 parity bar to measure the engine and not the weights."""
    for tag, *_ in CASES:
        assert fx[f"std_db0_{tag}"] > 0.05 and fx[f"std_mask_{tag}"] > 0.05, (tag, fx[f"std_db0_{tag}"], fx[f"std_mask_{tag}"])
        for k in TAPS:
            assert 0.05 <= fx[f"std_{k}_{tag}"] <= 50, (tag, k, fx[f"std_{k}_{tag}"])
        assert fx[f"f32_vs_f64_{tag}"] <= 5e-5, (tag, fx[f"f32_vs_f64_{tag}"])
        assert fx[f"margin_share_{tag}"] <= 0.01, (tag, fx[f"margin_share_{tag}"])


def make_fixtures(path: str = FIXTURE):
    fx = fixture()
    check_conditions(fx)
    np.savez_compressed(path, source="manga_translator/detection/dbnet_convnext.py:450-509", **fx)
    return path


if __name__ == "__main__":
    print(make_fixtures())
