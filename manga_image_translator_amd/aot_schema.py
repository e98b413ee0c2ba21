"""State-dict layout of the reference AOT inpainter (``inpainting.ckpt`` = AOTGenerator(in_ch=4, out_ch=3, ch=32)).

Key names of ``AOTGenerator`` (manga_translator/inpainting/inpainting_aot.py:240-274): gated head layers ``head.{0,2,4}``,
ten ``AOTBlock(128)`` as ``body_conv.{i}`` (four dilated branches ``block0{0..3}.1``, ``fuse.1``, ``gate.1``; :170-193), gated
tail layers ``tail.{0,2,4,6,8}`` (``tail.4`` / ``tail.6`` transposed).  Every gated layer holds two scaled-WS convolutions
``conv`` / ``conv_gate`` with ``weight``, ``bias`` and ``gain`` (:53-146); the gain of a transposed layer is per INPUT channel.
tests/test_aot_cpu.py pins these names and shapes against the reference module's own state_dict.

The seeded gains and biases are chosen so that a synthetic page really exercises the network: the pre-clip output has a
standard deviation of a few tenths and a few percent of it clips (with PyTorch's default init every pixel decodes to ~127).
The branch and fuse weights are halved: the blend's sigmoid(5 * (2 z - 1)) amplifies rounding differences from block to block,
and smaller fuse outputs keep that growth (and with it the distance between any two fp32 implementations) small.
"""
from __future__ import annotations

from .synth import Schema

CH = 32
RATES = (2, 4, 8, 16)
N_BLOCKS = 10
# (prefix, Cin, Cout, k, transposed) of the gated layers, in forward order
GATED = (("head.0", 4, CH, 3, False), ("head.2", CH, 2 * CH, 4, False), ("head.4", 2 * CH, 4 * CH, 4, False),
         ("tail.0", 4 * CH, 4 * CH, 3, False), ("tail.2", 4 * CH, 4 * CH, 3, False), ("tail.4", 4 * CH, 2 * CH, 4, True),
         ("tail.6", 2 * CH, CH, 4, True), ("tail.8", CH, 3, 3, False))
GAIN_MUL = {"tail.8.conv": "*10.0"}   # the output layer's signal branch


def _gated(prefix: str, cin: int, cout: int, k: int, transposed: bool) -> Schema:
    s: Schema = []
    for cv in ("conv", "conv_gate"):
        p = f"{prefix}.{cv}"
        if transposed:
            s += [(p + ".weight", (cin, cout, k, k), "convT"), (p + ".bias", (cout,), "bias"), (p + ".gain", (cin, 1, 1, 1), "gain")]
        else:
            s += [(p + ".weight", (cout, cin, k, k), "conv"), (p + ".bias", (cout,), "bias"),
                  (p + ".gain", (cout, 1, 1, 1), "gain" + GAIN_MUL.get(p, ""))]
    return s


def aot_generator_schema() -> Schema:
    s: Schema = []
    for prefix, cin, cout, k, tr in GATED[:3]:
        s += _gated(prefix, cin, cout, k, tr)
    C = 4 * CH
    for i in range(N_BLOCKS):
        p = f"body_conv.{i}"
        for j in range(len(RATES)):
            s += [(f"{p}.block{j:02d}.1.weight", (C // 4, C, 3, 3), "conv*0.5"), (f"{p}.block{j:02d}.1.bias", (C // 4,), "bias")]
        s += [(f"{p}.fuse.1.weight", (C, C, 3, 3), "conv*0.5"), (f"{p}.fuse.1.bias", (C,), "bias")]
        s += [(f"{p}.gate.1.weight", (C, C, 3, 3), "conv"), (f"{p}.gate.1.bias", (C,), "bias")]
    for prefix, cin, cout, k, tr in GATED[3:]:
        s += _gated(prefix, cin, cout, k, tr)
    return s
