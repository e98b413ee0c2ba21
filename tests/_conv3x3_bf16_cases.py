"""What the GPU tests of the two bf16-resident 3x3 convolutions share (tests/test_rdb_bf16_gpu.py, tests/test_aot_bf16_kernels_gpu.py):
sentinel-filled padded buffers, the seeded operand recipe, the bit views and the check of the fp32 output against the derived bound
(9 * Cin + 8) * 2^-24 * mag, whose argument is in the docstring of tests/test_rdb_bf16_gpu.py."""
import torch

SENT_BF16, SENT_F32 = 777.0, -12345.0
U = 2.0 ** -24


def _padded(B, H, W, Cn, ld, dtype, fill, dev, c0=0):
    """A [B, H, W, Cn] view (channels c0 .. c0 + Cn) of a [B, H, W + 1, ld] buffer filled with ``fill``: padded x and y strides."""
    base = torch.full((B, H, W + 1, ld), fill, dtype=dtype, device=dev)
    return base, base[:, :, :W, c0:c0 + Cn]


def _activations(g, B, H, W, Cin):
    """bf16 activations (CPU) whose images differ in magnitude by 1000x."""
    a = torch.randn(B, H, W, Cin, generator=g)
    return (a * torch.tensor([1.0, 1000.0])[:B].view(B, 1, 1, 1)).to(torch.bfloat16)


def _weight(g, N, Cin):
    return torch.randn(N, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)


def _check_f32(got, ref, mag, Cin, what):
    err = (got.double() - ref).abs()
    tol = (9 * Cin + 8) * U * mag
    worst = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err / tol {worst:.3f}")
    assert bool((err <= tol).all()), (what, worst)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _bits32(t):
    return t.contiguous().view(torch.int32)
