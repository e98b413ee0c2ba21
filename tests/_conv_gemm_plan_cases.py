"""Descriptors for the tile-choice tests (test_conv_gemm_plan.py on the CPU, test_conv_gemm_gpu.py on the device): fixed nested
loops, no random numbers.  ``mit_conv_gemm_plan`` dereferences no operand pointer, so the CPU cases carry fake, aligned ones."""
from manga_image_translator_amd import lib

FAKE_A, FAKE_W, FAKE_C, FAKE_WS = 4096, 8192, 16384, 32768

MODES = (0, 6, 9)
MIN_TILES = (0, 1280)
VARIANTS = ((0, 0), (0, 1), (1, 1), (1, 0))  # (nprod, w_split present); the last is refused
ZS = (1, 8, 36)
SHAPES = ((1, 1, 160), (1, 184, 1), (1, 64, 64), (1, 192, 160), (1, 1024, 1024), (4, 512, 512))  # (NB, Ho, Wo): 160 rows .. 4 x 512 x 512
CINS = (4, 16, 32, 48, 64, 320)
TAPS = (1, 4, 9, 16, 17)
NS = (1, 3, 4, 24, 32, 33, 64, 65, 80, 96, 128, 160, 192, 256, 320, 384)
STRETCH = (0, 1)  # 1: pixel stride stretched until the largest A offset is about 2^30 elements (past 2^31 bytes, below 2^31 elements)
KEEP_EVERY = 11   # the full product is 414,720 descriptors; every 11th of the flat loop index (a prime that divides no loop length,
                  # so every value of every loop meets every value of every other) is planned

# batches whose activations exceed 2^31 elements (the cut into runs): (NB, Ho, Wo), Cin, taps, N
CUT_SHAPES = ((16, 2048, 1456), (5, 2048, 1456), (3, 4096, 4096), (2, 8192, 8192))
CUT_CINS = (16, 64, 72)
CUT_TAPS = (1, 9, 17)
CUT_NS = (64, 128)


def desc(NB, Ho, Wo, Cin, taps, N, Z=1, split=0, nprod=0, stretch=0, a=FAKE_A, w=FAKE_W, c=FAKE_C, w_split=FAKE_WS):
    """A stride-1 ``taps``-tap layer over an NHWC activation [NB, Ho, Wo, Cin] into [NB, Ho, Wo, N] (all taps read the output pixel)."""
    d = lib.MitConvGemm()
    d.a, d.w, d.c.base = a, w, c
    d.NB, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.sy, d.sx = NB, Ho, Wo, Cin, Ho, Wo, 1, 1
    d.a_xs = max(Cin, ((1 << 30) // (NB * Ho * Wo) + 3) // 4 * 4) if stretch else Cin
    d.a_ys = d.a_xs * Wo
    d.a_bs = d.a_ys * Ho
    d.ntaps = taps
    K = taps * Cin
    Kp, Np = (K + 15) // 16 * 16, (N + 3) // 4 * 4
    d.ldw, d.Kw, d.Nw, d.N, d.Z, d.zdiv = Np, Kp, Np, N, Z, 1
    d.c.xs, d.c.ys, d.c.bs = Np, Np * Wo, Np * Wo * Ho
    if split:
        d.w_split, d.ws_zs0 = w_split, 0
    d.nprod = nprod
    return d


def sweep():
    """(mode, min_tiles, descriptor arguments) of every planned case, in the order of the golden file."""
    i = -1
    for mode in MODES:
        for mt in MIN_TILES:
            for nprod, split in VARIANTS:
                for Z in ZS:
                    for NB, Ho, Wo in SHAPES:
                        for Cin in CINS:
                            for taps in TAPS:
                                for N in NS:
                                    for stretch in STRETCH:
                                        i += 1
                                        if i % KEEP_EVERY == 0:
                                            yield mode, mt, dict(NB=NB, Ho=Ho, Wo=Wo, Cin=Cin, taps=taps, N=N, Z=Z, split=split, nprod=nprod, stretch=stretch)
    for mode in MODES:
        for nprod, split in VARIANTS[:3]:
            for NB, Ho, Wo in CUT_SHAPES:
                for Cin in CUT_CINS:
                    for taps in CUT_TAPS:
                        for N in CUT_NS:
                            yield mode, 0, dict(NB=NB, Ho=Ho, Wo=Wo, Cin=Cin, taps=taps, N=N, Z=1, split=split, nprod=nprod, stretch=0)


# The six launches of the device test (test_conv_gemm_gpu.py::test_launch_is_filed_under_the_planned_tile), each the smallest that
# still reaches its branch: name -> (mode, descriptor arguments).  Their expected tiles are in the golden file as well.
GPU_CASES = {
    "gemv": (6, dict(NB=1, Ho=32, Wo=32, Cin=64, taps=9, N=3)),
    "generic": (6, dict(NB=1, Ho=24, Wo=24, Cin=12, taps=9, N=64)),
    "fp32_underfilled": (0, dict(NB=1, Ho=40, Wo=40, Cin=64, taps=1, N=128)),
    "linear_bk32_mode6": (6, dict(NB=1, Ho=1, Wo=160, Cin=320, taps=1, N=960, split=1)),
    "linear_bk32_mode9": (9, dict(NB=1, Ho=1, Wo=160, Cin=320, taps=1, N=960, split=1)),
    "p1_k16": (6, dict(NB=1, Ho=24, Wo=24, Cin=48, taps=9, N=64, split=1, nprod=1)),
}


def tile_names(handle):
    names = []
    while handle.mit_conv_gemm_config_name(len(names)) is not None:
        names.append(handle.mit_conv_gemm_config_name(len(names)).decode())
    return names


def plan(handle, d, cfg=-1):
    """'name:nb_run' of mit_conv_gemm_plan, or the refusal text."""
    import ctypes as C

    tile, nb = C.c_int32(-1), C.c_int32(0)
    if handle.mit_conv_gemm_plan(C.byref(d), cfg, C.byref(tile), C.byref(nb)) != 0:
        return "refused: " + handle.mit_last_error().decode()
    return f"{handle.mit_conv_gemm_config_name(tile.value).decode()}:{nb.value}"
