"""The C-ABI library: loads and exports every function include/mit_hip.h declares; the ctypes binding lib.py derives from that header
(cheader.py) has every declared function, the C compiler's size and field offsets for every struct (gcc compiles a probe against the
real header) and the literal prototypes pinned below; the header reader refuses what it cannot read.  No compute calls: those are the
``-m gpu`` tests."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mit_hip.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mit_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from manga_image_translator_amd import lib

    handle = lib.load(build_if_missing=True)
    names = _declared_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(handle, n), f"{n} declared in mit_hip.h but not exported by libmit_hip.so"
        assert n in lib.SYMBOLS, f"{n} has no ctypes prototype in lib.SYMBOLS"
    assert set(lib.SYMBOLS) <= set(names), sorted(set(lib.SYMBOLS) - set(names))
    assert handle.mit_abi_version() == lib.MIT_ABI_VERSION
    assert handle.mit_conv_gemm_config_name(0) == b"128x128x16" and handle.mit_conv_gemm_config_name(99) is None


def test_error_channel_without_gpu():
    """Argument validation happens before any HIP call, so it is observable on a CPU-only box."""
    from manga_image_translator_amd import lib

    handle = lib.load()
    assert handle.mit_conv_gemm(None, None) != 0
    assert b"null descriptor" in handle.mit_last_error()
    d = lib.MitConvGemm()
    assert handle.mit_conv_gemm(C.byref(d), None) != 0
    assert b"null operand" in handle.mit_last_error()
    with pytest.raises(RuntimeError, match="null operand"):
        lib.check(1, "probe")
    assert handle.mit_ocr_warp_lines(None, 1, 1, None, 0, None, 48, 8, None) != 0


def test_pgemm_argument_checks_without_gpu():
    """mit_pgemm validates its descriptor before any HIP call (sizes, alignment, output kind, activation)."""
    from manga_image_translator_amd import lib

    handle = lib.load()
    assert handle.mit_pgemm(None, None) != 0 and b"null descriptor" in handle.mit_last_error()
    d = lib.MitPGemm()
    assert handle.mit_pgemm(C.byref(d), None) != 0 and b"null operand" in handle.mit_last_error()
    d.a_planes, d.w_planes = 4096, 8192     # never dereferenced: every case below is refused first
    d.M, d.N, d.K, d.Z, d.lda, d.ldw = 128, 64, 24, 1, 128, 64
    assert handle.mit_pgemm(C.byref(d), None) != 0 and b"K % 16" in handle.mit_last_error()
    d.K = 32
    assert handle.mit_pgemm(C.byref(d), None) != 0 and b"exactly one of c / c_planes" in handle.mit_last_error()
    d.c, d.ldc = 16384, 62
    assert handle.mit_pgemm(C.byref(d), None) != 0 and b"ldc % 4" in handle.mit_last_error()
    d.ldc, d.act = 64, lib.ACT_SILU
    assert handle.mit_pgemm(C.byref(d), None) != 0 and b"none / relu / gelu" in handle.mit_last_error()
    d.act, d.lda = lib.ACT_RELU, 100
    assert handle.mit_pgemm(C.byref(d), None) != 0 and b"lda / ldw" in handle.mit_last_error()
    d.lda, d.c, d.c_planes, d.ld_cp, d.N = 128, None, 16384, 128, 60
    assert handle.mit_pgemm(C.byref(d), None) != 0 and b"N % 8" in handle.mit_last_error()
    assert handle.mit_pgemm_supported(C.byref(d)) == 0
    d.N = 64
    assert handle.mit_pgemm_supported(C.byref(d)) == 1
    names = []
    while handle.mit_pgemm_tile_name(len(names)) is not None:
        names.append(handle.mit_pgemm_tile_name(len(names)).decode())
    assert names[:4] == ["pg128x128s3p6", "pg128x64s3p6", "pg128x128s3p6P", "pg128x64s3p6P"] and len(set(names)) == len(names)
    assert handle.mit_split_planes(None, 0, 1, 8, None, 1, None) != 0 and b"null pointer" in handle.mit_last_error()
    assert handle.mit_split_planes(4096, 12, 4, 12, 8192, 4, None) != 0 and b"K % 8" in handle.mit_last_error()


def test_ocr48_decode_refuses_unknown_forms_without_gpu():
    """MitOcr48DecodeArgs.forms_off is checked before the decoder is read and before any HIP call: a bit that names no kernel form
    is an error, not a form silently left on."""
    from manga_image_translator_amd import lib

    handle = lib.load()
    dec, a = lib.MitOcr48Decoder(), lib.MitOcr48DecodeArgs()
    a.forms_off = 1 << 9
    assert handle.mit_ocr48_decode(C.byref(dec), C.byref(a), None) != 0
    assert b"forms_off" in handle.mit_last_error()
    assert (lib.MIT_OCR48_FORM_ROWS, lib.MIT_OCR48_FORM_LN_FUSED, lib.MIT_OCR48_FORM_Q2_FUSED, lib.MIT_OCR48_FORM_FF2_SPLITK,
            lib.MIT_OCR48_FORM_SELF_ROWS, lib.MIT_OCR48_ROWS_MAX) == (1, 2, 4, 8, 16, 2560)


def test_ctypes_structs_match_c_layout(tmp_path):
    """Every struct the header declares, not a hand-kept list: size and every field offset as gcc lays them out."""
    from manga_image_translator_amd import lib

    structs = lib.STRUCTS
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert set(structs) == set(re.findall(r"typedef\s+struct\s+(\w+)", src)) and len(structs) >= 19
    assert all(getattr(lib, name) is st for name, st in structs.items())
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for name, st in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for fname, *_ in st._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ["return 0; }"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, st in structs.items():
        assert int(out[name]) == C.sizeof(st), name
        for fname, *_ in st._fields_:
            assert int(out[f"{name}.{fname}"]) == getattr(st, fname).offset, f"{name}.{fname}"


def test_prototype_pins():
    """Literal prototypes of entries that exercise each rule of the header reader: a wrong scalar width (int for int64_t) would
    truncate a stride silently."""
    from manga_image_translator_amd import lib

    P, I, Q, F, D, S = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_char_p
    assert lib.SYMBOLS["mit_last_error"] == (S, [])
    assert lib.SYMBOLS["mit_device_name"] == (I, [I, S, I])
    assert lib.SYMBOLS["mit_lama_tail_need_work"] == (Q, [I, I, I])
    assert lib.SYMBOLS["mit_convt_cout1"] == (I, [P, Q, Q, Q, I, I, I, I, P, I, I, I, P, P, I, F, P, Q, Q, Q, I, I, P])
    assert lib.SYMBOLS["mit_mask_assign_lines"] == (I, [P, I, I, P, P, P, I, I, D, P, Q, P, Q, P, P, P])
    assert lib.SYMBOLS["mit_ocr32_decode"] == (I, [P, P, P])
    assert lib.SYMBOLS["mit_prof_enable"] == (I, [I])
    assert lib.SYMBOLS["mit_logsoftmax_top5"] == (I, [P, Q, I, I, I, P, P, I, P])
    assert (lib.MIT_ABI_VERSION, lib.MIT_MAX_TAPS, lib.MIT_CONVT_COUT1_STRIP_K4, lib.MIT_CONVT_COUT1_STRIP_K2) == (26, 64, 16, 64)
    assert (lib.ACT_NONE, lib.ACT_RELU, lib.ACT_LEAKY, lib.ACT_SILU, lib.ACT_SIGMOID, lib.ACT_GELU) == tuple(range(6))
    assert (lib.ACT_POST_FIRST, lib.PAD_ZERO, lib.PAD_REFLECT) == (0x100, 0, 1)


@pytest.mark.parametrize("text, named", [
    ("int mit_f(size_t n);", "size_t"),                                    # an unknown type
    ("typedef struct S { foo_t *p; } S;", "foo_t"),                       # ... also behind a pointer
    ("int mit_f(void (*cb)(int), int n);", "mit_f"),                       # a function-pointer parameter
    ("typedef struct S { int a : 3; } S;", "a : 3"),                       # a bit-field
    ("typedef union U { int a; float b; } U;", "typedef union U"),         # a union
    ("typedef struct S { union { int a; float b; } u; } S;", "struct S"),  # ... also inside a struct
    ("int mit_f(int, float x);", "int"),                                   # an unnamed parameter
    ("typedef struct S { int a[N]; } S;", "N"),                            # an extent that is no #define
    ("enum E { A, B };", "A"),                                             # an enumerator without a value
    ("#define MIT_F(x) (x)", "MIT_F"),                                     # a function-like macro
    ("int mit_f(int n)", "mit_f"),                                         # a declaration that never ends
    ("int mit_ok(int n);", "mit_ok"),                                      # a second prototype of one name
    ("int mit_f(int n[4]);", "mit_f"),                                     # an array parameter
])
def test_header_reader_refuses_what_it_cannot_read(text, named):
    from manga_image_translator_amd import cheader

    with pytest.raises(cheader.HeaderError, match=re.escape(named)):
        cheader.parse("/* c */ int mit_ok(void);\n" + text)


def test_header_reader_on_a_synthetic_header():
    from manga_image_translator_amd import cheader

    consts, structs, funcs, enums = cheader.parse("""
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define N 3 /* extent */
        #define MASK 0x10
        enum E { E_A = 0, E_B = 7 };
        typedef struct In { int8_t tag; double ms, a, b; } In;  /* several declarators on a line */
        typedef struct Out {
            char name[5];
            const float *w, *b;
            int16_t taps[N];   /* sized by a #define */
            In rows[2];        /* an array of nested structs */
            In one;
            int32_t n, _pad;
        } Out;
        const char *mit_name(void);
        int64_t mit_run(const Out *o, char *buf, uint64_t *sums, float alpha,
                        void *stream);
        void mit_reset(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert consts == {"N": 3, "MASK": 16} and enums == {"E_A": 0, "E_B": 7}
    In, Out = structs["In"], structs["Out"]
    assert [f[0] for f in In._fields_] == ["tag", "ms", "a", "b"] and C.sizeof(In) == 32 and In.ms.offset == 8 and In.b.offset == 24
    assert [(n, getattr(Out, n).offset, getattr(Out, n).size) for n, _ in Out._fields_] == [
        ("name", 0, 5), ("w", 8, 8), ("b", 16, 8), ("taps", 24, 6), ("rows", 32, 64), ("one", 96, 32), ("n", 128, 4), ("_pad", 132, 4)]
    assert C.sizeof(Out) == 136
    assert dict(Out._fields_)["w"] is C.c_void_p and dict(Out._fields_)["rows"] is In * 2 and dict(Out._fields_)["taps"] is C.c_int16 * 3
    assert funcs == {"mit_name": (C.c_char_p, []), "mit_reset": (None, []),
                     "mit_run": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_float, C.c_void_p])}


def test_stale_library_is_refused(tmp_path, monkeypatch):
    """lib.load() compares the digest embedded in the binary with the digest of the sources in the tree: a library built
    from other sources is an error when rebuilding is not allowed (never validated or measured silently)."""
    from manga_image_translator_amd import build, lib

    handle = lib.load(build_if_missing=True)
    assert handle.mit_source_digest().decode() == build.source_digest()
    assert not lib._stale(lib.lib_path(), build.source_digest())
    assert lib._stale(lib.lib_path(), "0" * 64) and lib._stale(tmp_path / "missing.so", build.source_digest())
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(build, "source_digest", lambda: "0" * 64)
    with pytest.raises(RuntimeError, match="different sources"):
        lib.load(build_if_missing=False)


def test_workspace_is_bounded_by_the_largest_request():
    """Engine workspaces are grow-only slabs keyed by name: heterogeneous page sizes re-view one slab instead of allocating a
    buffer set per shape."""
    import torch

    from manga_image_translator_amd import ops

    ws = ops.Workspace("cpu")
    a = ws.buf("x", 2, 8, 8, 4)
    assert a.shape == (2, 8, 8, 4) and a.is_contiguous()
    big = ws.buf("x", 1, 32, 16, 4)
    n = ws.nbytes()
    for shape in [(2, 8, 8, 4), (1, 16, 16, 4), (1, 31, 16, 4), (1, 32, 16, 4)]:
        t = ws.buf("x", *shape)
        assert t.data_ptr() == big.data_ptr() and tuple(t.shape) == shape
    assert ws.nbytes() == n == 1 * 32 * 16 * 4 * 4
    assert ws.buf("x", 4, dtype=torch.uint8).data_ptr() != big.data_ptr()  # other dtype, other slab
    ws.release()
    assert ws.nbytes() == 0
    sc = ops.ShapeCache(2)
    made = []
    for k in [(1, 1), (2, 2), (1, 1), (3, 3), (2, 2)]:
        sc.get(k, lambda k=k: made.append(k) or k)
    assert made == [(1, 1), (2, 2), (3, 3), (2, 2)] and len(sc) == 2
