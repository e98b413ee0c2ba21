"""ctypes binding of the C-ABI in ``include/mit_hip.h``.

The library is the product: if it cannot be loaded the import of any op raises — there is
no CPU or PyTorch fallback behind these entry points.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

from . import cheader

# The header is the single source of the binding (it is read at run time anyway: build.source_digest() hashes it on every load()).
# Nothing below restates a type or a value: the struct classes (MitConvGemm, MitProfStat, ...), the prototypes and the constants are
# what cheader.parse() reads out of it, under its one pointer rule (char * is c_char_p, every other pointer c_void_p).
HEADER = Path(__file__).resolve().parent.parent / "include" / "mit_hip.h"
CONSTANTS, STRUCTS, SYMBOLS, ENUMS = cheader.parse(HEADER.read_text())  # SYMBOLS: every declared function, name -> (restype, argtypes)

globals().update(STRUCTS)    # lib.MitTensorMap ... lib.MitOcr32DecodeArgs
globals().update(CONSTANTS)  # MIT_ABI_VERSION, MIT_MAX_TAPS, MIT_CONVT_COUT1_STRIP_K4 / _K2, MIT_ACT_POST_FIRST
# the activation and padding codes go by their short names: ACT_NONE ... ACT_GELU, ACT_POST_FIRST, PAD_ZERO, PAD_REFLECT
globals().update({k[len("MIT_"):]: v for k, v in {**ENUMS, "MIT_ACT_POST_FIRST": CONSTANTS["MIT_ACT_POST_FIRST"]}.items()})

_lib = None


def lib_path() -> Path:
    return Path(__file__).resolve().parent / "libmit_hip.so"


def _stale(path: Path, want: str) -> bool:
    """True when the binary at ``path`` was built from other sources than the tree's.  The digest is read from the marker
    string in the file, not through dlopen: a stale library must not stay mapped when its replacement is loaded."""
    needle = b"MIT_SOURCE_DIGEST=" + want.encode()
    try:
        with open(path, "rb") as f:  # chunked scan: the library is ~10 MB and every process start checks it
            tail = b""
            while True:
                chunk = f.read(1 << 20)
                if not chunk:
                    return True
                if needle in tail + chunk:
                    return False
                tail = chunk[-len(needle):]
    except OSError:
        return True


def load(build_if_missing: bool = True) -> C.CDLL:
    """Load ``libmit_hip.so``.  A missing library, or one built from other sources than the tree's (``mit_source_digest()``
    against ``build.source_digest()``), is rebuilt with hipcc when ``build_if_missing`` — otherwise that is an error: old
    kernels are never validated or measured silently.  Raises on any failure."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build as _build

    path = lib_path()
    want = _build.source_digest()
    if not path.exists() or _stale(path, want):
        if not build_if_missing:
            what = "is missing" if not path.exists() else "was built from different sources than this tree"
            raise RuntimeError(f"{path} {what}: run `python -m manga_image_translator_amd.build`")
        # several processes (the ranks of a multi-GPU launch, pytest workers) may find the library stale at the same moment: one of
        # them builds under an exclusive file lock, the others wait and re-check; the build links to a temporary name and renames
        import fcntl

        with open(str(path) + ".lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if not path.exists() or _stale(path, want):
                    _build.build(force=True)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.mit_abi_version() != CONSTANTS["MIT_ABI_VERSION"]:
        raise RuntimeError(f"libmit_hip.so ABI {lib.mit_abi_version()} != header {CONSTANTS['MIT_ABI_VERSION']}")
    if lib.mit_source_digest().decode() != want:
        raise RuntimeError(f"{path} does not match the sources it was just built from (digest mismatch)")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    """Turn a non-zero status into RuntimeError carrying ``mit_last_error()``."""
    if rc != 0:
        msg = load().mit_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what}: {msg}" if what else msg)
