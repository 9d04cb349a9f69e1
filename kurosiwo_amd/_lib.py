"""ctypes binding of libksmi.so, derived from include/ksmi.h (the C-ABI) when this module is first imported.

The header is the one place where an entry point, a descriptor struct or a constant is written down: _abi.parse reads it (one pass,
nothing kept on disk) into SIGNATURES (name -> (restype, argtypes)), the ctypes.Structure classes and the KSMI_* constants below.
To add an entry point, declare it in include/ksmi.h and re-run tools/gen_thunks.py; there is no table to extend here.

The product path has NO fallback: if the header does not parse, the shared library is missing or a symbol is absent, this raises.
"""
import ctypes as C
import os

from ._abi import KsmiError, parse, sig_codes  # noqa: F401  (sig_codes: the letter codes of the call thunks, for launch.py and the tools)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libksmi.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ksmi.h")

try:
    with open(HEADER_PATH) as _f:
        ABI = parse(_f.read())
except OSError as e:
    raise KsmiError(f"{HEADER_PATH}: the binding is derived from this header and cannot be built without it") from e

SIGNATURES = ABI.signatures          # name -> (restype, argtypes), every entry point of the header; load fails if the library lacks one
Src, Dst, ConvDesc, PackDesc, WgradDesc, RowsumDesc, TiffInfo, Op = (
    ABI.structs["ksmi_" + n] for n in ("src", "dst", "conv_desc", "pack_desc", "wgrad_desc", "rowsum_desc", "tiff_info", "op"))
KSMI_F32, KSMI_BF16, ABI_VERSION, MAX_SRC, MAX_CHUNKS, LOSS_DICE, LOSS_LOVASZ, LOSS_FOCAL, OP_CALL, OP_ORDER, OP_WAIT_SIDE = (
    ABI.constants["KSMI_" + n] for n in ("F32", "BF16", "ABI_VERSION", "MAX_SRC", "MAX_CHUNKS", "LOSS_DICE", "LOSS_LOVASZ", "LOSS_FOCAL",
                                         "OP_CALL", "OP_ORDER", "OP_WAIT_SIDE"))

_lib = None


def load():
    """dlopen libksmi.so and bind every declared symbol.  Raises KsmiError on any problem."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KsmiError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C kurosiwo_amd/csrc`.")
    try:
        import torch  # noqa: F401  (libamdhip64 is resolved from the torch process first)
    except Exception:  # pragma: no cover
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise KsmiError(f"libksmi.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.ksmi_abi_version() != ABI_VERSION:
        raise KsmiError(f"libksmi ABI {lib.ksmi_abi_version()} != binding {ABI_VERSION}")
    for which, cls in enumerate((ConvDesc, WgradDesc, PackDesc, RowsumDesc, TiffInfo)):        # this .so was built from this header
        if lib.ksmi_desc_size(which) != C.sizeof(cls):
            raise KsmiError(f"libksmi {cls.__name__}: {lib.ksmi_desc_size(which)} bytes in the library, {C.sizeof(cls)} in the binding")
    _lib = lib
    return lib


def set_knob(name, value):
    """ksmi_set_knob (include/ksmi.h): a run-time switch of the launchers (tests / probes only); value None = built-in default"""
    rc = load().ksmi_set_knob(name.encode(), None if value is None else str(value).encode())
    if rc != 0:
        check(rc, "ksmi_set_knob")


class knobs:
    """with knobs(KSMI_IGEMM4_CUS="3", KSMI_IGEMM4_VAR="8,2"): ...  -- restores the built-in defaults on exit"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            set_knob(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            set_knob(k, None)
        return False


def check(rc, what=""):
    if rc != 0:
        msg = load().ksmi_last_error()
        raise KsmiError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
