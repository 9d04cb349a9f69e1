"""CPU: the reader of include/ksmi.h (kurosiwo_amd/_abi.py), from which the ctypes binding and the call thunks are derived.  Every
construct the header uses on small snippets, every construct the reader refuses with its KsmiError, and the derived struct layouts
and constants against a C compiler that reads the same header."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from kurosiwo_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants():
    abi = _abi.parse("""
        #ifndef KSMI_H
        #define KSMI_H          /* a guard is no constant */
        #include <stdint.h>
        #define KSMI_ABI_VERSION 8   /* 8: a long story; 7: with a #define KSMI_NOT 1 inside the comment */
        #define KSMI_E_ARG (-1)
        #define KSMI_MASK 0x10
        #define KSMI_NAME "text"
        #define OTHER_THING 3
        #endif
    """)
    assert abi.constants == {"KSMI_ABI_VERSION": 8, "KSMI_E_ARG": -1, "KSMI_MASK": 16}
    assert not abi.structs and not abi.signatures


def test_struct_members():
    abi = _abi.parse("""
        #define KSMI_MAX_SRC 6
        typedef struct ksmi_src {
          const void* ptr;     /* NHWC activations */
          const float* scale; const float* shift;
          int32_t C, c_off;    // two declarators
          float *a, b;         /* the star belongs to a alone */
        } ksmi_src;
        typedef struct ksmi_conv_desc {
          ksmi_src src[KSMI_MAX_SRC];
          int32_t nsrc, ndst;
          uint16_t chunk_c0[KSMI_MAX_SRC];
          uint8_t chunk_src[ 3 ];
          double origin[2], tie_pixel[2];
          int64_t sK;
          const uint64_t* args;
          float alpha;
        } ksmi_conv_desc;
    """)
    src, desc = abi.structs["ksmi_src"], abi.structs["ksmi_conv_desc"]
    assert (src.__name__, desc.__name__) == ("Src", "ConvDesc") and issubclass(desc, C.Structure)
    assert src._fields_ == [("ptr", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p), ("C", C.c_int32), ("c_off", C.c_int32),
                            ("a", C.c_void_p), ("b", C.c_float)]
    assert desc._fields_ == [("src", src * 6), ("nsrc", C.c_int32), ("ndst", C.c_int32), ("chunk_c0", C.c_uint16 * 6),
                             ("chunk_src", C.c_uint8 * 3), ("origin", C.c_double * 2), ("tie_pixel", C.c_double * 2),
                             ("sK", C.c_int64), ("args", C.c_void_p), ("alpha", C.c_float)]
    assert C.sizeof(src) == 48 and desc.nsrc.offset == 6 * 48


def test_function_declarations():
    abi = _abi.parse("""
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct ksmi_d { int32_t n; } ksmi_d;
        int ksmi_abi_version(void);
        const char* ksmi_last_error(void);
        void* ksmi_runner_create(void);
        size_t ksmi_workspace(const ksmi_d* d, int dtype);
        int64_t ksmi_scratch(int64_t n);
        void ksmi_nothing();
        int ksmi_pool(const void* const x[4], float* avg, int32_t* argmax /* or NULL */,
                      void** out, unsigned* sink, const char* const* paths, const unsigned char* valid,
                      int B, int64_t npix, size_t nbytes, uint32_t seed, unsigned int bits, float eps, double count,
                      void* stream);
        int ksmi_host_only(const char* path, ksmi_d* info);
        #ifdef __cplusplus
        }
        #endif
    """)
    vp = C.c_void_p
    assert abi.signatures == {
        "ksmi_abi_version": (C.c_int, []), "ksmi_last_error": (C.c_char_p, []), "ksmi_runner_create": (vp, []),
        "ksmi_workspace": (C.c_size_t, [vp, C.c_int]), "ksmi_scratch": (C.c_int64, [C.c_int64]), "ksmi_nothing": (None, []),
        "ksmi_pool": (C.c_int, [vp] * 7 + [C.c_int, C.c_int64, C.c_size_t, C.c_uint32, C.c_uint32, C.c_float, C.c_double, vp]),
        "ksmi_host_only": (C.c_int, [vp, vp])}
    assert abi.params["ksmi_pool"] == ["x", "avg", "argmax", "out", "sink", "paths", "valid", "B", "npix", "nbytes", "seed", "bits", "eps",
                                       "count", "stream"]
    assert abi.listable() == {"ksmi_pool": "pppppppilzuufd"}            # int status and `stream` last; the stream has no letter
    assert _abi.sig_codes([vp, C.c_char_p, C.POINTER(C.c_int), vp * 4, C.c_int, C.c_int32, C.c_uint32, C.c_int64, C.c_size_t, C.c_float,
                           C.c_double]) == "ppppiiulzfd"


@pytest.mark.parametrize("snippet, names", [
    ("int ksmi_f(long n);", "long n"),                                                    # a type the rule does not name
    ("int ksmi_f(struct foo* p);", "struct foo* p"),
    ("typedef struct ksmi_s { wchar_t c; } ksmi_s;", "wchar_t c"),
    ("int ksmi_f(int (*callback)(int), void* stream);", "ksmi_f"),                        # a function-pointer parameter
    ("typedef struct ksmi_s { int (*callback)(int); } ksmi_s;", "callback"),
    ("typedef struct ksmi_s { int32_t flag : 1; } ksmi_s;", "flag : 1"),                  # a bit-field
    ("typedef union ksmi_u { int32_t i; float f; } ksmi_u;", "typedef union ksmi_u"),     # a union
    ("typedef struct ksmi_s { union { int32_t i; float f; } u; } ksmi_s;", "typedef struct ksmi_s"),
    ("#define KSMI_N (2 * 3)\ntypedef struct ksmi_s { int32_t t[KSMI_N]; } ksmi_s;", "KSMI_N"),     # not an integer macro
    ("#define KSMI_N 1.5\nint ksmi_f(const float w[KSMI_N]);", "KSMI_N"),
    ("typedef struct ksmi_s { int32_t t[UNDEFINED]; } ksmi_s;", "UNDEFINED"),
    ("typedef struct ksmi_s { int32_t t[2][3]; } ksmi_s;", "t[2][3]"),
    ("typedef struct ksmi_s { int32_t; } ksmi_s;", "int32_t"),                            # a member without a name
    ("typedef struct ksmi_s { void v; } ksmi_s;", "v"),
    ("typedef struct ksmi_s { } ksmi_s;", "ksmi_s"),
    ("typedef struct ksmi_d { int32_t n; } ksmi_d;\nint ksmi_f(ksmi_d d);", "ksmi_d"),    # a struct by value
    ("typedef struct ksmi_d { int32_t n; } ksmi_d;\nksmi_d ksmi_f(void);", "ksmi_f"),
    ("int ksmi_f(uint8_t flag);", "uint8_t"),                                             # (a member type only: no thunk letter)
    ("int ksmi_f(char c);", "char"),
    ("typedef int ksmi_status;", "typedef int ksmi_status"),
    ("extern int ksmi_counter;", "ksmi_counter"),
    ("static inline int ksmi_f(int a) { return a; }", "ksmi_f"),                          # a definition
    ("int ksmi_f(int a)", "ksmi_f"),                                                      # no semicolon
])
def test_what_the_reader_does_not_recognise_raises(snippet, names):
    with pytest.raises(_lib.KsmiError, match="ksmi.h: ") as e:
        _abi.parse(snippet)
    assert names in str(e.value), str(e.value)


def _host_compiler():
    """the compiler that built the host side of the library: cc, else the clang of the ROCm tree that holds hipcc"""
    cc = shutil.which("cc")
    if cc:
        return cc
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    top = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(top, "llvm", "bin", "clang"), os.path.join(top, "lib", "llvm", "bin", "clang")):
        if os.path.exists(cand):
            return cand
    pytest.fail(f"no host C compiler: neither cc nor a clang next to {hipcc}")


def test_layouts_and_constants_against_the_compiler(tmp_path):
    """a C program that includes ksmi.h prints sizeof of every struct, offsetof / sizeof of every member and every KSMI_* constant"""
    abi = _lib.ABI
    assert len(abi.structs) == 8 and len(abi.constants) >= 14
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ksmi.h"', 'int main(void) {']
    expect = []
    for cname, cls in abi.structs.items():
        src.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        expect.append(f"{cname} {C.sizeof(cls)}")
        for field, _ in cls._fields_:
            src.append(f'  printf("{cname}.{field} %zu %zu\\n", offsetof({cname}, {field}), sizeof((({cname}*)0)->{field}));')
            expect.append(f"{cname}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    for name, value in abi.constants.items():
        src.append(f'  printf("{name} %lld\\n", (long long)({name}));')
        expect.append(f"{name} {value}")
    src += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) > 170
    assert got == expect
    # the names the package uses are those classes and values
    assert (_lib.Src, _lib.Dst, _lib.ConvDesc, _lib.PackDesc, _lib.WgradDesc, _lib.RowsumDesc, _lib.TiffInfo, _lib.Op) == tuple(
        abi.structs[n] for n in ("ksmi_src", "ksmi_dst", "ksmi_conv_desc", "ksmi_pack_desc", "ksmi_wgrad_desc", "ksmi_rowsum_desc",
                                 "ksmi_tiff_info", "ksmi_op"))
    assert (_lib.KSMI_F32, _lib.KSMI_BF16, _lib.MAX_SRC, _lib.MAX_CHUNKS, _lib.ABI_VERSION) == (0, 1, 6, 72, 8)
    assert (_lib.LOSS_DICE, _lib.LOSS_LOVASZ, _lib.LOSS_FOCAL, _lib.OP_CALL, _lib.OP_ORDER, _lib.OP_WAIT_SIDE) == (1, 2, 3, 0, 1, 2)
