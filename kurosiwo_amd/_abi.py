"""Reader of include/ksmi.h: the header is the ONE description of the C-ABI of libksmi.so; the ctypes binding (_lib.py) and the call
thunks of the launch-list executor (tools/gen_thunks.py) are derived from what parse() returns.

parse(text) reads `#define KSMI_* <integer>` into constants, `typedef struct ... { ... } name;` into ctypes.Structure classes and
every `ret name(args);` into (restype, argtypes).  It knows the C the header is written in and nothing more: whatever it does not
recognise (an unknown type, a function-pointer parameter, a bit-field, a union, an array sized by something that is not an integer)
raises KsmiError with the declaration in the message.  It never guesses and never skips a declaration.

Type rule.  Scalars map by name (SCALARS).  Every pointer parameter, array parameter and pointer member is c_void_p: the header
cannot tell a host pointer from a device address, and c_void_p takes what the call sites pass (data_ptr() integers, None, byref(),
ctypes arrays, bytes).  A `char*` return is c_char_p, any other pointer return c_void_p.
"""
import ctypes as C
import re


class KsmiError(RuntimeError):
    pass


# C scalar -> (ctypes type, letter of the call-thunk signature strings; None: a struct member only, never passed by value)
SCALARS = {
    "int": (C.c_int, "i"), "int32_t": (C.c_int32, "i"),
    "unsigned": (C.c_uint32, "u"), "unsigned int": (C.c_uint32, "u"), "uint32_t": (C.c_uint32, "u"),
    "int64_t": (C.c_int64, "l"), "size_t": (C.c_size_t, "z"), "float": (C.c_float, "f"), "double": (C.c_double, "d"),
    "uint8_t": (C.c_uint8, None), "uint16_t": (C.c_uint16, None), "uint64_t": (C.c_uint64, None),
}
_POINTEES = ("void", "char", "unsigned char")          # types the header names only behind a `*`
_LETTER = {t: c for t, c in SCALARS.values() if c}


def sig_codes(argtypes):
    """signature string of the call thunks: one letter per ctypes argument type (p pointer, i int, u unsigned, l int64, z size_t,
    f float, d double)"""
    return "".join("p" if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)) else _LETTER[t] for t in argtypes)


def struct_class_name(cname):
    """ksmi_conv_desc -> ConvDesc"""
    return "".join(w.capitalize() for w in cname.removeprefix("ksmi_").split("_"))


class Abi:
    """constants: {"KSMI_MAX_SRC": 6, ...}; structs: {"ksmi_src": <Structure class Src>, ...}; signatures: {name: (restype, argtypes)};
    params: {name: [parameter names]}"""

    def __init__(self):
        self.constants, self.structs, self.signatures, self.params = {}, {}, {}, {}

    def listable(self):
        """the entry points a launch list may hold -- int status, last parameter `void* stream` -- with their signature strings
        (the arguments WITHOUT the stream): {name: "ppli", ...}"""
        return {n: sig_codes(a[:-1]) for n, (r, a) in self.signatures.items()
                if r is C.c_int and a and a[-1] is C.c_void_p and self.params[n][-1] == "stream"}


def _declarator(text, abi, where):
    """`const float* m_mean`, `ksmi_src src[KSMI_MAX_SRC]`, `void** out` -> (base type, pointer?, name or None, array length or None)"""
    m = re.fullmatch(r"([\w\s*]+?)(?:\[\s*(\w+)\s*\])?", text.strip())
    if not m:
        raise KsmiError(f"ksmi.h: cannot read `{' '.join(text.split())}` in `{where}`")
    words = [w for w in m[1].replace("*", " ").split() if w != "const"]
    known = lambda t: t in SCALARS or t in _POINTEES or t in abi.structs        # noqa: E731
    if known(" ".join(words)):                       # (first, so that `unsigned int` is a type and not an `unsigned` called int)
        base, name = " ".join(words), None
    elif known(" ".join(words[:-1])):
        base, name = " ".join(words[:-1]), words[-1]
    else:
        raise KsmiError(f"ksmi.h: unknown type in `{' '.join(text.split())}` in `{where}`")
    n = m[2]
    if n is not None:
        n = int(n) if n.isdigit() else abi.constants.get(n)
        if n is None:
            raise KsmiError(f"ksmi.h: the array size `{m[2]}` is not an integer constant in `{where}`")
    return base, "*" in m[1], name, n


def _struct(cname, body, abi):
    where = f"struct {cname}"
    fields = []
    for stmt in body.split(";")[:-1]:
        base = None
        for piece in stmt.split(","):              # `int32_t nsrc, ndst`: the base type carries over, a `*` does not (as in C)
            base, ptr, name, n = _declarator(piece if base is None else f"{base} {piece}", abi, where)
            if name is None:
                raise KsmiError(f"ksmi.h: a member without a name in `{' '.join(stmt.split())}` of `{where}`")
            if ptr:
                t = C.c_void_p
            elif base in _POINTEES:
                raise KsmiError(f"ksmi.h: a `{base}` member `{name}` by value in `{where}`")
            else:
                t = abi.structs[base] if base in abi.structs else SCALARS[base][0]
            fields.append((name, t if n is None else t * n))
    if body.split(";")[-1].strip() or not fields:
        raise KsmiError(f"ksmi.h: cannot read the members of `{where}`")
    return type(struct_class_name(cname), (C.Structure,), {"_fields_": fields, "__doc__": f"{cname} (include/ksmi.h)"})


def _function(decl, abi):
    where = " ".join(decl.split())
    m = re.fullmatch(r"([\w\s*]+?)(\w+)\s*\((.*)\)", decl.strip(), re.S)
    if not m or "(" in m[3] or ")" in m[3]:
        raise KsmiError(f"ksmi.h: not a plain function declaration: `{where}`")
    base, ptr, name, n = _declarator(m[1], abi, where)
    if name is not None or n is not None or base in abi.structs or (base in _POINTEES[1:] and not ptr):
        raise KsmiError(f"ksmi.h: cannot read the return type of `{where}`")
    res = (C.c_char_p if base == "char" else C.c_void_p) if ptr else None if base == "void" else SCALARS[base][0]
    args, names = [], []
    for piece in ([] if m[3].strip() in ("", "void") else m[3].split(",")):
        base, ptr, name, n = _declarator(piece, abi, where)
        if ptr or n is not None:
            args.append(C.c_void_p)
        elif base in SCALARS and SCALARS[base][1]:
            args.append(SCALARS[base][0])
        else:
            raise KsmiError(f"ksmi.h: a `{base}` parameter by value in `{where}`")
        names.append(name)
    return m[2], (res, args), names


_TOP = re.compile(r"\s*(?:typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;|([^;{}]+);)")


def parse(text):
    """one pass over the text of a header in the style of include/ksmi.h -> Abi"""
    abi = Abi()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(KSMI_\w+)[ \t]+\(?[ \t]*(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*\)?[ \t]*$", text, re.M):
        abi.constants[name] = int(value, 0)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", text)
    pos = 0
    while True:
        m = _TOP.match(text, pos)
        if not m:
            break
        pos = m.end()
        if m[2]:
            abi.structs[m[2]] = _struct(m[2], m[1], abi)
        else:
            name, sig, names = _function(m[3], abi)
            abi.signatures[name], abi.params[name] = sig, names
    if text[pos:].split() != ["}"] * wrapped:
        raise KsmiError(f"ksmi.h: cannot read the declaration at `{' '.join(text[pos:].split())[:120]}`")
    return abi
