"""The C ABI as ctypes sees it, read from include/stem_*.h: the headers are its single statement.

A reader for those three headers as they are written, not a C front end, and a strict one: a type outside the map below, an
aggregate by value, an array parameter or a declaration it cannot read to the end raises HeaderError with the function's name
and the offending text.  Nothing defaults to int.  Standard library only (tools load this file by path, without the package).
"""
import ctypes as C
import functools
import re

_SCALAR = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "long": C.c_long, "unsigned long": C.c_ulong,
           "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
_POINTEE = set(_SCALAR) | {"void", "char", "unsigned char", "uint8_t"}
_DECLARATOR = re.compile(r"(.*[\s*])(\w+)", re.S)       # type as written, then the name


class HeaderError(ValueError):
    pass


def _ctype(text, who, structs, fnptrs):
    """ctypes class of a C type as written (without the declared name); `who` names the declaration in errors"""
    base = " ".join(w for w in text.replace("*", " ").split() if w != "const")
    if "*" in text:
        if base not in _POINTEE and base not in structs:
            raise HeaderError(f"{who}: pointer to a type outside the map in {text.strip()!r}")
        return C.c_char_p if base == "char" and text.count("*") == 1 and "const" in text.replace("*", " ").split() else C.c_void_p
    if base in _SCALAR:
        return _SCALAR[base]
    if base in fnptrs:
        return C.c_void_p
    if base in structs or base.split()[:1] in (["struct"], ["union"]):
        raise HeaderError(f"{who}: aggregate passed by value: {text.strip()!r}")
    raise HeaderError(f"{who}: type outside the map: {text.strip()!r}")


def _declarator(text, who):
    m = _DECLARATOR.fullmatch(text.strip())
    if "[" in text:
        raise HeaderError(f"{who}: array declarator {text.strip()!r}")
    if not m:
        raise HeaderError(f"{who}: cannot read {text.strip()!r}")
    return m.group(1), m.group(2)


_STRUCT = r"typedef\s+struct\s*\{([^}]*)\}\s*(\w+)\s*;"
_FNPTR = r"typedef\s+[\w\s*]+?\(\s*\*\s*(\w+)\s*\)\s*\([^()]*\)\s*;"


@functools.lru_cache(maxsize=None)            # stem_hip.h is asked for its prototypes and for its structs
def _parse(header):
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(header).read(), flags=re.S)
    src = re.sub(r"^[ \t]*#.*$", "", src.replace("\\\n", " "), flags=re.M)        # preprocessor lines: values are not read
    bodies, fnptrs = re.findall(_STRUCT, src), set(re.findall(_FNPTR, src))
    src = re.sub(_STRUCT + "|" + _FNPTR + r"|enum\s*\{[^}]*\}\s*;", "", src)
    src = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", src, flags=re.S)
    structs = {}
    for body, name in bodies:
        fields = structs[name] = []
        for line in filter(str.strip, body.split(";")):                           # `int K, C, R;`: one type, several plain names
            first, *more = line.split(",")
            ty, field = _declarator(first, name)
            if more and ("*" in ty or not all(re.fullmatch(r"\s*\w+\s*", f) for f in more)):
                raise HeaderError(f"{name}: cannot read {line.strip()!r}")
            cty = _ctype(ty, f"{name}.{field}", structs, fnptrs)
            fields += [(f.strip(), cty) for f in [field] + more]
    protos = {}
    for stmt in filter(str.strip, src.split(";")):
        m = re.fullmatch(r"\s*(.*[\s*])(stem_\w+)\s*\(([^()]*)\)\s*", stmt, flags=re.S)
        if not m:
            raise HeaderError(f"{header}: cannot read the declaration {' '.join(stmt.split())!r}")
        ret, name, params = m.groups()
        args = [] if params.strip() == "void" else [_ctype(_declarator(p, name)[0], name, structs, fnptrs) for p in params.split(",")]
        protos[name] = (None if ret.strip() == "void" else _ctype(ret, name, structs, fnptrs), args)
    return protos, structs


def prototypes(header):
    """{name: (restype, [argtypes])} of every stem_* function the header declares"""
    return _parse(header)[0]


def structs(header):
    """{typedef name: [(field, ctype), ...]} of the header's `typedef struct { ... } name;` blocks"""
    return _parse(header)[1]
