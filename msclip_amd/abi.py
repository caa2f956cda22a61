"""The C ABI as Python binds it, read from include/msclip_hip.h: the header is the only statement of it.  The extension headers
include/msclip_ext.h, msclip_ext2.h, msclip_ext3.h, msclip_ext4.h and msclip_ext5.h (declarations newer than that header's ABI version) are read by the same
rules, each under its own version macro.

The mapping rule, for prototype parameters and struct members alike:
    int -> c_int, float -> c_float, long long -> c_longlong;
    `T**` and `T* const*` -> POINTER(c_void_p);
    every other pointer -> c_void_p, struct pointers included (callers pass byref(desc), a ctypes array or an address);
    a return type is `int` -> c_int or `const char*` -> c_char_p.
A struct member whose name is a Python keyword gets a trailing underscore (`in` -> `in_`).

The reader knows the C subset that the header's comment block names and raises AbiError on anything else; it never guesses.
"""
import collections
import ctypes
import keyword
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msclip_hip.h")
VERSION_MACRO = "MSCLIP_ABI_VERSION"
# the extension header: declarations newer than msclip_hip.h's ABI version, versioned on their own until they are folded in
EXT_HEADER = os.path.join(os.path.dirname(HEADER), "msclip_ext.h")
EXT_VERSION_MACRO = "MSCLIP_EXT_ABI_VERSION"
# the second extension header (the row-scale entry points of stochastic depth): its prototypes point to structs of msclip_hip.h,
# so it is read with those names known (load(..., known=...))
EXT2_HEADER = os.path.join(os.path.dirname(HEADER), "msclip_ext2.h")
EXT2_VERSION_MACRO = "MSCLIP_EXT2_ABI_VERSION"
# the third extension header (the LAMB entry points and their table item), read like the second
EXT3_HEADER = os.path.join(os.path.dirname(HEADER), "msclip_ext3.h")
EXT3_VERSION_MACRO = "MSCLIP_EXT3_ABI_VERSION"
# the fourth extension header (the non-finite guard of the optimizer phase): its prototypes point to msclip_adamw_tensor of
# msclip_hip.h and to msclip_lamb_tensor of the third, so it is read with both headers' names known
EXT4_HEADER = os.path.join(os.path.dirname(HEADER), "msclip_ext4.h")
EXT4_VERSION_MACRO = "MSCLIP_EXT4_ABI_VERSION"
# the fifth extension header (linear probing: the classifier's row pass, its loss fold, the bf16 hi/lo split): scalars and plain
# pointers only, read like the first
EXT5_HEADER = os.path.join(os.path.dirname(HEADER), "msclip_ext5.h")
EXT5_VERSION_MACRO = "MSCLIP_EXT5_ABI_VERSION"

Abi = collections.namedtuple("Abi", "version structs protos")   # int, {C name: Structure subclass}, {name: (restype, [argtypes])}


class AbiError(ValueError):
    pass


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
_BASE = r"(?:const\s+)?(int|float|long long|void|char|msclip_\w+)\b"
_DECL = re.compile(_BASE + r"\s*(\*|\*\s*\*|\*\s*const\s*\*)?\s*([A-Za-z_]\w*)")
_PROTO = re.compile(r"(int|const\s+char\s*\*)\s*(msclip_\w+)\s*\((.*)\)", re.S)
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)(?:\s*\{([^{}]*)\}\s*|\s+)(\w+)")


def _declarator(text, known):
    """`const float* x` -> ("x", c_void_p).  `known`: the struct names declared so far."""
    m = _DECL.fullmatch(text.strip())
    if not m:
        raise AbiError(f"cannot read the declarator {text.strip()!r}")
    base, stars, name = m.groups()
    if base.startswith("msclip_") and base not in known:
        raise AbiError(f"unknown type {base!r} in {text.strip()!r}")
    if not stars:
        if base not in _SCALARS:
            raise AbiError(f"{base!r} by value in {text.strip()!r}")
        return name, _SCALARS[base]
    return name, ctypes.c_void_p if stars == "*" else ctypes.POINTER(ctypes.c_void_p)


def _members(body, known):
    fields = []
    for line in filter(None, (s.strip() for s in body.split(";"))):
        first, *rest = line.split(",")
        base = re.match(_BASE, first)                   # `const float *g, *b;`: the later declarators share the first one's type
        if not base:
            raise AbiError(f"cannot read the struct member {line!r}")
        for d in [first] + [base.group(0) + " " + r for r in rest]:
            name, ctype = _declarator(d, known)
            fields.append((name + "_" * keyword.iskeyword(name), ctype))
    return fields


def parse(text, version_macro=VERSION_MACRO, known=()):
    """Header text -> Abi; `version_macro`: the name of the header's `#define <name> <number>`; `known`: struct names that a
    header included by this one declares (they may be pointed to; they are not part of the result)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    version = re.findall(r"^[ \t]*#[ \t]*define[ \t]+" + re.escape(version_macro) + r"[ \t]+(\d+)[ \t]*$", text, flags=re.M)
    if len(version) != 1:
        raise AbiError(f"expected one '#define {version_macro} <number>', found {len(version)}")
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)      # extern "C" { ... }
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    structs, protos = {name: None for name in known}, {}
    for stmt in filter(None, (s.strip() for s in re.split(r";(?![^{}]*\})", text))):      # (a struct body's own `;` do not split)
        struct = _STRUCT.fullmatch(stmt)
        proto = _PROTO.fullmatch(stmt)
        if struct:
            tag, body, name = struct.groups()
            if tag != name or name in structs:
                raise AbiError(f"struct {tag!r} / typedef {name!r}: one name, declared once")
            structs[name] = None                        # opaque (`typedef struct T T;`): only ever pointed to
            if body is not None:
                mirror = {"_fields_": _members(body, structs), "__doc__": f"Mirror of struct {name}."}
                structs[name] = type(name, (ctypes.Structure,), mirror)
        elif proto:
            if proto.group(2) in protos:
                raise AbiError(f"{proto.group(2)} is declared twice")
            params = proto.group(3).strip()
            args = [] if params == "void" else [_declarator(p, structs)[1] for p in params.split(",")]
            protos[proto.group(2)] = (ctypes.c_int if proto.group(1) == "int" else ctypes.c_char_p, args)
        else:
            raise AbiError(f"cannot read the declaration {stmt[:80]!r}")
    return Abi(int(version[0]), {k: v for k, v in structs.items() if v}, protos)


def load(path=HEADER, version_macro=VERSION_MACRO, known=()):
    with open(path) as f:
        return parse(f.read(), version_macro, known)
