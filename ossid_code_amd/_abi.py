"""Reader of include/ossid_hip.h: the header is the one statement of the C ABI, and the ctypes binding (_lib.py) is built
from what parse() returns. The header keeps to a form a few regular expressions can read -- integer #defines, flat
`typedef struct N { ... } N;` blocks, plain prototypes -- and the reader is strict about it: anything else raises ValueError
naming the text, so a declaration is either bound exactly or refuses to import."""
import ctypes as C
import functools
import re

# C scalar -> ctypes. Every pointer is c_void_p (it takes byref(), arrays, pointer instances, None and plain addresses),
# except char*, which is c_char_p.
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "long long": C.c_longlong, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_POINTEES = ("void", "char")        # what may be pointed to besides SCALARS and the header's own structs


def _split(ctext):
    words = [w for w in re.findall(r"\w+|\*|[^\w\s*]+", ctext) if w != "const"]
    return " ".join(w for w in words if w != "*"), words.count("*")


@functools.lru_cache(maxsize=None)
def ctype(ctext):
    """The ctypes type of a C type as parse() spells it (None for void)."""
    base, stars = _split(ctext)
    if stars:
        return C.c_char_p if (base, stars) == ("char", 1) else C.c_void_p
    return None if base == "void" else SCALARS[base]


def parse(text):
    """(constants, structs, prototypes) of a header's text:
    {OSSID_NAME: int}, {struct: [(field, C type, array length or 0)]} in declaration order, {name: (C type, [C types])}."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, structs, protos, checked, code, in_cxx = {}, {}, {}, {}, [], False
    for line in text.split("\n"):
        s = line.strip()
        if not s.startswith("#"):
            if not in_cxx:           # the extern "C" braces live between #ifdef __cplusplus and #endif
                code.append(line)
            continue
        m = re.fullmatch(r"#\s*define\s+(OSSID_\w+)(?:\s+(-?\d+|\(\s*-?\d+\s*\)))?", s)
        if m and m.group(2):
            consts[m.group(1)] = int(m.group(2).strip("() "))
        elif s.split() == ["#ifdef", "__cplusplus"]:
            in_cxx = True
        elif re.fullmatch(r"#\s*endif", s):
            in_cxx = False
        elif not (m or re.fullmatch(r"#\s*(ifndef\s+\w+|include\s*<[\w./]+>)", s)):     # m: the include guard's #define
            raise ValueError("unreadable preprocessor line: %r" % s)

    def typ(ctext, what, void_ok=False):
        if (ctext, void_ok) not in checked:      # ~1 400 parameters and fields, ~40 spellings
            base, stars = _split(ctext)
            if not (base in SCALARS or stars and (base in _POINTEES or base in structs) or void_ok and base == "void"):
                raise ValueError("unknown type %r in %r" % (ctext.strip(), what))
            checked[ctext, void_ok] = re.sub(r"\s*\*", "*", " ".join(ctext.split()))
        return checked[ctext, void_ok]

    def struct(m):
        name, fields = m.group(1), []
        if m.group(3) != name or name in structs:
            raise ValueError("struct %s: typedef name %s" % (name, m.group(3)))
        for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
            first, *more = (d.strip() for d in decl.split(","))
            m1 = re.fullmatch(r"(.*[\s*])(\w+(?:\[\w+\])?)", first)
            if not m1 or not all(re.fullmatch(r"\w+(\[\w+\])?", d) for d in more):
                raise ValueError("struct %s: unreadable field %r" % (name, decl))
            t = typ(m1.group(1), decl)
            for d in [m1.group(2)] + more:
                field, _, dim = d.rstrip("]").partition("[")
                if dim and not dim.isdigit() and dim not in consts:
                    raise ValueError("struct %s: array length %r of %r is not defined" % (name, dim, decl))
                fields.append((field, t, (int(dim) if dim.isdigit() else consts[dim]) if dim else 0))
        structs[name] = fields
        return ";"

    rest = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, "\n".join(code))
    *decls, tail = (d.strip() for d in rest.split(";"))
    if tail:
        raise ValueError("declaration without its ';': %r" % tail)
    for decl in filter(None, decls):
        m = re.fullmatch(r"(.*[\s*])(\w+)\s*\(([^()]*)\)", decl, flags=re.S)
        if not m or m.group(2) in protos:
            raise ValueError("unreadable declaration: %r" % decl)
        params = [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")]
        named = [re.fullmatch(r"(.*[\s*])\w+", p, flags=re.S) for p in params]
        if not all(named):
            raise ValueError("%s: unreadable parameter in (%s)" % (m.group(2), " ".join(m.group(3).split())))
        protos[m.group(2)] = (typ(m.group(1), decl, void_ok=True), [typ(p.group(1), decl) for p in named])
    return consts, structs, protos
