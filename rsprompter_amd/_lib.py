"""ctypes binding of librsp_hip.so, derived from include/rsp_hip.h at import.

The header is the only declaration of the C ABI.  `parse_header` reads it once and yields
  PROTOTYPES   name -> (restype, argtypes) of every entry point,
  the `Rsp*` ctypes.Structure classes (module attributes, e.g. `_lib.RspGemmDesc`),
  CONST        name -> value of every object-like integer `#define` (status codes, flags, limits);
a new entry point, descriptor field or limit needs no line here.

The product path has NO fallback: if the header or the library is missing, or a call returns a non-zero status, a
RuntimeError is raised.  Nothing here imports `oracle/`.
"""
import ctypes
import os
import re

from .build import HEADER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librsp_hip.so")

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_int64 = ctypes.c_int64
c_float = ctypes.c_float
c_double = ctypes.c_double

# by-value C types; a pointer is POINTER(struct) to a struct declared above it, c_char_p as a `const char*` result and
# c_void_p otherwise (from_param takes device addresses, ctypes arrays of host values, byref() results and None)
SCALARS = {"int": c_int, "int32_t": c_int, "int64_t": c_int64, "float": c_float, "double": c_double,
           "rsp_stream_t": c_void_p}
_INT = r"(0[xX][0-9a-fA-F]+|\d+)[uUlL]*"
_DECL = r"(?:const\s)?(\w+)\s*(\**)\s*(\w*)\s*(\[\s*\d*\s*\])?"      # one parameter or result: base, stars, name, array


def parse_header(text):
    """(structs, prototypes, constants) of a header in the C subset that include/rsp_hip.h keeps to:
      /* */ comments (a `//` outside a string is an error);
      `#define NAME <integers, RSP_* macros defined above it, unary minus, ( ) << * / - +, suffixes u / L / LL>` (/ of
        non-negative values); function-like macros, the include guard and every other directive are passed over;
      `typedef struct [Name] { ... } Name;` of scalars, pointers, arrays `T x[4]` and earlier structs by value, several
        declarators (`int32_t M, N, K;`) or declarations on a line;
      prototypes of `rsp_*` functions over any number of lines, `(void)`, array parameters;
      `typedef void* rsp_stream_t;` and the `extern "C" { }` pair.
    Anything else raises RuntimeError with the text in question: nothing is skipped."""
    def fail(what, at):
        raise RuntimeError(f"rsp_hip.h: {what}: {' '.join(at.split())[:200]!r}")

    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"//.*", re.sub(r'"[^"\n]*"', '""', code))
    if m:
        fail("`//` comment (only /* */ is read)", m.group(0))
    code = code.replace("\\\n", " ")

    const = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(?!\()[ \t]+(\S.*)$", code, re.M):
        value = re.sub(r"\bRSP_\w+", lambda k: f"({const[k.group(0)]})" if k.group(0) in const else k.group(0), m.group(2))
        if not re.fullmatch(rf"(?:{_INT}|<<|[-+*/()\s])+", value):
            fail("macro value is not an integer expression", m.group(0))
        try:
            const[m.group(1)] = eval(re.sub(_INT, lambda k: str(int(k.group(1), 0)), value).replace("/", "//"),
                                     {"__builtins__": {}})
        except (SyntaxError, ValueError, ZeroDivisionError):
            fail("macro value does not evaluate", m.group(0))
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M)
    calls = re.findall(r"(rsp_[a-z0-9_]+)\s*\(", code)

    structs = {}

    def ctype(base, pointer, at):
        if pointer:
            return ctypes.POINTER(structs[base]) if base in structs else c_void_p
        if base in SCALARS or base in structs:
            return SCALARS.get(base) or structs[base]
        fail(f"type `{base}` by value", at)

    def take_struct(m):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(2).split(";"))):
            d = re.fullmatch(r"(?:const\s)?(\w+)\b\s*(.+)", decl) or fail("struct field", decl)
            for item in d.group(2).split(","):
                f = re.fullmatch(r"(\**)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?", item.strip()) or fail("struct field", decl)
                t = ctype(d.group(1), f.group(1), decl)
                fields.append((f.group(2), t * int(f.group(3)) if f.group(3) else t))
        structs[m.group(3)] = type(m.group(3), (ctypes.Structure,), {"_fields_": fields})
        return ""

    code = re.sub(r"typedef\s+struct\s*(\w*)\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, code, flags=re.S)

    protos = {}

    def take_proto(m):
        r = re.fullmatch(_DECL, m.group(1).strip())
        if not r or r.group(3) or r.group(4):
            fail("result type", m.group(0))
        res = (ctypes.c_char_p if r.group(1) == "char" else c_void_p) if r.group(2) else ctype(r.group(1), "", m.group(0))
        args = []
        for par in (p.strip() for p in m.group(3).split(",")) if m.group(3).strip() != "void" else ():
            a = re.fullmatch(_DECL, par) or fail("parameter", f"{par} in {m.group(2)}")
            args.append(ctype(a.group(1), a.group(2) or a.group(4), f"{par} in {m.group(2)}"))
        protos[m.group(2)] = (res, args)
        return ""

    code = re.sub(r"((?:const\s+)?\w+[\s*]+)\b(rsp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", take_proto, code)
    if len(calls) != len(protos):
        fail(f"{len(calls)} `rsp_*(` but {len(protos)} prototypes parsed; missed or declared twice",
             " ".join(sorted(n for n in set(calls) if n not in protos or calls.count(n) > 1)))
    rest = re.sub(r'typedef\s+void\s*\*\s*rsp_stream_t\s*;|extern\s+"C"\s*\{|\}', "", code)
    if rest.strip():
        fail("not parsed", rest)
    return structs, protos, const


if not os.path.exists(HEADER):
    raise RuntimeError(f"{os.path.normpath(HEADER)} is missing: it is the declaration of the C ABI that this module binds. "
                       "There is no fallback path.")
with open(HEADER) as _f:
    STRUCTS, PROTOTYPES, CONST = parse_header(_f.read())
globals().update(STRUCTS)       # RspGemmDesc, RspAttnDesc, ...: one ctypes.Structure per `typedef struct` of the header

_lib = None


def load():
    """Load librsp_hip.so (after torch, so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- makes libamdhip64.so.7 resident first
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m rsprompter_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no fallback path.")
    # a library left over from older sources would be loaded silently and its struct layouts (RspGemmDesc, ...) would
    # no longer match the header: compare the source digest recorded at build time; rebuild when hipcc is here, else fail
    from . import build as _build
    try:
        stale = (not os.path.exists(_build.STAMP)) or open(_build.STAMP).read().strip() != _build._digest()
    except OSError:
        stale = True
    if stale:
        if os.path.exists(_build.HIPCC) and os.access(os.path.dirname(LIB_PATH), os.W_OK):
            _build.build(verbose=False)
        else:
            raise RuntimeError(f"{LIB_PATH} was built from different sources than the ones in this tree "
                               "(digest mismatch) and hipcc is not available to rebuild it")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        raise RuntimeError(f"librsp_hip: {what} failed with status {status}")
