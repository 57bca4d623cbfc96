"""ctypes binding of libnopesac_hip.so, read from the header that declares its C ABI (include/nopesac_hip.h): prototypes, constants
and structs are stated there once, and every kernel file is compiled against the same text.

There is NO fallback: if the shared library is missing or a symbol cannot be resolved, importing
the ops raises.  Build it with `python -m nopesac_amd.build` (or `__graft_entry__.build()`).
"""
from __future__ import annotations

import ctypes
import os
import re
from collections import namedtuple
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_void_p
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnopesac_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "nopesac_hip.h")


class HeaderError(RuntimeError):
    """include/nopesac_hip.h holds something the reader below does not know.  The reader never guesses a type."""


Header = namedtuple("Header", "signatures restypes constants structs status")
_SCALARS = {"int": c_int, "int64_t": c_int64, "long long": c_int64, "float": c_float, "double": c_double}
_RETURNS = {"int": c_int, "int64_t": c_int64, "long long": c_int64, "const char*": c_char_p, "void*": c_void_p, "void": None,
            "nps_status": c_int}      # nps_status: the header's `typedef int`, 0 = enqueued, < 0 = NPS_E_*, > 0 = hipError_t


def _norm(ctype: str) -> str:
    return re.sub(r"\s*\*\s*", "*", " ".join(ctype.split()))


def _declarator(text: str, where: str):
    """'const float* bias' -> ('const float*', 'bias'): one declarator, its name last."""
    m = re.fullmatch(r"(.*[\s*])(\w+)", text.strip(), re.S)
    if not m:
        raise HeaderError(f"{where}: cannot split {text.strip()!r} into a type and a name")
    return _norm(m[1]), m[2]


def _ctype(ctype: str, where: str):
    """ctypes class of a parameter or field of type `ctype`.  Every pointer travels as c_void_p (the wrappers pass tensor.data_ptr()),
    except the tape handle's out-parameter."""
    if ctype in _SCALARS:
        return _SCALARS[ctype]
    if ctype == "void**":
        return ctypes.POINTER(c_void_p)
    if ctype.endswith("*"):
        return c_void_p
    raise HeaderError(f"{where}: unknown type {ctype!r}")


def _constant(name: str, value: str, known: dict) -> int:
    """An integer #define: a literal, a parenthesised negative, or a sum of products of literals and constants defined above it."""
    value = value.strip()
    terms = value[1:-1] if value.startswith("(") and value.endswith(")") else value
    total = 0
    for term in terms.split("+"):
        product = 1
        for factor in (f.strip() for f in term.split("*")):
            if factor in known:
                product *= known[factor]
            elif re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)", factor):
                product *= int(factor, 0)
            else:
                raise HeaderError(f"{name}: cannot evaluate {value!r}")
        total += product
    return total


def _struct(name: str, body: str, constants: dict, structs: dict):
    """ctypes.Structure of a `typedef struct` body: `type a, b, c;` field lists and arrays sized by a constant."""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")
        array = re.fullmatch(r"(.*)\[\s*(\w+)\s*\]", first, re.S)
        ctype, field = _declarator(array[1] if array else first, name)
        cls = structs[ctype] if ctype in structs else _ctype(ctype, f"{name}.{field}")
        if array:
            if array[2] not in constants:
                raise HeaderError(f"{name}.{field}: unknown array size {array[2]!r}")
            cls = cls * constants[array[2]]
        if more and (array or "*" in ctype or not all(re.fullmatch(r"\w+", n.strip()) for n in more)):
            raise HeaderError(f"{name}: cannot read the field list {decl!r}")
        fields += [(f, cls) for f in [field] + [n.strip() for n in more]]
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def read_header(text: str) -> Header:
    """The C ABI as the text of include/nopesac_hip.h states it: argtypes and restype of every `ret nopesac_*(args);` prototype, the
    set of those declared `nps_status` (their result is a status, every other result a value), the integer NPS_* / NOPESAC_*
    constants, the `typedef struct`s as ctypes.Structure classes.  Not a C parser: it reads the narrow grammar this header keeps, and
    raises HeaderError, naming the symbol, on anything else."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants, structs, signatures, restypes, status = {}, {}, {}, {}, set()
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+((?:NPS|NOPESAC)_\w+)[ \t]+(\S.*)$", text, flags=re.M):   # (a guard has no value)
        constants[name] = _constant(name, value, constants)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    block = re.search(r'extern\s+"C"\s*\{(.*)\}', text, flags=re.S)
    text = block[1] if block else text

    def take_struct(m):
        if m[1] != m[3] or m[1] in structs:
            raise HeaderError(f"{m[3]}: struct tag and typedef name differ, or defined twice")
        structs[m[1]] = _struct(m[1], m[2], constants, structs)
        return ""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, text, flags=re.S)
    text = re.sub(r"typedef\s+int\s+nps_status\s*;", "", text)
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.+?)\b(nopesac_\w+)\s*\((.*)\)", stmt, re.S)
        if not m:
            raise HeaderError(f"cannot read the declaration {' '.join(stmt.split())[:80]!r}")
        ret, name, params = _norm(m[1]), m[2], m[3].strip()
        if ret not in _RETURNS or name in signatures:
            raise HeaderError(f"{name}: unknown return type {ret!r}, or declared twice")
        restypes[name] = _RETURNS[ret]
        if ret == "nps_status":
            status.add(name)
        signatures[name] = [] if params == "void" else [_ctype(_declarator(p, name)[0], name) for p in params.split(",")]
    return Header(signatures, restypes, constants, structs, frozenset(status))


def load_header(path: str = HEADER_PATH) -> Header:
    try:
        with open(path) as f:
            return read_header(f.read())
    except OSError as e:
        raise RuntimeError(f"{path} not readable ({e.strerror}): nopesac_amd binds libnopesac_hip.so from its header") from e


# Read at import: the wrappers bind their constants (nopesac_amd.ops, nopesac_amd.jpeg) when they are imported, before any load().
_HEADER = load_header()
SIGNATURES, RESTYPES = _HEADER.signatures, _HEADER.restypes     # name -> argtypes, name -> restype
STATUS = _HEADER.status                                         # the entry points whose int result is a status, not a value
H = SimpleNamespace(**_HEADER.constants)                        # H.NPS_ACT_RELU, H.NOPESAC_JPEG_IMG_I32, ...
MlpLayer, MlpChain = _HEADER.structs["nopesac_mlp_layer"], _HEADER.structs["nopesac_mlp_chain"]
PlaneCriterionArgs = _HEADER.structs["nopesac_plane_criterion"]
OptSegment, OptSource, OptUnit = (_HEADER.structs["nopesac_opt_" + n] for n in ("segment", "source", "unit"))
OptStepArgs = _HEADER.structs["nopesac_opt_step_args"]
MLP_MAX_IN, MLP_MAX_WIDTH, MLP_MAX_LAYERS = H.NOPESAC_MLP_MAX_IN, H.NOPESAC_MLP_MAX_WIDTH, H.NOPESAC_MLP_MAX_LAYERS

_lib = None


def declared_symbols() -> list:
    """Every entry point include/nopesac_hip.h declares."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nopesac_\w+)\s*\(", text)))


def load():
    """Load (once) and type the library.  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    lib_path = os.environ.get("NOPESAC_AB_LIBRARY") or LIB_PATH           # A/B runs only: another BUILD of this library (e.g. last round's)
    if not os.path.exists(lib_path):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built.  Run `python -m nopesac_amd.build` "
            "(needs hipcc for gfx950).  nopesac_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64; whichever copy is loaded first serves the whole process.  Import torch first so
    # that this library (linked against the same SONAME) shares torch's runtime, streams and device context - loading the
    # system copy first leaves the kernels of this library without a device ("no ROCm-capable device is detected").
    import torch  # noqa: F401
    lib = ctypes.CDLL(lib_path)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    vars(C).update({name: _raising(getattr(lib, name)) if name in STATUS else getattr(lib, name) for name in SIGNATURES})
    _lib = lib
    return lib


class HipKernelError(RuntimeError):
    pass


def check(rc: int, name: str):
    if rc != 0:
        msg = load().nopesac_last_error()
        raise HipKernelError(f"{name} failed (rc={rc}): {msg.decode() if msg else ''}")


def _raising(fn):
    def call(*args):
        rc = fn(*args)
        if rc:
            check(rc, fn.__name__)
    return call


class _Checked:
    """The library as the wrappers call it: C.nopesac_x(...) raises HipKernelError when a status entry point (STATUS) does not return
    0, and is the raw function for an entry point that returns a value.  load() fills it once with every entry point, so a call costs
    one attribute read of this object; only the first read, before load(), comes through __getattr__.  The raw library (load()) is for
    the few callers that branch on a status themselves."""

    def __getattr__(self, name):
        load()
        try:
            return self.__dict__[name]
        except KeyError:
            raise AttributeError(f"include/nopesac_hip.h declares no entry point {name!r}") from None


C = _Checked()
