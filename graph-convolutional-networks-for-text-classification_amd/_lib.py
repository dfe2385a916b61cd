"""ctypes binding of libgcnk.so (the C-ABI declared in include/gcnk.h and its family headers).

The headers are the only statement of the ABI: every entry point's signature,
every struct and every ``GCNK_*`` constant is read from them when this module
is imported (``read_headers``), so a new entry point is declared in its
family's header, or in a new header that gcnk.h includes, implemented, and
bound.  What the reader cannot take whole it refuses.

The shared library is built in-tree by ``__graft_entry__.build()`` (or
``make -C <package>/csrc``).  There is no fallback: if the library is missing
or fails to load, every op raises ``RuntimeError`` — the hot path never
silently runs anywhere but the HIP kernels.
"""
import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(_HERE, "libgcnk.so")
VARIANT_DIR = os.path.join(os.path.dirname(_HERE), "_variants")


def _resolve_lib():
    """The in-tree library, unless GCNK_LIB names an experiment variant built by
    `make -C <pkg>/csrc variant` (it must live in <repo>/_variants/; anything
    else is refused, so a stale export cannot swap in a foreign binary).  A
    variant is announced on stderr; tests/conftest.py refuses to run on one."""
    want = os.environ.get("GCNK_LIB")
    if not want:
        return PRODUCT_LIB
    path = os.path.realpath(want)
    if os.path.dirname(path) != os.path.realpath(VARIANT_DIR):
        raise RuntimeError(f"GCNK_LIB={want}: only experiment variants in {VARIANT_DIR} may replace {PRODUCT_LIB}")
    import sys
    print(f"[gcnk] loading experiment variant {path} (not the product library)", file=sys.stderr)
    return path


LIB_PATH = _resolve_lib()

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gcnk.h")

# ---- The binding is read from include/gcnk.h and the headers it includes, once, at import: they alone state the ABI.
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = ("void", "char", "uint8_t")   # what a pointer may point to besides a scalar and a struct
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+GCNK_(\w+)[ \t]+(\S.*?)[ \t]*$", re.M)   # (not function-like)
_STRUCT = re.compile(r"typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;\s*")
_FUNCTION = re.compile(r"([\w\s*]+?)\b(gcnk_\w+)\s*\(([^()]*)\)\s*;\s*")
_DECLARATOR = re.compile(r"(.*?[\s*])((?:\w+(?:\[\d+\])?\s*,\s*)*\w+(?:\[\d+\])?)", re.S)
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"(gcnk_\w+\.h)"', re.M)   # a family header, beside the one naming it


def _ctype(spelling, structs, decl, header):
    """The ctypes class of a C type as the header spells it: a pointer is c_void_p (``const char*``: c_char_p), a
    scalar its ctypes namesake, an earlier struct that struct.  ``decl``, ``header``: for the error."""
    words = spelling.replace("*", " * ").split()
    base = [w for w in words if w not in ("const", "*")]
    if len(base) != 1 or not (base[0] in _SCALARS or base[0] in structs or ("*" in words and base[0] in _POINTEES)):
        raise RuntimeError(f"{header}: unknown type '{' '.join(spelling.split())}' in '{decl}'")
    if "*" in words:
        return ctypes.c_char_p if base[0] == "char" and "const" in words else ctypes.c_void_p
    return _SCALARS.get(base[0]) or structs[base[0]]


def _declared(decl, structs, member, header):
    """[(name, ctypes class)] of a struct's member declaration (``T a, b``, ``T a[16]``) or of a function's parameter
    (one name, no array)."""
    decl = " ".join(decl.split())
    m = _DECLARATOR.fullmatch(decl)
    if not m or ("*" in m.group(1) and "," in m.group(2)) or ("[" in m.group(2) and not member):
        raise RuntimeError(f"{header}: cannot read the declaration '{decl}'")
    ctype = _ctype(m.group(1), structs, decl, header)
    names = [d.strip().rstrip("]").partition("[") for d in m.group(2).split(",")]
    return [(name, ctype * int(dim) if dim else ctype) for name, _, dim in names]


def parse_header(text, header="gcnk.h"):
    """(signatures, structs, constants) of a header in include/gcnk.h's form: {entry point: (restype, [argtypes])},
    {typedef'd struct: its ctypes.Structure} and {NAME: value} for every ``#define GCNK_<NAME> <integer>``.  Besides
    comments and preprocessor lines the text is one ``extern "C" { ... }`` of function declarations and struct
    typedefs; anything else raises RuntimeError naming ``header`` and it, because an entry point left unbound would
    be called with ctypes' default conversions (a pointer passed as a 32-bit int)."""
    text = _COMMENT.sub(" ", text)
    constants = {}
    for name, value in _DEFINE.findall(text):
        try:
            constants[name] = int(value[1:-1] if value[0] + value[-1] == "()" else value, 0)
        except ValueError:   # (an expression, or another macro's name)
            raise RuntimeError(f"{header}: GCNK_{name} is defined as '{value}', not as an integer") from None
    code = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    block = re.fullmatch(r'\s*extern\s+"C"\s*\{\s*(.*)\}\s*', code, re.S)
    if not block:
        raise RuntimeError(f'{header}: expected one extern "C" {{ ... }} block and nothing outside it')
    body, pos, signatures, structs = block.group(1), 0, {}, {}
    while pos < len(body):
        s = _STRUCT.match(body, pos)
        f = None if s else _FUNCTION.match(body, pos)
        if s:
            fields = [fld for d in s.group(1).split(";") if d.strip() for fld in _declared(d, structs, True, header)]
            structs[s.group(2)] = type(s.group(2), (ctypes.Structure,), {"_fields_": fields})
        elif f:
            params = [] if f.group(3).strip() == "void" else f.group(3).split(",")
            signatures[f.group(2)] = (_ctype(f.group(1), structs, f.group(2), header),
                                      [_declared(p, structs, False, header)[0][1] for p in params])
        else:
            stmt = " ".join(body[pos:body.find(";", pos) + 1 or None].split())
            raise RuntimeError(f"{header}: neither a function declaration nor a struct typedef: '{stmt[:200]}'")
        pos = (s or f).end()   # (each pattern takes the white space behind its statement)
    return signatures, structs, constants


def _header_text(path):
    if not os.path.exists(path):
        raise RuntimeError(f"header not found at {path}: libgcnk.so is bound from its source tree's include/ alone")
    with open(path) as f:
        return f.read()


def read_header(path=HEADER_PATH):
    return parse_header(_header_text(path), os.path.basename(path))


def read_headers(path=HEADER_PATH):
    """The header at ``path`` and then every ``#include "gcnk_*.h"`` it names, beside it and in the order named, as
    one ABI -> (paths, {entry point: its header's basename}, signatures, structs, constants).  An entry point, struct
    or constant that two headers declare raises RuntimeError naming both."""
    names = _INCLUDE.findall(_COMMENT.sub(" ", _header_text(path)))
    paths = [path] + [os.path.join(os.path.dirname(path), name) for name in names]
    where, merged = {}, ({}, {}, {})   # C name -> header; signatures, structs, constants
    for p in paths:
        for into, part, prefix in zip(merged, read_header(p), ("", "", "GCNK_")):
            for key, value in part.items():
                if prefix + key in where:
                    raise RuntimeError(f"{os.path.basename(p)}: {prefix}{key} is declared in {where[prefix + key]} too")
                where[prefix + key], into[key] = os.path.basename(p), value
    return (paths, {name: where[name] for name in merged[0]}, *merged)


# header paths, gcnk.h's first; entry point -> header, -> (restype, argtypes); struct -> class; GCNK_<NAME> -> value
HEADERS, DECLARED_IN, SIGNATURES, STRUCTS, CONSTANTS = read_headers()
if set(CONSTANTS) & set(globals()):
    raise RuntimeError(f"GCNK_{sorted(set(CONSTANTS) & set(globals()))[0]} would replace a name of {__name__}")
globals().update(CONSTANTS)   # GCNK_OK is _lib.OK, GCNK_EPI_BIAS_RELU _lib.EPI_BIAS_RELU, ..., GCNK_ABI_VERSION too
AdamTensor, EpochState = STRUCTS["gcnk_adam_tensor"], STRUCTS["gcnk_epoch_state"]
KeepTensor, KeepState = STRUCTS["gcnk_keep_tensor"], STRUCTS["gcnk_keep_state"]


class LaunchTables:
    """The host tensor tables of a multi-tensor entry point (gcnk_adam_f32,
    gcnk_keep_best_f32): rows of the ctypes ``struct`` (a tensor's pointers,
    then ``numel``), at most ``per_call`` of them a launch."""

    def __init__(self, struct, per_call):
        self.struct, self.per_call, self._cache = struct, per_call, {}   # launch -> (pointers, struct array)
        self.clear = self._cache.clear

    def launches(self, ptrs, numels, first=0, last=True):
        """[(table, rows, hold)] for the tensors with pointer tuples ``ptrs``, the
        launches numbered from ``first``; a table is rebuilt only when one of
        its pointers changed.  ``hold`` (the entry point's HOLD flag is due): on
        every launch but the last, and on that too unless ``last``."""
        out = []
        for i in range(0, len(ptrs), self.per_call):
            key, li = tuple(ptrs[i:i + self.per_call]), first + len(out)
            if self._cache.get(li, (None,))[0] != key:
                self._cache[li] = (key, (self.struct * len(key))(*[(*p, n) for p, n in zip(key, numels[i:])]))
            out.append((self._cache[li][1], len(key), not last or i + self.per_call < len(ptrs)))
        return out


def epoch_row_words(nclass):
    """gcnk.h GCNK_EPOCH_ROW_WORDS: train_loss | val_loss | TP | FP | FN | correct"""
    return 3 * nclass + 3


# added within ABI 13 (gc2 from the hub factor, the backward's and the factored gc1's route reports, and every family
# header's entry points): absent from variants of an older tree
NEWER_THAN_SOME_VARIANTS = ("gcnk_hubfactor_gc2_f32", "gcnk_factor_diag_f32", "gcnk_gcn_bwd2_route",
                            "gcnk_hubfactor_gc1_route", "gcnk_score_docs_f32", "gcnk_score_docs_route",
                            "gcnk_spmm_route", "gcnk_dense_gc1_route",
                            *(name for name, header in DECLARED_IN.items() if header != "gcnk.h"))

_lock = threading.Lock()
_lib = None


class GcnkError(RuntimeError):
    """Raised when a libgcnk entry point returns a non-zero code."""


def load():
    """Load libgcnk.so once and bind every declared symbol; raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libgcnk.so not found at {LIB_PATH}: build it with __graft_entry__.build() "
                "or `make -C <package>/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                # an experiment variant built from an older csrc (an A/B's parent library)
                # may lack the newest entry points: their callers test for them
                if LIB_PATH == PRODUCT_LIB or name not in NEWER_THAN_SOME_VARIANTS:
                    raise RuntimeError(f"{LIB_PATH} does not export {name}")
                continue
            fn.restype = res
            fn.argtypes = args
        v = lib.gcnk_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"libgcnk ABI version {v} != expected {ABI_VERSION}")
        _lib = lib
        return lib


def stream(device):
    """The current stream of ``device`` as the ``void* stream`` every launch takes."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc, what):
    if rc != OK:
        msg = load().gcnk_last_error().decode(errors="replace")
        kind = {EARG: "bad argument", EUNSUP: "unsupported", EHIP: "HIP error"}.get(rc, "error")
        raise GcnkError(f"{what} failed ({kind}, rc={rc}): {msg} [{LIB_PATH}]")
