"""ctypes binding of libevoworld_hip.so, derived from include/evoworld_hip.h.

The header is the only description of the C ABI.  `Header` parses it once at import -- every ew_* prototype, the two argument
structs, the EW_* defines and the enum members -- and everything the binding needs comes from that parse: argtypes / restype of
every function (`bind`), the ctypes.Structure classes (GemmArgs, FfArgs), ABI_VERSION, the error codes and enum values (module
attributes under their header names).  A type without a mapping raises; nothing defaults to int.

The library is built in-tree by `make -C evoworld_amd/csrc` (or __graft_entry__.build()).  Loading fails
loudly -- there is no CPU / PyTorch fallback for the product path.
"""
import contextlib
import ctypes
import os
import re

import torch  # noqa: F401  MUST precede the CDLL below: torch bundles its own libamdhip64.so.7; loading ours first
#                     would pull /opt/rocm's copy and leave two HIP runtimes in the process ("no ROCm-capable device").

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EW_LIB_PATH") or os.path.join(_HERE, "libevoworld_hip.so")   # EW_LIB_PATH: another build of the same ABI (A/B tools)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "evoworld_hip.h")

_SCALARS = {"int": ctypes.c_int, "ew_status": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong,
            "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}


class EvoWorldHipError(RuntimeError):
    pass


def strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def _typed_name(decl):
    """'const void* a' -> ('const void*', 'a'): the C type normalised to single spaces with '*' attached to it"""
    m = re.fullmatch(r"(.*[\s*])(\w+)", decl.strip(), flags=re.S)
    if not m:
        raise EvoWorldHipError(f"evoworld_hip.h: cannot read the declaration '{decl.strip()}'")
    return re.sub(r"\s*\*\s*", "*", " ".join(m.group(1).split())), m.group(2)


class Header:
    """The parse of evoworld_hip.h.  As C text: `functions` {name: (return type, [parameter types])} and `struct_fields`
    {struct: [(type, field)]}; `constants` {EW_*: int} (defines and enum members); as ctypes: `structs` {struct: Structure class}
    and `signatures` {name: (restype, argtypes)}."""

    def __init__(self, text):
        text = strip_comments(text)
        self.constants = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(EW_\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$", text, flags=re.M)}
        for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
            for member in filter(None, (s.strip() for s in body.split(","))):
                m = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", member)
                if not m:
                    raise EvoWorldHipError(f"evoworld_hip.h: enum member '{member}' has no explicit integer value")
                self.constants[m.group(1)] = int(m.group(2))
        text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
        self.struct_fields, self.structs = {}, {}
        for name, body, alias in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
            if alias != name:
                raise EvoWorldHipError(f"evoworld_hip.h: struct {name} is typedef'd to another name ({alias})")
            fields = []
            for decl in filter(None, (s.strip() for s in body.split(";"))):
                first, *more = decl.split(",")
                ctype, field = _typed_name(first)
                if more and "*" in ctype or not all(re.fullmatch(r"\s*\w+\s*", s) for s in more):
                    raise EvoWorldHipError(f"evoworld_hip.h: cannot read the declarators of '{decl}' in struct {name}")
                fields += [(ctype, f.strip()) for f in (field, *more)]
            self.struct_fields[name] = fields
            self.structs[name] = type("".join(p.title() for p in name.split("_")[1:]), (ctypes.Structure,),
                                      {"_fields_": [(f, self.ctype(t)) for t, f in fields], "__doc__": f"struct {name} (include/evoworld_hip.h)."})
        self.functions, self.signatures = {}, {}
        for ret, name, params in re.findall(r"(?:\A|(?<=[;{}]))\s*([\w\s*]+?)\s*\b(ew_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
            ret = re.sub(r"\s*\*\s*", "*", " ".join(ret.split()))
            types = [] if params.strip() == "void" else [_typed_name(p)[0] for p in params.split(",")]
            self.functions[name] = (ret, types)
            self.signatures[name] = (self.ctype(ret, ret=True), [self.ctype(t) for t in types])
        unread = set(re.findall(r"\b(ew_[a-z0-9_]+)\s*\(", text)) - set(self.functions)
        if unread:
            raise EvoWorldHipError(f"evoworld_hip.h: cannot read the prototype of {sorted(unread)}")

    def ctype(self, t, ret=False):
        """C type text -> ctypes type"""
        if t.endswith("*"):
            base = t[:-1].replace("const ", "").strip()
            if ret and base == "char":
                return ctypes.c_char_p
            return ctypes.POINTER(self.structs[base]) if base in self.structs else ctypes.c_void_p
        if ret and t == "void":
            return None
        if t not in _SCALARS:
            raise EvoWorldHipError(f"evoworld_hip.h: no ctypes mapping for the type '{t}'")
        return _SCALARS[t]


with open(HEADER_PATH) as _f:
    HEADER = Header(_f.read())
globals().update(HEADER.constants)                      # EW_OK, EW_ERR_*, EW_A_*, EW_ACT_*, EW_IM2COL_*, EW_ABI_VERSION
ABI_VERSION = HEADER.constants["EW_ABI_VERSION"]
GemmArgs, FfArgs = HEADER.structs["ew_gemm_args"], HEADER.structs["ew_ff_args"]

_lib = None


def bind(cdll):
    """Set restype / argtypes of every function the header declares on `cdll` (any build of the library); returns it."""
    for name, (restype, argtypes) in HEADER.signatures.items():
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            raise EvoWorldHipError(f"{cdll._name} does not export {name}") from None
        fn.restype, fn.argtypes = restype, argtypes
    return cdll


def load():
    """Load the shared library once; raise (never fall back) if it is missing or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EvoWorldHipError(
            f"{LIB_PATH} not found: build it with `make -C evoworld_amd/csrc` (hipcc --offload-arch=gfx950). "
            "evoworld_amd has no CPU fallback.")
    lib = bind(ctypes.CDLL(LIB_PATH))       # (EW_LIB_PATH: another BUILD of the same ABI -- A/B of two compilations in one process; older ABIs are refused)
    if lib.ew_abi_version() != ABI_VERSION:
        raise EvoWorldHipError(f"ABI mismatch: library {lib.ew_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


@contextlib.contextmanager
def using(lib):
    """Inside the block load() returns `lib` -- another build of the same ABI, already bound (`bind`) -- so that every ops.* call
    goes to it; the previous library is back on exit, also after an exception."""
    global _lib
    if lib.ew_abi_version() != ABI_VERSION:
        raise EvoWorldHipError(f"ABI mismatch: library {lib.ew_abi_version()} != binding {ABI_VERSION}")
    keep, _lib = _lib, lib
    try:
        yield lib
    finally:
        _lib = keep


def check(status, what):
    if status != 0:
        msg = load().ew_last_error()
        raise EvoWorldHipError(f"{what} failed ({status}): {msg.decode() if msg else ''}")
