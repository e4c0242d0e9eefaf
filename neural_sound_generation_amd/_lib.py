"""ctypes binding of libnsg.so (the C ABI declared in include/nsg.h).

There is no fallback: if the HIP library is missing or a call fails, a RuntimeError is raised.
The oracle under oracle/ is never imported from here.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_size_t, c_void_p

from .build import INCLUDE

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libnsg.so")
HEADER_PATH = os.path.join(INCLUDE, "nsg.h")


class NsgError(RuntimeError):
    pass


class ConvDesc(Structure):
    """struct nsg_conv_desc; its _fields_ are the header's, filled in below."""

    def key(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


_SCALARS = {"int": c_int32, "int32_t": c_int32, "int64_t": c_int64, "size_t": c_size_t, "float": c_float}
_PROTO = re.compile(r"NSG_API\s+([\w\s\*]+?)\b(nsg_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, proto, ret=False):
    """ctypes type of one parameter declaration of `proto`, or (ret) of its return type.  Nothing is defaulted."""
    words = re.findall(r"\w+|\*", decl)
    if "*" in words:
        if ret:
            if words == ["const", "char", "*"]:
                return c_char_p
        else:
            return POINTER(ConvDesc) if "nsg_conv_desc" in words else c_void_p
    else:
        words = [w for w in words if w != "const"]
        typ = " ".join(words if ret or len(words) == 1 else words[:-1])     # a parameter's last word is its name
        if typ in _SCALARS:
            return _SCALARS[typ]
    raise NsgError(f"include/nsg.h: no ctypes mapping for '{decl.strip()}' in: {proto}")


def parse_header(text):
    """The ABI as header text states it -> (signatures: name -> (restype, argtypes), every NSG_API prototype in order;
    constants: name -> int, the integer #defines and enumerators; the field names of struct nsg_conv_desc, in order)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)      # the header's prose quotes function names
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(NSG_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    for body in re.findall(r"\benum\s*\w*\s*\{([^}]*)\}", text):
        for item in filter(str.strip, body.split(",")):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item)
            if not m:
                raise NsgError(f"include/nsg.h: enumerator without an explicit integer value: '{item.strip()}'")
            consts[m[1]] = int(m[2])
    fields = []
    m = re.search(r"\bstruct\s+nsg_conv_desc\s*\{([^}]*)\}", text)
    for stmt in filter(str.strip, m[1].split(";")) if m else ():
        typ, _, names = stmt.strip().partition(" ")
        if typ != "int32_t":
            raise NsgError(f"include/nsg.h: struct nsg_conv_desc holds int32_t fields only, got '{stmt.strip()}'")
        fields += [n.strip() for n in names.split(",")]
    sigs = {}
    body = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)             # (#define NSG_API ... is not a prototype)
    for at in re.finditer(r"\bNSG_API\b", body):
        m = _PROTO.match(body, at.start())
        if not m:
            raise NsgError("include/nsg.h: cannot parse the prototype: " + " ".join(body[at.start():].split(";")[0].split()))
        proto = " ".join(m[0].split())
        params = [] if m[3].strip() == "void" else m[3].split(",")
        sigs[m[2]] = (_ctype(m[1], proto, ret=True), [_ctype(a, proto) for a in params])
    return sigs, consts, fields


def _header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise NsgError(f"{HEADER_PATH}: cannot read the ABI header ({e})")


# name -> (restype, argtypes) of every entry point include/nsg.h declares: exactly the product library's exports
_SIGS, _CONSTS, _fields = _header()
if not _fields:
    raise NsgError(f"{HEADER_PATH}: struct nsg_conv_desc not found")
ConvDesc._fields_ = [(f, c_int32) for f in _fields]
HEADER_SYMBOLS = list(_SIGS)
NSG_VERSION = _CONSTS["NSG_VERSION"]      # bumped in the header on ANY signature change; a library of another version is refused
NSG_RELU_IN, NSG_TANH_OUT, NSG_OUT_F32, NSG_RELU_OUT, NSG_F32, NSG_BF16, NSG_C1_MOMENTS = (_CONSTS[n] for n in (
    "NSG_RELU_IN", "NSG_TANH_OUT", "NSG_OUT_F32", "NSG_RELU_OUT", "NSG_F32", "NSG_BF16", "NSG_C1_MOMENTS"))
NSG_DTW_MAX_FRAMES, NSG_DTW_BLOCK_COLS = _CONSTS["NSG_DTW_MAX_FRAMES"], _CONSTS["NSG_DTW_BLOCK_COLS"]
NSG_F0_MAX_CANDIDATES, NSG_F0_VITERBI_LDS_FRAMES = _CONSTS["NSG_F0_MAX_CANDIDATES"], _CONSTS["NSG_F0_VITERBI_LDS_FRAMES"]
NSG_PSOLA_MIN_WEIGHT_LOG2 = _CONSTS["NSG_PSOLA_MIN_WEIGHT_LOG2"]

_lib = None


def _bind(lib):
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    if lib.nsg_version() != NSG_VERSION:
        raise NsgError(f"the HIP library reports ABI version {lib.nsg_version()}, include/nsg.h declares version {NSG_VERSION}: rebuild it "
                       "(python -m neural_sound_generation_amd.build --force)")
    return lib


DIAG_LIB_PATH = os.path.join(_PKG, "libnsg_diag.so")
# run-time switches of the DIAGNOSTICS library (never of libnsg.so): name -> argument type
_DIAG_SWITCHES = {"nsg_debug_set_patch_gemm": c_int32, "nsg_debug_set_patch_grid": c_int32, "nsg_debug_set_wgrad_strip": c_int32,
                  "nsg_debug_set_c1_moments": c_int32, "nsg_debug_set_wgrad_bf16_native": c_int32, "nsg_debug_set_wgrad_stagger": c_int32,
                  "nsg_debug_set_wgrad_diag": c_int32, "nsg_debug_set_wgrad_stamp_buffer": c_void_p, "nsg_debug_set_stamp_buffer": c_void_p,
                  "nsg_debug_set_f0_direct": c_int32}
_diag = None


def load_diag():
    """The diagnostics build of the same library (libnsg_diag.so: -DNSG_DIAG + diag.hip; `python -m
    neural_sound_generation_amd.build --diag`): kernel-variant switches and cycle stamps for scripts/ and the A/B tests."""
    global _diag
    if _diag is None:
        import torch  # noqa: F401
        if not os.path.exists(DIAG_LIB_PATH):
            raise NsgError(f"{DIAG_LIB_PATH} is missing: python -m neural_sound_generation_amd.build --diag")
        lib = _bind(ctypes.CDLL(DIAG_LIB_PATH))
        for name, at in _DIAG_SWITCHES.items():
            fn = getattr(lib, name)
            fn.argtypes = [at]
            fn.restype = None
        _diag = lib
    return _diag


class use_diag:
    """with use_diag() as lib: every ops.* call inside goes to the diagnostics library (whose nsg_debug_set_* switches `lib`
    exposes); the product library is back afterwards."""

    def __enter__(self):
        global _lib
        load()
        self._saved = _lib
        _lib = load_diag()
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self._saved
        return False


def load():
    """Load libnsg.so; raises RuntimeError (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # Device memory and streams come from PyTorch-ROCm, so libnsg.so must bind to the HIP runtime
    # torch carries (same SONAME as /opt/rocm's): load torch's first, or the process ends up with
    # two HIP runtimes and the second one finds no device.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise NsgError(
            f"{LIB_PATH} is missing: build the HIP kernels first (python -m neural_sound_generation_amd.build). "
            "There is no CPU fallback for this path.")
    _lib = _bind(ctypes.CDLL(LIB_PATH))
    return _lib


# Optional per-call census for bench.py's roofline table: when CENSUS is set (an object with begin() / end(label, start,
# flops, nbytes)), every entry-point call is bracketed by events on the launch stream.  A wrapper that knows the call's
# algorithmic work announces it with tag(label, flops, nbytes) right before the call; untagged calls go under their C name.
CENSUS = None
_TAG = None


def tag(label: str, flops: float = 0.0, nbytes: float = 0.0):
    global _TAG
    if CENSUS is not None:
        _TAG = (label, float(flops), float(nbytes))


def call(name: str, *args):
    """Call a status-returning entry point; raise with the library's message on failure."""
    global _TAG
    lib = load()
    if CENSUS is not None:
        t, _TAG = _TAG, None
        start = CENSUS.begin()
        rc = getattr(lib, name)(*args)
        label, fl, nb = t if t is not None else (name, 0.0, 0.0)
        CENSUS.end(label, start, fl, nb)
    else:
        rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.nsg_last_error_string()
        raise NsgError(f"{name} failed (status {rc}): {msg.decode() if msg else ''}")


def query(name: str, *args):
    return getattr(load(), name)(*args)
