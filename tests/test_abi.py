"""CPU: libnsg.so loads and exports every entry point include/nsg.h declares; argument validation
and the pure size queries work without a GPU (no kernel is launched here)."""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_size_t, c_void_p

import pytest

from neural_sound_generation_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    return sorted(set(re.findall(r"NSG_API\s+[\w\s\*]+?\b(nsg_\w+)\s*\(", text)))


def exported_symbols(path):
    """Dynamic symbols a shared object DEFINES (nm -D --defined-only), nsg_* only."""
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("nsg_")})


def test_library_exports_exactly_the_declared_symbols():
    """include/nsg.h IS the ABI, in both directions: every declared entry point is exported, and libnsg.so exports no nsg_*
    symbol the header does not declare (round 2's library carried 13 undeclared nsg_debug_set_* switches over process-global
    state; they now exist only in the diagnostics build, libnsg_diag.so)."""
    lib = _lib.load()
    declared = header_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/nsg.h but not exported by libnsg.so"
    assert sorted(_lib.HEADER_SYMBOLS) == declared, "the ctypes table and include/nsg.h disagree"
    exported = exported_symbols(_lib.LIB_PATH)
    extra = sorted(set(exported) - set(declared))
    assert not extra, f"libnsg.so exports symbols include/nsg.h does not declare: {extra}"
    assert not [n for n in exported if n.startswith("nsg_debug_set")], "a run-time variant switch leaked into the product library"
    m = re.search(r"#define\s+NSG_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "nsg.h")).read())
    assert lib.nsg_version() == int(m.group(1)) == _lib.NSG_VERSION


def test_diagnostics_library_is_a_superset_with_the_switches():
    if not os.path.exists(_lib.DIAG_LIB_PATH):
        pytest.skip("libnsg_diag.so not built (python -m neural_sound_generation_amd.build --diag)")
    exported = set(exported_symbols(_lib.DIAG_LIB_PATH))
    assert set(header_symbols()) <= exported
    assert set(_lib._DIAG_SWITCHES) <= exported


def test_invalid_arguments_are_rejected_before_any_launch():
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    assert lib.nsg_rowsumsq(null, 4, 8, null, null) == -1
    assert b"nsg_rowsumsq" in lib.nsg_last_error_string()
    with pytest.raises(_lib.NsgError, match="nsg_adam_step"):
        _lib.call("nsg_adam_step", null, null, null, null, 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, null)
    # D > 256 is outside what the VQ kernel implements
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.nsg_vq_forward(p, p, 1, 300, 4, p, null, null, p, 1 << 20, null) == -2


def test_size_queries():
    lib = _lib.load()
    assert lib.nsg_vq_workspace_bytes(1000, 128, 512) >= (1000 + 512) * 4
    d = _lib.ConvDesc(2, 20, 16, 8, 20, 16, 8, 3, 1, 1, 0)
    assert lib.nsg_packed_weight_floats(ctypes.byref(d)) == 9 * 8 * 8
    assert lib.nsg_conv_workspace_bytes(ctypes.byref(d)) > 0
    bad = _lib.ConvDesc(2, 20, 16, 6, 20, 16, 8, 3, 1, 1, 0)   # C_in % 4 != 0
    assert lib.nsg_conv_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.nsg_bn_workspace_bytes(5120, 128) > 0
    assert lib.nsg_reduce_workspace_bytes(10) >= 8


def test_packed_weight_image_sizes_include_the_fragment_ordered_copy():
    """nsg_conv_forward / nsg_conv_dgrad read, for the bf16 shapes gemm_patch.hip takes, a fragment-ordered copy BEHIND the plain
    [tap][n][c] image: the allocation size the header tells callers to use must account for it -- and must not
    for the shapes that have none."""
    lib = _lib.load()
    def n(desc):
        return lib.nsg_packed_weight_floats(ctypes.byref(desc))
    plain = 9 * 128 * 128
    assert n(_lib.ConvDesc(2, 20, 64, 128, 20, 64, 128, 3, 1, 1, 0, _lib.NSG_BF16)) == 2 * plain          # bf16 3x3 128->128: twin
    assert n(_lib.ConvDesc(2, 20, 64, 128, 20, 64, 128, 3, 1, 1, 0, _lib.NSG_F32)) == plain               # fp32: none
    assert n(_lib.ConvDesc(2, 20, 64, 32, 20, 64, 32, 3, 1, 1, 0, _lib.NSG_BF16)) == 9 * 32 * 32          # narrow bf16: none
    assert n(_lib.ConvDesc(2, 20, 64, 256, 40, 128, 256, 4, 2, 1, 1, _lib.NSG_BF16)) == 2 * 16 * 256 * 256   # transposed 4/2/1, D = 256


def test_gather_gemm_rejects_tensors_past_its_32_bit_row_offsets():
    """A transposed conv's output is 4x its input: (820, 20, 256, 128) bf16 passes the 4 GiB operand limit but the
    (820, 40, 512, 128) output has more than 2^31 elements, which the kernel's int row offsets cannot address
    (ADVICE r1).  The launcher must refuse before touching the GPU -- fake pointers, no allocation, runs on CPU."""
    lib = _lib.load()
    fake, null = ctypes.c_void_p(0x10000), ctypes.c_void_p(0)
    d = _lib.ConvDesc(820, 20, 256, 128, 40, 512, 128, 4, 2, 1, 1, _lib.NSG_BF16)
    assert lib.nsg_conv_forward(ctypes.byref(d), fake, fake, null, fake, 0, fake, 1 << 30, null) == -2
    assert b"2^31" in lib.nsg_last_error_string()
    # the data gradient of Conv2d(128, 128, 4, 2, 1) writes the same 4x tensor (with the fused add / mask operands on the same offsets)
    d = _lib.ConvDesc(820, 40, 512, 128, 20, 256, 128, 4, 2, 1, 0, _lib.NSG_BF16)
    assert lib.nsg_conv_dgrad_relu_add(ctypes.byref(d), fake, fake, fake, fake, fake, 0, fake, 1 << 30, null) == -2
    assert b"2^31" in lib.nsg_last_error_string()
    # one clip fewer fits: the guard must not fire early (it would launch, so only the pure checks are exercised up to here)
    d = _lib.ConvDesc(1 << 20, 20, 256, 128, 40, 512, 128, 4, 2, 1, 1, _lib.NSG_BF16)   # the row count itself overflows
    assert lib.nsg_conv_forward(ctypes.byref(d), fake, fake, null, fake, 0, fake, 1 << 30, null) == -2


def test_loader_refuses_a_library_of_another_abi_version(monkeypatch):
    """entry points changed signature under an unchanged NSG_VERSION, and a stale libnsg.so then took a stream handle
    for a data pointer.  NSG_VERSION is now bumped on any signature change and the loader compares it."""
    lib = _lib.load()
    monkeypatch.setattr(_lib, "NSG_VERSION", lib.nsg_version() + 1)
    with pytest.raises(_lib.NsgError, match="ABI version"):
        _lib._bind(ctypes.CDLL(_lib.LIB_PATH))


def test_prior_walk_size_query_and_argument_checks():
    """nsg_prior_walk_weight_floats is the size of GatedPixelCNN._walk_blob inside the walk's envelope and 0 outside it;
    nsg_prior_walk refuses each bad argument, and a shape outside the envelope, with dummy pointers before any launch."""
    from neural_sound_generation_amd.prior import GatedPixelCNN
    from tests.test_gpu_prior_walk_envelope import DEEPEST, WIDTHS, deepest_layers
    lib = _lib.load()
    for K, dim, L in WIDTHS:
        L = deepest_layers(K, dim) if L is DEEPEST else L
        assert lib.nsg_prior_walk_weight_floats(dim, L, K) == GatedPixelCNN(K, dim, L)._walk_blob(K).numel(), (K, dim, L)
    outside = [(8, 2, 64), (20, 2, 64), (136, 2, 64), (0, 2, 64), (-16, 2, 64), (16, 0, 64), (16, -1, 64), (16, 2, 0),
               (16, 2, -1), (16, 2, 1025), (128, deepest_layers(1024, 128) + 1, 1024), (64, deepest_layers(512, 64) + 1, 512)]
    for dim, L, K in outside:
        assert lib.nsg_prior_walk_weight_floats(dim, L, K) == 0, (dim, L, K)

    ok, odd = 0x10000, 0x10004      # never dereferenced: every call below fails its checks before the launch
    B, H, W, dim = 5, 4, 37, 16
    good = dict(w=ok, emb=ok, cond=ok, vh=ok, u=ok, x_in=0, codes=ok, e_row=ok, e_clip_stride=W * dim, logits=0,
                B=B, H=H, W=W, dim=dim, n_layers=2, input_dim=64, row=0)

    def walk(**change):
        a = dict(good, **change)
        p = [ctypes.c_void_p(a[k]) for k in ("w", "emb", "cond", "vh", "u", "x_in", "codes", "e_row")]
        return lib.nsg_prior_walk(*p, a["e_clip_stride"], ctypes.c_void_p(a["logits"]), a["B"], a["H"], a["W"], a["dim"],
                                  a["n_layers"], a["input_dim"], a["row"], None)

    invalid = [dict(w=0), dict(emb=0), dict(cond=0), dict(vh=0), dict(e_row=0),
               dict(x_in=ok), dict(u=0), dict(codes=0),                              # both u and x_in, neither, no codes
               dict(B=0), dict(H=0), dict(W=0), dict(row=-1), dict(row=H),
               dict(e_clip_stride=W * dim - 4), dict(e_clip_stride=W * dim + 2),
               dict(w=odd), dict(emb=odd), dict(cond=odd), dict(vh=odd), dict(e_row=odd)]
    for change in invalid:
        assert walk(**change) == -1, change
        assert b"nsg_prior_walk" in lib.nsg_last_error_string()
    unsupported = [dict(dim=8), dict(dim=20), dict(dim=136), dict(n_layers=0), dict(input_dim=0), dict(input_dim=1025),
                   dict(dim=128, n_layers=deepest_layers(1024, 128) + 1, input_dim=1024, e_clip_stride=W * 128)]
    for change in unsupported:
        assert walk(**change) == -2, change
        assert b"outside the envelope" in lib.nsg_last_error_string()


# ---- the binding is derived from include/nsg.h (_lib.parse_header): the tests below fail if the parser mis-maps a type ----
_P = c_void_p
FROZEN = {
    "nsg_version": (c_int32, []),
    "nsg_last_error_string": (c_char_p, []),
    "nsg_vq_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "nsg_adam_step": (c_int32, [_P, _P, _P, _P, c_int64, c_float, c_float, c_float, c_float, c_int32, c_float, _P]),
    "nsg_pack_conv_weights_batch": (c_int32, [c_int32, POINTER(_lib.ConvDesc), _P, _P, _P, _P]),
    "nsg_bn_backward_conv1x1_dgrad_wgrad": (c_int32, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                      c_int64, c_int32, c_int32, _P, c_size_t, _P]),
}


def test_frozen_signatures():
    """Six prototypes that between them meet every mapping rule, written out by hand: return types int / const char * / size_t,
    scalar parameters of each of the four kinds, plain and double pointers, the descriptor pointer, (void), 24 parameters."""
    assert len(FROZEN["nsg_bn_backward_conv1x1_dgrad_wgrad"][1]) == 24
    for name, want in FROZEN.items():
        assert _lib._SIGS[name] == want, name
    lib = _lib.load()
    for name, (res, args) in FROZEN.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_header_parser_on_snippets():
    parse = _lib.parse_header
    sigs, consts, fields = parse("""
        /* NSG_API int nsg_in_a_block_comment(double x); spread
           over lines */
        // NSG_API int nsg_in_a_line_comment(double x);
        int nsg_not_an_entry_point(double x);
        NSG_API size_t
        nsg_spread(const float *const *w,
                   int64_t n,   /* a comment between parameters */
                   const int flag, void *const *out,
                   float
                   scale);
        NSG_API int32_t nsg_nothing(void);
        #define NSG_SOME 7
        #define NSG_NEG -3
        #define NSG_NOT_AN_INT 1.5
        enum { NSG_A = 4, NSG_B = -2 };
        typedef struct nsg_conv_desc { int32_t a, b; int32_t c; /* note */ } nsg_conv_desc;
    """)
    assert sigs == {"nsg_spread": (c_size_t, [c_void_p, c_int64, c_int32, c_void_p, c_float]), "nsg_nothing": (c_int32, [])}
    assert consts == {"NSG_SOME": 7, "NSG_NEG": -3, "NSG_A": 4, "NSG_B": -2}
    assert fields == ["a", "b", "c"]
    assert parse("NSG_API int nsg_f(const nsg_conv_desc *d, nsg_conv_desc *const e);")[0] == {
        "nsg_f": (c_int32, [POINTER(_lib.ConvDesc)] * 2)}
    for bad in ("NSG_API int nsg_f(double x);", "NSG_API int nsg_f(int32_t a, unsigned n);", "NSG_API int nsg_f(unsigned int n);",
                "NSG_API int nsg_f(nsg_conv_desc d);", "NSG_API int nsg_f(const nsg_conv_desc d, void *s);",
                "NSG_API double nsg_f(void);", "NSG_API void nsg_f(int32_t a);", "NSG_API float *nsg_f(int32_t a);",
                "NSG_API int nsg_f(int32_t a, void (*cb)(int));", "NSG_API int nsg_f(int32_t a", "NSG_API int f(int32_t a);",
                "NSG_API int nsg_f(int32_t a) { return a; }", "NSG_API int nsg_f();", "NSG_API int nsg_f(long n);",
                "NSG_API int nsg_f(int32_t);\nNSG_API int nsg_g(uint8_t k);"):
        with pytest.raises(_lib.NsgError, match="nsg.h") as e:
            parse(bad)
        assert bad.split("\n")[-1][:20] in str(e.value), (bad, str(e.value))       # the message names the prototype
    with pytest.raises(_lib.NsgError):
        parse("enum { NSG_A = 4, NSG_B };")
    with pytest.raises(_lib.NsgError):
        parse("struct nsg_conv_desc { int32_t a; int64_t b; };")


def test_header_constants_and_struct_are_the_ones_the_package_exports(monkeypatch, tmp_path):
    from neural_sound_generation_amd import ops
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    sigs, consts, fields = _lib.parse_header(text)
    assert sigs == _lib._SIGS and list(sigs) == _lib.HEADER_SYMBOLS == list(_lib._SIGS) and len(sigs) == len(header_symbols())
    for name in ("NSG_RELU_IN", "NSG_TANH_OUT", "NSG_OUT_F32", "NSG_RELU_OUT", "NSG_F32", "NSG_BF16", "NSG_VERSION", "NSG_C1_MOMENTS"):
        assert getattr(_lib, name) == consts[name] == int(re.search(r"\b%s\b\s*=?\s*(-?\d+)" % name, text).group(1)), name
    for name in ("NSG_RELU_IN", "NSG_TANH_OUT", "NSG_OUT_F32", "NSG_RELU_OUT", "NSG_F32", "NSG_BF16"):
        assert getattr(ops, name) == consts[name]
    assert (consts["NSG_RELU_IN"], consts["NSG_TANH_OUT"], consts["NSG_RELU_IN2"], consts["NSG_OUT_F32"], consts["NSG_RELU_OUT"]) == (1, 2, 4, 8, 16)
    assert (consts["NSG_OK"], consts["NSG_E_INVALID"], consts["NSG_E_UNSUPPORTED"], consts["NSG_E_WORKSPACE"]) == (0, -1, -2, -3)
    assert ops.C1_MOMENTS == consts["NSG_C1_MOMENTS"] == 273 and (consts["NSG_F32"], consts["NSG_BF16"]) == (0, 1)
    exported = [n for n, _ in _lib.ConvDesc._fields_]
    assert fields == exported == ["B", "IH", "IW", "C_in", "OH", "OW", "C_out", "k", "stride", "pad", "transposed", "dtype", "k_w", "pad_w"]
    assert all(t is c_int32 for _, t in _lib.ConvDesc._fields_) and ctypes.sizeof(_lib.ConvDesc) == 4 * len(fields)
    swapped = text.replace("int32_t k, stride, pad;", "int32_t stride, k, pad;")
    assert swapped != text
    got = _lib.parse_header(swapped)[2]
    assert got != exported and sorted(got) == sorted(exported) and got.index("stride") + 1 == got.index("k") == exported.index("k") + 1
    # a missing header is an error that names the path
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "nsg.h"))
    with pytest.raises(_lib.NsgError, match=re.escape(str(tmp_path / "nsg.h"))):
        _lib._header()


def test_bound_argtypes_convert_plain_numbers_and_refuse_a_float_for_an_integer():
    """ops.py / audio.py pass plain Python and numpy numbers: the argtypes bound from the header convert them, and a float where
    the header declares an integer raises before the call."""
    import numpy as np
    lib = _lib.load()
    want = lib.nsg_vq_workspace_bytes(c_int64(1000), c_int32(128), c_int32(512))
    assert want > 0 and _lib.query("nsg_vq_workspace_bytes", 1000, np.int64(128), np.int32(512)) == want
    assert _lib.query("nsg_bn_relu_conv1x1_supported", True, 128) == 1                       # bool -> int32 (NSG_BF16 == 1)
    with pytest.raises(ctypes.ArgumentError):
        _lib.query("nsg_vq_workspace_bytes", 1000, 128.0, 512)
    with pytest.raises(_lib.NsgError, match="nsg_adam_step"):                                # an int for a float, None for a pointer
        _lib.call("nsg_adam_step", None, None, None, None, 4, 1, 0.9, np.float32(0.999), 1e-8, 1, 1, None)
    descs = (_lib.ConvDesc * 1)()                                                            # a descriptor array passes as it is
    assert lib.nsg_pack_conv_weights_batch(1, descs, None, None, None, None) == -1
