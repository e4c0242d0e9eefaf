"""CPU: nsg_adamw_step and nsg_grad_sumsq refuse each bad argument with dummy pointers before any launch (the manner of
tests/test_prior_walk_ctl_abi.py), and the binding derived from include/nsg.h maps their prototypes as written here by hand."""
import ctypes
import math
from ctypes import c_float, c_int32, c_int64, c_size_t, c_void_p

from neural_sound_generation_amd import _lib

OK, OK2, OK3, OK4, ODD = 0x10000, 0x20000, 0x30000, 0x40000, 0x10004    # never dereferenced: every call fails its checks first
N = 4
GOOD = dict(p=OK, g=OK2, m=OK3, v=OK4, n=N, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.0,
            seg_end=0x50000, seg_wd=0x60000, n_seg=2, sumsq=0x70000, max_norm=1.0, skip_nonfinite=1, shadow=0x80000,
            one_minus_decay=1e-4, stats=0x90000)
_PTRS = ("p", "g", "m", "v", "seg_end", "seg_wd", "sumsq", "shadow", "stats")
_ORDER = ("p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "step", "grad_scale", "seg_end", "seg_wd", "n_seg", "sumsq",
          "max_norm", "skip_nonfinite", "shadow", "one_minus_decay", "stats")


def adamw(lib, **change):
    a = dict(GOOD, **change)
    return lib.nsg_adamw_step(*[ctypes.c_void_p(a[k]) if k in _PTRS else a[k] for k in _ORDER], None)


def test_adamw_step_argument_checks():
    lib = _lib.load()
    invalid = [dict(p=0), dict(g=0), dict(m=0), dict(v=0), dict(n=-1),
               dict(seg_wd=0), dict(seg_end=0),                                   # half a segment table
               dict(n_seg=0), dict(seg_end=0, seg_wd=0),                          # a table without entries, entries without a table
               dict(sumsq=0, skip_nonfinite=0),                                   # max_norm > 0 without the sum of squares
               dict(sumsq=0, max_norm=0.0),                                       # the guard without it
               dict(max_norm=math.nan),
               dict(one_minus_decay=1.5), dict(one_minus_decay=-1.0001), dict(one_minus_decay=math.nan),
               dict(step=0), dict(step=-3),
               dict(shadow=OK), dict(shadow=OK + 4), dict(shadow=OK - 4),         # the shadow is p, or overlaps it
               dict(sumsq=0x70004), dict(stats=0x90002)]
    for change in invalid:
        assert adamw(lib, **change) == -1, change
        assert b"nsg_adamw_step" in lib.nsg_last_error_string(), change
    # every extension at its neutral value and nothing to do: accepted without a launch
    neutral = dict(n=0, seg_end=0, seg_wd=0, n_seg=0, sumsq=0, max_norm=0.0, skip_nonfinite=0, shadow=0, one_minus_decay=0.0, stats=0)
    assert adamw(lib, **neutral) == 0
    assert adamw(lib, n=0) == 0                                                   # and with every extension given
    assert adamw(lib, **dict(neutral, max_norm=-1.0, one_minus_decay=1.0)) == 0   # max_norm <= 0 is "off"; decay 0 is legal
    assert adamw(lib, **dict(neutral, step=0)) == -1


def test_grad_sumsq_argument_checks():
    lib = _lib.load()
    need = lib.nsg_grad_sumsq_workspace_bytes(1 << 20)
    assert need >= 8 and need == lib.nsg_grad_sumsq_workspace_bytes(1)            # one double per block of a fixed grid

    def sumsq(g=OK, n=N, out=OK2, ws=OK3, nb=need):
        return lib.nsg_grad_sumsq(c_void_p(g), n, c_void_p(out), c_void_p(ws), nb, None)

    for kw in (dict(g=0), dict(out=0), dict(n=-1), dict(out=OK2 + 4), dict(ws=OK3 + 4)):
        assert sumsq(**kw) == -1, kw
        assert b"nsg_grad_sumsq" in lib.nsg_last_error_string(), kw
    for kw in (dict(ws=0), dict(nb=need - 1), dict(nb=0)):
        assert sumsq(**kw) == -3, kw
        assert b"nsg_grad_sumsq" in lib.nsg_last_error_string(), kw


def test_prototypes_as_the_binding_derives_them():
    P = c_void_p
    assert _lib._SIGS["nsg_adamw_step"] == (c_int32, [P, P, P, P, c_int64, c_float, c_float, c_float, c_float, c_int32, c_float,
                                                       P, P, c_int32, P, c_float, c_int32, P, c_float, P, P])
    assert _lib._SIGS["nsg_grad_sumsq"] == (c_int32, [P, c_int64, P, P, c_size_t, P])
    assert _lib._SIGS["nsg_grad_sumsq_workspace_bytes"] == (c_size_t, [c_int64])
    # the old entry point stays as it was, and so does the ABI version's rule: no existing signature changed
    assert _lib._SIGS["nsg_adam_step"][1] == _lib._SIGS["nsg_adamw_step"][1][:11] + [P]
