"""CPU: the entry points of the prior's training step (nsg_cross_entropy_masked, nsg_gated_activation_sum_forward / _backward,
nsg_gated_activation_backward_colsum) are declared, bound and exported, and refuse each bad argument with dummy pointers
before any launch."""
import ctypes

from neural_sound_generation_amd import _lib
from tests.test_abi import exported_symbols, header_symbols

OK, ODD = 0x10000, 0x10004          # never dereferenced: every call below fails its checks before the launch
NEW = ["nsg_cross_entropy_masked", "nsg_cross_entropy_masked_workspace_bytes", "nsg_gated_activation_sum_forward",
       "nsg_gated_activation_sum_backward", "nsg_gated_activation_backward_colsum", "nsg_gated_colsum_workspace_bytes"]


def _p(v):
    return ctypes.c_void_p(v)


def test_new_entry_points_are_declared_bound_and_exported():
    lib = _lib.load()
    declared, exported = header_symbols(), exported_symbols(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib._SIGS and name in exported, name
        assert hasattr(lib, name)


def test_workspace_size_queries():
    lib = _lib.load()
    M, rpc = 3 * 240, 240
    assert lib.nsg_cross_entropy_masked_workspace_bytes(M, rpc) >= M * 4 + 256 * 8 + 3 * 8 + 12
    assert lib.nsg_cross_entropy_masked_workspace_bytes(M, rpc) >= lib.nsg_cross_entropy_workspace_bytes(M)
    for bad in ((0, 1), (-4, 2), (10, 0), (10, -1), (10, 3)):
        assert lib.nsg_cross_entropy_masked_workspace_bytes(*bad) == 0, bad
    assert lib.nsg_gated_colsum_workspace_bytes(M, 16, rpc) >= 3 * 32 * 8
    for bad in ((0, 16, 1), (M, 0, rpc), (M, 6, rpc), (M, 1028, rpc), (M, 16, 0), (M, 16, 7)):
        assert lib.nsg_gated_colsum_workspace_bytes(*bad) == 0, bad


def test_cross_entropy_masked_argument_checks():
    lib = _lib.load()
    M, K, rpc = 720, 32, 240
    need = lib.nsg_cross_entropy_masked_workspace_bytes(M, rpc)
    good = dict(logits=OK, target=OK, M=M, K=K, rpc=rpc, loss=OK, dl=OK, nll=OK, cnt=OK, ws=OK, nb=need)

    def ce(**change):
        a = dict(good, **change)
        return lib.nsg_cross_entropy_masked(_p(a["logits"]), _p(a["target"]), a["M"], a["K"], a["rpc"], 1.0, _p(a["loss"]), _p(a["dl"]),
                                            _p(a["nll"]), _p(a["cnt"]), _p(a["ws"]), a["nb"], None)

    for change in (dict(logits=0), dict(target=0), dict(loss=0), dict(M=0), dict(M=-720), dict(K=0), dict(rpc=0), dict(rpc=-1), dict(rpc=7)):
        assert ce(**change) == -1, change
        assert b"nsg_cross_entropy_masked" in lib.nsg_last_error_string(), change
    for change in (dict(ws=0), dict(nb=need - 1), dict(nb=0), dict(ws=ODD)):
        assert ce(**change) == -3, change
        assert b"nsg_cross_entropy_masked" in lib.nsg_last_error_string(), change


def test_gate_of_a_sum_argument_checks():
    lib = _lib.load()
    M, C, rpc = 720, 16, 240
    need = lib.nsg_gated_colsum_workspace_bytes(M, C, rpc)
    good = dict(a=OK, b=OK, cond=OK, y=OK, dy=OK, dx=OK, dcond=OK, M=M, C=C, rpc=rpc, ws=OK, nb=need)

    def fwd(**change):
        a = dict(good, **change)
        return lib.nsg_gated_activation_sum_forward(_p(a["a"]), _p(a["b"]), _p(a["cond"]), _p(a["y"]), a["M"], a["C"], a["rpc"], None)

    def bwd(**change):
        a = dict(good, **change)
        return lib.nsg_gated_activation_sum_backward(_p(a["a"]), _p(a["b"]), _p(a["cond"]), _p(a["dy"]), _p(a["dx"]), _p(a["dcond"]), a["M"],
                                                     a["C"], a["rpc"], _p(a["ws"]), a["nb"], None)

    def bwd_plain(**change):
        a = dict(good, **change)
        return lib.nsg_gated_activation_backward_colsum(_p(a["a"]), _p(a["cond"]), _p(a["dy"]), _p(a["dx"]), _p(a["dcond"]), a["M"], a["C"],
                                                        a["rpc"], _p(a["ws"]), a["nb"], None)

    common = [dict(a=0), dict(M=0), dict(M=-1), dict(C=0), dict(C=6), dict(C=-4), dict(rpc=0), dict(a=ODD), dict(cond=ODD)]
    for change in common + [dict(b=0), dict(y=0), dict(b=ODD), dict(y=ODD)]:
        assert fwd(**change) == -1, change
        assert b"nsg_gated_activation_sum_forward" in lib.nsg_last_error_string(), change
    for change in common + [dict(b=0), dict(dy=0), dict(dx=0), dict(b=ODD), dict(dy=ODD), dict(dx=ODD), dict(rpc=7)]:
        assert bwd(**change) == -1, change
        assert b"nsg_gated_activation_sum_backward" in lib.nsg_last_error_string(), change
    for change in common + [dict(dy=0), dict(dx=0), dict(dcond=0), dict(dy=ODD), dict(dx=ODD), dict(rpc=7)]:
        assert bwd_plain(**change) == -1, change
        assert b"nsg_gated_activation_backward_colsum" in lib.nsg_last_error_string(), change
    for fn in (bwd, bwd_plain):
        for change in (dict(ws=0), dict(nb=need - 1), dict(nb=0), dict(ws=ODD)):
            assert fn(**change) == -3, change
        assert fn(C=1028, M=4, rpc=4, nb=1 << 30) == -2                       # the column sums take C <= 1024
