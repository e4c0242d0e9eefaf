"""CPU: the size query and the entry point of every workspace agree.

Each entry point that cuts its workspace into sections takes the sections from the layout function its size query returns the
total of (csrc: *_layout).  Here every such entry point is called with valid shapes (the tiny fixture's: 2 clips of 80 x 64,
D = 32, K = 64), fake 16-byte-aligned pointers that are never dereferenced, and ONE BYTE LESS workspace than its own query
asks for: it must answer NSG_E_WORKSPACE and name itself before anything is launched.  An entry point that checked against
another expression than its query's would pass this check and go on to launch (no GPU here: another error code).

nsg_cross_entropy_masked and nsg_audio_griffin_lim are held to the same in test_prior_train_abi.py and
test_audio_entry_points.py.  Entry points that share an implementation report under its name (nsg_vq_forward_bf16x3_cond as
nsg_vq_forward_bf16x3, nsg_index_add_rows_bf16x2 as nsg_index_add_rows, ...): the expected name is given with each case."""
import ctypes

import pytest

from neural_sound_generation_amd import _lib

P = ctypes.c_void_p(0x10000)
F32, BF16 = _lib.NSG_F32, _lib.NSG_BF16
B, H, W, D, K = 2, 80, 64, 32, 64
N = B * (H // 4) * (W // 4)             # rows of the latent grid


def desc(*a):
    return _lib.ConvDesc(*a)


# the layers of the tiny model as nsg_conv_desc: (B, IH, IW, C_in, OH, OW, C_out, k, stride, pad, transposed, dtype)
CONV_3X3 = desc(B, H // 4, W // 4, D, H // 4, W // 4, D, 3, 1, 1, 0, BF16)
CONV_T = desc(B, H // 4, W // 4, D, H // 2, W // 2, D, 4, 2, 1, 1, F32)
CONV_C1 = desc(B, H, W, 1, H // 2, W // 2, D, 4, 2, 1, 0, BF16)
CONVT_C1 = desc(B, H // 2, W // 2, D, H, W, 1, 4, 2, 1, 1, F32)


def conv_ws(d):
    return ("nsg_conv_workspace_bytes", (ctypes.byref(d),))


# (entry point, name in the error text, (size query, its arguments), arguments with WS where workspace, workspace_bytes go)
WS = object()
CASES = [
    ("nsg_vq_forward", "nsg_vq_forward", ("nsg_vq_workspace_bytes", (N, D, K)), (P, P, N, D, K, P, P, P, WS, None)),
    ("nsg_debug_vq_forward_valu", "nsg_vq_forward", ("nsg_vq_workspace_bytes", (N, D, K)), (P, P, N, D, K, P, P, P, WS, None)),
    # (81920 rows against 8192 codes: the search runs in slices, which have sections of their own)
    ("nsg_vq_forward", "nsg_vq_forward", ("nsg_vq_workspace_bytes", (81920, 128, 8192)), (P, P, 81920, 128, 8192, P, P, P, WS, None)),
    ("nsg_vq_forward_bf16x3", "nsg_vq_forward_bf16x3", ("nsg_vq_bf16x3_workspace_bytes", (N, D, K)), (P, P, N, D, K, P, P, P, P, 0, WS, None)),
    ("nsg_vq_forward_bf16x3_cond", "nsg_vq_forward_bf16x3", ("nsg_vq_bf16x3_workspace_bytes", (N, D, K)),
     (P, P, N, D, K, P, P, P, P, 0, P, N // B, WS, None)),
    ("nsg_vq_forward_bf16x3_bnres", "nsg_vq_forward_bf16x3", ("nsg_vq_bf16x3_workspace_bytes", (N, D, K)),
     (P, P, P, P, P, P, P, N, D, K, P, P, P, 0, P, N // B, WS, None)),
    ("nsg_index_add_rows", "nsg_index_add_rows", ("nsg_index_add_workspace_bytes", (N, D, K)), (P, P, N, D, K, P, P, WS, None)),
    ("nsg_index_add_rows_bf16x2", "nsg_index_add_rows", ("nsg_index_add_workspace_bytes", (N, 64, K)), (P, P, N, 64, K, P, P, WS, None)),
    ("nsg_index_add_rows_sorted", "nsg_index_add_rows_sorted", ("nsg_index_add_sorted_workspace_bytes", (N, D, K)), (P, P, N, D, K, P, P, WS, None)),
    ("nsg_index_add_rows_sorted_bnres", "nsg_index_add_rows_sorted", ("nsg_index_add_sorted_workspace_bytes", (N, D, K)),
     (P, P, P, P, P, P, P, N, D, K, P, P, WS, None)),
    ("nsg_conv_forward_bnstats", "nsg_conv_forward_bnstats", conv_ws(CONV_3X3),
     (ctypes.byref(CONV_3X3), P, P, P, P, 0, 1e-5, 0.1, P, P, P, P, WS, None)),
    ("nsg_conv_forward_bnstats", "nsg_conv_forward_bnstats", conv_ws(CONV_T), (ctypes.byref(CONV_T), P, P, P, P, 0, 1e-5, 0.1, P, P, P, P, WS, None)),
    ("nsg_conv_wgrad", "nsg_conv_wgrad", conv_ws(CONV_3X3), (ctypes.byref(CONV_3X3), P, P, P, P, 0, WS, None)),
    ("nsg_conv_wgrad", "nsg_conv_wgrad", conv_ws(CONV_T), (ctypes.byref(CONV_T), P, P, P, P, 0, WS, None)),
    ("nsg_conv_wgrad", "nsg_conv_wgrad", conv_ws(CONV_C1), (ctypes.byref(CONV_C1), P, P, P, P, 0, WS, None)),
    ("nsg_conv_wgrad", "nsg_conv_wgrad", conv_ws(CONVT_C1), (ctypes.byref(CONVT_C1), P, P, P, P, 0, WS, None)),
    ("nsg_conv_forward", "nsg_conv_forward", conv_ws(CONV_C1), (ctypes.byref(CONV_C1), P, P, P, P, 0, WS, None)),
    ("nsg_conv_forward", "nsg_conv_forward", conv_ws(CONVT_C1), (ctypes.byref(CONVT_C1), P, P, P, P, 0, WS, None)),
    ("nsg_conv_dgrad", "nsg_conv_dgrad", conv_ws(CONV_C1), (ctypes.byref(CONV_C1), P, P, P, 0, WS, None)),
    ("nsg_conv_dgrad", "nsg_conv_dgrad", conv_ws(CONVT_C1), (ctypes.byref(CONVT_C1), P, P, P, 0, WS, None)),
    ("nsg_bn_relu_c1convt_forward", "nsg_bn_relu_c1convt_forward", ("nsg_bn_relu_c1convt_workspace_bytes", (B, H // 2, W // 2, D)),
     (P, BF16, P, P, P, P, P, P, P, 0, B, H // 2, W // 2, D, WS, None)),
    ("nsg_bn_relu_c1convt_forward_mse", "nsg_bn_relu_c1convt_forward_mse", ("nsg_bn_relu_c1convt_workspace_bytes", (B, H // 2, W // 2, D)),
     (P, BF16, P, P, P, P, P, P, P, P, W, 1.0, P, P, P, B, H // 2, W // 2, D, WS, None)),
    ("nsg_bn_relu_c1convt_backward", "nsg_bn_relu_c1convt_backward", ("nsg_bn_relu_c1convt_workspace_bytes", (B, H // 2, W // 2, D)),
     (P, BF16, P, P, P, P, P, P, P, P, P, P, P, P, B, H // 2, W // 2, D, WS, None)),
    # (128 clips: there the forward's sections, not the backward's, set the size both directions are held to)
    ("nsg_bn_relu_c1convt_backward", "nsg_bn_relu_c1convt_backward", ("nsg_bn_relu_c1convt_workspace_bytes", (128, H // 2, W // 2, D)),
     (P, BF16, P, P, P, P, P, P, P, P, P, P, P, P, 128, H // 2, W // 2, D, WS, None)),
    ("nsg_bn_relu_conv1x1_forward", "nsg_bn_relu_conv1x1_forward", ("nsg_bn_relu_conv1x1_workspace_bytes", (N, D)),
     (P, P, P, P, P, P, P, P, N, D, BF16, WS, None)),
    ("nsg_bn_relu_conv1x1_forward_bnstats", "nsg_bn_relu_conv1x1_forward_bnstats", ("nsg_bn_relu_conv1x1_workspace_bytes", (N, D)),
     (P, P, P, P, P, P, P, P, 1e-5, 0.1, P, P, P, P, N, D, BF16, WS, None)),
    ("nsg_bn_relu_conv1x1_wgrad", "nsg_bn_relu_conv1x1_wgrad", ("nsg_bn_relu_conv1x1_workspace_bytes", (N, D)),
     (P, P, P, P, P, P, P, N, D, BF16, WS, None)),
    # (655360 rows: there the weight gradient's slabs, not the flat GEMM's sections, set the size)
    ("nsg_bn_relu_conv1x1_wgrad", "nsg_bn_relu_conv1x1_wgrad", ("nsg_bn_relu_conv1x1_workspace_bytes", (655360, 128)),
     (P, P, P, P, P, P, P, 655360, 128, BF16, WS, None)),
    ("nsg_bn_backward_conv1x1_dgrad", "nsg_bn_backward_conv1x1_dgrad", ("nsg_bn_relu_conv1x1_workspace_bytes", (N, D)),
     (P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, N, D, BF16, WS, None)),
    ("nsg_bn_backward_conv1x1_dgrad_wgrad", "nsg_bn_backward_conv1x1_dgrad_wgrad", ("nsg_bn_backward_conv1x1_dgrad_wgrad_workspace_bytes", (N, 128)),
     (P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, N, 128, BF16, WS, None)),
    ("nsg_c1conv_bn_relu_forward", "nsg_c1conv_bn_relu_forward", ("nsg_c1conv_bn_workspace_bytes", (D,)),
     (P, P, P, P, P, P, P, P, P, 1e-5, 0.1, 1, P, BF16, B, H, W, D, WS, P, None)),
    ("nsg_c1conv_bn_relu_backward", "nsg_c1conv_bn_relu_backward", ("nsg_c1conv_bn_workspace_bytes", (D,)),
     (P, P, P, P, P, P, P, P, BF16, P, P, P, P, B, H, W, D, WS, P, None)),
    ("nsg_vq_losses_indexed_bn", "nsg_vq_losses_indexed_bn", ("nsg_vq_losses_indexed_bn_workspace_bytes", (N, D)),
     (P, P, P, N, D, K, 1.0, P, P, P, BF16, P, P, P, P, P, WS, None)),
    ("nsg_vq_losses_indexed_bnres", "nsg_vq_losses_indexed_bnres", ("nsg_vq_losses_indexed_bn_workspace_bytes", (N, D)),
     (P, P, P, P, P, P, P, P, N, D, K, 1.0, P, P, P, P, P, WS, None)),
    ("nsg_cross_entropy", "nsg_cross_entropy", ("nsg_cross_entropy_workspace_bytes", (N,)), (P, P, N, K, 1.0, P, P, WS, None)),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: f"{i}-{CASES[i][0]}")
def test_one_byte_less_than_the_query_is_refused(case):
    name, reported, (query, qargs), args = CASES[case]
    lib = _lib.load()
    need = getattr(lib, query)(*qargs)
    assert need > 1, (query, qargs)

    def call(nbytes):
        full = []
        for a in args:
            full.extend((P, nbytes) if a is WS else (a,))
        return getattr(lib, name)(*full)

    assert call(need - 1) == -3         # NSG_E_WORKSPACE
    msg = lib.nsg_last_error_string()
    assert reported.encode() in msg and b"workspace too small" in msg, msg
    assert call(0) == -3
