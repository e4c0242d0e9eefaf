"""CPU: nsg_prior_walk_cfg (the controlled column walk under classifier-free guidance) is exported with the header's
signature and refuses an odd B, a bad guidance, each argument nsg_prior_walk_ctl refuses and a shape outside the walk's
envelope, with dummy pointers before any launch; GatedPixelCNN.sample refuses a bad guidance or null label before it touches
a GPU."""
import ctypes
import math
import re

import pytest
import torch

from neural_sound_generation_amd import _lib
from neural_sound_generation_amd.prior import GatedPixelCNN
from tests.test_gpu_prior_walk_envelope import deepest_layers

OK, ODD = 0x10000, 0x10004          # never dereferenced: every call below fails its checks before the launch
B, H, W, DIM = 6, 4, 37, 16
GOOD = dict(w=OK, emb=OK, cond=OK, vh=OK, u=OK, x_in=0, keep=0, codes=OK, e_row=OK, e_clip_stride=W * DIM, logits=0,
            B=B, H=H, W=W, dim=DIM, n_layers=2, input_dim=64, row=0, temperature=0.8, top_k=7, top_p=0.9, guidance=2.0)


def walk_cfg(lib, **change):
    a = dict(GOOD, **change)
    p = [ctypes.c_void_p(a[k]) for k in ("w", "emb", "cond", "vh", "u", "x_in", "keep", "codes", "e_row")]
    return lib.nsg_prior_walk_cfg(*p, a["e_clip_stride"], ctypes.c_void_p(a["logits"]), a["B"], a["H"], a["W"], a["dim"],
                                  a["n_layers"], a["input_dim"], a["row"], a["temperature"], a["top_k"], a["top_p"], a["guidance"], None)


def test_prior_walk_cfg_is_exported_with_the_headers_signature():
    """nsg_prior_walk_ctl's parameters plus `float guidance` before the stream, as include/nsg.h declares them."""
    lib = _lib.load()
    assert "nsg_prior_walk_cfg" in _lib.HEADER_SYMBOLS
    fn = lib.nsg_prior_walk_cfg                                  # AttributeError if the library does not export it
    ctl_res, ctl_args = _lib._SIGS["nsg_prior_walk_ctl"]
    res, args = _lib._SIGS["nsg_prior_walk_cfg"]
    assert res is ctypes.c_int32 and res is ctl_res
    assert args == ctl_args[:-1] + [ctypes.c_float, ctypes.c_void_p]
    assert fn.restype is res and list(fn.argtypes) == args
    with open(_lib.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)

    def names(entry):
        params = re.search(r"NSG_API\s+int\s+" + entry + r"\s*\(([^()]*)\)\s*;", text)[1]
        return [" ".join(p.split()) for p in params.split(",")]

    assert names("nsg_prior_walk_cfg") == names("nsg_prior_walk_ctl")[:-1] + ["float guidance", "void *stream"]


def test_prior_walk_cfg_argument_checks():
    lib = _lib.load()
    invalid = [dict(B=5), dict(B=1), dict(B=7, input_dim=0),                          # an odd B, also ahead of the envelope check
               dict(guidance=math.nan), dict(guidance=math.inf), dict(guidance=-math.inf), dict(guidance=-0.5), dict(guidance=1024.5),
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf),
               dict(temperature=-math.inf), dict(temperature=1e-45),                 # 1 / T overflows fp32
               dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.5), dict(top_p=math.nan),
               dict(u=0), dict(codes=0), dict(x_in=OK), dict(keep=OK),               # x_in without keep and keep without x_in
               dict(w=0), dict(emb=0), dict(cond=0), dict(vh=0), dict(e_row=0),
               dict(B=0), dict(H=0), dict(W=0), dict(row=-1), dict(row=H),
               dict(e_clip_stride=W * DIM - 4), dict(e_clip_stride=W * DIM + 2),
               dict(w=ODD), dict(emb=ODD), dict(cond=ODD), dict(vh=ODD), dict(e_row=ODD)]
    for change in invalid:
        assert walk_cfg(lib, **change) == -1, change
        assert b"nsg_prior_walk_cfg" in lib.nsg_last_error_string(), change
    unsupported = [dict(dim=8), dict(dim=20), dict(dim=136), dict(n_layers=0), dict(input_dim=0), dict(input_dim=1025),
                   dict(dim=128, n_layers=deepest_layers(1024, 128) + 1, input_dim=1024, e_clip_stride=W * 128)]
    for change in unsupported:
        assert walk_cfg(lib, **change) == -2, change
        msg = lib.nsg_last_error_string()
        assert b"nsg_prior_walk_cfg" in msg and b"outside the envelope" in msg, change
    # the same with kept codes, with the controls at their neutral values, and at both ends of the guidance range
    assert walk_cfg(lib, x_in=OK, keep=OK, dim=8) == -2
    assert walk_cfg(lib, temperature=1.0, top_k=0, top_p=1.0, dim=8) == -2
    assert walk_cfg(lib, guidance=0.0, dim=8) == -2
    assert walk_cfg(lib, guidance=1024.0, dim=8) == -2


def test_sample_validates_guidance_before_the_gpu():
    """ValueError for each bad guidance or null label, raised before anything is sent to a device (the labels live on the CPU
    here, and so does the model)."""
    model = GatedPixelCNN(64, 16, 2, 4)
    label = torch.tensor([0, 3])
    args = dict(shape=(3, 5), batch_size=2)
    for bad in (dict(guidance=True, null_label=3), dict(guidance="strong", null_label=3), dict(guidance=math.nan, null_label=3),
                dict(guidance=math.inf, null_label=3), dict(guidance=-1.0, null_label=3), dict(guidance=1025, null_label=3),
                dict(guidance=1.0), dict(null_label=3), dict(guidance=0, null_label=3), dict(guidance=1.0, null_label=4),
                dict(guidance=1.0, null_label=-1), dict(guidance=1.0, null_label=2.0), dict(guidance=1.0, null_label=False)):
        with pytest.raises(ValueError):
            model.sample(label, **args, **bad)
        with pytest.raises(ValueError):
            model.continue_codes(torch.zeros(2, 3, 4, dtype=torch.int64), label, 5, **bad)
