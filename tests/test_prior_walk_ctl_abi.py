"""CPU: nsg_prior_walk_ctl (the column walk with temperature, top-k, top-p and kept codes) refuses each bad argument, and a
shape outside the walk's envelope, with dummy pointers before any launch; the Python layers refuse the same before they
touch a GPU."""
import ctypes
import math

import pytest
import torch

from neural_sound_generation_amd import _lib
from neural_sound_generation_amd.prior import GatedPixelCNN
from tests.test_gpu_prior_walk_envelope import deepest_layers

OK, ODD = 0x10000, 0x10004          # never dereferenced: every call below fails its checks before the launch
B, H, W, DIM = 5, 4, 37, 16
GOOD = dict(w=OK, emb=OK, cond=OK, vh=OK, u=OK, x_in=0, keep=0, codes=OK, e_row=OK, e_clip_stride=W * DIM, logits=0,
            B=B, H=H, W=W, dim=DIM, n_layers=2, input_dim=64, row=0, temperature=0.8, top_k=7, top_p=0.9)


def walk_ctl(lib, **change):
    a = dict(GOOD, **change)
    p = [ctypes.c_void_p(a[k]) for k in ("w", "emb", "cond", "vh", "u", "x_in", "keep", "codes", "e_row")]
    return lib.nsg_prior_walk_ctl(*p, a["e_clip_stride"], ctypes.c_void_p(a["logits"]), a["B"], a["H"], a["W"], a["dim"],
                                  a["n_layers"], a["input_dim"], a["row"], a["temperature"], a["top_k"], a["top_p"], None)


def test_prior_walk_ctl_argument_checks():
    lib = _lib.load()
    invalid = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf),
               dict(temperature=-math.inf), dict(temperature=1e-45),                 # 1 / T overflows fp32
               dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.5), dict(top_p=math.nan),
               dict(u=0), dict(codes=0), dict(x_in=OK), dict(keep=OK),               # x_in without keep and keep without x_in
               dict(w=0), dict(emb=0), dict(cond=0), dict(vh=0), dict(e_row=0),
               dict(B=0), dict(H=0), dict(W=0), dict(row=-1), dict(row=H),
               dict(e_clip_stride=W * DIM - 4), dict(e_clip_stride=W * DIM + 2),
               dict(w=ODD), dict(emb=ODD), dict(cond=ODD), dict(vh=ODD), dict(e_row=ODD)]
    for change in invalid:
        assert walk_ctl(lib, **change) == -1, change
        assert b"nsg_prior_walk_ctl" in lib.nsg_last_error_string(), change
    unsupported = [dict(dim=8), dict(dim=20), dict(dim=136), dict(n_layers=0), dict(input_dim=0), dict(input_dim=1025),
                   dict(dim=128, n_layers=deepest_layers(1024, 128) + 1, input_dim=1024, e_clip_stride=W * 128)]
    for change in unsupported:
        assert walk_ctl(lib, **change) == -2, change
        msg = lib.nsg_last_error_string()
        assert b"nsg_prior_walk_ctl" in msg and b"outside the envelope" in msg, change
    # the same with kept codes and with the controls at their neutral values
    assert walk_ctl(lib, x_in=OK, keep=OK, dim=8) == -2
    assert walk_ctl(lib, temperature=1.0, top_k=0, top_p=1.0, dim=8) == -2


def test_sample_validates_its_controls_before_the_gpu():
    """ValueError for each bad control, for given without keep and the reverse, and for a prefix wider than the grid: all
    raised before anything is sent to a device (the labels live on the CPU here)."""
    model = GatedPixelCNN(64, 16, 2, 4)
    label = torch.tensor([0, 3])
    shape = (3, 5)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf),
                dict(temperature="warm"), dict(top_k=-1), dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=math.nan)):
        with pytest.raises(ValueError):
            model.sample(label, shape=shape, batch_size=2, **bad)
    given, keep = torch.zeros(2, 3, 5, dtype=torch.int64), torch.zeros(2, 3, 5, dtype=torch.bool)
    with pytest.raises(ValueError):
        model.sample(label, shape=shape, batch_size=2, given=given)
    with pytest.raises(ValueError):
        model.sample(label, shape=shape, batch_size=2, keep=keep)
    with pytest.raises(ValueError):
        model.sample(label, shape=shape, batch_size=2, given=given[:, :, :4], keep=keep)           # shape
    with pytest.raises(ValueError):
        model.sample(label, shape=shape, batch_size=2, given=given, keep=keep[:1])
    with pytest.raises(ValueError):
        model.sample(label, shape=shape, batch_size=2, given=given.int(), keep=keep)               # dtype
    with pytest.raises(ValueError):
        model.sample(label, shape=shape, batch_size=2, given=given, keep=keep.long())
    keep[1, 2, 4] = True
    for code in (-1, 64):
        given[1, 2, 4] = code
        with pytest.raises(ValueError):
            model.sample(label, shape=shape, batch_size=2, given=given, keep=keep)                 # a kept code outside [0, K)
    with pytest.raises(ValueError):
        model.continue_codes(torch.zeros(2, 3, 6, dtype=torch.int64), label, 5)
    with pytest.raises(ValueError):
        model.continue_codes(torch.zeros(2, 3, 4, dtype=torch.int32), label, 5)
