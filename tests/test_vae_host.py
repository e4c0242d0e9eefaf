"""CPU: the continuous VAE's module surface against tests/golden/vae_tiny.npz, the new descriptor family and the latent entry
points through the C ABI with no kernel launched (fake 16-byte-aligned pointers that are never dereferenced), and the fp64
yardstick of the latent kernels against torch.autograd."""
import ctypes
import os

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, models as M
from tests.helpers import vae_ref64 as R
import fixture_io

P = ctypes.c_void_p(0x10000)
ODD = ctypes.c_void_p(0x10004)
NULL = ctypes.c_void_p(0)
F32, BF16 = _lib.NSG_F32, _lib.NSG_BF16
OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def g(golden_dir):
    return fixture_io.load(os.path.join(golden_dir, "vae_tiny.npz"))


# ---- the module ------------------------------------------------------------------------------------------------------
def test_module_tree_and_state_dict_are_the_fixtures(g):
    m = M.VAE(1, 8, 4)
    assert [n for n, _ in m.named_children()] == ["encoder", "decoder"]
    assert [type(c).__name__ for c in m.encoder] == ["Conv2d", "BatchNorm2d", "ReLU"] * 3 + ["Conv2d", "BatchNorm2d"]
    assert [type(c).__name__ for c in m.decoder] == ["ConvTranspose2d", "BatchNorm2d", "ReLU"] * 3 + ["ConvTranspose2d", "Tanh"]
    want = {k[len("sd0."):]: g[k] for k in g.files if k.startswith("sd0.")}
    sd = m.state_dict()
    assert list(sd) == list(want)
    for k, v in sd.items():
        assert tuple(v.shape) == want[k].shape and str(v.dtype).split(".")[1] == str(want[k].dtype), k
    params = [n for n, _ in m.named_parameters()]
    assert [k for k in want if k.split(".")[1] in "0 1 3 4 6 7 9 10".split() and k.endswith(("weight", "bias"))] == params


def test_construction_consumes_the_rng_as_the_reference(g):
    torch.manual_seed(1)
    sd = M.VAE(1, 8, 4).state_dict()
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g["init." + k]), k


def test_refusals():
    with pytest.raises(NotImplementedError):
        M.VAE(3, 8, 4)
    with pytest.raises(ValueError):
        M.VAE(1, 6, 4)
    with pytest.raises(ValueError):
        M.VAE(1, 8, 6)
    m = M.VAE(1, 8, 4)
    with pytest.raises(ValueError, match="T >= 28"):
        m(torch.zeros(2, 1, 80, 27))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 1, 64, 44))
    with pytest.raises(ValueError, match="eps must be"):
        m(torch.zeros(2, 1, 80, 44), eps=torch.zeros(2, 4, 14, 4))
    assert M.VAE.latent_grid((2, 1, 80, 28)) == (14, 1) and M.VAE.latent_grid((2, 1, 80, 31)) == (14, 1)
    assert M.VAE.latent_grid((2, 1, 80, 44)) == (14, 5)
    from neural_sound_generation_amd.vae_train import VAETrainStep
    with pytest.raises(RuntimeError):       # (a CPU model: FlatAdam has no CPU path; nothing falls back)
        VAETrainStep(m).step(torch.zeros(2, 1, 80, 44))


def test_vae_loss_is_the_references_sum_over_batch():
    from neural_sound_generation_amd.vae_train import vae_loss
    gen = torch.Generator().manual_seed(0)
    x_tilde, c = torch.rand(2, 1, 80, 28, generator=gen), torch.rand(2, 1, 80, 31, generator=gen)
    target = torch.zeros_like(c)
    target[:, :, :, :28] = x_tilde
    want = ((target - c) ** 2).sum() / 2 + 0.5
    assert torch.allclose(vae_loss(x_tilde, c, torch.tensor(0.5)), want, rtol=1e-6)


# ---- the stride-1 transposed descriptor family -----------------------------------------------------------------------
def s1(B=2, IH=14, IW=5, ci=8, co=12, k=3, pad=0, dtype=F32, k_w=0, pad_w=0, OH=None, OW=None):
    return _lib.ConvDesc(B, IH, IW, ci, IH + k - 1 - 2 * pad if OH is None else OH, IW + k - 1 - 2 * pad if OW is None else OW, co, k, 1, pad, 1,
                         dtype, k_w, pad_w)


@pytest.mark.parametrize("k,pad", [(3, 0), (5, 0), (3, 1), (7, 3), (7, 5), (1, 0)])
def test_stride1_transposed_descriptors_are_accepted(k, pad):
    lib = _lib.load()
    d = s1(k=k, pad=pad)
    need = lib.nsg_conv_workspace_bytes(ctypes.byref(d))
    assert need > 0
    assert lib.nsg_packed_weight_floats(ctypes.byref(d)) == k * k * 8 * 12
    # one layout, shared by the size query and the carve: one byte less is refused by name before anything is launched
    for name, args in (("nsg_conv_wgrad", (P, P, P, P, 0)), ("nsg_conv_forward_bnstats", (P, P, P, P, 0, 1e-5, 0.1, P, P, P, P))):
        assert getattr(lib, name)(ctypes.byref(d), *args, P, need - 1, None) == E_WORKSPACE
        msg = lib.nsg_last_error_string()
        assert name.encode() in msg and b"workspace too small" in msg, msg


@pytest.mark.parametrize("why,d,code", [
    ("bf16", s1(dtype=BF16, ci=8, co=16), E_UNSUPPORTED),
    ("rectangular", s1(k_w=5, pad_w=0), E_UNSUPPORTED),
    ("k > 7", s1(k=8), E_UNSUPPORTED),
    ("pad >= k", s1(k=3, pad=3, OH=10, OW=1), E_UNSUPPORTED),
    ("C_in % 4", s1(ci=6), E_UNSUPPORTED),
    ("C_out = 1", s1(co=1), E_UNSUPPORTED),
    ("extent", s1(OH=15), E_INVALID),
])
def test_refused_stride1_transposed_descriptors(why, d, code):
    lib = _lib.load()
    assert lib.nsg_conv_workspace_bytes(ctypes.byref(d)) == 0, why
    assert lib.nsg_conv_forward(ctypes.byref(d), P, P, P, P, 0, P, 1 << 30, None) == code, why
    assert lib.nsg_conv_dgrad(ctypes.byref(d), P, P, P, 0, P, 1 << 30, None) == code, why
    assert lib.nsg_conv_wgrad(ctypes.byref(d), P, P, P, P, 0, P, 1 << 30, None) == code, why
    w = (ctypes.c_void_p * 1)(0x10000)
    assert lib.nsg_pack_conv_weights_batch(1, ctypes.byref(d), ctypes.cast(w, ctypes.c_void_p), ctypes.cast(w, ctypes.c_void_p),
                                           ctypes.cast(w, ctypes.c_void_p), None) == code, why


# ---- the latent entry points' validation -------------------------------------------------------------------------------
def fwd(h=P, mean=P, invstd=P, gamma=P, beta=P, eps=P, z=P, kl=P, M_=28, Z=4, ws=P, nbytes=None):
    lib = _lib.load()
    nbytes = lib.nsg_vae_latent_workspace_bytes(M_, Z) if nbytes is None else nbytes
    return lib.nsg_vae_latent_forward(h, mean, invstd, gamma, beta, eps, z, kl, M_, Z, ws, nbytes, None)


def bwd(h=P, mean=P, invstd=P, gamma=P, beta=P, eps=P, dz=P, kl_grad=NULL, dy=P, dgamma=P, dbeta=P, M_=28, Z=4, ws=P, nbytes=None):
    lib = _lib.load()
    nbytes = lib.nsg_vae_latent_workspace_bytes(M_, Z) if nbytes is None else nbytes
    return lib.nsg_vae_latent_backward(h, mean, invstd, gamma, beta, eps, dz, 1.0, kl_grad, dy, dgamma, dbeta, M_, Z, ws, nbytes, None)


def test_latent_workspace_query():
    lib = _lib.load()
    assert lib.nsg_vae_latent_workspace_bytes(28, 4) > 0
    assert lib.nsg_vae_latent_workspace_bytes(70001, 128) >= 1015 * 2 * 256 * 4        # 69 rows per slab: 1015 slabs of [2][2Z] floats
    for M_, Z in ((0, 4), (28, 0), (28, 2), (28, 6), (28, 516), (1 << 28, 4)):
        assert lib.nsg_vae_latent_workspace_bytes(M_, Z) == 0, (M_, Z)


def test_latent_validation_codes():
    for name in ("h", "mean", "invstd", "gamma", "beta", "eps", "z", "kl"):
        assert fwd(**{name: NULL}) == E_INVALID, name
    for name in ("h", "mean", "invstd", "gamma", "beta", "eps", "dz", "dy", "dgamma", "dbeta"):
        assert bwd(**{name: NULL}) == E_INVALID, name
    for call in (fwd, bwd):
        assert call(M_=0, nbytes=1 << 20) == E_INVALID
        assert call(M_=-3, nbytes=1 << 20) == E_INVALID
        for Z in (0, 2, 6, 516):
            assert call(Z=Z, nbytes=1 << 20) == E_UNSUPPORTED, Z
        assert call(M_=1 << 28, Z=4, nbytes=1 << 40) == E_UNSUPPORTED          # M * 2Z = 2^31
        assert call(M_=(1 << 28) - 1, Z=4, nbytes=0) == E_WORKSPACE            # the largest M at Z = 4 passes the size check
        need = _lib.load().nsg_vae_latent_workspace_bytes(28, 4)
        assert call(nbytes=need - 1) == E_WORKSPACE
        assert b"workspace too small" in _lib.load().nsg_last_error_string()
        assert call(ws=NULL) == E_WORKSPACE
    for name in ("h", "eps", "z"):
        assert fwd(**{name: ODD}) == E_INVALID, name
    for name in ("h", "eps", "dz", "dy"):
        assert bwd(**{name: ODD}) == E_INVALID, name


# ---- the yardstick itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M_,Z", [(1, 4), (28, 4), (65, 36)])
def test_latent_ref64_is_autograds_gradient(M_, Z):
    gen = torch.Generator().manual_seed(M_ + Z)
    h = torch.randn(M_, 2 * Z, generator=gen)
    mean, invstd = torch.randn(2 * Z, generator=gen) * 0.1, torch.rand(2 * Z, generator=gen) + 0.5
    gamma, beta = torch.rand(2 * Z, generator=gen) + 0.5, torch.rand(2 * Z, generator=gen) * 0.6 - 0.3
    eps, dz = torch.randn(M_, Z, generator=gen), torch.randn(M_, Z, generator=gen)
    for kl_scale, kl_grad in ((1.0, 1.0), (0.25, -1.7)):
        z, kl, dy = R.latent_autograd(h, mean, invstd, gamma, beta, eps, dz, kl_scale, kl_grad)
        z64, kl64, _ = R.latent_forward(h, mean, invstd, gamma, beta, eps)
        dy64 = R.latent_backward(h, mean, invstd, gamma, beta, eps, dz, kl_scale, kl_grad)[0]
        assert torch.allclose(z, z64, rtol=1e-12, atol=1e-12) and torch.allclose(kl, kl64, rtol=1e-12)
        assert torch.allclose(dy, dy64, rtol=1e-10, atol=1e-12)
