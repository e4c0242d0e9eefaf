"""CPU: the F0-conditioned decoder's host side (include/nsg.h: nsg_add_cond, nsg_column_sum, nsg_f0_bins) -- the ABI, the
launchers' refusals with fake pointers before any launch, the model's state_dict with and without the table, the ValueErrors
of the Python layers before a device is touched, audio.f0_affine in closed form, and the bins' fp32 restatement against their
fp64 definition on a large random draw (tests/helpers/f0_cond_ref.py)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from neural_sound_generation_amd import _lib, audio, evaluate, models, ops, train
from tests.helpers import f0_cond_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, ODD, NULL = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004), ctypes.c_void_p(0)


def test_symbols_are_declared_exported_and_take_no_workspace():
    text = open(os.path.join(ROOT, "include", "nsg.h")).read()
    lib = _lib.load()
    for name in ("nsg_add_cond", "nsg_column_sum", "nsg_f0_bins"):
        assert re.search(r"NSG_API\s+int\s+%s\s*\(" % name, text), name
        assert name in _lib.HEADER_SYMBOLS and hasattr(lib, name)
    sigs, _, _ = _lib.parse_header(text)
    V, I32, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    assert sigs["nsg_add_cond"] == (I32, [V] * 6 + [I32] * 8 + [V])
    assert sigs["nsg_column_sum"] == (I32, [V, I32, I32, I32, I32, I32, V, V])
    assert sigs["nsg_f0_bins"] == (I32, [V] * 5 + [I32] * 4 + [F32] * 2 + [V])
    # no size query came with them: the 24 the header had, none of them for these entry points
    queries = set(re.findall(r"NSG_API\s+size_t\s+(nsg_\w+_workspace_bytes)\s*\(", text))
    assert len(queries) == 24, sorted(queries)
    assert not [q for q in queries if re.search(r"add_cond|column_sum|f0_bins", q)]
    assert all(ctypes.c_size_t not in sigs[n][1] for n in ("nsg_add_cond", "nsg_column_sum", "nsg_f0_bins"))


def test_launchers_refuse_before_any_launch():
    lib = _lib.load()
    F32, BF16 = _lib.NSG_F32, _lib.NSG_BF16

    def add_cond(x=P, idx=NULL, clip=P, table=P, bins=P, y=P, B=2, H=3, W=5, C=8, K=0, n_rows=9, relu=0, dt=F32):
        return lib.nsg_add_cond(x, idx, clip, table, bins, y, B, H, W, C, K, n_rows, relu, dt, None)

    bad = [dict(x=NULL), dict(table=NULL), dict(bins=NULL), dict(y=NULL),                                 # null pointers
           dict(B=0), dict(H=0), dict(W=0), dict(C=0), dict(n_rows=0), dict(B=-1), dict(idx=P, K=0),      # non-positive sizes
           dict(dt=2), dict(dt=-1),                                                                       # unknown dtype
           dict(C=6), dict(C=12, dt=BF16), dict(C=4, dt=BF16),                                            # C not a multiple of the vector width
           dict(x=ODD), dict(clip=ODD), dict(table=ODD), dict(y=ODD), dict(bins=ODD), dict(idx=ODD, K=4),  # misaligned
           dict(B=1 << 14, H=1 << 7, W=1 << 7, C=8), dict(n_rows=1 << 29, C=8), dict(idx=P, K=1 << 29, C=8)]   # products >= 2^31
    for kw in bad:
        assert add_cond(**kw) == -1 and b"nsg_add_cond" in lib.nsg_last_error_string(), kw

    def column_sum(x=P, dt=F32, B=2, H=3, W=5, C=8, out=P):
        return lib.nsg_column_sum(x, dt, B, H, W, C, out, None)

    bad = [dict(x=NULL), dict(out=NULL), dict(B=0), dict(H=0), dict(W=0), dict(C=0), dict(H=-3), dict(dt=2), dict(C=6), dict(C=12, dt=BF16),
           dict(x=ODD), dict(out=ODD), dict(B=1 << 14, H=1 << 7, W=1 << 7, C=8)]
    for kw in bad:
        assert column_sum(**kw) == -1 and b"nsg_column_sum" in lib.nsg_last_error_string(), kw

    def f0_bins(f0=P, frames=NULL, affine=NULL, bins=P, logf=NULL, B=4, T=26, W=6, n_bins=32, fmin=65.0, fmax=500.0):
        return lib.nsg_f0_bins(f0, frames, affine, bins, logf, B, T, W, n_bins, fmin, fmax, None)

    odd2 = ctypes.c_void_p(0x10002)
    nan, inf = float("nan"), float("inf")
    bad = [dict(f0=NULL), dict(bins=NULL), dict(B=0), dict(T=0), dict(W=0), dict(W=7), dict(T=23), dict(n_bins=0), dict(n_bins=-1),
           dict(fmin=0.0), dict(fmin=-65.0), dict(fmin=500.0), dict(fmin=600.0), dict(fmin=nan), dict(fmax=nan), dict(fmax=inf),
           dict(f0=odd2), dict(frames=odd2), dict(affine=odd2), dict(logf=odd2), dict(bins=ODD), dict(B=1 << 16, T=1 << 15, W=8)]
    for kw in bad:
        assert f0_bins(**kw) == -1 and b"nsg_f0_bins" in lib.nsg_last_error_string(), kw


def test_wrappers_check_before_anything_is_launched():
    z = torch.zeros(2, 3, 5, 8)
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        ops.add_cond(z, torch.zeros(9, 8), torch.zeros(2, 5, dtype=torch.int64))
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        ops.column_sum(z)
    with pytest.raises(_lib.NsgError, match="expected a GPU tensor"):
        ops.f0_bins(torch.zeros(2, 26), 6, 32, 65.0, 500.0)
    f = torch.zeros(2, 26)
    for kw, msg in ((dict(n_bins=0), "n_bins"), (dict(n_bins=2.0), "n_bins"), (dict(fmin=0.0), "fmin"), (dict(fmin=500.0, fmax=65.0), "fmin")):
        with pytest.raises(ValueError, match=msg):
            audio.f0_bins(f, **kw)
    with pytest.raises(ValueError, match="no latent column"):
        audio.f0_bins(torch.zeros(2, 3))
    with pytest.raises(ValueError, match=r"\(B, T\)"):
        audio.f0_bins(torch.zeros(26))


def test_state_dict_with_and_without_the_table():
    torch.manual_seed(3)
    plain = models.VQVAE(1, 16, 32, n_speakers=7)
    keys = list(plain.state_dict())
    assert not [k for k in keys if "f0" in k] and not hasattr(plain, "f0_embedding") and plain.n_f0_bins is None
    after_plain = torch.rand(1)
    torch.manual_seed(3)
    again = models.VQVAE(1, 16, 32, n_speakers=7, n_f0_bins=None)
    assert list(again.state_dict()) == keys and torch.equal(torch.rand(1), after_plain)      # the same RNG draws
    torch.manual_seed(3)
    m = models.VQVAE(1, 16, 32, n_speakers=7, n_f0_bins=8)
    sd = m.state_dict()
    assert list(sd) == keys + ["f0_embedding.weight"]                # created after the speaker table
    assert tuple(sd["f0_embedding.weight"].shape) == (9, 16) and m.f0_range == (65.0, 500.0)
    for k in keys:                                                   # (n_f0_bins=None: the very weights of the model without the argument)
        assert torch.equal(again.state_dict()[k], plain.state_dict()[k]), k
    assert 0.03 < float(sd["f0_embedding.weight"].std()) < 0.3       # normal_(0, 0.1), 144 draws
    no_spk = models.VQVAE(1, 16, 32, n_f0_bins=4)
    assert tuple(no_spk.state_dict()["f0_embedding.weight"].shape) == (5, 16) and "speaker_embedding.weight" not in no_spk.state_dict()
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_f0_bins"):
            models.VQVAE(1, 16, 32, n_f0_bins=bad)
    for bad in ((0.0, 500.0), (500.0, 65.0), (65.0, float("inf"))):
        with pytest.raises(ValueError, match="f0_range"):
            models.VQVAE(1, 16, 32, n_f0_bins=8, f0_range=bad)


def test_python_layers_raise_on_the_cpu_before_touching_a_device():
    with_f0 = models.VQVAE(1, 16, 32, n_speakers=2, n_f0_bins=8)
    without = models.VQVAE(1, 16, 32, n_speakers=2)
    mel, g = torch.zeros(2, 1, 80, 32), torch.tensor([0, 1])
    bins = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="convert_voice: .*F0-conditioned.*give f0_bins"):
        evaluate.convert_voice(with_f0, mel, g)
    with pytest.raises(ValueError, match="convert_voice: f0_bins given to a model without an F0 table"):
        evaluate.convert_voice(without, mel, g, bins)
    for bad in (bins[:, :7], bins.to(torch.int32), bins[:1], bins + 9, bins - 1, bins.tolist()):
        with pytest.raises(ValueError, match="convert_voice: f0_bins must"):
            evaluate.convert_voice(with_f0, mel, g, bad)
    # the module paths check the same on the host
    for bad in (bins[:, :7], bins.to(torch.int32), bins + 9):
        with pytest.raises(ValueError, match="f0_bins must"):
            with_f0._condition(torch.zeros(2, 16, 20, 8), None, bad)
    with pytest.raises(ValueError, match="without an F0 table"):
        without._condition(torch.zeros(2, 16, 20, 8), None, bins)
    cpu = torch.device("cpu")
    stats = np.array([[7.0, 0.2], [7.5, 0.3]])
    with pytest.raises(ValueError, match="test_conversion_f0: f0_stats given to a model without an F0 table"):
        evaluate.test_conversion_f0(None, without, [], cpu, 0, f0_stats=stats)
    with pytest.raises(ValueError, match=r"f0_stats must be \(2, 2\)"):
        evaluate.test_conversion_f0(None, with_f0, [], cpu, 0, f0_stats=stats[:1])
    with pytest.raises(ValueError, match="empty loader"):
        evaluate.test_conversion_f0(None, with_f0, [], cpu, 0, f0_stats=stats)
    wav, lens = torch.zeros(2, 4096), np.array([4096, 4096])
    nan_stats = np.array([[7.0, 0.2], [float("nan"), float("nan")]])
    with pytest.raises(ValueError, match=r"f0_stats of the target speakers \[1\] are not finite"):
        evaluate.test_conversion_f0(None, with_f0, [(wav, lens, wav, lens, torch.tensor([0, 1]))], cpu, 0, f0_stats=nan_stats)
    with pytest.raises(ValueError, match="tracker must be"):
        evaluate.speaker_f0_stats([], 2, cpu, tracker="pyin")
    with pytest.raises(ValueError, match="empty loader"):
        evaluate.speaker_f0_stats([], 2, cpu)
    # the fused step and its driver
    args = types.SimpleNamespace(log_interval=1)
    batch = (None, None, torch.zeros(2, 80, 32), torch.tensor([0, 1]), torch.tensor([8192, 8192]))
    with pytest.raises(ValueError, match=r"train_conditioned: .*get_data_loaders\(with_audio=True\)"):
        train.train_conditioned(args, with_f0, None, [batch], cpu, 0)
    with pytest.raises(ValueError, match="tracker must be"):
        train.train_conditioned(args, with_f0, None, [batch], cpu, 0, tracker="pyin")


def test_f0_affine_closed_form():
    sums = torch.tensor([[4.0, 28.0, 200.0],        # {6, 8, 6, 8}: mean 7, variance 1
                         [1.0, 7.25, 7.25 ** 2],    # one voiced frame: no spread to scale
                         [0.0, 0.0, 0.0],           # no voiced frame: nothing moves
                         [3.0, 24.0, 192.0],        # {8, 8, 8}: zero spread
                         [2.0, 15.0, 112.625]],     # {7.25, 7.75}: mean 7.5, variance 1/16
                        dtype=torch.float64)
    got = audio.f0_affine(sums, torch.tensor([7.5, 7.5, 6.0, 9.0, 7.0]), torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5]))
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, 3)
    want = [[7.0, 0.5, 7.5], [7.25, 1.0, 7.5], [6.0, 1.0, 6.0], [8.0, 1.0, 9.0], [7.5, 2.0, 7.0]]
    assert got.tolist() == want
    assert audio.f0_affine(sums, 7.5, 0.5)[:, 2].tolist() == [7.5] * 5              # numbers serve every clip
    np.testing.assert_array_equal(R.affine_f64(sums.numpy(), [7.5, 7.5, 6.0, 9.0, 7.0], 0.5), np.array(want, dtype=np.float32))
    # logf0_sums on the host restates the helper's moments
    f0 = torch.tensor([[64.0, 0.0, 256.0, 128.0, 256.0], [0.0, 0.0, 100.0, 0.0, 0.0]])
    np.testing.assert_array_equal(audio.logf0_sums(f0, [4, 5]).numpy(), R.logf0_sums_f64(f0.numpy(), [4, 5]))
    assert audio.logf0_sums(f0, [4, 5])[0].tolist() == [3.0, 21.0, 149.0]
    for bad in (sums.float(), sums[:, :2], sums[0]):
        with pytest.raises(ValueError, match="f0_affine: sums_src"):
            audio.f0_affine(bad, 7.0, 0.5)
    with pytest.raises(ValueError, match="target_mean and target_std"):
        audio.f0_affine(sums, torch.zeros(4), 0.5)


def test_fp32_restatement_agrees_with_fp64_on_every_decided_column():
    rs = np.random.RandomState(11)
    cols, n_bins, fmin, fmax = 200_000, 32, 65.0, 500.0
    f0 = rs.uniform(50.0, 600.0, size=(1, 4 * cols)).astype(np.float32)
    f0[rs.uniform(size=f0.shape) >= 0.7] = 0.0
    b64, l64, u64, voiced = R.bins_f64(f0, cols, n_bins, fmin, fmax)
    b32, l32 = R.bins_f32(f0, cols, n_bins, fmin, fmax)
    dec = R.decided(u64)
    assert int(voiced.sum()) > 0.9 * cols and not dec[~voiced].any()
    assert np.array_equal(b32[~voiced], b64[~voiced]) and not b64[~voiced].any()
    assert int((b32[dec] != b64[dec]).sum()) == 0
    undecided = voiced & ~dec
    share = undecided.sum() / voiced.sum()
    print(f"undecided share of the voiced columns: {100 * share:.4f} % ({int(undecided.sum())} of {int(voiced.sum())})")
    assert share < 1e-3                                              # (2 margin = 0.02 % expected)
    assert int(np.abs(b32[undecided] - b64[undecided]).max(initial=0)) <= 1
    assert (np.abs(l32.astype(np.float64) - l64) <= 4 * np.spacing(np.abs(l64).astype(np.float32)))[voiced].all()      # 4 fp32 ulps
    assert b64.min() == 0 and b64.max() == n_bins and set(np.unique(b64)) == set(range(n_bins + 1))
