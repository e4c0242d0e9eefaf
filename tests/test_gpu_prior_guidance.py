"""GPU tests of classifier-free guidance in the prior's sampler (nsg_prior_walk_cfg through GatedPixelCNN.sample(guidance=,
null_label=)).  The rule is the one include/nsg.h states: the pick of nsg_prior_walk_ctl on l_c + guidance * (l_c - l_u), the
two branches walking the same codes.

The sampler's invariants make it testable to the bit: a clip's arithmetic is the same in any batch, so each branch's logits
are the teacher-forced ones of the sampled codes under that branch's label; the combination is three rounded fp32 operations
that numpy restates; the pick is held to the fp64 rule of tests/test_gpu_prior_sampling_controls.py with its caps as they are."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from neural_sound_generation_amd import _lib, ops  # noqa: E402
from neural_sound_generation_amd.evaluate import sample_mels  # noqa: E402
from neural_sound_generation_amd.prior import GatedPixelCNN  # noqa: E402
from tests.test_gpu_prior_sampling import _production  # noqa: E402
from tests.test_gpu_prior_sampling_controls import _inputs, assert_filtered_inverse_cdf, filter64, pick_status, walk  # noqa: E402,F401
from tests.test_gpu_prior_walk_envelope import N_CLASSES, _model  # noqa: E402

DEV = "cuda:0"
NEUTRAL = (1.0, 0, 1.0)
CONTROLS = (0.8, 64, 0.95)
NULL = N_CLASSES - 1                 # the last class serves as the null label
H, W = 4, 37
MODELS = {"65x32x3": (65, 32, 3), "1000x128x3": (1000, 128, 3)}     # K % 4 != 0; the 16-codes-per-lane pick at the widest dim


def _labels_and_u(P, h, w, seed):
    """Labels that are never the null class, and u: (P,), (P, h, w)."""
    return _inputs(P, h, w, seed, n_classes=N_CLASSES - 1)


def _nulls(label, null=NULL):
    return torch.full_like(label, null)


def guided_walk(model, label, shape, u, guidance, ctl=NEUTRAL, given=None, keep=None, null=NULL):
    """ops.prior_walk_cfg on the interleaved 2P clips, with the raw logits of both branches: (codes (P, h, w), logits
    (2P, h, w, K))."""
    P, (h, w) = label.shape[0], shape
    pairs = torch.stack([label, _nulls(label, null)], 1).reshape(-1)
    codes = torch.empty((P, h, w), dtype=torch.int64, device=DEV)
    logits = torch.empty((2 * P, h, w, model.embedding.num_embeddings), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        model._walk_rows(pairs, 2 * P, h, w, u=u, codes=codes, x_in=given, keep=keep, logits=logits, ctl=ctl, guidance=guidance)
    return codes, logits


def assert_the_rule(model, label, shape, u, guidance, ctl):
    """x sampled under guidance is the header's pick on l32 = lc + fp32(guidance) * (lc - lu), formed in fp32 in that order
    from the teacher-forced logits of x under the label and under the null label; the walk's own raw logits are those two."""
    P = label.shape[0]
    T, top_k, top_p = ctl
    x = model.sample(label, shape=shape, batch_size=P, u=u, temperature=T, top_k=top_k, top_p=top_p, guidance=guidance, null_label=NULL)
    assert tuple(x.shape) == (P,) + tuple(shape) and x.dtype == torch.int64
    lc = model.incremental_logits(x, label)
    lu = model.incremental_logits(x, _nulls(label))
    a, b = lc.cpu().numpy(), lu.cpu().numpy()
    d = a - b
    assert d.dtype == np.float32 and float(np.abs(d).max()) > 0, "the two branches do not differ: the case checks nothing"
    l32 = a + np.float32(guidance) * d
    assert l32.dtype == np.float32
    assert_filtered_inverse_cdf(x, torch.from_numpy(l32), u, T, top_k, top_p, max_ambiguous=0.05, max_near_clips=3)
    x2, raw = guided_walk(model, label, shape, u, guidance, ctl)
    assert torch.equal(x2, x)
    assert torch.equal(raw[0::2].view(torch.int32), lc.view(torch.int32)), "the conditional branch's logits are not the teacher-forced ones"
    assert torch.equal(raw[1::2].view(torch.int32), lu.view(torch.int32)), "the unconditional branch's logits are not the teacher-forced ones"


# ----------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctl", [NEUTRAL, CONTROLS], ids=["neutral", "controls"])
@pytest.mark.parametrize("guidance", [0.5, 3.0])
@pytest.mark.parametrize("which", list(MODELS))
def test_guided_sampling_is_the_rule_on_the_combined_logits(which, guidance, ctl):
    torch.set_num_threads(16)
    model, _ = _model(*MODELS[which])
    label, u = _labels_and_u(5, H, W, 21)
    assert_the_rule(model, label, (H, W), u, guidance, ctl)


def test_the_rule_at_production_width():
    torch.set_num_threads(16)
    model, _ = _production()
    label, u = _labels_and_u(8, 20, 32, 22)
    assert_the_rule(model, label, (20, 32), u, 2.0, NEUTRAL)


# ----------------------------------------------------------------------------------------------------------------------
# 2. exact identity: a null label equal to the clip's own label
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctl", [NEUTRAL, CONTROLS], ids=["neutral", "controls"])
@pytest.mark.parametrize("which", list(MODELS))
def test_equal_branches_are_the_unguided_sampler_bit_for_bit(which, ctl):
    """lc - lu is exactly 0, so l is lc under any guidance, and the codes are nsg_prior_walk_ctl's."""
    model, _ = _model(*MODELS[which])
    P = 5
    _, u = _labels_and_u(P, H, W, 23)
    for null in (0, 4):
        label = torch.full((P,), null, dtype=torch.int64, device=DEV)
        want = walk(model, label, (H, W), u, ctl=ctl)                       # the ctl walk, forced where the controls are neutral
        for guidance in (0.5, 3.0, 1024.0):
            got = model.sample(label, shape=(H, W), batch_size=P, u=u, temperature=ctl[0], top_k=ctl[1], top_p=ctl[2],
                               guidance=guidance, null_label=null)
            assert torch.equal(got, want), f"null_label = label = {null}, guidance {guidance}: {int((got != want).sum())} codes moved"


# ----------------------------------------------------------------------------------------------------------------------
# 3. pair independence and determinism
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(H, W), (1, 1)], ids=["4x37", "1x1"])
@pytest.mark.parametrize("P", [1, 3, 5])
@pytest.mark.parametrize("which", list(MODELS))
def test_a_pair_alone_equals_the_pair_in_the_batch(which, P, shape):
    """An odd number of pairs leaves a workgroup with one pair; every pair alone has the bits it has in the batch."""
    model, _ = _model(*MODELS[which])
    K = model.embedding.num_embeddings
    label, u = _labels_and_u(P, *shape, 24)
    g = torch.Generator().manual_seed(240)
    given = torch.randint(0, K, (P,) + shape, generator=g).to(DEV)
    keep = (torch.rand((P,) + shape, generator=g) < 0.3).to(DEV)
    args = dict(shape=shape, temperature=0.8, top_k=64, top_p=0.95, guidance=1.5, null_label=NULL)
    a = model.sample(label, batch_size=P, u=u, given=given, keep=keep, **args)
    assert torch.equal(a, model.sample(label, batch_size=P, u=u, given=given, keep=keep, **args)), "two calls differ"
    assert torch.equal(a[keep], given[keep]) and int(a.min()) >= 0 and int(a.max()) < K
    for p in range(P):
        one = model.sample(label[p:p + 1], batch_size=1, u=u[p:p + 1], given=given[p:p + 1], keep=keep[p:p + 1], **args)
        assert torch.equal(one[0], a[p]), f"pair {p}: sampled alone differs from its row in the batch"
    if shape == (H, W):
        assert not torch.equal(a, model.sample(label, batch_size=P, u=u, given=given, keep=keep, shape=shape, temperature=0.8, top_k=64,
                                               top_p=0.95)), "guidance changed nothing"


# ----------------------------------------------------------------------------------------------------------------------
# 4. priming under guidance
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(MODELS))
def test_priming_under_guidance(which):
    model, _ = _model(*MODELS[which])
    K = model.embedding.num_embeddings
    P = 5
    label, u = _labels_and_u(P, H, W, 25)
    g = torch.Generator().manual_seed(250)
    given = torch.randint(0, K, (P, H, W), generator=g).to(DEV)
    everything = torch.ones((P, H, W), dtype=torch.bool, device=DEV)
    args = dict(shape=(H, W), batch_size=P, u=u, guidance=2.0, null_label=NULL)
    # everything kept: given comes back, and both branches were walked on it
    x, raw = guided_walk(model, label, (H, W), u, 2.0, given=given, keep=everything)
    assert torch.equal(x, given)
    assert torch.equal(raw[0::2].view(torch.int32), model.incremental_logits(given, label).view(torch.int32))
    assert torch.equal(raw[1::2].view(torch.int32), model.incremental_logits(given, _nulls(label)).view(torch.int32))
    assert torch.equal(model.sample(label, given=given, keep=everything, temperature=0.7, top_p=0.5, **args), given)
    # nothing kept: the unprimed draw
    for controls in (dict(), dict(temperature=0.8, top_k=64, top_p=0.95)):
        a = model.sample(label, **args, **controls)
        assert torch.equal(model.sample(label, given=given, keep=~everything, **args, **controls), a)
        # a draw's own codes under a random mask reproduce it; what is not kept is not read
        m = (torch.rand((P, H, W), generator=g) < 0.5).to(DEV)
        assert torch.equal(model.sample(label, given=a, keep=m, **args, **controls), a)
        assert torch.equal(model.sample(label, given=torch.where(m, a, (a + 1) % K), keep=m, **args, **controls), a)
    # continue_codes keeps the prefix and is sample with the prefix columns kept
    W0 = 9
    prefix = given[:, :, :W0].contiguous()
    out = model.continue_codes(prefix, label, W, u=u, top_k=100, guidance=2.0, null_label=NULL)
    assert tuple(out.shape) == (P, H, W) and torch.equal(out[:, :, :W0], prefix)
    keep = torch.zeros((P, H, W), dtype=torch.bool, device=DEV)
    keep[:, :, :W0] = True
    assert torch.equal(out, model.sample(label, given=torch.where(keep, given, torch.zeros_like(given)), keep=keep, top_k=100, **args))
    assert not torch.equal(out, model.continue_codes(prefix, label, W, u=u, top_k=100)), "guidance changed nothing"


# ----------------------------------------------------------------------------------------------------------------------
# 5. dispatch: guidance = 0 is the sampler as it was, through the same launches
# ----------------------------------------------------------------------------------------------------------------------
def test_no_guidance_takes_the_existing_dispatch(monkeypatch):
    model, _ = _model(65, 32, 3)
    B = 5
    label, u = _labels_and_u(B, H, W, 26)
    plain = model.sample(label, shape=(H, W), batch_size=B, u=u)
    controlled = model.sample(label, shape=(H, W), batch_size=B, u=u, temperature=0.8, top_k=64, top_p=0.95)
    calls = []

    def counted(name):
        real = getattr(ops, name)

        def f(w, emb, cond, *a, **k):
            calls.append((name, cond.shape[1]))
            return real(w, emb, cond, *a, **k)
        return f

    def unreachable(*a, **k):
        raise AssertionError("guidance = 0 reached the guided walk")

    monkeypatch.setattr(ops, "prior_walk", counted("prior_walk"))
    monkeypatch.setattr(ops, "prior_walk_ctl", counted("prior_walk_ctl"))
    monkeypatch.setattr(ops, "prior_walk_cfg", unreachable)
    for guidance in (0, 0.0):
        assert torch.equal(model.sample(label, shape=(H, W), batch_size=B, u=u, guidance=guidance), plain)
        assert torch.equal(model.sample(label, shape=(H, W), batch_size=B, u=u, temperature=0.8, top_k=64, top_p=0.95, guidance=guidance),
                           controlled)
    assert calls == ([("prior_walk", B)] * H + [("prior_walk_ctl", B)] * H) * 2, calls


# ----------------------------------------------------------------------------------------------------------------------
# 6. validation, before any launch
# ----------------------------------------------------------------------------------------------------------------------
def test_guidance_is_validated_before_a_launch(monkeypatch):
    model, _ = _model(65, 32, 3)
    B, h, w = 2, 3, 5
    label, u = _labels_and_u(B, h, w, 27)
    K, dim, L = 65, 32, 3
    blob = model._walk_blob(K)
    emb = model.embedding.weight.detach().contiguous()

    def unreachable(*a, **k):
        raise AssertionError("an entry point was reached")

    monkeypatch.setattr(_lib, "call", unreachable)
    args = dict(shape=(h, w), batch_size=B, u=u)
    for bad in (dict(guidance=True, null_label=NULL), dict(guidance="strong", null_label=NULL), dict(guidance=math.nan, null_label=NULL),
                dict(guidance=math.inf, null_label=NULL), dict(guidance=-0.5, null_label=NULL), dict(guidance=1024.5, null_label=NULL),
                dict(guidance=2.0), dict(guidance=0.0, null_label=NULL), dict(null_label=NULL), dict(guidance=2.0, null_label=N_CLASSES),
                dict(guidance=2.0, null_label=-1), dict(guidance=2.0, null_label=1.0), dict(guidance=2.0, null_label=True)):
        with pytest.raises(ValueError):
            model.sample(label, **args, **bad)
        with pytest.raises(ValueError):
            model.continue_codes(torch.zeros((B, h, 2), dtype=torch.int64, device=DEV), label, w, **bad)
    # ops.prior_walk_cfg: an odd number of clips, a bad guidance, per-pair tensors of the clips' extent
    def tensors(n):
        return (torch.zeros((L, n, 2 * dim), device=DEV), torch.zeros((L, n, 1, w, 2 * dim), device=DEV), torch.zeros((n, w, dim), device=DEV))

    cond, vh, e_row = tensors(4)
    up, codes = torch.rand((2, h, w), device=DEV), torch.zeros((2, h, w), dtype=torch.int64, device=DEV)
    with pytest.raises(AssertionError):                                      # the good call reaches the entry point
        ops.prior_walk_cfg(blob, emb, cond, vh, e_row, h, 0, up, codes, 2.0)
    for guidance in (math.nan, math.inf, -1.0, 1025.0):
        with pytest.raises(_lib.NsgError):
            ops.prior_walk_cfg(blob, emb, cond, vh, e_row, h, 0, up, codes, guidance)
    with pytest.raises(_lib.NsgError):
        ops.prior_walk_cfg(blob, emb, *tensors(3), h, 0, up, codes, 2.0)
    u4, codes4 = torch.rand((4, h, w), device=DEV), torch.zeros((4, h, w), dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.NsgError):
        ops.prior_walk_cfg(blob, emb, cond, vh, e_row, h, 0, u4, codes, 2.0)
    with pytest.raises(_lib.NsgError):
        ops.prior_walk_cfg(blob, emb, cond, vh, e_row, h, 0, up, codes4, 2.0)
    with pytest.raises(_lib.NsgError):
        ops.prior_walk_cfg(blob, emb, cond, vh, e_row, h, 0, up, codes, 2.0, x_in=codes)
    with pytest.raises(_lib.NsgError):
        ops.prior_walk_cfg(blob, emb, cond, vh, e_row, h, 0, up, codes, 2.0, temperature=0.0)


# ----------------------------------------------------------------------------------------------------------------------
# 7. the keywords pass through sample_mels
# ----------------------------------------------------------------------------------------------------------------------
def test_sample_mels_passes_guidance_through():
    from neural_sound_generation_amd import models as M
    torch.manual_seed(2)
    vqvae = M.VQVAE(1, 32, 64).to(DEV).eval()
    prior = GatedPixelCNN(64, 16, 2, 4).to(DEV)
    label = torch.tensor([0, 2, 1], device=DEV)
    codes, mels = sample_mels(vqvae, prior, label, 48, generator=torch.Generator(device=DEV).manual_seed(7), top_p=0.9, guidance=1.5,
                              null_label=3)
    want = prior.sample(label, shape=(20, 12), batch_size=3, generator=torch.Generator(device=DEV).manual_seed(7), top_p=0.9, guidance=1.5,
                        null_label=3)
    assert torch.equal(codes, want) and tuple(mels.shape) == (3, 1, 80, 48)
    assert not torch.equal(codes, prior.sample(label, shape=(20, 12), batch_size=3, generator=torch.Generator(device=DEV).manual_seed(7), top_p=0.9))
