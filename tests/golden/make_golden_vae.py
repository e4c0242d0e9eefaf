"""Generates tests/golden/vae_tiny.npz by IMPORTING the reference's continuous VAE (src/models.py:64-118) and its loss
(src/loss.py:23-29).

Runs only where the reference checkout is (never on the GPU machine, which uses the committed .npz):
    python tests/golden/make_golden_vae.py

src/train.py cannot be imported (tqdm / librosa absent), so the step below drives the reference model the way
train.py:42-83 does: zero_grad, forward, zero-pad x_tilde to the input width, loss.mse_loss(target, c, kl_d), backward,
torch.optim.Adam(lr=1e-3).step().

Configuration: VAE(1, 8, 4) under torch.manual_seed(1) (`init.*`: the state_dict as constructed), then every BatchNorm's gamma
re-drawn U(0.5, 1.5) and beta U(-0.3, 0.3) (`sd0.*`).  c = torch.rand(2, 1, 80, T) for T = 31 (odd width, ONE latent column,
BatchNorm over 28 rows) and T = 44 (5 columns).  The sample's noise is recovered by re-seeding: Normal.rsample draws
torch.empty(shape).normal_() and nothing before it in the forward consumes the generator; the script asserts
z == mu + eps * exp(.5 logvar) bit for bit.

Per T (`t31.*`, `t44.*`): c, eps, mu, logvar, x_tilde, kl, rec, grad.<parameter>, after.<state_dict key> (parameters and
BatchNorm buffers after one Adam step); f64.<the same> from a float64 copy of the model on the same eps; dead.<bias>: the
per-channel sum |dy| of the conv output's gradient (fp64) for the seven conv biases that feed a training-mode BatchNorm.
T = 44 only: traj.eps (5 steps' noise), traj.rec / traj.kl, and eval.eps / eval.x_tilde / eval.kl: the eval-mode forward after
step 1.  Before writing, the reference's own fp32 results are held to every bound tests/test_gpu_vae.py applies.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference/src")

import models as ref_models  # noqa: E402
from loss import mse_loss as ref_mse_loss  # noqa: E402
import fixture_io  # noqa: E402

torch.set_num_threads(1)        # one thread: the fp32 sums of the reference run in one order, so the file reproduces bit for bit

DEAD = ("encoder.0", "encoder.3", "encoder.6", "encoder.9", "decoder.0", "decoder.3", "decoder.6")
LOSS_RTOL, TENSOR_TOL, SUM_TOL = 1e-5, 3e-5, 2e-5


def npy(t):
    return t.detach().cpu().numpy().copy()


def forward_with_eps(model, c, eps):
    """models.py:104-118 with the sample's noise given: rsample() is loc + eps * scale."""
    mu, logvar = model.encoder(c).chunk(2, dim=1)
    q = ref_models.Normal(mu, logvar.mul(.5).exp())
    p = ref_models.Normal(torch.zeros_like(mu), torch.ones_like(logvar))
    kl = ref_models.kl_divergence(q, p).sum(1).mean()
    z = mu + eps * logvar.mul(.5).exp()
    return model.decoder(z), kl, mu, logvar, z


def padded(x_tilde, c):
    target = torch.zeros(c.size(0), c.size(1), c.size(2), c.size(3), dtype=c.dtype)      # train.py:62-64
    target[:, :, :, :x_tilde.size(3)] = x_tilde
    return target


def ref_step(model, opt, c, seed):
    """One batch of train_vae (train.py:48-75) through the reference's own forward; -> the record and the recovered noise."""
    model.train()
    opt.zero_grad()
    seen = {}
    hook = model.decoder[0].register_forward_hook(lambda m, inp, out: seen.update(z=inp[0].detach().clone()))
    torch.manual_seed(seed)
    x_tilde, kl = model(c)
    hook.remove()
    with torch.no_grad():
        mu, logvar = [t.clone() for t in seen_encoder(model, c)]
    torch.manual_seed(seed)
    eps = torch.empty(mu.shape).normal_()
    assert torch.equal(seen["z"], mu + eps * logvar.mul(.5).exp()), "the recovered noise does not reproduce the reference's sample"
    loss = ref_mse_loss(padded(x_tilde, c), c, kl)
    loss.backward()
    rec = dict(eps=eps, mu=mu, logvar=logvar, x_tilde=x_tilde.detach(), kl=kl.detach(), rec=(loss - kl).detach(),
               grads={k: p.grad.detach().clone() for k, p in model.named_parameters()})
    opt.step()
    rec["after"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return rec


def seen_encoder(model, c):
    """mu, logvar of the batch the training forward just saw: the encoder again on a copy (BatchNorm buffers untouched)."""
    m = copy.deepcopy(model).train()
    return m.encoder(c).chunk(2, dim=1)


def f64_step(sd, c, eps):
    """The same step in float64 on the same noise, plus the dead biases' sum |dy|."""
    model = ref_models.VAE(1, 8, 4).double()
    model.load_state_dict({k: v.double() for k, v in sd.items()})
    model.train()
    outs = {}
    def keep(name):
        def hook(module, inputs, output):
            output.retain_grad()
            outs[name] = output
        return hook
    hooks = [dict(model.named_modules())[n].register_forward_hook(keep(n)) for n in DEAD]
    x_tilde, kl, mu, logvar, _ = forward_with_eps(model, c.double(), eps.double())
    loss = ref_mse_loss(padded(x_tilde, c.double()), c.double(), kl)
    loss.backward()
    for h in hooks:
        h.remove()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    opt.step()
    return dict(mu=mu.detach(), logvar=logvar.detach(), x_tilde=x_tilde.detach(), kl=kl.detach(), rec=(loss - kl).detach(), grads=grads,
                after={k: v.detach().clone() for k, v in model.state_dict().items()},
                dead={n: outs[n].grad.abs().sum((0, 2, 3)) for n in DEAD})


def check_reference_meets_the_bounds(r32, r64, tag):
    for k in ("kl", "rec"):
        rel = abs(float(r32[k]) - float(r64[k])) / abs(float(r64[k]))
        assert rel <= LOSS_RTOL, (tag, k, rel)
    for k in ("mu", "logvar", "x_tilde"):
        err = float((r32[k].double() - r64[k]).abs().max()) / float(r64[k].abs().max())
        assert err <= TENSOR_TOL, (tag, k, err)
    for k, g in r32["grads"].items():
        want = r64["grads"][k]
        if k.endswith(".bias") and k[:-len(".bias")] in DEAD:
            assert bool((g.double().abs() <= SUM_TOL * r64["dead"][k[:-len(".bias")]]).all()), (tag, k)
        else:
            err = float((g.double() - want).abs().max()) / float(want.abs().max())
            assert err <= TENSOR_TOL, (tag, k, err)


def record(out, prefix, r, r64):
    for k in ("eps", "mu", "logvar", "x_tilde", "kl", "rec"):
        out[f"{prefix}.{k}"] = npy(r[k])
    for k, g in r["grads"].items():
        out[f"{prefix}.grad.{k}"] = npy(g)
    for k, v in r["after"].items():
        out[f"{prefix}.after.{k}"] = npy(v)
    for k in ("mu", "logvar", "x_tilde", "kl", "rec"):
        out[f"{prefix}.f64.{k}"] = npy(r64[k])
    for k, g in r64["grads"].items():
        out[f"{prefix}.f64.grad.{k}"] = npy(g)
    for n, v in r64["dead"].items():
        out[f"{prefix}.dead.{n}.bias"] = npy(v)


def main():
    out = {}
    torch.manual_seed(1)
    model = ref_models.VAE(1, 8, 4)
    out.update({"init." + k: npy(v) for k, v in model.state_dict().items()})
    g = torch.Generator().manual_seed(2)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.rand(m.bias.shape, generator=g) * 0.6 - 0.3
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out.update({"sd0." + k: npy(v) for k, v in sd0.items()})
    for T in (31, 44):
        c = torch.rand(2, 1, 80, T, generator=torch.Generator().manual_seed(1000 + T))
        out[f"t{T}.c"] = npy(c)
        m = ref_models.VAE(1, 8, 4)
        m.load_state_dict(sd0)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        r = ref_step(m, opt, c, seed=100)
        r64 = f64_step(sd0, c, r["eps"])
        check_reference_meets_the_bounds(r, r64, f"T={T}")
        record(out, f"t{T}", r, r64)
        if T == 44:
            # the eval-mode forward after step 1 (test_vae: running statistics, and it still samples)
            m.eval()
            torch.manual_seed(999)
            with torch.no_grad():
                mu_e, _ = m.encoder(c).chunk(2, dim=1)
                eps_e = torch.empty(mu_e.shape).normal_()
                xt_e, kl_e, _, _, _ = forward_with_eps(m, c, eps_e)
            out.update({"t44.eval.eps": npy(eps_e), "t44.eval.x_tilde": npy(xt_e), "t44.eval.kl": npy(kl_e)})
            traj = [r]
            for k in range(1, 5):
                traj.append(ref_step(m, opt, c, seed=100 + k))
            out["t44.traj.eps"] = np.stack([npy(t["eps"]) for t in traj])
            out["t44.traj.rec"] = np.array([float(t["rec"]) for t in traj], dtype=np.float64)
            out["t44.traj.kl"] = np.array([float(t["kl"]) for t in traj], dtype=np.float64)
    path = os.path.join(HERE, "vae_tiny.npz")
    paths = fixture_io.save(path, out)
    print("wrote", [(p, os.path.getsize(p)) for p in paths], len(out), "arrays")


if __name__ == "__main__":
    main()
