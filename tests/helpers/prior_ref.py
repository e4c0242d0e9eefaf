"""What several GPU modules of the latent prior share: the tiny fixture's model and the fp64 cross-entropy (moved here verbatim
from tests/test_gpu_prior.py and tests/test_gpu_prior_width.py, which import them back)."""
import numpy as np
import torch

from neural_sound_generation_amd.prior import GatedPixelCNN

DEV = "cuda:0"


def build(g):
    input_dim, dim, n_layers, n_classes = (int(v) for v in g["cfg"])
    m = GatedPixelCNN(input_dim, dim, n_layers, n_classes)
    m.load_state_dict({k[4:]: torch.from_numpy(np.array(g[k])) for k in g.files if k.startswith("sd0.")})
    return m.to(DEV), n_layers


def _ce64(l, t, grad_scale):
    """fp64 mean cross-entropy and its gradient on the fp32 logits, written so that nothing rounds at the scale of the row's
    maximum mx = l[a]: with s = sum over k != a of exp(l[k] - mx), a row's loss is (mx - l[t]) + log1p(s), its softmax
    exp(l[k] - mx) / (1 + s), and the gradient at a confident target -s / (1 + s).  (fp64 F.cross_entropy forms
    mx + log(1 + s) - l[t]: on a row 30 above the rest that keeps a few digits of a 1e-13 loss.  It is held to this
    closed form below, within its own rounding.)"""
    l64 = l.double()
    M, K = l64.shape
    rows = torch.arange(M, device=l.device)
    a = torch.argmax(l64, dim=1)                        # the first index of the maximum
    mx = l64[rows, a]
    e = torch.exp(l64 - mx[:, None])
    e[rows, a] = 0.0
    s = e.sum(dim=1)
    loss = ((mx - l64[rows, t]) + torch.log1p(s)).mean()
    e[rows, a] = 1.0
    g = e / (1.0 + s)[:, None]
    g[rows, t] -= 1.0
    at = a == t
    g[rows[at], t[at]] = -s[at] / (1.0 + s[at])
    return loss, g * (grad_scale / M)
