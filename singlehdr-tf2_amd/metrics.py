"""Validation metrics on the device: is a checkpoint any good?

    ev = metrics.Evaluator()
    for ldr, hdr in batches:
        ev.update(inference(ldr), hdr)            # two launches per batch, no host synchronisation
    print(ev.result())                            # ONE host read: {"images", "psnr_l", "psnr_mu", "ssim_mu", "l1_logc", ...}

The numbers (csrc/metrics.hip, include/shdr.h "validation metrics"; DESIGN.md "Validation metrics"), per image:

  * both images are mean-normalised like the fine-tuning data (finetune_real_dataset.py:47,173: x * 0.5 / (1e-6 + mean(x)); switch it
    off with normalise=False for images that share an absolute scale), clamped at 0; `peak` is the ground truth's maximum;
  * psnr_l   = -10 log10( mean((p - g)^2) / peak^2 )                       PSNR of the linear values
  * psnr_mu  = -10 log10( mean((T(p) - T(g))^2) ),  T(x) = log(1 + mu min(x / peak, 1)) / log(1 + mu),  mu = 5000
  * ssim_mu  = SSIM (Wang et al. 2004; 11x11 Gaussian of sigma 1.5, valid windows, C1 = 1e-4, C2 = 9e-4) of T(p) against T(g)
  * l1_logc  = mean |logc(p) - logc(g)|, the fine-tuning loss (joint_training.py:166-173): a validation number in the units of the
    training curve.

An all-black ground truth has peak 0: its metrics are the IEEE results (NaN / inf), and an Evaluator that has seen one reports them.
"""
import math

import torch

try:
    from . import _ops as K
except ImportError:
    import _ops as K


def hdr_metrics(pred, gt, normalise=True, mu=5000.0):
    """K.hdr_metrics plus psnr_l and psnr_mu: a dict of float64 device tensors [N]; no host synchronisation"""
    m = K.hdr_metrics(pred, gt, normalise, mu)
    m["psnr_l"] = -10.0 * torch.log10(m["mse_l"])
    m["psnr_mu"] = -10.0 * torch.log10(m["mse_mu"])
    return m


class Evaluator:
    """Running means of the per-image metrics.  `state` is ONE float64 device tensor
        [images, sum psnr_l, sum psnr_mu, sum ssim_mu, sum l1_logc, -min psnr_l, -min psnr_mu]
    (the minima are kept negated: the sums are combined over ranks by an all-reduce SUM of state[:5], the minima by an all-reduce MAX
    of state[5:]; no collective is issued here).  update() never synchronises; result() reads the state once."""

    SUMS = ("psnr_l", "psnr_mu", "ssim_mu", "l1_logc")

    def __init__(self, normalise=True, mu=5000.0):
        self.normalise, self.mu = normalise, mu
        self.state = None

    def reset(self):
        self.state = None

    def update(self, pred, gt):
        m = hdr_metrics(pred, gt, self.normalise, self.mu)
        if self.state is None:
            self.state = torch.zeros(7, device=m["psnr_l"].device, dtype=torch.float64)
            self.state[5:] = -math.inf
        per = torch.stack([m[k] for k in self.SUMS])                                  # [4, N]
        self.state[0] += per.shape[1]
        self.state[1:5] += per.sum(dim=1)
        self.state[5:] = torch.maximum(self.state[5:], (-per[:2]).amax(dim=1))
        return m

    def result(self):
        if self.state is None:
            raise RuntimeError("Evaluator.result: no images yet")
        s = self.state.cpu().tolist()
        out = {"images": int(s[0])}
        for i, k in enumerate(self.SUMS):
            out[k] = s[1 + i] / s[0]
        out["psnr_l_min"], out["psnr_mu_min"] = -s[5], -s[6]
        return out
