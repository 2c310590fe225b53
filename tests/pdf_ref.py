"""Torch restatement of the inverse-CDF hierarchical sampler (csrc/sample_pdf.hip; include/mcnerf.h: mcnerf_sample_pdf), the
checker of the `fine_sampler = "pdf"` tests.  The reference has no such sampler (its fine pass is the weight-threshold
refinement), so this is the sampler's contract written out in tensor ops, not reference code; the fine pass on its depths is
checked with the oracle's general `inference()` / `composite()`, which take any [N,S] `z_vals`."""
import torch


def pdf_cdf_ref(w):
    """w [N,Sc] coarse selection weights -> (pdf [N,Sc-2], cdf [N,Sc-1]) of the interior bins, cdf[:, 0] = 0."""
    wb = w.float()[:, 1:-1] + 1e-5                                        # interior weights, floored [N, Sc-2]
    # the total and the running sums are the correctly rounded ones (fp64 accumulation, one rounding to fp32): the sampler's CDF does
    # not depend on the order of a sum
    pdf = wb / wb.double().sum(-1, keepdim=True).float()
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf.double(), -1).float()], -1)       # [N, Sc-1]
    return pdf, cdf


def sample_pdf_ref(w, zgrid, jitter, u):
    """w [N,Sc] coarse selection weights, zgrid [Sc], jitter [N] / [N,1] or None, u [N,I] in [0,1] (any order)
    -> (z_all [N,Sc+I] sorted, zs [N,I] the importance samples in u's order, zc [N,Sc] the coarse depths)."""
    N, Sc = w.shape
    w, u = w.float(), u.float()
    jit = torch.zeros(N, dtype=torch.float32, device=w.device) if jitter is None else jitter.reshape(N).float()
    zc = zgrid.reshape(1, Sc).float() + jit.unsqueeze(1)                 # the coarse pass's depths (one fp32 rounding)
    mid = 0.5 * (zc[:, :-1] + zc[:, 1:])                                  # bin edges [N, Sc-1]
    pdf, cdf = pdf_cdf_ref(w)
    ind = torch.searchsorted(cdf, u.contiguous(), right=True)             # #{i : cdf[i] <= u}
    below = (ind - 1).clamp(min=0)
    above = ind.clamp(max=Sc - 2)
    interior = (ind >= 1) & (ind <= Sc - 2)
    denom = torch.where(interior, pdf.gather(1, (ind - 1).clamp(0, Sc - 3)), torch.zeros_like(u))     # the bin's own pdf entry
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf.gather(1, below)) / denom
    m_lo, m_hi = mid.gather(1, below), mid.gather(1, above)
    zs = m_lo + t * (m_hi - m_lo)
    return torch.sort(torch.cat([zc, zs], -1), -1).values, zs, zc


def split_rows(z_all, zc):
    """The device's sorted rows z_all [N,Sc+I] -> (zs_sorted [N,I], zc_found [N,Sc]): the coarse depths are taken out at the places a
    merge that puts a coarse depth before an equal sample gives them (j + #{z_all < zc[j]} - #{zc < zc[j]})."""
    N, T = z_all.shape
    Sc = zc.shape[1]
    j = torch.arange(Sc, device=z_all.device).expand(N, -1)
    pos = j + torch.searchsorted(z_all.contiguous(), zc.contiguous()) - torch.searchsorted(zc.contiguous(), zc.contiguous())
    pos = pos.clamp(0, T - 1)
    keep = torch.ones(N, T, dtype=torch.bool, device=z_all.device)
    keep.scatter_(1, pos, False)
    assert bool((keep.sum(1) == T - Sc).all()), "a row of z_all does not hold its coarse depths at distinct places"
    return z_all[keep].reshape(N, T - Sc), z_all.gather(1, pos)
