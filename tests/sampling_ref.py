"""Plain-torch float64 restatement of the sampling head with controls (csrc/k_head.h, sample_head_ctl_kernel), for the tests:
mask -> temperature -> top-k -> top-p -> inverse-CDF pick from a given uniform, and the two log-probs.  No device, no library.

Order and rules are HF's (TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper with min_tokens_to_keep=1):
  s = masked / temperature (a true division);
  top-k keeps s >= the k-th largest value, duplicates counted (0: no filter);
  top-p orders what is left by probability descending, lower id first among equals, and keeps a candidate iff the probability mass
  strictly ahead of it is < top_p (the first is always kept);
  the draw is the inverse CDF over the kept candidates in ascending token id.
"""
import math

import torch


def grammar_mask(grammar, t, counter, V, eos=2):
    """Allowed ids of the device grammars (0 none, 1 NAIVE9, 2 LR_ABSCO) at step t with the counter AFTER its update: bool [V]."""
    ok = torch.ones(V, dtype=torch.bool)
    i = torch.arange(V)
    if grammar == 2:
        if t == 0:
            ok = i == 5
        elif counter > 0:
            ok = i >= 6
        else:
            ok = (i == 3) | (i == 4) | (i == 5) | (i == eos)
    elif grammar == 1:
        ok = (i >= 3) | ((i == eos) & (t % 9 == 1))
    return ok


def filtered(masked, temperature=1.0, top_k=0, top_p=1.0):
    """masked: float [V] with -inf where forbidden.  Returns (s, keep, margin): the scaled scores in float64, the bool [V] kept set and
    the smallest |mass ahead of a candidate - top_p| over the finite candidates that reach the top-p step (inf when top_p == 1)."""
    s = masked.double() / float(temperature)
    finite = torch.isfinite(s)
    keep = finite.clone()
    if top_k > 0:
        k = min(int(top_k), s.numel())
        kth = torch.topk(s, k).values[-1]
        keep &= s >= kth
    margin = math.inf
    if top_p < 1.0:
        cand = torch.nonzero(keep).flatten()
        p = torch.softmax(s[cand], dim=0)
        order = torch.sort(p, descending=True, stable=True).indices        # stable: lower id first among equals
        ahead = torch.cumsum(p[order], dim=0) - p[order]
        stay = ahead < top_p
        stay[0] = True
        keep = torch.zeros_like(keep)
        keep[cand[order[stay]]] = True
        margin = float((ahead - top_p).abs().min())
    return s, keep, margin


def policy_logprobs(s, keep):
    """log of the renormalised probabilities over the kept set: float64 [V], -inf outside."""
    return torch.log_softmax(torch.where(keep, s, torch.full_like(s, -math.inf)), dim=0)


def pick(s, keep, u):
    """Inverse CDF in ascending token id: the first kept id whose inclusive cumulative probability exceeds u (the last kept id when
    rounding leaves none).  Also returns the inclusive CDF over all ids (float64 [V])."""
    p = policy_logprobs(s, keep).exp()
    cdf = torch.cumsum(p, dim=0)
    hit = torch.nonzero(keep & (cdf > u)).flatten()
    idx = int(hit[0]) if len(hit) else int(torch.nonzero(keep).flatten()[-1])
    return idx, cdf


def model_logprobs(logits):
    """log_softmax of the raw row in float64: what LMM.score reports as -nll."""
    return torch.log_softmax(logits.double(), dim=0)
