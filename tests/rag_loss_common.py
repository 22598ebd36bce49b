"""Shared by tests/test_rag_loss_host.py and tests/test_rag_loss_gpu.py (and profiles/rag_loss_probe.py): the fixture's cases,
a torch restatement of the marginalised loss (`RagModelForBlip.get_loss`, rag_model_blip.py:826-1026, written out here: the full
log_softmax, the `cat` with the document term at position p, two gathers -- the expression the fused pair replaces; it does not
touch the caller's target), and the error yardstick.

Yardstick for ll, lse and the gradients: e_ref = the error of an fp32 torch evaluation against the fp64 evaluation of the same
inputs; the code under test may be at most 2 x e_ref off the fp64 values (both are fp32 evaluations with one rounding per
operation: another summation order cannot be asked to beat torch, only to stay in its class).
Scalar losses: a single number's e_ref can be anything from 0 to half an ulp by luck, so a scalar gets, beside 2 x e_ref, the
a-priori bound of an fp32 sum of its n terms in any order, n * 2^-24 * sum|terms| (Higham, Accuracy and Stability of Numerical
Algorithms, eq. 4.4), divided by the count where the loss is a mean."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import ROOT

LOSS_TYPES = ["Approach1", "Approach2", "Approach3", "Approach4", "Approach5", "Approach6", "NoPR"]
U32 = 2.0 ** -24
_cases = None


def fixture_cases():
    """name -> dict(logits, doc_scores, target, retrieval_labels | None, n_docs, bos, loss_type, reduce_loss, f32={...}, f64={...})"""
    global _cases
    if _cases is None:
        z = dict(np.load(os.path.join(ROOT, "tests", "golden", "rag_loss.npz")))
        _cases = {}
        for name in sorted(k[:-5] for k in z if k.endswith(".meta")):
            src = str(z[name + ".inputs_of"]) if name + ".inputs_of" in z else name
            n_docs, bos, lt, red = (int(v) for v in z[name + ".meta"])
            c = dict(logits=z[src + ".logits"], doc_scores=z[src + ".doc_scores"], target=z[src + ".target"],
                     retrieval_labels=z.get(src + ".retrieval_labels"), n_docs=n_docs, bos=None if bos < 0 else bos,
                     loss_type=LOSS_TYPES[lt], reduce_loss=bool(red))
            for tag in ("f32", "f64"):
                c[tag] = {k: z[f"{name}.{tag}.{k}"] for k in ("nll_loss", "rag_loss", "additional_loss", "ddoc_scores")}
                c[tag]["dlogits"] = z[f"{src}.{tag}.dlogits"]
            _cases[name] = c
    return _cases


def restate_ll(logits, target, ignore_index=-100):
    """(ll [R, T], lse [R, T, 2] = (row maximum, log sum exp(x - maximum)), first_argmax [R]) in the logits' dtype by the full
    log_softmax; ignored positions 0."""
    pad = target == ignore_index
    ll = F.log_softmax(logits, dim=-1).gather(-1, target.masked_fill(pad, 0).unsqueeze(-1)).squeeze(-1).masked_fill(pad, 0.0)
    m = logits.max(-1).values
    lse = torch.stack([m, (logits - m.unsqueeze(-1)).exp().sum(-1).log()], dim=-1).masked_fill(pad.unsqueeze(-1), 0.0)
    return ll, lse, logits[:, 0].argmax(-1)


def restate_loss(seq_logits, doc_scores, target, n_docs, bos_token_id=None, ignore_index=-100, retrieval_labels=None, loss_type=None,
                 reduce_loss=True):
    """The marginalised loss as the reference's torch expression, in seq_logits' dtype, target untouched -> dict of three."""
    R, T, V = seq_logits.shape
    B = R // n_docs
    use_bos = bos_token_id is not None and bool(target[:, 0].eq(bos_token_id).all())
    seq_logprobs = F.log_softmax(seq_logits, dim=-1).view(B, n_docs, T, V)
    doc_logprobs = F.log_softmax(doc_scores.to(seq_logits.dtype), dim=1).unsqueeze(-1).unsqueeze(-1)
    first = seq_logprobs[:, :, :1]
    if use_bos:
        rag_logprobs = torch.cat([first, seq_logprobs[:, :, 1:2] + doc_logprobs, seq_logprobs[:, :, 2:]], dim=2)
    else:
        rag_logprobs = torch.cat([first + doc_logprobs, seq_logprobs[:, :, 1:]], dim=2)
    pad = target.view(B, n_docs, T, 1) == ignore_index
    index = target.view(B, n_docs, T, 1).masked_fill(pad, 0) if ignore_index < 0 else target.view(B, n_docs, T, 1)
    ll = seq_logprobs.gather(-1, index).masked_fill(pad, 0.0).squeeze(-1)
    rag_ll = rag_logprobs.gather(-1, index).masked_fill(pad, 0.0).squeeze(-1)
    out = {"nll_loss": -ll.sum() / (~pad).sum() if reduce_loss else -ll, "rag_loss": -rag_ll.sum(2).logsumexp(1).sum()}
    if retrieval_labels is None:
        out["additional_loss"] = doc_scores.new_zeros(())
        return out
    pred = (first.detach().squeeze(2).argmax(-1) == index[:, :, 0, 0])
    ret = retrieval_labels.to(seq_logits.device) != 0
    either, both = pred | ret, pred & ret
    merged, ignore = {"Approach1": (either, ~either), "Approach2": (either, pred & ~ret), "Approach3": (either, ~ret),
                      "Approach4": (ret, pred & ~ret), "Approach5": (both, ~both), "Approach6": (both, pred ^ ret),
                      "NoPR": (pred, torch.zeros_like(pred))}[loss_type]
    probs = F.softmax(doc_scores, dim=-1)
    dist = F.binary_cross_entropy(probs, merged.to(probs.dtype), reduction="none").masked_fill(ignore, 0.0)
    n = torch.count_nonzero(dist)
    out["additional_loss"] = dist.sum() / n if int(n) else doc_scores.new_zeros(())
    return out


def total_of(losses):
    """The scalar the fixture differentiated: nll_loss (summed where it is not reduced) + rag_loss + additional_loss."""
    return losses["nll_loss"].sum() + losses["rag_loss"] + losses["additional_loss"]


def ratio(got, f32, f64):
    """(error of `got` against f64, e_ref = error of f32 against f64), maxima over the elements."""
    got, f32, f64 = (np.asarray(v, dtype=np.float64) for v in (got, f32, f64))
    assert got.shape == f64.shape == f32.shape, (got.shape, f32.shape, f64.shape)
    assert np.isfinite(got).all()
    return float(np.max(np.abs(got - f64), initial=0.0)), float(np.max(np.abs(f32 - f64), initial=0.0))


def assert_in_class(got, f32, f64, what, extra=0.0):
    """err(got) <= 2 x e_ref (+ `extra`, the a-priori summation bound of a scalar), printed before it is asserted."""
    err, e_ref = ratio(got, f32, f64)
    print(f"{what}: err {err:.3e}  e_ref {e_ref:.3e}  ratio {err / e_ref if e_ref else float('inf') if err else 0.0:.2f}"
          + (f"  (+ {extra:.3e})" if extra else ""))
    assert err <= 2.0 * e_ref + extra, f"{what}: err {err:.3e} > 2 x e_ref {e_ref:.3e}" + (f" + {extra:.3e}" if extra else "")
    return err, e_ref


def scalar_bounds(case):
    """The a-priori fp32 summation bounds of the three scalar losses of a fixture case, from its fp64 record."""
    c = case
    x, t = torch.from_numpy(c["logits"]).double(), torch.from_numpy(c["target"])
    ll, _, _ = restate_ll(x, t)
    n, s = int((t != -100).sum()), float(ll.abs().sum())
    docs = c["doc_scores"].size
    bound = n * U32 * s
    return {"nll_loss": bound / max(n, 1) if c["reduce_loss"] else 0.0, "rag_loss": bound,
            "additional_loss": docs * U32 * abs(float(c["f64"]["additional_loss"]))}


class TorchOps:
    """torch stand-ins of ops.rag_token_ll_fwd / _bwd / checked_rag_targets on the CPU, fp32 arithmetic, recording the calls."""

    def __init__(self):
        self.calls = []
        from ravqa_amd import ops
        self._check = ops.checked_rag_targets

    def checked_rag_targets(self, target, R, T, V, ignore_index, device):
        return self._check(target, R, T, V, ignore_index, "cpu")

    def rag_token_ll_fwd(self, logits, target, ignore_index=-100):
        self.calls.append(("fwd", logits.dtype, tuple(logits.shape)))
        R, T, V = logits.shape
        tgt = self.checked_rag_targets(target, R, T, V, ignore_index, "cpu")
        ll, lse, first = restate_ll(logits.float(), tgt, ignore_index)
        return ll, lse, first.int()

    def rag_token_ll_bwd(self, logits, target, lse, grad_ll, ignore_index=-100, out=None):
        self.calls.append(("bwd", logits.dtype, tuple(logits.shape)))
        pad = (target == ignore_index).unsqueeze(-1)
        onehot = F.one_hot(target.masked_fill(pad.squeeze(-1), 0), logits.size(-1)).float()
        d = grad_ll.float().unsqueeze(-1) * (onehot - torch.exp((logits.float() - lse[..., :1]) - lse[..., 1:]))
        return d.masked_fill(pad, 0.0).to(logits.dtype)
