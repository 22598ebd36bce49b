#!/usr/bin/env python3
"""Golden vectors for rag.marginalised_loss / rag.token_log_likelihood (flmr_rag_token_ll_fwd / _bwd): the REFERENCE's own
`RagModelForBlip.get_loss` (src/models/rag/rag_model_blip.py:826-1026), taken from its checkout at generation time -- the module
is parsed with `ast`, that one function definition is compiled and run with torch, nn, F and a small attribute-dict in its
namespace, so none of the module's other dependencies is imported -- on CPU tensors under torch's autograd.  `self` is a
SimpleNamespace holding config.model_config.{num_knowledge_passages, loss_ratio, RAVQA_loss_type} and
generator.config.bos_token_id.

    python tests/golden/make_golden_rag_loss.py      # writes tests/golden/rag_loss.npz

Every case is run twice: on fp32 inputs, and on the same values as fp64 (the yardstick the fp32 run's own error is measured
against).  Recorded per case and precision: nll_loss, rag_loss, additional_loss, and the gradients of
nll_loss (summed if not reduced) + rag_loss + additional_loss with respect to the logits and doc_scores.  The reference mutates
its `target` argument; it is handed a copy.

Cases (B = 3, n_docs = 4, T = 6, V in {37, 97} unless the name says otherwise): bos_token_id None and set; the seven loss types;
a row ignored from position 3 on; a fully ignored row; position p ignored (bos None); position 0 ignored; retrieval_labels None; an
additional_loss whose count is zero; n_docs = 1; T = 1 with and without bos; reduce_loss=False.  The first position's logits are
redrawn until their top-two gap is >= 1e-3, so no rounding can flip `first_token_prediction`; half of the rows have that winner
planted as their first target (so prediction_labels holds both values); one row of `tie` has an exact tie, whose lowest index is
recorded (`tie.first_argmax`).  The seven loss types of one bos setting share one draw of inputs (stored once, with the
logits' gradient, which no loss type changes).  Only DATA is written, kept under 1 MiB.
"""
import ast
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FLMR_REFERENCE_ROOT", "/root/reference")
GAP = 1e-3
LOSS_TYPES = ["Approach1", "Approach2", "Approach3", "Approach4", "Approach5", "Approach6", "NoPR"]


class EasyDict(dict):
    def __getattr__(self, k):
        return self[k]

    def __setattr__(self, k, v):
        self[k] = v


def reference_get_loss():
    path = os.path.join(REF, "src", "models", "rag", "rag_model_blip.py")
    tree = ast.parse(open(path).read(), path)
    fn = next(n for c in tree.body if isinstance(c, ast.ClassDef) and c.name == "RagModelForBlip"
              for n in c.body if isinstance(n, ast.FunctionDef) and n.name == "get_loss")
    # (its `F` is torch's, except that binary_cross_entropy takes the fp32 labels `.float()` yields beside fp64 scores: the cast
    # is to the scores' dtype, a no-op in the fp32 run)
    bce = lambda inp, tgt, **kw: F.binary_cross_entropy(inp, tgt.to(inp.dtype), **kw)
    Fns = SimpleNamespace(softmax=F.softmax, log_softmax=F.log_softmax, binary_cross_entropy=bce)
    ns = {"torch": torch, "nn": nn, "F": Fns, "EasyDict": EasyDict}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["get_loss"]


GET_LOSS = reference_get_loss()


def run(logits, doc_scores, target, n_docs, bos, labels, loss_type, reduce_loss, dtype):
    me = SimpleNamespace(config=SimpleNamespace(model_config=SimpleNamespace(
        num_knowledge_passages=n_docs, loss_ratio=EasyDict(nll_loss=1, rag_loss=1, additional_loss=1), RAVQA_loss_type=loss_type)),
        generator=SimpleNamespace(config=SimpleNamespace(bos_token_id=bos)))
    x = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    s = torch.from_numpy(doc_scores).to(dtype).requires_grad_(True)
    d = GET_LOSS(me, seq_logits=x, doc_scores=s, target=torch.from_numpy(target).clone(), reduce_loss=reduce_loss, n_docs=n_docs,
                 retrieval_labels=None if labels is None else torch.from_numpy(labels))
    total = d.nll_loss.sum() + d.rag_loss + d.additional_loss
    total.backward()
    val = lambda v: v.detach().numpy() if torch.is_tensor(v) else np.asarray(float(v))
    return {"nll_loss": val(d.nll_loss), "rag_loss": val(d.rag_loss), "additional_loss": val(d.additional_loss),
            "dlogits": x.grad.numpy(), "ddoc_scores": s.grad.numpy() if s.grad is not None else np.zeros_like(doc_scores)}


def draw(rng, B, n_docs, T, V, bos=None, ignore_index=-100):
    R = B * n_docs
    logits = (3.0 * rng.standard_normal((R, T, V))).astype(np.float32)
    for r in range(R):
        while True:
            top = np.sort(logits[r, 0].astype(np.float64))
            if top[-1] - top[-2] >= GAP:
                break
            logits[r, 0] = (3.0 * rng.standard_normal(V)).astype(np.float32)
    target = rng.integers(0, V, (R, T)).astype(np.int64)
    target[::2, 0] = logits[::2, 0].argmax(-1)              # half of the first targets are the predicted token
    if bos is not None:
        target[:, 0] = bos
        logits[::2, 0, bos] = logits[::2, 0].max(-1) + 1.0   # ... and under bos, half of the rows predict it
    doc_scores = (10.0 + 4.0 * rng.standard_normal((B, n_docs))).astype(np.float32)
    labels = (rng.random((B, n_docs)) < 0.5).astype(np.int64)
    return logits, doc_scores, target, labels


def case(out, name, logits, doc_scores, target, labels, n_docs, bos=None, loss_type="Approach6", reduce_loss=True, inputs_of=None):
    """inputs_of: the case that already holds these inputs (and dlogits, which no loss type changes); only the name is stored."""
    if inputs_of is None:
        out[f"{name}.logits"], out[f"{name}.doc_scores"], out[f"{name}.target"] = logits, doc_scores, target
        if labels is not None:
            out[f"{name}.retrieval_labels"] = labels
    else:
        out[f"{name}.inputs_of"] = np.array(inputs_of)
    out[f"{name}.meta"] = np.array([n_docs, -1 if bos is None else bos, LOSS_TYPES.index(loss_type), int(reduce_loss)], dtype=np.int64)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        for k, v in run(logits, doc_scores, target, n_docs, bos, labels, loss_type, reduce_loss, dtype).items():
            if inputs_of is not None and k == "dlogits":
                assert np.array_equal(v, out[f"{inputs_of}.{tag}.dlogits"])
                continue
            out[f"{name}.{tag}.{k}"] = v


def main():
    rng = np.random.default_rng(20261018)
    out = {}
    B, n_docs, T = 3, 4, 6
    IGN = -100
    # the seven rules, bos None (V = 37) and set (V = 97), with a row ignored from position 3 on and a fully ignored row
    for bos, V in ((None, 37), (5, 97)):
        x, s, t, lab = draw(rng, B, n_docs, T, V, bos)
        t[1, 3:] = IGN
        if bos is None:
            t[6, :] = IGN
        else:
            t[6, 1:] = IGN       # (under bos the first target stays bos; the rest of the row is ignored)
        names = [f"{lt}_bos{'None' if bos is None else bos}" for lt in LOSS_TYPES]
        for lt, name in zip(LOSS_TYPES, names):
            case(out, name, x, s, t, lab, n_docs, bos, lt, inputs_of=None if name == names[0] else names[0])
    # position p ignored (bos None: p = 0), in some rows only
    x, s, t, lab = draw(rng, B, n_docs, T, 37)
    t[[0, 5, 9], 0] = IGN
    case(out, "p_ignored", x, s, t, lab, n_docs, None, "Approach6")
    # position 0 ignored in every row of one question, and a bos that then no longer holds everywhere (use_bos false)
    x, s, t, lab = draw(rng, B, n_docs, T, 97, bos=5)
    t[4:8, 0] = IGN
    case(out, "pos0_ignored_bos_broken", x, s, t, lab, n_docs, 5, "NoPR")
    # position 1 ignored under bos (the document term disappears for those rows)
    x, s, t, lab = draw(rng, B, n_docs, T, 97, bos=5)
    t[[2, 3, 10], 1] = IGN
    case(out, "p1_ignored_bos", x, s, t, lab, n_docs, 5, "Approach2")
    # retrieval_labels None
    x, s, t, lab = draw(rng, B, n_docs, T, 37)
    case(out, "no_labels", x, s, t, None, n_docs, None, "Approach1")
    # additional_loss count zero: Approach5 with no positive label ignores every document
    x, s, t, lab = draw(rng, B, n_docs, T, 37)
    case(out, "count_zero", x, s, t, np.zeros_like(lab), n_docs, None, "Approach5")
    # n_docs = 1
    x, s, t, lab = draw(rng, B, 1, T, 37)
    t[2, 4:] = IGN
    case(out, "ndocs1", x, s, t, lab, 1, None, "Approach3")
    # T = 1 with and without bos (with it the reference's [1:2] slice is empty: no document term)
    x, s, t, lab = draw(rng, B, n_docs, 1, 37)
    case(out, "T1", x, s, t, lab, n_docs, None, "Approach4")
    x, s, t, lab = draw(rng, B, n_docs, 1, 97, bos=5)
    case(out, "T1_bos", x, s, t, lab, n_docs, 5, "Approach4")
    # reduce_loss=False
    x, s, t, lab = draw(rng, B, n_docs, T, 97)
    t[3, 2:] = IGN
    case(out, "not_reduced", x, s, t, lab, n_docs, None, "Approach6", reduce_loss=False)
    # an exact tie at the first position of row 1: values 7.5 at indices 11 and 23, everything else below
    x, s, t, lab = draw(rng, B, n_docs, T, 37)
    x[1, 0] = np.minimum(x[1, 0], 5.0)
    x[1, 0, [11, 23]] = 7.5
    t[1, 0] = 11
    case(out, "tie", x, s, t, lab, n_docs, None, "NoPR")
    out["tie.first_argmax"] = torch.from_numpy(x[:, 0]).argmax(-1).numpy().astype(np.int32)
    assert out["tie.first_argmax"][1] == 11
    path = os.path.join(HERE, "rag_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
