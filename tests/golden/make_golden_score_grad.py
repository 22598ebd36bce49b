#!/usr/bin/env python3
"""Golden vectors for the padded MaxSim under autograd (scoring.colbert_score_differentiable, in_batch_negative_loss):
the REFERENCE's own code, imported from its checkout and run on CPU fp32 tensors, with torch's autograd.

    python tests/golden/make_golden_score_grad.py      # writes tests/golden/score_grad.npz

What runs the reference's code:
  * colbert_score (colbert/modeling/colbert.py:268-286) -> colbert_score_reduce (:235-263), both interactions; the gradients
    are torch's autograd of that expression: `(scores * grad_out).sum().backward()`;
  * ColBERT.compute_ib_loss_new (:82-113), called unbound on a stand-in `self` that holds `colbert_config` and `loss_fn`
    (torch.nn.CrossEntropyLoss, :42), and its `.backward()`.
The argmax recorded per column is what torch's max(dim) returns on the masked score tensor (the index autograd routes the
gradient to), with -1 where that token is padded.  Random query columns are redrawn until the gap between the best and the
second-best distinct real-token score is >= 1e-4 in every document, so the kernel's ~1e-6 error cannot flip a winner; the
deliberate exact ties are zeroed query rows (flmr.py:49-50), duplicated document tokens and an all-padded document.
Only DATA is written.
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FLMR_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, os.path.join(REF, "third_party", "ColBERT"))
sys.path.insert(0, os.path.join(HERE, "_shims"))
os.environ.setdefault("TORCH_EXTENSIONS_DIR", "/tmp/flmr_ref_torch_ext")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import transformers  # noqa: E402

if not hasattr(transformers, "AdamW"):
    transformers.AdamW = torch.optim.AdamW

from colbert.infra.config import ColBERTConfig  # noqa: E402
from colbert.modeling.colbert import ColBERT, colbert_score  # noqa: E402

DIM = 128
GAP = 1e-4


def unit(rng, *shape):
    x = rng.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def make_docs(rng, B, Ld, lengths, holes=(), dup=()):
    """D [B, Ld, 128] unit rows, mask [B, Ld]: the first lengths[b] tokens real, minus (b, t) in `holes`; (b, src, dst) in
    `dup` copies token src over dst (an exact tie)."""
    D = unit(rng, B, Ld, DIM)
    M = np.zeros((B, Ld), dtype=bool)
    for b, n in enumerate(lengths):
        M[b, :n] = True
    for b, t in holes:
        M[b, t] = False
    for b, s, d in dup:
        D[b, d] = D[b, s]
    return D.astype(np.float32), M


def redraw(rng, Q, D, M, docs_of, fixed):
    """Redraw query columns (q, i) not in `fixed` until every document they meet has a top-two gap >= GAP."""
    D64 = D.astype(np.float64)
    for _ in range(200):
        bad = []
        for q in range(Q.shape[0]):
            for i in range(Q.shape[1]):
                if (q, i) in fixed:
                    continue
                for b in docs_of(q):
                    s = np.unique(D64[b][M[b]] @ Q[q, i].astype(np.float64))
                    if s.size >= 2 and s[-1] - s[-2] < GAP:
                        bad.append((q, i))
                        break
        if not bad:
            return Q
        for q, i in bad:
            Q[q, i] = unit(rng, DIM).astype(np.float32)
    raise RuntimeError("could not draw well-separated columns")


def ref_argmax(Qs, D, M):
    """torch's max(dim=1).indices of the masked score tensor [rows, Ld, Nq], -1 where the winner is padded."""
    s = torch.from_numpy(D) @ Qs.permute(0, 2, 1)
    s[~torch.from_numpy(M)] = -9999
    idx = s.max(1).indices
    pad = ~torch.from_numpy(M).gather(1, idx)
    return torch.where(pad, torch.full_like(idx, -1), idx).numpy().astype(np.int32)


def padded_case(rng, out, name, q_batch, B, Ld, Nq, lengths, config, holes=(), dup=(), zero_rows=(), copy_cols=()):
    """colbert_score with autograd.  zero_rows: (q, i) zeroed; copy_cols: (q, i, b, t) sets Q[q, i] = D[b, t] (that token,
    and any duplicate of it, wins the column)."""
    D, M = make_docs(rng, B, Ld, lengths, holes, dup)
    Q = unit(rng, q_batch, Nq, DIM).astype(np.float32)
    fixed = set(zero_rows) | {(q, i) for q, i, _, _ in copy_cols}
    for q, i in zero_rows:
        Q[q, i] = 0.0
    for q, i, b, t in copy_cols:
        Q[q, i] = D[b, t]
    Q = redraw(rng, Q, D, M, (lambda q: range(B)) if q_batch == 1 else (lambda q: [q]), fixed)
    Qt, Dt = torch.from_numpy(Q).requires_grad_(True), torch.from_numpy(D).requires_grad_(True)
    scores = colbert_score(Qt, Dt, torch.from_numpy(M), config=config)
    g = torch.from_numpy(rng.uniform(0.5, 1.5, B).astype(np.float32))
    (scores * g).sum().backward()
    Qs = torch.from_numpy(Q).expand(B, -1, -1) if q_batch == 1 else torch.from_numpy(Q)
    out.update({f"{name}.Q": Q, f"{name}.D": D, f"{name}.mask": M, f"{name}.scores": scores.detach().numpy(),
                f"{name}.grad_out": g.numpy(), f"{name}.dQ": Qt.grad.numpy(), f"{name}.dD": Dt.grad.numpy(),
                f"{name}.argmax": ref_argmax(Qs, D, M), f"{name}.flipr": np.int32(config.interaction == "flipr")})


def ib_case(rng, out, name, nQ, nway, Ld, Nq, lengths, zero_rows=()):
    """ColBERT.compute_ib_loss_new on a stand-in self, and its backward."""
    B = nQ * nway
    D, M = make_docs(rng, B, Ld, lengths, dup=[(1, 3, 7)])
    Q = unit(rng, nQ, Nq, DIM).astype(np.float32)
    for q, i in zero_rows:
        Q[q, i] = 0.0
    Q = redraw(rng, Q, D, M, lambda q: range(B), set(zero_rows))
    cfg = ColBERTConfig(interaction="colbert", nway=nway, use_ib_negatives=True)
    me = types.SimpleNamespace(colbert_config=cfg, loss_fn=torch.nn.CrossEntropyLoss())
    Qt, Dt = torch.from_numpy(Q).requires_grad_(True), torch.from_numpy(D).requires_grad_(True)
    Mt = torch.from_numpy(M).unsqueeze(-1)   # [B, Ld, 1], as ColBERT.doc(keep_dims='return_mask') hands it over
    loss = ColBERT.compute_ib_loss_new(me, Qt, Dt, Mt)
    loss.backward()
    Qx = torch.from_numpy(Q).repeat_interleave(B, dim=0)                        # rows q * B + b (query-major)
    Dx, Mx = np.tile(D, (nQ, 1, 1)), np.tile(M, (nQ, 1))
    with torch.no_grad():
        cross = colbert_score(Qx, torch.from_numpy(Dx), torch.from_numpy(Mx), config=cfg).reshape(nQ, B)
    out.update({f"{name}.Q": Q, f"{name}.D": D, f"{name}.mask": M, f"{name}.scores": cross.numpy(),
                f"{name}.loss": np.float32(loss.item()), f"{name}.dQ": Qt.grad.numpy(), f"{name}.dD": Dt.grad.numpy(),
                f"{name}.argmax": ref_argmax(Qx, Dx, Mx).reshape(nQ, B, Nq), f"{name}.nway": np.int32(nway)})


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    colb = ColBERTConfig(interaction="colbert")
    flipr = ColBERTConfig(interaction="flipr", query_maxlen=64)
    # q_batch = B; doc 2 all padded; doc 1 has holes; doc 0 duplicates token 3 at 9 and query 0 column 5 is that token;
    # query rows 1/2 have zeroed columns (exact 0-ties across every real token; doc 1 begins with a hole)
    padded_case(rng, out, "padded_qb", 4, 4, 40, 32, [37, 40, 0, 12], colb, holes=[(1, 0), (1, 17), (1, 33)],
                dup=[(0, 3, 9), (3, 2, 11)], zero_rows=[(1, 30), (1, 31), (3, 0), (2, 4)],
                copy_cols=[(0, 5, 0, 3), (3, 7, 3, 2)])
    # q_batch = 1 against 5 documents
    padded_case(rng, out, "padded_q1", 1, 5, 33, 32, [33, 20, 1, 32, 7], colb, holes=[(0, 0)], dup=[(1, 4, 19)],
                zero_rows=[(0, 31)], copy_cols=[(0, 2, 1, 4)])
    # 'flipr': 64 + 16 columns
    padded_case(rng, out, "flipr", 2, 2, 24, 80, [24, 10], flipr, zero_rows=[(0, 70)])
    # in-batch negatives: 3 queries x nway 2
    ib_case(rng, out, "ib", 3, 2, 20, 32, [20, 18, 12, 20, 5, 1], zero_rows=[(2, 31), (0, 16)])
    path = os.path.join(HERE, "score_grad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
