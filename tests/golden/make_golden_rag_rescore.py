#!/usr/bin/env python3
"""Golden vectors for retrieve-and-rescore (rag.PassageEmbeddingStore.score, flmr_maxsim_gather_fwd / _bwd): the REFERENCE's
own scoring function (colbert_score, colbert/modeling/colbert.py:268-286 -- what ColBERT.score calls, :224), imported from its
checkout and run on CPU fp32 tensors under torch's autograd, fed the way the RAG model's training step feeds it
(src/models/rag/rag_model_blip.py:409-442; the steps are restated in this file's own code, `rescore_per_query`):

    a host dict  pid -> (embeddings [Ld, 128], mask [Ld, 1]);  per query: a torch.Tensor copy of every retrieved passage and
    of its mask, stacked; the query repeated k times; one colbert_score call; the per-query rows stacked to [n, k];
    then (doc_scores * grad_out).sum().backward().

    python tests/golden/make_golden_rag_rescore.py      # writes tests/golden/rag_rescore.npz

One store of 16 passages x 32 tokens (general fp32 values, so the fp16 split of the documents has a low part): passage 0
begins with a mask hole, 3 has interior holes (the punctuation skiplist, colbert.py:194-215), 5 is all padded, 7 and 11 hold
duplicated tokens (exact ties -> the lowest token).  Cases: Nq 32 and 320, k 5 and 50 (k = 50 over 16 passages repeats pids);
the same pid twice in one query's list; one pid shared by several queries; zeroed query rows (masked query positions,
src/models/retriever/FLMR.py:73-99: exact ties at 0); query columns copied from a duplicated token.  Random query columns are
redrawn until the top-two gap of distinct real-token scores is >= 1e-4 in every passage the query meets, so the kernel's
~1e-6 error cannot flip a winner.  The argmax recorded per row is torch's max(dim) index on the masked score tensor, -1 where
that token is padded.  Only DATA is written (kept under 1 MiB: the Nq = 320 cases hold one query).
"""
import os
import sys

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
from colbert.modeling.colbert import colbert_score  # noqa: E402

DIM, GAP = 128, 1e-4
P, LD = 16, 32


def unit(rng, *shape):
    x = rng.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def make_store(rng):
    D = unit(rng, P, LD, DIM)
    lengths = [32, 20, 32, 30, 7, 0, 32, 16, 1, 25, 32, 12, 31, 32, 9, 28]
    M = np.zeros((P, LD), dtype=bool)
    for p, n in enumerate(lengths):
        M[p, :n] = True
    for p, t in [(0, 0), (3, 4), (3, 17), (3, 18), (12, 0), (12, 1)]:
        M[p, t] = False
    for p, s, d in [(7, 2, 9), (11, 3, 8), (11, 3, 10)]:
        D[p, d] = D[p, s]
    return D.astype(np.float32), M


def redraw(rng, Q, D, M, pids, fixed):
    D64 = D.astype(np.float64)
    for _ in range(200):
        bad = []
        for q in range(Q.shape[0]):
            for i in range(Q.shape[1]):
                if (q, i) in fixed:
                    continue
                for p in sorted(set(pids[q].tolist())):
                    s = np.unique(D64[p][M[p]] @ Q[q, i].astype(np.float64))
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


def rescore_per_query(Qt, host_store, pids, config):
    """The hand-over of the training step, one query at a time: the passages of row q leave the host dict as torch.Tensor
    copies and are stacked ([k, Ld, 128] and [k, Ld, 1]), the query is repeated k times, and the reference's colbert_score
    scores the pairs; the rows are stacked to [n, k]."""
    rows = []
    for q in range(pids.shape[0]):
        picked = [host_store[int(p)] for p in pids[q]]
        D = torch.stack([torch.Tensor(emb) for emb, _ in picked])
        mask = torch.stack([torch.Tensor(m) for _, m in picked])
        rows.append(colbert_score(Qt[[q]].repeat_interleave(len(picked), 0), D, mask, config=config))
    return torch.stack(rows)


def case(rng, out, name, D, M, host_store, Q, pids, zero_rows=(), copy_cols=()):
    """zero_rows: (q, i) zeroed; copy_cols: (q, i, p, t) sets Q[q, i] = D[p, t]."""
    Q = Q.copy()
    fixed = set(zero_rows) | {(q, i) for q, i, _, _ in copy_cols}
    for q, i in zero_rows:
        Q[q, i] = 0.0
    for q, i, p, t in copy_cols:
        Q[q, i] = D[p, t]
    Q = redraw(rng, Q, D, M, pids, fixed)
    Qt = torch.from_numpy(Q).requires_grad_(True)
    doc_scores = rescore_per_query(Qt, host_store, pids, ColBERTConfig(interaction="colbert"))
    g = torch.from_numpy(rng.uniform(0.5, 1.5, pids.shape).astype(np.float32))
    (doc_scores * g).sum().backward()
    k = pids.shape[1]
    flat = pids.reshape(-1)
    am = ref_argmax(torch.from_numpy(Q).repeat_interleave(k, dim=0), D[flat], M[flat]).reshape(pids.shape + (Q.shape[1],))
    out.update({f"{name}.Q": Q, f"{name}.pids": pids.astype(np.int32), f"{name}.doc_scores": doc_scores.detach().numpy(),
                f"{name}.grad_out": g.numpy(), f"{name}.dQ": Qt.grad.numpy(), f"{name}.argmax": am})


def main():
    rng = np.random.default_rng(20261017)
    D, M = make_store(rng)
    host_store = {i: (D[i], M[i].astype(np.float32)[:, None]) for i in range(P)}   # (embeddings, mask [Ld, 1])
    out = {"store": D, "store_mask": M}
    Q32 = unit(rng, 3, 32, DIM).astype(np.float32)
    Q320 = unit(rng, 1, 320, DIM).astype(np.float32)
    # k = 5: pid 7 twice in query 0's list; pid 3 shared by all three queries; the all-padded passage 5; the one-token passage 8
    pids5 = np.array([[7, 3, 0, 7, 5], [3, 11, 12, 8, 1], [15, 5, 3, 11, 2]])
    case(rng, out, "nq32_k5", D, M, host_store, Q32, pids5, zero_rows=[(0, 30), (0, 31), (1, 0), (2, 17)],
         copy_cols=[(0, 4, 7, 2), (1, 6, 11, 3), (2, 9, 11, 3)])
    # k = 50 over 16 passages: every list repeats pids
    pids50 = rng.integers(0, P, (3, 50))
    pids50[0, :3] = [5, 5, 7]
    pids50[1, :2] = [5, 8]
    case(rng, out, "nq32_k50", D, M, host_store, Q32, pids50, zero_rows=[(1, 31), (2, 0)], copy_cols=[(0, 3, 7, 9)])
    case(rng, out, "nq320_k5", D, M, host_store, Q320, pids5[:1], zero_rows=[(0, i) for i in range(24, 32)],
         copy_cols=[(0, 100, 7, 2)])
    case(rng, out, "nq320_k50", D, M, host_store, Q320, pids50[1:2], zero_rows=[(0, i) for i in range(300, 320)],
         copy_cols=[(0, 40, 11, 8)])
    path = os.path.join(HERE, "rag_rescore.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
