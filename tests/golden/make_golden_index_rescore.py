#!/usr/bin/env python3
"""Golden vectors for re-scoring from the compressed index (rag.CompressedPassageStore.score, flmr_maxsim_index_fwd / _bwd):
the REFERENCE's own CPU branch of IndexScorer.score_pids (colbert/search/index_storage.py:160-182), imported from its checkout
and run on the four index fixtures tests/golden/idx_nb{1,2,4,8}.npz under torch's autograd:

    decompress_residuals_cpp (the reference's compiled extension) on the chosen pids -> F.normalize (fp32) ->
    StridedTensor(D_packed, doclens[pids]).as_padded_tensor() -> colbert_score(Q repeated k times, D_padded, D_mask);
    the per-query rows stacked to [n, k]; then (scores * G).sum().backward().

    python tests/golden/make_golden_index_rescore.py      # writes tests/golden/index_rescore.npz

Cases: per index Nq 32 with n = 4 queries x k = 5 passages; on idx_nb2 also one Nq 320 query (n = 1).  Every pid list is
drawn from the index's passages and then given: the length-0 passage 7 (an all-padded document: every column -9999, argmax -1),
the same pid twice in query 0's list, one pid shared by all queries, the index's longest and shortest non-empty passages.
Zeroed query rows (masked query positions, src/models/retriever/FLMR.py:73-99) tie exactly at 0 -> the lowest token.  Random
query rows are redrawn until the top-two gap of distinct token scores is >= 1e-4 in every passage the query meets, so the
kernel's ~1e-6 error cannot flip a winner and winners are compared exactly.  The argmax recorded per row is torch's
max(dim) index on the padded score tensor, -1 where that token is padding.  Only DATA is written (kept under 1 MiB).
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
from colbert.indexing.codecs.residual import ResidualCodec  # noqa: E402
from colbert.modeling.colbert import colbert_score  # noqa: E402
from colbert.search.index_storage import IndexScorer  # noqa: E402
from colbert.search.strided_tensor import StridedTensor  # noqa: E402

DIM, GAP = 128, 1e-4
EMPTY = 7   # a passage of length 0 in every idx_nb*.npz


def unit(rng, *shape):
    x = rng.standard_normal(shape)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


class RefIndex:
    """The tensors IndexScorer.score_pids hands to decompress_residuals_cpp, from one idx_nb*.npz."""

    def __init__(self, z):
        self.nbits = int(z["meta.nbits"])
        self.doclens = torch.from_numpy(z["index.doclens"].astype(np.int64))
        self.offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(self.doclens, 0)])
        self.codes = torch.from_numpy(z["index.codes"].astype(np.int32))
        self.residuals = torch.from_numpy(z["index.residuals"])
        self.centroids = torch.from_numpy(z["index.centroids_f16"].astype(np.float32))   # residual.py:29 on the CPU path
        self.bucket_weights = torch.from_numpy(z["index.bucket_weights"].astype(np.float32))
        # the codec's own tables, built the way ResidualCodec.__init__ builds them (residual.py:36-62)
        codec = ResidualCodec(config=ColBERTConfig(dim=DIM, nbits=self.nbits), centroids=self.centroids.half(),
                              avg_residual=torch.zeros(1), bucket_cutoffs=torch.from_numpy(z["index.bucket_cutoffs"]),
                              bucket_weights=self.bucket_weights)
        self.rbm, self.lut = codec.reversed_bit_map, codec.decompression_lookup_table

    def passages(self, pids):
        """index_storage.py:160-180 for one pid list -> (D_padded [k, L, 128], D_mask) as colbert_score takes them."""
        pids = torch.as_tensor(pids, dtype=torch.int32)
        D = IndexScorer.decompress_residuals(pids, self.doclens, self.offsets, self.bucket_weights, self.rbm, self.lut,
                                             self.residuals, self.codes, self.centroids, DIM, self.nbits)
        D = torch.nn.functional.normalize(D.to(torch.float32), p=2, dim=-1)
        return StridedTensor(D, self.doclens[pids.long()], use_gpu=False).as_padded_tensor()


def redraw(rng, Q, ix, pids, fixed):
    for _ in range(200):
        bad = []
        for q in range(Q.shape[0]):
            uniq = sorted(set(pids[q].tolist()))
            D, M = ix.passages(uniq)
            D64, M = D.numpy().astype(np.float64), M.numpy().reshape(len(uniq), -1).astype(bool)
            for i in range(Q.shape[1]):
                if (q, i) in fixed:
                    continue
                for r in range(len(uniq)):
                    s = np.unique(D64[r][M[r]] @ Q[q, i].astype(np.float64))
                    if s.size >= 2 and s[-1] - s[-2] < GAP:
                        bad.append((q, i))
                        break
        if not bad:
            return Q
        for q, i in bad:
            Q[q, i] = unit(rng, DIM)
    raise RuntimeError("could not draw well-separated columns")


def case(rng, out, name, ix, Q, pids, zero_rows):
    Q = Q.copy()
    for q, i in zero_rows:
        Q[q, i] = 0.0
    Q = redraw(rng, Q, ix, pids, set(zero_rows))
    Qt = torch.from_numpy(Q).requires_grad_(True)
    k = pids.shape[1]
    rows, am = [], []
    for q in range(pids.shape[0]):
        D, M = ix.passages(pids[q])
        Qk = Qt[[q]].repeat_interleave(k, 0)
        rows.append(colbert_score(Qk, D, M, config=ColBERTConfig(interaction="colbert")))
        Mb = M.reshape(k, -1).bool()
        s = (D @ Qk.detach().permute(0, 2, 1)).masked_fill(~Mb.unsqueeze(-1), -9999)
        idx = s.max(1).indices
        am.append(torch.where(Mb.gather(1, idx), idx, torch.full_like(idx, -1)))
    scores = torch.stack(rows)
    G = torch.from_numpy(rng.uniform(0.5, 1.5, pids.shape).astype(np.float32))
    (scores * G).sum().backward()
    out.update({f"{name}.Q": Q, f"{name}.pids": pids.astype(np.int32), f"{name}.scores": scores.detach().numpy(),
                f"{name}.G": G.numpy(), f"{name}.dQ": Qt.grad.numpy(), f"{name}.argmax": torch.stack(am).numpy().astype(np.int32)})


def pid_lists(rng, ix, n, k):
    dl = ix.doclens.numpy()
    assert dl[EMPTY] == 0
    nonempty = np.nonzero(dl > 0)[0]
    longest, shortest = int(nonempty[np.argmax(dl[nonempty])]), int(nonempty[np.argmin(dl[nonempty])])
    pids = rng.choice(nonempty, size=(n, k), replace=False)
    shared = int(pids[0, 2])
    pids[0, 0], pids[0, 1], pids[0, 3] = longest, EMPTY, longest          # a repeat and the empty passage in one list
    for q in range(1, n):
        pids[q, q % k] = shared                                            # one pid in every query's list
    pids[n - 1, k - 1] = shortest
    if n > 2:
        pids[2, 0] = EMPTY
    return pids


def main():
    IndexScorer.try_load_torch_extensions(False)
    rng = np.random.default_rng(20261017)
    out = {}
    for nb in (1, 2, 4, 8):
        ix = RefIndex(np.load(os.path.join(HERE, f"idx_nb{nb}.npz")))
        pids = pid_lists(rng, ix, 4, 5)
        case(rng, out, f"nb{nb}.nq32", ix, unit(rng, 4, 32, DIM), pids, zero_rows=[(0, 30), (0, 31), (1, 0), (2, 17), (3, 31)])
        if nb == 2:
            case(rng, out, f"nb{nb}.nq320", ix, unit(rng, 1, 320, DIM), pids[:1],
                 zero_rows=[(0, i) for i in range(24, 32)] + [(0, i) for i in range(300, 320)])
    path = os.path.join(HERE, "index_rescore.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
