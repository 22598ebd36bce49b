"""The FLMR / ColBERT scoring head -- host-side mirror of `colbert_score`, `colbert_score_packed`,
`colbert_score_reduce` and `ColBERT.segmented_maxsim` (TPC/modeling/colbert.py:235-311) and of the inherited
`score(Q, D_padded, D_mask)` of the FLMR model classes (src/models/retriever/FLMR.py; TPC/modeling/colbert.py:217-224).

`colbert_score` and the other search-side functions are forward only: they raise if an input requires grad instead of
silently computing without a graph.  The score under autograd -- RA-VQA's re-scoring inside the RAG model
(src/models/rag/rag_model_blip.py:430-435) and the in-batch-negative loss of retriever training (`compute_ib_loss_new`,
colbert.py:82-113) -- goes through `colbert_score_differentiable`, `colbert_score_cross_differentiable` and
`in_batch_negative_loss`: the HIP forward records the winning token of every column and the HIP backward gathers the
gradients from it (flmr_colbert_maxsim_fwd / _bwd), so the [B, Ld, Nq] score tensor is never materialised.  Where the
documents are passages of a device-resident store picked by pid -- the RAG model's re-scoring of what it has just retrieved --
`maxsim_gather_differentiable` (rag.PassageEmbeddingStore.score) does the same without building the padded document copy or the
duplicated queries (flmr_maxsim_gather_fwd / _bwd); `maxsim_index_differentiable` (rag.CompressedPassageStore.score) reads the
passages' tokens out of the compressed index itself (flmr_maxsim_index_fwd / _bwd), for corpora with no resident store.
"""
import torch

from . import ops
from .ops import maxsim_native_pair


def _no_grad_only(*tensors):
    if torch.is_grad_enabled() and any(getattr(t, "requires_grad", False) for t in tensors):
        raise RuntimeError("the HIP MaxSim scorer is forward-only; call it under torch.no_grad()/inference_mode()")


def _interaction(config):
    interaction = getattr(config, "interaction", "colbert") if config is not None else "colbert"
    assert interaction in ("colbert", "flipr"), interaction   # colbert.py:244
    return interaction


def reduce_colmax(colmax, config=None):
    """[B, Nq] per-column maxima -> [B] (the second half of colbert_score_reduce, colbert.py:244-263): their sum for
    'colbert'; for 'flipr' the 32 largest of the first 64 columns plus, when there are that many, the 8 largest of the rest."""
    if _interaction(config) == "flipr":
        assert config.query_maxlen == 64, ("for now", config)
        qm, K2 = config.query_maxlen, 8
        out = colmax[:, :qm].topk(qm // 2, dim=-1).values.sum(-1)
        if K2 <= colmax.size(1) - qm:
            out = out + colmax[:, qm:].topk(K2, dim=-1).values.sum(1)
        return out
    return colmax.sum(-1)


def colbert_score_reduce(scores_padded, D_mask, config=None):
    """[B, Ld, Nq] scores + mask -> [B] (colbert.py:235-263, both interactions): tiny torch epilogue kept for callers that
    already hold a padded score tensor on the device."""
    pad = ~D_mask.view(scores_padded.size(0), scores_padded.size(1)).bool()
    scores_padded = scores_padded.masked_fill(pad.unsqueeze(-1), -9999)
    return reduce_colmax(scores_padded.max(1).values, config)


def colbert_score(Q, D_padded, D_mask, config=None, use_gpu=False):
    """Padded late-interaction score (colbert.py:268-286): Q [1|B, Nq, d] x D [B, Ld, d] -> [B] on the device; the 'flipr'
    interaction takes the kernel's per-column maxima and reduces them as colbert.py:246-261 does."""
    _no_grad_only(Q, D_padded)
    assert Q.dim() == 3 and D_padded.dim() == 3 and Q.size(0) in (1, D_padded.size(0))
    if _interaction(config) == "flipr":
        return reduce_colmax(ops.colbert_colmax_padded(Q, D_padded, D_mask), config)
    return ops.colbert_score_padded(Q, D_padded, D_mask)


_device = "cuda"   # where the kernels run (the CPU plumbing tests point this at "cpu" with stand-in ops)


def _grad_colmax(grad, argmax, want_colmax):
    """dL/dcolmax, fp32 and contiguous, shaped like argmax, from the gradient of what a MaxSim Function returned: the column
    maxima themselves, or their sum (every column of a row then shares the row's gradient)."""
    return (grad.float() if want_colmax else grad.float().unsqueeze(-1).expand(argmax.shape)).contiguous()


def _reduced(apply, config, shape):
    """The scores, shaped `shape`, of a MaxSim Function called as apply(want_colmax): its own row sums for 'colbert', its
    differentiable column maxima reduced by reduce_colmax for 'flipr'."""
    if _interaction(config) == "flipr":
        return reduce_colmax(apply(True).flatten(0, -2), config).reshape(shape)
    return apply(False)


class _MaxSim(torch.autograd.Function):
    """Padded MaxSim with the gradient torch's autograd gives colbert_score_reduce (colbert.py:235-263): each column's
    gradient goes to its winning token, the lowest one on ties, and nowhere when that token is padded.  Returns the kernel's
    per-row sum (`colbert`, [rows]) or the per-column maxima ([rows, Nq]); rows are [nQ, B] in the cross form.

    Operand dtypes: fp32 Q and D, and fp16 D with fp32 or fp16 Q (what a drop-in training step holds), go to the kernels as they
    are -- no fp32 copy is made, the operands are saved as given and the backward writes each gradient in its input's dtype.
    Every other pair (bf16, fp64, fp16 Q with fp32 D) is widened exactly to fp32 for the kernels and its gradients are converted
    back."""

    @staticmethod
    def _operands(Q, D_padded):
        if maxsim_native_pair(Q.dtype, D_padded.dtype):
            return Q.detach(), D_padded.detach(), True
        return Q.detach().float(), D_padded.detach().float(), False

    @staticmethod
    def forward(ctx, Q, D_padded, D_mask, cross, want_colmax):
        Qk, Dk, _ = _MaxSim._operands(Q, D_padded)
        out, colmax, argmax = ops.colbert_maxsim_fwd(Qk, Dk, D_mask, cross=cross, want_out=not want_colmax, want_colmax=want_colmax)
        ctx.save_for_backward(Q, D_padded, argmax)
        ctx.cross, ctx.want_colmax = cross, want_colmax
        return colmax if want_colmax else out

    @staticmethod
    def backward(ctx, grad):
        Q, D_padded, argmax = ctx.saved_tensors
        need_dQ, need_dD = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_dQ or need_dD):
            return None, None, None, None, None
        G = _grad_colmax(grad, argmax, ctx.want_colmax)
        Qk, Dk, native = _MaxSim._operands(Q, D_padded)
        if native and (Q.dtype, D_padded.dtype) != (torch.float32, torch.float32):   # the kernels write each input's dtype
            dQ, dD = ops.colbert_maxsim_bwd(Qk, Dk, argmax, G, cross=ctx.cross, need_dQ=need_dQ, need_dD=need_dD,
                                            dq_dtype=Q.dtype, dd_dtype=D_padded.dtype)
            return dQ, dD, None, None, None
        dQ, dD = ops.colbert_maxsim_bwd(Qk, Dk, argmax, G, cross=ctx.cross, need_dQ=need_dQ, need_dD=need_dD)
        return (dQ.to(Q.dtype) if need_dQ else None, dD.to(D_padded.dtype) if need_dD else None, None, None, None)


def _maxsim(Q, D_padded, D_mask, config, cross):
    if Q.dim() != 3 or D_padded.dim() != 3 or Q.size(-1) != D_padded.size(-1):
        raise ValueError(f"Q {tuple(Q.shape)} / D {tuple(D_padded.shape)}: expected [n, Nq, d] and [B, Ld, d]")
    if not cross and Q.size(0) not in (1, D_padded.size(0)):
        raise ValueError(f"Q.size(0) = {Q.size(0)} must be 1 or B = {D_padded.size(0)}")   # colbert.py:278
    Q, D_padded = Q.to(_device), D_padded.to(_device)
    return _reduced(lambda want_colmax: _MaxSim.apply(Q, D_padded, D_mask, cross, want_colmax), config,
                    (Q.size(0), D_padded.size(0)) if cross else (D_padded.size(0),))


# A document source of _MaxSimGathered: (fwd(Q, pids, want_out=, want_colmax=), bwd(pids, argmax, G), tensors) -- the `ops` calls
# that read it (`ops` is looked up at each call: the CPU plumbing tests swap it) and the tensors it is made of, which the
# Function takes as inputs without a gradient.
def _store_source(store, store_mask):
    """The rows of a resident passage store [P, Ld, 128] (fp32 / fp16) + mask [P, Ld]."""
    return (lambda Q, pids, **want: ops.maxsim_gather_fwd(Q, store, store_mask, pids, **want),
            lambda pids, argmax, G: ops.maxsim_gather_bwd(store, pids, argmax, G), (store, store_mask))


def _index_source(device_index):
    """The resident compressed index (index.DeviceIndex): the passages' tokens are decompressed and normalised in the kernels."""
    return (lambda Q, pids, **want: ops.maxsim_index_fwd(device_index, Q, pids, **want),
            lambda pids, argmax, G: ops.maxsim_index_bwd(device_index, pids, argmax, G), ())


class _MaxSimGathered(torch.autograd.Function):
    """_MaxSim whose documents are passages of a document source picked by pid: row (q, j) is query q against passage
    pids[q, j] (< 0: an empty slot, an all-padded document).  Saves (Q, pids, argmax) and the source by reference; the source is
    a constant of training, so Q is the only input with a gradient.  Returns [n, k] sums or [n, k, Nq] column maxima."""

    @staticmethod
    def forward(ctx, Q, source, pids, want_colmax, *source_tensors):
        out, colmax, argmax = source[0](Q.detach().float(), pids, want_out=not want_colmax, want_colmax=want_colmax)
        ctx.save_for_backward(Q, pids, argmax)
        ctx.source, ctx.want_colmax = source, want_colmax
        return colmax if want_colmax else out

    @staticmethod
    def backward(ctx, grad):
        Q, pids, argmax = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * len(ctx.needs_input_grad)
        dQ = ctx.source[1](pids, argmax, _grad_colmax(grad, argmax, ctx.want_colmax))
        return (dQ.to(Q.dtype),) + (None,) * (len(ctx.needs_input_grad) - 1)


def _gathered(Q, source, pids, config):
    Q, pids = Q.to(_device), pids.to(device=_device, dtype=torch.int32)
    return _reduced(lambda want_colmax: _MaxSimGathered.apply(Q, source, pids, want_colmax, *source[2]), config, pids.shape)


def maxsim_gather_differentiable(Q, store, store_mask, pids, config=None):
    """Re-scoring of retrieved passages under autograd (rag_model_blip.py:430-435 for a whole batch): Q [n, Nq, 128], a resident
    store [P, Ld, 128] (fp32 / fp16) + mask [P, Ld], pids i32 [n, k] -> f32 [n, k], differentiable in Q only.  Values are those
    of colbert_score_differentiable(Q.repeat_interleave(k, 0), store[pids], mask[pids]); pids must be < P (the caller checks:
    rag.PassageEmbeddingStore.score does)."""
    if Q.dim() != 3 or store.dim() != 3 or Q.size(-1) != store.size(-1) or pids.dim() != 2 or pids.size(0) != Q.size(0):
        raise ValueError(f"Q {tuple(Q.shape)} / store {tuple(store.shape)} / pids {tuple(pids.shape)}: expected [n, Nq, d], "
                         "[P, Ld, d] and [n, k]")
    if store.requires_grad:
        raise RuntimeError("the passage store is a constant of training: there is no store gradient (detach it)")
    return _gathered(Q, _store_source(store, store_mask), pids, config)


def maxsim_index_differentiable(Q, device_index, pids, config=None):
    """maxsim_gather_differentiable from the compressed index: Q [n, Nq, 128] (fp32 / fp16 / bf16, widened exactly), a resident
    index.DeviceIndex, pids i32 [n, k] as the index's search returns them -> f32 [n, k], differentiable in Q only (dQ in Q's
    dtype).  Values are colbert_score (-9999 padding, no zero clamp) of Q[q] against the decompressed, normalised tokens of
    passage pids[q, j] (index_storage.py:160-173) in fp32, whatever numerics mode the searcher runs; a pid < 0 or outside the
    index and a passage of length 0 score as all-padded documents."""
    if Q.dim() != 3 or pids.dim() != 2 or pids.size(0) != Q.size(0):
        raise ValueError(f"Q {tuple(Q.shape)} / pids {tuple(pids.shape)}: expected [n, Nq, d] and [n, k]")
    return _gathered(Q, _index_source(device_index), pids, config)


def colbert_score_differentiable(Q, D_padded, D_mask, config=None):
    """colbert_score (colbert.py:268-286) under autograd: Q [1|B, Nq, 128], D [B, Ld, 128] -> f32 [B] on the device, with
    dQ / dD equal to what torch's autograd gives the reference expression.  fp16 D with fp16 or fp32 Q runs natively (no fp32
    copy; the bits of the fp32 path on the widened values); bf16 and every other pair are widened exactly to fp32.  Gradients
    come back in each input's dtype.  'colbert' values are bit-identical to ops.colbert_score_padded; 'flipr'
    reduces the differentiable column maxima with reduce_colmax."""
    return _maxsim(Q, D_padded, D_mask, config, cross=False)


def colbert_score_cross_differentiable(Q, D_padded, D_mask, config=None):
    """Every query against every document under autograd: Q [nQ, Nq, 128], D [B, Ld, 128] -> f32 [nQ, B] -- the
    `in_batch_scores` of compute_ib_loss_new (colbert.py:86-92, query-major), values bit-identical to ops.colbert_score_cross."""
    return _maxsim(Q, D_padded, D_mask, config, cross=True)


def in_batch_negative_loss(Q, D, D_mask, config=None, loss_fn=None):
    """compute_ib_loss_new (colbert.py:82-113): Q [nQ, Nq, 128], D [nQ * nway, Ld, 128] -> the cross-entropy of every query's
    scores against all nQ * nway documents, the label of query q being its first passage, column q * nway.  `loss_fn` defaults
    to torch.nn.CrossEntropyLoss() (colbert.py:42)."""
    scores = colbert_score_cross_differentiable(Q, D, D_mask, config)
    nway = D.size(0) // Q.size(0)
    labels = torch.arange(Q.size(0), device=scores.device) * nway
    return (loss_fn or torch.nn.CrossEntropyLoss())(scores, labels)


def colbert_score_packed(Q, D_packed, D_lengths, config=None):
    """Single-query packed score (colbert.py:289-311) from an already materialised D_packed: GEMM by torch on the
    device (plumbing), zero-clamped segmented MaxSim by the HIP op."""
    _no_grad_only(Q, D_packed)
    Qd = Q.squeeze(0).to("cuda", torch.float32)
    scores = D_packed.to("cuda", torch.float32) @ Qd.T
    return ops.segmented_maxsim(scores, torch.as_tensor(D_lengths).to("cuda"))


class ColBERT:
    """Only the class attribute the reference's packed scorer looks up (colbert.py:44-62, :311)."""
    segmented_maxsim = staticmethod(ops.segmented_maxsim)

    @classmethod
    def try_load_torch_extensions(cls, use_gpu):
        from . import _native
        _native.load(require_device=True)
        cls.loaded_extensions = True


class FLMRScoringHead:
    """`score(Q, D_padded, D_mask)` with the semantics the four FLMR model classes inherit from ColBERT.score
    (colbert.py:217-224, similarity == 'cosine' path): exhaustive-search and RAG re-scoring callers
    (src/executors/FLMR_executor.py:833, src/models/rag/rag_model_blip.py:435) can bind this in place of the
    torch expression when gradients are off.  When they are on -- the RAG model's training step -- the re-scoring goes through
    `rag.retrieve_and_rescore` / `rag.PassageEmbeddingStore.score`, which reads the retrieved passages from a device store."""

    def score(self, Q, D_padded, D_mask):
        return colbert_score(Q, D_padded, D_mask)


def exhaustive_search(query_embeddings, item_embeddings, item_embedding_mask, k, item_chunk=None):
    """Brute-force late-interaction search: every query against every item, top-k by score -- the `else` branch of
    `FLMRExecutor.evaluate_outputs` (src/executors/FLMR_executor.py:799-847), which fills `rate_batch[nq, n_items]` four
    items at a time through `model.score` and then sorts each row descending.

    query_embeddings [nq, Nq, d]; item_embeddings [n_items, Ld, d]; item_embedding_mask [n_items, Ld(,1)] (1 = real token).
    Returns (indices int64 [nq, k'], scores f32 [nq, k'], rate_batch f32 [nq, n_items]) on the device, k' = min(k, n_items).
    One launch of the padded MaxSim kernel per item chunk scores EVERY query against the chunk's items (the cross form,
    `flmr_colbert_score_cross`); `item_chunk` bounds the items resident per launch for corpora larger than HBM headroom.
    fp16 items (with fp16 or fp32 queries) are moved and scored chunk by chunk as fp16, with the bits of the run on their fp32
    image; other dtypes are widened to fp32 per chunk."""
    _no_grad_only(query_embeddings, item_embeddings)
    Q = torch.as_tensor(query_embeddings).to("cuda")
    D = torch.as_tensor(item_embeddings)
    native = maxsim_native_pair(Q.dtype, D.dtype)
    if not native:
        Q = Q.float()
    M = torch.as_tensor(item_embedding_mask)
    n_items = D.size(0)
    M = M.reshape(n_items, -1)
    item_chunk = item_chunk or n_items
    rate = torch.empty((Q.size(0), n_items), dtype=torch.float32, device="cuda")
    for i0 in range(0, n_items, item_chunk):
        Dc = D[i0:i0 + item_chunk].to("cuda", D.dtype if native else torch.float32).contiguous()
        Mc = M[i0:i0 + item_chunk].to("cuda")
        for q0 in range(0, Q.size(0), 65535):   # (grid dimension limit of the cross form)
            rate[q0:q0 + 65535, i0:i0 + Dc.size(0)] = ops.colbert_score_cross(Q[q0:q0 + 65535], Dc, Mc)
    scores, indices = torch.sort(rate, dim=-1, descending=True)
    kk = min(int(k), n_items)
    return indices[:, :kk], scores[:, :kk], rate


def exhaustive_ranking_dict(indices, scores):
    """(indices, scores) -> {query_index: [(item index, rank from 0, int(score))]} exactly as FLMR_executor.py:838-845
    builds it (the reference truncates the score to an int there; kept so downstream records match)."""
    idx, sc = indices.cpu(), scores.cpu()
    return {q: [(int(idx[q, i]), i, int(sc[q, i])) for i in range(idx.size(1))] for q in range(idx.size(0))}
