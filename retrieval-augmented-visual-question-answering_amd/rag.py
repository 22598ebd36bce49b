"""Retrieve-and-rescore for RAG training: search -> gather -> differentiable score, all on the device.

Inside a training step `RagModelForBlip.main_retrieve` (src/models/rag/rag_model_blip.py:339-443) encodes the questions,
searches the index with the detached embeddings (:397), then -- per query, in a Python loop -- pulls the retrieved passages'
uncompressed padded embeddings out of a host dict loaded from a pickle (:303-311, :419-428: `torch.Tensor(...)` per passage,
`stack`, `.to(device)`) and re-scores them under autograd with `question_encoder.score(Q_duplicated, D, mask)` (:430-435).
Here the dict is a `PassageEmbeddingStore` resident in HBM, and `retrieve_and_rescore` runs the three steps without a host
round trip: `IndexScorer.search_batch` hands over device pids, and `flmr_maxsim_gather_fwd / _bwd` read the store's rows by
pid, so neither `Q_duplicated` [B * k, Nq, 128] nor a padded document copy [B * k, Ld, 128] is ever built.

    store = PassageEmbeddingStore.from_reference_file(embedding_path)          # once, replaces :303-311
    r = searcher.retrieve_and_rescore(question_hidden_states, store, n_docs)   # per step, replaces :397-443
    doc_scores, ids = r.doc_scores, r.passage_ids                              # [B, n_docs] with grad to the encoder

Limits of the resident store: dim 128; one padded length Ld for the whole store; it must fit HBM (110 k passages x 512 x 128
fp16 = 14.4 GB).  A corpus too large for that -- the 1 M and 6 M passage corpora need 130 GB to 800 GB -- is re-scored from the
compressed index the searcher already holds: `CompressedPassageStore` (what `retrieve_and_rescore(Q, None, n_docs)` builds)
scores through flmr_maxsim_index_fwd / _bwd, which decode the passages' tokens inside the kernels, so there is no pickle, no
second copy of the corpus and no common padded length.  Out of scope there: a gradient to the documents, the
gpu-fp16 numerics mode (the re-score is always the fp32 CPU-path definition), ShardedSearcher, dim != 128 and the
prediction-file reader.

The step ends in `RagModelForBlip.get_loss` (:826-1026), where doc_scores meets the generator's logits [B * n_docs, T, V] in the
RAG-sequence marginalisation.  `marginalised_loss` is that call: the one part that touches the logits -- log_softmax and the gather
at the targets -- is `token_log_likelihood`, a fused HIP pair (flmr_rag_token_ll_fwd / _bwd) that reads the logits once per
direction, skips ignored positions and keeps 12 bytes per position; everything after it is torch on [B, n_docs, T] or smaller.

    out = rag.marginalised_loss(logits, r.doc_scores, generator_labels, n_docs, bos_token_id=generator.config.bos_token_id,
                                retrieval_labels=retrieval_labels, loss_type=config.model_config.RAVQA_loss_type)   # replaces :708-715
    loss = sum(out[name] * ratio for name, ratio in loss_ratio.items() if ratio != 0)
"""
import pickle

import numpy as np
import torch

from . import ops, scoring


def _rows(x, i0, i1):
    """Passages i0..i1 of a tensor / array / list of per-passage arrays as one CPU or device tensor [n, ...]."""
    if isinstance(x, (list, tuple)):
        return torch.stack([torch.as_tensor(np.asarray(a)) if not torch.is_tensor(a) else a for a in x[i0:i1]])
    return torch.as_tensor(x[i0:i1])


class PassageEmbeddingStore:
    """The device-resident replacement of the RAG model's `self.item_embeddings` dict (rag_model_blip.py:303-311):
    `embeddings` [P, Ld, 128] fp16 or fp32, `mask` uint8 [P, Ld] (1 = real token; interior holes allowed), and the reference's
    `passage_index2id`.  Built once; `score` re-scores device pids under autograd without copying a row."""

    def __init__(self, embeddings, mask, passage_index2id=None):
        assert embeddings.dim() == 3 and embeddings.dtype in (torch.float16, torch.float32), (embeddings.shape, embeddings.dtype)
        assert mask.shape == embeddings.shape[:2] and mask.dtype == torch.uint8, (mask.shape, mask.dtype)
        self.embeddings, self.mask, self.passage_index2id = embeddings, mask, passage_index2id

    @classmethod
    def from_padded(cls, item_embeddings, item_embedding_mask, passage_index2id=None, dtype="auto", device="cuda", chunk=1024):
        """item_embeddings: a tensor / array [P, Ld, 128] or the reference's list of P per-passage arrays [Ld, 128];
        item_embedding_mask: [P, Ld] or [P, Ld, 1] (what `doc(..., keep_dims="return_mask")` yields, colbert.py:194-215), or a
        list of per-passage [Ld] / [Ld, 1] arrays.  Uploaded `chunk` passages at a time, so the host never holds a second copy.

        dtype="auto" keeps fp16 when EVERY value survives x.half().float() == x (checked chunk by chunk on the device: the
        embeddings of an encoder that ran under autocast do) and fp32 otherwise -- scores are the same bits either way.
        dtype="float16" FORCES rounding to half: the store is half the size, and scores then differ from those of the fp32
        embeddings by the rounding of every document value (~2^-11 relative).  dtype="float32" never rounds.
        Device memory while building: "auto" starts in fp16 and, at the first chunk holding a value half cannot represent,
        allocates the fp32 store beside it and widens what is there, so the peak is 1.5x the final fp32 store (110 k passages x
        512 tokens: 14.4 GB + 28.8 GB).  For embeddings known not to be half-exact pass dtype="float32"."""
        if dtype not in ("auto", "float16", "float32"):
            raise ValueError(f"dtype must be 'auto', 'float16' or 'float32', got {dtype!r}")
        P = len(item_embeddings)
        if len(item_embedding_mask) != P:
            raise ValueError(f"{P} passages but {len(item_embedding_mask)} masks")
        if P == 0:
            raise ValueError("an empty passage store")
        first = _rows(item_embeddings, 0, 1)
        if first.dim() != 3 or first.size(-1) != 128:
            raise ValueError(f"passages must be [Ld, 128], got {tuple(first.shape[1:])}")
        Ld = first.size(1)
        half = dtype != "float32"
        emb = torch.empty((P, Ld, 128), dtype=torch.float16 if half else torch.float32, device=device)
        mask = torch.empty((P, Ld), dtype=torch.uint8, device=device)
        for i0 in range(0, P, max(int(chunk), 1)):
            i1 = min(i0 + max(int(chunk), 1), P)
            x = _rows(item_embeddings, i0, i1)
            if tuple(x.shape[1:]) != (Ld, 128):
                raise ValueError(f"passages {i0}..{i1}: {tuple(x.shape[1:])}, the store is padded to one length ({Ld}, 128)")
            m = _rows(item_embedding_mask, i0, i1).reshape(i1 - i0, -1)
            if m.size(1) != Ld:
                raise ValueError(f"masks {i0}..{i1}: {m.size(1)} tokens, embeddings have {Ld}")
            x = x.to(device)
            mask[i0:i1] = (m.to(device) != 0).to(torch.uint8)
            if x.dtype == torch.float16 and half:
                emb[i0:i1] = x
                continue
            x = x.float()
            if half and dtype == "auto" and not torch.equal(x.half().float(), x):
                # a value that half cannot hold: the store becomes fp32 (what is already there was exact, so widening it is too)
                wide = torch.empty((P, Ld, 128), dtype=torch.float32, device=device)
                wide[:i0] = emb[:i0]
                emb, half = wide, False
            emb[i0:i1] = x   # (rounds only under dtype="float16")
        return cls(emb, mask, passage_index2id)

    @classmethod
    def from_reference_file(cls, path, dtype="auto", device="cuda", chunk=1024):
        """The pickle the RAG model reads (rag_model_blip.py:305-311): a dict with "item_embeddings" and "item_embedding_mask",
        two parallel lists of per-passage arrays, and the dict "passage_index2id"."""
        with open(path, "rb") as f:
            data = pickle.load(f)
        return cls.from_padded(data["item_embeddings"], data["item_embedding_mask"], data.get("passage_index2id"), dtype=dtype,
                               device=device, chunk=chunk)

    def __len__(self):
        return self.embeddings.size(0)

    @property
    def dtype(self):
        return self.embeddings.dtype

    @property
    def device(self):
        return self.embeddings.device

    @property
    def nbytes(self):
        return self.embeddings.numel() * self.embeddings.element_size() + self.mask.numel()

    def _checked(self, pids):
        pids = torch.as_tensor(pids).to(self.device)
        if pids.numel() and int(pids.max()) >= len(self):   # one device reduction; < 0 is an empty slot
            raise IndexError(f"pid {int(pids.max())} is outside the store's {len(self)} passages")
        return pids

    def score(self, Q, pids, config=None):
        """Q [n, Nq, 128] (fp32 / fp16 / bf16, widened exactly), pids [n, k] (< 0 = empty slot, scored as an all-padded document)
        -> f32 [n, k], differentiable in Q; dQ comes back in Q's dtype.  'flipr' reduces the differentiable column maxima with
        scoring.reduce_colmax.  Raises IndexError for a pid >= len(self) before anything is launched: that check is one device
        reduction whose result the host waits for, so every call synchronises with the device once."""
        pids = self._checked(pids)
        return scoring.maxsim_gather_differentiable(Q.to(self.device), self.embeddings, self.mask, pids, config)

    def lookup(self, pids, dtype=torch.float32):
        """The padded copy, for callers that do want it: pids [...] -> (D [pids.numel(), Ld, 128] in `dtype`, mask bool
        [pids.numel(), Ld]); an empty slot (pid < 0) is a zero document with an all-zero mask."""
        flat = self._checked(pids).reshape(-1).long()
        live = flat >= 0
        idx = flat.clamp(min=0)
        D = self.embeddings[idx].to(dtype) * live.view(-1, 1, 1).to(dtype)
        return D, self.mask[idx].bool() & live.view(-1, 1)


class CompressedPassageStore:
    """The passage store that is nothing but the searcher's resident compressed index: `scorer` is its IndexScorer (the
    Searcher's `ranker`).  Passage p's embeddings are the rows the reference's CPU branch decompresses and normalises
    (index_storage.py:160-173), formed inside the kernels from codes, residuals and centroids in fp32 -- whatever numerics mode
    the scorer searches in.  Every passage has its own length (no Ld, no mask) and nothing is resident beyond the index."""

    def __init__(self, scorer, passage_index2id=None):
        self.scorer, self.passage_index2id = scorer, passage_index2id

    def __len__(self):
        return int(self.scorer.arrays.num_passages)

    @property
    def device(self):
        return torch.device(scoring._device)

    @property
    def nbytes(self):
        return 0   # nothing beyond the index

    def _checked(self, pids):
        pids = torch.as_tensor(pids).to(self.device)
        end = int(getattr(self.scorer.arrays, "pid_base", 0)) + len(self)
        if pids.numel() and int(pids.max()) >= end:   # one device reduction; < 0 is an empty slot
            raise IndexError(f"pid {int(pids.max())} is outside the index's {len(self)} passages")
        return pids

    def score(self, Q, pids, config=None):
        """Q [n, Nq, 128] (fp32 / fp16 / bf16, widened exactly), pids [n, k] as the scorer's search returns them (< 0 = empty
        slot; a passage of length 0 also scores as an all-padded document) -> f32 [n, k], differentiable in Q; dQ comes back in
        Q's dtype.  'flipr' reduces the differentiable column maxima with scoring.reduce_colmax.  Raises IndexError for a pid
        >= len(self) before anything is launched (one device reduction the host waits for, as PassageEmbeddingStore.score)."""
        pids = self._checked(pids)
        return scoring.maxsim_index_differentiable(Q.to(self.device), self.scorer.device_index, pids, config)

    def lookup(self, pids, dtype=torch.float32):
        """The padded copy, for callers that do want it (through scorer.lookup_pids): pids [...] -> (D [pids.numel(), L, 128]
        in `dtype`, mask bool [pids.numel(), L]) with L the longest of the passages asked for; an empty slot (pid < 0) is a zero
        document with an all-zero mask."""
        flat = self._checked(pids).reshape(-1).long()
        local = flat - int(getattr(self.scorer.arrays, "pid_base", 0))
        live = (flat >= 0).cpu()
        packed, lens = self.scorer.lookup_pids(local[live.to(local.device)].cpu(), out_device=self.device)
        lens_all = torch.zeros(flat.numel(), dtype=torch.int64)
        lens_all[live] = lens.cpu().long()
        L = max(int(lens_all.max()) if flat.numel() else 0, 1)
        mask = (torch.arange(L).unsqueeze(0) < lens_all.unsqueeze(1)).to(self.device)
        D = torch.zeros((flat.numel(), L, packed.size(-1)), dtype=dtype, device=self.device)
        D[mask] = packed.to(dtype)
        return D, mask


class RescoreResult:
    """What `retrieve_and_rescore` returns: pids i32 [B, n_docs] (-1 = empty slot), doc_scores f32 [B, n_docs] with a gradient
    to Q, the index's own scores [B, n_docs] (no gradient) and counts i32 [B] = the filled slots of each row, all on the
    device; `passage_ids` maps the pids through the store's passage_index2id on the host when it is first read."""

    def __init__(self, pids, doc_scores, index_scores, counts, store):
        self.pids, self.doc_scores, self.index_scores, self.counts = pids, doc_scores, index_scores, counts
        self._store, self._passage_ids = store, None

    @property
    def passage_ids(self):
        if self._passage_ids is None:
            m = self._store.passage_index2id
            rows = self.pids.cpu().tolist()
            self._passage_ids = [[None if p < 0 else (m[p] if m is not None else p) for p in row] for row in rows]
        return self._passage_ids


def retrieve_and_rescore(searcher, store, Q, n_docs, n_docs_retrieve=None, generator=None, config=None):
    """One training step's retrieval (rag_model_blip.py:392-443): search the index with Q.detach() on the device, then re-score
    the retrieved passages from `store` (a PassageEmbeddingStore, or a CompressedPassageStore over the searcher's own index:
    anything with `device`, `score` and `passage_index2id`) under autograd.  Q [B, Nq, 128] (with grad) -> RescoreResult.  `config` is the scoring
    model's ColBERT config (its `interaction`; None = 'colbert'), as for scoring.colbert_score_differentiable.

    The search is the batched branch of `Searcher._search_all_Q` (the searcher's k-policy, sticky on its config;
    kk = min(k, ndocs // 4); the checked batch where the ranker has one), so the pids are those `_search_all_Q` ranks, in rank
    order.  As the reference does for n_docs < 5 (:392-395, :412-413), max(n_docs, 5) passages are retrieved (or
    `n_docs_retrieve`) and n_docs of them kept, chosen uniformly without replacement per query -- here by `generator` (a torch
    generator of the store's device) and with the kept ones left in rank order, which `random.sample` does not guarantee; the
    reference draws from Python's unseeded `random`, so there is no sequence to reproduce.  A query for which the index returned
    fewer than n_docs passages keeps them all and has empty slots (pid -1, score of an all-padded document, no gradient) where
    the reference's `random.sample` / `np.array` would raise."""
    n_docs = int(n_docs)
    if n_docs < 1:
        raise ValueError(f"n_docs = {n_docs}")
    k = int(n_docs_retrieve) if n_docs_retrieve is not None else max(n_docs, 5)
    if k < n_docs:
        raise ValueError(f"n_docs_retrieve = {k} < n_docs = {n_docs}")
    searcher._apply_k_policy(k)
    c, ranker = searcher.config, searcher.ranker
    kk = min(k, max(c.ndocs // 4, 1))
    search = getattr(ranker, "search_batch_checked", None) or ranker.search_batch
    pids, scores, counts = search(Q.detach(), kk, c.ncells, c.centroid_score_threshold, c.ndocs, c.query_maxlen)
    if not hasattr(ranker, "search_batch_checked") and hasattr(ranker, "check"):
        ranker.check()
    pids, scores, counts = pids.to(store.device), scores.to(store.device), counts.to(store.device)
    slot = torch.arange(kk, device=store.device).unsqueeze(0)
    pids = torch.where(slot < counts.unsqueeze(1), pids, torch.full_like(pids, -1))
    if n_docs < kk:
        # a uniform draw without replacement among each row's filled slots: random keys, empty slots last, the n_docs smallest
        key = torch.rand(pids.shape, generator=generator, device=store.device).masked_fill(pids < 0, 2.0)
        keep = key.argsort(dim=1)[:, :n_docs].sort(dim=1).values
        pids, scores = pids.gather(1, keep), scores.gather(1, keep)
    elif n_docs > kk:   # (the policy's ndocs // 4 bound: fewer columns than asked for)
        pad = (pids.size(0), n_docs - kk)
        pids = torch.cat([pids, pids.new_full(pad, -1)], dim=1)
        scores = torch.cat([scores, scores.new_zeros(pad)], dim=1)
    counts = (pids >= 0).sum(dim=1).to(torch.int32)
    doc_scores = store.score(Q, pids.contiguous(), config)
    return RescoreResult(pids, doc_scores, scores, counts, store)


# ---- the marginalised loss (rag_model_blip.py:826-1026) -----------------------------------------------------------------------
LOSS_TYPES = ("Approach1", "Approach2", "Approach3", "Approach4", "Approach5", "Approach6", "NoPR")
LOSS_NAMES = ("nll_loss", "rag_loss", "additional_loss")


class _TokenLL(torch.autograd.Function):
    """log_softmax(logits).gather(-1, target), masked, without the log-probabilities: saves the logits the caller already holds,
    the target and lse f32 [R, T, 2]; the backward writes dlogits once, in the logits' dtype."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        ll, lse, first_argmax = ops.rag_token_ll_fwd(logits.detach(), target, ignore_index)
        ctx.save_for_backward(logits, target, lse)
        ctx.ignore_index = ignore_index
        ctx.mark_non_differentiable(first_argmax)
        return ll, first_argmax

    @staticmethod
    def backward(ctx, grad_ll, _):
        logits, target, lse = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        dlogits = ops.rag_token_ll_bwd(logits.detach(), target, lse, grad_ll.float().contiguous(), ctx.ignore_index)
        return dlogits, None, None


def token_log_likelihood(seq_logits, target, ignore_index=-100):
    """seq_logits [R, T, V] (fp32 / fp16 / bf16; any strides with a unit last one are read in place), target integers [R, T] ->
    (ll f32 [R, T], first_argmax i32 [R]).  ll[r, t] = log_softmax(seq_logits[r, t])[target[r, t]] in fp32, 0 where the target is
    ignore_index (those positions are never read), differentiable with respect to the logits (the gradient comes back in their
    dtype); first_argmax[r] = the lowest index of the maximum of seq_logits[r, 0].  A target that is neither ignore_index nor in
    [0, V) raises IndexError before anything is launched (one device reduction the host waits for); `target` is not modified."""
    if seq_logits.dim() != 3 or tuple(target.shape) != tuple(seq_logits.shape[:2]):
        raise ValueError(f"seq_logits {tuple(seq_logits.shape)} / target {tuple(target.shape)}: expected [R, T, V] and [R, T]")
    return _TokenLL.apply(seq_logits, target, int(ignore_index))


def _merged_labels(loss_type, prediction_labels, retrieval_labels):
    """The reference's seven RAVQA_loss_type rules (:942-1000) -> (merged_labels f32, ignore_mask bool), both [B, n_docs]."""
    pred, ret = prediction_labels, retrieval_labels != 0
    either, both = (pred | ret).float(), (pred & ret).float()
    if loss_type == "Approach1":
        return either, either == 0
    if loss_type == "Approach2":
        return either, pred & ~ret
    if loss_type == "Approach3":
        return either, ~ret
    if loss_type == "Approach4":
        return retrieval_labels, pred & ~ret
    if loss_type == "Approach5":
        return both, both == 0
    if loss_type == "Approach6":
        return both, pred ^ ret
    if loss_type == "NoPR":
        return pred.float(), torch.zeros_like(pred)
    raise ValueError(f"loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")


def marginalised_loss(seq_logits, doc_scores, target, n_docs, bos_token_id=None, ignore_index=-100, retrieval_labels=None,
                      loss_type=None, reduce_loss=True, want=LOSS_NAMES):
    """`RagModelForBlip.get_loss` (rag_model_blip.py:826-1026): seq_logits [B * n_docs, T, V], doc_scores [B, n_docs] (what
    retrieve_and_rescore returns, with its gradient to Q), target [B * n_docs, T] -> a dict with the keys named in `want`:

      nll_loss         -ll [B, n_docs, T]; with reduce_loss its sum over the count of positions that are not ignore_index;
      rag_loss         -sum_b logsumexp_d (sum_t ll[b, d, t] + log_softmax(doc_scores)[b, d]), the document term dropped where
                       position p of (b, d) is ignored or p >= T; p = 1 when bos_token_id is given and every target row starts
                       with it, else 0 (the position the reference adds doc_logprobs at, :866-874);
      additional_loss  binary_cross_entropy(softmax(doc_scores), merged labels), masked, over its non-zero count (0 when that is
                       0 or retrieval_labels is None); labels merged by `loss_type` (the model config's RAVQA_loss_type) from
                       retrieval_labels [B, n_docs] and prediction_labels = (argmax of the first position's logits == the first
                       target, which the reference reads as 0 where it is ignored and ignore_index < 0, :877-884, :933).

    ll comes from token_log_likelihood, in fp32 whatever the logits' dtype; the rest is torch on [B, n_docs, T] or smaller (summed in
    fp64, returned in fp32), and the gradient to doc_scores is plain autograd.  The reference fills the ignored entries of the caller's `target` with 0 in
    place; here `target` is left as it was."""
    unknown = [w for w in want if w not in LOSS_NAMES]
    if unknown:
        raise ValueError(f"want holds {unknown}; the losses are {LOSS_NAMES}")
    n_docs = int(n_docs)
    if seq_logits.dim() != 3 or n_docs < 1 or seq_logits.size(0) % n_docs:
        raise ValueError(f"seq_logits {tuple(seq_logits.shape)} with n_docs = {n_docs}: expected [B * n_docs, T, V]")
    R, T, _ = seq_logits.shape
    B = R // n_docs
    if tuple(doc_scores.shape) != (B, n_docs) or target.numel() != R * T:
        raise ValueError(f"doc_scores {tuple(doc_scores.shape)} / target {tuple(target.shape)}: expected {(B, n_docs)} and {(R, T)}")
    additional = "additional_loss" in want and retrieval_labels is not None
    need_ll = "nll_loss" in want or "rag_loss" in want
    out = {}
    if need_ll or additional:
        target = target.reshape(R, T).to(seq_logits.device)
        ll, first_argmax = token_log_likelihood(seq_logits, target, ignore_index)
        pad = (target == ignore_index).view(B, n_docs, T)
        ll = ll.view(B, n_docs, T)
    # past ll everything is small: the sums run in fp64 (their cost is nothing, and the posterior over documents -- the gradient
    # that reaches Q -- then carries the rounding of ll alone); the results come back in ll's fp32
    if "nll_loss" in want:
        out["nll_loss"] = (-ll.double().sum() / (~pad).sum()).to(ll.dtype) if reduce_loss else -ll
    if "rag_loss" in want:
        use_bos = bos_token_id is not None and T > 0 and bool(target[:, 0].eq(bos_token_id).all())
        p = 1 if use_bos else 0
        seq_ll = ll.double().sum(2)
        if p < T:
            doc_logprobs = torch.log_softmax(doc_scores.to(ll.device).double(), dim=1)
            seq_ll = seq_ll + doc_logprobs.masked_fill(pad[:, :, p], 0.0)
        out["rag_loss"] = (-seq_ll.logsumexp(1).sum()).to(ll.dtype)
    if "additional_loss" in want:
        if not additional:
            out["additional_loss"] = doc_scores.new_zeros(())
        else:
            first_target = target[:, 0]
            if ignore_index < 0:
                first_target = first_target.masked_fill(first_target == ignore_index, 0)
            prediction_labels = (first_argmax == first_target).view(B, n_docs)
            labels = torch.as_tensor(retrieval_labels).to(seq_logits.device).double().view(B, n_docs)
            merged, ignore = _merged_labels(loss_type, prediction_labels, labels)
            scores = doc_scores.to(seq_logits.device).double()
            dist = torch.nn.functional.binary_cross_entropy(torch.softmax(scores, dim=-1), merged.double(), reduction="none")
            dist = dist.masked_fill(ignore, 0.0)
            # (count 0 means every entry is 0: the sum over max(count, 1) is then the reference's 0, without a host round trip)
            out["additional_loss"] = (dist.sum() / torch.count_nonzero(dist).clamp(min=1)).to(doc_scores.dtype)
    return out
