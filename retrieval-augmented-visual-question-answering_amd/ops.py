"""torch-tensor front-ends of the op-level C-ABI entry points, with the reference's pybind signatures:

    filter_pids(pids, centroid_scores, codes, doclens, offsets, idx, nfiltered_docs)      filter_pids.cpp:126-164
    decompress_residuals(pids, lengths, offsets, bucket_weights, reversed_bit_map,
                         bucket_weight_combinations, binary_residuals, codes, centroids, dim, nbits)
                                                                                   decompress_residuals.cpp:80-155
    segmented_lookup(input, pids, lengths, offsets)                                segmented_lookup.cpp:127-144
    segmented_maxsim(scores, lengths)                                              segmented_maxsim.cpp:49-93

and of the training-side pairs (padded / gathered / index MaxSim forward and backward, the RAG loss's token log-likelihoods).

Inputs may be CPU tensors (as the reference passes them): they are staged to HBM, the HIP kernel runs, and the
result comes back as a CPU tensor like the reference's.  CUDA inputs are used in place.  There is no CPU
implementation behind these functions.
"""
import ctypes as C

import torch

from . import _native


def _d(t, dtype=None):
    t = torch.as_tensor(t)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.to("cuda").contiguous()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- operand dtypes of the padded MaxSim ----------------------------------------------------------------------------------
# (Q dtype, D dtype) pairs the kernels take as they are (flmr_colbert_*_typed).  Every other pair -- bf16, fp64, and fp16 Q with
# fp32 D, which no caller produces -- is widened exactly to fp32 first, as before.
MAXSIM_NATIVE_PAIRS = frozenset({(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float16, torch.float16)})


def maxsim_native_pair(q_dtype, d_dtype):
    """True when the padded MaxSim runs on these operand dtypes without a widened copy."""
    return (q_dtype, d_dtype) in MAXSIM_NATIVE_PAIRS


def _aligned(t):
    """CUDA, contiguous, dtype kept; copied when the storage offset breaks the 16-byte alignment the kernels' row loads need."""
    t = torch.as_tensor(t).to("cuda").contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _maxsim_operands(Q, D):
    """-> (Q, D, typed): the operands as given for a half pair (typed entry points), else both as fp32 (the fp32 entry points)."""
    Q, D = torch.as_tensor(Q), torch.as_tensor(D)
    if maxsim_native_pair(Q.dtype, D.dtype) and D.dtype == torch.float16:
        return _aligned(Q), _aligned(D), True
    return _d(Q, torch.float32), _d(D, torch.float32), False


def _ft(dtype):
    return _native.FLMR_F16 if dtype == torch.float16 else _native.FLMR_F32


def filter_pids(pids, centroid_scores, codes, doclens, offsets, idx, nfiltered_docs, _codes_dev=None, _offsets_dev=None):
    lib = _native.load()
    pd, cs = _d(pids, torch.int32), _d(centroid_scores, torch.float32)
    cd = _codes_dev if _codes_dev is not None else _d(codes, torch.int32)
    od = _offsets_dev if _offsets_dev is not None else _d(offsets, torch.int64)
    dl = _d(doclens, torch.int64)
    ix = _d(idx, torch.bool).view(torch.uint8)
    out = torch.empty(max(nfiltered_docs // 4, 1), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    _native.check(lib.flmr_filter_pids(_p(pd), pd.numel(), _p(cs), cs.size(0), cs.size(1), _p(cd), _p(dl), _p(od), _p(ix),
                                       int(nfiltered_docs), _p(out), _p(cnt), _native.stream_ptr()))
    return out[: int(cnt.item())].cpu()


def decompress_residuals(pids, lengths, offsets, bucket_weights, reversed_bit_map, bucket_weight_combinations,
                         binary_residuals, codes, centroids, dim, nbits, _on_device=False):
    lib = _native.load()
    pd = _d(pids, torch.int32)
    ln, of = _d(lengths, torch.int64), _d(offsets, torch.int64)
    nrows = int(torch.as_tensor(lengths).long()[torch.as_tensor(pids).long()].sum()) if pd.numel() else 0
    out = torch.zeros((nrows, dim), dtype=torch.float32, device="cuda")
    # keep every staged tensor referenced until the (synchronous) call returns
    bw, rbm, lut = _d(bucket_weights, torch.float32), _d(reversed_bit_map, torch.uint8), _d(bucket_weight_combinations, torch.uint8)
    res, cod, cen = _d(binary_residuals, torch.uint8), _d(codes, torch.int32), _d(centroids, torch.float32)
    if pd.numel():
        _native.check(lib.flmr_decompress_residuals(
            _p(pd), pd.numel(), _p(ln), _p(of), _p(bw), _p(rbm), _p(lut), _p(res), _p(cod), _p(cen), int(dim), int(nbits),
            _p(out), nrows, None, _native.stream_ptr()))
    return out if _on_device else out.cpu()


def segmented_lookup(input, pids, lengths, offsets):
    lib = _native.load()
    inp = torch.as_tensor(input)
    ind = inp.to("cuda").contiguous()
    ln, of = _d(lengths, torch.int64), _d(offsets, torch.int64)
    nrows = int(torch.as_tensor(lengths).long().sum())
    out = torch.zeros((nrows,) + tuple(inp.shape[1:]), dtype=inp.dtype, device="cuda")
    row_bytes = inp.element_size() * (int(torch.tensor(inp.shape[1:]).prod()) if inp.dim() > 1 else 1)
    if ln.numel():
        _native.check(lib.flmr_segmented_lookup(_p(ind), row_bytes, _p(ln), _p(of), ln.numel(), _p(out), nrows, None,
                                                _native.stream_ptr()))
    return out.cpu() if not inp.is_cuda else out


def segmented_maxsim(scores, lengths):
    lib = _native.load()
    sc, ln = _d(scores, torch.float32), _d(lengths, torch.int64)
    out = torch.zeros(ln.numel(), dtype=torch.float32, device="cuda")
    if ln.numel():
        _native.check(lib.flmr_segmented_maxsim(_p(sc), _p(ln), ln.numel(), sc.size(1), _p(out), _native.stream_ptr()))
    return out.cpu() if not torch.as_tensor(scores).is_cuda else out


def colbert_score_padded(Q, D_padded, D_mask):
    """Forward-only padded MaxSim (colbert.py:268-286): Q [1|B, Nq, d], D [B, Ld, d], mask [B, Ld(,1)] -> f32 [B].  fp16 D with
    fp16 or fp32 Q is scored as it is (flmr_colbert_score_typed: no fp32 copy, no workspace, no synchronise), with the bits of the
    fp32 kernel on the widened operands; every other dtype pair is widened exactly to fp32."""
    lib = _native.load()
    Qd, Dd, typed = _maxsim_operands(Q, D_padded)
    B, Ld, dim = Dd.shape
    md = _d(torch.as_tensor(D_mask).reshape(B, Ld), torch.bool).view(torch.uint8)
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    if typed:
        if B:
            _native.check(lib.flmr_colbert_score_typed(_p(Qd), _ft(Qd.dtype), Qd.size(0), Qd.size(1), _p(Dd), _ft(Dd.dtype), _p(md), B, Ld,
                                                       dim, 0, _p(out), None, _native.stream_ptr()))
        return out
    _native.check(lib.flmr_colbert_score_padded(_p(Qd), Qd.size(0), Qd.size(1), _p(Dd), _p(md), B, Ld, dim, _p(out),
                                                _native.stream_ptr()))
    return out


def colbert_score_cross(Q, D_padded, D_mask):
    """Every query against every document in ONE launch: Q [nqueries, Nq, d], D [B, Ld, d], mask [B, Ld(,1)] -> [nqueries, B]
    (the rate matrix of the executor's exhaustive search, FLMR_executor.py:799-847).  Operand dtypes as colbert_score_padded."""
    lib = _native.load()
    Qd, Dd, typed = _maxsim_operands(Q, D_padded)
    B, Ld, dim = Dd.shape
    md = _d(torch.as_tensor(D_mask).reshape(B, Ld), torch.bool).view(torch.uint8)
    out = torch.empty((Qd.size(0), B), dtype=torch.float32, device="cuda")
    if typed:
        if B and Qd.size(0):
            _native.check(lib.flmr_colbert_score_typed(_p(Qd), _ft(Qd.dtype), Qd.size(0), Qd.size(1), _p(Dd), _ft(Dd.dtype), _p(md), B, Ld,
                                                       dim, 1, _p(out), None, _native.stream_ptr()))
        return out
    _native.check(lib.flmr_colbert_score_cross(_p(Qd), Qd.size(0), Qd.size(1), _p(Dd), _p(md), B, Ld, dim, _p(out),
                                               _native.stream_ptr()))
    return out


def colbert_colmax_padded(Q, D_padded, D_mask):
    """The per-column maxima [B, Nq] of the padded MaxSim (-9999 padding) before their sum: what `colbert_score_reduce`
    reduces -- by a plain sum for 'colbert', by top-k sums for 'flipr' (colbert.py:235-263).  Operand dtypes as
    colbert_score_padded."""
    lib = _native.load()
    Qd, Dd, typed = _maxsim_operands(Q, D_padded)
    B, Ld, dim = Dd.shape
    md = _d(torch.as_tensor(D_mask).reshape(B, Ld), torch.bool).view(torch.uint8)
    out = torch.empty((B, Qd.size(1)), dtype=torch.float32, device="cuda")
    if typed:
        if B:
            _native.check(lib.flmr_colbert_score_typed(_p(Qd), _ft(Qd.dtype), Qd.size(0), Qd.size(1), _p(Dd), _ft(Dd.dtype), _p(md), B, Ld,
                                                       dim, 0, None, _p(out), _native.stream_ptr()))
        return out
    _native.check(lib.flmr_colbert_colmax_padded(_p(Qd), Qd.size(0), Qd.size(1), _p(Dd), _p(md), B, Ld, dim, _p(out),
                                                 _native.stream_ptr()))
    return out


def _maxsim_fwd_outputs(lead, nq, want_out, want_colmax, empty, launch):
    """The outputs of a MaxSim forward: allocates (out f32 [*lead] | None, colmax f32 [*lead, nq] | None, argmax i32 [*lead, nq])
    and has launch(out, colmax, argmax) fill them, unless the batch is `empty` (empty tensors may have NULL data pointers, which
    the C ABI rejects)."""
    out = torch.empty(lead, dtype=torch.float32, device="cuda") if want_out else None
    colmax = torch.empty(lead + (nq,), dtype=torch.float32, device="cuda") if want_colmax else None
    argmax = torch.empty(lead + (nq,), dtype=torch.int32, device="cuda")
    if not empty:
        launch(out, colmax, argmax)
    return out, colmax, argmax


def colbert_maxsim_fwd(Q, D_padded, D_mask, cross=False, want_out=True, want_colmax=False):
    """The autograd forward (flmr_colbert_maxsim_fwd / _fwd_typed): CUDA Q [q_batch, Nq, 128], D [B, Ld, 128], mask [B, Ld(,1)] ->
    (out f32 [rows] | None, colmax f32 [rows, Nq] | None, argmax i32 [rows, Nq]); rows = B, or q_batch * B query-major when
    `cross` (returned there as [q_batch, B] / [q_batch, B, Nq]).  argmax = the winning token, lowest on ties, -1 where the
    winner is padded.  out / colmax are bit-identical to colbert_score_padded / colbert_score_cross / colbert_colmax_padded.
    Native operand dtypes (MAXSIM_NATIVE_PAIRS): fp32 Q and D; fp16 D with fp32 or fp16 Q, read as they are with the bits of the
    fp32 kernel on the widened values.  Any other pair is widened exactly to fp32.  Enqueued on the current stream, no
    synchronisation."""
    lib = _native.load()
    Qd, Dd, typed = _maxsim_operands(Q, D_padded)
    B, Ld, dim = Dd.shape
    nQ, nq = Qd.size(0), Qd.size(1)
    md = _d(torch.as_tensor(D_mask).reshape(B, Ld), torch.bool).view(torch.uint8)

    def launch(out, colmax, argmax):
        if typed:
            _native.check(lib.flmr_colbert_maxsim_fwd_typed(_p(Qd), _ft(Qd.dtype), nQ, nq, _p(Dd), _ft(Dd.dtype), _p(md), B, Ld, dim,
                                                            int(bool(cross)), _p(out), _p(colmax), _p(argmax), _native.stream_ptr()))
        else:
            _native.check(lib.flmr_colbert_maxsim_fwd(_p(Qd), nQ, nq, _p(Dd), _p(md), B, Ld, dim, int(bool(cross)), _p(out), _p(colmax),
                                                      _p(argmax), _native.stream_ptr()))
    return _maxsim_fwd_outputs((nQ, B) if cross else (B,), nq, want_out, want_colmax, B == 0, launch)


def colbert_maxsim_bwd(Q, D_padded, argmax, grad_colmax, cross=False, need_dQ=True, need_dD=True, dq_dtype=torch.float32,
                       dd_dtype=torch.float32):
    """The autograd backward (flmr_colbert_maxsim_bwd / _bwd_typed): from the forward's argmax and G = dL/dcolmax (shaped like
    argmax) -> (dQ [q_batch, Nq, 128] | None in dq_dtype, dD [B, Ld, 128] | None in dd_dtype; fp32 unless asked otherwise).
    Operand dtypes as colbert_maxsim_fwd.  The sums are fp32 in a fixed order; an fp16 gradient is written by the kernel itself,
    rounded once (the bits of the fp32 gradient `.to(torch.float16)`); any other gradient dtype is converted from the fp32 result.
    Deterministic; enqueued on the current stream."""
    lib = _native.load()
    Qd, Dd, typed = _maxsim_operands(Q, D_padded)
    kdt = (torch.float32, torch.float16)
    oq, od = (dq_dtype if typed and dq_dtype in kdt else torch.float32), (dd_dtype if typed and dd_dtype in kdt else torch.float32)
    B, Ld, dim = Dd.shape
    nQ, nq = Qd.size(0), Qd.size(1)
    am, G = _d(argmax, torch.int32), _d(grad_colmax, torch.float32)
    rows = nQ * B if cross else B
    assert am.numel() == rows * nq and G.numel() == rows * nq, (tuple(am.shape), tuple(G.shape), rows, nq)
    dQ = torch.empty(Qd.shape, dtype=oq, device="cuda") if need_dQ else None
    dD = torch.empty(Dd.shape, dtype=od, device="cuda") if need_dD else None
    if B == 0:
        if dQ is not None:
            dQ.zero_()
    elif typed:
        _native.check(lib.flmr_colbert_maxsim_bwd_typed(_p(Qd), _ft(Qd.dtype), nQ, nq, _p(Dd), _ft(Dd.dtype), B, Ld, dim, int(bool(cross)),
                                                        _p(am), _p(G), _p(dQ), _ft(oq), _p(dD), _ft(od), _native.stream_ptr()))
    else:
        _native.check(lib.flmr_colbert_maxsim_bwd(_p(Qd), nQ, nq, _p(Dd), B, Ld, dim, int(bool(cross)), _p(am), _p(G), _p(dQ), _p(dD),
                                                  _native.stream_ptr()))
    return (dQ.to(dq_dtype) if dQ is not None else None), (dD.to(dd_dtype) if dD is not None else None)


def _store_dtype(store):
    if store.dtype == torch.float16:
        return _native.FLMR_F16
    if store.dtype == torch.float32:
        return _native.FLMR_F32
    raise TypeError(f"the passage store is fp32 or fp16, not {store.dtype}")


def maxsim_gather_fwd(Q, store, store_mask, pids, want_out=True, want_colmax=False):
    """The gathered autograd forward (flmr_maxsim_gather_fwd): fp32 CUDA Q [n, Nq, 128], a resident store [P, Ld, 128] (fp32 or
    fp16, used in place: never copied or widened), store_mask [P, Ld] (uint8 / bool), pids i32 [n, k] (< 0 = empty slot) ->
    (out f32 [n, k] | None, colmax f32 [n, k, Nq] | None, argmax i32 [n, k, Nq]).  Row (q, j) is query q against passage
    pids[q, j]; an fp32 store gives the bits of colbert_maxsim_fwd on Q.repeat_interleave(k) and store[pids], an fp16 store the
    bits of the fp32 store of the widened values.  pids >= P are the caller's error (rag.PassageEmbeddingStore validates).
    Enqueued on the current stream, no synchronisation."""
    lib = _native.load()
    Qd, pd = _d(Q, torch.float32), _d(pids, torch.int32)
    sd = store.to("cuda").contiguous()
    P, Ld, dim = sd.shape
    md = torch.as_tensor(store_mask).reshape(P, Ld)
    md = _d(md) if md.dtype == torch.uint8 else _d(md, torch.bool).view(torch.uint8)   # (a resident uint8 mask is used in place)
    n, nq = Qd.size(0), Qd.size(1)
    assert pd.dim() == 2 and pd.size(0) == n, (tuple(pd.shape), n)
    k = pd.size(1)

    def launch(out, colmax, argmax):
        _native.check(lib.flmr_maxsim_gather_fwd(_p(Qd), n, nq, _p(sd), _store_dtype(sd), _p(md), P, Ld, dim, _p(pd), k, _p(out),
                                                 _p(colmax), _p(argmax), _native.stream_ptr()))
    return _maxsim_fwd_outputs((n, k), nq, want_out, want_colmax, n * k == 0, launch)


def maxsim_gather_bwd(store, pids, argmax, grad_colmax):
    """The gathered autograd backward (flmr_maxsim_gather_bwd): the forward's argmax and G = dL/dcolmax, both [n, k, Nq] ->
    dQ f32 [n, Nq, 128], each (q, i) summed over the query's k passages in ascending j.  There is no store gradient.
    Deterministic; enqueued on the current stream."""
    lib = _native.load()
    sd = store.to("cuda").contiguous()
    P, Ld, dim = sd.shape
    pd, am, G = _d(pids, torch.int32), _d(argmax, torch.int32), _d(grad_colmax, torch.float32)
    n, k, nq = am.shape
    assert tuple(pd.shape) == (n, k) and G.shape == am.shape, (tuple(pd.shape), tuple(am.shape), tuple(G.shape))
    if n * k == 0:
        return torch.zeros((n, nq, dim), dtype=torch.float32, device="cuda")
    dQ = torch.empty((n, nq, dim), dtype=torch.float32, device="cuda")
    _native.check(lib.flmr_maxsim_gather_bwd(_p(sd), _store_dtype(sd), P, Ld, dim, _p(pd), n, k, nq, _p(am), _p(G), _p(dQ),
                                             _native.stream_ptr()))
    return dQ


def maxsim_index_fwd(device_index, Q, pids, want_out=True, want_colmax=False):
    """The gathered autograd forward with the compressed index as the document source (flmr_maxsim_index_fwd): a resident
    index.DeviceIndex, fp32 CUDA Q [n, Nq, 128], pids i32 [n, k] as search_batch returns them (< 0, outside the index or a
    passage of length 0: an all-padded document) -> (out f32 [n, k] | None, colmax f32 [n, k, Nq] | None, argmax i32 [n, k, Nq]).
    Row (q, j) is query q against the decompressed, normalised tokens of passage pids[q, j] (index_storage.py:160-173), -9999
    padding, no zero clamp.  Enqueued on the current stream, no synchronisation."""
    lib = _native.load()
    Qd, pd = _d(Q, torch.float32), _d(pids, torch.int32)
    n, nq = Qd.size(0), Qd.size(1)
    assert Qd.dim() == 3 and pd.dim() == 2 and pd.size(0) == n, (tuple(Qd.shape), tuple(pd.shape))
    k = pd.size(1)

    def launch(out, colmax, argmax):
        if Qd.size(2) != device_index.arrays.dim:
            raise ValueError(f"Q has dim {Qd.size(2)}, the index {device_index.arrays.dim}")
        _native.check(lib.flmr_maxsim_index_fwd(device_index.handle, _p(Qd), n, nq, _p(pd), k, _p(out), _p(colmax), _p(argmax),
                                                _native.stream_ptr()))
    return _maxsim_fwd_outputs((n, k), nq, want_out, want_colmax, n * k == 0, launch)


def maxsim_index_bwd(device_index, pids, argmax, grad_colmax):
    """The backward of maxsim_index_fwd (flmr_maxsim_index_bwd): the forward's argmax and G = dL/dcolmax, both [n, k, Nq] ->
    dQ f32 [n, Nq, 128], each (q, i) summed over the query's k passages in ascending j, the winner rows decoded from the index.
    The index is a constant: there is no other gradient.  Deterministic; enqueued on the current stream."""
    lib = _native.load()
    pd, am, G = _d(pids, torch.int32), _d(argmax, torch.int32), _d(grad_colmax, torch.float32)
    n, k, nq = am.shape
    assert tuple(pd.shape) == (n, k) and G.shape == am.shape, (tuple(pd.shape), tuple(am.shape), tuple(G.shape))
    dim = device_index.arrays.dim
    if n * k == 0:
        return torch.zeros((n, nq, dim), dtype=torch.float32, device="cuda")
    dQ = torch.empty((n, nq, dim), dtype=torch.float32, device="cuda")
    _native.check(lib.flmr_maxsim_index_bwd(device_index.handle, _p(pd), n, k, nq, _p(am), _p(G), _p(dQ), _native.stream_ptr()))
    return dQ


# ---- token log-likelihoods of the RAG marginalised loss ---------------------------------------------------------------------
_RAG_DTYPES = {torch.float32: _native.FLMR_F32, torch.float16: _native.FLMR_F16, torch.bfloat16: _native.FLMR_BF16}


def checked_rag_targets(target, R, T, V, ignore_index, device):
    """target [R, T] (any integer dtype) -> contiguous int64 on `device`, used in place when it already is that.  A value that is
    neither ignore_index nor in [0, V) raises IndexError before anything is launched: one device reduction whose result the host
    waits for (as rag.PassageEmbeddingStore._checked), so a call synchronises with the device once."""
    tgt = torch.as_tensor(target)
    if tuple(tgt.shape) != (R, T) or tgt.is_floating_point() or tgt.dtype == torch.bool:
        raise ValueError(f"target {tuple(tgt.shape)} {tgt.dtype}: expected integers [{R}, {T}]")
    tgt = tgt.to(device=device, dtype=torch.int64).contiguous()
    bad = ((tgt < 0) | (tgt >= V)) & (tgt != ignore_index)
    if tgt.numel() and bool(bad.any()):
        raise IndexError(f"target {int(tgt[bad][0])} is neither ignore_index ({ignore_index}) nor in [0, {V})")
    return tgt


def _rag_logits(logits):
    """CUDA [R, T, V] fp32 / fp16 / bf16, read in place through its r and t strides; copied only when the last stride is not 1."""
    x = torch.as_tensor(logits)
    if x.dim() != 3 or x.dtype not in _RAG_DTYPES:
        raise TypeError(f"logits {tuple(x.shape)} {x.dtype}: expected [R, T, V] in fp32, fp16 or bf16")
    if x.size(2) < 1:
        raise ValueError("logits with an empty vocabulary")
    x = x.to("cuda")
    if (x.size(2) > 1 and x.stride(2) != 1) or min(x.stride(0), x.stride(1)) < 0:
        x = x.contiguous()
    return x


def rag_token_ll_fwd(logits, target, ignore_index=-100, validate=True):
    """flmr_rag_token_ll_fwd: logits [R, T, V] (fp32 / fp16 / bf16, any r and t strides: a [:, :-1, :] view and a [..., :V] view
    of a wider buffer are read where they are), target [R, T] -> (ll f32 [R, T], lse f32 [R, T, 2], first_argmax i32 [R]).
    ll = logits[target] - logsumexp(logits) per position, in fp32 from one pass over the row; lse holds the log-sum-exp as its two
    words (row maximum, log of the sum of exp(x - maximum)): lse.sum(-1) is the value, the pair is what the backward needs to keep
    probabilities near 1 exact to fp32 roundoff.  Positions whose target is ignore_index are not read and hold ll = 0, lse = (0, 0); first_argmax[r] is the lowest index of the maximum of row (r, 0), ignored or
    not.  Other targets outside [0, V) raise IndexError (checked_rag_targets: the one point where the host waits for the device;
    validate=False skips it for a target already checked -- the kernels treat such a value as ignored, they never index with it).
    Enqueued on the current stream."""
    lib = _native.load()
    x = _rag_logits(logits)
    R, T, V = x.shape
    tgt = checked_rag_targets(target, R, T, V, ignore_index, "cuda") if validate else _d(target, torch.int64)
    ll = torch.empty((R, T), dtype=torch.float32, device="cuda")
    lse = torch.empty((R, T, 2), dtype=torch.float32, device="cuda")
    first = torch.zeros((R,), dtype=torch.int32, device="cuda")
    if R * T == 0:
        return ll, lse, first   # (empty tensors may have NULL data pointers, which the C ABI rejects)
    _native.check(lib.flmr_rag_token_ll_fwd(_p(x), _RAG_DTYPES[x.dtype], R, T, V, x.stride(0), x.stride(1), _p(tgt), int(ignore_index),
                                            _p(ll), _p(lse), _p(first), _native.stream_ptr()))
    return ll, lse, first


def rag_token_ll_bwd(logits, target, lse, grad_ll, ignore_index=-100, out=None):
    """flmr_rag_token_ll_bwd: the forward's logits, target (as the forward validated it) and lse [R, T, 2], and grad_ll = dL/dll [R, T] ->
    dlogits [R, T, V] contiguous in the logits' dtype = grad_ll * (onehot(target) - exp((logits - lse[..., 0]) - lse[..., 1])), the fp32 value rounded
    once.  Every element is written (`out`, if given, may hold anything): ignored positions are zeros and are not read.
    Deterministic; enqueued on the current stream."""
    lib = _native.load()
    x = _rag_logits(logits)
    R, T, V = x.shape
    tgt = _d(target, torch.int64)
    lse_d, g = _d(lse, torch.float32), _d(grad_ll, torch.float32)
    assert tuple(tgt.shape) == (R, T) and tuple(lse_d.shape) == (R, T, 2) and tuple(g.shape) == (R, T), (tuple(x.shape), tuple(tgt.shape),
                                                                                                   tuple(lse_d.shape), tuple(g.shape))
    if out is None:
        out = torch.empty((R, T, V), dtype=x.dtype, device="cuda")
    elif not (out.is_cuda and out.dtype == x.dtype and tuple(out.shape) == (R, T, V) and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous CUDA {x.dtype} tensor {(R, T, V)}")
    if R * T == 0:
        return out
    _native.check(lib.flmr_rag_token_ll_bwd(_p(x), _RAG_DTYPES[x.dtype], R, T, V, x.stride(0), x.stride(1), _p(tgt), int(ignore_index),
                                            _p(lse_d), _p(g), _p(out), _native.stream_ptr()))
    return out


def merge_topk(scores, pids):
    """scores f32 / pids i32 [nshards, nqueries, k] (CUDA) -> merged (scores, pids, counts) [nqueries, k]."""
    lib = _native.load()
    sc, pd = _d(scores, torch.float32), _d(pids, torch.int32)
    R, n, k = sc.shape
    os_ = torch.empty((n, k), dtype=torch.float32, device="cuda")
    op = torch.empty((n, k), dtype=torch.int32, device="cuda")
    oc = torch.empty((n,), dtype=torch.int32, device="cuda")
    _native.check(lib.flmr_merge_topk(_p(sc), _p(pd), R, n, k, _p(os_), _p(op), _p(oc), _native.stream_ptr()))
    return os_, op, oc


def topn_keys(keys, n, ordered=True):
    """keys int64 [nq, m] (u64 bit patterns: score bits << 32 | pid, 0 = empty) -> the n largest per row, descending;
    ordered=False: the same set in arbitrary order (radix select, any m)."""
    lib = _native.load()
    kd = keys.to("cuda").contiguous()
    out = torch.empty((kd.size(0), n), dtype=torch.int64, device="cuda")
    if not ordered:
        _native.check(lib.flmr_select_keys(_p(kd), kd.size(0), kd.size(1), int(n), _p(out), _native.stream_ptr()))
        return out
    if kd.size(1) > 2048 and kd.size(1) > 2 * n:
        # long rows: radix-select the n survivors first, then sort only those (a bitonic sort of 8192 keys per row costs
        # five times as much); the result is the same descending list
        kd = topn_keys(kd, n, ordered=False)
    _native.check(lib.flmr_topn_keys(_p(kd), kd.size(0), kd.size(1), int(n), _p(out), None, _native.stream_ptr()))
    return out


def unpack_keys(keys, k):
    """descending keys int64 [nq, n] -> (pids i32 [nq,k], scores f32 [nq,k], counts i32 [nq])."""
    lib = _native.load()
    kd = keys.to("cuda").contiguous()
    nq = kd.size(0)
    op = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    os_ = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    oc = torch.empty((nq,), dtype=torch.int32, device="cuda")
    _native.check(lib.flmr_unpack_keys(_p(kd), nq, kd.size(1), int(k), _p(op), _p(os_), _p(oc), _native.stream_ptr()))
    return op, os_, oc


# ---- index build (include/flmr_hip.h "Index build ops"; residual.py:169-222) -------------------------------------------
def nearest_centroids(embs, centroids):
    """codes int32 [N] = argmax_c centroids[c] . embs[t] (residual.py:206-216); centroids must be fp16-representable."""
    lib = _native.load()
    e, c = _d(embs, torch.float32), _d(centroids, torch.float32)
    assert e.dim() == 2 and e.size(1) == 128 and c.size(1) == 128
    out = torch.empty(e.size(0), dtype=torch.int32, device="cuda")
    _native.check(lib.flmr_nearest_centroids(_p(c), c.size(0), _p(e), e.size(0), _p(out), _native.stream_ptr()))
    return out


def compress_residuals(embs, centroids, codes, bucket_cutoffs, nbits):
    """packed residual bytes uint8 [N, 16*nbits] for the given codes (residual.py:186-204)."""
    lib = _native.load()
    e, c = _d(embs, torch.float32), _d(centroids, torch.float32)
    cd, cut = _d(codes, torch.int32), _d(bucket_cutoffs, torch.float32)
    assert cut.numel() == 2 ** nbits - 1, "bucket_cutoffs must hold 2^nbits - 1 values"
    out = torch.empty((e.size(0), 16 * nbits), dtype=torch.uint8, device="cuda")
    _native.check(lib.flmr_compress_residuals(_p(c), c.size(0), _p(e), _p(cd), e.size(0), _p(cut), int(nbits), _p(out),
                                              _native.stream_ptr()))
    return out


def compress(embs, centroids, bucket_cutoffs, nbits):
    """ResidualCodec.compress on the GPU -> (codes int32 [N], residuals uint8 [N, 16*nbits])."""
    codes = nearest_centroids(embs, centroids)
    return codes, compress_residuals(embs, centroids, codes, bucket_cutoffs, nbits)


def compress_f16(embs, centroids, bucket_cutoffs, nbits):
    """ResidualCodec.compress for fp16 token rows in ONE fused pass (flmr_compress_f16) -> (codes int32 [N], residuals uint8
    [N, 16*nbits]): codes = argmax of the fp32-accumulated fp16 dot product, residual bytes identical to
    compress_residuals(embs.float(), ...).  embs must be fp16 (no silent rounding of fp32 rows); centroids fp16, or fp32 values
    that are fp16-representable (what the index stores, residual.py:161)."""
    lib = _native.load()
    if torch.as_tensor(embs).dtype != torch.float16:
        raise TypeError("compress_f16 takes fp16 embeddings (use nearest_centroids + compress_residuals for fp32 rows)")
    e = _d(embs)
    c32 = _d(centroids, torch.float32)
    c = c32.half()
    if not torch.equal(c.float(), c32):
        raise ValueError("centroids must be fp16-representable (the index stores them as half): round them with .half() first")
    cut = _d(bucket_cutoffs, torch.float32)
    assert e.dim() == 2 and e.size(1) == 128 and c.dim() == 2 and c.size(1) == 128
    if nbits in (1, 2, 4, 8):
        assert cut.numel() == 2 ** nbits - 1, "bucket_cutoffs must hold 2^nbits - 1 values"
    codes = torch.empty(e.size(0), dtype=torch.int32, device="cuda")
    res = torch.empty((e.size(0), 16 * max(int(nbits), 1)), dtype=torch.uint8, device="cuda")
    if e.size(0) == 0 and nbits in (1, 2, 4, 8):
        return codes, res   # (empty tensors may have NULL data pointers, which the C ABI rejects)
    _native.check(lib.flmr_compress_f16(_p(c), c.size(0), _p(e), e.size(0), _p(cut), int(nbits), _p(codes), _p(res),
                                        _native.stream_ptr()))
    return codes, res


def build_ivf(codes, doclens, K):
    """(ivf pids int32 [sum unique], ivf_lengths int64 [K]) of an index on the GPU: optimize_ivf (TPC/indexing/utils.py:8-53)
    through flmr_build_ivf -- a stable device radix sort of (code, pid) by code, run flags, compaction."""
    lib = _native.load()
    cd = _d(codes, torch.int32)
    dl = torch.as_tensor(doclens).to(device="cuda", dtype=torch.int64)
    offsets = torch.zeros(dl.numel() + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(dl, 0)
    n = cd.numel()
    assert int(offsets[-1]) == n, "doclens must sum to the number of codes"
    ivf = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    lengths = torch.empty(int(K), dtype=torch.int64, device="cuda")
    import ctypes as C
    total = C.c_int64(0)
    _native.check(lib.flmr_build_ivf(_p(cd), n, _p(offsets), dl.numel(), int(K), _p(ivf), _p(lengths), C.byref(total), _native.stream_ptr()))
    return ivf[: total.value].clone(), lengths

