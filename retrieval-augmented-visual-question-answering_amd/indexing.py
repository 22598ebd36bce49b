"""Index build from token embeddings, written in the reference's on-disk format so that either this
package or the reference's own `Searcher` can read it.  "Next" row 8f-1: what precedes the search path.

Restates the steps of `CollectionIndexer.run` (TPC/indexing/collection_indexer.py:56-73) that do not involve the text
encoder -- the caller supplies the (already L2-normalised) token embeddings and the per-passage token counts:

  setup    num_partitions = 2^floor(log2(16*sqrt(N)))                                   (:93)
  train    k-means on a sample (the reference calls faiss.Kmeans(dim, K, niter=kmeans_niters, seed=123), :447-463; FAISS is
           not available on ROCm here: spherical Lloyd iterations whose assignment step is the HIP argmax kernel -- same
           objective on unit vectors, different RNG, hence validated by Recall, not bit-compared), centroids L2-normalised
           (:283) and stored as half; bucket cut-offs / weights = quantiles of held-out residuals (:286-308)
  index    nearest centroid by dot product, residual, bucketize, bit-pack            (residual.py:169-204)
  finalize IVF = sorted unique pids per centroid                                    (indexing/utils.py:8-53)

Two forms.  `build_index` holds every embedding on the device at once and returns one chunk.  `ChunkedIndexBuilder` follows the
reference's chunked run (collection_indexer.py:321-440): plan -> fit the codec on a sample -> compress and write one chunk of
passages at a time ({i}.codes.pt / {i}.residuals.pt / doclens.{i}.json / {i}.metadata.json, index_saver.py:79-90; chunk i
belongs to rank i % nranks, collection.py:64-81; with `resume` the chunks already on disk are skipped) -> finalize (offsets,
IVF over the codes of all chunks).  It never holds more than one chunk of embeddings; fp16 chunks (what encoders emit) go
through the fused one-pass kernel flmr_compress_f16, fp32 chunks through the two ops below.

Every heavy step runs on the MI355X through the C ABI (`ops`): the nearest-centroid argmax of k-means' assignment step and
of the final compression (flmr_nearest_centroids: the stage-0 fp16-split MFMA kernel with an argmax epilogue), the residual
bucketize + bit-pack (flmr_compress_residuals) and the IVF (flmr_build_ivf).  There is no host fallback in this module: the
embeddings must be on the GPU (tests of the HOST logic -- sampling, the Lloyd loop, the bucket tables, the file format -- pass
`backend=` an object with the same three functions restated in torch, tests/host_build_backend.py, exactly as they inject an
encoder).
"""
import json
import math
import os

import torch

from . import synth
from .index import IndexArrays


class HipBackend:
    """The three device steps of the build, on libflmr_hip.so (fails loudly without it / without a device)."""

    @staticmethod
    def nearest_centroids(x, centroids):
        from . import ops
        return ops.nearest_centroids(x, centroids)

    @staticmethod
    def compress_residuals(x, centroids, codes, cutoffs, nbits):
        from . import ops
        return ops.compress_residuals(x, centroids, codes, cutoffs, nbits)

    @staticmethod
    def compress_f16(x, centroids, cutoffs, nbits):
        from . import ops
        return ops.compress_f16(x, centroids, cutoffs, nbits)

    @staticmethod
    def build_ivf(codes, doclens, K):
        from . import ops
        return ops.build_ivf(codes, doclens, K)


def _require_unit_rows(x, what, n_check=4096):
    """The build assigns by DOT PRODUCT (k-means and the final codes): that is the reference's L2 choice (faiss.Kmeans,
    residual.py:206-220 `(centroids @ batch.T).max`) only for unit-norm rows -- what the encoders emit (colbert.py:207).  A cheap
    check on a strided sample; anything else must be normalised by the caller (silently normalising here would index different
    vectors than the ones handed in)."""
    if x.numel() == 0:
        return
    step = max(1, x.size(0) // n_check)
    nrm = x[::step][:n_check].float().norm(dim=-1)
    if bool(((nrm - 1.0).abs() > 1e-2).any()):
        raise ValueError(f"{what}: rows must be L2-normalised (norms in [{float(nrm.min()):.4f}, {float(nrm.max()):.4f}]); "
                         "the build assigns by dot product, which equals the reference's L2 assignment only on unit vectors")


def _require_device(x, backend, what):
    if backend is HipBackend and not x.is_cuda:
        raise ValueError(f"{what} must be on the GPU for the HIP build (there is no host path here; move the tensor once up "
                         "front, or pass backend= a host implementation as the tests do)")


def num_partitions_for(n_embeddings: int) -> int:
    return int(2 ** math.floor(math.log2(16 * math.sqrt(max(n_embeddings, 1)))))


def kmeans(sample, K, niters=4, seed=123, backend=HipBackend, chunk=1 << 20):
    """Spherical Lloyd iterations on unit-norm points (what the encoders emit, colbert.py:207: `normalize(D, p=2, dim=2)`):
    `niters` rounds from K distinct random sample points; assignment = nearest centroid by dot product -- for unit vectors the
    same choice as L2 -- through `backend.nearest_centroids` with the centroids re-normalised and rounded to fp16 each round
    (the index stores them as half anyway, residual.py:161; the MFMA argmax needs fp16-representable rows); empty clusters
    are re-seeded from random points.  The reference runs faiss.Kmeans (L2, its own RNG): same objective on the sphere,
    different arithmetic, hence validated by Recall, never bit-compared.  Returns fp32 centroids [K, dim] (unit rows)."""
    _require_device(sample, backend, "the k-means sample")
    _require_unit_rows(sample, "kmeans(sample)")
    g = torch.Generator(device=sample.device)
    g.manual_seed(seed)
    n = sample.size(0)
    if n < K:
        raise ValueError(f"k-means needs at least K={K} sample points, got {n}")
    sample = sample.float()
    centroids = sample[torch.randperm(n, generator=g, device=sample.device)[:K]].clone()
    for _ in range(niters):
        centroids = torch.nn.functional.normalize(centroids, dim=-1).half().float()
        assign = torch.empty(n, dtype=torch.long, device=sample.device)
        for i in range(0, n, chunk):
            assign[i:i + chunk] = backend.nearest_centroids(sample[i:i + chunk], centroids).long()
        sums = torch.zeros_like(centroids).index_add_(0, assign, sample)
        counts = torch.bincount(assign, minlength=K).to(sums.dtype)
        empty = counts == 0
        centroids = sums / counts.clamp(min=1).unsqueeze(1)
        if bool(empty.any()):
            ne = int(empty.sum())
            centroids[empty] = sample[torch.randint(0, n, (ne,), generator=g, device=sample.device)]
    return torch.nn.functional.normalize(centroids, dim=-1)


def build_index(embeddings, doclens, nbits=2, num_partitions=None, kmeans_niters=4, sample_size=None, seed=123,
                heldout_fraction=0.05, chunk=1 << 20, config=None, backend=HipBackend) -> IndexArrays:
    """embeddings: float tensor [N, 128] on the GPU, doclens: int tensor [P] with sum N.  Returns host IndexArrays
    (call `.save(path)` for the reference's directory layout)."""
    _require_device(embeddings, backend, "embeddings")
    _require_unit_rows(embeddings, "build_index(embeddings)")
    dev = embeddings.device
    N, dim = embeddings.shape
    doclens = torch.as_tensor(doclens, device=dev).long()
    assert int(doclens.sum()) == N, "doclens must sum to the number of embeddings"
    K = num_partitions or num_partitions_for(N)
    K = min(K, N)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    # ---- sample + held-out split (collection_indexer.py:206-256) ----
    sample_size = min(N, sample_size or max(K * 40, 1 << 14))
    perm = torch.randperm(N, generator=g, device=dev)[:sample_size]
    sample = embeddings[perm].float()
    n_held = max(1, min(int(heldout_fraction * sample_size), 50_000))
    heldout, train = sample[:n_held], sample[n_held:] if sample_size - n_held >= K else sample
    centroids = kmeans(train, K, kmeans_niters, seed, backend=backend).half().float()
    # ---- bucket tables from held-out residuals (:286-308) ----
    held_codes = backend.nearest_centroids(heldout, centroids).long()
    held_res = heldout - centroids[held_codes]
    cutoffs, weights = synth.bucket_tables(held_res, nbits)
    avg_residual = float(held_res.abs().mean())
    # ---- compress every embedding (residual.py:169-204) ----
    codes = torch.empty(N, dtype=torch.int32, device=dev)
    residuals = torch.empty((N, dim * nbits // 8), dtype=torch.uint8, device=dev)
    for i in range(0, N, chunk):
        e = embeddings[i:i + chunk].float()
        c = backend.nearest_centroids(e, centroids)
        codes[i:i + chunk] = c
        residuals[i:i + chunk] = backend.compress_residuals(e, centroids, c, cutoffs, nbits)
    ivf, ivf_lengths = backend.build_ivf(codes, doclens, K)
    cpu = lambda t: t.detach().cpu().numpy()
    cfg = dict(config or {})
    cfg.setdefault("kmeans_niters", kmeans_niters)
    return IndexArrays(dim, nbits, cpu(codes), cpu(residuals), cpu(doclens), cpu(ivf), cpu(ivf_lengths), cpu(centroids),
                       cpu(weights), bucket_cutoffs=cpu(cutoffs), avg_residual=avg_residual, config=cfg)


def chunks_of_rank(num_chunks, rank, nranks):
    """The chunks rank `rank` of `nranks` encodes and writes: chunk i belongs to rank i % nranks (collection.py:64-81)."""
    return [i for i in range(num_chunks) if i % nranks == rank]


def _save_atomic(obj, path):
    tmp = path + ".tmp"
    if path.endswith(".json"):
        with open(tmp, "w") as f:
            json.dump(obj, f, indent=4)
    else:
        torch.save(obj, tmp)
    os.replace(tmp, path)


class ChunkedIndexBuilder:
    """Chunk-by-chunk index build into the reference's on-disk layout (collection_indexer.py:321-440, index_saver.py:30-90).

        b = ChunkedIndexBuilder(path, nbits=2, resume=False)
        b.plan(num_passages, avg_doclen_est)              # plan.json: num_partitions, num_chunks (chunksize passages each)
        b.fit(sample_embs)                                # k-means + bucket tables -> centroids.pt, buckets.pt, avg_residual.pt
        for i in chunks_of_rank(b.num_chunks, rank, nranks):
            b.add_chunk(i, i * b.chunksize, embs_i, doclens_i)   # -> {i}.codes.pt, {i}.residuals.pt, doclens.{i}.json, {i}.metadata.json
        (barrier: the caller owns the ranks)
        b.finalize()                                      # embedding offsets, IVF -> ivf.pid.pt, metadata.json

    Only one chunk of embeddings is held at a time; host chunks are moved to the device one at a time.  With `resume`, an
    existing plan / codec is loaded instead of recomputed and `add_chunk` returns False for a chunk whose code and residual
    files are already on disk.  `backend` as for `build_index` (tests of the host logic pass a torch one)."""

    def __init__(self, index_path, nbits, resume=False, backend=HipBackend, config=None):
        assert nbits in (1, 2, 4, 8), nbits
        self.index_path, self.nbits, self.resume, self.backend = index_path, int(nbits), bool(resume), backend
        self.config = dict(config or {})
        self.config.update({"dim": 128, "nbits": self.nbits})
        self.config.setdefault("kmeans_niters", 4)
        self.num_partitions = self.num_chunks = self.chunksize = None
        self.centroids = self.cutoffs = self.weights = self.avg_residual = None
        os.makedirs(index_path, exist_ok=True)

    def _path(self, name):
        return os.path.join(self.index_path, name)

    def _dev(self, x):
        return x.cuda() if self.backend is HipBackend and not x.is_cuda else x

    # ---- plan (collection_indexer.py:75-113) ----
    def plan(self, num_passages, avg_doclen_est, chunksize=25_000):
        if self.resume and self._try_load_plan():
            return False
        assert num_passages >= 1 and chunksize >= 1
        num_embeddings_est = num_passages * avg_doclen_est
        self.num_partitions = num_partitions_for(num_embeddings_est)
        self.num_chunks = int(math.ceil(num_passages / chunksize))
        self.chunksize = int(chunksize)
        self.config["chunksize"] = self.chunksize
        self._write_plan(num_embeddings_est, avg_doclen_est)
        return True

    def _write_plan(self, num_embeddings_est, avg_doclen_est):
        self._plan_est = (num_embeddings_est, avg_doclen_est)
        _save_atomic({"config": self.config, "num_chunks": self.num_chunks, "num_partitions": self.num_partitions,
                      "num_embeddings_est": num_embeddings_est, "avg_doclen_est": avg_doclen_est}, self._path("plan.json"))

    def _try_load_plan(self):
        if not os.path.exists(self._path("plan.json")):
            return False
        with open(self._path("plan.json")) as f:
            plan = json.load(f)
        self.config.update(plan.get("config", {}))
        self.num_chunks, self.num_partitions = int(plan["num_chunks"]), int(plan["num_partitions"])
        self.chunksize = self.config.get("chunksize")
        self._plan_est = (plan.get("num_embeddings_est"), plan.get("avg_doclen_est"))
        return True

    # ---- codec (collection_indexer.py:206-308) ----
    def fit(self, sample_embs, seed=123, heldout_fraction=0.05):
        """k-means on the sample (held-out split and `kmeans` as in build_index), bucket tables and avg_residual from the
        held-out residuals; writes centroids.pt / buckets.pt / avg_residual.pt.  Returns False when `resume` loaded them."""
        assert self.num_partitions is not None, "plan() first"
        if self.resume and self.try_load_codec():
            return False
        sample = self._dev(sample_embs)
        _require_device(sample, self.backend, "the k-means sample")
        _require_unit_rows(sample, "fit(sample_embs)")
        sample = sample.float()
        n = sample.size(0)
        K = min(self.num_partitions, n)   # (a sample smaller than the planned partition count: tiny collections)
        g = torch.Generator(device=sample.device)
        g.manual_seed(seed)
        n = min(n, max(K * 40, 1 << 14))   # build_index's sample size
        sample = sample[torch.randperm(sample.size(0), generator=g, device=sample.device)[:n]]
        n_held = max(1, min(int(heldout_fraction * n), 50_000))
        heldout, train = sample[:n_held], sample[n_held:] if n - n_held >= K else sample
        centroids = kmeans(train, K, int(self.config["kmeans_niters"]), seed, backend=self.backend).half().float()
        held_codes = self.backend.nearest_centroids(heldout, centroids).long()
        held_res = heldout - centroids[held_codes]
        cutoffs, weights = synth.bucket_tables(held_res, self.nbits)
        self.set_codec(centroids, cutoffs, weights, held_res.abs().mean())
        return True

    def set_codec(self, centroids, cutoffs, weights, avg_residual):
        """Use (and write) a given codec: centroids [K, 128] (stored as half), bucket cut-offs [2^nbits - 1] / weights [2^nbits]."""
        c = torch.as_tensor(centroids)
        self.centroids = self._dev(c.half().float())
        self.cutoffs = self._dev(torch.as_tensor(cutoffs).float())
        self.weights = torch.as_tensor(weights).float()
        self.avg_residual = torch.as_tensor(avg_residual).float().reshape(()).cpu()
        assert self.cutoffs.numel() == 2 ** self.nbits - 1 and self.weights.numel() == 2 ** self.nbits
        if self.num_partitions != c.size(0):   # the codec's centroid count is the index's partition count
            self.num_partitions = int(c.size(0))
            if self.num_chunks is not None:
                self._write_plan(*self._plan_est)
        _save_atomic(self.centroids.half().cpu(), self._path("centroids.pt"))
        _save_atomic((self.cutoffs.cpu(), self.weights.cpu()), self._path("buckets.pt"))
        _save_atomic(self.avg_residual, self._path("avg_residual.pt"))

    def try_load_codec(self):
        names = ("centroids.pt", "buckets.pt", "avg_residual.pt")
        if not all(os.path.exists(self._path(x)) for x in names):
            return False
        self.centroids = self._dev(torch.load(self._path("centroids.pt"), map_location="cpu").float())
        cutoffs, weights = torch.load(self._path("buckets.pt"), map_location="cpu")
        self.cutoffs, self.weights = self._dev(cutoffs.float()), weights.float()
        self.avg_residual = torch.load(self._path("avg_residual.pt"), map_location="cpu").float()
        if self.num_partitions is None:
            self.num_partitions = int(self.centroids.size(0))
        return True

    # ---- chunks (collection_indexer.py:321-339, index_saver.py:30-90) ----
    def chunk_exists(self, i):
        return all(os.path.exists(self._path(f"{i}.{x}.pt")) for x in ("codes", "residuals"))

    def add_chunk(self, i, passage_offset, embs, doclens):
        """Compress chunk i (passages passage_offset .. + len(doclens)) and write its four files.  Returns False without
        computing anything when `resume` finds the chunk's codes and residuals on disk."""
        if self.resume and self.chunk_exists(i):
            return False
        assert self.centroids is not None, "fit() / set_codec() first"
        doclens = [int(x) for x in torch.as_tensor(doclens).reshape(-1).tolist()]
        n = int(embs.size(0))
        if sum(doclens) != n:
            raise ValueError(f"chunk {i}: doclens sum to {sum(doclens)}, the chunk has {n} embeddings")
        e = self._dev(embs)
        _require_device(e, self.backend, f"chunk {i}")
        _require_unit_rows(e, f"add_chunk({i})")
        if e.dtype == torch.float16:
            codes, residuals = self.backend.compress_f16(e, self.centroids, self.cutoffs, self.nbits)
        else:
            e = e.float()
            codes = self.backend.nearest_centroids(e, self.centroids)
            residuals = self.backend.compress_residuals(e, self.centroids, codes, self.cutoffs, self.nbits)
        # the code file goes last: its presence (with the residuals) marks a complete chunk for `resume`
        _save_atomic(doclens, self._path(f"doclens.{i}.json"))
        _save_atomic({"passage_offset": int(passage_offset), "num_passages": len(doclens), "num_embeddings": n},
                     self._path(f"{i}.metadata.json"))
        _save_atomic(residuals.to(torch.uint8).cpu(), self._path(f"{i}.residuals.pt"))
        _save_atomic(codes.to(torch.int32).cpu(), self._path(f"{i}.codes.pt"))
        return True

    # ---- finalize (collection_indexer.py:341-440) ----
    def finalize(self):
        if self.num_chunks is None and not self._try_load_plan():
            raise FileNotFoundError(f"{self.index_path}: no plan.json (plan() first)")
        missing = [i for i in range(self.num_chunks) if not (self.chunk_exists(i) and
                   os.path.exists(self._path(f"doclens.{i}.json")) and os.path.exists(self._path(f"{i}.metadata.json")))]
        if missing:
            raise FileNotFoundError(f"{self.index_path}: chunks {missing} of {self.num_chunks} are missing")
        metas, doclens, codes = [], [], []
        passage_offset = embedding_offset = 0
        for i in range(self.num_chunks):
            with open(self._path(f"{i}.metadata.json")) as f:
                meta = json.load(f)
            if int(meta["passage_offset"]) != passage_offset:
                raise ValueError(f"chunk {i} starts at passage {meta['passage_offset']}, expected {passage_offset} "
                                 "(chunks must cover the passages contiguously)")
            with open(self._path(f"doclens.{i}.json")) as f:
                dl = json.load(f)
            c = torch.load(self._path(f"{i}.codes.pt"), map_location="cpu")
            if len(dl) != int(meta["num_passages"]) or c.numel() != int(meta["num_embeddings"]) or sum(dl) != c.numel():
                raise ValueError(f"chunk {i}: metadata, doclens and codes disagree")
            meta["embedding_offset"] = embedding_offset
            metas.append(meta)
            doclens.extend(dl)
            codes.append(self._dev(c.to(torch.int32)))
            passage_offset += len(dl)
            embedding_offset += c.numel()
        for i, meta in enumerate(metas):
            _save_atomic(meta, self._path(f"{i}.metadata.json"))
        all_codes = torch.cat(codes)   # on the device for the HIP backend
        del codes
        ivf, ivf_lengths = self.backend.build_ivf(all_codes, self._dev(torch.tensor(doclens, dtype=torch.int64)),
                                                  self.num_partitions)
        _save_atomic((ivf.to(torch.int32).cpu(), ivf_lengths.to(torch.int64).cpu()), self._path("ivf.pid.pt"))
        _save_atomic({"config": self.config, "num_chunks": self.num_chunks, "num_partitions": self.num_partitions,
                      "num_embeddings": embedding_offset, "avg_doclen": embedding_offset / max(1, passage_offset)},
                     self._path("metadata.json"))
        return self.index_path
