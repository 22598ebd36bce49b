"""`Indexer` -- the reference's index-build entry point (TPC/indexer.py:15-85) over this build's GPU index build
(`indexing.build_index`: k-means in torch, nearest-centroid argmax + residual bit-packing on the HIP kernels of
csrc/flmr_build.hip, IVF), writing the reference's on-disk format.

Kept from the reference: `Indexer(checkpoint, config)`, config merge order (checkpoint config < `config` < the active
`Run().config`, indexer.py:25-26), `configure`, `get_index`, `erase` (same file selection, indexer.py:35-56), and
`index(name, collection, overwrite)` with `overwrite in {True, False, 'reuse', 'resume'}` and the same assertions /
path resolution (`config.index_path_` = {root}/{experiment}/indexes/{name}).

What differs: passage ENCODING (the BERT / ViT forward of `CollectionEncoder`, collection_indexer.py:318-340) is outside
this build's scope, so the embeddings come from `doc_encoder(list_of_passages) -> (embeddings [N, 128], doclens [P])` given
at construction, or `collection` may already be an `(embeddings, doclens)` pair.  There is no multi-process launcher: one
process builds the index on its GPU (the reference spawns `nranks` encoder processes, indexer.py:78-84).

Two build forms.  By default (`chunksize=None`) the whole collection is encoded in one call and built in one piece
(`build_index`, a single chunk); there 'resume' has nothing to resume from and behaves like `True`.  With
`Indexer(..., chunksize=C)` and a `doc_encoder`, `index()` follows the reference's order (collection_indexer.py:56-73, 321-339)
on `indexing.ChunkedIndexBuilder`: sample passages (`_sample_pids`), encode the sample and fit the codec, encode and write C
passages at a time, finalize.  Only one chunk of embeddings exists at a time, and 'resume' really resumes: the plan and codec
on disk are reused and chunks already written are neither encoded nor compressed again.  When `ravqa_amd.install()` is
active the reference's own `colbert.Indexer` is left in place -- this class is for running without the reference package.
"""
import math
import os
import random
import time

import torch

from . import config as _config
from .indexing import ChunkedIndexBuilder, build_index


class Indexer:
    ColBERTConfig = _config.ColBERTConfig
    Run = _config.Run

    def __init__(self, checkpoint=None, config=None, doc_encoder=None, build_backend=None, chunksize=None):
        self.index_path = None
        self.chunksize = chunksize           # None: one-piece build; an int: chunked build (ChunkedIndexBuilder)
        self.build_backend = build_backend   # None: the HIP kernels (indexing.HipBackend); tests of the host logic inject a torch one
        self.checkpoint = checkpoint
        self.checkpoint_config = self.ColBERTConfig.load_from_checkpoint(checkpoint) if isinstance(checkpoint, str) else None
        self.config = self.ColBERTConfig.from_existing(self.checkpoint_config, config, self.Run().config)
        self.configure(checkpoint=checkpoint)
        self.doc_encoder = doc_encoder

    def configure(self, **kw_args):
        self.config.configure(**kw_args)

    def get_index(self):
        return self.index_path

    def erase(self, wait_seconds=0):
        assert self.index_path is not None
        directory, deleted = self.index_path, []
        for filename in sorted(os.listdir(directory)):
            path = os.path.join(directory, filename)
            delete = path.endswith(".json") and ("metadata" in path or "doclen" in path or "plan" in path)
            if delete or path.endswith(".pt"):
                deleted.append(path)
        if deleted:
            if wait_seconds:
                time.sleep(wait_seconds)   # the reference waits 3 s before deleting (indexer.py:50-51)
            for path in deleted:
                os.remove(path)
        return deleted

    def _embeddings_of(self, collection):
        if isinstance(collection, (tuple, list)) and len(collection) == 2 and torch.is_tensor(collection[0]):
            return collection
        if self.doc_encoder is None:
            raise NotImplementedError("passage encoding (CollectionEncoder.encode_passages) is outside the retrieval hot path: "
                                      "construct Indexer(..., doc_encoder=fn) or pass collection=(embeddings, doclens)")
        passages = list(collection.data) if hasattr(collection, "data") else list(collection)
        return self.doc_encoder(passages)

    @staticmethod
    def _sample_pids(num_passages, seed=12345):
        """The passages whose embeddings train the codec (collection_indexer.py:115-130): 16 sqrt(120 P) of them, at most P."""
        n = min(1 + int(16 * math.sqrt(120 * num_passages)), num_passages)
        return sorted(random.Random(seed).sample(range(num_passages), n))

    def _chunked(self, collection):
        return self.chunksize is not None and self.doc_encoder is not None and not (
            isinstance(collection, (tuple, list)) and len(collection) == 2 and torch.is_tensor(collection[0]))

    def _cfg(self, name):
        return {"query_maxlen": self.config.query_maxlen, "doc_maxlen": self.config.doc_maxlen,
                "checkpoint": self.checkpoint if isinstance(self.checkpoint, str) else None, "index_name": name}

    def _index_chunked(self, name, collection, resume):
        passages = list(collection.data) if hasattr(collection, "data") else list(collection)
        kw = {} if self.build_backend is None else {"backend": self.build_backend}
        cfg = self._cfg(name)
        cfg["kmeans_niters"] = self.config.kmeans_niters
        b = ChunkedIndexBuilder(self.index_path, self.config.nbits, resume=resume, config=cfg, **kw)
        have = resume and b._try_load_plan() and b.try_load_codec()
        if not have:
            pids = self._sample_pids(len(passages))
            sample, sample_doclens = self.doc_encoder([passages[p] for p in pids])
            b.plan(len(passages), float(torch.as_tensor(sample_doclens).sum()) / len(pids), self.chunksize)
            b.fit(sample)
        for i in range(b.num_chunks):
            if resume and b.chunk_exists(i):
                continue   # not even encoded (collection_indexer.py:325-327)
            lo = i * b.chunksize
            embs, doclens = self.doc_encoder(passages[lo:lo + b.chunksize])
            b.add_chunk(i, lo, embs, doclens)
        b.finalize()

    def index(self, name, collection, overwrite=False):
        assert overwrite in [True, False, "reuse", "resume"]
        self.configure(index_name=name, resume=overwrite == "resume")
        self.index_path = self.config.index_path_
        index_does_not_exist = not os.path.exists(self.index_path)
        assert (overwrite in [True, "reuse", "resume"]) or index_does_not_exist, self.index_path
        os.makedirs(self.index_path, exist_ok=True)
        if self._chunked(collection) and (index_does_not_exist or overwrite != "reuse"):
            if overwrite is True:
                self.erase()
            self._index_chunked(name, collection, resume=overwrite == "resume")
            return self.index_path
        if overwrite is True or overwrite == "resume":
            self.erase()
        if index_does_not_exist or overwrite != "reuse":
            embeddings, doclens = self._embeddings_of(collection)
            if self.build_backend is None and not embeddings.is_cuda:
                embeddings = embeddings.cuda()   # the build runs on the MI355X (no host path: fails loudly without a device)
            cfg = self._cfg(name)
            kw = {} if self.build_backend is None else {"backend": self.build_backend}
            arrays = build_index(embeddings, torch.as_tensor(doclens), nbits=self.config.nbits,
                                 kmeans_niters=self.config.kmeans_niters, config=cfg, **kw)
            arrays.save(self.index_path)
        return self.index_path
