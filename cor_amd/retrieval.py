"""Retrieval end of the path: region embeddings, gallery similarity + top-k, gallery sharding across ranks.

The reference has no gallery / top-k code; the definitions come from its only region-vs-query
similarity, the training loss: region embedding = utils/loss_func.py:35-56 (mask_pooling), query = comb_support_feat
(lib/support_branch.py:85), score = F.cosine_similarity (utils/loss_func.py:84) = dot product of unit vectors.
Order: score descending, then global gallery index ascending.

Multi-GPU (one process per GPU, torch.distributed; backend "nccl" is RCCL over xGMI on ROCm, "gloo" in CPU tests):
the gallery is row-sharded, rank r owning rows [r*ceil(G/R), ...). One exchange step on the data path: an
all-gather of the [B_local, 256] query embeddings (<= 64 KB per rank: latency-bound). Each rank then scores
ALL queries against its shard with the HIP kernel (cor_similarity_topk), and the packed per-shard (score, global index)
lists go to one rank in ONE gather and are merged once on the host by (score desc, index asc).
"""
from __future__ import annotations

import contextlib
import math

import torch

from . import ops


def region_embedding(embeddings: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """ref: utils/loss_func.py:35-56. embeddings f32[B,C,H,W] (query_image_embeddings), mask f32[B,1,h,w] in [0,1]
    -> f32[B,1,C] unit-norm. HIP: cor_bilinear (clamped) + cor_masked_pool (NCHW, L2-normalised)."""
    B, C, H, W = embeddings.shape
    emb = embeddings.to(torch.float32).contiguous()
    m = mask.to(torch.float32).contiguous()
    if tuple(m.shape[-2:]) != (H, W):
        m = ops.bilinear(m, H, W)
    return ops.masked_pool(emb, m, B, H * W, C, feat_nchw=True, clamp01=True, l2norm=True).view(B, 1, C)


def merge_topk_host(scores_parts, idx_parts, k: int):
    """Host merge of per-shard lists by (score desc, index asc). parts: lists of CPU tensors [Bq, k_i]."""
    s = torch.cat(scores_parts, dim=1)
    i = torch.cat(idx_parts, dim=1)
    i_key = torch.where(i < 0, torch.full_like(i, torch.iinfo(torch.int64).max), i)   # missing entries last
    o1 = torch.sort(i_key, dim=1, stable=True).indices
    s, i = torch.gather(s, 1, o1), torch.gather(i, 1, o1)
    o2 = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, o2), torch.gather(i, 1, o2)


def merge_topk_distinct_host(scores_parts, idx_parts, group_parts, k: int):
    """Host merge of per-shard DISTINCT-group lists: the concatenated entries are ranked by (score desc, index asc), reduced to the
    best entry per non-negative group id (negative ids and nothing else are never merged; missing entries are dropped) and cut to
    k; fewer than k groups: the (-inf, -1) tail. parts: lists of CPU tensors [Bq, k_i]; group_parts int32/int64, one id per entry.
    Exact across shards: a global top-k representative r is its group's best row in its own shard, and fewer than k groups beat
    it anywhere, so fewer than k beat it there: r is in that shard's list. Every other listed row of r's group ranks behind r,
    and a group outside the global top-k only lists rows behind its own representative, hence behind the k-th."""
    s = torch.cat(scores_parts, dim=1)
    i = torch.cat(idx_parts, dim=1)
    g = torch.cat([torch.as_tensor(x).to(torch.int64) for x in group_parts], dim=1)
    B, N = s.shape
    i_key = torch.where(i < 0, torch.full_like(i, torch.iinfo(torch.int64).max), i)   # missing entries last
    o1 = torch.sort(i_key, dim=1, stable=True).indices
    s, i, g = torch.gather(s, 1, o1), torch.gather(i, 1, o1), torch.gather(g, 1, o1)
    o2 = torch.sort(s, dim=1, descending=True, stable=True).indices
    s, i, g = torch.gather(s, 1, o2), torch.gather(i, 1, o2), torch.gather(g, 1, o2)   # rank order
    g_key = torch.where(g >= 0, g, -1 - torch.arange(N, dtype=torch.int64).expand(B, N))   # a negative id: a group of its own
    o3 = torch.sort(g_key, dim=1, stable=True).indices                               # groups together, rank order inside
    gs = torch.gather(g_key, 1, o3)
    head = torch.ones((B, N), dtype=torch.bool)
    head[:, 1:] = gs[:, 1:] != gs[:, :-1]
    keep = torch.zeros((B, N), dtype=torch.bool).scatter_(1, o3, head) & (i >= 0)
    o4 = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :k]        # the kept entries first, in rank order
    out_s, out_i = torch.gather(s, 1, o4), torch.gather(i, 1, o4)
    if out_s.shape[1] < k:
        out_s = torch.cat([out_s, torch.full((B, k - out_s.shape[1]), float("-inf"))], dim=1)
        out_i = torch.cat([out_i, torch.full((B, k - out_i.shape[1]), -1, dtype=torch.int64)], dim=1)
    tail = torch.arange(k).expand(B, k) >= keep.sum(1, keepdim=True)
    return out_s.masked_fill(tail, float("-inf")), out_i.masked_fill(tail, -1)


def _on(dev):
    """The context that makes `dev` the current GPU; nothing for a CPU device (whose tensors the ops' own checks refuse)."""
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def _missing_lists(B, k, dev):
    """The all-missing lists of B queries: (scores f32[B,k] = -inf, idx i64[B,k] = -1)."""
    return torch.full((B, k), float("-inf"), device=dev), torch.full((B, k), -1, dtype=torch.int64, device=dev)


def _row_ids(ids, what, n, dev):
    """labels / group ids of a shard of n rows -> int32[n] on `dev`"""
    ids = torch.as_tensor(ids)
    if ids.dim() != 1 or ids.shape[0] != n:
        raise ValueError(f"GalleryShard: {tuple(ids.shape)} {what} for {n} rows")
    return ids.to(dev, torch.int32).contiguous()


def _merge_stacked(s, i, g, k: int):
    """Rounds of ops.merge_topk over stacked lists s, i[, g] of shape [P, B, kin] on one GPU -> (scores, idx, groups or None), [B, k]."""
    while s.shape[0] * s.shape[2] > ops.nat.MERGE_NMAX:
        per = max(1, ops.nat.MERGE_NMAX // s.shape[2])          # lists per launch; the outputs are lists of k <= 256, so a round shrinks
        outs = [ops.merge_topk(s[j:j + per], i[j:j + per], k, None if g is None else g[j:j + per]) for j in range(0, s.shape[0], per)]
        s, i = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
        g = None if g is None else torch.stack([o[2] for o in outs])
    out = ops.merge_topk(s, i, k, g)
    return (out[0], out[1], None) if g is None else out


def merge_topk_device(scores_parts, idx_parts, k: int, group_parts=None):
    """merge_topk_host / merge_topk_distinct_host on the GPU (ops.merge_topk, cor_merge_topk): parts are lists of device tensors
    [B, k_i] as the searches return them (missing entries (-inf, -1)); the result is bitwise what the host functions give on CPU
    copies of the same lists and stays on the device: (scores f32[B,k], idx i64[B,k]), with group_parts (int32 / int64 ids, one per
    entry: the distinct merge) a third tensor, the surviving entries' group ids i32[B,k] (-1 in the tail).
    Lists of unequal k_i are padded to the longest with missing entries; a list longer than one launch ranks (4096 entries) is cut
    into several. When all lists together exceed 4096 entries per query they are merged in ROUNDS: as many lists as fit go to one
    list of k, and those lists are merged again, the group ids travelling between rounds in the kernel's out_groups. The rounds are
    exact for both modes: a merged list is the (distinct) top-k of the union of its inputs, so it stands in for a shard in the proof
    in merge_topk_distinct_host's docstring (plain: the top-k of a union lies in the union of the parts' top-k)."""
    if len(scores_parts) == 0 or len(scores_parts) != len(idx_parts) or (group_parts is not None and len(group_parts) != len(idx_parts)):
        raise ValueError("merge_topk_device: need one or more lists, and as many index (and group) lists as score lists")
    nmax = ops.nat.MERGE_NMAX
    ss = [x for t in scores_parts for x in t.split(nmax, dim=1)]
    ii = [x for t in idx_parts for x in t.split(nmax, dim=1)]
    gg = None if group_parts is None else [x for t in group_parts for x in t.to(torch.int32).split(nmax, dim=1)]
    kin = max(t.shape[1] for t in ss)

    def stacked(parts, fill, dtype):
        out = torch.full((len(parts), parts[0].shape[0], kin), fill, dtype=dtype, device=parts[0].device)
        for p, t in enumerate(parts):
            out[p, :, :t.shape[1]] = t
        return out

    if all(t.shape[1] == kin for t in ss):
        s, i, g = torch.stack(ss), torch.stack(ii), None if gg is None else torch.stack(gg)
    else:
        s, i = stacked(ss, float("-inf"), torch.float32), stacked(ii, -1, torch.int64)
        g = None if gg is None else stacked(gg, -1, torch.int32)
    out_s, out_i, out_g = _merge_stacked(s, i, g, k)
    return (out_s, out_i) if group_parts is None else (out_s, out_i, out_g)


def fuse_lists_device(scores_parts, idx_parts, k: int, **fuse_kwargs):
    """Fusion of P ranked lists per query on the GPU (ops.fuse_lists, cor_fuse_lists): parts are lists of device tensors [Bq, k_i] as the
    stages return them, P rankings of the SAME Bq requests over the SAME global ids (several shots or views of a request, several
    galleries over one id space) -> (scores f32[Bq,k], idx i64[Bq,k][, count i32[Bq,k] with return_count=True]): one entry per distinct id,
    ranked by (fused score desc, id asc), on the device. fuse_kwargs: weights, mode ("rrf" / "sum" / "max"), rrf_c, normalize, missing,
    return_count, as ops.fuse_lists takes them. Lists of unequal k_i are padded to the longest with missing entries (-inf, -1), which are
    holes: they change no rank and no statistic. At most 16 lists and 4096 entries per query (P times the longest list), else ValueError:
    there are no rounds as in merge_topk_device, because a fused list is not a list that can be fused again exactly (its ranks and
    per-list statistics are those of the inputs). merge_topk_device is not this: it ranks entries and keeps a row that two lists name
    twice. Nothing leaves the device and the host is not waited for."""
    if len(scores_parts) == 0 or len(scores_parts) != len(idx_parts):
        raise ValueError("fuse_lists_device: need one or more lists, and as many index lists as score lists")
    P = len(scores_parts)
    if P > ops.nat.FUSE_PMAX:
        raise ValueError(f"fuse_lists_device: {P} lists, one fusion takes at most {ops.nat.FUSE_PMAX}")
    for s, i in zip(scores_parts, idx_parts):
        if s.dim() != 2 or s.shape[1] < 1 or i.shape != s.shape or s.shape[0] != scores_parts[0].shape[0]:
            raise ValueError(f"fuse_lists_device: every list is scores and idx [Bq, k_i >= 1] of one Bq, got {tuple(s.shape)} and {tuple(i.shape)}")
        if s.dtype != torch.float32 or i.dtype != torch.int64:
            raise ValueError(f"fuse_lists_device: scores must be float32 and idx int64, got {s.dtype} and {i.dtype}")
    kin = max(s.shape[1] for s in scores_parts)
    if P * kin > ops.nat.MERGE_NMAX:
        raise ValueError(f"fuse_lists_device: {P} lists padded to {kin} are {P * kin} entries per query, one fusion takes at most "
                         f"{ops.nat.MERGE_NMAX} (there are no rounds: a fused list cannot be fused again exactly)")
    ops.fuse_args("fuse_lists_device", P, k, **{a: v for a, v in fuse_kwargs.items() if a != "return_count"})
    dev = scores_parts[0].device
    with _on(dev):
        if all(s.shape[1] == kin for s in scores_parts):
            s, i = torch.stack(list(scores_parts)), torch.stack(list(idx_parts))
        else:
            s = torch.full((P, scores_parts[0].shape[0], kin), float("-inf"), dtype=torch.float32, device=dev)
            i = torch.full((P, scores_parts[0].shape[0], kin), -1, dtype=torch.int64, device=dev)
            for p, (sp, ip) in enumerate(zip(scores_parts, idx_parts)):
                s[p, :, :sp.shape[1]] = sp
                i[p, :, :ip.shape[1]] = ip
        return ops.fuse_lists(s, i, int(k), **fuse_kwargs)


def groups_of(idx, groups):
    """Global row ids -> group ids: idx i64[B,k] (as the searches return them; -1 = missing, stays -1), groups: one id per gallery
    row (the whole gallery, e.g. dataloader.gallery_labels(csv, column="Query_img")). Image-level Recall@K is then
    recall_at_k(groups_of(idx, groups), positive_image_ids)."""
    idx = torch.as_tensor(idx).cpu().long()
    groups = torch.as_tensor(groups).reshape(-1).cpu().long()
    return torch.where(idx >= 0, groups[idx.clamp(min=0)], torch.full_like(idx, -1))


def recall_at_k(idx, positives, ks=(1, 5, 10, 50, 100)) -> dict:
    """Recall@K of ranked lists: the fraction of queries with a positive among their first K entries.
    idx: i64[B, k] global gallery ids (as distributed_search / GalleryShard.search return them; -1 = missing).
    positives: one global id per query (a sequence or an i64[B] tensor) or, per query, a collection of ids.
    Returns {K: fraction} for every K in ks; raises ValueError if max(ks) > k."""
    idx = torch.as_tensor(idx).cpu().long()
    if idx.dim() != 2:
        raise ValueError(f"recall_at_k: idx must be [B, k], got {tuple(idx.shape)}")
    B, k = idx.shape
    ks = tuple(int(K) for K in ks)
    if not ks or min(ks) < 1 or max(ks) > k:
        raise ValueError(f"recall_at_k: every K must be in [1, {k}] (the lists hold {k} entries), got {ks}")
    if isinstance(positives, torch.Tensor) and positives.dim() == 1:
        positives = positives.tolist()
    if len(positives) != B:
        raise ValueError(f"recall_at_k: {len(positives)} positives for {B} queries")
    sets = [{int(p)} if isinstance(p, int) or (isinstance(p, torch.Tensor) and p.dim() == 0) else {int(x) for x in p} for p in positives]
    hit = torch.zeros((B, k), dtype=torch.bool)
    for b, pos in enumerate(sets):
        if pos:
            hit[b] = torch.isin(idx[b], torch.tensor(sorted(pos), dtype=torch.int64)) & (idx[b] >= 0)
    first = torch.where(hit.any(1), hit.float().argmax(1), torch.full((B,), k))    # rank of the first positive (k: none)
    return {K: int((first < K).sum()) / B if B else 0.0 for K in ks}


class NeighbourGraph:
    """The k-reciprocal neighbour graph of a gallery (GalleryShard.neighbour_graph / GallerySet.neighbour_graph), on the gallery's
    device. Per non-empty segment it was built from: rnbr i64[n, width], row g's k1 nearest rows as global ids, pruned to the reciprocal
    ones (-1 where the neighbour does not list g back, lies in no segment, or does not exist), and kth f32[n], the score of row g's
    k1-th neighbour (-inf when fewer than k1 rows exist). `offsets` / `lengths` name those segments: a graph is valid only for them;
    GallerySet.add / drop do not update it, and rerank raises ValueError for a gallery whose live segments differ."""

    def __init__(self, width: int, offsets, lengths, rnbr, kth):
        self.width = int(width)
        self.offsets, self.lengths = tuple(int(o) for o in offsets), tuple(int(n) for n in lengths)
        self.rnbr, self.kth = list(rnbr), list(kth)

    @property
    def segments(self):
        """[(rnbr, kth, offset)] as ops.rerank_reciprocal takes it."""
        return list(zip(self.rnbr, self.kth, self.offsets))

    def check(self, who, live):
        """ValueError unless `live` (the gallery's non-empty segments) are the segments this graph was built from."""
        spans = (tuple(int(sh.offset) for sh in live), tuple(len(sh) for sh in live))
        if spans != (self.offsets, self.lengths):
            raise ValueError(f"{who}: the graph was built from segments at offsets {self.offsets} of lengths {self.lengths}, the gallery "
                             f"now has {spans[0]} of lengths {spans[1]}: build a new graph (neighbour_graph)")


def _check_graph_args(who, k1, batch):
    if not 1 <= int(k1) <= ops.nat.TOPK_KMAX or int(batch) < 1:
        raise ValueError(f"{who}: k1 must be in [1, {ops.nat.TOPK_KMAX}] and batch at least 1, got k1={k1}, batch={batch}")


def _rows_as_queries(shard, lo, hi):
    """Rows [lo, hi) of `shard` as search queries: a GalleryShard's stored rows; a QuantizedShard's dequantised fp32 rows (an int8 search
    quantises them again: that is the definition of an int8 gallery's own neighbours)."""
    if isinstance(shard, QuantizedShard):
        with _on(shard.rows.device):
            return ops.dequantize_rows_i8(shard.rows[lo:hi], shard.scales[lo:hi])
    return shard.rows[lo:hi]


def _knn_lists(shard, k1, batch, nb):
    """(nbr i64[n,k1], kth f32[n]) of `shard`'s rows searched, unfiltered, in `nb`, `batch` rows at a time."""
    n, dev = len(shard), shard.rows.device
    nbr = torch.empty((n, k1), dtype=torch.int64, device=dev)
    kth = torch.empty((n,), dtype=torch.float32, device=dev)
    for lo in range(0, n, int(batch)):
        s, i = nb.search(_rows_as_queries(shard, lo, lo + int(batch)), k1)
        nbr[lo:lo + int(batch)] = i
        kth[lo:lo + int(batch)] = s[:, k1 - 1]
    return nbr, kth


def _pruned_graph(live, k1, lists):
    """NeighbourGraph of the non-empty segments `live` from their (nbr, kth) lists: one ops.knn_reciprocal launch per segment."""
    table = [(nbr, int(sh.offset)) for sh, (nbr, _) in zip(live, lists)]
    rnbr = []
    for n, sh in enumerate(live):
        with _on(sh.rows.device):
            rnbr.append(ops.knn_reciprocal(table, n))
    return NeighbourGraph(k1, [sh.offset for sh in live], [len(sh) for sh in live], rnbr, [kth for _, kth in lists])


def _rerank(who, live, scores, idx, graph, k1, lam, k):
    graph.check(who, live)
    if idx.dim() != 2:
        raise ValueError(f"{who}: idx must be [Bq, kin], got {tuple(idx.shape)}")
    k1 = graph.width if k1 is None else k1
    k = min(idx.shape[1], ops.nat.TOPK_KMAX) if k is None else k
    with _on(live[0].rows.device if live else scores.device):
        return ops.rerank_reciprocal(scores, idx, graph.segments, k1, lam, k)


def _diversify(who, table, dev, scores, idx, k, lam, max_sim, return_pos):
    if idx.dim() != 2:
        raise ValueError(f"{who}: idx must be [Bq, kin], got {tuple(idx.shape)}")
    k = min(idx.shape[1], ops.nat.TOPK_KMAX) if k is None else k
    with _on(dev):
        return ops.diversify_mmr(table, scores, idx, k, lam=lam, max_sim=max_sim, return_pos=return_pos)


def _diffuse(who, table, dev, scores, idx, k, kd, kq, gamma, alpha, iters, return_pos):
    if idx.dim() != 2:
        raise ValueError(f"{who}: idx must be [Bq, kin], got {tuple(idx.shape)}")
    k = min(idx.shape[1], ops.nat.TOPK_KMAX) if k is None else k
    with _on(dev):
        return ops.rerank_diffusion(table, scores, idx, k, kd=kd, kq=kq, gamma=gamma, alpha=alpha, iters=iters, return_pos=return_pos)


class Clustering:
    """What .cluster of a GalleryShard, a QuantizedGallery or a GallerySet returns. centroids: a GalleryShard of K unit fp32 rows, offset 0
    (its row index is the cluster id). assign: int32 on the device, the cluster of every row, one tensor per segment for a GallerySet (in
    the order of its non-empty segments) and ONE tensor for a shard: usable as `groups=` / `labels=` of a shard over the same rows as it
    is. counts: int32 [K] on the device. objective: a Python list, per assignment pass the mean over the rows of their score to their
    centre. iters: the passes made. converged: the last pass changed no row."""

    def __init__(self, centroids, assign, counts, objective, iters, converged):
        self.centroids, self.assign, self.counts = centroids, assign, counts
        self.objective, self.iters, self.converged = objective, iters, converged

    def assign_queries(self, queries: torch.Tensor):
        """queries f32[Bq,C] -> (scores f32[Bq,1], cluster ids i64[Bq,1]): the nearest centre of each query (centroids.search(q, 1))."""
        return self.centroids.search(queries, 1)


def _cluster(who, live, single, n_clusters, iters, init, first_id, batch):
    """Spherical k-means over the non-empty segments `live`. The assignment is the chain-exact search of the rows in the centres, the
    centre step is ops.kmeans_update: the whole loop is defined to the bit. One host synchronisation per pass."""
    n = sum(len(sh) for sh in live)
    K = int(n_clusters)
    if n == 0:
        raise ValueError(f"{who}: nothing to cluster (no rows)")
    if not 1 <= K <= min(n, ops.nat.KMEANS_KMAX):
        raise ValueError(f"{who}: n_clusters must be in [1, min({n} rows, {ops.nat.KMEANS_KMAX})], got {n_clusters}")
    if int(iters) < 1 or int(batch) < 1:
        raise ValueError(f"{who}: iters and batch must be at least 1, got iters={iters}, batch={batch}")
    if len(live) > ops.nat.CLUSTER_SEGMAX:
        raise ValueError(f"{who}: {len(live)} non-empty segments, one clustering spans at most {ops.nat.CLUSTER_SEGMAX}")
    C = live[0].rows.shape[1]
    if isinstance(init, torch.Tensor):
        if init.dtype != torch.float32 or tuple(init.shape) != (K, C):
            raise ValueError(f"{who}: init must be float32 [{K}, {C}], got {init.dtype} {tuple(init.shape)}")
    elif init != "maxmin":
        raise ValueError(f"{who}: init must be 'maxmin' or a float32 tensor [K, C], got {init!r}")
    dev = live[0].rows.device
    table = [(sh.rows, sh.scales, sh.offset) if isinstance(sh, QuantizedShard) else (sh.rows, sh.offset) for sh in live]
    with _on(dev):
        cent = init.to(dev).contiguous().clone() if isinstance(init, torch.Tensor) else ops.kmeans_seed(table, K, first_id)[1]
        assign = [torch.full((len(sh),), -1, dtype=torch.int32, device=dev) for sh in live]
        objective, converged, passes, counts = [], False, 0, None
        while passes < int(iters) and not converged:
            centres = GalleryShard(cent, offset=0)
            new, score = [], []
            for sh in live:
                a = torch.empty((len(sh),), dtype=torch.int32, device=dev)
                s = torch.empty((len(sh),), dtype=torch.float32, device=dev)
                for lo in range(0, len(sh), int(batch)):
                    bs, bi = centres.search(_rows_as_queries(sh, lo, lo + int(batch)), 1)
                    a[lo:lo + int(batch)] = bi[:, 0]
                    s[lo:lo + int(batch)] = bs[:, 0]
                new.append(a)
                score.append(s)
            changed = sum((a != b).sum() for a, b in zip(new, assign))
            cent, counts, sums = ops.kmeans_update(table, new, K, scores=score, prev=cent)
            host = torch.cat([sums.double(), changed.double().reshape(1)]).cpu().tolist()    # the pass's one synchronisation
            objective.append(math.fsum(host[:K]) / n)
            converged = host[K] == 0
            assign = new
            passes += 1
    return Clustering(GalleryShard(cent, offset=0), assign[0] if single else assign, counts, objective, passes, converged)


def _search(shard, who, fns, row_args, queries, k, query_labels, mode, distinct):
    """The search of GalleryShard and QuantizedShard: fns = the (plain, filtered, distinct) ops, row_args = (rows,) or (rows, scales).
    Both argument checks come before anything touches the device."""
    if distinct and shard.groups is None:
        raise ValueError(f"{who}: distinct=True but the shard has no group ids")
    if query_labels is not None and shard.labels is None:
        raise ValueError(f"{who}: query_labels given but the shard has no row labels")
    q = queries.reshape(-1, queries.shape[-1]).to(shard.rows.device, torch.float32).contiguous()
    if query_labels is not None:
        query_labels = torch.as_tensor(query_labels).reshape(-1).to(q.device)
    if shard.rows.shape[0] == 0:                     # an empty shard (more ranks than gallery rows): all-missing lists, like Ng < k
        return _missing_lists(q.shape[0], k, q.device)
    plain, filtered, distinct_fn = fns
    with _on(shard.rows.device):
        if distinct:
            return distinct_fn(q, *row_args, k, shard.groups, None if query_labels is None else shard.labels, query_labels, mode=mode,
                               g_offset=shard.offset)
        if query_labels is None:
            return plain(q, *row_args, k, g_offset=shard.offset)
        return filtered(q, *row_args, k, shard.labels, query_labels, mode=mode, g_offset=shard.offset)


class GalleryShard:
    """Rows [offset, offset + n) of a unit-norm gallery, resident in HBM as fp32 / bf16 / fp16. labels: optional int32[n], one label
    per row (a class, a dataset or a source image id: dataloader.gallery_labels), for filtered searches. groups: optional int32[n],
    one group id per row (typically the source image id; negative: a group of its own), for distinct searches."""

    def __init__(self, rows: torch.Tensor, offset: int = 0, dtype: torch.dtype | None = None, labels=None, groups=None):
        if not rows.is_cuda:
            raise RuntimeError("GalleryShard lives in GPU memory (no CPU path)")
        self.rows = rows.to(dtype or rows.dtype).contiguous()
        self.offset = int(offset)
        n, dev = self.rows.shape[0], self.rows.device
        self.labels = None if labels is None else _row_ids(labels, "labels", n, dev)
        self.groups = None if groups is None else _row_ids(groups, "group ids", n, dev)

    def __len__(self):
        return self.rows.shape[0]

    def search(self, queries: torch.Tensor, k: int, query_labels=None, mode: str = "eq", distinct: bool = False):
        """queries f32[Bq,C] (unit-norm) -> (scores f32[Bq,k], global idx i64[Bq,k]) on the GPU; 1 <= k <= 256.
        query_labels (int32[Bq], < 0 = unrestricted): only the rows allowed by the shard's labels and `mode` ("eq": same label, "ne":
        another label) are ranked (ops.similarity_topk_filtered); None: the whole shard.
        distinct: one row per group id of the shard's `groups`, the k best groups (ops.similarity_topk_distinct), with or without the
        filter; idx still names the winning ROW of each group."""
        return _search(self, "GalleryShard.search", (ops.similarity_topk, ops.similarity_topk_filtered, ops.similarity_topk_distinct), (self.rows,),
                       queries, k, query_labels, mode, distinct)

    def range_search(self, queries: torch.Tensor, min_score, k: int, query_labels=None, mode: str = "eq"):
        """Threshold search (ops.similarity_range): queries f32[Bq,C] -> (scores f32[Bq,k], global idx i64[Bq,k], count i32[Bq]) on the
        GPU. count[b] is the exact number of rows of this shard whose chain score is at least min_score (a float, or an f32 tensor [Bq]
        of per-query floors), whatever the shard's size; the lists hold the first k of them by (score desc, index asc), then the
        (-inf, -1) tail. Open-set retrieval accepts a query when count > 0; ingest-time de-duplication asks with the new rows as
        queries and a floor near 1. An empty shard: all-missing lists and zero counts.
        query_labels (int32[Bq], < 0 = unrestricted) and mode as in search: only the rows the shard's labels allow are counted and
        listed (ops.similarity_range_filtered), e.g. mode "ne" with the query's own image id; None: the whole shard."""
        if query_labels is not None and self.labels is None:
            raise ValueError("GalleryShard.range_search: query_labels given but the shard has no row labels")
        q = queries.reshape(-1, queries.shape[-1]).to(self.rows.device, torch.float32).contiguous()
        if self.rows.shape[0] == 0:
            if not 1 <= int(k) <= ops.nat.TOPK_KMAX:
                raise ValueError(f"GalleryShard.range_search: k must be in [1, {ops.nat.TOPK_KMAX}], got {k}")
            return (*_missing_lists(q.shape[0], k, q.device), torch.zeros((q.shape[0],), dtype=torch.int32, device=q.device))
        if isinstance(min_score, torch.Tensor):
            min_score = min_score.reshape(-1).to(q.device)
        with _on(self.rows.device):
            if query_labels is None:
                return ops.similarity_range(q, self.rows, min_score, k, g_offset=self.offset)
            query_labels = torch.as_tensor(query_labels).reshape(-1).to(q.device)
            return ops.similarity_range_filtered(q, self.rows, min_score, k, self.labels, query_labels, mode=mode, g_offset=self.offset)

    def rescore(self, queries: torch.Tensor, cand: torch.Tensor, k: int | None = None, return_pos: bool = False):
        """The second stage of a two-stage search: queries f32[Bq,C], cand i64[Bq,kin] global row ids (a coarse search's idx, a union
        of lists, the ids of known rows; at most 4096 per query) -> (scores f32[Bq,k], idx i64[Bq,k][, pos i32[Bq,k]]) on the GPU: the
        chain scores of the candidates this shard holds, ranked by (score desc, id asc), every id once (ops.rescore_topk). Ids outside
        [offset, offset + len) are dropped; fewer than k left: the (-inf, -1[, -1]) tail. k defaults to min(kin, 256). pos: each
        entry's position in its input list, to carry group ids or coarse scores along."""
        q = queries.reshape(-1, queries.shape[-1]).to(self.rows.device, torch.float32).contiguous()
        if cand.dim() != 2:
            raise ValueError(f"GalleryShard.rescore: cand must be [Bq, kin], got {tuple(cand.shape)}")
        k = min(cand.shape[1], ops.nat.TOPK_KMAX) if k is None else k
        with _on(self.rows.device):
            return ops.rescore_topk(q, self.rows, cand, k, g_offset=self.offset, return_pos=return_pos)

    def expand(self, queries, scores: torch.Tensor, idx: torch.Tensor, m: int, alpha: int = 3, query_weight: float = 1.0,
               normalize: bool = True, out_dtype: torch.dtype = torch.float32, out=None):
        """Query expansion over this shard's rows (ops.expand_queries): queries f32[Bq,C] (None with query_weight = 0), scores / idx
        [Bq,kin] a list as search / rescore return it -> [Bq,C] in out_dtype on the GPU: query_weight * query + the sum over the first m
        entries of max(score, 0)^alpha * row, L2-normalised if `normalize`. Entries this shard does not hold (-1, other shards' ids)
        contribute nothing."""
        q = None if queries is None else queries.reshape(-1, queries.shape[-1]).to(self.rows.device, torch.float32).contiguous()
        with _on(self.rows.device):
            return ops.expand_queries(q, [(self.rows, self.offset)], scores, idx, m, alpha=alpha, query_weight=query_weight,
                                      normalize=normalize, out_dtype=out_dtype, out=out)

    def augmented(self, m: int, alpha: int = 3, batch: int = 4096, dtype: torch.dtype | None = None, neighbours=None):
        """Database-side augmentation: a NEW GalleryShard (same offset, labels and groups; rows in `dtype`, default this shard's) whose
        every row is the expansion, with query_weight = 0, of the row's own top-m list over `neighbours` (a GalleryShard or GallerySet;
        default: this shard, where a unit-norm row finds itself with score 1), normalised. `batch` rows are searched and expanded at a
        time. This shard is left untouched. `neighbours` that only search (a QuantizedShard over this shard's id space, e.g.
        self.quantized()) find the lists, which are then expanded over THIS shard's rows; a QuantizedGallery, like every gallery that
        expands, is also summed over."""
        _check_expansion("GalleryShard.augmented", m=m, batch=batch)
        nb = self if neighbours is None else neighbours
        rows_of = nb if hasattr(nb, "expand") else self
        out = torch.empty(self.rows.shape, dtype=dtype or self.rows.dtype, device=self.rows.device)
        for lo in range(0, len(self), int(batch)):
            s, i = nb.search(self.rows[lo:lo + int(batch)], int(m))
            rows_of.expand(None, s, i, int(m), alpha=alpha, query_weight=0.0, out_dtype=out.dtype, out=out[lo:lo + int(batch)])
        return GalleryShard(out, offset=self.offset, labels=self.labels, groups=self.groups)

    def neighbour_graph(self, k1: int, batch: int = 4096, neighbours=None):
        """The k-reciprocal neighbour graph of this shard's rows (a NeighbourGraph of width k1, for rerank): every row's top-k1 list over
        `neighbours` (a GalleryShard or GallerySet over the same id space, e.g. a 16-bit copy; default: this shard, where a unit-norm row
        finds itself, so it stays in its own reciprocal list), unfiltered, `batch` rows at a time, then pruned on the device
        (ops.knn_reciprocal) to the neighbours that lie in this shard and list the row back. 1 <= k1 <= 256, batch >= 1, else
        ValueError."""
        _check_graph_args("GalleryShard.neighbour_graph", k1, batch)
        live = [self] if len(self) else []
        return _pruned_graph(live, int(k1), [_knn_lists(sh, int(k1), batch, self if neighbours is None else neighbours) for sh in live])

    def rerank(self, scores: torch.Tensor, idx: torch.Tensor, graph, k1: int | None = None, lam: float = 0.3, k: int | None = None):
        """k-reciprocal re-ranking (set form) of lists over this shard (ops.rerank_reciprocal): scores / idx [Bq,kin] as search, rescore,
        two_stage_search or expanded_search return them, graph = self.neighbour_graph(..) -> (scores f32[Bq,k], idx i64[Bq,k]) on the GPU,
        ranked by lam * score + (1 - lam) * Jaccard(the query's k-reciprocal set among its first k1 entries, the entry's reciprocal
        neighbours). k1 defaults to the graph's width, k to min(kin, 256). Entries this shard does not hold are dropped. ValueError if the
        graph was built from other segments."""
        return _rerank("GalleryShard.rerank", [self] if len(self) else [], scores, idx, graph, k1, lam, k)

    def diversify(self, scores: torch.Tensor, idx: torch.Tensor, k: int | None = None, lam: float = 0.5, max_sim: float | None = None,
                  return_pos: bool = False):
        """Diversified lists over this shard's rows (ops.diversify_mmr): scores / idx [Bq,kin] as search, rescore, two_stage_search or
        rerank return them -> (scores f32[Bq,k], idx i64[Bq,k][, pos i32[Bq,k]]) on the GPU: greedy MMR, k times the entry with the
        greatest lam * score - (1 - lam) * (largest chain similarity to an entry already chosen), each with its input score; with
        max_sim an entry at least that similar to a chosen one is dropped for good (lam = 1: plain near-duplicate suppression). k
        defaults to min(kin, 256). Entries this shard does not hold are dropped; fewer than k chosen: the (-inf, -1[, -1]) tail."""
        return _diversify("GalleryShard.diversify", [(self.rows, self.offset)], self.rows.device, scores, idx, k, lam, max_sim, return_pos)

    def diffuse(self, scores: torch.Tensor, idx: torch.Tensor, k: int | None = None, kd: int = 8, kq: int | None = None, gamma: int = 3,
                alpha: float = 0.9, iters: int = 20, return_pos: bool = False):
        """Diffusion re-ranking of lists over this shard's rows (ops.rerank_diffusion): scores / idx [Bq,kin <= 256] as search, rescore,
        two_stage_search or rerank return them -> (scores f32[Bq,k], idx i64[Bq,k][, pos i32[Bq,k]]) on the GPU: manifold ranking on the
        mutual kd-nearest-neighbour graph of each query's candidates (affinity: chain similarity clipped at 0, to the power gamma), the
        kq first entries (None: all) injecting score ** gamma, `iters` steps f <- alpha S f + (1 - alpha) y; the entries come back ranked
        by f, with f as their score. A row far from the query but linked to it through a chain of mutually close rows rises. k defaults
        to min(kin, 256). Entries this shard does not hold are dropped; fewer than k present: the (-inf, -1[, -1]) tail."""
        return _diffuse("GalleryShard.diffuse", [(self.rows, self.offset)], self.rows.device, scores, idx, k, kd, kq, gamma, alpha, iters, return_pos)

    def cluster(self, n_clusters: int, iters: int = 20, init="maxmin", first_id=None, batch: int = 4096):
        """Spherical k-means over this shard's rows -> Clustering (centroids, assign, counts, objective, iters, converged). init "maxmin": the
        centres start as ops.kmeans_seed's farthest-point rows (first_id: the first of them, None: the smallest id), deterministic; or a
        float32 tensor [n_clusters, C] of starting centres. Per pass every row is assigned to its nearest centre by the exact search
        (centroids.search(rows, 1), `batch` rows at a time: the score is the chain score, ties go to the lower cluster) and
        ops.kmeans_update recomputes the centres; a cluster that runs empty keeps its centre. The loop ends after a pass that changes no
        row, or after `iters` passes. Search and centre step are defined to the bit, so is the result. ValueError for no rows or for
        n_clusters above the row count."""
        return _cluster("GalleryShard.cluster", [self] if len(self) else [], True, n_clusters, iters, init, first_id, batch)

    def ivf(self, n_clusters: int, nprobe: int = 8, **cluster_kwargs):
        """cluster(n_clusters, **cluster_kwargs), then IVFIndex.build over the result: a cell-probing index of this shard's rows with `nprobe`
        as its default number of probes."""
        return _ivf(self, n_clusters, nprobe, cluster_kwargs)

    def quantized(self):
        """The int8 copy of this shard (a QuantizedShard with the same offset), quantised on the device (ops.quantize_rows_i8): the cheap
        coarse stage of two_stage_search over these rows. This shard is left untouched. The labels and the group ids are carried (the same
        tensors, nothing is copied), so the copy takes the filtered and the distinct searches this shard takes."""
        return QuantizedShard.from_rows(self.rows, offset=self.offset, labels=self.labels, groups=self.groups)


class QuantizedShard:
    """Rows [offset, offset + n) of a gallery as int8 with one fp32 scale per row (ops.quantize_rows_i8), scanned on the i8 matrix cores
    (ops.similarity_topk_i8): half the bytes of a 16-bit copy and scores that are defined to the bit. This class only SEARCHES: it is the
    coarse copy that stands beside real rows, and it has no rescore, expand, rerank, diversify or diffuse. Its subclass QuantizedGallery (below; gallery()
    turns one into the other without copying) is the int8-ONLY gallery, which takes every list stage over the quantised rows alone. Use a
    QuantizedShard wherever a coarse search is taken: `coarse` of two_stage_search, a segment of a GallerySet (where the set itself
    carries the list stages for it), `neighbours` of GalleryShard.augmented / neighbour_graph (search only; GalleryShard.augmented then
    expands over its own rows), the `shard` of distributed_search.
    labels (int32[n], one per row): the shard also takes the filtered searches of a GalleryShard (ops.similarity_topk_i8_filtered).
    groups (int32[n], one group id per row, typically the source image id; negative: a group of its own): it also takes the distinct
    searches (ops.similarity_topk_i8_distinct), with or without the filter. Without them `groups` is None."""

    def __init__(self, rows_i8: torch.Tensor, scales: torch.Tensor, offset: int = 0, labels=None, groups=None):
        if labels is not None:
            labels = torch.as_tensor(labels)
            if labels.dim() != 1 or rows_i8.dim() != 2 or labels.shape[0] != rows_i8.shape[0]:
                raise ValueError(f"QuantizedShard: {tuple(labels.shape)} labels for rows {tuple(rows_i8.shape)}")
        if groups is not None:
            groups = torch.as_tensor(groups)
            if groups.dim() != 1 or rows_i8.dim() != 2 or groups.shape[0] != rows_i8.shape[0]:
                raise ValueError(f"QuantizedShard: {tuple(groups.shape)} group ids for rows {tuple(rows_i8.shape)}")
        if not rows_i8.is_cuda or not scales.is_cuda:
            raise RuntimeError("QuantizedShard lives in GPU memory (no CPU path)")
        if rows_i8.dtype != torch.int8 or rows_i8.dim() != 2:
            raise ValueError(f"QuantizedShard: rows must be int8 [n, C], got {rows_i8.dtype} {tuple(rows_i8.shape)}")
        if scales.dtype != torch.float32 or scales.dim() != 1 or scales.shape[0] != rows_i8.shape[0]:
            raise ValueError(f"QuantizedShard: scales must be float32 [{rows_i8.shape[0]}], got {scales.dtype} {tuple(scales.shape)}")
        self.rows = rows_i8.contiguous()
        self.scales = scales.to(self.rows.device).contiguous()
        self.offset = int(offset)
        self.labels = None if labels is None else _row_ids(labels, "labels", self.rows.shape[0], self.rows.device)
        self.groups = None if groups is None else _row_ids(groups, "group ids", self.rows.shape[0], self.rows.device)

    @classmethod
    def from_rows(cls, rows: torch.Tensor, offset: int = 0, labels=None, groups=None):
        """Quantise fp32 / bf16 / fp16 rows [n, C] on their device; `rows` is left untouched. labels, groups: as the constructor takes
        them."""
        if not rows.is_cuda:
            raise RuntimeError("QuantizedShard lives in GPU memory (no CPU path)")
        if rows.shape[0] == 0:
            return cls(torch.empty(rows.shape, dtype=torch.int8, device=rows.device), torch.empty((0,), dtype=torch.float32, device=rows.device), offset,
                       labels, groups)
        with torch.cuda.device(rows.device):
            q, scale = ops.quantize_rows_i8(rows)
        return cls(q, scale, offset, labels, groups)

    def __len__(self):
        return self.rows.shape[0]

    def search(self, queries: torch.Tensor, k: int, query_labels=None, mode: str = "eq", distinct: bool = False):
        """queries f32[Bq,C] -> (scores f32[Bq,k], global idx i64[Bq,k]) on the GPU, the int8 scores of ops.similarity_topk_i8;
        1 <= k <= 256. query_labels (int32[Bq], < 0 = unrestricted): only the rows allowed by the shard's labels and `mode` ("eq": same
        label, "ne": another label) are ranked (ops.similarity_topk_i8_filtered); ValueError if the shard has no labels.
        distinct: one row per group id of the shard's `groups`, the k best groups (ops.similarity_topk_i8_distinct), with or without the
        filter; idx still names the winning ROW of each group. ValueError if the shard has no group ids."""
        return _search(self, "QuantizedShard.search", (ops.similarity_topk_i8, ops.similarity_topk_i8_filtered, ops.similarity_topk_i8_distinct),
                       (self.rows, self.scales), queries, k, query_labels, mode, distinct)

    def gallery(self):
        """This shard as a QuantizedGallery over the SAME tensors (nothing is copied): the int8-only gallery with the list stages."""
        return QuantizedGallery.of(self)


class QuantizedGallery(QuantizedShard):
    """An int8-ONLY gallery: a QuantizedShard (the same constructor, from_rows and searches) that is a gallery in its own right. Beside
    the searches it takes every list stage a GalleryShard takes, over the quantised rows alone: rescore (ops.rescore_topk_i8, the int8
    score), expand (ops.expand_queries over rows whose value is float(q) * scale), neighbour_graph, rerank, diversify, diffuse and augmented; no float copy of
    the rows has to be resident. dequantized() gives the float rows it stands for. Use it as `coarse`, `fine` or both of two_stage_search,
    as the gallery of expanded_search / reranked_search, as a segment of a GallerySet beside float segments, as `neighbours` of
    GalleryShard.augmented (which then sums over THIS gallery's rows) / neighbour_graph."""

    @classmethod
    def of(cls, shard: QuantizedShard):
        """A QuantizedGallery over the tensors of `shard` (rows, scales, labels, groups: the same objects, nothing is copied or checked
        again); a QuantizedGallery is returned as it is."""
        if isinstance(shard, cls):
            return shard
        g = cls.__new__(cls)
        g.rows, g.scales, g.offset, g.labels, g.groups = shard.rows, shard.scales, shard.offset, shard.labels, shard.groups
        return g

    def rescore(self, queries: torch.Tensor, cand: torch.Tensor, k: int | None = None, return_pos: bool = False):
        """GalleryShard.rescore over the int8 rows (ops.rescore_topk_i8): queries f32[Bq,C], cand i64[Bq,kin] global row ids (at most 4096
        per query) -> (scores f32[Bq,k], idx i64[Bq,k][, pos i32[Bq,k]]) on the GPU: the int8 scores (those of search) of the candidates
        this shard holds, ranked by (score desc, id asc), every id once. Ids outside [offset, offset + len) are dropped; fewer than k
        left: the (-inf, -1[, -1]) tail. k defaults to min(kin, 256). The list search returned comes back bitwise."""
        q = queries.reshape(-1, queries.shape[-1]).to(self.rows.device, torch.float32).contiguous()
        if cand.dim() != 2:
            raise ValueError(f"QuantizedGallery.rescore: cand must be [Bq, kin], got {tuple(cand.shape)}")
        k = min(cand.shape[1], ops.nat.TOPK_KMAX) if k is None else k
        with _on(self.rows.device):
            return ops.rescore_topk_i8(q, self.rows, self.scales, cand, k, g_offset=self.offset, return_pos=return_pos)

    def expand(self, queries, scores: torch.Tensor, idx: torch.Tensor, m: int, alpha: int = 3, query_weight: float = 1.0,
               normalize: bool = True, out_dtype: torch.dtype = torch.float32, out=None):
        """GalleryShard.expand over the int8 rows (ops.expand_queries with an int8 segment): a row's value is float(q) * scale, one rounded
        multiply, so the result equals bitwise the expansion over dequantized()'s fp32 rows."""
        q = None if queries is None else queries.reshape(-1, queries.shape[-1]).to(self.rows.device, torch.float32).contiguous()
        with _on(self.rows.device):
            return ops.expand_queries(q, [(self.rows, self.scales, self.offset)], scores, idx, m, alpha=alpha, query_weight=query_weight,
                                      normalize=normalize, out_dtype=out_dtype, out=out)

    def diversify(self, scores: torch.Tensor, idx: torch.Tensor, k: int | None = None, lam: float = 0.5, max_sim: float | None = None,
                  return_pos: bool = False):
        """GalleryShard.diversify over the int8 rows (ops.diversify_mmr with an int8 segment): a row's value is float(q) * scale and the
        similarity is the fp32 chain over those values (not the int8 search score), so the result equals bitwise the diversification over
        dequantized()'s fp32 rows."""
        return _diversify("QuantizedGallery.diversify", [(self.rows, self.scales, self.offset)], self.rows.device, scores, idx, k, lam, max_sim,
                          return_pos)

    def diffuse(self, scores: torch.Tensor, idx: torch.Tensor, k: int | None = None, kd: int = 8, kq: int | None = None, gamma: int = 3,
                alpha: float = 0.9, iters: int = 20, return_pos: bool = False):
        """GalleryShard.diffuse over the int8 rows (ops.rerank_diffusion with an int8 segment): a row's value is float(q) * scale and the
        similarity is the fp32 chain over those values (not the int8 search score), so the result equals bitwise the diffusion over
        dequantized()'s fp32 rows."""
        return _diffuse("QuantizedGallery.diffuse", [(self.rows, self.scales, self.offset)], self.rows.device, scores, idx, k, kd, kq, gamma, alpha,
                        iters, return_pos)

    def cluster(self, n_clusters: int, iters: int = 20, init="maxmin", first_id=None, batch: int = 4096):
        """GalleryShard.cluster over the int8 rows: a row's value is float(q) * scale, the queries of the assignment are those values, so the
        result equals bitwise the clustering of dequantized()'s fp32 rows."""
        return _cluster("QuantizedGallery.cluster", [self] if len(self) else [], True, n_clusters, iters, init, first_id, batch)

    def ivf(self, n_clusters: int, nprobe: int = 8, **cluster_kwargs):
        """cluster(n_clusters, **cluster_kwargs), then IVFIndex.build over the result: a cell-probing index of the int8 rows with `nprobe`
        as its default number of probes."""
        return _ivf(self, n_clusters, nprobe, cluster_kwargs)

    def dequantized(self, dtype: torch.dtype = torch.float32):
        """A GalleryShard (same offset, labels and groups) of the rows this shard stands for, float(q) * scale in fp32, rounded again to
        `dtype` if it is bfloat16 / float16 (ops.dequantize_rows_i8). This shard is left untouched."""
        with _on(self.rows.device):
            rows = ops.dequantize_rows_i8(self.rows, self.scales, out_dtype=dtype)
        return GalleryShard(rows, offset=self.offset, labels=self.labels, groups=self.groups)

    def neighbour_graph(self, k1: int, batch: int = 4096, neighbours=None):
        """GalleryShard.neighbour_graph of an int8 shard: the queries of a batch are that batch's dequantised fp32 rows (the search
        quantises them again), searched over `neighbours` (default: this shard), then pruned on the device. Only one batch of rows
        ever exists in fp32."""
        _check_graph_args("QuantizedGallery.neighbour_graph", k1, batch)
        live = [self] if len(self) else []
        return _pruned_graph(live, int(k1), [_knn_lists(sh, int(k1), batch, self if neighbours is None else neighbours) for sh in live])

    def rerank(self, scores: torch.Tensor, idx: torch.Tensor, graph, k1: int | None = None, lam: float = 0.3, k: int | None = None):
        """GalleryShard.rerank over this shard: the graph and the lists are all it reads. ValueError if the graph was built from other
        segments."""
        return _rerank("QuantizedGallery.rerank", [self] if len(self) else [], scores, idx, graph, k1, lam, k)

    def augmented(self, m: int, alpha: int = 3, batch: int = 4096, neighbours=None):
        """Database-side augmentation of an int8 gallery: a NEW QuantizedGallery (same offset, labels and groups). Per batch the dequantised
        rows are searched in `neighbours` (a gallery over the same id space; default: this shard), the top-m lists are expanded over
        `neighbours` with query_weight = 0 and normalised into fp32, and that batch is quantised into the new shard: only one batch
        ever exists in fp32. This shard is left untouched."""
        _check_expansion("QuantizedGallery.augmented", m=m, batch=batch)
        nb = self if neighbours is None else neighbours
        q = torch.empty(self.rows.shape, dtype=torch.int8, device=self.rows.device)
        sc = torch.empty(self.scales.shape, dtype=torch.float32, device=self.rows.device)
        for lo in range(0, len(self), int(batch)):
            s, i = nb.search(_rows_as_queries(self, lo, lo + int(batch)), int(m))
            x = nb.expand(None, s, i, int(m), alpha=alpha, query_weight=0.0)
            with _on(self.rows.device):
                q[lo:lo + int(batch)], sc[lo:lo + int(batch)] = ops.quantize_rows_i8(x)
        return QuantizedGallery(q, sc, offset=self.offset, labels=self.labels, groups=self.groups)


class GallerySet:
    """Several GalleryShard and / or QuantizedShard (or QuantizedGallery) segments on ONE device, searched as one gallery: a gallery that grows (index today's images as a new
    segment: add(); retire a segment: drop()) without concatenating the resident rows. The segments own pairwise disjoint global row
    ranges [offset, offset + len), share the embedding width and either all carry labels (groups) or none does; their row dtypes may
    differ. A search runs every non-empty segment and merges the lists on the device (merge_topk_device): the result stays there.
    For segments of one dtype it equals bitwise the search of a single GalleryShard over the concatenated rows, because a row's
    chain score does not depend on which rows share its shard. A set can stand in for a shard in distributed_search (a rank that
    owns several segments). Int8 segments take part in every call (rescore, expand, neighbour_graph, rerank, augmented) beside float ones;
    the set carries the list stages of an int8 segment itself, so a plain QuantizedShard will do as a segment. For int8 segments alone
    each call equals bitwise the same call on ONE QuantizedGallery over the concatenated rows and scales."""

    def __init__(self, shards=()):
        self._segments = []
        for sh in shards:
            self.add(sh)

    def add(self, shard):
        lo, hi = int(shard.offset), int(shard.offset) + len(shard)
        for other in self._segments:
            if shard.rows.device != other.rows.device:
                raise ValueError(f"GallerySet: segment on {shard.rows.device}, the set lives on {other.rows.device}")
            if shard.rows.shape[1] != other.rows.shape[1]:
                raise ValueError(f"GallerySet: segment of width {shard.rows.shape[1]}, the set has width {other.rows.shape[1]}")
            if (shard.labels is None) != (other.labels is None) or (shard.groups is None) != (other.groups is None):
                raise ValueError("GallerySet: labels (and likewise groups) must be present on all segments or on none")
            olo, ohi = int(other.offset), int(other.offset) + len(other)
            if lo < ohi and olo < hi:
                raise ValueError(f"GallerySet: rows [{lo}, {hi}) overlap the segment [{olo}, {ohi})")
            if lo == olo:
                raise ValueError(f"GallerySet: a segment already starts at offset {lo}")   # (an empty one: drop() names segments by offset)
        self._segments.append(shard)
        self._segments.sort(key=lambda sh: int(sh.offset))

    def drop(self, offset: int):
        """Remove and return the segment that starts at `offset`; KeyError if none does."""
        for n, sh in enumerate(self._segments):
            if int(sh.offset) == int(offset):
                return self._segments.pop(n)
        raise KeyError(offset)

    def __len__(self):
        return sum(len(sh) for sh in self._segments)

    @property
    def segments(self):
        return list(self._segments)

    def _live(self):
        """The segments with rows: the ones a search, a graph or a segment table is made of."""
        return [sh for sh in self._segments if len(sh)]

    @property
    def rows(self):
        """A zero-row view [0, C] of the first segment: the set has no single row matrix; this carries its device and width."""
        if not self._segments:
            raise ValueError("GallerySet: an empty set has no device yet")
        return self._segments[0].rows[:0]

    @property
    def labels(self):
        return [sh.labels for sh in self._segments] if self._segments and self._segments[0].labels is not None else None

    @property
    def groups(self):
        return [sh.groups for sh in self._segments] if self._segments and self._segments[0].groups is not None else None

    def entry_groups(self, idx: torch.Tensor) -> torch.Tensor:
        """Group ids (int32, same shape, on idx's device) of global row ids out of any segment; -1 for missing entries."""
        g = torch.full(idx.shape, -1, dtype=torch.int32, device=idx.device)
        for sh in self._live():
            inside = (idx >= int(sh.offset)) & (idx < int(sh.offset) + len(sh))
            g = torch.where(inside, _entry_groups(sh, torch.where(inside, idx, torch.full_like(idx, -1))), g)
        return g

    def search(self, queries: torch.Tensor, k: int, query_labels=None, mode: str = "eq", distinct: bool = False):
        """GalleryShard.search over all segments: (scores f32[Bq,k], global idx i64[Bq,k]) on the GPU. One search per non-empty segment
        and one device merge; a single non-empty segment's result is returned as it is; no segment with rows: the all-missing lists.
        distinct: the segments' entry group ids are gathered on the device and the merge keeps the best entry per group."""
        live = self._live()
        if distinct and self._segments and self.groups is None:
            raise ValueError("GallerySet.search: distinct=True but the segments have no group ids")
        if query_labels is not None and self._segments and self.labels is None:
            raise ValueError("GallerySet.search: query_labels given but the segments have no row labels")
        if not live:
            B = queries.reshape(-1, queries.shape[-1]).shape[0]
            return _missing_lists(B, k, self._segments[0].rows.device if self._segments else queries.device)
        res = [sh.search(queries, k, query_labels=query_labels, mode=mode, distinct=distinct) for sh in live]
        if len(live) == 1:
            return res[0]
        with torch.cuda.device(live[0].rows.device):
            if distinct:
                return merge_topk_device([r[0] for r in res], [r[1] for r in res], k, [_entry_groups(sh, r[1]) for sh, r in zip(live, res)])[:2]
            return merge_topk_device([r[0] for r in res], [r[1] for r in res], k)

    def range_search(self, queries: torch.Tensor, min_score, k: int, query_labels=None, mode: str = "eq"):
        """GalleryShard.range_search over all segments: (scores f32[Bq,k], global idx i64[Bq,k], count i32[Bq]) on the GPU. One call per
        non-empty segment; the lists are merged on the device (merge_topk_device: every list holds only rows at or above the floor, so
        the merged list does) and the counts are added there: the segments' row ranges are disjoint, so the sum is the exact count over
        the set. No segment with rows: all-missing lists and zero counts. An int8 segment raises ValueError: the range search has no
        int8 form yet (QuantizedShard has no range_search). query_labels / mode: the filter of GalleryShard.range_search, applied in
        every segment (allowed rows only, in lists and counts)."""
        if query_labels is not None and self._segments and self.labels is None:
            raise ValueError("GallerySet.range_search: query_labels given but the segments have no row labels")
        live = self._live()
        for sh in live:
            if isinstance(sh, QuantizedShard):
                raise ValueError("GallerySet.range_search: the segment at offset %d holds int8 rows; the range search covers fp32 / bf16 / "
                                 "fp16 segments only (no int8 range search yet)" % int(sh.offset))
        if not live:
            if not 1 <= int(k) <= ops.nat.TOPK_KMAX:
                raise ValueError(f"GallerySet.range_search: k must be in [1, {ops.nat.TOPK_KMAX}], got {k}")
            B = queries.reshape(-1, queries.shape[-1]).shape[0]
            dev = self._segments[0].rows.device if self._segments else queries.device
            return (*_missing_lists(B, k, dev), torch.zeros((B,), dtype=torch.int32, device=dev))
        if query_labels is None:
            res = [sh.range_search(queries, min_score, k) for sh in live]
        else:
            res = [sh.range_search(queries, min_score, k, query_labels=query_labels, mode=mode) for sh in live]
        if len(live) == 1:
            return res[0]
        with torch.cuda.device(live[0].rows.device):
            scores, idx = merge_topk_device([r[0] for r in res], [r[1] for r in res], k)
            return scores, idx, torch.stack([r[2] for r in res]).sum(0, dtype=torch.int32)

    def rescore(self, queries: torch.Tensor, cand: torch.Tensor, k: int):
        """GalleryShard.rescore over all segments: (scores f32[Bq,k], global idx i64[Bq,k]) on the GPU. Every non-empty segment
        re-scores the same cand; an id outside a segment is missing for it and the segments' ranges are disjoint, so every id is
        scored exactly once, and the lists are merged on the device (merge_topk_device). A single non-empty segment's result is
        returned as it is; no segment with rows: the all-missing lists. For segments of one dtype the result equals bitwise that of
        a single GalleryShard over the concatenated rows."""
        live = self._live()
        if not live:
            if not 1 <= int(k) <= ops.nat.TOPK_KMAX:
                raise ValueError(f"GallerySet.rescore: k must be in [1, {ops.nat.TOPK_KMAX}], got {k}")
            return _missing_lists(cand.shape[0], k, self._segments[0].rows.device if self._segments else cand.device)
        res = [_with_lists(sh).rescore(queries, cand, k) for sh in live]
        if len(live) == 1:
            return res[0]
        with torch.cuda.device(live[0].rows.device):
            return merge_topk_device([r[0] for r in res], [r[1] for r in res], k)

    def expand(self, queries, scores: torch.Tensor, idx: torch.Tensor, m: int, alpha: int = 3, query_weight: float = 1.0,
               normalize: bool = True, out_dtype: torch.dtype = torch.float32, out=None):
        """GalleryShard.expand over all segments in ONE launch: the kernel looks every listed id up in the table of the live segments
        (at most 16; their dtypes may differ, int8 segments with their row scales included), so nothing is concatenated and no
        per-segment partial sums exist. The result equals bitwise that of a single GalleryShard (for int8 segments alone: a single
        QuantizedGallery) over the concatenated rows."""
        live = self._live()
        dev = live[0].rows.device if live else scores.device
        q = None if queries is None else queries.reshape(-1, queries.shape[-1]).to(dev, torch.float32).contiguous()
        with _on(dev):
            table = [(sh.rows, sh.scales, sh.offset) if isinstance(sh, QuantizedShard) else (sh.rows, sh.offset) for sh in live]
            return ops.expand_queries(q, table, scores, idx, m, alpha=alpha, query_weight=query_weight,
                                      normalize=normalize, out_dtype=out_dtype, out=out)

    def diversify(self, scores: torch.Tensor, idx: torch.Tensor, k: int | None = None, lam: float = 0.5, max_sim: float | None = None,
                  return_pos: bool = False):
        """GalleryShard.diversify over all segments in ONE launch: the kernel looks every listed id up in the table of the live segments
        (at most 16; their dtypes may differ, int8 segments, a plain QuantizedShard included, with their row scales). The result equals
        bitwise that of a single fp32 GalleryShard over the concatenated widened / dequantised rows."""
        live = self._live()
        table = [(sh.rows, sh.scales, sh.offset) if isinstance(sh, QuantizedShard) else (sh.rows, sh.offset) for sh in live]
        return _diversify("GallerySet.diversify", table, live[0].rows.device if live else scores.device, scores, idx, k, lam, max_sim, return_pos)

    def diffuse(self, scores: torch.Tensor, idx: torch.Tensor, k: int | None = None, kd: int = 8, kq: int | None = None, gamma: int = 3,
                alpha: float = 0.9, iters: int = 20, return_pos: bool = False):
        """GalleryShard.diffuse over all segments in ONE launch: the kernel looks every listed id up in the table of the live segments
        (at most 16; their dtypes may differ, int8 segments, a plain QuantizedShard included, with their row scales). The result equals
        bitwise that of a single fp32 GalleryShard over the concatenated widened / dequantised rows."""
        live = self._live()
        table = [(sh.rows, sh.scales, sh.offset) if isinstance(sh, QuantizedShard) else (sh.rows, sh.offset) for sh in live]
        return _diffuse("GallerySet.diffuse", table, live[0].rows.device if live else scores.device, scores, idx, k, kd, kq, gamma, alpha, iters,
                        return_pos)

    def cluster(self, n_clusters: int, iters: int = 20, init="maxmin", first_id=None, batch: int = 4096):
        """GalleryShard.cluster over all segments as one gallery (at most 16 non-empty ones; their dtypes may differ, a plain
        QuantizedShard included). Clustering.assign is a list, one tensor per non-empty segment in offset order. The result equals bitwise
        that of a single fp32 GalleryShard over the concatenated widened / dequantised rows."""
        return _cluster("GallerySet.cluster", self._live(), False, n_clusters, iters, init, first_id, batch)

    def ivf(self, n_clusters: int, nprobe: int = 8, **cluster_kwargs):
        """cluster(n_clusters, **cluster_kwargs), then IVFIndex.build over the result: a cell-probing index of all segments (they must share one dtype) with `nprobe`
        as its default number of probes."""
        return _ivf(self, n_clusters, nprobe, cluster_kwargs)

    def augmented(self, m: int, alpha: int = 3, batch: int = 4096, dtype: torch.dtype | None = None):
        """Database-side augmentation of every segment with the WHOLE set as neighbours (GalleryShard.augmented(neighbours=self)): a new
        GallerySet of new segments; this set and its segments are left untouched. An int8 segment becomes a new int8 segment
        (QuantizedGallery.augmented; `dtype` applies to the float segments)."""
        return GallerySet([QuantizedGallery.of(sh).augmented(m, alpha=alpha, batch=batch, neighbours=self) if isinstance(sh, QuantizedShard) else
                           sh.augmented(m, alpha=alpha, batch=batch, dtype=dtype, neighbours=self) for sh in self._segments])

    def neighbour_graph(self, k1: int, batch: int = 4096):
        """GalleryShard.neighbour_graph over all segments: every row's top-k1 list over the WHOLE set, pruned against the lists of all
        segments (at most 16 non-empty ones). The graph is valid for the segments the set has now; add / drop do not update it."""
        _check_graph_args("GallerySet.neighbour_graph", k1, batch)
        live = self._live()
        if len(live) > ops.nat.RERANK_SEGMAX:
            raise ValueError(f"GallerySet.neighbour_graph: {len(live)} non-empty segments, a graph spans at most {ops.nat.RERANK_SEGMAX}")
        return _pruned_graph(live, int(k1), [_knn_lists(sh, int(k1), batch, self) for sh in live])

    def rerank(self, scores: torch.Tensor, idx: torch.Tensor, graph, k1: int | None = None, lam: float = 0.3, k: int | None = None):
        """GalleryShard.rerank over all segments in ONE launch: the kernel looks every id up in the graph's segment table. The result
        equals bitwise that of a single GalleryShard over the concatenated rows with the same lists. ValueError if the set's non-empty
        segments are not the ones the graph was built from."""
        return _rerank("GallerySet.rerank", self._live(), scores, idx, graph, k1, lam, k)


class IVFIndex:
    """A cell-probing index ("IVF-flat") over a clustered gallery: the rows stored cell by cell (ops.ivf_build), searched by scoring only
    the rows of the `nprobe` cells whose centres a query scores best against (ops.ivf_search). The result is the EXACT top-k of those
    rows, by the gallery dtype's own score and order, with global ids; at nprobe = K it is the gallery's exact search bit for bit.
    centroids: a GalleryShard of the K centres (offset 0: its row index is the cell). rows, scales (int8 rows only, else None), ids,
    cell_start: the cell-contiguous storage. counts: int32 [K], the cells' sizes. max_cell: the largest of them, read ONCE at build (the
    build's one host synchronisation). nprobe: the default number of probes.
    The index is fixed at build: no rows are added or removed, and it takes no label filter, no distinct= and no range search."""

    def __init__(self, centroids, rows, scales, ids, cell_start, counts, max_cell, nprobe=8):
        self.centroids, self.rows, self.scales, self.ids, self.cell_start = centroids, rows, scales, ids, cell_start
        self.counts, self.max_cell, self.nprobe = counts, int(max_cell), int(nprobe)

    def __len__(self):
        return self.rows.shape[0]

    @property
    def n_cells(self):
        return len(self.centroids)

    @classmethod
    def build(cls, gallery, clustering=None, *, centroids=None, assign=None, nprobe: int = 8):
        """gallery: a GalleryShard, a QuantizedGallery (or QuantizedShard) or a GallerySet whose segments share one dtype. clustering: what
        gallery.cluster returned; or centroids (float32 [K,C] tensor or a GalleryShard) and assign (int32, one tensor over all rows in
        ascending global id, or one per non-empty segment in offset order), e.g. as save_gallery carried them. A row whose assign value
        lies outside [0, K) is not indexed. One host synchronisation (max_cell)."""
        who = "IVFIndex.build"
        if (clustering is None) == (centroids is None and assign is None) or (clustering is None and (centroids is None or assign is None)):
            raise ValueError(f"{who}: pass a Clustering, or both centroids= and assign=")
        if clustering is not None:
            centroids, assign = clustering.centroids, clustering.assign
        if int(nprobe) < 1:
            raise ValueError(f"{who}: nprobe must be at least 1, got {nprobe}")
        live = gallery._live() if isinstance(gallery, GallerySet) else ([gallery] if len(gallery) else [])
        if not live:
            raise ValueError(f"{who}: nothing to index (no rows)")
        if len(live) > ops.nat.CLUSTER_SEGMAX:
            raise ValueError(f"{who}: {len(live)} non-empty segments, one index spans at most {ops.nat.CLUSTER_SEGMAX}")
        if len({(isinstance(sh, QuantizedShard), sh.rows.dtype) for sh in live}) != 1:
            raise ValueError(f"{who}: the segments must share one dtype (rows are copied, never converted)")
        dev, C = live[0].rows.device, live[0].rows.shape[1]
        cent = centroids.rows if isinstance(centroids, GalleryShard) else centroids
        if not isinstance(cent, torch.Tensor) or cent.dtype != torch.float32 or cent.dim() != 2 or cent.shape[1] != C or not 1 <= cent.shape[0] <= ops.nat.KMEANS_KMAX:
            raise ValueError(f"{who}: centroids must be float32 [1..{ops.nat.KMEANS_KMAX}, {C}]")
        if isinstance(centroids, GalleryShard) and centroids.offset != 0:
            raise ValueError(f"{who}: the centroid shard must start at offset 0 (its row index is the cell)")
        K = cent.shape[0]
        if isinstance(assign, torch.Tensor):
            if assign.dim() != 1 or assign.shape[0] != sum(len(sh) for sh in live):
                raise ValueError(f"{who}: assign has {tuple(assign.shape)} entries, the gallery {sum(len(sh) for sh in live)} rows")
            assign = list(torch.split(assign, [len(sh) for sh in live]))
        assign = list(assign)
        if len(assign) != len(live) or any(a.dim() != 1 or a.shape[0] != len(sh) or a.dtype != torch.int32 for a, sh in zip(assign, live)):
            raise ValueError(f"{who}: assign must be int32, one entry per row (one tensor per non-empty segment in offset order)")
        table = [(sh.rows, sh.scales, sh.offset) if isinstance(sh, QuantizedShard) else (sh.rows, sh.offset) for sh in live]
        with _on(dev):
            rows, scales, ids, cell_start = ops.ivf_build(table, [a.to(dev) for a in assign], K)
            counts = cell_start[1:] - cell_start[:-1]
            max_cell = max(int(counts.max().item()), 1)                  # the build's one synchronisation
            centres = centroids if isinstance(centroids, GalleryShard) and centroids.rows.device == dev else GalleryShard(cent.to(dev), offset=0)
        return cls(centres, rows, scales, ids, cell_start, counts, max_cell, nprobe)

    def search(self, queries: torch.Tensor, k: int, nprobe: int | None = None, return_scanned: bool = False):
        """queries f32[Bq,C] -> (scores f32[Bq,k], global idx i64[Bq,k][, scanned i32[Bq]]) on the GPU; 1 <= k <= 256. The probes are
        centroids.search(queries, min(nprobe, K)) (the exact search; nprobe defaults to the index's, at most 256), then ops.ivf_search
        scores the rows of those cells: the exact top-k among them, then the (-inf, -1) tail. scanned: how many rows each query scored.
        Nothing leaves the device and the host is not waited for."""
        np_ = self.nprobe if nprobe is None else int(nprobe)
        if np_ < 1:
            raise ValueError(f"IVFIndex.search: nprobe must be at least 1, got {nprobe}")
        if not 1 <= int(k) <= ops.nat.TOPK_KMAX:
            raise ValueError(f"IVFIndex.search: k must be in [1, {ops.nat.TOPK_KMAX}], got {k}")
        np_ = min(np_, self.n_cells, ops.nat.IVF_NPROBE_MAX)
        dev = self.rows.device
        q = queries.reshape(-1, queries.shape[-1]).to(dev, torch.float32).contiguous()
        if q.shape[0] == 0:
            s, i = _missing_lists(0, int(k), dev)
            return (s, i, torch.empty((0,), dtype=torch.int32, device=dev)) if return_scanned else (s, i)
        probes = self.centroids.search(q, np_)[1]
        with _on(dev):
            return ops.ivf_search(q, self.rows, self.scales, self.ids, self.cell_start, probes, int(k), self.max_cell,
                                  return_scanned=return_scanned)


def _ivf(gallery, n_clusters, nprobe, cluster_kwargs):
    """.ivf of the gallery classes: cluster, then build."""
    return IVFIndex.build(gallery, gallery.cluster(n_clusters, **cluster_kwargs), nprobe=nprobe)


def _with_lists(shard):
    """A segment as something that takes the list stages: a plain QuantizedShard as the QuantizedGallery over its tensors."""
    return QuantizedGallery.of(shard) if isinstance(shard, QuantizedShard) else shard


def two_stage_search(queries: torch.Tensor, coarse, fine, k: int, k_coarse: int, fine_queries: torch.Tensor | None = None, **search_kwargs):
    """Two-stage search on one device: coarse.search(queries, k_coarse, **search_kwargs) finds the candidates, fine.rescore(fine_queries
    if given else queries, idx, k) orders them again and keeps k -> (scores f32[Bq,k], idx i64[Bq,k]) on the GPU, the scores being
    `fine`'s scores (chain scores of float rows, int8 scores of a QuantizedGallery). coarse and fine are each a GalleryShard, a QuantizedShard
    (coarse only), a QuantizedGallery or a GallerySet (float, int8 or mixed segments) over the SAME global id space: typically a bf16 /
    fp16 copy that is scanned on the matrix cores and the fp32 master rows, which give the final order at fp32 precision (the 16-bit
    stage rounds the query to the gallery dtype too; the second stage takes it unrounded). fine_queries: another embedding of the same
    requests for the second stage (e.g. the exact-query mode's fp32 feat). A candidate row that `fine` does not hold drops out; fewer
    than k left: the (-inf, -1) tail. k <= k_coarse <= 256, else ValueError. search_kwargs go to the coarse search (query_labels, mode,
    distinct). With distinct=True the COARSE stage fixes each group's representative row and the k_coarse groups; the second stage
    re-orders those rows and does not look for a better row of a group. Nothing leaves the device and the host is not waited for."""
    if not 1 <= int(k) <= int(k_coarse) <= ops.nat.TOPK_KMAX:
        raise ValueError(f"two_stage_search: need 1 <= k <= k_coarse <= {ops.nat.TOPK_KMAX}, got k={k}, k_coarse={k_coarse}")
    _, idx = coarse.search(queries, int(k_coarse), **search_kwargs)
    return fine.rescore(queries if fine_queries is None else fine_queries, idx, int(k))


def _check_expansion(who, m=1, k=1, rounds=1, batch=1):
    if not 1 <= int(m) <= ops.nat.TOPK_KMAX or not 1 <= int(k) <= ops.nat.TOPK_KMAX:
        raise ValueError(f"{who}: m and k must be in [1, {ops.nat.TOPK_KMAX}], got m={m}, k={k}")
    if int(rounds) < 1 or int(batch) < 1:
        raise ValueError(f"{who}: rounds and batch must be at least 1, got rounds={rounds}, batch={batch}")


def expanded_search(queries: torch.Tensor, gallery, k: int, m: int, alpha: int = 3, query_weight: float = 1.0, rounds: int = 1, **search_kwargs):
    """Search with query expansion on one device: `rounds` times q <- gallery.expand(q, *gallery.search(q, m, **search_kwargs), m)
    (q starts as `queries`; each round expands the query of the round before), then gallery.search(q, k, **search_kwargs)
    -> (scores f32[Bq,k], idx i64[Bq,k], expanded queries f32[Bq,C]) on the GPU. gallery: a GalleryShard, a QuantizedGallery (an int8-only
    gallery) or a GallerySet of either. alpha and
    query_weight as in ops.expand_queries (alpha = 0, query_weight = 1: plain AQE); the expanded query is L2-normalised. 1 <= m <= 256,
    1 <= k <= 256, rounds >= 1, else ValueError. search_kwargs (query_labels, mode, distinct) apply to EVERY search, so a filtered
    expansion only sums rows the filter allows. Nothing leaves the device and the host is not waited for. distributed_search has no
    such option: the rows to sum live on other ranks."""
    _check_expansion("expanded_search", m=m, k=k, rounds=rounds)
    q = queries
    for _ in range(int(rounds)):
        s, i = gallery.search(q, int(m), **search_kwargs)
        q = gallery.expand(q, s, i, int(m), alpha=alpha, query_weight=query_weight)
    s, i = gallery.search(q, int(k), **search_kwargs)
    return s, i, q


def reranked_search(queries: torch.Tensor, gallery, graph, k: int, k_coarse: int, k1: int | None = None, lam: float = 0.3, **search_kwargs):
    """Search with k-reciprocal re-ranking on one device: gallery.search(queries, k_coarse, **search_kwargs) followed by
    gallery.rerank(scores, idx, graph, k1=k1, lam=lam, k=k) -> (scores f32[Bq,k], idx i64[Bq,k]) on the GPU. gallery: a GalleryShard, a
    QuantizedGallery (an int8-only gallery) or a GallerySet of either, graph: its neighbour_graph. 1 <= k <= k_coarse <= 256, else ValueError; k1 defaults to the graph's width and must not
    exceed k_coarse. search_kwargs (query_labels, mode, distinct) go to the search; with distinct=True the candidates are the
    representatives' rows and their graph rows are used as they are. Nothing leaves the device and the host is not waited for.
    distributed_search has no such option: a candidate's graph row lives on the rank that owns the row."""
    if not 1 <= int(k) <= int(k_coarse) <= ops.nat.TOPK_KMAX:
        raise ValueError(f"reranked_search: need 1 <= k <= k_coarse <= {ops.nat.TOPK_KMAX}, got k={k}, k_coarse={k_coarse}")
    s, i = gallery.search(queries, int(k_coarse), **search_kwargs)
    return gallery.rerank(s, i, graph, k1=k1, lam=lam, k=int(k))


def diversified_search(queries: torch.Tensor, gallery, k: int, k_coarse: int, lam: float = 0.5, max_sim: float | None = None, **search_kwargs):
    """Search with diversified results on one device: gallery.search(queries, k_coarse, **search_kwargs) followed by
    gallery.diversify(scores, idx, k=k, lam=lam, max_sim=max_sim) -> (scores f32[Bq,k], idx i64[Bq,k]) on the GPU: the k entries greedy MMR
    picks out of the k_coarse best, each with its search score. gallery: a GalleryShard, a QuantizedGallery (an int8-only gallery) or a
    GallerySet of either. 1 <= k <= k_coarse <= 256, 0 <= lam <= 1, max_sim not NaN, else ValueError before anything runs. search_kwargs
    (query_labels, mode, distinct) go to the search; distinct=True removes repeats that share a group id, the diversification those that
    merely look alike. Nothing leaves the device and the host is not waited for. distributed_search has no such option: a candidate's row
    lives on the rank that owns it."""
    if not 1 <= int(k) <= int(k_coarse) <= ops.nat.TOPK_KMAX:
        raise ValueError(f"diversified_search: need 1 <= k <= k_coarse <= {ops.nat.TOPK_KMAX}, got k={k}, k_coarse={k_coarse}")
    if not 0.0 <= float(lam) <= 1.0 or (max_sim is not None and float(max_sim) != float(max_sim)):
        raise ValueError(f"diversified_search: lam must be in [0, 1] and max_sim not NaN, got lam={lam}, max_sim={max_sim}")
    s, i = gallery.search(queries, int(k_coarse), **search_kwargs)
    return gallery.diversify(s, i, k=int(k), lam=lam, max_sim=max_sim)


def diffused_search(queries: torch.Tensor, gallery, k: int, k_coarse: int, kd: int = 8, kq: int | None = None, gamma: int = 3, alpha: float = 0.9,
                    iters: int = 20, **search_kwargs):
    """Search with diffusion re-ranking on one device: gallery.search(queries, k_coarse, **search_kwargs) followed by
    gallery.diffuse(scores, idx, k=k, kd=kd, kq=kq, gamma=gamma, alpha=alpha, iters=iters) -> (scores f32[Bq,k], idx i64[Bq,k]) on the GPU:
    the k_coarse best re-ranked by manifold ranking on their mutual kd-nearest-neighbour graph, the scores being the diffused values.
    gallery: a GalleryShard, a QuantizedGallery (an int8-only gallery) or a GallerySet of either. 1 <= k <= k_coarse <= 256,
    1 <= kd <= 32, kq >= 1 or None, 1 <= gamma <= 4, 0 <= alpha < 1, 1 <= iters <= 64, else ValueError before anything runs.
    search_kwargs (query_labels, mode, distinct) go to the search. Nothing leaves the device and the host is not waited for.
    distributed_search has no such option: a candidate's row lives on the rank that owns it."""
    if not 1 <= int(k) <= int(k_coarse) <= ops.nat.DIFFUSE_NMAX:
        raise ValueError(f"diffused_search: need 1 <= k <= k_coarse <= {ops.nat.DIFFUSE_NMAX}, got k={k}, k_coarse={k_coarse}")
    if not 1 <= int(kd) <= ops.nat.DIFFUSE_KDMAX or (kq is not None and int(kq) < 1) or not 1 <= int(gamma) <= 4 or not 1 <= int(iters) <= 64:
        raise ValueError(f"diffused_search: need 1 <= kd <= {ops.nat.DIFFUSE_KDMAX}, kq >= 1, 1 <= gamma <= 4, 1 <= iters <= 64, "
                         f"got kd={kd}, kq={kq}, gamma={gamma}, iters={iters}")
    if not 0.0 <= float(alpha) < 1.0:
        raise ValueError(f"diffused_search: alpha must be in [0, 1), got {alpha}")
    s, i = gallery.search(queries, int(k_coarse), **search_kwargs)
    return gallery.diffuse(s, i, k=int(k), kd=kd, kq=kq, gamma=gamma, alpha=alpha, iters=iters)


def fused_search(queries, gallery, k: int, k_each: int, weights=None, mode: str = "rrf", rrf_c: float = 60.0, normalize: str = "none",
                 missing: str = "zero", **search_kwargs):
    """Search with late fusion on one device: P searches at k_each and one fusion (fuse_lists_device) -> (scores f32[Bq,k], idx i64[Bq,k])
    on the GPU, one entry per distinct gallery row, ranked by the fused score. queries: a sequence of P tensors [Bq,C] or one tensor
    [P,Bq,C], the P shots or views of the same Bq requests (several (support image, mask, text) triplets of one target; the composed query,
    its expanded form and the exact-query feat). gallery: one gallery, searched by every view, or a sequence of P galleries over the SAME
    global id space, view p searching gallery p (the fp32 master rows and their augmented() copy; a QuantizedGallery and a bf16
    GalleryShard); each a GalleryShard, a QuantizedShard, a QuantizedGallery or a GallerySet. weights, mode, rrf_c, normalize, missing as
    ops.fuse_lists takes them; reciprocal-rank fusion is the default. 1 <= P <= 16, 1 <= k <= 256, 1 <= k_each <= 256, else ValueError
    before anything runs. search_kwargs (query_labels, distinct; the filter's "eq" / "ne" goes as filter_mode, because mode names the
    fusion) apply to EVERY search. Nothing leaves the device and the host is not waited for. distributed_search has no such option: ranks and per-list
    statistics are per shard, so fusing before the merge is not the fusion of the global lists."""
    if isinstance(queries, torch.Tensor):
        if queries.dim() != 3:
            raise ValueError(f"fused_search: queries must be a sequence of [Bq, C] tensors or one [P, Bq, C] tensor, got {tuple(queries.shape)}")
        views = list(queries.unbind(0))
    else:
        views = list(queries)
    P = len(views)
    if not 1 <= int(k_each) <= ops.nat.TOPK_KMAX:
        raise ValueError(f"fused_search: k_each must be in [1, {ops.nat.TOPK_KMAX}], got {k_each}")
    ops.fuse_args("fused_search", P, k, weights, mode, rrf_c, normalize, missing)
    galleries = list(gallery) if isinstance(gallery, (list, tuple)) else [gallery] * P
    if len(galleries) != P:
        raise ValueError(f"fused_search: {len(galleries)} galleries for {P} views: one gallery, or one per view")
    if any(v.dim() != 2 or v.shape != views[0].shape for v in views):
        raise ValueError(f"fused_search: the views must be [Bq, C] tensors of one shape, got {[tuple(v.shape) for v in views]}")
    if "filter_mode" in search_kwargs:
        search_kwargs["mode"] = search_kwargs.pop("filter_mode")
    res = [g.search(v, int(k_each), **search_kwargs) for g, v in zip(galleries, views)]
    return fuse_lists_device([r[0] for r in res], [r[1] for r in res], int(k), weights=weights, mode=mode, rrf_c=rrf_c, normalize=normalize,
                             missing=missing)


def shard_bounds(n_rows: int, world: int, rank: int):
    per = -(-n_rows // world)
    lo = min(rank * per, n_rows)
    return lo, min(lo + per, n_rows)


def _pack_lists(s: torch.Tensor, i: torch.Tensor) -> torch.Tensor:
    """(scores f32[B,k], idx i64[B,k]) -> ONE int32 tensor [B,k,3] (score bits, index lo, index hi): 12 B per entry."""
    out = torch.empty(s.shape + (3,), dtype=torch.int32, device=s.device)
    out[..., 0] = s.contiguous().view(torch.int32)
    out[..., 1:] = i.contiguous().view(torch.int32).view(i.shape + (2,))
    return out


def _entry_groups(shard, i: torch.Tensor) -> torch.Tensor:
    """Group ids (int32, same shape) of the global row ids i of `shard` (on i's device); a missing entry (-1) gets -1 (the clamps
    only keep its gather in range). The searches behind this never run with TOPK_NO_FALLBACK, so no -2 marker arrives here. For a
    GalleryShard the groups already live on that device and the conversion below copies nothing."""
    local = (i - int(shard.offset)).clamp(min=0)
    groups = torch.as_tensor(shard.groups).to(i.device)
    if groups.shape[0] == 0:
        return torch.full(i.shape, -1, dtype=torch.int32, device=i.device)
    g = groups[local.clamp(max=groups.shape[0] - 1)].to(torch.int32)
    return torch.where(i >= 0, g, torch.full_like(g, -1))


def _unpack_lists(p: torch.Tensor):
    return p[..., 0].contiguous().view(torch.float32), p[..., 1:].contiguous().view(torch.int64).squeeze(-1)


class _Marks:
    """Time marks of one distributed_search call (bench.py's `rccl` record): device events on the CURRENT stream under RCCL
    (torch's collectives run on their own stream, but the blocking forms make the current stream wait for them, so events on the
    current stream bracket them), host clocks under gloo (whose collectives work on host copies and synchronise anyway)."""

    def __init__(self, dev, host):
        self.dev, self.host, self.t = dev, host, []

    def mark(self):
        if self.host:
            import time
            self.t.append(time.perf_counter())
        else:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream(self.dev))
            self.t.append(ev)

    def ms(self, a, b):
        return (self.t[b] - self.t[a]) * 1e3 if self.host else self.t[a].elapsed_time(self.t[b])


def resolve_timing(timing: list) -> dict:
    """Means over the calls recorded in `timing` (after a device synchronisation): collective_ms = query all-gather + list gather,
    search_ms = this rank's shard against all query slots (+ packing; + the host copies under gloo)."""
    n = max(len(timing), 1)
    ag = sum(m.ms(0, 1) for m in timing) / n
    se = sum(m.ms(1, 2) for m in timing) / n
    ga = sum(m.ms(2, 3) for m in timing) / n
    return dict(calls=len(timing), allgather_ms=ag, search_ms=se, gather_ms=ga, collective_ms=ag + ga)


class PendingSearch:
    """A search whose lists are still on their way to the host (distributed_search(..., defer=True)): the ONE device-to-host copy
    went to pinned memory behind an event, so the caller can enqueue the next step's forward first and call result() afterwards -
    the GPU never waits for the host merge. result() -> (scores, idx) CPU tensors on `dst` (every rank for dst=None), (None, None)
    elsewhere ((scores, idx, count) and (None, None, None) for a range search, min_score); idempotent."""

    def __init__(self, finish=None, event=None, value=None):
        self._finish, self._event, self._value = finish, event, value

    def result(self):
        if self._finish is not None:
            if self._event is not None:
                self._event.synchronize()
            self._value, self._finish, self._event = self._finish(), None, None
        return self._value


def _to_host_async(t: torch.Tensor):
    """Device tensor -> pinned host tensor, non-blocking, + the event that marks the copy's completion on the current stream."""
    if not t.is_cuda:
        return t, None
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(t.device))
    return h, ev


def distributed_search(local_queries: torch.Tensor, shard: GalleryShard, k: int, group=None, max_local: int | None = None,
                       dst: int | None = 0, timing: list | None = None, always_collective: bool = False, defer: bool = False,
                       query_labels=None, filter_mode: str = "eq", distinct: bool = False, merge: str = "host", min_score=None):
    """All ranks call this with their own queries [B_local, C] and their gallery shard.

    Two collectives in all, as BASELINE.json's north_star describes it:
      1. ONE all-gather of the query embeddings over RCCL/xGMI (<= 64 KB per rank: latency-bound). The payload is a
         fixed-size block [max_local + 1, C]: rows 0..B_local-1 are the queries, the rest zeros, the last row carries B_local,
         so a ragged last batch (B_local differing between ranks) is legal as long as every rank passes the same `max_local`
         (a configuration constant, e.g. the loader's batch size; default: this rank's B_local, i.e. equal batches);
      2. each rank scores ALL world * max_local query SLOTS against its shard (cor_similarity_topk; the slots beyond a rank's
         count are zero rows whose results are dropped at the end - nothing is compacted, so the counts never have to reach
         the host in the middle of the step) and the packed per-shard lists ([slots,k,3] int32 = 12 B per entry) go to rank
         `dst` in ONE gather, where they are merged ONCE on the host by (score desc, global index asc). dst=None: all-gather
         instead, every rank merges.
    Host synchronisation (backend nccl = RCCL): none on the ranks that return (None, None); on `dst` exactly one device-to-host
    copy at the very end (lists + per-rank counts in one buffer) - the next step's forward can be enqueued before it is awaited.
    Under the gloo REHEARSAL backend the collectives work on host copies, so every rank synchronises twice (queries, lists).
    `max_local` must be given (and equal on all ranks) whenever per-rank query counts can differ: the all-gather is fixed-size.
    timing: a list that receives one _Marks per call (resolve_timing() turns them into milliseconds after a synchronisation).
    always_collective: take the collective path even in a group of ONE rank (tests: the only way to put this code on RCCL with a
    single GPU - a one-rank nccl group still moves the device tensors through all_gather_into_tensor / gather).
    defer: return a PendingSearch instead of the tensors: the device-to-host copy is enqueued (pinned memory + event) and the host merge
    happens in its result() - call it after enqueuing the next step's forward, so that the GPU does not idle through the host's turn.
    Returns (scores f32[B_total,k], idx i64[B_total,k]) CPU tensors, queries ordered by rank, on rank `dst` (every rank
    for dst=None); (None, None) on the other ranks. k: 1 .. 256 (recall_at_k turns the lists into Recall@K).
    query_labels: int32[B_local] (< 0 = unrestricted), best on the queries' device: a filtered search (GalleryShard.search with
    filter_mode "eq" / "ne" over each shard's row labels). The labels travel bit-cast in one extra column of the same fixed-size
    all-gather block, so the call keeps its two collectives; None leaves the payload and the call shard.search(q, k) as they were.
    distinct: one entry per group id (shard.groups, e.g. the source image), the k best groups over ALL shards although an image's
    regions may sit in two of them: every rank searches with distinct=True, its packed list carries a fourth int32 per entry, the
    entry's group id (gathered on the device from shard.groups), and the host merge keeps the best entry per non-negative group id
    before it cuts to k (merge_topk_distinct_host has the proof). Still two collectives and one device-to-host copy; defer works.
    Without it the payloads, the [B,k,3] packing and the calls to shard.search are exactly as above.
    merge: "host" (default) is the path described above. "device" (RCCL groups only; under gloo the lists are host copies: ValueError
    on every rank before any collective): the merging rank(s) unpack the gathered lists and merge ALL world * max_local slots on the GPU
    (merge_topk_device's kernel; plain or distinct), so the one device-to-host copy carries [slots, k] scores and indices plus the
    per-rank counts instead of `world` lists per slot, and the host only drops the slots beyond each rank's count. Same results,
    bitwise; defer, dst=None, query_labels and distinct work as before; the single-rank shortcut's lists are final either way.
    shard: a GalleryShard, or a GallerySet for a rank that owns several segments (anything with .search, .rows.device, .groups and
    either .offset or an entry_groups(idx) method).
    min_score: None (default) leaves payloads, calls and the return value exactly as described above. A float, or an f32 tensor [B_local]
    of per-query floors, turns the call into a RANGE search over all shards (shard.range_search, with query_labels / filter_mode when
    labels are given): the result is (scores, idx, count), count int64 [B_total] = the sum of the shards' exact member counts, on the
    merging rank(s), (None, None, None) elsewhere; the lists are the first k members over all shards. Still two collectives and one
    device-to-host copy: the floors travel bit-cast in one more column of the all-gather block (beside the label column when there is
    one; a padding slot gets +inf, so it has no member and no band row) and each slot's count travels as one more int32 behind its packed
    list ([slots, 3 k + 1]) in the second collective. dst=None, defer and both merges work as before. distinct=True with min_score, or
    a shard without range_search (int8 rows: QuantizedShard, or a set with an int8 segment) raise ValueError on every rank before any
    collective."""
    import torch.distributed as dist
    if merge not in ("host", "device"):
        raise ValueError(f"distributed_search: merge must be 'host' or 'device', got {merge!r}")
    if distinct and getattr(shard, "groups", None) is None:
        raise ValueError("distributed_search: distinct=True but the shard has no group ids")
    ranged = min_score is not None
    if ranged:
        if distinct:
            raise ValueError("distributed_search: min_score and distinct=True do not go together (the range search has no distinct form)")
        if not hasattr(shard, "range_search") or any(isinstance(sh, QuantizedShard) for sh in getattr(shard, "segments", ())):
            raise ValueError("distributed_search: min_score needs a shard with range_search; int8 rows (QuantizedShard) have no range "
                             "search yet")
        if not (isinstance(min_score, (int, float)) and not isinstance(min_score, bool)) and not (
                isinstance(min_score, torch.Tensor) and min_score.dtype == torch.float32):
            raise ValueError("distributed_search: min_score must be a float or an f32 tensor [B_local]")

    def search(q, labels, floors=None):                          # the call forms the docstring promises
        if ranged:
            if query_labels is None:
                return shard.range_search(q, floors, k)
            return shard.range_search(q, floors, k, query_labels=labels, mode=filter_mode)
        if distinct:
            return shard.search(q, k, query_labels=labels, mode=filter_mode, distinct=True)
        return shard.search(q, k) if query_labels is None else shard.search(q, k, query_labels=labels, mode=filter_mode)

    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not always_collective):
        if ranged:
            s, i, c = search(local_queries, query_labels, min_score)
            if defer:                                            # one copy: the packed lists with each query's count behind them
                both, ev = _to_host_async(torch.cat([_pack_lists(s, i).reshape(s.shape[0], -1), c.reshape(-1, 1).to(torch.int32)], dim=1))
                return PendingSearch(lambda: (*_unpack_lists(both[:, :-1].reshape(s.shape + (3,))), both[:, -1].to(torch.int64)), ev)
            return s.cpu(), i.cpu(), c.cpu().to(torch.int64)
        s, i = search(local_queries, query_labels)
        if defer:
            both, ev = _to_host_async(_pack_lists(s, i))         # one copy instead of two
            return PendingSearch(lambda: _unpack_lists(both), ev)
        return s.cpu(), i.cpu()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    q = local_queries.reshape(-1, local_queries.shape[-1]).to(torch.float32).contiguous()
    b_local, C = q.shape
    cap = int(max_local) if max_local is not None else b_local
    if b_local > cap:
        raise ValueError(f"distributed_search: {b_local} local queries exceed max_local={cap}")
    dev = shard.rows.device
    host_coll = dist.get_backend(group) == "gloo"               # CPU rehearsal backend: collectives on host copies
    if host_coll and merge == "device":                          # (the same on every rank: nobody is left waiting in a collective)
        raise ValueError("distributed_search: merge='device' needs a device backend (nccl / RCCL); under gloo the gathered lists are host copies")
    cdev = torch.device("cpu") if host_coll else dev
    fcol = C if query_labels is None else C + 1                   # filtered: column C carries each query's label (int32 bits)
    width = fcol + 1 if ranged else fcol                          # range search: the last column carries each query's floor
    block = torch.zeros((cap + 1, width), dtype=torch.float32, device=cdev)
    block[:b_local, :C] = q.to(cdev)
    if query_labels is not None:
        ql = torch.as_tensor(query_labels).reshape(-1)
        if ql.shape[0] != b_local:
            raise ValueError(f"distributed_search: {ql.shape[0]} query labels for {b_local} local queries")
        block[:b_local, C] = ql.to(cdev, torch.int32).view(torch.float32)
    if ranged:                                                   # padding slots: +inf, no member and no band row (a zero query against a floor
        block[:, fcol].fill_(float("inf"))                       # of 0 would make every row a band row and take the fallback)
        if isinstance(min_score, torch.Tensor):
            if min_score.reshape(-1).shape[0] != b_local:
                raise ValueError(f"distributed_search: {min_score.reshape(-1).shape[0]} floors for {b_local} local queries")
            block[:b_local, fcol] = min_score.reshape(-1).to(cdev)
        else:
            block[:b_local, fcol].fill_(float(min_score))
    block[cap, :1].fill_(float(b_local))                         # (a fill kernel; `block[cap, 0] = x` copies a host scalar: the host would wait for the stream)
    allb = torch.empty((world * (cap + 1), width), dtype=torch.float32, device=cdev)
    marks = _Marks(dev, host_coll) if timing is not None else None
    if marks:
        marks.mark()
    dist.all_gather_into_tensor(allb, block, group=group)        # collective 1 (RCCL over xGMI)
    if marks:
        marks.mark()
    allb = allb.view(world, cap + 1, width)
    slots = allb[:, :cap, :C].reshape(world * cap, C).to(dev)    # every slot is scored; counts stay where they are
    slot_labels = None if query_labels is None else allb[:, :cap, C].contiguous().view(torch.int32).reshape(world * cap).to(dev)
    if ranged:                                                   # [slots, 3 k + 1]: each slot's packed list, then its count
        s, i, c = search(slots, slot_labels, allb[:, :cap, fcol].reshape(world * cap).to(dev))
        packed = torch.cat([_pack_lists(s, i).reshape(world * cap, 3 * k), c.reshape(-1, 1).to(torch.int32)], dim=1)
    else:
        s, i = search(slots, slot_labels)                        # local shard vs ALL query slots
        packed = _pack_lists(s, i)
    if distinct:                                                 # [slots,k,4]: + the entry's group id
        eg = shard.entry_groups(i) if hasattr(shard, "entry_groups") else _entry_groups(shard, i)    # (a GallerySet looks up its segments)
        packed = torch.cat([packed, eg.unsqueeze(-1)], dim=-1)
    packed = packed.to(cdev)
    if marks:
        marks.mark()
    if dst is None:
        parts = torch.empty((world * packed.shape[0],) + tuple(packed.shape[1:]), dtype=torch.int32, device=cdev)
        dist.all_gather_into_tensor(parts, packed, group=group)  # collective 2 (all ranks merge)
        parts = parts.view((world,) + tuple(packed.shape))
        if marks:
            marks.mark(); timing.append(marks)
    else:
        glist = [torch.empty_like(packed) for _ in range(world)] if rank == dst else None
        dist.gather(packed, glist, dst=dist.get_global_rank(group, dst) if group is not None else dst, group=group)   # collective 2
        if marks:
            marks.mark(); timing.append(marks)
        if rank != dst:
            none = (None, None, None) if ranged else (None, None)
            return PendingSearch(value=none) if defer else none
        parts = torch.stack(glist, dim=0)
    # the ONE device-to-host copy: lists of all shards + the per-rank counts (as int32) in one buffer
    counts_i = allb[:, cap, 0].to(torch.int32)
    if merge == "device":
        if ranged:
            return _finish_device_merge(parts[..., :3 * k].reshape(world, world * cap, k, 3), counts_i, k, cap, False, defer, parts[..., 3 * k])
        return _finish_device_merge(parts, counts_i, k, cap, distinct, defer)
    flat = torch.cat([parts.reshape(-1), counts_i.to(parts.device)])
    pshape = tuple(parts.shape)

    def finish(host):
        keep = _kept_slots(host, world, cap)
        lists = host[:-world].view(pshape)
        if ranged:                                               # [world(shard), world*cap(slot), 3 k + 1]
            ps, pi = _unpack_lists(lists[..., :3 * k].reshape(world, world * cap, k, 3))
            return (*merge_topk_host(list(ps[:, keep]), list(pi[:, keep]), k), lists[..., 3 * k].to(torch.int64).sum(0)[keep])
        ps, pi = _unpack_lists(lists[..., :3])                   # [world(shard), world*cap(slot), k]
        if distinct:
            return merge_topk_distinct_host(list(ps[:, keep]), list(pi[:, keep]), list(lists[..., 3][:, keep]), k)
        return merge_topk_host(list(ps[:, keep]), list(pi[:, keep]), k)

    if defer:
        host, ev = _to_host_async(flat)
        return PendingSearch(lambda: finish(host), ev)
    return finish(flat.cpu())


def _kept_slots(host, world, cap):
    """The slots that hold a query, out of the per-rank counts at the end of the host buffer: rank r's first counts[r] of its `cap`."""
    counts = host[-world:].tolist()
    if any(c < 0 or c > cap for c in counts):
        raise RuntimeError(f"distributed_search: inconsistent per-rank query counts {counts} for max_local={cap}")
    return torch.cat([torch.arange(r * cap, r * cap + counts[r]) for r in range(world)])


def _finish_device_merge(parts, counts_i, k, cap, distinct, defer, members=None):
    """distributed_search(merge="device") on a merging rank: parts int32 [world, slots, k, 3|4] (the gathered packed lists, on the GPU) are
    merged there for every slot; ONE copy takes [slots, k] indices and scores and the per-rank counts (all as int32) to the host.
    members (a range search): int32 [world, slots], every shard's member count per slot; their int64 sums over the shards ride in the same
    copy and the result gains them as a third tensor."""
    world, slots, n = parts.shape[0], parts.shape[1], parts.shape[1] * k
    ps, pi = _unpack_lists(parts[..., :3])
    with torch.cuda.device(parts.device):
        ms, mi, _ = _merge_stacked(ps, pi, parts[..., 3].contiguous() if distinct else None, k)
    total = [] if members is None else [members.to(torch.int64).sum(0).view(torch.int32).reshape(-1)]
    m = 2 * slots if total else 0                                # (the 8-byte indices and sums first: aligned)
    flat = torch.cat([mi.view(torch.int32).reshape(-1), *total, ms.view(torch.int32).reshape(-1), counts_i.to(parts.device)])

    def finish(host):
        keep = _kept_slots(host, world, cap)
        lists = host[2 * n + m:3 * n + m].view(torch.float32).view(-1, k)[keep], host[:2 * n].view(torch.int64).view(-1, k)[keep]
        return lists if members is None else (*lists, host[2 * n:2 * n + m].view(torch.int64)[keep])

    if defer:
        host, ev = _to_host_async(flat)
        return PendingSearch(lambda: finish(host), ev)
    return finish(flat.cpu())


@torch.no_grad()
def build_gallery(model, batches, dtype=torch.float16):
    """Offline gallery builder: SAM image encoder over gallery images + region mask pooling
    (utils/loss_func.py:35-56) -> unit-norm rows [G, 256] in `dtype`, in input order.
    `batches` yields dicts with "query_img" f32[B,3,1024,1024] and "query_mask" f32[B,1,h,w] (the reference's loader
    field names, utils/dataloader.py:244-369). Only the encoder half of the forward runs (engine.sam_encoder)."""
    from . import engine
    rows = []
    T = model._resolve_dtype()
    W = model.packed(T)
    cfg = model.image_encoder.cfg
    g = cfg["img"] // cfg["patch"]
    for b in batches:
        img = b["query_img"].to(model.device, torch.float32).contiguous()
        B = img.shape[0]
        tok = engine.sam_encoder(W, img, cfg, T)                                       # [B*g*g, 256] fp32 tokens
        m = b["query_mask"].to(model.device, torch.float32).contiguous()
        if tuple(m.shape[-2:]) != (g, g):
            m = ops.bilinear(m, g, g)
        # tokens are channels-last: pool them directly (feat_nchw=False), clamp + L2-normalise as mask_pooling does
        rows.append(ops.masked_pool(tok, m, B, g * g, cfg["out"], feat_nchw=False, clamp01=True, l2norm=True).to(dtype))
    return torch.cat(rows, dim=0)


@torch.no_grad()
def build_gallery_regions(model, batches, dtype=torch.float16):
    """Multi-region gallery builder: every image goes through the SAM image encoder ONCE, all of its region masks are pooled against
    its tokens in one launch (ops.region_pool) -> (rows [sum R, 256] unit-norm in `dtype`, groups int32[sum R]: the image id of each
    row), ready for GalleryShard(rows, groups=groups) / save_gallery(path, rows, world, groups=groups) / search(distinct=True).
    `batches` yields dicts with "query_img" f32[B,3,1024,1024], "region_masks" f32[R,1,h,w] and "region_offsets" int[B+1] (host or
    device; CSR: regions [off[b], off[b+1]) belong to image b, an image may have none), optionally "image_ids" int[B] (global ids of
    the batch's images; default: a running count of the images seen) and "row_index" int[R] (the position of each region's row in the
    finished gallery; default: arrival order). A row_index that is not a permutation of 0 .. sum R - 1 raises ValueError.
    dataloader.gallery_region_batches yields such batches from the reference's CSV, with row_index = the CSV row. A row has the
    arithmetic of build_gallery's (the pooling is bit-identical given the same tokens)."""
    from . import engine
    T = model._resolve_dtype()
    W = model.packed(T)
    cfg = model.image_encoder.cfg
    g = cfg["img"] // cfg["patch"]
    rows, groups, index, seen, indexed = [], [], [], 0, None
    for b in batches:
        img = b["query_img"].to(model.device, torch.float32).contiguous()
        B = img.shape[0]
        off = torch.as_tensor(b["region_offsets"]).reshape(-1)
        off_host = off.cpu().to(torch.int64)
        m = b["region_masks"].to(model.device, torch.float32).contiguous()
        R = m.shape[0]
        if off_host.shape[0] != B + 1 or int(off_host[0]) != 0 or int(off_host[-1]) != R or bool((off_host[1:] < off_host[:-1]).any()):
            raise ValueError(f"build_gallery_regions: region_offsets {off_host.tolist()} do not describe {R} regions of {B} images")
        ids = torch.as_tensor(b["image_ids"]).reshape(-1).cpu().to(torch.int64) if b.get("image_ids") is not None \
            else torch.arange(seen, seen + B, dtype=torch.int64)
        if ids.shape[0] != B:
            raise ValueError(f"build_gallery_regions: {ids.shape[0]} image ids for {B} images")
        seen += B
        has_index = b.get("row_index") is not None
        if indexed is not None and has_index != indexed:
            raise ValueError("build_gallery_regions: row_index must be given by every batch or by none")
        indexed = has_index
        if indexed:
            ri = torch.as_tensor(b["row_index"]).reshape(-1).cpu().to(torch.int64)
            if ri.shape[0] != R:
                raise ValueError(f"build_gallery_regions: {ri.shape[0]} row indices for {R} regions")
            index.append(ri)
        groups.append(torch.repeat_interleave(ids, off_host[1:] - off_host[:-1]).to(torch.int32))
        tok = engine.sam_encoder(W, img, cfg, T)                                       # [B*g*g, 256] fp32 tokens, once per image
        if R and tuple(m.shape[-2:]) != (g, g):
            m = ops.bilinear(m, g, g)
        rows.append(ops.region_pool(tok, m.reshape(R, g * g), off.to(model.device, torch.int32).contiguous(), B, g * g, cfg["out"],
                                    out_dtype=dtype, clamp01=True, l2norm=True))
    if not rows:
        return torch.empty((0, cfg["out"]), dtype=dtype, device=model.device), torch.empty((0,), dtype=torch.int32)
    rows, groups = torch.cat(rows, dim=0), torch.cat(groups)
    if indexed:
        index = torch.cat(index)
        n = rows.shape[0]
        if index.shape[0] != n or not torch.equal(torch.sort(index).values, torch.arange(n, dtype=torch.int64)):
            raise ValueError(f"build_gallery_regions: row_index is not a permutation of 0..{n - 1}")
        inv = torch.empty(n, dtype=torch.int64)
        inv[index] = torch.arange(n, dtype=torch.int64)        # finished[index[j]] = arrival[j]
        rows, groups = rows[inv.to(rows.device)], groups[inv]
    return rows, groups


def save_gallery(path, rows, world=1, labels=None, groups=None, scales=None):
    """On-disk format: <path>.shardNN.pt (rows of shard NN as a tensor) + <path>.manifest.json (row ranges). labels (int32[n], one
    per row): also <path>.shardNN.labels.pt per shard and "labels": true in the manifest; groups (int32[n], one group id per row):
    <path>.shardNN.groups.pt and "groups": true likewise. scales (float32[n], with int8 rows: a quantised gallery, QuantizedShard.rows /
    .scales): <path>.shardNN.scales.pt and "scales": true, and load_gallery_shard returns a QuantizedShard. Without scales the files and
    the manifest are as they always were."""
    import json
    n = rows.shape[0]
    if scales is not None:
        if rows.dtype != torch.int8:
            raise ValueError(f"save_gallery: scales go with int8 rows, got {rows.dtype}")
        scales = torch.as_tensor(scales).reshape(-1).to(torch.float32).cpu()
        if scales.shape[0] != n:
            raise ValueError(f"save_gallery: {scales.shape[0]} scales for {n} rows")
    ids = {}                                                     # "labels" / "groups" -> int32[n] on the host, those that were given
    for name, what, t in (("labels", "labels", labels), ("groups", "group ids", groups)):
        if t is not None:
            ids[name] = torch.as_tensor(t).reshape(-1).to(torch.int32).cpu()
            if ids[name].shape[0] != n:
                raise ValueError(f"save_gallery: {ids[name].shape[0]} {what} for {n} rows")
    shards = []
    for r in range(world):
        lo, hi = shard_bounds(n, world, r)
        torch.save(rows[lo:hi].cpu().contiguous(), f"{path}.shard{r:02d}.pt")
        shards.append(dict(rank=r, lo=lo, hi=hi, file=f"{path}.shard{r:02d}.pt"))
        for name, t in ids.items():
            torch.save(t[lo:hi].clone(), f"{path}.shard{r:02d}.{name}.pt")
            shards[-1][f"{name}_file"] = f"{path}.shard{r:02d}.{name}.pt"
        if scales is not None:
            torch.save(scales[lo:hi].clone(), f"{path}.shard{r:02d}.scales.pt")
            shards[-1]["scales_file"] = f"{path}.shard{r:02d}.scales.pt"
    man = dict(rows=n, dim=int(rows.shape[1]), dtype=str(rows.dtype), world=world, labels="labels" in ids, groups="groups" in ids, shards=shards)
    if scales is not None:
        man["scales"] = True
    with open(f"{path}.manifest.json", "w") as f:
        json.dump(man, f, indent=1)


def load_gallery_shard(path, rank, device):
    import json
    man = json.load(open(f"{path}.manifest.json"))
    sh = man["shards"][rank]
    labels = torch.load(sh["labels_file"]) if man.get("labels") else None
    groups = torch.load(sh["groups_file"]) if man.get("groups") else None
    if man.get("scales"):
        return QuantizedShard(torch.load(sh["file"]).to(device), torch.load(sh["scales_file"]).to(device), offset=sh["lo"], labels=labels,
                              groups=groups)
    return GalleryShard(torch.load(sh["file"]).to(device), offset=sh["lo"], labels=labels, groups=groups)
