"""Wide-k gallery top-k (33 <= k <= 256, include/cor_amd.h COR_TOPK_KMAX): Recall@50/100 and two-stage re-ranking.

Every wide-k call is held BITWISE (scores and indices, ties included, zero excused positions) to the CPU fmaf-chain oracle
(oracle/c/sim_chain.c via oracle.retrieval.similarity_topk_chain), for fp32, bf16 and fp16 galleries and for any C."""
import numpy as np
import pytest
import torch

from oracle import retrieval as oret

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def _ops():
    from cor_amd import ops, _native as nat
    return ops, nat


def _unit(rng, n, C):
    return torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((n, C), dtype=np.float32)), dim=-1)


def _data(Bq, Ng, gdt, C=256, seed=0):
    """unit queries and gallery rows with planted duplicates: a tie inside a tile, and three copies across slices and in the ragged
    last tile"""
    rng = np.random.default_rng(Bq + Ng + C + seed)
    Q = _unit(rng, Bq, C)
    G = _unit(rng, Ng, C).to(gdt)
    G[5] = G[3]
    if Ng > 300:
        G[Ng - 1] = G[17]; G[Ng - 200] = G[17]
    return Q, G


def _oracle(Q, G, k, margin=2e-4):
    Qr = Q if G.dtype == F32 else Q.to(G.dtype).float()
    return oret.similarity_topk_chain(Qr, G.float(), k, margin=margin)


def _assert_bitwise(s, i, rs, ri, g_offset, k, Ng):
    kk = min(k, Ng)
    s, i = s.cpu(), i.cpu()
    mism = int((i[:, :kk] - g_offset != ri).sum())
    bits = int((s[:, :kk].view(torch.int32) != rs.view(torch.int32)).sum())
    assert mism == 0, f"{mism} of {ri.numel()} top-k indices differ from the chain oracle"
    assert bits == 0, f"{bits} of {ri.numel()} scores are not bit-identical to the chain oracle"
    if k > Ng:
        assert (i[:, Ng:] == -1).all() and torch.isneginf(s[:, Ng:]).all()


WIDE_CASES = [(32, 100000, 50), (32, 100000, 100), (512, 12500, 100), (512, 125000, 100), (300, 70001, 256), (64, 4097, 33),
              (257, 4096, 64), (7, 200, 256)]
WIDE_PARAMS = [(Bq, Ng, k, g) for (Bq, Ng, k) in WIDE_CASES for g in (F32, BF16, F16)] + [(512, 1000000, 100, BF16), (512, 1000000, 100, F16)]


@pytest.mark.parametrize("Bq,Ng,k,gdt", WIDE_PARAMS)
def test_wide_topk_bitwise_vs_chain_oracle(Bq, Ng, k, gdt):
    ops, nat = _ops()
    Q, G = _data(Bq, Ng, gdt)
    s, i = ops.similarity_topk(Q.to(DEV), G.to(DEV), k, g_offset=1000)
    rs, ri = _oracle(Q, G, k)
    _assert_bitwise(s, i, rs, ri, 1000, k, Ng)
    # random data stays off the overflow path (it would be exact too, but slow)
    _, raw = ops.similarity_topk(Q.to(DEV), G.to(DEV), k, g_offset=1000, flags=nat.TOPK_NO_FALLBACK)
    assert int((raw == -2).any(dim=1).sum()) == 0


@pytest.mark.parametrize("C", [128, 64])
@pytest.mark.parametrize("Bq,Ng", [(64, 20000), (33, 3001)])
@pytest.mark.parametrize("gdt", [F32, BF16, F16])
def test_wide_topk_any_C_bitwise_vs_chain_oracle(C, Bq, Ng, gdt):
    """C != 256: the tile kernels scan; 16-bit scores are re-scored with the chain over C / 8 chunks, so (unlike k <= 32) the result
    is bitwise the chain oracle's for the 16-bit dtypes too."""
    ops, _ = _ops()
    k = 64
    Q, G = _data(Bq, Ng, gdt, C=C)
    s, i = ops.similarity_topk(Q.to(DEV), G.to(DEV), k, g_offset=1000)
    rs, ri = _oracle(Q, G, k)
    _assert_bitwise(s, i, rs, ri, 1000, k, Ng)


@pytest.mark.parametrize("C,gdt,Bq,Ng", [(256, BF16, 300, 20011), (256, F16, 64, 40000), (256, F32, 64, 20011), (128, F32, 33, 5000),
                                         (256, BF16, 512, 4000)])
def test_wide_topk_prefix_equals_the_k32_call(C, gdt, Bq, Ng):
    """Across the boundary: the first 32 entries of a k = 33 and of a k = 256 call equal a k = 32 call (different kernels) bit for
    bit, where k <= 32 is already bitwise (16-bit with C = 256, fp32 with any C)."""
    ops, _ = _ops()
    Q, G = _data(Bq, Ng, gdt, C=C, seed=1)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    s32, i32 = ops.similarity_topk(Qd, Gd, 32, g_offset=9)
    for k in (33, 256):
        s, i = ops.similarity_topk(Qd, Gd, k, g_offset=9)
        assert torch.equal(i[:, :32], i32), k
        assert torch.equal(s[:, :32].view(torch.int32), s32.view(torch.int32)), k


# (gdt, C, queries, rows): the record (scan-form) selection kernel, then the entry-list (tile-form) one for fp32 and for C != 256
OVERFLOW_CASES = [(BF16, 256, 40, 60000), (F32, 256, 16, 20000), (F16, 128, 16, 20000)]


@pytest.mark.parametrize("gdt,C,nq,Ng", OVERFLOW_CASES, ids=["bf16-256", "f32-256", "f16-128"])
def test_wide_topk_overflow_falls_back_on_the_device(gdt, C, nq, Ng):
    """A slice of 3000 identical rows close to query 0 ties far more rows than the short list holds at k = 100: the query overflows,
    is flagged (COR_TOPK_NO_FALLBACK: -2 in every slot) and, by default, ranked exactly inside the selection kernel (radix select over
    the chain scores of the whole shard, the first k tied rows in index order). The other queries are exact either way."""
    ops, nat = _ops()
    k = 100
    rng = np.random.default_rng(5)
    Q = _unit(rng, nq, C)
    row = _unit(rng, 1, C)
    G = _unit(rng, Ng, C)
    G[10000:13000] = torch.nn.functional.normalize(Q[0:1] + 0.05 * row, dim=-1)
    G = G.to(gdt)
    s, i = ops.similarity_topk(Q.to(DEV), G.to(DEV), k)
    _, raw = ops.similarity_topk(Q.to(DEV), G.to(DEV), k, flags=nat.TOPK_NO_FALLBACK)
    flagged = (raw == -2).all(dim=1).cpu()
    assert bool(flagged[0]) and int(flagged.sum()) < nq, flagged
    assert bool(((raw == -2).any(dim=1).cpu() == flagged).all())
    assert torch.equal(i[0].cpu(), torch.arange(10000, 10000 + k))
    assert torch.equal(raw[~flagged.to(DEV)], i[~flagged.to(DEV)])
    rs, ri = _oracle(Q, G, k, margin=1e-3)
    _assert_bitwise(s, i, rs, ri, 0, k, G.shape[0])
    # every row identical: every query overflows; the answer is the first k rows, all with the same score
    G1 = row.repeat(20000, 1).to(gdt)
    s1, i1 = ops.similarity_topk(Q.to(DEV), G1.to(DEV), k)
    assert torch.equal(i1.cpu(), torch.arange(k).repeat(nq, 1))
    _, raw1 = ops.similarity_topk(Q.to(DEV), G1.to(DEV), k, flags=nat.TOPK_NO_FALLBACK)
    assert (raw1 == -2).all()
    rs1, _ = _oracle(Q, G1, k, margin=1e-3)
    assert torch.equal(s1.cpu().view(torch.int32), rs1.view(torch.int32))


@pytest.mark.parametrize("gdt,C", [(BF16, 256), (F32, 256), (F16, 128)])
def test_wide_topk_is_deterministic(gdt, C):
    ops, _ = _ops()
    Q, G = _data(512, 125000, gdt, C=C, seed=2)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    s1, i1 = ops.similarity_topk(Qd, Gd, 100)
    s2, i2 = ops.similarity_topk(Qd, Gd, 100)
    assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))


def test_wide_topk_limits_and_flags():
    """k > 256 is refused (ENOSUPPORT from the search, EINVAL from the workspace query); the register-list and one-wave A/B flags
    are k <= 32 only; ops refuses a bad k before any launch."""
    ops, nat = _ops()
    lib = nat.load()
    Q, G = _data(8, 5000, BF16, seed=3)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    assert lib.cor_topk_workspace_bytes(8, 5000, 257) == nat.EINVAL
    assert lib.cor_topk_workspace_bytes(8, 5000, 256) > 0 and lib.cor_topk_workspace_bytes(8, 5000, 40) > 0
    nb = max(lib.cor_topk_workspace_bytes(8, 5000, 256), lib.cor_topk_workspace_bytes(8, 5000, 40))
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    out_s = torch.empty((8, 257), dtype=torch.float32, device=DEV)
    out_i = torch.empty((8, 257), dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(k, flags):
        return lib.cor_similarity_topk(Qd.data_ptr(), Gd.data_ptr(), nat.BF16, 8, 5000, 256, k, 0, out_s.data_ptr(), out_i.data_ptr(),
                                       ws.data_ptr(), flags, stream)
    assert call(257, 0) == nat.ENOSUPPORT
    assert call(40, nat.TOPK_FORCE_LISTS) == nat.ENOSUPPORT
    assert call(40, nat.TOPK_WAVE_FINAL) == nat.ENOSUPPORT
    assert call(40, 0) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.similarity_topk(Qd, Gd, 257)
    with pytest.raises(ValueError):
        ops.similarity_topk(Qd, Gd, 0)
    with pytest.raises(nat.NativeError):
        ops.similarity_topk(Qd, Gd, 40, flags=nat.TOPK_FORCE_LISTS)
    # COR_TOPK_FORCE_GLOBAL_THRESHOLD is a no-op for wide k
    s, i = ops.similarity_topk(Qd, Gd, 40)
    s2, i2 = ops.similarity_topk(Qd, Gd, 40, flags=nat.TOPK_FORCE_GLOBAL_THRESHOLD)
    assert torch.equal(i, i2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))


def test_wide_topk_public_layer_and_one_rank_rccl_group():
    """GalleryShard.search(q, 100) is ops.similarity_topk with the shard's offset; distributed_search at k = 100 on a one-rank nccl
    group (always_collective, gather and deferred forms) returns the same lists."""
    import socket
    import torch.distributed as dist
    from cor_amd import ops, retrieval
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    k = 100
    Q, G = _data(5, 12500, BF16, seed=4)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    shard = retrieval.GalleryShard(Gd, offset=100)
    s0, i0 = shard.search(Qd, k)
    sd, id_ = ops.similarity_topk(Qd, Gd, k, g_offset=100)
    assert torch.equal(i0, id_) and torch.equal(s0.view(torch.int32), sd.view(torch.int32))
    rs, ri = _oracle(Q, G, k)
    _assert_bitwise(s0, i0, rs, ri, 100, k, G.shape[0])
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        s1, i1 = retrieval.distributed_search(Qd, shard, k, max_local=8, always_collective=True)
        pend = retrieval.distributed_search(Qd, shard, k, max_local=8, always_collective=True, defer=True)
        s2, i2 = pend.result()
        torch.cuda.synchronize()
        for s_, i_ in ((s1, i1), (s2, i2)):
            assert torch.equal(i_, i0.cpu()) and torch.equal(s_.view(torch.int32), s0.cpu().view(torch.int32))
    finally:
        dist.destroy_process_group()
