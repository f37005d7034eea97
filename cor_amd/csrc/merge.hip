// cor_amd — device merge of top-k lists (cor_merge_topk): P lists of kin (score, global index[, group id]) entries per query
// -> the k best by (score desc, index asc), optionally one entry per non-negative group id. Contract: include/cor_amd.h.
//
// One block per query, ranklist.h's scheme. The n = P*kin entries become rank keys in LDS (no -0.0 flag: the scores are read back through
// the position) and the bitonic network ranks them, ties by the 64-bit global index (MergeBefore below).
// Distinct: the ranked entries are keyed [group id | rank] and sorted a second time, the first entry of every run of equal group
// ids is its group's best (a negative id is kept without taking part), and the keep scan in rank order places the first k
// survivors: what retrieval.merge_topk_distinct_host does with five host sorts.
// LDS: 8 B per key (plain), + 2 B position and 1 B keep flag per rank (distinct): <= 44 KB at n = 4096; the 16-B records stay in
// global memory and only the k winners are gathered.
#include "ranklist.h"

namespace {

struct MergeLists {
  const unsigned* scores;
  const long long* idx;
  const int* groups;
  long long qoff, lstride;   // entry e of list p of this block's query: p * lstride + qoff + e
  int kin;
  __device__ __forceinline__ long long at(unsigned pos) const {
    const unsigned p = pos / (unsigned)kin;
    return (long long)p * lstride + qoff + (pos - p * (unsigned)kin);
  }
};

// ranklist.h's tie rule in this kernel's own copy, in the form the file had before ranklist.h: with RankBefore the kernel had one more
// instruction and another block layout in the tie path, and 8 lists of 256 merged 1.8 % (plain) and 0.6 % (distinct) slower, beyond the
// run-to-run spread (profiles/list_kernels_refactor_disasm.txt). BY_INDEX false: plain <, for the sort by group id.
template <bool BY_INDEX> struct MergeBefore {
  const MergeLists& L;
  __device__ __forceinline__ bool operator()(u64 a, u64 b) const {
    if (BY_INDEX) {
      const unsigned ha = (unsigned)(a >> 32), hb = (unsigned)(b >> 32);
      if (ha == hb && ha != RANK_MISSING) {      // a tie between two PRESENT entries: positions < n, indices >= 0
        const long long ia = L.idx[L.at((unsigned)a & RANK_POS_MASK)], ib = L.idx[L.at((unsigned)b & RANK_POS_MASK)];
        if (ia != ib) return ia < ib;
      }
    }
    return a < b;
  }
};

__global__ __launch_bounds__(1024) void merge_topk_kernel(const unsigned* __restrict__ scores, const long long* __restrict__ idx,
                                                          const int* __restrict__ groups, int Bq, int kin, int n, int npad, int k,
                                                          unsigned* __restrict__ out_scores, long long* __restrict__ out_idx,
                                                          int* __restrict__ out_groups) {
  extern __shared__ __align__(16) unsigned char merge_lds[];
  __shared__ int s_present, s_wsum[16];
  u64* key = (u64*)merge_lds;
  const int tid = threadIdx.x, T = blockDim.x;
  const long long out0 = (long long)blockIdx.x * k;
  MergeLists L{scores, idx, groups, (long long)blockIdx.x * kin, (long long)Bq * kin, kin};

  if (tid == 0) s_present = 0;
  __syncthreads();
  int mine = 0;
  for (int pos = tid; pos < npad; pos += T) {
    unsigned hi = RANK_MISSING;
    if (pos < n) {
      const long long at = L.at(pos);
      if (idx[at] >= 0) hi = rank_score_key(scores[at]);
    }
    mine += hi != RANK_MISSING;                  // counted by the KEY: the first `present` ranks are exactly the keys below MISSING
    key[pos] = ((u64)hi << 32) | (unsigned)pos;
  }
  if (mine) atomicAdd(&s_present, mine);
  __syncthreads();
  block_bitonic_sort(key, npad, MergeBefore<true>{L});
  const int present = s_present;

  if (groups == nullptr) {
    for (int r = tid; r < k; r += T) {
      if (r < present) {
        const long long at = L.at((unsigned)key[r] & RANK_POS_MASK);
        out_scores[out0 + r] = scores[at];
        out_idx[out0 + r] = idx[at];
      } else {
        out_scores[out0 + r] = RANK_NEG_INF;
        out_idx[out0 + r] = -1;
      }
      if (out_groups) out_groups[out0 + r] = -1;
    }
    return;
  }

  unsigned short* posr = (unsigned short*)(merge_lds + 8 * (size_t)npad);   // rank -> position
  unsigned char* keep = merge_lds + 10 * (size_t)npad;                      // rank -> survives
  for (int r = tid; r < npad; r += T) {          // every thread rewrites only the keys it has just read
    const unsigned pos = (unsigned)key[r] & RANK_POS_MASK;
    unsigned hi = RANK_MISSING;                  // missing entries, padding and negative ids stay out of the group runs
    unsigned char kp = 0;
    if (r < present) {
      const int g = groups[L.at(pos)];
      if (g >= 0) hi = (unsigned)g; else kp = 1;
    }
    posr[r] = (unsigned short)pos;
    keep[r] = kp;
    key[r] = ((u64)hi << 32) | (unsigned)r;
  }
  __syncthreads();
  block_bitonic_sort(key, npad, MergeBefore<false>{L});
  for (int j = tid; j < npad; j += T) {
    const u64 kj = key[j];
    const unsigned hi = (unsigned)(kj >> 32);
    if (hi != RANK_MISSING && (j == 0 || (unsigned)(key[j - 1] >> 32) != hi)) keep[(unsigned)kj & RANK_POS_MASK] = 1;
  }
  __syncthreads();

  const KeepScan sc = rank_keep_scan(keep, npad, s_wsum);
  int o = sc.slot;
  for (int r = sc.lo; r < sc.hi && o < k; ++r)
    if (keep[r]) {
      const long long at = L.at(posr[r]);
      out_scores[out0 + o] = scores[at];
      out_idx[out0 + o] = idx[at];
      if (out_groups) out_groups[out0 + o] = groups[at];
      ++o;
    }
  rank_fill_tail(sc.total, k, out0, out_scores, out_idx, out_groups);
}

int merge_shape_check(int P, int Bq, int kin, int k) {
  if (P < 1 || Bq < 0 || kin < 1 || k < 1 || k > COR_TOPK_KMAX) return COR_EINVAL;
  if ((long)P * kin > COR_MERGE_NMAX) return COR_ENOSUPPORT;
  return 0;
}

}  // namespace

extern "C" long cor_merge_topk_workspace_bytes(int P, int Bq, int kin, int k) { return merge_shape_check(P, Bq, kin, k); }

extern "C" int cor_merge_topk(const float* scores, const long long* idx, const int* groups, int P, int Bq, int kin, int k, float* out_scores,
                              long long* out_idx, int* out_groups, void* workspace, void* stream) {
  (void)workspace;
  if (!scores || !idx || !out_scores || !out_idx) return COR_EINVAL;
  const int rc = merge_shape_check(P, Bq, kin, k);
  if (rc) return rc;
  if (Bq == 0) return 0;
  const int n = P * kin;
  const int npad = next_pow2(n);
  const int threads = npad / 2 < 64 ? 64 : (npad / 2 > 1024 ? 1024 : npad / 2);
  const size_t lds = (size_t)npad * (groups ? 11 : 8);
  hipLaunchKernelGGL(merge_topk_kernel, dim3((unsigned)Bq), dim3(threads), lds, (hipStream_t)stream, (const unsigned*)scores, idx, groups, Bq,
                     kin, n, npad, k, (unsigned*)out_scores, out_idx, out_groups);
  COR_CHECK_LAUNCH();
  return 0;
}
