// cor_amd — device merge of top-k lists (cor_merge_topk): P lists of kin (score, global index[, group id]) entries per query
// -> the k best by (score desc, index asc), optionally one entry per non-negative group id. Contract: include/cor_amd.h.
//
// One block per query. The n = P*kin entries become 64-bit sort keys in LDS: [order-preserving score key, descending | position in
// the concatenated lists]; a missing entry (index < 0) and the padding up to the next power of two carry the largest score key, so
// they sort behind every present entry and nothing is ever indexed with a missing entry's index or group value. A bitonic network
// ranks the keys; equal score keys are decided by the 64-bit global index, read through the position (only then: for scores of
// distinct rows ties are rare, and the lists of one query are a few KB that stay in cache), then by the position.
// Distinct: the ranked entries are keyed [group id | rank] and sorted a second time, the first entry of every run of equal group
// ids is its group's best (a negative id is kept without taking part), and a block scan over the keep flags in rank order places
// the first k survivors: what retrieval.merge_topk_distinct_host does with five host sorts.
// LDS: 8 B per key (plain), + 2 B position and 1 B keep flag per rank (distinct): <= 44 KB at n = 4096; the 16-B records stay in
// global memory and only the k winners are gathered.
#include "common.h"

namespace {

constexpr int MERGE_NMAX = COR_MERGE_NMAX;     // entries per query in one launch: 4096 = 12 position bits in the key
static_assert(MERGE_NMAX == 4096, "the sort keys carry 12 position bits and the rank -> position table is 16-bit");
constexpr unsigned MERGE_POS_MASK = MERGE_NMAX - 1;
constexpr unsigned MERGE_MISSING = 0xffffffffu;   // score key of missing entries and padding: above every non-NaN score's key
constexpr unsigned MERGE_NEG_INF = 0xff800000u;

typedef unsigned long long u64;

// float bits -> key that ascends as the score DEscends; -0.0 keys as +0.0 (for the key only: the output copies the input bits)
__device__ __forceinline__ unsigned merge_score_key(unsigned u) {
  if (u == 0x80000000u) u = 0u;
  const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

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

template <bool BY_INDEX> __device__ __forceinline__ bool merge_before(u64 a, u64 b, const MergeLists& L) {
  if (BY_INDEX) {
    const unsigned ha = (unsigned)(a >> 32), hb = (unsigned)(b >> 32);
    if (ha == hb && ha != MERGE_MISSING) {       // a tie between two PRESENT entries: positions < n, indices >= 0
      const long long ia = L.idx[L.at((unsigned)a & MERGE_POS_MASK)], ib = L.idx[L.at((unsigned)b & MERGE_POS_MASK)];
      if (ia != ib) return ia < ib;
    }
  }
  return a < b;
}

// ascending bitonic sort of key[0, npad) (npad a power of two >= 2); ends with a barrier
template <bool BY_INDEX> __device__ void merge_sort(u64* key, int npad, const MergeLists& L) {
  const int half = npad >> 1;
  for (int size = 2; size <= npad; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < half; t += blockDim.x) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const u64 a = key[i], b = key[j];
        if (merge_before<BY_INDEX>(b, a, L) == ((i & size) == 0)) { key[i] = b; key[j] = a; }
      }
      __syncthreads();
    }
}

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
    unsigned hi = MERGE_MISSING;
    if (pos < n) {
      const long long at = L.at(pos);
      if (idx[at] >= 0) hi = merge_score_key(scores[at]);
    }
    mine += hi != MERGE_MISSING;                 // counted by the KEY: the first `present` ranks are exactly the keys below MISSING
    key[pos] = ((u64)hi << 32) | (unsigned)pos;
  }
  if (mine) atomicAdd(&s_present, mine);
  __syncthreads();
  merge_sort<true>(key, npad, L);
  const int present = s_present;

  if (groups == nullptr) {
    for (int r = tid; r < k; r += T) {
      if (r < present) {
        const long long at = L.at((unsigned)key[r] & MERGE_POS_MASK);
        out_scores[out0 + r] = scores[at];
        out_idx[out0 + r] = idx[at];
      } else {
        out_scores[out0 + r] = MERGE_NEG_INF;
        out_idx[out0 + r] = -1;
      }
      if (out_groups) out_groups[out0 + r] = -1;
    }
    return;
  }

  unsigned short* posr = (unsigned short*)(merge_lds + 8 * (size_t)npad);   // rank -> position
  unsigned char* keep = merge_lds + 10 * (size_t)npad;                      // rank -> survives
  for (int r = tid; r < npad; r += T) {          // every thread rewrites only the keys it has just read
    const unsigned pos = (unsigned)key[r] & MERGE_POS_MASK;
    unsigned hi = MERGE_MISSING;                 // missing entries, padding and negative ids stay out of the group runs
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
  merge_sort<false>(key, npad, L);
  for (int j = tid; j < npad; j += T) {
    const u64 kj = key[j];
    const unsigned hi = (unsigned)(kj >> 32);
    if (hi != MERGE_MISSING && (j == 0 || (unsigned)(key[j - 1] >> 32) != hi)) keep[(unsigned)kj & MERGE_POS_MASK] = 1;
  }
  __syncthreads();

  // exclusive scan of the keep flags in rank order: thread t owns ranks [t*chunk, (t+1)*chunk)
  const int chunk = (npad + T - 1) / T, lo = min(tid * chunk, npad), hi_r = min(lo + chunk, npad);
  int cnt = 0;
  for (int r = lo; r < hi_r; ++r) cnt += keep[r];
  const int lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) s_wsum[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < nwaves; ++w) {
    const int v = s_wsum[w];
    if (w < wave) before += v;
    total += v;
  }
  int o = before + incl - cnt;
  for (int r = lo; r < hi_r && o < k; ++r)
    if (keep[r]) {
      const long long at = L.at(posr[r]);
      out_scores[out0 + o] = scores[at];
      out_idx[out0 + o] = idx[at];
      if (out_groups) out_groups[out0 + o] = groups[at];
      ++o;
    }
  for (int t = min(total, k) + tid; t < k; t += T) {
    out_scores[out0 + t] = MERGE_NEG_INF;
    out_idx[out0 + t] = -1;
    if (out_groups) out_groups[out0 + t] = -1;
  }
}

int merge_shape_check(int P, int Bq, int kin, int k) {
  if (P < 1 || Bq < 0 || kin < 1 || k < 1 || k > COR_TOPK_KMAX) return COR_EINVAL;
  if ((long)P * kin > MERGE_NMAX) return COR_ENOSUPPORT;
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
  int npad = 2;
  while (npad < n) npad <<= 1;
  const int threads = npad / 2 < 64 ? 64 : (npad / 2 > 1024 ? 1024 : npad / 2);
  const size_t lds = (size_t)npad * (groups ? 11 : 8);
  hipLaunchKernelGGL(merge_topk_kernel, dim3((unsigned)Bq), dim3(threads), lds, (hipStream_t)stream, (const unsigned*)scores, idx, groups, Bq,
                     kin, n, npad, k, (unsigned*)out_scores, out_idx, out_groups);
  COR_CHECK_LAUNCH();
  return 0;
}
