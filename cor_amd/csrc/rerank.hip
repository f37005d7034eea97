// cor_amd — k-reciprocal re-ranking, set form (cor_knn_reciprocal, cor_rerank_reciprocal): a neighbour graph pruned to its reciprocal
// edges, and per query a list of kin (score, id) entries re-ordered by lam * score + (1 - lam) * Jaccard(query's k-reciprocal set, the
// candidate's reciprocal neighbours). Contract and the definition, fixed to the bit: include/cor_amd.h.
//
// cor_knn_reciprocal: one thread per edge (g, j) of one segment. h = nbr[g, j] is tested against every segment's [offset, offset + n)
//   by ranklist.h's seg_lookup, and only a hit forms the address of h's list; the thread walks
//   h's k1 ids until it meets g's global id. Output to a buffer of its own.
// cor_rerank_reciprocal: one block per query, T = npad threads (64 .. 1024; npad = kin rounded up to a power of two), three phases.
//   1. A. Thread j < k1 tests entry j's id against the segment table and, if it is present and scores[j] >= kth[id], puts the id into
//      A (LDS, at most 256 ids; the other slots hold INT64_MAX); a bitonic network sorts A ascending; |A| is counted beside it.
//   2. Jaccard. Thread-per-candidate: the threads take the positions t, t + T, ..; a present candidate's rnbr row is read straight
//      from global memory, 8 ids at a time with 16-byte loads when the rows are 16-byte aligned (kg even), and every non-negative id
//      is looked up in the sorted A by binary search (at most 8 steps). I and |B| are counted in integers; J and f are five separately
//      rounded fp32 operations (`#pragma clang fp contract(off)` for the file, plain `/`, no fast-math flag in the Makefile).
//   3. Rank. ranklist.h's keys (of f, with the -0.0 flag), network and tie rule. The present entries' ids are pairwise different
//      (precondition), so rank r goes to output slot r without a scan; f's bits come back out of the key.
// LDS: 8 B per key + 2 KiB for A + 2 counters = 34 KiB at kin = 4096, all in the dynamic region; no scratch memory in global.
#include "ranklist.h"

#pragma clang fp contract(off)

namespace {

constexpr int RR_SEGMAX = COR_RERANK_SEGMAX;
constexpr int RR_KMAX = COR_TOPK_KMAX;         // k, k1 and the graph width kg
static_assert(RR_KMAX == 256, "A holds 256 ids");
constexpr long long RR_ID_MAX = 0x7fffffffffffffffLL;

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// the segment tables, passed BY VALUE in the kernel argument block: no device allocation, no copy, nothing to keep alive
struct RrSegs {
  const long long* rnbr[RR_SEGMAX];
  const float* kth[RR_SEGMAX];
  long long off[RR_SEGMAX];
  int n[RR_SEGMAX];
};
struct KrSegs {
  const long long* nbr[RR_SEGMAX];
  long long off[RR_SEGMAX];
  int n[RR_SEGMAX];
};

// ---------------------------------------------------------------------------------------------------------------- graph pruning

__global__ __launch_bounds__(256) void knn_reciprocal_kernel(const KrSegs segs, int nseg, const long long* __restrict__ nbr, long long g_offset,
                                                             long long total, int k1, long long* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;         // edge (g, j) = (e / k1, e % k1)
  if (e >= total) return;
  const long long gid = g_offset + (long long)((u64)e / (unsigned)k1);
  const long long h = nbr[e];
  const long long* list = nullptr;
  seg_lookup(segs, nseg, h, [&](int s, u64 local) { list = segs.nbr[s] + local * (u64)k1; });   // the only place a list's address is formed
  bool found = false;
  if (list)
    for (int t = 0; t < k1 && !found; ++t) found = list[t] == gid;
  out[e] = found ? h : -1;
}

// ------------------------------------------------------------------------------------------------------------------- re-ranking

// id -> the entry's rnbr row and kth value, or false
__device__ __forceinline__ bool rr_lookup(const RrSegs& segs, int nseg, int kg, long long id, const long long*& row, const float*& kth) {
  return seg_lookup(segs, nseg, id, [&](int s, u64 local) {
    row = segs.rnbr[s] + local * (u64)kg;
    kth = segs.kth[s] + local;
  });
}

struct RrIdAt {
  const long long* ids;   // this query's kin ids
  __device__ __forceinline__ long long operator()(unsigned pos) const { return ids[pos]; }
};

// one id of a candidate's list against the sorted A[0, nA): counts it into |B| and, if A holds it, into I
__device__ __forceinline__ void rr_count(const long long* A, int nA, long long h, int& nB, int& I) {
  if (h < 0) return;
  ++nB;
  int lo = 0, n = nA;
  while (n > 0) {                                                        // lower bound: lo + n <= nA throughout
    const int half = n >> 1;
    if (A[lo + half] < h) { lo += half + 1; n -= half + 1; } else n = half;
  }
  I += lo < nA && A[lo] == h;
}

template <bool VEC>
__global__ __launch_bounds__(1024) void rerank_kernel(const float* __restrict__ scores, const long long* __restrict__ idx, const RrSegs segs,
                                                      int nseg, int kin, int npad, int apad, int kg, int k1, float lam, int k,
                                                      unsigned* __restrict__ out_scores, long long* __restrict__ out_idx,
                                                      int* __restrict__ out_pos) {
  extern __shared__ __align__(16) unsigned char rr_lds[];
  u64* key = (u64*)rr_lds;                                               // [npad]
  long long* A = (long long*)(rr_lds + 8 * (size_t)npad);                // [RR_KMAX], apad of them used
  int* cnt = (int*)(rr_lds + 8 * (size_t)npad + 8 * RR_KMAX);            // [0]: |A|, [1]: present entries
  const int tid = threadIdx.x, T = blockDim.x;
  const long long* ids = idx + (long long)blockIdx.x * kin;
  const float* sc = scores + (long long)blockIdx.x * kin;
  const long long out0 = (long long)blockIdx.x * k;

  if (tid < 2) cnt[tid] = 0;
  __syncthreads();

  // 1. A: the entries j < k1 whose row counts the query among its k1 nearest
  int mine = 0;
  for (int j = tid; j < apad; j += T) {
    long long a = RR_ID_MAX;
    if (j < k1) {
      const long long id = ids[j];
      const long long* row = nullptr;
      const float* kth = nullptr;
      if (rr_lookup(segs, nseg, kg, id, row, kth) && sc[j] >= *kth) { a = id; ++mine; }   // a missing entry's score is never read
    }
    A[j] = a;
  }
  if (mine) atomicAdd(&cnt[0], mine);
  __syncthreads();
  block_bitonic_sort(A, apad, PlainBefore{});                            // the |A| ids first (an id equal to the filler sorts beside it)
  const int nA = cnt[0];

  // 2. f of every present entry, as its sort key
  const float oml = 1.0f - lam;
  mine = 0;
  for (int pos = tid; pos < npad; pos += T) {
    unsigned hi = RANK_MISSING, lo = (unsigned)pos;
    if (pos < kin) {
      const long long id = ids[pos];
      const long long* row = nullptr;
      const float* kth = nullptr;
      if (rr_lookup(segs, nseg, kg, id, row, kth)) {
        int nB = 0, I = 0, t = 0;
        if constexpr (VEC) {                                             // kg even, rows 16-byte aligned
          const i64x2* r2 = (const i64x2*)row;
          for (; t + 8 <= kg; t += 8) {                                  // four loads in flight, then the eight searches
            const i64x2 v0 = r2[t / 2], v1 = r2[t / 2 + 1], v2 = r2[t / 2 + 2], v3 = r2[t / 2 + 3];
            rr_count(A, nA, v0[0], nB, I); rr_count(A, nA, v0[1], nB, I); rr_count(A, nA, v1[0], nB, I); rr_count(A, nA, v1[1], nB, I);
            rr_count(A, nA, v2[0], nB, I); rr_count(A, nA, v2[1], nB, I); rr_count(A, nA, v3[0], nB, I); rr_count(A, nA, v3[1], nB, I);
          }
          for (; t < kg; t += 2) {
            const i64x2 v = r2[t / 2];
            rr_count(A, nA, v[0], nB, I); rr_count(A, nA, v[1], nB, I);
          }
        } else {
          for (; t + 4 <= kg; t += 4) {
            const long long h0 = row[t], h1 = row[t + 1], h2 = row[t + 2], h3 = row[t + 3];
            rr_count(A, nA, h0, nB, I); rr_count(A, nA, h1, nB, I); rr_count(A, nA, h2, nB, I); rr_count(A, nA, h3, nB, I);
          }
          for (; t < kg; ++t) rr_count(A, nA, row[t], nB, I);
        }
        const int U = nA + nB - I;
        const float J = U > 0 ? (float)I / (float)U : 0.f;
        const float f = (lam * sc[pos]) + (oml * J);
        const unsigned u = __float_as_uint(f);
        hi = rank_score_key(u);
        if (u == 0x80000000u) lo |= RANK_NEGZERO;
      }
    }
    mine += hi != RANK_MISSING;                  // counted by the KEY: the first `present` ranks are exactly the keys below MISSING
    key[pos] = ((u64)hi << 32) | lo;
  }
  if (mine) atomicAdd(&cnt[1], mine);
  __syncthreads();

  // 3. rank, and the first k
  block_bitonic_sort(key, npad, RankBefore<RrIdAt>{{ids}});
  const int present = cnt[1];
  for (int r = tid; r < k; r += T) {
    if (r < present) {                           // r < present <= kin <= npad
      const u64 kr = key[r];
      const unsigned pos = (unsigned)kr & RANK_POS_MASK;
      out_scores[out0 + r] = rank_key_score(kr);
      out_idx[out0 + r] = ids[pos];
      if (out_pos) out_pos[out0 + r] = (int)pos;
    } else {
      out_scores[out0 + r] = RANK_NEG_INF;
      out_idx[out0 + r] = -1;
      if (out_pos) out_pos[out0 + r] = -1;
    }
  }
}

}  // namespace

extern "C" int cor_knn_reciprocal(const long long* const* seg_nbr, const long long* seg_offset, const int* seg_n, int nseg, int k1, int seg,
                                  long long* out, void* stream) {
  if (!seg_nbr || !seg_offset || !seg_n || nseg < 1 || k1 < 1 || seg < 0 || seg >= nseg) return COR_EINVAL;
  if (nseg > RR_SEGMAX) return COR_ENOSUPPORT;                           // (before the arrays are read: they hold nseg entries)
  for (int s = 0; s < nseg; ++s)
    if (seg_entry_bad(seg_n[s], seg_nbr[s])) return COR_EINVAL;
  if (!out && seg_n[seg] > 0) return COR_EINVAL;
  if (k1 > RR_KMAX) return COR_ENOSUPPORT;
  KrSegs segs = {};
  for (int s = 0; s < nseg; ++s) {
    segs.nbr[s] = seg_nbr[s];
    segs.off[s] = seg_offset[s];
    segs.n[s] = seg_n[s];
  }
  if (seg_n[seg] == 0) return 0;
  const long long total = (long long)seg_n[seg] * k1;                    // < 2^39: at most 2^31 blocks
  hipLaunchKernelGGL(knn_reciprocal_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, segs, nseg, seg_nbr[seg],
                     seg_offset[seg], total, k1, out);
  COR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cor_rerank_reciprocal(const float* scores, const long long* idx, const long long* const* seg_rnbr, const float* const* seg_kth,
                                     const long long* seg_offset, const int* seg_n, int nseg, int Bq, int kin, int kg, int k1, float lam, int k,
                                     float* out_scores, long long* out_idx, int* out_pos, void* stream) {
  if (!scores || !idx || !out_scores || !out_idx || Bq < 0 || kin < 1 || kg < 1 || k1 < 1 || k < 1 || k1 > kin || nseg < 0) return COR_EINVAL;
  if (nseg > 0 && (!seg_rnbr || !seg_kth || !seg_offset || !seg_n)) return COR_EINVAL;
  if (nseg > RR_SEGMAX) return COR_ENOSUPPORT;                           // (before the arrays are read: they hold nseg entries)
  for (int s = 0; s < nseg; ++s)
    if (seg_entry_bad(seg_n[s], seg_rnbr[s] && seg_kth[s])) return COR_EINVAL;
  if (kin > COR_MERGE_NMAX || k > RR_KMAX || k1 > RR_KMAX || kg > RR_KMAX) return COR_ENOSUPPORT;
  RrSegs segs = {};
  bool vec = (kg & 1) == 0;                                              // rows of kg ids are 16-byte aligned if the base is and kg is even
  for (int s = 0; s < nseg; ++s) {
    segs.rnbr[s] = seg_rnbr[s];
    segs.kth[s] = seg_kth[s];
    segs.off[s] = seg_offset[s];
    segs.n[s] = seg_n[s];
    if (seg_n[s] > 0 && ((uintptr_t)seg_rnbr[s] & 15)) vec = false;
  }
  if (Bq == 0) return 0;
  const int npad = next_pow2(kin), apad = next_pow2(k1);
  const int threads = npad < 64 ? 64 : (npad > 1024 ? 1024 : npad);
  const size_t lds = 8 * (size_t)npad + 8 * RR_KMAX + 16;
  const dim3 grid((unsigned)Bq), block(threads);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(rerank_kernel<true>, grid, block, lds, st, scores, idx, segs, nseg, kin, npad, apad, kg, k1, lam, k, (unsigned*)out_scores,
                       out_idx, out_pos);
  else
    hipLaunchKernelGGL(rerank_kernel<false>, grid, block, lds, st, scores, idx, segs, nseg, kin, npad, apad, kg, k1, lam, k, (unsigned*)out_scores,
                       out_idx, out_pos);
  COR_CHECK_LAUNCH();
  return 0;
}
