// cor_amd — the device steps the one-block-per-query list kernels share (merge.hip, rescore.hip, rescore_i8.hip, rerank.hip, diffuse.hip, fuse.hip;
// the bitonic sort also member_sort.h and ivf.hip) and the id -> segment lookup (rerank.hip, and through segrows.h, which holds the tables of
// gallery rows and their loaders, expand.hip, diversify.hip and diffuse.hip). Integer code only: the files that include this keep their own
// floating-point rules. Not for retrieval.hip, whose block_sort_u64 / rank_key use another key layout.
//
// Rank keys. An entry of a list of n <= COR_MERGE_NMAX = 4096 becomes a 64-bit key in LDS,
//     [score key: 32 bits | 0: 19 bits | -0.0 flag: bit 12 | position in the list: 12 bits],
// sorted ASCENDING. The score key ascends as the score descends and keys -0.0 as +0.0; a kernel that takes the score bits back out of
// the key (rank_key_score) sets the flag for a -0.0, one that reads them through the position sets none. A missing entry and the padding
// up to the next power of two carry RANK_MISSING, above every non-NaN score's key: they sort behind every present entry, the first
// `present` ranks are exactly the keys below RANK_MISSING, and nothing is ever indexed with a missing entry's id.
// Ties. Equal score keys of two PRESENT entries are decided by the 64-bit id, read through the position, and only then (ties between
// scores of distinct rows are rare, and the ids of one query are a few KB that stay in cache); after that by the rest of the key, i.e.
// the position.
// Keep scan. Kernels that drop entries mark the survivors in keep[rank]; rank_keep_scan gives every thread a run of ranks and the
// number of survivors before it, the thread places its survivors while slots are left, rank_fill_tail writes the (-inf, -1, -1) tail.
// Segment lookup. A 64-bit id from a list is hostile: seg_lookup tests it against every segment's [off, off + n) FIRST, takes the
// unsigned difference behind the test (exact there) and hands (segment, local row) to the caller only after a pass: no address is ever
// formed from an id that failed.
#pragma once
#include "common.h"

typedef unsigned long long u64;

static_assert(COR_MERGE_NMAX == 4096, "the rank keys carry 12 position bits, bit 12 is the -0.0 flag, rank -> position tables are 16-bit");
constexpr unsigned RANK_POS_MASK = COR_MERGE_NMAX - 1;
constexpr unsigned RANK_NEGZERO = COR_MERGE_NMAX;   // bit 12 of the key's low word: the score is -0.0 (its score key is that of +0.0)
constexpr unsigned RANK_MISSING = 0xffffffffu;      // score key of missing entries and padding
constexpr unsigned RANK_NEG_INF = 0xff800000u;      // the score bits of the tail

// float bits -> key that ascends as the score DEscends; -0.0 keys as +0.0
__device__ __forceinline__ unsigned rank_score_key(unsigned u) {
  if (u == 0x80000000u) u = 0u;
  const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}
// and back: the score bits of a present entry's key
__device__ __forceinline__ unsigned rank_key_score(u64 key) {
  if ((unsigned)key & RANK_NEGZERO) return 0x80000000u;
  const unsigned asc = ~(unsigned)(key >> 32);
  return (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
}

// the tie rule; id_at(position) is called only for two present entries with equal score keys (positions < n, ids readable)
template <typename IdAt> struct RankBefore {
  IdAt id_at;
  __device__ __forceinline__ bool operator()(u64 a, u64 b) const {
    const unsigned ha = (unsigned)(a >> 32), hb = (unsigned)(b >> 32);
    if (ha == hb && ha != RANK_MISSING) {
      const long long ia = id_at((unsigned)a & RANK_POS_MASK), ib = id_at((unsigned)b & RANK_POS_MASK);
      if (ia != ib) return ia < ib;
    }
    return a < b;
  }
};
struct PlainBefore {
  template <typename T> __device__ __forceinline__ bool operator()(T a, T b) const { return a < b; }
};

// ascending bitonic sort of key[0, npad) in LDS (npad a power of two >= 2) by the whole block; ends with a barrier
template <typename T, typename Before> __device__ void block_bitonic_sort(T* key, int npad, const Before before) {
  const int half = npad >> 1;
  for (int size = 2; size <= npad; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < half; t += blockDim.x) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const T a = key[i], b = key[j];
        if (before(b, a) == ((i & size) == 0)) { key[i] = b; key[j] = a; }
      }
      __syncthreads();
    }
}

// exclusive scan of keep[0, npad) in rank order: the thread owns ranks [lo, hi), `slot` survivors precede them, `total` in all.
// wsum: 16 ints of the caller's LDS; keep must be published (barrier) before the call
struct KeepScan { int lo, hi, slot, total; };
__device__ __forceinline__ KeepScan rank_keep_scan(const unsigned char* keep, int npad, int* wsum) {
  const int tid = threadIdx.x, T = blockDim.x;
  const int chunk = (npad + T - 1) / T, lo = min(tid * chunk, npad), hi = min(lo + chunk, npad);
  int cnt = 0;
  for (int r = lo; r < hi; ++r) cnt += keep[r];
  const int lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < nwaves; ++w) {
    const int v = wsum[w];
    if (w < wave) before += v;
    total += v;
  }
  return KeepScan{lo, hi, before + incl - cnt, total};
}
// the tail of a query's k output slots, [out0 + min(total, k), out0 + k); `third` (positions or group ids) may be null
__device__ __forceinline__ void rank_fill_tail(int total, int k, long long out0, unsigned* __restrict__ out_scores, long long* __restrict__ out_idx,
                                               int* __restrict__ third) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int t = min(total, k) + tid; t < k; t += T) {
    out_scores[out0 + t] = RANK_NEG_INF;
    out_idx[out0 + t] = -1;
    if (third) third[out0 + t] = -1;
  }
}

// the id list of one query (the rescore kernels): kin global row ids, read by position and through a key's position
struct RankIdList {
  const long long* ids;
  __device__ __forceinline__ long long operator()(unsigned pos) const { return ids[pos]; }
  __device__ __forceinline__ long long at(u64 key) const { return ids[(unsigned)key & RANK_POS_MASK]; }
};

// Rank and place of the rescore kernels, by the whole block of T threads (rescore_i8.hip calls it; rescore.hip writes the same lines out,
// see there). The thread hands in the score bits of its NI candidates (positions tid + j T) and whether each is present; every position
// < npad becomes a key, the keys are sorted, the first of every run of equal ids is kept (the lowest position) and the first k survivors
// are written, then the (-inf, -1, -1) tail. key [npad], keep [npad], s_present (zeroed behind a barrier by the caller) and s_wsum [16]
// are the caller's LDS.
template <int NI>
__device__ __forceinline__ void rank_and_place(const unsigned (&bits)[NI], const bool (&has)[NI], const RankIdList L, u64* key,
                                               unsigned char* keep, int* s_present, int* s_wsum, int npad, int k, long long out0,
                                               unsigned* out_scores, long long* out_idx, int* out_pos) {
  const int tid = threadIdx.x, T = blockDim.x;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int pos = tid + j * T;
    if (pos < npad) {
      unsigned hi = RANK_MISSING, lo = (unsigned)pos;
      if (has[j]) {
        const unsigned u = bits[j];
        hi = rank_score_key(u);
        if (u == 0x80000000u) lo |= RANK_NEGZERO;
      }
      mine += hi != RANK_MISSING;                // counted by the KEY: the first `present` ranks are exactly the keys below MISSING
      key[pos] = ((u64)hi << 32) | lo;
    }
  }
  if (mine) atomicAdd(s_present, mine);
  __syncthreads();
  block_bitonic_sort(key, npad, RankBefore<RankIdList>{L});
  const int present = *s_present;
  for (int r = tid; r < npad; r += T) keep[r] = r < present && (r == 0 || L.at(key[r - 1]) != L.at(key[r]));
  __syncthreads();
  const KeepScan sc = rank_keep_scan(keep, npad, s_wsum);
  int o = sc.slot;
  for (int r = sc.lo; r < sc.hi && o < k; ++r)
    if (keep[r]) {
      const u64 kr = key[r];
      out_scores[out0 + o] = rank_key_score(kr);
      out_idx[out0 + o] = L.at(kr);
      if (out_pos) out_pos[out0 + o] = (int)((unsigned)kr & RANK_POS_MASK);
      ++o;
    }
  rank_fill_tail(sc.total, k, out0, out_scores, out_idx, out_pos);
}

// the list shapes cor_rescore_topk and cor_rescore_topk_i8 accept (also their workspace query: 0 bytes or the error)
inline int rescore_shape_check(int Bq, int kin, int k) {
  if (Bq < 0 || kin < 1 || k < 1 || k > COR_TOPK_KMAX) return COR_EINVAL;
  if (kin > COR_MERGE_NMAX) return COR_ENOSUPPORT;
  return 0;
}

// id -> on_hit(segment, local row) and true, or false: the id lies in no segment. Every segment is visited (the table sits in scalar
// registers and nseg is uniform); the callers form their addresses inside on_hit, from a hit alone
template <typename Segs, typename OnHit> __device__ __forceinline__ bool seg_lookup(const Segs& segs, int nseg, long long id, const OnHit on_hit) {
  bool present = false;
  for (int s = 0; s < nseg; ++s) {
    const long long so = segs.off[s];
    if (!present && id >= so) {
      const u64 local = (u64)id - (u64)so;                                 // exact: id >= so
      if (local < (u64)segs.n[s]) {
        present = true;
        on_hit(s, local);
      }
    }
  }
  return present;
}
