// cor_amd — fusion of ranked lists (cor_fuse_lists): P lists of kin (score, global id) entries per query over ONE id space -> one entry per
// distinct id with a fused score (reciprocal-rank fusion, CombSUM, CombMAX), ranked by (fused score desc, id asc), the first k.
// Contract and the definition, fixed to the bit: include/cor_amd.h.
//
// One block per query, merge.hip's shape: n = P*kin entries, npad = next_pow2(n), max(64, min(npad / 2, 1024)) threads, dynamic LDS.
//   1. Holes. Every position becomes a 16-bit sort key [hole: bit 15 | position: 12 bits]; an entry with idx < 0 or a non-finite score, and
//      the padding, are holes. The 64-bit ids are copied into LDS once.
//   2. First sort, by (id, position), holes last: ranklist.h's bitonic network over the 16-bit keys with FuseIdBefore, which reads the two
//      ids out of LDS. Equal ids then form runs in ascending list order, and the repeats of an id inside one list stand side by side, the
//      lowest position first.
//      The choice of step 2. The other form, comparing through the position with the ids left in global memory (RankBefore's way), costs
//      no LDS for the ids but puts two dependent global loads into the compare-exchange of every one of the network's 78 stages (n = 4096),
//      where merge.hip pays them on score ties only; here the id IS the key. In the generated code the LDS form's compare-exchange is two
//      ds_read_u16, two ds_read_b64 and a v_cmp_lt_i64 between barriers with no vmcnt wait at all. So the ids live in LDS (32 KB at
//      n = 4096).
//   3. Validity and statistics (only when normalize or missing needs them): the entry at sorted slot r is a repeat if slot r - 1 holds the
//      same id from the same list; the flags go back to position order and every (list, 64 entries) chunk is reduced by one wave
//      (min and max of an order-preserving integer key, -0.0 keyed as +0.0), lane 0 folding the chunk into the list's LDS slot.
//   4. Walk. The thread at a run's head walks its run: for p = 0 .. P-1 in that order the run's next entry either belongs to list p (its
//      first entry there contributes, the repeats are stepped over) or list p does not hold the id (MISSING_FLOOR adds w_p * f_p).
//      The head's slot becomes a rank key [fused score key | -0.0 flag | slot]; every other slot carries RANK_MISSING.
//   5. Second sort with ranklist.h's tie rule (the id read through slot -> position -> LDS), the first k go out through the slot:
//      rank_key_score gives the fused bits back, the count comes from the slot's byte; then the (-inf, -1, -1) tail.
// LDS: 8 B rank key + 8 B id + 2 B sort key + 1 B flag / count per padded entry = 19 npad bytes, 76 KB at n = 4096.
// Arithmetic: `#pragma clang fp contract(off)` holds for the whole file (expand.hip's header says why the __f*_rn intrinsics are not the
// way): every + - * / below is one separately rounded IEEE fp32 operation.
#include "ranklist.h"

#pragma clang fp contract(off)

namespace {

constexpr int FU_PMAX = COR_FUSE_PMAX;
constexpr unsigned FU_HOLE = 0x8000u;            // bit 15 of a first-sort key: no valid entry at this position
constexpr unsigned FU_NOSTAT = 0xffffffffu;      // a list's min slot while it has no valid entry (no finite score has this key)
static_assert(COR_MERGE_NMAX <= FU_HOLE, "a position and the hole bit share 16 bits");

// the weights and the switches, passed BY VALUE in the kernel argument block: no device allocation, no copy, nothing to keep alive
struct FuseArgs {
  float w[FU_PMAX];
  float rrf_c;
  int mode, normalize, missing;
};

struct FuseLists {
  const unsigned* scores;
  const long long* idx;
  long long qoff, lstride;   // entry e of list p of this block's query: p * lstride + qoff + e
  __device__ __forceinline__ long long at(unsigned p, unsigned e) const { return (long long)p * lstride + qoff + e; }
};

// order-preserving integer key of a finite score (ascending with the score), -0.0 as +0.0, and back
__device__ __forceinline__ unsigned fu_asc_key(unsigned u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fu_asc_value(unsigned a) { return __uint_as_float((a & 0x80000000u) ? (a & 0x7fffffffu) : ~a); }

// the first sort's order: (id, position) among the valid entries, then the holes; ids[] is LDS, indexed by position
struct FuseIdBefore {
  const long long* ids;
  __device__ __forceinline__ bool operator()(unsigned short a, unsigned short b) const {
    if (((a | b) & FU_HOLE) == 0) {
      const long long ia = ids[a], ib = ids[b];
      if (ia != ib) return ia < ib;
    }
    return a < b;
  }
};
// the second sort's tie rule reads the id of a head's slot
struct FuseSlotId {
  const long long* ids;
  const unsigned short* order;
  __device__ __forceinline__ long long operator()(unsigned slot) const { return ids[order[slot]]; }
};

__global__ __launch_bounds__(1024) void fuse_lists_kernel(const unsigned* __restrict__ scores, const long long* __restrict__ idx, int Bq, int kin,
                                                          int P, int n, int npad, int k, const FuseArgs fa, unsigned* __restrict__ out_scores,
                                                          long long* __restrict__ out_idx, int* __restrict__ out_count) {
  extern __shared__ __align__(16) unsigned char fuse_lds[];
  __shared__ int s_present, s_heads;
  __shared__ unsigned s_mn[FU_PMAX], s_mx[FU_PMAX];
  u64* key = (u64*)fuse_lds;                                               // second sort: rank keys by slot
  long long* ids = (long long*)(fuse_lds + 8 * (size_t)npad);              // position -> id
  unsigned short* order = (unsigned short*)(fuse_lds + 16 * (size_t)npad);  // first sort: slot -> [hole | position]
  unsigned char* flag = fuse_lds + 18 * (size_t)npad;                      // step 3: position -> valid; from step 4 on: slot -> count
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
  const long long out0 = (long long)blockIdx.x * k;
  const FuseLists L{scores, idx, (long long)blockIdx.x * kin, (long long)Bq * kin};
  const bool stats = fa.normalize == COR_FUSE_NORM_MINMAX || fa.missing == COR_FUSE_MISSING_FLOOR;

  // 1. holes, ids into LDS
  if (tid == 0) { s_present = 0; s_heads = 0; }
  if (tid < FU_PMAX) { s_mn[tid] = FU_NOSTAT; s_mx[tid] = 0u; }
  __syncthreads();
  int mine = 0;
  for (int pos = tid; pos < npad; pos += T) {
    unsigned o = FU_HOLE | (unsigned)pos;
    long long id = -1;
    if (pos < n) {
      const unsigned p = (unsigned)pos / (unsigned)kin;
      const long long at = L.at(p, (unsigned)pos - p * (unsigned)kin);
      id = idx[at];
      if (id >= 0 && (scores[at] & 0x7f800000u) != 0x7f800000u) { o = (unsigned)pos; ++mine; }
    }
    ids[pos] = id;
    order[pos] = (unsigned short)o;
  }
  if (mine) atomicAdd(&s_present, mine);
  __syncthreads();

  // 2. by (id, position), holes last
  block_bitonic_sort(order, npad, FuseIdBefore{ids});
  const int present = s_present;

  // 3. repeats inside a list are not valid; per-list min / max over the valid entries
  if (stats) {
    for (int r = tid; r < npad; r += T) {
      const unsigned pos = order[r] & RANK_POS_MASK;
      unsigned char v = 0;
      if (r < present) {
        v = 1;
        if (r > 0) {
          const unsigned prev = order[r - 1];                            // r - 1 < present: no hole
          if (ids[prev] == ids[pos] && prev / (unsigned)kin == pos / (unsigned)kin) v = 0;
        }
      }
      flag[pos] = v;                                                     // every position < npad is some slot's: each byte is written once
    }
    __syncthreads();
    const int chunks = (kin + 63) >> 6;
    for (int task = wave; task < P * chunks; task += nwaves) {           // (wave-uniform)
      const unsigned p = (unsigned)task / (unsigned)chunks, e = ((unsigned)task - p * (unsigned)chunks) * 64u + (unsigned)lane;
      unsigned mn = FU_NOSTAT, mx = 0u;
      if (e < (unsigned)kin && flag[p * (unsigned)kin + e]) mn = mx = fu_asc_key(scores[L.at(p, e)]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, (unsigned)__shfl_xor((int)mn, o, 64));
        mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
      }
      if (lane == 0 && mn != FU_NOSTAT) { atomicMin(&s_mn[p], mn); atomicMax(&s_mx[p], mx); }
    }
    __syncthreads();
  }

  // 4. the head of every run walks it
  int heads = 0;
  for (int r = tid; r < npad; r += T) {
    unsigned hi = RANK_MISSING, lo = (unsigned)r;
    unsigned char cnt = 0;
    if (r < present) {
      const long long id = ids[order[r]];
      if (r == 0 || ids[order[r - 1]] != id) {
        float acc = 0.f;
        int j = r;
        for (int p = 0; p < P; ++p) {                                    // (uniform: the weights and the statistics are scalar reads)
          const unsigned base = (unsigned)p * (unsigned)kin;
          unsigned pj = 0;
          bool holds = false;
          if (j < present) {
            pj = order[j];
            holds = pj - base < (unsigned)kin && ids[pj] == id;          // the run's next entry lies in list p
          }
          if (holds) {
            const unsigned e = pj - base;
            float c;
            if (fa.mode == COR_FUSE_RRF) {
              c = fa.w[p] / (fa.rrf_c + (float)(e + 1u));
            } else {
              float v = __uint_as_float(scores[L.at((unsigned)p, e)]);
              if (fa.normalize == COR_FUSE_NORM_MINMAX) {
                const float mn = fu_asc_value(s_mn[p]), mx = fu_asc_value(s_mx[p]);
                v = mx == mn ? 1.0f : (v - mn) / (mx - mn);
              }
              c = fa.w[p] * v;
            }
            if (fa.mode == COR_FUSE_MAX) {
              if (cnt == 0 || c > acc) acc = c;
            } else {
              acc = acc + c;
            }
            ++cnt;
            do ++j; while (j < present && (unsigned)order[j] - base < (unsigned)kin && ids[order[j]] == id);   // its repeats in list p
          } else if (fa.missing == COR_FUSE_MISSING_FLOOR && s_mn[p] != FU_NOSTAT) {
            const float f = fa.normalize == COR_FUSE_NORM_MINMAX ? 0.0f : fu_asc_value(s_mn[p]);
            acc = acc + fa.w[p] * f;
          }
        }
        const unsigned u = __float_as_uint(acc);
        hi = min(rank_score_key(u), RANK_MISSING - 1u);                   // (only a NaN with every bit set would reach RANK_MISSING)
        if (u == 0x80000000u) lo |= RANK_NEGZERO;
        ++heads;
      }
    }
    key[r] = ((u64)hi << 32) | lo;
    flag[r] = cnt;                                                       // (step 3's readers are behind its barrier)
  }
  if (heads) atomicAdd(&s_heads, heads);
  __syncthreads();

  // 5. rank the heads, write the first k through the slot
  block_bitonic_sort(key, npad, RankBefore<FuseSlotId>{FuseSlotId{ids, order}});
  const int total = s_heads;                                             // the first `total` ranks are exactly the heads
  for (int r = tid; r < k && r < total; r += T) {
    const u64 kr = key[r];
    const unsigned slot = (unsigned)kr & RANK_POS_MASK;
    out_scores[out0 + r] = rank_key_score(kr);
    out_idx[out0 + r] = ids[order[slot]];
    if (out_count) out_count[out0 + r] = flag[slot];
  }
  rank_fill_tail(total, k, out0, out_scores, out_idx, out_count);
}

int fuse_shape_check(int P, int Bq, int kin, int k) {
  if (P < 1 || Bq < 0 || kin < 1 || k < 1) return COR_EINVAL;
  if (P > FU_PMAX || (long)P * kin > COR_MERGE_NMAX || k > COR_TOPK_KMAX) return COR_ENOSUPPORT;
  return 0;
}

inline bool fu_finite(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) != 0x7f800000u; }

}  // namespace

extern "C" long cor_fuse_lists_workspace_bytes(int P, int Bq, int kin, int k) { return fuse_shape_check(P, Bq, kin, k); }

extern "C" int cor_fuse_lists(const float* scores, const long long* idx, int P, int Bq, int kin, const float* weights_host, int mode,
                              int normalize, int missing, float rrf_c, int k, float* out_scores, long long* out_idx, int* out_count,
                              void* workspace, void* stream) {
  (void)workspace;
  if (!scores || !idx || !weights_host || !out_scores || !out_idx) return COR_EINVAL;
  if (mode != COR_FUSE_RRF && mode != COR_FUSE_SUM && mode != COR_FUSE_MAX) return COR_EINVAL;
  if (normalize != COR_FUSE_NORM_NONE && normalize != COR_FUSE_NORM_MINMAX) return COR_EINVAL;
  if (missing != COR_FUSE_MISSING_ZERO && missing != COR_FUSE_MISSING_FLOOR) return COR_EINVAL;
  if (mode == COR_FUSE_RRF && (normalize != COR_FUSE_NORM_NONE || missing != COR_FUSE_MISSING_ZERO)) return COR_EINVAL;
  if (mode == COR_FUSE_MAX && missing != COR_FUSE_MISSING_ZERO) return COR_EINVAL;
  if (mode == COR_FUSE_RRF && (!fu_finite(rrf_c) || rrf_c < 0.f)) return COR_EINVAL;
  const int rc = fuse_shape_check(P, Bq, kin, k);                          // (before the weights are read: they are P <= 16 floats)
  if (rc) return rc;
  FuseArgs fa = {};
  for (int p = 0; p < P; ++p) {
    if (!fu_finite(weights_host[p])) return COR_EINVAL;
    fa.w[p] = weights_host[p];
  }
  fa.rrf_c = rrf_c;
  fa.mode = mode;
  fa.normalize = normalize;
  fa.missing = missing;
  if (Bq == 0) return 0;
  const int n = P * kin;
  const int npad = next_pow2(n);
  const int threads = npad / 2 < 64 ? 64 : (npad / 2 > 1024 ? 1024 : npad / 2);
  const size_t lds = (size_t)npad * 19;
  static DevOnce once;
  cor_max_dyn_lds((const void*)fuse_lists_kernel, 19 * COR_MERGE_NMAX, once);
  hipLaunchKernelGGL(fuse_lists_kernel, dim3((unsigned)Bq), dim3(threads), lds, (hipStream_t)stream, (const unsigned*)scores, idx, Bq, kin, P, n,
                     npad, k, fa, (unsigned*)out_scores, out_idx, out_count);
  COR_CHECK_LAUNCH();
  return 0;
}
