// cor_amd — re-scoring of candidate lists (cor_rescore_topk): per query a list of kin global row ids -> the chain score of every row
// the shard holds, ranked by (score desc, id asc), every id once, the first k. Contract: include/cor_amd.h.
//
// One block per query, T = npad / 4 threads (64 .. 1024; npad = kin rounded up to a power of two), in three phases.
//   1. Scores. The query, rounded to the gallery dtype and widened back, sits in LDS. Thread t owns the candidates at positions
//      t, t + T, t + 2T, t + 3T. An id is tested against [g_offset, g_offset + Ng) BEFORE anything is derived from it; a candidate that
//      fails is MISSING and loads nothing. The four rows are read straight from global memory 16 elements at a time with 16-byte
//      loads (thread-per-candidate gather) and their four fmaf chains advance interleaved: a chain is C dependent fmaf, four of them
//      fill the issue slots between. The order inside a chain is that of oracle/c/sim_chain.c: chunk c of 8, k = 8c+i then 8c+4+i.
//   2. Rank. Every position becomes a 64-bit key in LDS, [order-preserving score key, descending | -0.0 flag | position]; a missing
//      entry and the padding carry the largest score key and sort last. The bitonic network of merge.hip ranks them: equal score keys
//      are decided by the 64-bit id read through the position, then by the rest of the key. Repeats of an id have the same score
//      bits, so they end up adjacent, the first occurrence in front.
//   3. Place. keep[r] = rank r is present and the rank before it holds another id; a block scan over the keep flags places the first k
//      survivors, the rest of the k slots get (-inf, -1, -1). The score bits come back out of the key (the flag restores -0.0).
// LDS: 8 B per key + 1 B keep flag per rank + 1 KiB query = 37 KiB at kin = 4096; no scratch memory in global.
#include "common.h"

namespace {

constexpr int RS_NMAX = COR_MERGE_NMAX;        // candidates per query: 4096 = 12 position bits in the key
static_assert(RS_NMAX == 4096, "the sort keys carry 12 position bits and bit 12 is the -0.0 flag");
constexpr unsigned RS_POS_MASK = RS_NMAX - 1;
constexpr unsigned RS_NEGZERO = RS_NMAX;       // bit 12 of the key's low word: the score is -0.0 (its score key is that of +0.0)
constexpr unsigned RS_MISSING = 0xffffffffu;   // score key of missing entries and padding: above every non-NaN score's key
constexpr unsigned RS_NEG_INF = 0xff800000u;
constexpr int RS_CMAX = 256;                   // embedding width limit of the searches
constexpr int RS_NI = 4;                       // candidates per thread, chains interleaved

typedef unsigned long long u64;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// float bits -> key that ascends as the score DEscends; -0.0 keys as +0.0
__device__ __forceinline__ unsigned rs_score_key(unsigned u) {
  if (u == 0x80000000u) u = 0u;
  const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}
// and back: the score bits of a present entry's key
__device__ __forceinline__ unsigned rs_key_score(u64 key) {
  if ((unsigned)key & RS_NEGZERO) return 0x80000000u;
  const unsigned asc = ~(unsigned)(key >> 32);
  return (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
}

// elements [16 s, 16 s + 16) of a gallery row, widened exactly to fp32 (16-byte loads; rows are 16-byte aligned, C % 16 == 0)
template <typename TG> __device__ __forceinline__ void rs_load16(const TG* __restrict__ row, int s, float (&g)[16]) {
  if constexpr (sizeof(TG) == 4) {
    const f32x4* p = (const f32x4*)row + 4 * s;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const f32x4 x = p[v];
      g[4 * v] = x[0]; g[4 * v + 1] = x[1]; g[4 * v + 2] = x[2]; g[4 * v + 3] = x[3];
    }
  } else {
    const uint4* p = (const uint4*)row + 2 * s;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const uint4 x = p[v];
      if constexpr (__is_same(TG, bf16_t)) {
        const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) { g[8 * v + 2 * e] = __uint_as_float(w[e] << 16); g[8 * v + 2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
      } else {
        const f16x8 h = __builtin_bit_cast(f16x8, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[8 * v + e] = (float)h[e];
      }
    }
  }
}

struct RsList {
  const long long* ids;   // this query's kin candidates
  __device__ __forceinline__ long long at(u64 key) const { return ids[(unsigned)key & RS_POS_MASK]; }
};

__device__ __forceinline__ bool rs_before(u64 a, u64 b, const RsList& L) {
  const unsigned ha = (unsigned)(a >> 32), hb = (unsigned)(b >> 32);
  if (ha == hb && ha != RS_MISSING) {            // a tie between two PRESENT entries: positions < kin
    const long long ia = L.at(a), ib = L.at(b);
    if (ia != ib) return ia < ib;
  }
  return a < b;
}

// ascending bitonic sort of key[0, npad) (npad a power of two >= 2); ends with a barrier
__device__ void rs_sort(u64* key, int npad, const RsList& L) {
  const int half = npad >> 1;
  for (int size = 2; size <= npad; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < half; t += blockDim.x) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const u64 a = key[i], b = key[j];
        if (rs_before(b, a, L) == ((i & size) == 0)) { key[i] = b; key[j] = a; }
      }
      __syncthreads();
    }
}

template <typename TG>
__global__ __launch_bounds__(1024) void rescore_topk_kernel(const float* __restrict__ Q, const TG* __restrict__ G, int Ng, int C,
                                                            long long g_offset, const long long* __restrict__ cand, int kin, int npad, int k,
                                                            unsigned* __restrict__ out_scores, long long* __restrict__ out_idx,
                                                            int* __restrict__ out_pos) {
  extern __shared__ __align__(16) unsigned char rs_lds[];
  __shared__ int s_present, s_wsum[16];
  u64* key = (u64*)rs_lds;                                         // [npad]
  float* qs = (float*)(rs_lds + 8 * (size_t)npad);                 // [RS_CMAX]
  unsigned char* keep = rs_lds + 8 * (size_t)npad + 4 * RS_CMAX;   // [npad]
  const int tid = threadIdx.x, T = blockDim.x;
  const long long out0 = (long long)blockIdx.x * k;
  const RsList L{cand + (long long)blockIdx.x * kin};

  for (int c = tid; c < C; c += T) qs[c] = round_to<TG>(Q[(long long)blockIdx.x * C + c]);
  if (tid == 0) s_present = 0;
  __syncthreads();

  // 1. scores: positions tid + j T, j < RS_NI (host: RS_NI * T >= npad)
  const TG* row[RS_NI];
  float acc[RS_NI];
#pragma unroll
  for (int j = 0; j < RS_NI; ++j) {
    const int pos = tid + j * T;
    row[j] = nullptr;
    acc[j] = 0.f;
    if (pos < kin) {
      const long long id = L.ids[pos];
      const u64 local = (u64)id - (u64)g_offset;                   // exact when id >= g_offset
      if (id >= g_offset && local < (u64)Ng) row[j] = G + local * (u64)C;   // the only place a row address is formed
    }
  }
  for (int s = 0; s < C / 16; ++s) {
    float g[RS_NI][16];
#pragma unroll
    for (int j = 0; j < RS_NI; ++j) {
      if (row[j]) rs_load16<TG>(row[j], s, g[j]);
      else {
#pragma unroll
        for (int e = 0; e < 16; ++e) g[j][e] = 0.f;
      }
    }
    float q[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const f32x4 x = ((const f32x4*)qs)[4 * s + v];
      q[4 * v] = x[0]; q[4 * v + 1] = x[1]; q[4 * v + 2] = x[2]; q[4 * v + 3] = x[3];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < RS_NI; ++j) acc[j] = fmaf(g[j][8 * c + i], q[8 * c + i], acc[j]);
#pragma unroll
        for (int j = 0; j < RS_NI; ++j) acc[j] = fmaf(g[j][8 * c + 4 + i], q[8 * c + 4 + i], acc[j]);
      }
  }

  // 2. keys and rank
  int mine = 0;
#pragma unroll
  for (int j = 0; j < RS_NI; ++j) {
    const int pos = tid + j * T;
    if (pos < npad) {
      unsigned hi = RS_MISSING, lo = (unsigned)pos;
      if (row[j]) {
        const unsigned u = __float_as_uint(acc[j]);
        hi = rs_score_key(u);
        if (u == 0x80000000u) lo |= RS_NEGZERO;
      }
      mine += hi != RS_MISSING;                  // counted by the KEY: the first `present` ranks are exactly the keys below MISSING
      key[pos] = ((u64)hi << 32) | lo;
    }
  }
  if (mine) atomicAdd(&s_present, mine);
  __syncthreads();
  rs_sort(key, npad, L);
  const int present = s_present;

  // 3. one entry per id (the first of every run of equal ids: the lowest position), the first k of them
  for (int r = tid; r < npad; r += T) keep[r] = r < present && (r == 0 || L.at(key[r - 1]) != L.at(key[r]));
  __syncthreads();
  // exclusive scan of the keep flags in rank order: thread t owns ranks [t*chunk, (t+1)*chunk)
  const int chunk = (npad + T - 1) / T, lo_r = min(tid * chunk, npad), hi_r = min(lo_r + chunk, npad);
  int cnt = 0;
  for (int r = lo_r; r < hi_r; ++r) cnt += keep[r];
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
  for (int r = lo_r; r < hi_r && o < k; ++r)
    if (keep[r]) {
      const u64 kr = key[r];
      out_scores[out0 + o] = rs_key_score(kr);
      out_idx[out0 + o] = L.at(kr);
      if (out_pos) out_pos[out0 + o] = (int)((unsigned)kr & RS_POS_MASK);
      ++o;
    }
  for (int t = min(total, k) + tid; t < k; t += T) {
    out_scores[out0 + t] = RS_NEG_INF;
    out_idx[out0 + t] = -1;
    if (out_pos) out_pos[out0 + t] = -1;
  }
}

int rescore_shape_check(int Bq, int kin, int k) {
  if (Bq < 0 || kin < 1 || k < 1 || k > COR_TOPK_KMAX) return COR_EINVAL;
  if (kin > RS_NMAX) return COR_ENOSUPPORT;
  return 0;
}

template <typename TG>
int launch_rescore(const float* Q, const void* G, int Bq, int Ng, int C, long long g_offset, const long long* cand, int kin, int k,
                   float* out_scores, long long* out_idx, int* out_pos, hipStream_t s) {
  int npad = 2;
  while (npad < kin) npad <<= 1;
  const int threads = npad / RS_NI < 64 ? 64 : npad / RS_NI;         // <= 1024; RS_NI * threads >= npad
  const size_t lds = 9 * (size_t)npad + 4 * RS_CMAX;
  hipLaunchKernelGGL(rescore_topk_kernel<TG>, dim3((unsigned)Bq), dim3(threads), lds, s, Q, (const TG*)G, Ng, C, g_offset, cand, kin, npad,
                     k, (unsigned*)out_scores, out_idx, out_pos);
  COR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" long cor_rescore_workspace_bytes(int Bq, int kin, int k) { return rescore_shape_check(Bq, kin, k); }

extern "C" int cor_rescore_topk(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, long long g_offset, const long long* cand,
                                int kin, int k, float* out_scores, long long* out_idx, int* out_pos, void* workspace, void* stream) {
  (void)workspace;
  if (!Q || !cand || !out_scores || !out_idx || (!G && Ng > 0) || Ng < 0 || C < 1) return COR_EINVAL;
  const int rc = rescore_shape_check(Bq, kin, k);
  if (rc) return rc;
  if (C > RS_CMAX || C % 16 != 0) return COR_ENOSUPPORT;
  if (g_dtype != COR_F32 && g_dtype != COR_BF16 && g_dtype != COR_F16) return COR_ENOSUPPORT;
  if (Bq == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  switch (g_dtype) {
    case COR_F32: return launch_rescore<float>(Q, G, Bq, Ng, C, g_offset, cand, kin, k, out_scores, out_idx, out_pos, s);
    case COR_BF16: return launch_rescore<bf16_t>(Q, G, Bq, Ng, C, g_offset, cand, kin, k, out_scores, out_idx, out_pos, s);
    default: return launch_rescore<_Float16>(Q, G, Bq, Ng, C, g_offset, cand, kin, k, out_scores, out_idx, out_pos, s);
  }
}
