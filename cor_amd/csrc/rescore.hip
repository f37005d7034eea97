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
//      entry and the padding carry the largest score key and sort last (ranklist.h has the scheme and the tie rule). Repeats of an id
//      have the same score bits, so they end up adjacent, the first occurrence in front.
//   3. Place. keep[r] = rank r is present and the rank before it holds another id; a block scan over the keep flags places the first k
//      survivors, the rest of the k slots get (-inf, -1, -1). The score bits come back out of the key (the flag restores -0.0).
// LDS: 8 B per key + 1 B keep flag per rank + 1 KiB query = 37 KiB at kin = 4096; no scratch memory in global.
#include "ranklist.h"

namespace {

constexpr int RS_CMAX = 256;                   // embedding width limit of the searches
constexpr int RS_NI = 4;                       // candidates per thread, chains interleaved

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

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
  const RankIdList L{cand + (long long)blockIdx.x * kin};

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

  // 2. keys and rank: rank_and_place (ranklist.h), written out. Through the shared function the bf16 instantiation compiled to other code
  // (20 instructions and 10 VGPRs fewer) that measured 0.2 % slower at kin = 256, beyond the parent's spread
  int mine = 0;
#pragma unroll
  for (int j = 0; j < RS_NI; ++j) {
    const int pos = tid + j * T;
    if (pos < npad) {
      unsigned hi = RANK_MISSING, lo = (unsigned)pos;
      if (row[j]) {
        const unsigned u = __float_as_uint(acc[j]);
        hi = rank_score_key(u);
        if (u == 0x80000000u) lo |= RANK_NEGZERO;
      }
      mine += hi != RANK_MISSING;                // counted by the KEY: the first `present` ranks are exactly the keys below MISSING
      key[pos] = ((u64)hi << 32) | lo;
    }
  }
  if (mine) atomicAdd(&s_present, mine);
  __syncthreads();
  block_bitonic_sort(key, npad, RankBefore<RankIdList>{L});
  const int present = s_present;

  // 3. one entry per id (the first of every run of equal ids: the lowest position), the first k of them
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

template <typename TG>
int launch_rescore(const float* Q, const void* G, int Bq, int Ng, int C, long long g_offset, const long long* cand, int kin, int k,
                   float* out_scores, long long* out_idx, int* out_pos, hipStream_t s) {
  const int npad = next_pow2(kin);
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
