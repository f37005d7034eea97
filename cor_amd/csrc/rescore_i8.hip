// cor_amd — re-scoring of candidate lists against an int8 gallery (cor_rescore_topk_i8): cor_rescore_topk's PRESENT / MISSING rule, order,
// first occurrence per id, out_pos and tail, with the score of cor_similarity_topk_i8. Contract: include/cor_amd.h.
//
// One block per query, T = npad / 4 threads (64 .. 1024; npad = kin rounded up to a power of two), as rescore.hip.
//   0. Query. The first wave quantises the fp32 query by the rule of cor_quantize_rows_i8 (quant_i8.h): lane l holds channels [4l, 4l + 4),
//      the row's amax is a wave maximum, the lane's four int8 values are one word of the C-byte query in LDS; qscale goes to LDS too.
//   1. Scores. Thread t owns the candidates at positions t, t + T, t + 2T, t + 3T. An id is tested against [g_offset, g_offset + Ng)
//      BEFORE anything is derived from it; a candidate that fails is MISSING and loads nothing. A row is C bytes: 16 at a time with one
//      16-byte load per candidate (thread-per-candidate gather, the four candidates' loads interleaved), four v_dot4 per load against the
//      query's words (one broadcast LDS read). d is the exact int32 dot product, score = ((float)d * qscale) * gscale[row]: two separately
//      rounded fp32 multiplies, no addition, so there is nothing to contract.
//   2. Rank and 3. Place: the steps of rescore.hip (ranklist.h): 64-bit keys [score key | -0.0 flag | position], bitonic sort with the id
//      read through the position on ties, keep flags where the rank before holds another id, block scan, (-inf, -1, -1) tail.
// LDS: 8 B per key + 1 B keep flag per rank + 256 B query = 36.25 KiB at kin = 4096; no scratch memory in global.
#include "quant_i8.h"
#include "ranklist.h"

namespace {

constexpr int RI_CMAX = 256;                   // embedding width limit of the searches
constexpr int RI_NI = 4;                       // candidates per thread, loads interleaved

__global__ __launch_bounds__(1024) void rescore_topk_i8_kernel(const float* __restrict__ Q, const signed char* __restrict__ G,
                                                               const float* __restrict__ gscale, int Ng, int C, long long g_offset,
                                                               const long long* __restrict__ cand, int kin, int npad, int k,
                                                               unsigned* __restrict__ out_scores, long long* __restrict__ out_idx,
                                                               int* __restrict__ out_pos) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ri_lds[];
  __shared__ int s_present, s_wsum[16];
  __shared__ float s_qscale;
  u64* key = (u64*)ri_lds;                                         // [npad]
  unsigned* qq = (unsigned*)(ri_lds + 8 * (size_t)npad);           // [RI_CMAX / 4]: the int8 query, four channels to a word
  unsigned char* keep = ri_lds + 8 * (size_t)npad + RI_CMAX;       // [npad]
  const int tid = threadIdx.x, T = blockDim.x;
  const long long out0 = (long long)blockIdx.x * k;
  const RankIdList L{cand + (long long)blockIdx.x * kin};

  // 0. the query, quantised by the first wave (T >= 64)
  if (tid < 64) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (4 * tid < C) {
      const f32x4 x = *(const f32x4*)(Q + (long long)blockIdx.x * C + 4 * tid);
      v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fabsf(v[i]));
    amax = wave_max(amax);
    const float inv = q8_inv(amax);
    unsigned w = 0u;
    if (amax != 0.f) {
#pragma unroll
      for (int i = 0; i < 4; ++i) w |= ((unsigned)q8_value(v[i], inv) & 0xffu) << (8 * i);
    }
    qq[tid] = w;                                                   // the lanes past C / 4 write zero words, never read
    if (tid == 0) { s_qscale = q8_scale(amax); s_present = 0; }
  }
  __syncthreads();
  const float qscale = s_qscale;

  // 1. scores: positions tid + j T, j < RI_NI (host: RI_NI * T >= npad)
  const signed char* row[RI_NI];
  float gs[RI_NI];
  int d[RI_NI];
#pragma unroll
  for (int j = 0; j < RI_NI; ++j) {
    const int pos = tid + j * T;
    row[j] = nullptr;
    gs[j] = 0.f;
    d[j] = 0;
    if (pos < kin) {
      const long long id = L.ids[pos];
      const u64 local = (u64)id - (u64)g_offset;                   // exact when id >= g_offset
      if (id >= g_offset && local < (u64)Ng) {                     // the only place a row address is formed
        row[j] = G + local * (u64)C;
        gs[j] = gscale[local];
      }
    }
  }
  for (int s = 0; s < C / 16; ++s) {
    uint4 g[RI_NI];
#pragma unroll
    for (int j = 0; j < RI_NI; ++j) g[j] = row[j] ? ((const uint4*)row[j])[s] : make_uint4(0u, 0u, 0u, 0u);
    const uint4 q = ((const uint4*)qq)[s];
#pragma unroll
    for (int j = 0; j < RI_NI; ++j) {
      d[j] = __builtin_amdgcn_sdot4((int)g[j].x, (int)q.x, d[j], false);
      d[j] = __builtin_amdgcn_sdot4((int)g[j].y, (int)q.y, d[j], false);
      d[j] = __builtin_amdgcn_sdot4((int)g[j].z, (int)q.z, d[j], false);
      d[j] = __builtin_amdgcn_sdot4((int)g[j].w, (int)q.w, d[j], false);
    }
  }

  // 2. rank and 3. place (ranklist.h)
  unsigned bits[RI_NI]; bool has[RI_NI];
#pragma unroll
  for (int j = 0; j < RI_NI; ++j) { bits[j] = __float_as_uint(((float)d[j] * qscale) * gs[j]); has[j] = row[j] != nullptr; }
  rank_and_place<RI_NI>(bits, has, L, key, keep, &s_present, s_wsum, npad, k, out0, out_scores, out_idx, out_pos);
}

}  // namespace

extern "C" long cor_rescore_i8_workspace_bytes(int Bq, int kin, int k) { return rescore_shape_check(Bq, kin, k); }

extern "C" int cor_rescore_topk_i8(const float* Q, const signed char* Gq, const float* gscale, int Bq, int Ng, int C, long long g_offset,
                                   const long long* cand, int kin, int k, float* out_scores, long long* out_idx, int* out_pos, void* workspace,
                                   void* stream) {
  (void)workspace;
  if (!Q || !cand || !out_scores || !out_idx || ((!Gq || !gscale) && Ng > 0) || Ng < 0 || C < 1) return COR_EINVAL;
  const int rc = rescore_shape_check(Bq, kin, k);
  if (rc) return rc;
  if (C > RI_CMAX || C % 16 != 0) return COR_ENOSUPPORT;
  if (Bq == 0) return 0;
  const int npad = next_pow2(kin);
  const int threads = npad / RI_NI < 64 ? 64 : npad / RI_NI;         // <= 1024; RI_NI * threads >= npad
  const size_t lds = 9 * (size_t)npad + RI_CMAX;
  hipLaunchKernelGGL(rescore_topk_i8_kernel, dim3((unsigned)Bq), dim3(threads), lds, (hipStream_t)stream, Q, Gq, gscale, Ng, C, g_offset, cand,
                     kin, npad, k, (unsigned*)out_scores, out_idx, out_pos);
  COR_CHECK_LAUNCH();
  return 0;
}
