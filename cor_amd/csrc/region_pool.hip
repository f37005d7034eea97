// cor_amd — region pooling for the multi-region gallery builder (gfx950): many masks pooled against ONE image's tokens.
// cor_masked_pool walks an image's P x D tokens once per mask; here a block owns (image, tile of RP_T regions) and walks them once
// for the whole tile. Bandwidth- / latency-shaped, no MFMA: every (region, channel) result is the same p-ordered fmaf chain, the
// same fixed-shape denominator and norm reductions as masked_pool_kernel's channels-last branch, so an f32 row is bit-identical to
// what cor_masked_pool returns for that mask alone, whatever tile the region falls in.
#include "common.h"

namespace {

constexpr int RP_T = 8;      // regions per block: accumulators per thread; 8 fmaf + 2 broadcast ds_read_b128 per token row
constexpr int RP_PC = 256;   // mask positions staged per LDS chunk (= block size: thread tid stages p = chunk * 256 + tid, which is
                             // exactly masked_pool_kernel's strided partial sum of the denominator)
constexpr int RP_UB = 16;    // token rows per register buffer; RP_NB buffers form a ring: while buffer b is consumed, the rows of the
constexpr int RP_NB = 4;     // next RP_NB - 1 buffers are in flight (48 rows ahead: ~1000 cycles of fmaf work against the HBM latency)
constexpr int RP_U = RP_UB * RP_NB;
constexpr int RP_DMAX = 1024;

template <typename TO> __device__ __forceinline__ void rp_st(TO* p, float v);
template <> __device__ __forceinline__ void rp_st<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void rp_st<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }
template <> __device__ __forceinline__ void rp_st<_Float16>(_Float16* p, float v) {
  // the fp16 row is the ROUNDED fp32 row rounded again (what .to(float16) of the fp32 output gives). Without the empty asm hipcc folds
  // the caller's multiply into v_fma_mixlo_f16, which rounds the exact product once: a different last bit now and then.
  asm volatile("" : "+v"(v));
  *p = (_Float16)v;                                            // v_cvt_f16_f32: nearest-even
}

// the mask values of position p for the tile's regions (0 for the slots beyond the tile's count and for p >= P)
template <int T>
__device__ __forceinline__ void rp_load_masks(const float* mrow, int nt, int P, int p, float (&v)[T]) {
#pragma unroll
  for (int t = 0; t < T; ++t) v[t] = (t < nt && p < P) ? mrow[(long)t * P + p] : 0.f;
}

// clamp, add to this thread's partial denominators (p ascending over the calls), write the T values of row `tid` of an LDS chunk
template <int T>
__device__ __forceinline__ void rp_stage(const float (&v)[T], float* chunk, int tid, bool pok, int clamp01, float (&ms)[T]) {
  float w[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    w[t] = v[t];
    if (clamp01) w[t] = fminf(fmaxf(w[t], 0.f), 1.f);
    if (pok) ms[t] += w[t];
  }
#pragma unroll
  for (int j = 0; j < T / 4; ++j) {
    f32x4 o; o[0] = w[4 * j]; o[1] = w[4 * j + 1]; o[2] = w[4 * j + 2]; o[3] = w[4 * j + 3];
    *(f32x4*)(chunk + tid * T + 4 * j) = o;
  }
}

// one token value against the T mask values of its position (the same address in every lane: broadcast reads)
template <int T>
__device__ __forceinline__ void rp_fma_row(float x, const float* m, float (&acc)[T]) {
#pragma unroll
  for (int j = 0; j < T / 4; ++j) {
    const f32x4 v = *(const f32x4*)(m + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[4 * j + e] = fmaf(x, v[e], acc[4 * j + e]);
  }
}

// grid: one block per (image, tile); the host only knows an upper bound of the tile count (ceil(R/T) + B), every block finds its
// tile by walking the offsets, blocks beyond the last tile leave. Offsets are clamped into [0, R] and made non-decreasing pairwise,
// so nothing outside tokens[B,P,D], masks[R,P] and out[R,D] is touched whatever they hold.
template <int T, typename TO>
__global__ void __launch_bounds__(256) region_pool_kernel(const float* __restrict__ tokens, const float* __restrict__ masks,
                                                          const int* __restrict__ offs, TO* __restrict__ out, int B, int R, int P, int D,
                                                          int clamp01, int l2norm) {
  static_assert(T % 4 == 0 && RP_PC % RP_U == 0 && RP_U <= 64, "tile / ring shapes");
  extern __shared__ __attribute__((aligned(16))) float sm[];   // mk[2][RP_PC][T] | res[T][D] | red[T][8]
  float* mk = sm; float* res = sm + 2 * RP_PC * T; float* red = res + T * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int img = -1, r0 = 0, nt = 0;
  for (int i = 0, left = blockIdx.x; i < B; ++i) {
    const int lo = min(max(offs[i], 0), R), hi = min(max(offs[i + 1], lo), R);
    const int tiles = (hi - lo + T - 1) / T;
    if (left < tiles) { img = i; r0 = lo + left * T; nt = min(T, hi - r0); break; }
    left -= tiles;
  }
  if (img < 0) return;
  const float* mrow = masks + (long)r0 * P;
  const float* tok = tokens + (long)img * P * D;
  const int nc = (P + RP_PC - 1) / RP_PC;
  float denom[T];
  for (int dc = 0; dc < D; dc += 256) {                        // thread = channel; D > 256: the walk is repeated per 256 channels
    const int d = dc + tid;
    const bool dok = d < D;
    const unsigned dcl = dok ? d : D - 1, Du = D, plast = P - 1;   // 32-bit element offsets inside one image (the host checks P * D)
    unsigned pn = 0;                                           // the next token row to request, clamped to the last one
    float acc[T], ms[T], nv[T], tk[RP_U];
#pragma unroll
    for (int t = 0; t < T; ++t) { acc[t] = 0.f; ms[t] = 0.f; }
    rp_load_masks<T>(mrow, nt, P, tid, nv);
    rp_stage<T>(nv, mk, tid, tid < P, clamp01, ms);
    if (nc > 1) rp_load_masks<T>(mrow, nt, P, RP_PC + tid, nv);  // the masks run one chunk ahead of their LDS write: no drain of the token loads
#pragma unroll
    for (int u = 0; u < RP_U - RP_UB; ++u) { tk[u] = tok[pn * Du + dcl]; pn = min(pn + 1, plast); }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      if (c + 1 < nc) {
        rp_stage<T>(nv, mk + ((c + 1) & 1) * RP_PC * T, tid, (c + 1) * RP_PC + tid < P, clamp01, ms);
        if (c + 2 < nc) rp_load_masks<T>(mrow, nt, P, (c + 2) * RP_PC + tid, nv);
      }
      const float* mb = mk + (c & 1) * RP_PC * T;
      const int pbeg = c * RP_PC, pend = min(P, pbeg + RP_PC);
      // RP_U rows: on entry buffer b holds token rows min(p + b * RP_UB + u, P - 1) for b < RP_NB - 1, the last buffer is free. The
      // scheduling barriers keep every buffer's loads where they are written: RP_NB - 1 buffers ahead of their use.
      auto rows = [&](int p, bool guard) {
#pragma unroll
        for (int b = 0; b < RP_NB; ++b) {
          const int nb = (b + RP_NB - 1) % RP_NB;
#pragma unroll
          for (int u = 0; u < RP_UB; ++u) { tk[nb * RP_UB + u] = tok[pn * Du + dcl]; pn = min(pn + 1, plast); }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < RP_UB; ++u)
            if (!guard || p + b * RP_UB + u < pend) rp_fma_row<T>(tk[b * RP_UB + u], mb + (p - pbeg + b * RP_UB + u) * T, acc);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      int p = pbeg;
      for (; p + RP_U <= pend; p += RP_U) rows(p, false);
      if (p < pend) rows(p, true);                             // the last, partial block of the last chunk
      __syncthreads();
    }
    if (dc == 0) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float s = wave_sum(ms[t]);
        if (lane == 0) red[t * 8 + wave] = s;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < T; ++t) denom[t] = red[t * 8] + red[t * 8 + 1] + red[t * 8 + 2] + red[t * 8 + 3] + 1e-8f;
    }
    if (dok) {
#pragma unroll
      for (int t = 0; t < T; ++t) res[t * D + d] = acc[t] / denom[t];
    }
  }
  __syncthreads();
  float inv[T];
#pragma unroll
  for (int t = 0; t < T; ++t) inv[t] = 1.f;
  if (l2norm) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      float q = 0.f;
      for (int dd = tid; dd < D; dd += 256) q += res[t * D + dd] * res[t * D + dd];
      q = wave_sum(q);
      if (lane == 0) red[t * 8 + 4 + wave] = q;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < T; ++t) inv[t] = 1.0f / fmaxf(sqrtf(red[t * 8 + 4] + red[t * 8 + 5] + red[t * 8 + 6] + red[t * 8 + 7]), 1e-12f);
  }
#pragma unroll
  for (int t = 0; t < T; ++t)
    if (t < nt)
      for (int dd = tid; dd < D; dd += 256) rp_st<TO>(out + (long)(r0 + t) * D + dd, res[t * D + dd] * inv[t]);
}

}  // namespace

extern "C" int cor_region_pool(const float* tokens, const float* masks, const int* region_offsets, void* out, int out_dtype, int B, int R,
                               int P, int D, int clamp01, int l2norm, void* stream) {
  if (!tokens || !masks || !region_offsets || !out || B < 0 || R < 0 || P <= 0 || D <= 0) return COR_EINVAL;
  if (out_dtype != COR_F32 && out_dtype != COR_BF16 && out_dtype != COR_F16) return COR_EINVAL;
  if (R == 0 || B == 0) return 0;
  if (D > RP_DMAX || (long)P * D > (1L << 30)) return COR_ENOSUPPORT;   // 32-bit byte offsets inside one image's tokens
  const size_t lds = ((size_t)2 * RP_PC * RP_T + (size_t)RP_T * D + 8 * RP_T) * sizeof(float);   // 16 KB + 32 D + 256 B: 48.3 KB at D = 1024
  const dim3 grid((unsigned)((long)cdiv(R, RP_T) + B));
  if (out_dtype == COR_F32)
    hipLaunchKernelGGL((region_pool_kernel<RP_T, float>), grid, dim3(256), lds, (hipStream_t)stream, tokens, masks, region_offsets, (float*)out, B, R, P, D, clamp01, l2norm);
  else if (out_dtype == COR_BF16)
    hipLaunchKernelGGL((region_pool_kernel<RP_T, bf16_t>), grid, dim3(256), lds, (hipStream_t)stream, tokens, masks, region_offsets, (bf16_t*)out, B, R, P, D, clamp01, l2norm);
  else
    hipLaunchKernelGGL((region_pool_kernel<RP_T, _Float16>), grid, dim3(256), lds, (hipStream_t)stream, tokens, masks, region_offsets, (_Float16*)out, B, R, P, D, clamp01, l2norm);
  COR_CHECK_LAUNCH();
  return 0;
}
