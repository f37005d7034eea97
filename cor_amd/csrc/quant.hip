// cor_amd — per-row scalar quantisation to int8 (cor_quantize_rows_i8): the gallery rows of an int8 index and, inside
// cor_similarity_topk_i8, the queries. The definition, fixed to the bit: include/cor_amd.h. Every floating-point step is one separately
// rounded fp32 operation (`#pragma clang fp contract(off)`, plain `/`, no fast-math flag in the Makefile).
//
// Sixteen lanes per row, sixteen consecutive values per lane (C <= 256): 16-byte loads (four for fp32, two for the 16-bit types), the
// row's amax by four xor-shuffles inside the 16-lane group, one 16-byte store of the sixteen int8 values. A block of 256 threads takes
// 16 rows. Memory-bound: the row is read once and never staged.
#include "common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename T>
__device__ __forceinline__ void load16(const T* p, float* v) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 x = ((const f32x4*)p)[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[4 * j + i] = x[i];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint4 u = ((const uint4*)p)[j];
      if constexpr (__is_same(T, bf16_t)) {
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[8 * j + 2 * i] = __uint_as_float(w[i] << 16); v[8 * j + 2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
      } else {
        const f16x8 h = __builtin_bit_cast(f16x8, u);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[8 * j + i] = (float)h[i];
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) quantize_rows_i8_kernel(const T* __restrict__ X, int n, int C, signed char* __restrict__ q,
                                                               float* __restrict__ scale) {
#pragma clang fp contract(off)
  const int sub = threadIdx.x & 15;
  const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = row < n && sub * 16 < C;
  float v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = 0.f;
  if (live) load16<T>(X + row * C + sub * 16, v);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(v[i]));
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));   // stays inside the row's 16 lanes
  if (!live) return;
  const float inv = 127.0f / amax;
  unsigned w[4] = {0u, 0u, 0u, 0u};
  if (amax != 0.f) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qi = (int)fminf(fmaxf(rintf(v[i] * inv), -127.0f), 127.0f);
      w[i >> 2] |= ((unsigned)qi & 0xffu) << (8 * (i & 3));
    }
  }
  *(uint4*)(q + row * C + sub * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  if (sub == 0) scale[row] = amax != 0.f ? amax / 127.0f : 0.f;
}

}  // namespace

extern "C" int cor_quantize_rows_i8(const void* X, int x_dtype, int n, int C, signed char* q, float* scale, void* stream) {
  if (!X || !q || !scale || n < 0 || C <= 0) return COR_EINVAL;
  if (C > 256 || (C & 15) || (x_dtype != COR_F32 && x_dtype != COR_BF16 && x_dtype != COR_F16)) return COR_ENOSUPPORT;
  if ((((uintptr_t)X | (uintptr_t)q) & 15) || ((uintptr_t)scale & 3)) return COR_EINVAL;
  if (n == 0) return 0;
  const dim3 grid(cdiv(n, 16)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (x_dtype == COR_F32) hipLaunchKernelGGL((quantize_rows_i8_kernel<float>), grid, block, 0, s, (const float*)X, n, C, q, scale);
  else if (x_dtype == COR_BF16) hipLaunchKernelGGL((quantize_rows_i8_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)X, n, C, q, scale);
  else hipLaunchKernelGGL((quantize_rows_i8_kernel<_Float16>), grid, block, 0, s, (const _Float16*)X, n, C, q, scale);
  COR_CHECK_LAUNCH();
  return 0;
}
