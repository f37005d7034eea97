// cor_amd — per-row scalar quantisation to int8 (cor_quantize_rows_i8): the gallery rows of an int8 index and, inside
// cor_similarity_topk_i8, the queries; and the way back, cor_dequantize_rows_i8 (below). The definition, fixed to the bit: include/cor_amd.h. Every floating-point step is one separately
// rounded fp32 operation (`#pragma clang fp contract(off)`, plain `/`, no fast-math flag in the Makefile).
//
// Sixteen lanes per row, sixteen consecutive values per lane (C <= 256): 16-byte loads (four for fp32, two for the 16-bit types), the
// row's amax by four xor-shuffles inside the 16-lane group, one 16-byte store of the sixteen int8 values. A block of 256 threads takes
// 16 rows. Memory-bound: the row is read once and never staged.
#include "quant_i8.h"

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
  const float inv = q8_inv(amax);                                                // the rule: quant_i8.h
  unsigned w[4] = {0u, 0u, 0u, 0u};
  if (amax != 0.f) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qi = q8_value(v[i], inv);
      w[i >> 2] |= ((unsigned)qi & 0xffu) << (8 * (i & 3));
    }
  }
  *(uint4*)(q + row * C + sub * 16) = make_uint4(w[0], w[1], w[2], w[3]);
  if (sub == 0) scale[row] = q8_scale(amax);
}

// cor_dequantize_rows_i8: x = (float)q * scale[row], ONE rounded fp32 multiply, stored as fp32 or rounded again (nearest even) to bf16 /
// fp16. The same geometry: sixteen lanes per row, one 16-byte load of sixteen int8 values per lane, four (fp32) or two (16-bit) 16-byte
// stores. The empty asm keeps the multiply a multiply: without it hipcc folds it into the conversion (v_fma_mixlo_f16 rounds the exact
// product once, a different last bit now and then; region_pool.hip met the same).
template <typename T>
__global__ void __launch_bounds__(256) dequantize_rows_i8_kernel(const signed char* __restrict__ q, const float* __restrict__ scale, int n, int C,
                                                                 T* __restrict__ X) {
#pragma clang fp contract(off)
  const int sub = threadIdx.x & 15;
  const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= n || sub * 16 >= C) return;
  const uint4 u = *(const uint4*)(q + row * C + sub * 16);
  const float s = scale[row];
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
  float x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    x[i] = (float)(int)(signed char)(w[i >> 2] >> (8 * (i & 3))) * s;
    asm volatile("" : "+v"(x[i]));
  }
  T* dst = X + row * C + sub * 16;
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 y;
      y[0] = x[4 * j]; y[1] = x[4 * j + 1]; y[2] = x[4 * j + 2]; y[3] = x[4 * j + 3];
      ((f32x4*)dst)[j] = y;
    }
  } else {
    unsigned h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      unsigned short a, b;
      if constexpr (__is_same(T, bf16_t)) { a = f2bf(x[2 * i]); b = f2bf(x[2 * i + 1]); }
      else { a = __builtin_bit_cast(unsigned short, (_Float16)x[2 * i]); b = __builtin_bit_cast(unsigned short, (_Float16)x[2 * i + 1]); }
      h[i] = (unsigned)a | ((unsigned)b << 16);
    }
    ((uint4*)dst)[0] = make_uint4(h[0], h[1], h[2], h[3]);
    ((uint4*)dst)[1] = make_uint4(h[4], h[5], h[6], h[7]);
  }
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

extern "C" int cor_dequantize_rows_i8(const signed char* q, const float* scale, int n, int C, void* X, int x_dtype, void* stream) {
  if (!X || !q || !scale || n < 0 || C <= 0) return COR_EINVAL;
  if (C > 256 || (C & 15) || (x_dtype != COR_F32 && x_dtype != COR_BF16 && x_dtype != COR_F16)) return COR_ENOSUPPORT;
  if ((((uintptr_t)X | (uintptr_t)q) & 15) || ((uintptr_t)scale & 3)) return COR_EINVAL;
  if (n == 0) return 0;
  const dim3 grid(cdiv(n, 16)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (x_dtype == COR_F32) hipLaunchKernelGGL((dequantize_rows_i8_kernel<float>), grid, block, 0, s, q, scale, n, C, (float*)X);
  else if (x_dtype == COR_BF16) hipLaunchKernelGGL((dequantize_rows_i8_kernel<bf16_t>), grid, block, 0, s, q, scale, n, C, (bf16_t*)X);
  else hipLaunchKernelGGL((dequantize_rows_i8_kernel<_Float16>), grid, block, 0, s, q, scale, n, C, (_Float16*)X);
  COR_CHECK_LAUNCH();
  return 0;
}
