// cor_amd — the per-row int8 rule of cor_quantize_rows_i8 (include/cor_amd.h), shared by the kernels that quantise: quant.hip (gallery
// rows and the queries of the int8 searches) and rescore_i8.hip (the query, inside the call). Given the row's amax = max |x| in fp32:
//     amax == 0: every q = 0 and scale = 0;   else inv = 127.0f / amax,  q = clamp((int)rintf(x * inv), -127, 127),  scale = amax / 127.0f
// every step one separately rounded fp32 operation (plain division; rintf rounds half to even). The callers test amax != 0 themselves
// and call q8_value only behind it.
#pragma once
#include "common.h"

__device__ __forceinline__ float q8_inv(float amax) { return 127.0f / amax; }
__device__ __forceinline__ int q8_value(float x, float inv) { return (int)fminf(fmaxf(rintf(x * inv), -127.0f), 127.0f); }
__device__ __forceinline__ float q8_scale(float amax) { return amax != 0.f ? amax / 127.0f : 0.f; }
