// cor_amd — query expansion / database-side augmentation (cor_expand_queries): per query the weighted sum of the first m rows its list
// names, plus the weighted query, optionally L2-normalised. Contract and the definition, fixed to the bit: include/cor_amd.h.
//
// One wave per query, EX_QPB = 4 queries per 256-thread block; there is no block-level cooperation, hence no barrier and no LDS.
//   Lane l owns channels [4l, 4l + 4): a row is ONE coalesced wave load, 16 B per lane for fp32 rows and 8 B for 16-bit rows (C = 256: all
//   64 lanes; smaller C: the lanes past C / 4 re-read channels 0..3, stay out of the tree and store nothing, so no load or store is masked).
//   1. List. 64 entries at a time, lane j takes entry j: its id is looked up in the segment table (ranklist.h's seg_lookup: the range test
//      comes first) and only a hit forms the row address; the entry's weight w = max(score, +0)^alpha
//      is computed there too (alpha dependent multiplies). The segment table is a by-value kernel argument, read with scalar loads.
//   2. Rows. A ballot gives the present entries of the 64; they are walked in list order, lowest set bit first, 8 at a time (then 4, 2,
//      1 for what is left): the entry's row address, weight and dtype come out of lane j by v_readlane, the loads of the whole group are
//      issued, then the group's products and sums follow in list order. A missing entry costs nothing and loads nothing.
//   3. Norm. s = v * v per channel (+0 in the lanes past C / 4); the tree s[c] += s[c + h], h = 128 .. 1, is 6 lane exchanges at distance
//      h / 4 = 32 .. 1 on the lane's four values, then s[0] += s[2], s[1] += s[3], s[0] += s[1] inside lane 0.
// cor_expand_queries_sq is the same body over a table that also carries the row scales of int8 segments: an int8 row is 4 B per lane (one
// dword), its value (float)q * scale, one rounded multiply, the scale fetched in step 1 by the lane that looked the id up.
// Arithmetic: every operation is one separately rounded IEEE fp32 operation. `#pragma clang fp contract(off)` below holds for the whole
// file: HIP's __fmul_rn / __fadd_rn are plain * and + (contractible under the default -ffp-contract=fast) and its __fsqrt_rn is the
// APPROXIMATE native square root, so none of them is used here; a / b and __builtin_sqrtf are correctly rounded in a build without
// fast-math flags (-fhip-fp32-correctly-rounded-divide-sqrt is the default), and the Makefile adds no such flag for this file.
#include "ranklist.h"

#pragma clang fp contract(off)

namespace {

constexpr int EX_SEGMAX = COR_EXPAND_SEGMAX;
constexpr int EX_QPB = 4;        // queries (waves) per block
constexpr int EX_CMAX = 256;     // 64 lanes x 4 channels
constexpr int EX_ALPHA_MAX = 8;

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// the segment table, passed BY VALUE in the kernel argument block (384 B): no device allocation, no copy, nothing to keep alive
struct ExSegs {
  const unsigned char* rows[EX_SEGMAX];
  long long off[EX_SEGMAX];
  int n[EX_SEGMAX];
  int dt[EX_SEGMAX];
};
// the table of cor_expand_queries_sq: one more pointer per segment, the row scales of a COR_I8 segment (512 B by value)
struct ExSegsSq {
  const unsigned char* rows[EX_SEGMAX];
  long long off[EX_SEGMAX];
  int n[EX_SEGMAX];
  int dt[EX_SEGMAX];
  const float* scale[EX_SEGMAX];
};

// the lane's four channels of one row, as stored. The row address travels as an integer (two v_readlane halves); the loads name the GLOBAL
// address space, so they are global_load (scalar base + lane offset), not flat_load. ESZ = 4 / 2: every segment has rows of that element
// size; ESZ = 0: sizes differ between segments, two 8-byte loads whose second one repeats the first for a 16-bit row (no branch around a load)
// ESZ = 1: every segment holds int8 rows, the lane's four channels are ONE dword (C = 256: a row is one 256-byte wave load). ESZ = -1: int8
// and float segments together: a dword, a second dword and an 8-byte load at offsets chosen by the dtype, every one inside the row (an
// int8 row's second and third load repeat bytes the lane does not use), again no branch around a load
#define EX_GLOBAL __attribute__((address_space(1)))
template <int ESZ> __device__ __forceinline__ u32x4 ex_load(u64 row, int c0, int dt) {
  u32x4 r = {0u, 0u, 0u, 0u};
  if constexpr (ESZ == 4) {
    r = *(const EX_GLOBAL u32x4*)(row + 4u * c0);
  } else if constexpr (ESZ == 1) {
    r[0] = *(const EX_GLOBAL unsigned*)(row + (unsigned)c0);
  } else if constexpr (ESZ == -1) {
    const bool wide = dt == COR_F32, narrow = dt == COR_I8;
    const unsigned o = wide ? 4u * c0 : narrow ? (unsigned)c0 : 2u * c0;
    const unsigned a = *(const EX_GLOBAL unsigned*)(row + o), b = *(const EX_GLOBAL unsigned*)(row + o + (narrow ? 0u : 4u));
    const u32x2 c = *(const EX_GLOBAL u32x2*)(row + (wide ? o + 8u : narrow ? (unsigned)c0 & ~7u : o));
    r[0] = a; r[1] = b; r[2] = c[0]; r[3] = c[1];
  } else if constexpr (ESZ == 2) {
    const u32x2 a = *(const EX_GLOBAL u32x2*)(row + 2u * c0);
    r[0] = a[0]; r[1] = a[1];
  } else {
    const bool wide = dt == COR_F32;
    const unsigned o = wide ? 4u * c0 : 2u * c0;
    const u32x2 a = *(const EX_GLOBAL u32x2*)(row + o), b = *(const EX_GLOBAL u32x2*)(row + o + (wide ? 8u : 0u));
    r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1];
  }
  return r;
}

// stored values -> fp32, exactly (dt is wave-uniform); an int8 row's value is (float)q * rs, rs the row's scale: one rounded multiply
template <int ESZ> __device__ __forceinline__ void ex_widen(const u32x4 r, int dt, float rs, float (&x)[4]) {
  if (ESZ == 1 || (ESZ == -1 && dt == COR_I8)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = (float)(int)(signed char)(r[0] >> (8 * e)) * rs;
  } else if (ESZ == 4 || ((ESZ == 0 || ESZ == -1) && dt == COR_F32)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = __uint_as_float(r[e]);
  } else if (dt == COR_BF16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = __uint_as_float(e & 1 ? r[e >> 1] & 0xffff0000u : r[e >> 1] << 16);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = (float)__builtin_bit_cast(_Float16, (unsigned short)(e & 1 ? r[e >> 1] >> 16 : r[e >> 1] & 0xffffu));
  }
}

// the next U present entries of `mask` (lowest bit first = list order): all U rows are requested before the first add
template <int ESZ, int U>
__device__ __forceinline__ void ex_group(u64& mask, unsigned plo, unsigned phi, float w, float rs, int dt, int c0, float (&v)[4]) {
  u32x4 raw[U];
  float wu[U], su[U];
  int du[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = __builtin_ctzll(mask);                                 // mask has at least U bits set (the caller counted them)
    mask &= mask - 1;
    const u64 row = ((u64)(unsigned)__builtin_amdgcn_readlane((int)phi, j) << 32) | (unsigned)__builtin_amdgcn_readlane((int)plo, j);
    wu[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), j));
    du[u] = __builtin_amdgcn_readlane(dt, j);
    su[u] = 0.f;
    if constexpr (ESZ == 1 || ESZ == -1) su[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rs), j));   // travels with the weight
    raw[u] = ex_load<ESZ>(row, c0, du[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float x[4];
    ex_widen<ESZ>(raw[u], du[u], su[u], x);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] + (wu[u] * x[e]);
  }
}

template <int ESZ, typename Segs>
__device__ __forceinline__ void expand_body(const float* __restrict__ Q, float qw, const Segs& segs, int nseg,
                                            const float* __restrict__ scores, const long long* __restrict__ idx, int Bq,
                                            int kin, int m, int C, int alpha, int normalize, void* __restrict__ out,
                                            int out_dtype) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * EX_QPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b >= Bq) return;                                                   // the whole wave leaves; no barrier follows
  const bool active = 4 * lane < C;
  const int c0 = active ? 4 * lane : 0;                                  // a lane past the row reads channels 0..3 again: in bounds, unused

  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (qw != 0.f) {                                                       // (Q may be NULL otherwise)
    const f32x4 q = *(const f32x4*)(Q + b * C + c0);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = qw * q[e];
  }

  const long long* ids = idx + b * kin;
  const float* sc = scores + b * kin;
  for (int j0 = 0; j0 < m; j0 += 64) {
    // 1. lane j: entry j0 + j
    const int j = j0 + lane;
    u64 row = 0;
    float w = 0.f, rs = 0.f;
    int dt = COR_F32;
    bool present = false;
    if (j < m) {
      present = seg_lookup(segs, nseg, ids[j], [&](int s, u64 local) {   // the only place a row address is formed
        dt = segs.dt[s];
        if constexpr (ESZ == 1 || ESZ == -1) {
          row = (u64)segs.rows[s] + local * (u64)(C * (dt == COR_F32 ? 4 : dt == COR_I8 ? 1 : 2));
          if (dt == COR_I8) rs = segs.scale[s][local];                   // the row's scale, fetched by the lane that looked the id up
        } else {
          row = (u64)segs.rows[s] + local * (u64)(C * (dt == COR_F32 ? 4 : 2));
        }
      });
      if (present) {                                                     // a missing entry's score is never read
        const float t0 = sc[j];
        const float t = t0 > 0.f ? t0 : 0.f;                             // NaN, -0.0 and negatives: +0
        w = 1.f;
        for (int a = 0; a < alpha; ++a) w = w * t;
      }
    }
    // 2. the present entries in list order
    u64 mask = __ballot(present);
    int cnt = __builtin_popcountll(mask);
    const unsigned plo = (unsigned)row, phi = (unsigned)(row >> 32);
    for (; cnt >= 8; cnt -= 8) ex_group<ESZ, 8>(mask, plo, phi, w, rs, dt, c0, v);
    if (cnt & 4) ex_group<ESZ, 4>(mask, plo, phi, w, rs, dt, c0, v);
    if (cnt & 2) ex_group<ESZ, 2>(mask, plo, phi, w, rs, dt, c0, v);
    if (cnt & 1) ex_group<ESZ, 1>(mask, plo, phi, w, rs, dt, c0, v);
  }

  // 3. the norm: the stride-halving tree over 256 channel slots
  if (normalize) {
    float s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = active ? v[e] * v[e] : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                                   // h = 4 o: channel c + h lives in lane l + o, same slot
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = s[e] + __shfl_xor(s[e], o, 64); // lanes < o hold the tree's values (l ^ o = l + o there)
    }
    s[0] = s[0] + s[2];                                                  // h = 2
    s[1] = s[1] + s[3];
    s[0] = s[0] + s[1];                                                  // h = 1
    const float s0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s[0])));
    const float d = fmaxf(__builtin_sqrtf(s0), 1e-12f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] / d;
  }

  if (active) {
    const long long o = b * C + 4 * lane;
    if (out_dtype == COR_F32) {
      f32x4 y;
      y[0] = v[0]; y[1] = v[1]; y[2] = v[2]; y[3] = v[3];
      *(f32x4*)((float*)out + o) = y;
    } else {
      unsigned short h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = out_dtype == COR_BF16 ? f2bf(v[e]) : __builtin_bit_cast(unsigned short, (_Float16)v[e]);
      uint2 y;
      y.x = (unsigned)h[0] | ((unsigned)h[1] << 16);
      y.y = (unsigned)h[2] | ((unsigned)h[3] << 16);
      *(uint2*)((unsigned short*)out + o) = y;
    }
  }
}

template <int ESZ>
__global__ __launch_bounds__(64 * EX_QPB) void expand_kernel(const float* __restrict__ Q, float qw, const ExSegs segs, int nseg,
                                                             const float* __restrict__ scores, const long long* __restrict__ idx, int Bq,
                                                             int kin, int m, int C, int alpha, int normalize, void* __restrict__ out,
                                                             int out_dtype) {
  expand_body<ESZ>(Q, qw, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
}
// the table with row scales: ESZ = 1 (int8 segments alone) or -1 (int8 and float segments together)
template <int ESZ>
__global__ __launch_bounds__(64 * EX_QPB) void expand_sq_kernel(const float* __restrict__ Q, float qw, const ExSegsSq segs, int nseg,
                                                                const float* __restrict__ scores, const long long* __restrict__ idx, int Bq,
                                                                int kin, int m, int C, int alpha, int normalize, void* __restrict__ out,
                                                                int out_dtype) {
  expand_body<ESZ>(Q, qw, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
}

}  // namespace

extern "C" int cor_expand_queries(const float* Q, float query_weight, const void* const* seg_rows, const long long* seg_offset, const int* seg_n,
                                  const int* seg_dtype, int nseg, const float* scores, const long long* idx, int Bq, int kin, int m, int C, int alpha,
                                  int normalize, void* out, int out_dtype, void* stream) {
  if (!scores || !idx || !out || Bq < 0 || kin < 1 || m < 1 || m > kin || alpha < 0 || alpha > EX_ALPHA_MAX || nseg < 0 || C < 1) return COR_EINVAL;
  if (nseg > 0 && (!seg_rows || !seg_offset || !seg_n || !seg_dtype)) return COR_EINVAL;
  if (out_dtype != COR_F32 && out_dtype != COR_BF16 && out_dtype != COR_F16) return COR_EINVAL;
  if (!Q && query_weight != 0.f) return COR_EINVAL;
  if (nseg > EX_SEGMAX) return COR_ENOSUPPORT;                           // (before the arrays are read: they hold nseg entries)
  for (int s = 0; s < nseg; ++s)
    if (seg_entry_bad(seg_n[s], seg_rows[s])) return COR_EINVAL;
  if (m > COR_TOPK_KMAX || C > EX_CMAX || C % 16 != 0) return COR_ENOSUPPORT;
  ExSegs segs = {};
  int sizes = 0;                                                         // bit 0: a segment of 16-bit rows, bit 1: one of fp32 rows
  for (int s = 0; s < nseg; ++s) {
    if (seg_dtype[s] != COR_F32 && seg_dtype[s] != COR_BF16 && seg_dtype[s] != COR_F16) return COR_ENOSUPPORT;
    segs.rows[s] = (const unsigned char*)seg_rows[s];
    segs.off[s] = seg_offset[s];
    segs.n[s] = seg_n[s];
    segs.dt[s] = seg_dtype[s];
    if (seg_n[s] > 0) sizes |= seg_dtype[s] == COR_F32 ? 2 : 1;
  }
  if (Bq == 0) return 0;
  const dim3 grid((unsigned)(((long long)Bq + EX_QPB - 1) / EX_QPB)), block(64 * EX_QPB);
  hipStream_t st = (hipStream_t)stream;
  if (sizes == 3)
    hipLaunchKernelGGL(expand_kernel<0>, grid, block, 0, st, Q, query_weight, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
  else if (sizes == 2)
    hipLaunchKernelGGL(expand_kernel<4>, grid, block, 0, st, Q, query_weight, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
  else
    hipLaunchKernelGGL(expand_kernel<2>, grid, block, 0, st, Q, query_weight, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
  COR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cor_expand_queries_sq(const float* Q, float query_weight, const void* const* seg_rows, const float* const* seg_scale,
                                     const long long* seg_offset, const int* seg_n, const int* seg_dtype, int nseg, const float* scores,
                                     const long long* idx, int Bq, int kin, int m, int C, int alpha, int normalize, void* out, int out_dtype,
                                     void* stream) {
  if (!scores || !idx || !out || Bq < 0 || kin < 1 || m < 1 || m > kin || alpha < 0 || alpha > EX_ALPHA_MAX || nseg < 0 || C < 1) return COR_EINVAL;
  if (nseg > 0 && (!seg_rows || !seg_offset || !seg_n || !seg_dtype)) return COR_EINVAL;
  if (out_dtype != COR_F32 && out_dtype != COR_BF16 && out_dtype != COR_F16) return COR_EINVAL;
  if (!Q && query_weight != 0.f) return COR_EINVAL;
  if (nseg > EX_SEGMAX) return COR_ENOSUPPORT;                           // (before the arrays are read: they hold nseg entries)
  for (int s = 0; s < nseg; ++s)
    if (seg_entry_bad(seg_n[s], seg_rows[s] && (seg_dtype[s] != COR_I8 || (seg_scale && seg_scale[s])))) return COR_EINVAL;
  if (m > COR_TOPK_KMAX || C > EX_CMAX || C % 16 != 0) return COR_ENOSUPPORT;
  ExSegsSq segs = {};
  int sizes = 0;                                                         // bit 0: 16-bit rows, bit 1: fp32 rows, bit 2: int8 rows
  for (int s = 0; s < nseg; ++s) {
    if (seg_dtype[s] != COR_F32 && seg_dtype[s] != COR_BF16 && seg_dtype[s] != COR_F16 && seg_dtype[s] != COR_I8) return COR_ENOSUPPORT;
    segs.rows[s] = (const unsigned char*)seg_rows[s];
    segs.off[s] = seg_offset[s];
    segs.n[s] = seg_n[s];
    segs.dt[s] = seg_dtype[s];
    segs.scale[s] = seg_dtype[s] == COR_I8 && seg_scale ? seg_scale[s] : nullptr;
    if (seg_n[s] > 0) sizes |= seg_dtype[s] == COR_F32 ? 2 : seg_dtype[s] == COR_I8 ? 4 : 1;
  }
  if (Bq == 0) return 0;
  const dim3 grid((unsigned)(((long long)Bq + EX_QPB - 1) / EX_QPB)), block(64 * EX_QPB);
  hipStream_t st = (hipStream_t)stream;
  if (!(sizes & 4)) {                                                    // no int8 row to read: the kernels of cor_expand_queries
    ExSegs fs = {};
    for (int s = 0; s < nseg; ++s) { fs.rows[s] = segs.rows[s]; fs.off[s] = segs.off[s]; fs.n[s] = segs.n[s]; fs.dt[s] = segs.dt[s]; }
    if (sizes == 3)
      hipLaunchKernelGGL(expand_kernel<0>, grid, block, 0, st, Q, query_weight, fs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
    else if (sizes == 2)
      hipLaunchKernelGGL(expand_kernel<4>, grid, block, 0, st, Q, query_weight, fs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
    else
      hipLaunchKernelGGL(expand_kernel<2>, grid, block, 0, st, Q, query_weight, fs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
  } else if (sizes == 4) {
    hipLaunchKernelGGL(expand_sq_kernel<1>, grid, block, 0, st, Q, query_weight, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
  } else {
    hipLaunchKernelGGL(expand_sq_kernel<-1>, grid, block, 0, st, Q, query_weight, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
  }
  COR_CHECK_LAUNCH();
  return 0;
}
