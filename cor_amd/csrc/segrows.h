// cor_amd — the by-value table of gallery-row segments and everything the calls that read rows through it share (expand.hip,
// diversify.hip, diffuse.hip, cluster.hip, ivf.hip; member_sort.h takes the table from here): the table in its three sizes, the row
// address, the two row loaders, the norm tree, and the host-side checks and fill. Not for rerank.hip, whose tables hold neighbour lists.
//
// Device side. An id (ranklist.h's seg_lookup) or a flat position (member_sort.h's km_locate) is range-tested first; seg_row is called
// inside their on_hit alone and is the only place a row address is formed. Two loaders widen a stored row to fp32, exactly:
//   seg_load8     elements [8s, 8s + 8) by one thread (the fmaf chains of diversify, diffuse and the seeding);
//   seg_lane_*    lane l of a wave holds channels [4l, 4l + 4), a row is ONE coalesced wave load (expand, the k-means chunk sums).
// Arithmetic: every function here that rounds sets `#pragma clang fp contract(off)` for its own body, so an int8 value is
// (float)q * rs, ONE rounded multiply that is never fused into the chain or sum it feeds, whatever the including file sets; the files
// that use the loaders set the same pragma for the whole file.
// Host side, in the order include/cor_amd.h documents for every call: seg_table_check (null arrays -> COR_EINVAL, the segment count ->
// COR_ENOSUPPORT before any array is read, the entries -> COR_EINVAL), then the call's own limits, then seg_table_fill (an unknown
// dtype -> COR_ENOSUPPORT, the table, `seen`).
#pragma once
#include <type_traits>
#include "ranklist.h"

namespace {

constexpr int SEG_MAX = 16;
static_assert(COR_EXPAND_SEGMAX == SEG_MAX && COR_DIVERSIFY_SEGMAX == SEG_MAX && COR_DIFFUSE_SEGMAX == SEG_MAX && COR_CLUSTER_SEGMAX == SEG_MAX,
              "every call that takes a row table takes the one table of this header");
constexpr int SEG_MIXED = -1;                  // kernel variant: the dtype is read per row

// the segment table, passed BY VALUE in the kernel argument block (384 B): no device allocation, no copy, nothing to keep alive
struct SegRows {
  const unsigned char* rows[SEG_MAX];
  long long off[SEG_MAX];
  int n[SEG_MAX];
  int dt[SEG_MAX];
};
// ... with the row scales of COR_I8 segments (512 B)
struct SegRowsSq : SegRows {
  const float* scale[SEG_MAX];
};
// ... and a cell id and a score per row: cor_kmeans_update and cor_ivf_build (768 B)
struct SegRowsAssign : SegRowsSq {
  const int* assign[SEG_MAX];
  const float* score[SEG_MAX];                 // NULL without scores
};
static_assert(sizeof(SegRows) == 384 && sizeof(SegRowsSq) == 512 && sizeof(SegRowsAssign) == 768, "the kernel argument blocks");

// I8 = false: a table without scales holds no int8 rows
template <bool I8 = true> __host__ __device__ __forceinline__ int seg_esize(int dt) { return dt == COR_F32 ? 4 : I8 && dt == COR_I8 ? 1 : 2; }

// (dtype, row address, row scale) of local row `local` of segment s; called only from the on_hit of seg_lookup / km_locate
template <typename Segs> __device__ __forceinline__ void seg_row(const Segs& segs, int s, u64 local, int C, int& dt, u64& row, float& rs) {
  constexpr bool SQ = std::is_base_of<SegRowsSq, Segs>::value;
  dt = segs.dt[s];
  row = (u64)segs.rows[s] + local * (u64)(C * seg_esize<SQ>(dt));
  if constexpr (SQ) {
    if (dt == COR_I8) rs = segs.scale[s][local];                           // fetched by the thread that looked the row up
  }
}

// row addresses travel as integers (v_readlane halves, LDS slots); the loads name the GLOBAL address space, so they are global_load
// (scalar base + lane offset), not flat_load
#define SEG_GLOBAL __attribute__((address_space(1)))
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------------- 8 elements per thread

// one chunk of a chain (8 elements) as stored, w[0 .. 2 esize), -> fp32 values: fp32 as stored, bf16 / fp16 widened exactly, int8
// (float)q * rs (one rounded multiply). DT >= 0: the dtype of every row; SEG_MIXED: `dt` decides
template <int DT> __device__ __forceinline__ void seg_widen8(const unsigned (&w)[8], int dt, float rs, float (&g)[8]) {
#pragma clang fp contract(off)
  const int d = DT >= 0 ? DT : dt;
  if (d == COR_F32) {
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = __uint_as_float(w[e]);
  } else if (d == COR_I8) {
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = (float)(int)(signed char)(w[e >> 2] >> (8 * (e & 3))) * rs;
  } else if (d == COR_BF16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { g[2 * e] = __uint_as_float(w[e] << 16); g[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = (float)__builtin_bit_cast(_Float16, (unsigned short)(e & 1 ? w[e >> 1] >> 16 : w[e >> 1] & 0xffffu));
  }
}

// elements [8 s, 8 s + 8) of a row in global memory, as fp32 values: two 16-byte loads (fp32), one (16-bit) or one 8-byte load (int8);
// rows are 16-byte aligned and C % 16 == 0. With SEG_MIXED the dtype may differ between the threads of a wave. Every dtype converts
// straight out of its own load: through seg_widen8 (one load per element size, then the conversions) a table of ONE dtype compiles to
// the same code, a SEG_MIXED kernel to other code (DESIGN.md has the kernels and what they measured)
template <int DT> __device__ __forceinline__ void seg_load8(u64 row, int dt, float rs, int s, float (&g)[8]) {
#pragma clang fp contract(off)
  const int d = DT >= 0 ? DT : dt;
  if (d == COR_F32) {
    const u32x4 x = *(const SEG_GLOBAL u32x4*)(row + 32u * s), y = *(const SEG_GLOBAL u32x4*)(row + 32u * s + 16u);
#pragma unroll
    for (int e = 0; e < 4; ++e) { g[e] = __uint_as_float(x[e]); g[4 + e] = __uint_as_float(y[e]); }
  } else if (d == COR_I8) {
    const u32x2 x = *(const SEG_GLOBAL u32x2*)(row + 8u * s);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = (float)(int)(signed char)(x[e >> 2] >> (8 * (e & 3))) * rs;
  } else if (d == COR_BF16) {
    const u32x4 x = *(const SEG_GLOBAL u32x4*)(row + 16u * s);
#pragma unroll
    for (int e = 0; e < 4; ++e) { g[2 * e] = __uint_as_float(x[e] << 16); g[2 * e + 1] = __uint_as_float(x[e] & 0xffff0000u); }
  } else {
    const u32x4 x = *(const SEG_GLOBAL u32x4*)(row + 16u * s);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = (float)__builtin_bit_cast(_Float16, (unsigned short)(e & 1 ? x[e >> 1] >> 16 : x[e >> 1] & 0xffffu));
  }
}

// ---------------------------------------------------------------------------------------------------------------- 4 channels per lane

// the lane's four channels [c0, c0 + 4) of one row, as stored. ESZ = 4 / 2: every segment has rows of that element size; ESZ = 0: fp32 and
// 16-bit segments together, two 8-byte loads whose second one repeats the first for a 16-bit row (no branch around a load); ESZ = 1:
// every segment holds int8 rows, the lane's four channels are ONE dword (C = 256: a row is one 256-byte wave load); ESZ = -1: int8 and
// float segments together: a dword, a second dword and an 8-byte load at offsets chosen by the dtype, every one inside the row (an
// int8 row's second and third load repeat bytes the lane does not use), again no branch around a load
template <int ESZ> __device__ __forceinline__ u32x4 seg_lane_load(u64 row, int c0, int dt) {
  u32x4 r = {0u, 0u, 0u, 0u};
  if constexpr (ESZ == 4) {
    r = *(const SEG_GLOBAL u32x4*)(row + 4u * c0);
  } else if constexpr (ESZ == 1) {
    r[0] = *(const SEG_GLOBAL unsigned*)(row + (unsigned)c0);
  } else if constexpr (ESZ == -1) {
    const bool wide = dt == COR_F32, narrow = dt == COR_I8;
    const unsigned o = wide ? 4u * c0 : narrow ? (unsigned)c0 : 2u * c0;
    const unsigned a = *(const SEG_GLOBAL unsigned*)(row + o), b = *(const SEG_GLOBAL unsigned*)(row + o + (narrow ? 0u : 4u));
    const u32x2 c = *(const SEG_GLOBAL u32x2*)(row + (wide ? o + 8u : narrow ? (unsigned)c0 & ~7u : o));
    r[0] = a; r[1] = b; r[2] = c[0]; r[3] = c[1];
  } else if constexpr (ESZ == 2) {
    const u32x2 a = *(const SEG_GLOBAL u32x2*)(row + 2u * c0);
    r[0] = a[0]; r[1] = a[1];
  } else {
    const bool wide = dt == COR_F32;
    const unsigned o = wide ? 4u * c0 : 2u * c0;
    const u32x2 a = *(const SEG_GLOBAL u32x2*)(row + o), b = *(const SEG_GLOBAL u32x2*)(row + o + (wide ? 8u : 0u));
    r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1];
  }
  return r;
}

// stored values -> fp32, exactly (dt is wave-uniform); an int8 row's value is (float)q * rs, rs the row's scale: one rounded multiply
template <int ESZ> __device__ __forceinline__ void seg_lane_widen(const u32x4 r, int dt, float rs, float (&x)[4]) {
#pragma clang fp contract(off)
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

// the next U set bits of `mask` (lowest first = list order): entry j's row address (plo, phi), weight w, scale rs and dtype come out of
// lane j by v_readlane, all U rows are requested before the first use, then use(w_j, x_j) follows in list order
template <int ESZ, int U, typename Use>
__device__ __forceinline__ void seg_lane_group(u64& mask, unsigned plo, unsigned phi, float w, float rs, int dt, int c0, const Use use) {
  u32x4 raw[U];
  float wu[U], su[U];
  int du[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = __builtin_ctzll(mask);                                   // mask has at least U bits set (the caller counted them)
    mask &= mask - 1;
    const u64 row = ((u64)(unsigned)__builtin_amdgcn_readlane((int)phi, j) << 32) | (unsigned)__builtin_amdgcn_readlane((int)plo, j);
    wu[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), j));
    du[u] = __builtin_amdgcn_readlane(dt, j);
    su[u] = 0.f;
    if constexpr (ESZ == 1 || ESZ == -1) su[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rs), j));   // travels with the weight
    raw[u] = seg_lane_load<ESZ>(row, c0, du[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float x[4];
    seg_lane_widen<ESZ>(raw[u], du[u], su[u], x);
    use(wu[u], x);
  }
}
// the present entries of the wave's 64 in list order, 8 at a time, then 4, 2, 1 for what is left; a missing entry costs and loads nothing
template <int ESZ, typename Use>
__device__ __forceinline__ void seg_lane_walk(bool present, u64 row, float w, float rs, int dt, int c0, const Use use) {
  u64 mask = __ballot(present);
  int cnt = __builtin_popcountll(mask);
  const unsigned plo = (unsigned)row, phi = (unsigned)(row >> 32);
  for (; cnt >= 8; cnt -= 8) seg_lane_group<ESZ, 8>(mask, plo, phi, w, rs, dt, c0, use);
  if (cnt & 4) seg_lane_group<ESZ, 4>(mask, plo, phi, w, rs, dt, c0, use);
  if (cnt & 2) seg_lane_group<ESZ, 2>(mask, plo, phi, w, rs, dt, c0, use);
  if (cnt & 1) seg_lane_group<ESZ, 1>(mask, plo, phi, w, rs, dt, c0, use);
}

// the norm of a wave's row v (lane l: channels [4l, 4l + 4), `active` = 4l < C) -> d = max(sqrt(sum of squares), 1e-12), the sum by the
// stride-halving tree over 256 channel slots: s = v * v per channel (+0 in the lanes past C / 4); s[c] += s[c + h], h = 128 .. 1, is 6
// lane exchanges at distance h / 4 = 32 .. 1 on the lane's four values, then s[0] += s[2], s[1] += s[3], s[0] += s[1] inside lane 0
__device__ __forceinline__ float seg_lane_norm(const float (&v)[4], bool active) {
#pragma clang fp contract(off)
  float s[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) s[e] = active ? v[e] * v[e] : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                                       // h = 4 o: channel c + h lives in lane l + o, same slot
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = s[e] + __shfl_xor(s[e], o, 64);     // lanes < o hold the tree's values (l ^ o = l + o there)
  }
  s[0] = s[0] + s[2];                                                      // h = 2
  s[1] = s[1] + s[3];
  s[0] = s[0] + s[1];                                                      // h = 1
  const float s0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s[0])));
  return fmaxf(__builtin_sqrtf(s0), 1e-12f);
}

// ---------------------------------------------------------------------------------------------------------------- host

// the arrays of a call's table as the caller passed them; i8: the call takes COR_I8 segments (with their scales); with_assign: it takes a
// cell id per row. scale / assign / score may be NULL where the call's contract lets them
struct SegArrays {
  const void* const* rows;
  const float* const* scale;
  const long long* off;
  const int* n;
  const int* dtype;
  int nseg;                                                                // >= 0 (the caller's own checks)
  bool i8;
  const int* const* assign;
  bool with_assign;
  const float* const* score;
};

// in front of the call's own limits: null arrays -> COR_EINVAL, nseg > SEG_MAX -> COR_ENOSUPPORT (before the arrays are read: they hold
// nseg entries), an entry with n < 0, or with rows and a pointer missing -> COR_EINVAL
inline int seg_table_check(const SegArrays& a) {
  if (a.nseg > 0 && (!a.rows || !a.off || !a.n || !a.dtype || (a.with_assign && !a.assign))) return COR_EINVAL;
  if (a.nseg > SEG_MAX) return COR_ENOSUPPORT;
  for (int s = 0; s < a.nseg; ++s)
    if (seg_entry_bad(a.n[s], a.rows[s] && (!a.i8 || a.dtype[s] != COR_I8 || (a.scale && a.scale[s])) && (!a.with_assign || a.assign[s]) &&
                                  (!a.score || a.score[s])))
      return COR_EINVAL;
  return 0;
}

// behind them: an unknown dtype -> COR_ENOSUPPORT; else the table (drop_empty: of the non-empty segments alone, in table order), -> live =
// the segments it holds, seen = bit dt for every non-empty segment of that dtype
template <typename Segs> inline int seg_table_fill(const SegArrays& a, bool drop_empty, Segs& segs, int& live, int& seen) {
  segs = Segs{};
  live = seen = 0;
  for (int s = 0; s < a.nseg; ++s) {
    const int dt = a.dtype[s];
    if (dt != COR_F32 && dt != COR_BF16 && dt != COR_F16 && !(a.i8 && dt == COR_I8)) return COR_ENOSUPPORT;
    if (a.n[s] > 0) seen |= 1 << dt;
    else if (drop_empty) continue;
    segs.rows[live] = (const unsigned char*)a.rows[s];
    segs.off[live] = a.off[s];
    segs.n[live] = a.n[s];
    segs.dt[live] = dt;
    if constexpr (std::is_base_of<SegRowsSq, Segs>::value) segs.scale[live] = dt == COR_I8 && a.scale ? a.scale[s] : nullptr;
    if constexpr (std::is_base_of<SegRowsAssign, Segs>::value) {
      segs.assign[live] = a.with_assign ? a.assign[s] : nullptr;
      segs.score[live] = a.score ? a.score[s] : nullptr;
    }
    ++live;
  }
  return 0;
}

// seen -> launch(the table's one storage dtype as a std::integral_constant, or SEG_MIXED); no rows at all: every entry is missing
template <typename Launch> inline int seg_dispatch_dtype(int seen, const Launch launch) {
  switch (seen) {
    case 0:
    case 1 << COR_F32: return launch(std::integral_constant<int, COR_F32>{});
    case 1 << COR_BF16: return launch(std::integral_constant<int, COR_BF16>{});
    case 1 << COR_F16: return launch(std::integral_constant<int, COR_F16>{});
    case 1 << COR_I8: return launch(std::integral_constant<int, COR_I8>{});
    default: return launch(std::integral_constant<int, SEG_MIXED>{});
  }
}

}  // namespace
