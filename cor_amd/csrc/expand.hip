// cor_amd — query expansion / database-side augmentation (cor_expand_queries): per query the weighted sum of the first m rows its list
// names, plus the weighted query, optionally L2-normalised. Contract and the definition, fixed to the bit: include/cor_amd.h.
//
// One wave per query, EX_QPB = 4 queries per 256-thread block; there is no block-level cooperation, hence no barrier and no LDS.
//   Lane l owns channels [4l, 4l + 4): a row is ONE coalesced wave load, 16 B per lane for fp32 rows and 8 B for 16-bit rows (C = 256: all
//   64 lanes; smaller C: the lanes past C / 4 re-read channels 0..3, stay out of the tree and store nothing, so no load or store is masked).
//   The table, the row address, the lane loader and the norm tree are segrows.h's, shared with the other calls that read gallery rows.
//   1. List. 64 entries at a time, lane j takes entry j: its id is looked up in the segment table (ranklist.h's seg_lookup: the range test
//      comes first) and only a hit forms the row address; the entry's weight w = max(score, +0)^alpha
//      is computed there too (alpha dependent multiplies). The segment table is a by-value kernel argument, read with scalar loads.
//   2. Rows. A ballot gives the present entries of the 64; they are walked in list order, lowest set bit first, 8 at a time (then 4, 2,
//      1 for what is left): the entry's row address, weight and dtype come out of lane j by v_readlane, the loads of the whole group are
//      issued, then the group's products and sums follow in list order. A missing entry costs nothing and loads nothing.
//   3. Norm. The stride-halving tree over 256 channel slots (seg_lane_norm), then v / d.
// cor_expand_queries_sq is the same body over the table that also carries the row scales of int8 segments: an int8 row is 4 B per lane (one
// dword), its value (float)q * scale, one rounded multiply, the scale fetched in step 1 by the lane that looked the id up. Without an
// int8 segment it launches the kernels of cor_expand_queries.
// Arithmetic: every operation is one separately rounded IEEE fp32 operation. `#pragma clang fp contract(off)` below holds for the whole
// file: HIP's __fmul_rn / __fadd_rn are plain * and + (contractible under the default -ffp-contract=fast) and its __fsqrt_rn is the
// APPROXIMATE native square root, so none of them is used here; a / b and __builtin_sqrtf are correctly rounded in a build without
// fast-math flags (-fhip-fp32-correctly-rounded-divide-sqrt is the default), and the Makefile adds no such flag for this file.
#include "segrows.h"

#pragma clang fp contract(off)

namespace {

constexpr int EX_QPB = 4;        // queries (waves) per block
constexpr int EX_CMAX = 256;     // 64 lanes x 4 channels
constexpr int EX_ALPHA_MAX = 8;

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
    if (j < m) {                                                         // (the only place a row address is formed)
      present = seg_lookup(segs, nseg, ids[j], [&](int s, u64 local) { seg_row(segs, s, local, C, dt, row, rs); });
      if (present) {                                                     // a missing entry's score is never read
        const float t0 = sc[j];
        const float t = t0 > 0.f ? t0 : 0.f;                             // NaN, -0.0 and negatives: +0
        w = 1.f;
        for (int a = 0; a < alpha; ++a) w = w * t;
      }
    }
    // 2. the present entries in list order
    seg_lane_walk<ESZ>(present, row, w, rs, dt, c0, [&](float wj, const float (&x)[4]) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] + (wj * x[e]);
    });
  }

  // 3. the norm
  if (normalize) {
    const float d = seg_lane_norm(v, active);
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
__global__ __launch_bounds__(64 * EX_QPB) void expand_kernel(const float* __restrict__ Q, float qw, const SegRows segs, int nseg,
                                                             const float* __restrict__ scores, const long long* __restrict__ idx, int Bq,
                                                             int kin, int m, int C, int alpha, int normalize, void* __restrict__ out,
                                                             int out_dtype) {
  expand_body<ESZ>(Q, qw, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
}
// the table with row scales: ESZ = 1 (int8 segments alone) or -1 (int8 and float segments together)
template <int ESZ>
__global__ __launch_bounds__(64 * EX_QPB) void expand_sq_kernel(const float* __restrict__ Q, float qw, const SegRowsSq segs, int nseg,
                                                                const float* __restrict__ scores, const long long* __restrict__ idx, int Bq,
                                                                int kin, int m, int C, int alpha, int normalize, void* __restrict__ out,
                                                                int out_dtype) {
  expand_body<ESZ>(Q, qw, segs, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype);
}

// both calls; t.i8: the table may hold COR_I8 segments (cor_expand_queries_sq)
int expand_queries(const float* Q, float query_weight, const SegArrays& t, const float* scores, const long long* idx, int Bq, int kin, int m, int C,
                   int alpha, int normalize, void* out, int out_dtype, void* stream) {
  if (!scores || !idx || !out || Bq < 0 || kin < 1 || m < 1 || m > kin || alpha < 0 || alpha > EX_ALPHA_MAX || t.nseg < 0 || C < 1) return COR_EINVAL;
  if (out_dtype != COR_F32 && out_dtype != COR_BF16 && out_dtype != COR_F16) return COR_EINVAL;
  if (!Q && query_weight != 0.f) return COR_EINVAL;
  if (const int rc = seg_table_check(t)) return rc;
  if (m > COR_TOPK_KMAX || C > EX_CMAX || C % 16 != 0) return COR_ENOSUPPORT;
  SegRowsSq segs;
  int nseg = 0, seen = 0;
  if (const int rc = seg_table_fill(t, false, segs, nseg, seen)) return rc;
  if (Bq == 0) return 0;
  const dim3 grid((unsigned)(((long long)Bq + EX_QPB - 1) / EX_QPB)), block(64 * EX_QPB);
  hipStream_t st = (hipStream_t)stream;
#define EX_LAUNCH(KERNEL, TABLE) \
  hipLaunchKernelGGL(KERNEL, grid, block, 0, st, Q, query_weight, TABLE, nseg, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype)
  constexpr int F32 = 1 << COR_F32, I8 = 1 << COR_I8;
  const SegRows& fs = segs;                                              // no int8 row to read: the table without the scales
  if (seen == I8) EX_LAUNCH(expand_sq_kernel<1>, segs);
  else if (seen & I8) EX_LAUNCH(expand_sq_kernel<-1>, segs);
  else if (seen == F32) EX_LAUNCH(expand_kernel<4>, fs);
  else if (seen & F32) EX_LAUNCH(expand_kernel<0>, fs);
  else EX_LAUNCH(expand_kernel<2>, fs);
#undef EX_LAUNCH
  COR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int cor_expand_queries(const float* Q, float query_weight, const void* const* seg_rows, const long long* seg_offset, const int* seg_n,
                                  const int* seg_dtype, int nseg, const float* scores, const long long* idx, int Bq, int kin, int m, int C, int alpha,
                                  int normalize, void* out, int out_dtype, void* stream) {
  const SegArrays t = {seg_rows, nullptr, seg_offset, seg_n, seg_dtype, nseg, false};
  return expand_queries(Q, query_weight, t, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype, stream);
}

extern "C" int cor_expand_queries_sq(const float* Q, float query_weight, const void* const* seg_rows, const float* const* seg_scale,
                                     const long long* seg_offset, const int* seg_n, const int* seg_dtype, int nseg, const float* scores,
                                     const long long* idx, int Bq, int kin, int m, int C, int alpha, int normalize, void* out, int out_dtype,
                                     void* stream) {
  const SegArrays t = {seg_rows, seg_scale, seg_offset, seg_n, seg_dtype, nseg, true};
  return expand_queries(Q, query_weight, t, scores, idx, Bq, kin, m, C, alpha, normalize, out, out_dtype, stream);
}
