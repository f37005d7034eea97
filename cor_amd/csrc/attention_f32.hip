// cor_amd — flash_fwd_f32: exact-fp32 multi-head attention on the f32-input matrix cores (v_mfma_f32_16x16x4_f32) for gfx950.
//
// Serves the SigLIP towers of the exact-query mode (cor_attention_f32): plain MHA, head_dim 64 / 72 / 80, fp32 q/k/v (column slices
// of the fp32 qkv GEMM output), fp32 online softmax, P kept in fp32. Every product is an exact f32 product summed by the MFMA as a
// k-ordered f32 fma chain, so the error is that of an fp32 evaluation (the fp32 compute mode keeps attn_rowlane: its outputs do not move).
//
// Block = 4 waves = 64 queries of one (sample, head); wave w owns queries 16w .. 16w+15. Keys / values go through LDS in tiles of 64
// (fp32, row stride HD + 4: conflict-free fragment reads). Orientation: the wave computes S^T = K.Q^T per 16-key subtile (A = K from
// LDS, B = Q^T held in registers for the whole launch), so the C/D layout puts the QUERY on the lane (col = lane & 15) and four keys
// in the registers (row = 4 (lane >> 4) + r). The softmax statistics of a query then need only two cross-lane steps (xor 16, 32), and
// O^T = V^T.P^T takes P straight from those registers as its B operand: k-step (t, r) of the product pairs k-index g with key
// 16 t + 4 g + r, and the A operand (V^T) is read from LDS in that same key order. No LDS round trip for P.
// Four independent accumulator chains per product (4 key subtiles for S, 4-5 channel tiles for O) cover the 40-cycle dependent latency
// of the 32-cycle MFMA.
#include "common.h"

namespace {

struct F32AttnArgs {
  const float* q; const float* k; const float* v; void* o;
  long q_sb, q_st, k_sb, k_st, v_sb, v_st, o_sb, o_st;   // element strides: batch, token (o: in elements of the output type)
  int H, Tq, Tk;
  float scale;
};

constexpr int KT = 64;    // keys per LDS tile
constexpr int QB = 64;    // queries per block (4 waves x 16)

template <int HD, bool X3OUT>
__global__ void __launch_bounds__(256) flash_fwd_f32(const F32AttnArgs a) {
  constexpr int LS = HD + 4;              // LDS row stride (floats): LS = 4 (mod 16) words apart per key -> no bank conflicts
  constexpr int NS = HD / 4;              // k-steps of the score product
  constexpr int NC = (HD + 15) / 16;      // 16-channel output tiles (hd 72: the last tile is half padding)
  __shared__ __attribute__((aligned(16))) float Ks[KT * LS];
  __shared__ __attribute__((aligned(16))) float Vs[KT * LS + 16];   // + 16: the padded channels of hd 72 never leave the array
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int col = lane & 15, grp = lane >> 4;
  const int qi = blockIdx.x * QB + wave * 16 + col;       // this lane's query
  const int qrow = min(qi, a.Tq - 1);

  // B operand of S^T = K.Q^T: lane holds Q[query col][4 s + grp] for every k-step s
  float qf[NS];
  {
    const float* qp = a.q + (long)b * a.q_sb + (long)qrow * a.q_st + h * HD + grp;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = qp[4 * s];
  }
  f32x4 oacc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) oacc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                           // running max (per query) and this lane's partial sum of p

  const float* kb = a.k + (long)b * a.k_sb + h * HD;
  const float* vb = a.v + (long)b * a.v_sb + h * HD;
  for (int k0 = 0; k0 < a.Tk; k0 += KT) {
    __syncthreads();                                      // every wave is done with the previous tile
    for (int i = tid; i < KT * (HD / 4); i += 256) {
      const int r = i / (HD / 4), c4 = (i - r * (HD / 4)) * 4, key = k0 + r;
      f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};   // keys past Tk: zeros (masked below; 0 * 0 in the P.V product)
      if (key < a.Tk) {
        kv = *(const f32x4*)(kb + (long)key * a.k_st + c4);
        vv = *(const f32x4*)(vb + (long)key * a.v_st + c4);
      }
      *(f32x4*)(Ks + r * LS + c4) = kv;
      *(f32x4*)(Vs + r * LS + c4) = vv;
    }
    __syncthreads();

    // four partial chains per subtile over consecutive quarters of the head dimension, summed pairwise: a quarter of the fma-chain
    // length per score (the score's rounding error is what exp() amplifies at large logits), 16 independent MFMA chains
    f32x4 sacc[4], part[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) part[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        part[t][s * 4 / NS] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(16 * t + col) * LS + 4 * s + grp], qf[s], part[t][s * 4 / NS], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) sacc[t] = (part[t][0] + part[t][1]) + (part[t][2] + part[t][3]);

    // sacc[t][r] = S[query col][key k0 + 16 t + 4 grp + r]
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sc = (k0 + 16 * t + 4 * grp + r < a.Tk) ? sacc[t][r] * a.scale : -INFINITY;
        sacc[t][r] = sc;
        mx = fmaxf(mx, sc);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);                        // finite: every tile holds at least one real key
    const float alpha = __expf(m - mn);
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(sacc[t][r] - mn);
        sacc[t][r] = p;
        ps += p;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int c = 0; c < NC; ++c) oacc[c] *= alpha;

    // O^T[c][q] += sum_key V[key][c] P[q][key]; k-step (t, r): k-index grp <-> key 16 t + 4 grp + r (lane's own register sacc[t][r])
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vrow = Vs + (16 * t + 4 * grp + r) * LS;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int ch = 16 * c + col;
          const float va = (HD % 16 == 0 || ch < HD) ? vrow[ch] : 0.f;
          oacc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(va, sacc[t][r], oacc[c], 0, 0, 0);
        }
      }
  }

  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qi >= a.Tq) return;
  const float inv = 1.0f / l;
  // oacc[c][r] = O[query col][channel 16 c + 4 grp + r]
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = 16 * c + 4 * grp;
    if (HD % 16 != 0 && ch >= HD) continue;
    const f32x4 o = oacc[c] * inv;
    if constexpr (X3OUT) {
      bf16_t* orow = (bf16_t*)a.o + (long)b * a.o_sb + (long)qi * a.o_st;
      st4_x3(orow, (long)a.H * HD, h * HD + ch, o);
    } else {
      *(f32x4*)((float*)a.o + (long)b * a.o_sb + (long)qi * a.o_st + h * HD + ch) = o;
    }
  }
}

template <int HD>
int launch_f32(const F32AttnArgs& a, int B, int out_dtype, hipStream_t s) {
  const dim3 grid(cdiv(a.Tq, QB), B * a.H), block(256);
  if (out_dtype == COR_F32) hipLaunchKernelGGL((flash_fwd_f32<HD, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((flash_fwd_f32<HD, true>), grid, block, 0, s, a);
  COR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int cor_attention_f32(const float* q, long q_sb, long q_st, const float* k, long k_sb, long k_st, const float* v, long v_sb,
                                 long v_st, void* out, long o_sb, long o_st, int out_dtype, int B, int H, int Tq, int Tk, int hd,
                                 float scale, void* stream) {
  if (!q || !k || !v || !out || B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0 || (long)B * H > 65535) return COR_EINVAL;
  if (out_dtype != COR_F32 && out_dtype != COR_BF16X3) return COR_ENOSUPPORT;
  if (hd != 64 && hd != 72 && hd != 80) return COR_ENOSUPPORT;
  // 16-B loads of k / v rows, 16-B (fp32) or 8-B (x3) stores: strides and bases must allow them
  const long strides = q_sb | q_st | k_sb | k_st | v_sb | v_st | o_sb | o_st;
  if ((strides & 3) || (((uintptr_t)k | (uintptr_t)v) & 15) || ((uintptr_t)out & (out_dtype == COR_F32 ? 15 : 7)) || ((uintptr_t)q & 3))
    return COR_ENOSUPPORT;
  if (out_dtype == COR_BF16X3 && o_st < 3L * H * hd) return COR_EINVAL;
  if (out_dtype == COR_F32 && o_st < (long)H * hd) return COR_EINVAL;
  F32AttnArgs a{q, k, v, out, q_sb, q_st, k_sb, k_st, v_sb, v_st, o_sb, o_st, H, Tq, Tk, scale};
  hipStream_t s = (hipStream_t)stream;
  switch (hd) {
    case 64: return launch_f32<64>(a, B, out_dtype, s);
    case 72: return launch_f32<72>(a, B, out_dtype, s);
    default: return launch_f32<80>(a, B, out_dtype, s);
  }
}
