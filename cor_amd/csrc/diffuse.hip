// cor_amd — diffusion re-ranking of candidate lists (cor_rerank_diffusion): manifold ranking (Zhou et al., NIPS 2003; Iscen et al., CVPR 2017)
// on the mutual k-nearest-neighbour graph of a query's candidates. Per query: the chain similarities of all pairs of present entries,
// raised to the power gamma, give each entry its kd best neighbours; the mutual ones form a symmetric graph whose edges are normalised
// by the degrees; `iters` Jacobi steps f <- alpha S f + (1 - alpha) y spread the scores of the query's kq best entries over it; the entries
// are ranked by f. Contract and the definition, fixed to the bit: include/cor_amd.h.
//
// One launch, one block per query, T = max(64, npad) threads (npad = kin rounded up to a power of two, kin <= 256): one thread per
// candidate. No global workspace and no Gram matrix: the full n x n set of chains is computed (not the upper triangle: with one row per
// thread the triangle leaves the waves as unbalanced as the full square is long), and a row of affinities lives only as
// long as the tile it was computed in. The state is in dynamic LDS, sized by (T, C, kd): 84 KiB at kin = 256, C = 256, kd = 32, 54 KiB at kd = 8.
//   0. Presence. Every id is looked up in the segment table (ranklist.h's seg_lookup: the range test comes first); only a hit forms a
//      row address and reads its score. The present entries are numbered p = 0 .. n-1 in list order (ballot + wave sums) and their
//      row address, scale, dtype, position and y = pw(score) (p < kq) go to LDS slot p. From here on thread p IS entry p.
//   1. Chains and neighbour selection, DF_TP = 32 partner rows at a time: the block widens the partner rows into an LDS tile of 32 C
//      floats ([chunk][pair of rows][place in the chain][row of the pair], so that one 16-byte broadcast read holds two steps of the
//      chains of two partners, side by side as a packed fma wants them); then thread p walks C in the chain's order
//      (oracle/c/sim_chain.c: chunk c of 8, k = 8c+i then 8c+4+i), its own row coming 8 channels at a time from global memory / L2, one
//      chunk ahead of its use, against 16 pairs of accumulators in registers, four pairs (16 reads, 32 packed fmas in four independent
//      chains) at a time. After the tile a = pw(chain) of every partner p' != p with a > 0 is offered to the thread's neighbour list: at
//      most kd (a, p') pairs sorted by (a desc, p' asc). Partners arrive in ascending p', so a newcomer goes behind every pair with a
//      value >= a, and a full list takes only a > its last value. Two variants: kd <= 8 keeps the list in 8 + 8 registers (a carry
//      walks down the list, no memory, no divergent loop) and writes it to LDS once, behind the last tile; a larger kd keeps it in LDS
//      column p ([kd][T], so that the lanes of a wave touch different banks) and shifts there. (32 + 32 registers for kd = 32 compiled
//      to 245 VGPRs, 16 to 33 spilled SGPRs and half a megabyte of code per kernel: not shipped.) At kin = 256, C = 256 the LDS lists
//      cost 5 times the chains at kd = 32; the register lists a tenth of them at kd = 8.
//   2. Mutual test. p is in N(p') exactly if N(p') is not full, or (a, p) does not rank behind N(p')'s last pair; since sim is bitwise
//      symmetric a(p', p) is the a the thread holds. Every thread publishes (count, last value, last index), barrier, then keeps the
//      mutual members of its own column in place, order kept, and sums its degree in that order. r = 1 / sqrtf(d) through LDS, barrier,
//      and the column's values become the edge weights a * (r_p * r_p').
//   3. iters Jacobi steps over two f vectors in LDS, a barrier per step: g = fmaf(S, f[p'], g) down the column, then
//      (alpha * g) + ((1 - alpha) * y).
//   4. Rank: ranklist.h's keys [f key | list position], block_bitonic_sort with the id read on ties, the first min(n, k) ranks go out,
//      rank_fill_tail writes the rest. f is never negative and never -0.0 (sums and products of values >= +0), so the key carries no -0.0
//      flag, and (id asc, position asc) is RankBefore's order as it stands.
// Arithmetic: `#pragma clang fp contract(off)` holds for the whole file, so every * and + of the definition is rounded on its own and
// an int8 value's (float)q * scale is never fused into the chain; the chain's and the iteration's explicit fmaf stay an fma.
// 1.0f / sqrtf(d) must be the two correctly rounded IEEE operations: hipcc's default for HIP code is (the expansion around v_sqrt_f32, and
// v_div_scale / v_div_fmas / v_div_fixup). NO FLAG MAY CHANGE THAT: this file is built without -ffast-math, -fno-hip-fp32-correctly-
// rounded-divide-sqrt, -fapprox-func or any denormal-flushing option (cor_amd/csrc/Makefile gives it no FLAGS_ line).
// The segment table, the row address and the row loader are segrows.h's, shared with the other calls that read gallery rows.
#include "segrows.h"

#pragma clang fp contract(off)

namespace {

constexpr int DF_NMAX = COR_DIFFUSE_NMAX;
constexpr int DF_KDMAX = COR_DIFFUSE_KDMAX;
constexpr int DF_CMAX = 256;                   // embedding width limit of the searches
constexpr int DF_TP = 32;                      // partner rows per tile = chain accumulators per thread
constexpr int DF_KD_SMALL = 8;                // kernel variants: kd <= 8 keeps a thread's neighbour list in 8 + 8 registers, a larger kd in LDS
constexpr int DF_JB = 4;                      // pairs of partner rows whose chains a thread advances side by side
static_assert(DF_NMAX <= 256, "neighbour indices are stored as bytes and a block has one thread per candidate");
static_assert(DF_NMAX <= COR_MERGE_NMAX, "the rank keys carry the list position");

// the scalars of the definition
struct DfParams {
  int kin, C, kd, kq, gamma, iters, k;
  float alpha;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// pw(v): +0 unless v > 0, else v multiplied gamma - 1 times by v, each product rounded
__device__ __forceinline__ float df_pw(float v, int gamma) {
  if (!(v > 0.f)) return 0.f;
  float w = v;
  for (int e = 1; e < gamma; ++e) w = w * v;
  return w;
}

// dynamic LDS of a block of T threads, in this order (every array 16-byte aligned: T % 64 == 0, C % 16 == 0)
__host__ __device__ inline size_t df_lds_bytes(int T, int C, int kd) {
  return (size_t)T * (8 + 8) + (size_t)DF_TP * C * 4 + (size_t)kd * T * 4 + (size_t)T * 4 * 8 + (size_t)kd * T + (size_t)T;
}

template <int DT, int KD>
__global__ __launch_bounds__(256) void rerank_diffusion_kernel(const SegRowsSq segs, int nseg, const float* __restrict__ scores,
                                                               const long long* __restrict__ idx, const DfParams P,
                                                               unsigned* __restrict__ out_scores, long long* __restrict__ out_idx,
                                                               int* __restrict__ out_pos) {
  extern __shared__ __align__(16) unsigned char df_lds[];
  __shared__ int s_wcount[4];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
  const int kin = P.kin, C = P.C, kd = P.kd;
  u64* e_row = (u64*)df_lds;                                         // [T] slot p: the row's address
  u64* key = e_row + T;                                              // [T] the rank keys of step 4
  float* tile = (float*)(key + T);                                   // [C / 8][DF_TP / 2][8][2] the partner rows of a tile, widened: chunk, pair of rows, place in the chain, row of the pair
  float* nbv = tile + DF_TP * C;                                     // [kd][T] column p: N(p)'s values, then M(p)'s, then the edge weights
  float* e_rs = nbv + kd * T;                                        // [T] row scale (int8 rows)
  float* e_y = e_rs + T;                                             // [T] the query vector
  float* e_r = e_y + T;                                              // [T] 1 / sqrt(degree)
  float* fa = e_r + T;                                               // [T] f, double buffered
  float* fb = fa + T;
  float* lastv = fb + T;                                             // [T] the last value of N(p)
  int* e_pos = (int*)(lastv + T);                                    // [T] the entry's position in the list
  int* cntlast = e_pos + T;                                          // [T] |N(p)| | the last index of N(p) << 8
  unsigned char* nbi = (unsigned char*)(cntlast + T);                // [kd][T] column p: the indices p' that go with nbv
  unsigned char* e_dt = nbi + kd * T;                                // [T] storage dtype of the row
  const long long* ids = idx + (long long)blockIdx.x * kin;
  const float* sc = scores + (long long)blockIdx.x * kin;
  const long long out0 = (long long)blockIdx.x * P.k;

  // 0. presence, and the present entries numbered in list order
  int n;
  {
    int dt = COR_F32;
    u64 r = 0;
    float sr = 0.f;
    bool present = false;
    if (tid < kin)
      present = seg_lookup(segs, nseg, ids[tid], [&](int sg, u64 local) { seg_row(segs, sg, local, C, dt, r, sr); });   // the only place a row address is formed
    const unsigned long long bal = __ballot(present);
    if (lane == 0) s_wcount[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < nwaves; ++w) {
      const int v = s_wcount[w];
      if (w < wave) before += v;
      total += v;
    }
    n = total;
    if (present) {
      const int p = before + __popcll(bal & ((1ull << lane) - 1ull));
      e_row[p] = r; e_rs[p] = sr; e_dt[p] = (unsigned char)dt; e_pos[p] = tid;
      e_y[p] = p < P.kq ? df_pw(sc[tid], P.gamma) : 0.f;                        // a missing entry's score is never read
    }
    __syncthreads();
  }
  const int p = tid;
  const bool act = p < n;                                            // this thread is entry p

  // 1. chains against DF_TP partner rows at a time, and the kd best neighbours of every entry
  constexpr int KR = KD > 0 ? KD : 1;
  float nv[KR];                                                      // KD > 0: N(p), sorted by (a desc, p' asc), in registers; 0 = an empty place (a > 0 always)
  int nq[KR];
#pragma unroll
  for (int i = 0; i < KR; ++i) { nv[i] = 0.f; nq[i] = 0; }
  float thr = 0.f;                                                   // N(p)'s kd-th value: what a newcomer must beat (0 while the list is not full)
  int cnt = 0;                                                       // KD == 0: |N(p)|, the list being column p of nbv / nbi
  {
    const u64 myrow = act ? e_row[p] : 0;
    const float myrs = act ? e_rs[p] : 0.f;
    const int mydt = act ? e_dt[p] : COR_F32;
    const int chunks = C >> 3;
    for (int t0 = 0; t0 < n; t0 += DF_TP) {
      for (int e = tid; e < DF_TP * chunks; e += T) {
        const int s = e / DF_TP, r = e - s * DF_TP, q = t0 + r;      // (DF_TP is a power of two)
        float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (q < n) seg_load8<DT>(e_row[q], e_dt[q], e_rs[q], s, g);  // rows past n: zeros, never used
        // tile[s][r / 2][t][r % 2], t the place of the element in the chain's order (8 c + i, then 8 c + 4 + i): float offset 16 (s 16 + r / 2) + 2 t + r % 2
        float* dst = tile + 16 * (s * (DF_TP / 2) + (r >> 1)) + (r & 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dst[4 * i] = g[i];
          dst[4 * i + 2] = g[4 + i];
        }
      }
      __syncthreads();
      f32x2 acc2[DF_TP / 2];
#pragma unroll
      for (int j = 0; j < DF_TP / 2; ++j) acc2[j] = f32x2{0.f, 0.f};
      if (act) {
        float g[8];
        seg_load8<DT>(myrow, mydt, myrs, 0, g);
        for (int c = 0; c < chunks; ++c) {
          float gn[8];                                               // the next chunk of the own row is on its way while this one is used
          seg_load8<DT>(myrow, mydt, myrs, c + 1 < chunks ? c + 1 : c, gn);
          const f32x4* tq = (const f32x4*)tile + 4 * (DF_TP / 2) * c;
#pragma unroll
          for (int jb = 0; jb < DF_TP / 2; jb += DF_JB) {            // DF_JB pairs of partners at a time: independent chains side by side
            f32x4 q[DF_JB][4];
#pragma unroll
            for (int u = 0; u < DF_JB; ++u)
#pragma unroll
              for (int v = 0; v < 4; ++v) q[u][v] = tq[4 * (jb + u) + v];
#pragma unroll
            for (int t = 0; t < 8; ++t) {                            // the chain's order: element 8 c + (t & 1) * 4 + t / 2
              const float gv = g[(t & 1) * 4 + (t >> 1)];
#pragma unroll
              for (int u = 0; u < DF_JB; ++u) {
                const f32x2 qq = {q[u][t >> 1][2 * (t & 1)], q[u][t >> 1][2 * (t & 1) + 1]};
                acc2[jb + u] = __builtin_elementwise_fma(f32x2{gv, gv}, qq, acc2[jb + u]);   // two fmaf, one per partner of the pair
              }
            }
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) g[e] = gn[e];
        }
      }
      float acc[DF_TP];
#pragma unroll
      for (int j = 0; j < DF_TP; ++j) acc[j] = acc2[j >> 1][j & 1];
      __syncthreads();                                               // the tile has been read: the next turn may overwrite it
      if (act) {
#pragma unroll
        for (int j = 0; j < DF_TP; ++j) {
          const int q = t0 + j;
          const float a = df_pw(acc[j], P.gamma);
          if (q < n && q != p && a > thr) {                          // (thr >= 0, so a > 0)
            if constexpr (KD > 0) {
              float ca = a;                                          // carried down the list: it takes the place of the first smaller value
              int cq = q;                                            // (strictly smaller: partners come in ascending p'); from there on every
              bool sw = false;                                       // pair moves one place down, equal values included
#pragma unroll
              for (int i = 0; i < KD; ++i) {
                sw = sw || ca > nv[i];
                const float tv = nv[i];
                const int tq = nq[i];
                nv[i] = sw ? ca : tv; nq[i] = sw ? cq : tq;
                ca = sw ? tv : ca; cq = sw ? tq : cq;
                if (i == kd - 1) thr = nv[i];                        // places past kd - 1 hold what fell out: never read
              }
            } else {
              int i = cnt < kd ? cnt : kd - 1;                       // a full list loses its last pair
              while (i > 0) {
                const float v = nbv[(i - 1) * T + p];
                if (!(v < a)) break;                                 // behind every pair with a value >= a: partners come in ascending p'
                nbv[i * T + p] = v;
                nbi[i * T + p] = nbi[(i - 1) * T + p];
                --i;
              }
              nbv[i * T + p] = a;
              nbi[i * T + p] = (unsigned char)q;
              if (cnt < kd) ++cnt;
              if (cnt == kd) thr = nbv[(kd - 1) * T + p];
            }
          }
        }
      }
    }
  }
  if constexpr (KD > 0) {
    if (act) {
#pragma unroll
      for (int i = 0; i < KD; ++i)
        if (i < kd) {
          nbv[i * T + p] = nv[i];
          nbi[i * T + p] = (unsigned char)nq[i];
          cnt += nv[i] > 0.f;
        }
    }
  }

  // 2. the mutual graph, the degrees and the edge weights
  if (act) {
    cntlast[p] = cnt | (cnt ? (int)nbi[(cnt - 1) * T + p] << 8 : 0);
    lastv[p] = cnt ? nbv[(cnt - 1) * T + p] : 0.f;
  }
  __syncthreads();
  int m = 0;
  if (act) {
    float d = 0.f;
    for (int i = 0; i < cnt; ++i) {
      const float a = nbv[i * T + p];
      const int q = nbi[i * T + p];                                  // < n: written from a partner index
      const int cl = cntlast[q], qcnt = cl & 0xff, qlast = cl >> 8;
      const float qv = lastv[q];
      if (qcnt < kd || a > qv || (a == qv && p <= qlast)) {          // p is in N(q): a(q, p) has the bits of a
        nbv[m * T + p] = a;
        nbi[m * T + p] = (unsigned char)q;
        d = d + a;
        ++m;
      }
    }
    e_r[p] = d > 0.f ? 1.0f / sqrtf(d) : 0.f;
    fa[p] = e_y[p];
  }
  __syncthreads();
  if (act) {
    const float rp = e_r[p];
    for (int i = 0; i < m; ++i) nbv[i * T + p] = nbv[i * T + p] * (rp * e_r[nbi[i * T + p]]);
  }

  // 3. the iteration (the columns are the thread's own: the barrier above already separates fa's writes from the reads)
  float* f0 = fa;
  float* f1 = fb;
  {
    const float y = act ? e_y[p] : 0.f, oma = 1.0f - P.alpha;
    for (int t = 0; t < P.iters; ++t) {
      if (act) {
        float g = 0.f;
        for (int i = 0; i < m; ++i) g = fmaf(nbv[i * T + p], f0[nbi[i * T + p]], g);
        f1[p] = (P.alpha * g) + (oma * y);
      }
      __syncthreads();
      float* sw = f0; f0 = f1; f1 = sw;
    }
  }

  // 4. rank by (f desc, id asc, position asc) and place
  const int npad = T < 2 ? 2 : T;                                    // T is a power of two >= 64
  key[p] = act ? ((u64)rank_score_key(__float_as_uint(f0[p])) << 32) | (unsigned)e_pos[p] : ((u64)RANK_MISSING << 32) | (unsigned)p;
  __syncthreads();
  const RankIdList L{ids};
  block_bitonic_sort(key, npad, RankBefore<RankIdList>{L});
  if (tid < n && tid < P.k) {
    const u64 kr = key[tid];
    if ((unsigned)(kr >> 32) != RANK_MISSING) {
      out_scores[out0 + tid] = rank_key_score(kr);
      out_idx[out0 + tid] = L.at(kr);
      if (out_pos) out_pos[out0 + tid] = (int)((unsigned)kr & RANK_POS_MASK);
    } else {                                                         // (an f that is NaN: outside the contract, inside the bounds)
      out_scores[out0 + tid] = RANK_NEG_INF;
      out_idx[out0 + tid] = -1;
      if (out_pos) out_pos[out0 + tid] = -1;
    }
  }
  rank_fill_tail(n, P.k, out0, out_scores, out_idx, out_pos);
}

template <int DT>
int launch_diffusion(const SegRowsSq& segs, int nseg, const float* scores, const long long* idx, int Bq, const DfParams& P, float* out_scores,
                     long long* out_idx, int* out_pos, hipStream_t st) {
  const int npad = next_pow2(P.kin);
  const int threads = npad < 64 ? 64 : npad;                         // 64, 128 or 256: one thread per candidate
  const size_t lds = df_lds_bytes(threads, P.C, P.kd);
  if (P.kd <= DF_KD_SMALL) {
    static DevOnce once;
    cor_max_dyn_lds((const void*)rerank_diffusion_kernel<DT, DF_KD_SMALL>, (int)df_lds_bytes(DF_NMAX, DF_CMAX, DF_KD_SMALL), once);
    hipLaunchKernelGGL((rerank_diffusion_kernel<DT, DF_KD_SMALL>), dim3((unsigned)Bq), dim3(threads), lds, st, segs, nseg, scores, idx, P,
                       (unsigned*)out_scores, out_idx, out_pos);
  } else {
    static DevOnce once;
    cor_max_dyn_lds((const void*)rerank_diffusion_kernel<DT, 0>, (int)df_lds_bytes(DF_NMAX, DF_CMAX, DF_KDMAX), once);
    hipLaunchKernelGGL((rerank_diffusion_kernel<DT, 0>), dim3((unsigned)Bq), dim3(threads), lds, st, segs, nseg, scores, idx, P,
                       (unsigned*)out_scores, out_idx, out_pos);
  }
  COR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int cor_rerank_diffusion(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                                    const int* seg_dtype, int nseg, const float* scores, const long long* idx, int Bq, int kin, int C, int kd,
                                    int kq, int gamma, float alpha, int iters, int k, float* out_scores, long long* out_idx, int* out_pos,
                                    void* stream) {
  if (!scores || !idx || !out_scores || !out_idx || Bq < 0 || kin < 1 || k < 1 || kd < 1 || kq < 1 || gamma < 1 || iters < 1 || nseg < 0 || C < 1)
    return COR_EINVAL;
  if (!(alpha >= 0.f && alpha < 1.f)) return COR_EINVAL;                 // (a NaN alpha fails both comparisons)
  const SegArrays t = {seg_rows, seg_scale, seg_offset, seg_n, seg_dtype, nseg, true};
  if (const int rc = seg_table_check(t)) return rc;
  if (kin > DF_NMAX || kd > DF_KDMAX || gamma > 4 || iters > 64 || k > COR_TOPK_KMAX || C > DF_CMAX || C % 16 != 0) return COR_ENOSUPPORT;
  SegRowsSq segs;
  int seen = 0;
  if (const int rc = seg_table_fill(t, false, segs, nseg, seen)) return rc;
  if (Bq == 0) return 0;
  const DfParams P = {kin, C, kd, kq, gamma, iters, k, alpha};
  return seg_dispatch_dtype(seen, [&](auto dt) {
    return launch_diffusion<decltype(dt)::value>(segs, nseg, scores, idx, Bq, P, out_scores, out_idx, out_pos, (hipStream_t)stream);
  });
}
