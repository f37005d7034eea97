// cor_amd — gallery similarity + top-k for gfx950 (the retrieval end of the path).
//
//   score[b,g] = Q[b,:] . G[g,:]   (unit vectors: cosine, utils/loss_func.py:84)  ->  per query top-k by
//   (score desc, global index asc).
//
// The [Bq, Ng] score matrix is never written to HBM. 16-bit galleries with C = 256 (the CORE embedding width) take the
// threshold-and-append pipeline further down (sim_scan: MFMA scan + exact fp32-chain re-scoring of the short list =>
// top-k indices and scores BIT-IDENTICAL to the CPU chain oracle); what follows first are the per-lane sorted-list kernels
// (fp32 galleries: the exact-chain form; 16-bit: the always-available fallback). One WAVE owns 32 queries (their K-fragments stay in
// registers for the whole kernel) and streams a slice of gallery rows through the MFMA as the A operand:
// D[row = gallery row, col = query] puts each query on a lane, so every lane keeps a private sorted top-k list
// of its own 16 scores per 32x32 tile (compare against the list minimum; insertion is rare after warm-up).
// Partial lists (2 lane-halves x nsplit gallery slices) go to a small workspace; a second kernel merges them.
//
// fp32 gallery: v_mfma_f32_32x32x2_f32 — bitwise a k-ordered fmaf chain. With 16-B operand loads the chain
// order is, for c = 0..C/8-1, i = 0..3:  k = 8c+i  then  k = 8c+4+i. oracle/c/sim_chain.c restates exactly this
// chain, so fp32 scores (and hence top-k indices) can be checked BITWISE against the CPU.
// bf16 / fp16 gallery: v_mfma_f32_32x32x16_{bf16,f16}; Q is rounded to the gallery dtype in registers.
// Everything up to the "WIDE k" section serves k <= 32; 33 <= k <= 256 takes the route of that section (launch_topk dispatches on k first).
#include <limits.h>
#include <algorithm>

#include "common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

struct TopkPlan { int nqt, nsplit, tiles_per_split, nparts, kmax; };

inline TopkPlan make_plan(int Bq, int Ng, int k) {
  TopkPlan p;
  p.kmax = k <= 8 ? 8 : 32;
  p.nqt = cdiv(Bq, 32);
  const int tiles = cdiv(Ng, 32);
  int want = cdiv(4096, p.nqt);                       // ~16 waves per CU over the whole chip
  const int cap = (4096 / p.kmax) / 2;                // merge kernel holds nparts*kmax <= 4096 candidates (32 KiB) in LDS
  if (want > cap) want = cap;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  p.tiles_per_split = cdiv(tiles, want);
  p.nsplit = cdiv(tiles, p.tiles_per_split);
  p.nparts = 2 * p.nsplit;
  return p;
}

template <int KMAX>
__device__ __forceinline__ void topk_insert(float (&ls)[KMAX], int (&li)[KMAX], float s, int idx) {
  if (s > ls[KMAX - 1]) {
    ls[KMAX - 1] = s; li[KMAX - 1] = idx;
#pragma unroll
    for (int j = KMAX - 1; j > 0; --j) {
      if (ls[j] > ls[j - 1]) {       // strict: an equal, earlier (smaller index) entry stays ahead
        const float ts = ls[j]; ls[j] = ls[j - 1]; ls[j - 1] = ts;
        const int ti = li[j]; li[j] = li[j - 1]; li[j - 1] = ti;
      }
    }
  }
}

// Offer the 16 scores of one 32x32 accumulator tile (this lane's query, gallery rows g0 + row(e,h)) to the lane's list.
// After warm-up almost no score beats the list minimum, so the insertion bubble (a few hundred predicated moves once
// unrolled) must not even be ISSUED in the common case: one max over the tile and one wave-uniform ballot skip it all,
// and inside, each element is again guarded by a ballot (hipcc otherwise predicates the bubble without a branch and a
// tile cost ~15k cycles of v_mov with an empty EXEC mask).
template <int KMAX>
__device__ __forceinline__ void topk_offer_tile(float (&ls)[KMAX], int (&li)[KMAX], const f32x16& acc, int g0, int h, int Ng) {
  float sc[16];
  float tmax = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int g = g0 + (e & 3) + 8 * (e >> 2) + 4 * h;
    sc[e] = g < Ng ? acc[e] : -INFINITY;
    tmax = fmaxf(tmax, sc[e]);
  }
  if (__builtin_amdgcn_ballot_w64(tmax > ls[KMAX - 1]) == 0) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (__builtin_amdgcn_ballot_w64(sc[e] > ls[KMAX - 1]) != 0) topk_insert<KMAX>(ls, li, sc[e], g0 + (e & 3) + 8 * (e >> 2) + 4 * h);
  }
}

// TG: float (exact chain), bf16_t, _Float16. C (embedding dim) <= 256, multiple of 16.
template <typename TG, int KMAX>
__global__ void __launch_bounds__(256) sim_topk_partial(const float* __restrict__ Q, const TG* __restrict__ G, int Bq, int Ng, int C,
                                                        TopkPlan plan, float* ws_s, int* ws_i) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= plan.nqt * plan.nsplit) return;
  const int qt = wid % plan.nqt, split = wid / plan.nqt;
  const int q = qt * 32 + r;
  const float* qrow = Q + (long)min(q, Bq - 1) * C;

  constexpr bool F32 = sizeof(TG) == 4;
  constexpr int CH = F32 ? 8 : 16;          // k per chunk pair
  constexpr int NCH = 256 / CH;             // max chunks held in registers
  const int nch = C / CH;
  uint4 qf[NCH];                            // fp32: 4 floats ; 16-bit: 8 values
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c < nch) {
      if (F32) {
        qf[c] = *(const uint4*)(qrow + c * 8 + 4 * h);
      } else {
        const f32x4 lo = *(const f32x4*)(qrow + c * 16 + 8 * h), hi = *(const f32x4*)(qrow + c * 16 + 8 * h + 4);
        if (sizeof(TG) == 2 && __is_same(TG, bf16_t)) {
          qf[c].x = (uint32_t)f2bf(lo[0]) | ((uint32_t)f2bf(lo[1]) << 16); qf[c].y = (uint32_t)f2bf(lo[2]) | ((uint32_t)f2bf(lo[3]) << 16);
          qf[c].z = (uint32_t)f2bf(hi[0]) | ((uint32_t)f2bf(hi[1]) << 16); qf[c].w = (uint32_t)f2bf(hi[2]) | ((uint32_t)f2bf(hi[3]) << 16);
        } else {
          f16x8 t = {(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3], (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
          qf[c] = __builtin_bit_cast(uint4, t);
        }
      }
    }
  }

  float ls[KMAX]; int li[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) { ls[j] = -INFINITY; li[j] = INT_MAX; }

  const int t0 = split * plan.tiles_per_split;
  const int t1 = min(t0 + plan.tiles_per_split, cdiv(Ng, 32));
  for (int t = t0; t < t1; ++t) {
    const int g0 = t * 32;
    const char* grow = (const char*)(G + (long)min(g0 + r, Ng - 1) * C) + 16 * h;   // lane's 16-B column inside each 32-B chunk pair
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c < nch) {
        const uint4 a = *(const uint4*)(grow + c * 32);
        if (F32) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(qf[c].x), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(qf[c].y), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(qf[c].z), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(qf[c].w), acc, 0, 0, 0);
        } else if (__is_same(TG, bf16_t)) {
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, qf[c]), acc, 0, 0, 0);
        } else {
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, qf[c]), acc, 0, 0, 0);
        }
      }
    }
    topk_offer_tile<KMAX>(ls, li, acc, g0, h, Ng);
  }
  if (q < Bq) {
    const long base = ((long)q * plan.nparts + split * 2 + h) * KMAX;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { ws_s[base + j] = ls[j]; ws_i[base + j] = li[j]; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// v2 (16-bit galleries): the MFMA-bound form for B_tot >= ~256. One block per CU = 4 waves x 64 queries: every wave keeps
// the K-fragments of TWO 32-query blocks in registers (128 VGPRs) for the whole kernel, the gallery slice streams through
// LDS in 32-row tiles (16 KiB, register-staged, double-buffered, shared by the 4 waves => each gallery byte is fetched
// once per 256 queries), and each A fragment read from LDS feeds two MFMAs (one per query block). LDS rows are 512 B, so
// chunk c of row r sits in slot c ^ (r & 15): the 16 rows of a ds_read_b128 lane group hit 16 distinct 16-B slots.
struct TopkPlan2 { int nqg, nsplit, tiles_per_split, nparts, kmax; };

inline TopkPlan2 make_plan2(int Bq, int Ng, int k, int n_cu) {
  TopkPlan2 p;
  p.kmax = k <= 8 ? 8 : (k <= 16 ? 16 : 32);
  p.nqg = cdiv(Bq, 256);
  const int tiles = cdiv(Ng, 32);
  int want = n_cu / p.nqg;                            // one resident block per CU
  const int cap = (8192 / p.kmax) / 2;                // merge kernel: nparts*kmax <= 8192 candidates in LDS
  if (want > cap) want = cap;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  p.tiles_per_split = cdiv(tiles, want);
  p.nsplit = cdiv(tiles, p.tiles_per_split);
  p.nparts = 2 * p.nsplit;
  return p;
}

template <typename TG>
__device__ __forceinline__ uint4 q_frag16_vals(const f32x4 lo, const f32x4 hi) {       // 8 fp32 values -> one 16-byte K-fragment piece
  if (__is_same(TG, bf16_t)) {
    uint4 u;
    u.x = (uint32_t)f2bf(lo[0]) | ((uint32_t)f2bf(lo[1]) << 16); u.y = (uint32_t)f2bf(lo[2]) | ((uint32_t)f2bf(lo[3]) << 16);
    u.z = (uint32_t)f2bf(hi[0]) | ((uint32_t)f2bf(hi[1]) << 16); u.w = (uint32_t)f2bf(hi[2]) | ((uint32_t)f2bf(hi[3]) << 16);
    return u;
  }
  f16x8 t = {(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3], (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
  return __builtin_bit_cast(uint4, t);
}
template <typename TG>
__device__ __forceinline__ uint4 q_frag16(const float* qrow, int c, int h) {
  return q_frag16_vals<TG>(*(const f32x4*)(qrow + c * 16 + 8 * h), *(const f32x4*)(qrow + c * 16 + 8 * h + 4));
}

template <typename TG, int KMAX>
__global__ void __launch_bounds__(256, 1) sim_topk_v2(const float* __restrict__ Q, const TG* __restrict__ G, int Bq, int Ng,
                                                      TopkPlan2 plan, float* ws_s, int* ws_i, const int* gate) {
  if (gate && *gate == 0) return;                               // device-side fallback: runs only after a candidate overflow
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 x 16 KiB gallery tiles
  constexpr int C = 256, TILE = 32 * C * 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int qg = blockIdx.x % plan.nqg, split = blockIdx.x / plan.nqg;
  const int q0 = qg * 256 + wave * 64;
  const bool active = q0 < Bq;                                  // wave-uniform: idle waves still stage and barrier

  uint4 qf[2][16];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const float* qrow = Q + (long)min(q0 + qb * 32 + r, Bq - 1) * C;
#pragma unroll
    for (int c = 0; c < 16; ++c) qf[qb][c] = q_frag16<TG>(qrow, c, h);
  }
  float ls[2][KMAX]; int li[2][KMAX];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { ls[qb][j] = -INFINITY; li[qb][j] = INT_MAX; }

  // staging: thread owns chunks c = tid + 256 i (i < 4) of the 32 x 32-chunk tile
  int st_row[4], st_dst[4], st_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i, row = c >> 5, ch = c & 31;
    st_row[i] = row; st_src[i] = ch * 8; st_dst[i] = row * 512 + ((ch ^ (row & 15)) << 4);
  }
  int rd[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) rd[c] = r * 512 + (((2 * c + h) ^ (r & 15)) << 4);

  const int ntiles = cdiv(Ng, 32);
  const int t0 = split * plan.tiles_per_split, t1 = min(t0 + plan.tiles_per_split, ntiles);
  uint4 rg0, rg1, rg2, rg3;
#define SIM_GLOAD(T_)                                                                              \
  {                                                                                                \
    const int g0_ = (T_) * 32;                                                                     \
    rg0 = *(const uint4*)(G + (long)min(g0_ + st_row[0], Ng - 1) * C + st_src[0]);                 \
    rg1 = *(const uint4*)(G + (long)min(g0_ + st_row[1], Ng - 1) * C + st_src[1]);                 \
    rg2 = *(const uint4*)(G + (long)min(g0_ + st_row[2], Ng - 1) * C + st_src[2]);                 \
    rg3 = *(const uint4*)(G + (long)min(g0_ + st_row[3], Ng - 1) * C + st_src[3]);                 \
  }
#define SIM_LSTORE(B_)                                                                             \
  {                                                                                                \
    char* d_ = smem + (B_) * TILE;                                                                 \
    *(uint4*)(d_ + st_dst[0]) = rg0; *(uint4*)(d_ + st_dst[1]) = rg1;                              \
    *(uint4*)(d_ + st_dst[2]) = rg2; *(uint4*)(d_ + st_dst[3]) = rg3;                              \
  }
  if (t0 < t1) {
    SIM_GLOAD(t0)
    SIM_LSTORE(0)
  }
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const bool more = t + 1 < t1;
    if (more) SIM_GLOAD(t + 1)
    const char* buf = smem + ((t - t0) & 1) * TILE;
    if (active) {
      f32x16 acc0, acc1;
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const uint4 a = *(const uint4*)(buf + rd[c]);
        if (__is_same(TG, bf16_t)) {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, qf[0][c]), acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, qf[1][c]), acc1, 0, 0, 0);
        } else {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, qf[0][c]), acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, qf[1][c]), acc1, 0, 0, 0);
        }
      }
      topk_offer_tile<KMAX>(ls[0], li[0], acc0, t * 32, h, Ng);
      topk_offer_tile<KMAX>(ls[1], li[1], acc1, t * 32, h, Ng);
    }
    if (more) SIM_LSTORE((t + 1 - t0) & 1)
    __syncthreads();
  }
#undef SIM_GLOAD
#undef SIM_LSTORE
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int q = q0 + qb * 32 + r;
    if (q < Bq) {
      const long base = ((long)q * plan.nparts + split * 2 + h) * KMAX;
#pragma unroll
      for (int j = 0; j < KMAX; ++j) { ws_s[base + j] = ls[qb][j]; ws_i[base + j] = li[qb][j]; }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// v3 (16-bit galleries, C = 256, every shard size): threshold-and-append with EXACT re-scoring.
// Per-lane sorted lists cost one divergent insertion bubble (~500 wave cycles) per accepted score, and a stream of n scores
// accepts ~k ln(n/k) of them per lane: measured 9x the MFMA time. Instead, four launches (sim_prep + these three):
//   A. sim_scan<SAMPLE>: MFMA scores of a strided SAMPLE of 32-row tiles; every (gallery slice, lane quarter) group keeps only
//      its MAXIMUM per query and folds it (atomic max on order-preserving keys) into one of 32 SUPER-GROUPS per query. The
//      super-groups are disjoint row sets, so the k-th largest of their maxima is a LOWER bound of the query's k-th best score over
//      the whole shard (no dense score matrix, no selection pass).
//   B. tau_q = that k-th largest maximum minus delta_q: ranked in the PROLOGUE of pass C (thread <-> query, a 32-element bitonic
//      network in registers). Rounds 2-3 ranked all 512 group maxima in a launch of their own (sim_tau, 5-7 us, launch-bound); the
//      32 unions admit ~15 % more candidates and cost the prologue ~3 us: one launch fewer, 0-2 % faster in a same-box A/B.
//   C. sim_scan<APPEND>: MFMA scores of the WHOLE shard; a lane compares its tile maximum with tau_q and appends the rare
//      scores >= tau_q to the private list of its (query, gallery slice, lane quarter) stream (register counter, no atomics).
//   D. sim_final: per query, the candidates are compacted into LDS, the k-th best MFMA score T is bounded by a 2-pass radix
//      select (16 key bits), the SHORT LIST (MFMA score >= T - delta_q, ~k entries) is RE-SCORED with the exact fp32 fmaf chain of
//      oracle/c/sim_chain.c over the stored 16-bit values (the query rounded to the gallery dtype), and ranked by
//      (chain score desc, index asc).
// Exactness. Let s~ be the MFMA score (fp32 accumulation of exact bf16/fp16 products in the matrix core's order) and s the
// chain score. Both are fp32 summations of the same 256 exact products, so |s~ - s| <= eps_q := 2^-23 * 255/... bounded by
// 2 * 255 * 2^-24 * sum|q_k g_k| <= 3.1e-5 * |q| |g| (one rounding per addition either way; doubled for a truncating
// adder). If g is in the chain top-k then s~_g >= T - 2 eps_q (the k rows of the MFMA top-k have chain scores
// >= T - eps_q, hence the k-th best chain score is >= T - eps_q), so with delta_q = 6.4e-5 * max(1, |q|) * 1.01 (gallery rows
// are unit vectors: cosine similarity) the short list contains every row of the exact answer, tau_q - delta_q admits all
// of them in pass C, and the output (scores AND indices) is bit-identical to ranking the chain scores of the whole shard.
// Overflows (a stream list, the LDS candidate buffer or the short list: pathological score distributions such as tens of
// thousands of identical rows) are detected ON THE DEVICE: sim_final flags the query and the gated list kernels
// (sim_topk_v2 + sim_topk_merge, launched behind it, a few microseconds when idle) recompute exactly those queries:
// no host synchronisation, no process-global mode.
constexpr float SIM_DELTA = 6.4e-5f * 1.01f;
constexpr int FS_MAX = 8192;                           // candidates per query held in LDS by sim_final (64 KiB)
constexpr int SL_MAX = 512;                            // short list (re-scored exactly)
constexpr int SCAN_NS = 5, SCAN_AHEAD = 4;             // LDS-DMA ring of 32-KiB gallery super-tiles (64 rows): 160 KiB = all of LDS, one block per CU

struct ScanArgs {
  int Bq, Ng, nqg, nsplit, tiles_per_split;
  int ntiles;                      // 64-row super-tiles this launch walks (SAMPLE: sample super-tiles; APPEND: all of them)
  int tile_stride;                 // super-tiles between consecutive walked super-tiles (SAMPLE: >= 1; APPEND: 1)
  const uint4* qimg;               // queries rounded to the gallery dtype, fragment-major (sim_prep)
  unsigned* sg; int Bqp;           // 32 SUPER-GROUP maxima per query as order-preserving keys, sg[g * Bqp + q] (zeroed by sim_prep; 0 = empty):
                                   // SAMPLE: atomic max of the group (slice, lane quarter) maximum into super-group (split * 4 + rq) & 31; APPEND: read
  const float* dq; int k;          // APPEND: delta_q (sim_prep) and k: tau_q = k-th largest super-group maximum - delta_q, computed in the prologue
  float tau_add;                   // 0; timing-only ablation (COR_TOPK_DEBUG_NOCAND): +1e30 = no candidate ever passes
  int probe_same;                  // COR_PROBES (timing only): every block streams the same 8 super-tiles (cache-resident gallery)
  unsigned long long* stamps;      // COR_PROBES: cycle stamps of waves 0 and 4 of block 0 (tools/sim_stamps.py scan)
  float* tau; int* cnt; float* rec_s; int* rec_g; int cap;           // APPEND: tau_q (written by the blocks of slice 0 for the selection kernel); record i of stream (q, slice, lane quarter): 8 scores + first row
  const int* rlab; const int* qlab; int ne;                           // FILTER: row / query labels, COR_FILTER_NE (filtered wide route only)
  int* sgrow;                                                         // GROUP SAMPLE: the shard row behind every stored sample value (distinct-group route only)
  const float* rng_a; const float* rng_h; int* sure;                  // RANGE APPEND: the bounds A_q and H_q (sim_range_bounds; a.tau holds B_q) and the sure counts per stream
};

// One block = 8 waves = 256 * QB queries (wave w owns queries q0 + 32 * QB * w ..): with QB = 2 all 512 queries of an
// 8-GPU all-gather (8 x 64) sit in ONE block, so every gallery byte is fetched from HBM once per launch (512 MB at 1M rows)
// and the kernel is MFMA-bound (arithmetic intensity = queries per block FLOP/B against a ridge of ~400); the K-fragments of
// the wave's queries stay in registers for the whole kernel (QB * 64 VGPRs) and each A fragment read from LDS feeds 2 QB MFMAs
// (v_mfma_f32_16x16x32 since round 5: see the kernel).
// Gallery super-tiles (64 rows x 512 B = two 32-row tiles) stream through a 5-slot LDS-DMA ring, 4 of them (128 KiB per CU) in
// flight: counted s_waitcnt vmcnt, ONE barrier per 64 rows. The LDS image is lane-linear per wave-instruction (64 lanes x 16 B = two 512-B
// rows), so slot (row, sl) is fed from source chunk sl ^ (row & 15) and the reads apply the same XOR (conflict-free b128).
// max of three. NOT inline asm: hipcc pads no MFMA -> VALU read hazard for an asm statement, so a v_max3_f32 in asm read the
// accumulators before the matrix pipe had written them (sporadic missed candidates). The file is built with -fno-honor-nans
// (Makefile) so that fmaxf needs no canonicalising v_max x,x,x per operand and folds to v_max3_f32 by itself.
__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
// order-preserving float <-> unsigned keys (0 is below every float's key: "empty")
__device__ __forceinline__ unsigned f2key(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float key2f_floor(unsigned key) {      // the smallest float whose order-preserving key is >= key's prefix
  const unsigned u = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
  return __uint_as_float(u);
}

// ---------------------------------------------------------------------------------------------------------------------
// SHARED SCAN STEPS: the one copy of what sim_scan (16-bit rows, C = 256), sim_wide_scan (fp32 rows or C != 256) and sim_i8_scan (int8 rows)
// do alike around their tile loops. Forced inline, values by reference: the callers' register arrays stay in registers. They live in this
// file because the fmaxf / fminf folding depends on its -fno-honor-nans (Makefile). DESIGN.md lists which kernel uses which step, and the
// sites that keep their own lines because the shared form compiled to more registers there.
// The filter rule (include/cor_amd.h): a query with label ql < 0 is unrestricted; otherwise COR_FILTER_EQ (ne == 0) allows the rows that
// carry ql, COR_FILTER_NE the rows that do not. Callers keep their own outer terms (!FILTER, rlab == nullptr, the row-inside-the-shard tests).
__device__ __forceinline__ bool label_allows(int label, int ql, int ne) { return ql < 0 || ((label == ql) != (ne != 0)); }
// the same for row g of a label array: an unrestricted query reads no label (rlab may be null then)
__device__ __forceinline__ bool row_allowed(const int* __restrict__ rlab, int g, int ql, int ne) { return ql < 0 || label_allows(rlab[g], ql, ne); }

// p[row .. row + 3] of an array of Ng elements as one 16-byte load (row % 4 == 0, p 16-byte aligned); the ragged end element by element,
// zero beyond Ng: nothing is read past the array. V4: the caller's 16-byte vector type.
template <typename V4, typename T, typename I> __device__ __forceinline__ V4 load4_or_zero(const T* __restrict__ p, I row, int Ng) {
  typedef T vec4 __attribute__((ext_vector_type(4)));
  vec4 v;
  if (row + 4 <= Ng) v = *(const vec4*)(p + row);
  else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row + e < Ng ? p[row + e] : T(0);
  }
  return __builtin_bit_cast(V4, v);
}

// The tiles slice `split` of nsplit walks, t = t0 .. t1 - 1 -> tile(t): a contiguous run of tiles_per_split tiles, or with FILTER the
// interleaved tiles split, split + nsplit, ... (a class-sorted gallery spreads over every slice, stream and sample group).
template <bool FILTER> struct SliceWalk {
  int t0, t1, split, nsplit;
  __device__ __forceinline__ SliceWalk(int split_, int nsplit_, int tiles_per_split, int ntiles) : split(split_), nsplit(nsplit_) {
    t0 = FILTER ? 0 : split * tiles_per_split;
    t1 = FILTER ? cdiv(ntiles - split, nsplit) : min(t0 + tiles_per_split, ntiles);
  }
  __device__ __forceinline__ int tile(int t) const { return FILTER ? split + t * nsplit : t; }
};

// FILTER SAMPLE: a sample group's four best allowed scores, descending. offer is branch-free (-inf, a masked score, changes nothing);
// store writes the four keys to the group's four slots (16-byte aligned).
struct Best4 {
  float v[4];
  __device__ __forceinline__ void clear() { v[0] = v[1] = v[2] = v[3] = -INFINITY; }
  __device__ __forceinline__ void offer(float x) {
    v[3] = fmaxf(v[3], fminf(v[2], x));
    v[2] = fmaxf(v[2], fminf(v[1], x));
    v[1] = fmaxf(v[1], fminf(v[0], x));
    v[0] = fmaxf(v[0], x);
  }
  __device__ __forceinline__ void store(unsigned* sg4) const { *(uint4*)sg4 = make_uint4(f2key(v[0]), f2key(v[1]), f2key(v[2]), f2key(v[3])); }
};
// GROUP SAMPLE (the distinct routes): a sample group's NV best allowed scores, descending, each with the ROW behind it (NV = 1, or 4 with
// FILTER). A masked / out-of-shard score is -inf and never kept; an empty slot holds (-inf, row 0). Offers are rare after warm-up: the
// callers put one wave-uniform test of the tile maximum against v[NV - 1] in front. store: keys to sg, rows to sgrow, at the same index.
template <int NV> struct BestRows {
  float v[NV]; int row[NV];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < NV; ++j) { v[j] = -INFINITY; row[j] = 0; }
  }
  __device__ __forceinline__ void offer(float x, int r) {
    if (x > v[NV - 1]) { v[NV - 1] = x; row[NV - 1] = r; }
#pragma unroll
    for (int j = NV - 1; j > 0; --j) {
      const float s0 = v[j - 1], s1 = v[j];
      const int i0 = row[j - 1], i1 = row[j];
      const bool up = s1 > s0;
      v[j - 1] = up ? s1 : s0; v[j] = up ? s0 : s1;
      row[j - 1] = up ? i1 : i0; row[j] = up ? i0 : i1;
    }
  }
  __device__ __forceinline__ void store(unsigned* sg, int* sgrow, long at) const {
#pragma unroll
    for (int j = 0; j < NV; ++j) { sg[at + j] = f2key(v[j]); sgrow[at + j] = row[j]; }
  }
};

// APPEND of sim_wide_scan / sim_i8_scan. The threshold a lane compares with: tau_q, floored so that a masked -inf score stays out of the
// lists when tau_q is -inf; a padding lane (not `real`: q >= Bq or an idle wave) gets +inf: it never appends and never reads tau.
__device__ __forceinline__ float append_threshold(bool real, const float* tau, int q) { return real ? fmaxf(tau[q], -3.0e38f) : INFINITY; }
// One (score bits, row) entry into the private list dst [cap] of a stream; n keeps counting past cap (the selection sees the overflow).
__device__ __forceinline__ void append_entry(uint2* dst, int& n, int cap, float score, int row) {
  if (n < cap) dst[n] = make_uint2(__float_as_uint(score), (unsigned)row);
  ++n;
}

// WIDE (33 <= k <= 256, see the wide-k route below): SAMPLE stores every (slice, lane quarter) group maximum on its own, sg[q * Bqp + split * 4 + rq]
// with Bqp = the group count (no super-group folding: tau needs >= k groups); APPEND reads tau_q from a.tau (sim_tau_wide ranked the groups).
// FILTER (the filtered wide route, any k; implies WIDE): a disallowed score is -inf before every maximum and compare. Slice `split` walks the
// super-tiles split, split + nsplit, ... (a class-sorted gallery spreads over every slice and stream), the labels of those rows are copied
// into LDS once in the prologue (a 4-slot ring: the fifth slot holds them), SAMPLE keeps the FOUR best allowed scores per group
// (sg[q * Bqp + (split * 4 + rq) * 4 + j]: a clustered subset still yields >= k values), and APPEND decides on the allow predicate.
// GROUP (the distinct-group route; SAMPLE only, implies WIDE; APPEND is the plain WIDE / FILTER instantiation): every stored sample value
// keeps its ROW beside it (a.sgrow, same index as a.sg), NV = 1 (4 with FILTER) best allowed scores per (slice, lane quarter) group:
// sim_tau_distinct needs the rows' group ids to count DISTINCT groups above the threshold.
// RANGE (cor_similarity_range; APPEND only, implies WIDE, no FILTER): a.tau holds B_q = thr_q - delta_q, the lowest score that matters, and
// one wave-uniform test of the tile maximum against it guards everything else. Behind it a lane counts its scores >= H_q = thr_q + delta_q
// (sure members: counted in registers, written next to cnt at the end of the slice, no atomics) and appends its column when it holds a
// list candidate (>= A_q = max(tau_q, B_q)) or a band row (B_q <= s < H_q, for the chain to decide). A_q and H_q of the lane's NQ queries
// share ONE register each: lane (n16, rq) keeps those of query block rq % NQ and the guarded branch fetches them across lanes; the sure
// count shares ncand's register (low 16 bits; the records above them): make_wide keeps a slice at <= 4095 super-tiles = 65 520 scores per
// lane. With a counter of its own per query block the QB = 2 instantiation spilled four registers.
// FILTER + RANGE (cor_similarity_range_filtered): the label mask first, then the RANGE branch on the masked scores; B_q, A_q and H_q are
// >= -3e38, so a masked -inf is never counted, never a band row and never appended. Instantiated with QB = 1 only: QB = 2 (254 VGPRs
// without the filter) needs the lane's query labels and row labels as well and came out of the compiler with 256 VGPRs, four spilled
// registers and 20 bytes of scratch per lane; make_wide plans the filtered range with QB = 1 for every Bq (170 VGPRs, no spill).
template <typename TG, int QB, bool SAMPLE, bool WIDE = false, bool FILTER = false, bool GROUP = false, bool RANGE = false>
__global__ void __launch_bounds__(512, 2) sim_scan(const TG* __restrict__ G, const ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int C = 256, TILE = 32 * C * 2, STILE = 2 * TILE, NS = FILTER ? SCAN_NS - 1 : SCAN_NS, AHEAD = FILTER ? SCAN_AHEAD - 1 : SCAN_AHEAD;
  // Round 5: v_mfma_f32_16x16x32 instead of 32x32x16. A wave's 32 rows x 32 QB queries are 2 x NQ blocks of 16 x 16 = 2 NQ INDEPENDENT
  // accumulators of four registers (the 32 x 32 form had QB = 2 dependent chains: a wave alone issued an MFMA every ~43 cycles instead of 32),
  // and the chip holds a higher clock on this shape (MI355X guide, DVFS item 7): 512 x 1M 280-300 -> 185-200 us in the timing probe. Operand
  // lane (n16 = lane & 15: gallery row of a 16-row block / query of a 16-query block, rq = lane >> 4: K quarter of a 32-deep step);
  // accumulator lane: query n16, rows 4 rq + e of the row block. Same LDS image, same number of ds_read_b128, same register count.
  constexpr int NQ = 2 * QB;                           // 16-query blocks per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), n16 = lane & 15, rq = lane >> 4;
  const int qg = blockIdx.x % a.nqg, split = blockIdx.x / a.nqg;
  const int q0 = qg * (256 * QB) + wave * (32 * QB);
  const bool active = q0 < a.Bq;                     // wave-uniform: idle waves still stage and barrier
  // Waves w and w + 4 share a SIMD and, running the same program between the same barriers, would reach their MFMAs, their
  // VALU epilogues and the barrier TOGETHER: the matrix pipe then idles through every epilogue. The younger half (waves 4-7)
  // therefore runs the epilogue of a tile AFTER the next barrier, in front of its next MFMAs, i.e. beside the MFMAs of its
  // SIMD partner (MI355X guide, "two waves per SIMD", item 9); the accumulators are not overwritten until then, so no
  // double buffering is needed.
  const bool late = wave >= 4;

  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((__attribute__((address_space(3))) char*)smem));
  // A super-tile = 64 rows x 512 B; wave w copies rows 8w .. 8w+7 with FOUR LDS-DMA instructions of two rows each under ONE M0 setting: the
  // instruction offsets 0 / 1024 / 2048 / 3072 move the LDS and the global address alike (rows are contiguous in both), the per-lane
  // offset carries the row of the pair and the swizzled chunk. (Round 5 stamps: per-lane 64-bit addresses + an M0 save / set / restore per
  // instruction cost a wave 520-630 cycles per super-tile, both waves of a SIMD at the same time.)
  const unsigned wbase = (unsigned)wave * 4096u;       // this wave's first row (bytes) in a ring slot
  const int st_e = lane >> 5, st_sl = lane & 31;
  unsigned st_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) st_off[i] = (unsigned)(st_e * 512 + ((st_sl ^ ((8 * wave + 2 * i + st_e) & 15)) << 4));
  // super-tiles of 64 rows (SliceWalk; FILTER: t counts the slice's walked super-tiles)
  const SliceWalk<FILTER> walk(split, a.nsplit, a.tiles_per_split, a.ntiles);
  const int t0 = walk.t0, t1 = walk.t1;
  auto issue = [&](int t) {
#ifdef COR_PROBES
    const long g0 = (long)((a.probe_same & 1) ? (walk.tile(t) & 7) : walk.tile(t)) * a.tile_stride * 64;
#else
    const long g0 = (long)walk.tile(t) * a.tile_stride * 64;
#endif
    const unsigned dst = lds0 + ((t - t0) % NS) * STILE + wbase;
    if (g0 + 64 <= a.Ng) {                             // (scalar) every row of the super-tile is inside the shard
      const char* sb = (const char*)G + (g0 + 8 * wave) * 512;
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\t"
                   "global_load_lds_dwordx4 %1, %5\n\tglobal_load_lds_dwordx4 %2, %5 offset:1024\n\t"
                   "global_load_lds_dwordx4 %3, %5 offset:2048\n\tglobal_load_lds_dwordx4 %4, %5 offset:3072\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(st_off[0]), "v"(st_off[1]), "v"(st_off[2]), "v"(st_off[3]), "s"(sb), "s"(dst) : "memory");
    } else {                                           // the shard's last super-tile: clamped duplicates (masked to -inf in the epilogue)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 8 * wave + 2 * i + st_e;
        glds16(G + min(g0 + row, (long)a.Ng - 1) * C + ((st_sl ^ (row & 15)) << 3), dst + 1024 * i);
      }
    }
  };
  // The ring is filled FIRST: the HBM round trip of the first super-tiles runs under the prologue below (threshold network, 32 KiB of
  // K-fragments per wave); tau_s sits in the slot these copies do not touch.
  for (int t = t0; t < min(t0 + AHEAD, t1); ++t) issue(t);

  // APPEND: tau_q in the prologue (round 4: no sim_tau launch). Thread <-> query of this block: its 32 super-group maxima, a 32-element
  // bitonic network in registers (the K-fragments are not loaded yet), tau_q = k-th largest - delta_q (fewer than k non-empty super-groups:
  // -inf, every row is a candidate). Any lower bound of the k-th best score is valid, so 32 unions of the (slice, lane quarter) groups serve
  // as well as the 512 groups the launch ranked (~15 % more candidates).
  float* tau_s = (float*)(smem + (NS - 1) * STILE);   // in the LAST ring slot: first written by the copies behind the loop's first barrier
  // FILTER: the labels of the rows this slice walks, lab_s[(t - t0) * 64 + row of the super-tile], behind the 4-slot ring (<= 128 super-tiles:
  // make_wide keeps tiles_per_split below that); rows past the shard read label 0 (their scores are -inf anyway)
  const int* lab_s = (const int*)(smem + NS * STILE);
  if constexpr (FILTER) {
    int* lab_w = (int*)(smem + NS * STILE);
    for (int i = tid; i < (t1 - t0) * 16; i += 512) {
      const long row = (long)walk.tile(t0 + (i >> 4)) * a.tile_stride * 64 + 4 * (i & 15);
      *(int4*)(lab_w + 4 * i) = load4_or_zero<int4>(a.rlab, row, a.Ng);
    }
    __syncthreads();
  }
  if (!SAMPLE && WIDE) {
    if (tid < 256 * QB) tau_s[tid] = a.tau[min(qg * (256 * QB) + tid, a.Bq - 1)];
    __syncthreads();
  } else if (!SAMPLE) {
    const int ql = tid;                                // 256 * QB queries per block, 512 threads
    if (ql < 256 * QB) {
      const int qg_ = min(qg * (256 * QB) + ql, a.Bq - 1);
      float v[32];
#pragma unroll
      for (int g = 0; g < 32; ++g) { const unsigned key = a.sg[(long)g * a.Bqp + qg_]; v[g] = key == 0u ? -INFINITY : key2f_floor(key); }
#pragma unroll
      for (int kk = 2; kk <= 32; kk <<= 1)
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1)
#pragma unroll
          for (int i = 0; i < 32; ++i) {
            const int l = i ^ j;
            if (l > i) {
              const float x = v[i], y = v[l];
              if ((i & kk) == 0) { v[i] = fmaxf(x, y); v[l] = fminf(x, y); }
              else               { v[i] = fminf(x, y); v[l] = fmaxf(x, y); }
            }
          }
      float kth = v[0];
#pragma unroll
      for (int c = 1; c < 32; ++c) kth = (c == a.k - 1) ? v[c] : kth;
      const float t = kth - a.dq[qg_];                 // -inf stays -inf
      tau_s[ql] = t;
      if (split == 0 && qg * (256 * QB) + ql < a.Bq) a.tau[qg * (256 * QB) + ql] = t;      // for the selection kernel
    }
    __syncthreads();
  }
  uint4 qf[NQ][8];
  float tau[NQ], gmax[NQ];
  int ncand[NQ];
  float pack_a = 0.f, pack_h = 0.f;                    // RANGE: A_q / H_q of query (block rq % NQ, n16)
  if constexpr (RANGE) {
    const int qp = min(q0 + (rq % NQ) * 16 + n16, a.Bq - 1);
    pack_a = a.rng_a[qp]; pack_h = a.rng_h[qp];
  }
  int ql[NQ];                                          // FILTER: the lane's query labels (< 0: unrestricted)
  Best4 top4[NQ];                                      // FILTER SAMPLE: the group's four best allowed scores (Best4)
  constexpr int NV = GROUP && FILTER ? 4 : 1;          // GROUP SAMPLE: the group's NV best allowed scores and their rows (BestRows)
  BestRows<NV> best[NQ];
  const int nstreams = a.nsplit * 4;                   // a stream = (query, gallery slice, lane quarter rq)
#pragma unroll
  for (int qb = 0; qb < NQ; ++qb) {
    // K-fragments from the fragment-major image sim_prep wrote (16-query block, 32-deep K-step, lane) x 16 B: 1 KiB per wave-instruction,
    // 8 of them per query block (reading the fp32 rows cost every CU 512 KiB of L2 traffic per launch: ~7 us)
    const uint4* qimg = a.qimg + ((long)(q0 / 16 + qb) * 8) * 64 + lane;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) qf[qb][kk] = active ? qimg[kk * 64] : make_uint4(0, 0, 0, 0);
    tau[qb] = SAMPLE ? 0.f : tau_s[wave * (32 * QB) + qb * 16 + n16] + a.tau_add;
    gmax[qb] = -INFINITY; ncand[qb] = 0;
    if constexpr (FILTER) {
      ql[qb] = a.qlab[min(q0 + qb * 16 + n16, a.Bq - 1)];
      top4[qb].clear();
    }
    if constexpr (GROUP) best[qb].clear();
  }
  // read address of 32-deep K-step kk, row block rb: row rb * 16 + n16, chunk (4 kk + rq) ^ n16 = ((kk ^ (n16 >> 2)) << 2) | (rq ^ (n16 & 3)): one XOR
  // per read. Conflict-free ds_read_b128: every 16-lane service group holds 16 different n16 (the two K quarters it mixes map onto disjoint slots).
  const int rd_base = n16 * 512 + ((rq ^ (n16 & 3)) << 4), rd_x = n16 >> 2;
#define SIM_RD(rb_, kk_) (rd_base + (rb_) * 8192 + ((((kk_) ^ rd_x)) << 6))

  f32x4 acc[NQ][2];                                    // [16-query block][16-row block]: register e = row 4 rq + e of the row block
  // epilogue of one 32-row tile (rows g0 ..): SAMPLE keeps the group maximum; APPEND compares the tile maximum with tau and
  // appends the rare scores >= tau to the lane's private stream list
  const int r4 = 4 * rq;
  auto epilogue = [&](int g0, int lo) {               // lo: FILTER, the tile's first row in lab_s
    const int lim = a.Ng - g0;                         // rows of this tile inside the shard (scalar); < 32 only at the shard's end
    int lr[2][4];                                      // FILTER: labels of the lane's 8 rows (16 rb + 4 rq + e)
    if constexpr (FILTER) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const int4 v = *(const int4*)(lab_s + lo + 16 * rb + r4);
        lr[rb][0] = v.x; lr[rb][1] = v.y; lr[rb][2] = v.z; lr[rb][3] = v.w;
      }
    }
#pragma unroll
    for (int qb = 0; qb < NQ; ++qb) {
      if (lim < 32) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (16 * rb + r4 + e >= lim) acc[qb][rb][e] = -INFINITY;                 // clamped duplicate rows never count
      }
      bool ok = false;                                 // FILTER: some row of the lane's 8 is inside the shard and allowed
      if constexpr (FILTER) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            // label_allows, spelled out: as a call it changed the epilogue's code and spilled six VGPRs into the tile loop
            const bool allow = (ql[qb] < 0 || ((lr[rb][e] == ql[qb]) != (a.ne != 0))) && (lim >= 32 || 16 * rb + r4 + e < lim);
            acc[qb][rb][e] = allow ? acc[qb][rb][e] : -INFINITY;
            ok = ok || allow;
          }
      }
      float tmax = max3f(acc[qb][0][0], acc[qb][0][1], acc[qb][0][2]);
      tmax = max3f(tmax, acc[qb][0][3], acc[qb][1][0]);
      tmax = max3f(tmax, acc[qb][1][1], acc[qb][1][2]);
      tmax = fmaxf(tmax, acc[qb][1][3]);
      if constexpr (SAMPLE && GROUP) {                 // rare after warm-up: one wave-uniform test skips the offers
        if (__builtin_amdgcn_ballot_w64(tmax > best[qb].v[NV - 1]) != 0) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int e = 0; e < 4; ++e) best[qb].offer(acc[qb][rb][e], g0 + 16 * rb + r4 + e);      // masked / out-of-shard scores are -inf
        }
      } else if (SAMPLE && FILTER) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int e = 0; e < 4; ++e) top4[qb].offer(acc[qb][rb][e]);
      } else if (SAMPLE) {
        gmax[qb] = fmaxf(gmax[qb], tmax);
      } else if (RANGE) {
        if (__builtin_amdgcn_ballot_w64(tmax >= tau[qb]) != 0) {      // tau[qb] = B_q: some lane holds a score that counts or is appended
          const float aq = __shfl(pack_a, qb * 16 + n16, 64), hq = __shfl(pack_h, qb * 16 + n16, 64);   // (every lane takes part)
          int q = q0 + qb * 16 + n16;
          asm volatile("" : "+v"(q));                  // opaque, as below
          if (tmax >= tau[qb] && q < a.Bq) {
            int ns = 0;
            bool keep = tmax >= aq;                    // a list candidate; or a band row (B_q >= -3e38: never a masked -inf)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float sc = acc[qb][rb][e];
                ns += sc >= hq ? 1 : 0;
                keep = keep || (sc >= tau[qb] && sc < hq);
              }
            ncand[qb] += ns;
            if (keep) {
              const int nrec = ncand[qb] >> 16;
              if (nrec < a.cap) {
                const long rec = ((long)q * nstreams + split * 4 + rq) * a.cap + nrec;
                f32x4* dst = (f32x4*)(a.rec_s + rec * 8);
                dst[0] = acc[qb][0]; dst[1] = acc[qb][1];
                a.rec_g[rec] = g0;
              }
              ncand[qb] += 1 << 16;
            }
          }
        }
      } else if (auto pass = [&] { return FILTER ? ok && tmax >= tau[qb] : tmax >= tau[qb]; }; __builtin_amdgcn_ballot_w64(pass()) != 0) {
        // Some lane of the wave has a candidate in this tile. Testing the registers one by one cost ~80 instructions per triggered tile
        // (70 us of a 270-us scan in round 2); instead a lane whose tile maximum passes appends its WHOLE 8-score column as one record
        // (2 x 16-byte stores + the tile's first row) to its private stream list, and sim_final filters the records against tau.
        // FILTER: the allow predicate decides too (tau_q = -inf admits every ALLOWED row, never a masked one)
        int q = q0 + qb * 16 + n16;
        asm volatile("" : "+v"(q));                    // opaque: keeps the list address arithmetic HERE (hoisted out of the tile loop
        if (pass() && q < a.Bq) {                      // it was spilled, and a spill reload inside the loop drains the DMA ring)
          if (ncand[qb] < a.cap) {
            const long rec = ((long)q * nstreams + split * 4 + rq) * a.cap + ncand[qb];
            f32x4* dst = (f32x4*)(a.rec_s + rec * 8);
            dst[0] = acc[qb][0]; dst[1] = acc[qb][1];  // FILTER: masked slots are -inf, sim_final_wide skips them
            a.rec_g[rec] = g0;
          }
          ++ncand[qb];
        }
      }
    }
  };
  auto mfma_tile = [&](const char* buf) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};           // C operand of the first K-step: the inline constant 0 (no v_mov per tile)
    uint4 af[4];                                       // A fragments two K-steps (four reads) ahead of the MFMAs that consume them
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = *(const uint4*)(buf + SIM_RD(i & 1, i >> 1));
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const uint4 av = af[(2 * kk + rb) & 3];
        if (kk + 2 < 8) af[(2 * kk + rb) & 3] = *(const uint4*)(buf + SIM_RD(rb, kk + 2));
#pragma unroll
        for (int qb = 0; qb < NQ; ++qb) {
          if (__is_same(TG, bf16_t))
            acc[qb][rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, qf[qb][kk]), kk == 0 ? zero : acc[qb][rb], 0, 0, 0);
          else
            acc[qb][rb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, qf[qb][kk]), kk == 0 ? zero : acc[qb][rb], 0, 0, 0);
        }
      }
  };

  // (s_setprio 1 for the younger half - waves 4-7 - before the loop, the guide's static-priority item, and a sample stride of 32 instead of 16
  // at 1M rows: no difference in a same-box A/B on the round-4 kernel. Round 5, measured with cycle stamps: priority 2 for the younger half
  // during its FIRST tile only balances the two halves, below.)
  int g_pending = -1, lo_pending = 0;                  // late waves: tile whose epilogue is still owed
#ifdef COR_PROBES
#define SC_STAMP(i_) do { if (!SAMPLE && a.stamps && blockIdx.x == 0 && (tid & 255) == 0 && t - t0 < 24) { __builtin_amdgcn_sched_barrier(0); \
    a.stamps[((tid >> 8) * 24 + (t - t0)) * 8 + (i_)] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define SC_STAMP(i_) do { } while (0)
#endif
  for (int t = t0; t < t1; ++t) {
    // super-tile t has landed once at most 4 * (super-tiles issued after t) of this wave's DMA are still outstanding (VMEM
    // retires in order; candidate stores issued in between only make the wait stricter)
    // Round 5 (cycle stamps, tools/sim_stamps.py): VMEM retires in order, so the ~5 candidate stores of a record appended in the last period
    // count among "the 4 (AHEAD - 1) youngest operations" and the wait below then also waits for copies issued one period ago (500-1 000
    // cycles per super-tile with a ring of 4). A ring of FIVE (all 160 KiB of LDS; tau_s lives in the last slot until the first barrier) puts
    // one more period between a copy's issue and the wait that can be forced onto it.
    const int later = min(t1 - 1 - t, AHEAD - 1);
    if (later >= 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (later == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (later == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    SC_STAMP(0);
    __builtin_amdgcn_s_barrier();                      // every wave's part of super-tile t is in LDS; t-1 is fully consumed
    SC_STAMP(1);
    if (t + AHEAD < t1) issue(t + AHEAD);              // -> ring slot of super-tile t-1
#ifdef COR_PROBES
    if (a.probe_same & 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // probe: how deep is the backlog? (everything but the newest super-tile)
    if (a.probe_same & 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
#endif
    SC_STAMP(2);
    const char* buf = smem + ((t - t0) % NS) * STILE;
    const int g0 = walk.tile(t) * a.tile_stride * 64, lo = (t - t0) * 64;
    if (active) {
      if (late && g_pending >= 0) epilogue(g_pending, lo_pending);
      SC_STAMP(3);
      if (late) __builtin_amdgcn_s_setprio(2);
      mfma_tile(buf);
      if (late) __builtin_amdgcn_s_setprio(0);
      SC_STAMP(4);
      epilogue(g0, lo);
      SC_STAMP(5);
      mfma_tile(buf + TILE);
      SC_STAMP(6);
      if (late) { g_pending = g0 + 32; lo_pending = lo + 32; } else epilogue(g0 + 32, lo + 32);
      SC_STAMP(7);
    }
  }
  if (active && late && g_pending >= 0) epilogue(g_pending, lo_pending);
#undef SIM_RD
  if (active) {
#pragma unroll
    for (int qb = 0; qb < NQ; ++qb) {
      const int q = q0 + qb * 16 + n16;
      if (q < a.Bq) {
        if constexpr (SAMPLE && GROUP) best[qb].store(a.sg, a.sgrow, (long)q * a.Bqp + (split * 4 + rq) * NV);
        else if (SAMPLE && FILTER) top4[qb].store(a.sg + (long)q * a.Bqp + (split * 4 + rq) * 4);
        else if (SAMPLE && WIDE) a.sg[(long)q * a.Bqp + split * 4 + rq] = f2key(gmax[qb]);                  // one writer per group: no atomic
        else if (SAMPLE) atomicMax(a.sg + (long)((split * 4 + rq) & 31) * a.Bqp + q, f2key(gmax[qb]));    // (a group without a tile: key(-inf) > 0 = empty)
        else if (RANGE) {
          a.cnt[(long)q * nstreams + split * 4 + rq] = ncand[qb] >> 16;
          a.sure[(long)q * nstreams + split * 4 + rq] = ncand[qb] & 0xffff;
        } else a.cnt[(long)q * nstreams + split * 4 + rq] = ncand[qb];
      }
    }
  }
}

// Queries rounded to the gallery dtype in the fragment order of v_mfma_f32_16x16x32: image[(qblk16 * 8 + kk) * 64 + lane] = 16 B =
// q[qblk16*16 + (lane&15)][32 kk + 8 (lane>>4) .. +8]; rows beyond Bq repeat the last query (their results are never written). Also
// clears the per-call overflow flags. One block of 256 threads per 32 queries.
template <typename TG>
__global__ void __launch_bounds__(256) sim_prep(const float* __restrict__ Q, int Bq, uint4* img, int* flags, int* ovf_q, unsigned* sg, int Bqp,
                                                float* dq) {
  __shared__ float part[32][33];                       // |q|^2 partials of the block's 32 queries: [query][K-step * 2 + lane half]
  const int qblk = blockIdx.x, tid = threadIdx.x;
  if (qblk == 0 && tid == 0) flags[0] = 0;
  if (tid < 32 && qblk * 32 + tid < Bq) ovf_q[qblk * 32 + tid] = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) sg[(long)(tid >> 5 | (i << 3)) * Bqp + qblk * 32 + (tid & 31)] = 0u;     // the 32 super-group maxima of these queries: empty
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int item = tid + 256 * i, c = item >> 6, lane = item & 63, r = lane & 31, h = lane >> 5;
    const float* qrow = Q + (long)min(qblk * 32 + r, Bq - 1) * 256;
    const uint4 f = q_frag16<TG>(qrow, c, h);           // chunk ch = 2 c + h of the query: values 8 ch .. 8 ch + 7
    // v_mfma_f32_16x16x32 fragment order: image[(qblk16 * 8 + kk) * 64 + lane'] with lane' = 16 * (ch & 3) + (query & 15), kk = ch >> 2
    { const int ch = 2 * c + h; img[((long)(qblk * 2 + (r >> 4)) * 8 + (ch >> 2)) * 64 + 16 * (ch & 3) + (r & 15)] = f; }
    float n2 = 0.f;                                    // of the values as the MFMA sees them
    const uint32_t w[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float lo, hi;
      if (__is_same(TG, bf16_t)) { lo = __uint_as_float(w[j] << 16); hi = __uint_as_float(w[j] & 0xffff0000u); }
      else { typedef _Float16 h2 __attribute__((ext_vector_type(2))); const h2 t2 = __builtin_bit_cast(h2, w[j]); lo = (float)t2[0]; hi = (float)t2[1]; }
      n2 = fmaf(lo, lo, n2); n2 = fmaf(hi, hi, n2);
    }
    part[r][c * 2 + h] = n2;
  }
  __syncthreads();
  if (tid < 32 && qblk * 32 + tid < Bq) {
    float n2 = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) n2 += part[tid][j];   // fixed order: delta_q is reproducible
    dq[qblk * 32 + tid] = SIM_DELTA * fmaxf(1.f, sqrtf(n2));
  }
}

// chain score of gallery row `idx` against the query in LDS (oracle/c/sim_chain.c order: chunk c of 8: k = 8c+i then 8c+4+i)
template <typename TG>
__device__ __forceinline__ float chain_score(const TG* __restrict__ G, long idx, const float* qs) {
  const uint4* row = (const uint4*)(G + idx * 256);
  float acc = 0.f;
#pragma unroll 4
  for (int c = 0; c < 32; ++c) {
    const uint4 v = row[c];
    float g[8];
    if (__is_same(TG, bf16_t)) {
      g[0] = __uint_as_float(v.x << 16); g[1] = __uint_as_float(v.x & 0xffff0000u); g[2] = __uint_as_float(v.y << 16); g[3] = __uint_as_float(v.y & 0xffff0000u);
      g[4] = __uint_as_float(v.z << 16); g[5] = __uint_as_float(v.z & 0xffff0000u); g[6] = __uint_as_float(v.w << 16); g[7] = __uint_as_float(v.w & 0xffff0000u);
    } else {
      const f16x8 hv = __builtin_bit_cast(f16x8, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) g[i] = (float)hv[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc = fmaf(g[i], qs[8 * c + i], acc);
      acc = fmaf(g[4 + i], qs[8 * c + 4 + i], acc);
    }
  }
  return acc;
}

// Exact fallback of ONE query (block of 256 threads): every row's chain score, per-thread sorted top-k lists in LDS (thread t
// owns slots [t*k, t*k + k) of cs/ci: 256 * k <= FS_MAX), then k rounds of block-wide arg-best by (score desc, index asc).
template <typename TG, int NT = 256>
__device__ void brute_force_topk(const TG* __restrict__ G, int Ng, const float* qs, float* cs, int* ci, int k, long long g_offset,
                                 float* out_s, long long* out_i) {
  constexpr int NW = NT / 64;
  __shared__ float rs[NW]; __shared__ int ri[NW], rp[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, base = tid * k;
  for (int j = 0; j < k; ++j) { cs[base + j] = -INFINITY; ci[base + j] = INT_MAX; }
  for (int g = tid; g < Ng; g += NT) {                  // ascending rows: a tie keeps the earlier (smaller) index ahead
    const float sc = chain_score<TG>(G, g, qs);
    if (sc > cs[base + k - 1]) {
      int j = k - 1;
      while (j > 0 && sc > cs[base + j - 1]) { cs[base + j] = cs[base + j - 1]; ci[base + j] = ci[base + j - 1]; --j; }
      cs[base + j] = sc; ci[base + j] = g;
    }
  }
  __syncthreads();
  const int n = NT * k;
  for (int round = 0; round < k; ++round) {
    float bs = -INFINITY; int bi = INT_MAX, bp = -1;
    for (int i = tid; i < n; i += NT)
      if (ci[i] != INT_MAX && (bp < 0 || cs[i] > bs || (cs[i] == bs && ci[i] < bi))) { bs = cs[i]; bi = ci[i]; bp = i; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64); const int oi = __shfl_xor(bi, o, 64), op = __shfl_xor(bp, o, 64);
      if (op >= 0 && (bp < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; bp = op; }
    }
    if (lane == 0) { rs[wave] = bs; ri[wave] = bi; rp[wave] = bp; }
    __syncthreads();
    if (tid == 0) {
      float fs = rs[0]; int fi = ri[0], fp = rp[0];
      for (int w = 1; w < NW; ++w) if (rp[w] >= 0 && (fp < 0 || rs[w] > fs || (rs[w] == fs && ri[w] < fi))) { fs = rs[w]; fi = ri[w]; fp = rp[w]; }
      out_s[round] = fp >= 0 ? fs : -INFINITY;
      out_i[round] = fp >= 0 ? (long long)fi + g_offset : -1LL;
      if (fp >= 0) ci[fp] = INT_MAX;
    }
    __syncthreads();
  }
}

// chain score of a gallery row staged in LDS (32 chunks of 16 B; chunk c sits in slot c ^ x): the order of oracle/c/sim_chain.c
template <typename TG>
__device__ __forceinline__ float chain_score_lds(const char* row, int x, const float* qs) {
  float acc = 0.f;
#pragma unroll 4
  for (int c = 0; c < 32; ++c) {
    const uint4 v = *(const uint4*)(row + ((c ^ x) << 4));
    const f32x4 qa = *(const f32x4*)(qs + 8 * c), qb = *(const f32x4*)(qs + 8 * c + 4);
    float g[8];
    if (__is_same(TG, bf16_t)) {
      g[0] = __uint_as_float(v.x << 16); g[1] = __uint_as_float(v.x & 0xffff0000u); g[2] = __uint_as_float(v.y << 16); g[3] = __uint_as_float(v.y & 0xffff0000u);
      g[4] = __uint_as_float(v.z << 16); g[5] = __uint_as_float(v.z & 0xffff0000u); g[6] = __uint_as_float(v.w << 16); g[7] = __uint_as_float(v.w & 0xffff0000u);
    } else {
      const f16x8 hv = __builtin_bit_cast(f16x8, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) g[i] = (float)hv[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc = fmaf(g[i], qa[i], acc);
      acc = fmaf(g[4 + i], qb[i], acc);
    }
  }
  return acc;
}

// D. exact top-k of one query's candidates. LDS: cs/ci [FS_MAX] | sl_s/sl_i [SL_MAX] | qs[256] | hist[256].
template <typename TG>
__global__ void __launch_bounds__(256) sim_final(const float* __restrict__ Q, const TG* __restrict__ G, const float* rec_s, const int* rec_g,
                                                 const float* tau, const int* cnt, int nstreams, int cap, int Ng, int k, long long g_offset,
                                                 float* out_s, long long* out_i, int* flags, int* ovf_q, int no_fallback) {
  extern __shared__ __attribute__((aligned(16))) char fsraw[];
  float* cs = (float*)fsraw; int* ci = (int*)(cs + FS_MAX);
  float* sl_s = (float*)(ci + FS_MAX); int* sl_i = (int*)(sl_s + SL_MAX);
  float* qs = (float*)(sl_i + SL_MAX); int* hist = (int*)(qs + 256);
  __shared__ int ovf, total, nsl, sel_bin, k_rem;
  __shared__ float qn2[4];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { ovf = 0; total = 0; nsl = 0; }
  const float qv = round_to<TG>(Q[(long)q * 256 + tid]);          // the query as the MFMA saw it
  qs[tid] = qv;
  const float part = wave_sum(qv * qv);
  if (lane == 0) qn2[wave] = part;
  __syncthreads();
  const float delta = SIM_DELTA * fmaxf(1.f, sqrtf(qn2[0] + qn2[1] + qn2[2] + qn2[3]));
  // 1. the private stream lists hold whole 8-score columns (records: two 16-row blocks x four rows of one lane quarter): keep the scores
  // >= tau_q (the admission threshold of the scan, delta already subtracted) and compact them into LDS. Score [g][i] of lane quarter rq is
  // row g0 + 16 g + 4 rq + i.
  const float tq = tau[q];
  auto take = [&](const f32x4 (&v)[2], int g0, int r4) {            // ONE returning LDS atomic per record (round 2: one per passing score,
    int np = 0;                                                       // up to 16 dependent LDS round trips per record)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) np += (v[g][i] >= tq && v[g][i] > -INFINITY) ? 1 : 0;
    if (np == 0) return;
    int p = atomicAdd(&total, np);
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (v[g][i] >= tq && v[g][i] > -INFINITY) {
          if (p < FS_MAX) { cs[p] = v[g][i]; ci[p] = g0 + i + 16 * g + r4; }
          ++p;
        }
  };
  // Two round trips: the thread's (up to four: 1024 streams) COUNTS first - contiguous per query, coalesced - then record 0 of its non-empty
  // streams, all issued together. (Rounds 3-4 fetched record 0 WITH the count, one trip: with 1000 mostly empty streams per query that is
  // 2 000 scattered 32-byte sectors per query, 64 MB per 512-query search: 5.5 us slower than this at 32k-125k rows.)
  for (int st0 = 0; st0 < nstreams; st0 += 1024) {
    int cc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int st = st0 + 256 * u + tid;
      cc[u] = st < nstreams ? cnt[(long)q * nstreams + st] : 0;
    }
    f32x4 v0[4][2]; int g00[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int st = st0 + 256 * u + tid;
      if (cc[u] > 0) {
        const long rec0 = ((long)q * nstreams + st) * cap;
        const f32x4* src = (const f32x4*)(rec_s + rec0 * 8);
        v0[u][0] = src[0]; v0[u][1] = src[1];
        g00[u] = rec_g[rec0];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int st = st0 + 256 * u + tid;
      if (cc[u] > cap) ovf = 1;
      const int n = min(cc[u], cap), r4 = 4 * (st & 3);
      if (n > 0) take(v0[u], g00[u], r4);
      if (n > 1) {
        const long rec0 = ((long)q * nstreams + st) * cap;
        for (int j = 1; j < n; ++j) {
          const f32x4* sj = (const f32x4*)(rec_s + (rec0 + j) * 8);
          const f32x4 vj[2] = {sj[0], sj[1]};
          take(vj, rec_g[rec0 + j], r4);
        }
      }
    }
  }
  __syncthreads();
  if (total > FS_MAX) ovf = 1;
  const int n = min(total, FS_MAX);
  __syncthreads();
  // 2. T_lo <= T = k-th best MFMA score (2-pass radix select over order-preserving keys); n <= k: every candidate is in
  float T = -INFINITY;
  if (!ovf && n > k) {
    unsigned prefix = 0;
    if (tid == 0) k_rem = k;
    for (int pass = 0; pass < 2; ++pass) {               // 16 key bits: sign, exponent, 7 mantissa bits
      const int shift = 24 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < n; i += 256) {
        const unsigned key = f2key(cs[i]);
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1);
      }
      __syncthreads();
      if (wave == 0) {                                   // bins 4*lane .. 4*lane+3; suffix sums from the top bin down
        const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const int mine = h0 + h1 + h2 + h3;
        int above = mine;                                // inclusive suffix sum over lanes >= this one
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(above, o, 64); if (lane + o < 64) above += t; }
        above -= mine;                                   // elements in bins above this lane's four
        const int kr = k_rem;
        if (above < kr && kr <= above + mine) {          // exactly one lane
          int a3 = above, b = 3;
          if (kr <= a3 + h3) b = 3; else { a3 += h3; if (kr <= a3 + h2) b = 2; else { a3 += h2; if (kr <= a3 + h1) b = 1; else { a3 += h1; b = 0; } } }
          sel_bin = 4 * lane + b; k_rem = kr - a3;
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | (unsigned)sel_bin;
      __syncthreads();
    }
    // T_lo = the smallest float whose key starts with the k-th best score's 16 bits: T_lo <= T (within 2^-7 relative), so the
    // short list cut T_lo - delta admits a superset of what T - delta would (exactness is unaffected; two passes saved)
    const unsigned key_lo = prefix << 16;
    const unsigned u = (key_lo & 0x80000000u) ? (key_lo & 0x7fffffffu) : ~key_lo;
    T = __uint_as_float(u);
  }
  // 3. short list: MFMA score >= T - delta
  if (!ovf) {
    const float cut = T - delta;
    for (int i = tid; i < n; i += 256) {
      if (cs[i] >= cut) {
        const int p = atomicAdd(&nsl, 1);
        if (p < SL_MAX) sl_i[p] = ci[i];
      }
    }
  }
  __syncthreads();
  if (nsl > SL_MAX) ovf = 1;
  __syncthreads();
  if (ovf) {
    // Candidate overflow (a stream list, the LDS buffer or the short list: pathological score distributions such as tens of
    // thousands of identical rows). No host round trip and no second launch: THIS block ranks the whole shard for its query
    // with the exact chain (256 threads x Ng / 256 rows x 256 dependent fmaf: ~2 ms per query at 1M rows - slow, exact, rare).
    if (tid == 0) { ovf_q[q] = 1; atomicOr(flags, 1); }
    if (no_fallback) {                                   // tests: expose the raw overflow marker
      for (int j = tid; j < k; j += 256) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -2LL; }
      return;
    }
    __syncthreads();
    brute_force_topk<TG>(G, Ng, qs, cs, ci, k, g_offset, out_s + (long)q * k, out_i + (long)q * k);
    return;
  }
  const int m = nsl;
  // 4. exact re-scoring: the fmaf chain of oracle/c/sim_chain.c (chunk c = 0..31 of 8: k = 8c+i then 8c+4+i, i = 0..3)
  // The rows arrive by LDS-DMA in the candidate buffer (dead from here: 64 rows x 512 B per round, wave w stages rows 16 w ..; slot
  // (lane & 31) of row j is fed from source chunk (lane & 31) ^ (j & 31)), all in flight at once; then thread j runs the chain over
  // its row. Round 2 read the rows from global memory inside the chain: 32 loads, four in flight = eight dependent round trips.
  {
    const int lane_ = tid & 63, wave_ = tid >> 6;
    const unsigned ldsR = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((__attribute__((address_space(3))) char*)cs)) + (unsigned)wave_ * 8192u;
    for (int base = 0; base < m; base += 64) {
      const int nr = min(64, m - base);
      __syncthreads();                                   // the candidate buffer / the previous round's rows are no longer read
#pragma unroll 1
      for (int i = 0; i < 8; ++i) {
        const int jj = wave_ * 16 + 2 * i + (lane_ >> 5);
        if (wave_ * 16 + 2 * i < nr) {                   // wave-uniform
          const long idx = sl_i[base + min(jj, nr - 1)];
          glds16(G + idx * 256 + (((lane_ & 31) ^ (jj & 31)) << 3), __builtin_amdgcn_readfirstlane(ldsR + 1024u * i));
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid < nr) sl_s[base + tid] = chain_score_lds<TG>((const char*)cs + tid * 512, tid & 31, qs);
    }
  }
  __syncthreads();
  // 5. rank by (chain score desc, index asc); entries beyond the short list (Ng < k) are (-inf, -1)
  for (int j = tid; j < m; j += 256) {
    const float s = sl_s[j]; const int idx = sl_i[j];
    int rank = 0;
    for (int i = 0; i < m; ++i) rank += (sl_s[i] > s || (sl_s[i] == s && sl_i[i] < idx)) ? 1 : 0;
    if (rank < k) { out_s[(long)q * k + rank] = s; out_i[(long)q * k + rank] = (long long)idx + g_offset; }
  }
  for (int j = m + tid; j < k; j += 256) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -1LL; }
}

__device__ __forceinline__ bool better(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// one block per query: k rounds of block-wide arg-best over nparts*KMAX candidates held in LDS.
__global__ void __launch_bounds__(256) sim_topk_merge(const float* ws_s, const int* ws_i, int n, int k, long long g_offset,
                                                      float* out_s, long long* out_i, const int* gate_q) {
  if (gate_q && gate_q[blockIdx.x] == 0) return;                // fallback: only the queries whose candidate lists overflowed
  extern __shared__ __attribute__((aligned(16))) char smraw[];
  float* cs = (float*)smraw; int* ci = (int*)(cs + n);
  __shared__ float rs[4]; __shared__ int ri[4]; __shared__ int rp[4];
  const int qb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < n; i += 256) { cs[i] = ws_s[(long)qb * n + i]; ci[i] = ws_i[(long)qb * n + i]; }
  __syncthreads();
  for (int round = 0; round < k; ++round) {
    float bs = -INFINITY; int bi = INT_MAX, bp = -1;
    for (int i = tid; i < n; i += 256)
      if (bp < 0 || better(cs[i], ci[i], bs, bi)) { bs = cs[i]; bi = ci[i]; bp = i; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64); const int oi = __shfl_xor(bi, o, 64), op = __shfl_xor(bp, o, 64);
      if (op >= 0 && (bp < 0 || better(os, oi, bs, bi) || (os == bs && oi == bi && op < bp))) { bs = os; bi = oi; bp = op; }
    }
    if (lane == 0) { rs[wave] = bs; ri[wave] = bi; rp[wave] = bp; }
    __syncthreads();
    if (tid == 0) {
      float fs = rs[0]; int fi = ri[0], fp = rp[0];
      for (int w = 1; w < 4; ++w)
        if (rp[w] >= 0 && (fp < 0 || better(rs[w], ri[w], fs, fi) || (rs[w] == fs && ri[w] == fi && rp[w] < fp))) { fs = rs[w]; fi = ri[w]; fp = rp[w]; }
      out_s[(long)qb * k + round] = fs;
      out_i[(long)qb * k + round] = (fi == INT_MAX) ? -1LL : (long long)fi + g_offset;
      if (fp >= 0) { cs[fp] = -INFINITY; ci[fp] = INT_MAX; }
    }
    __syncthreads();
  }
}

inline int device_cus() { return cor_device_cus(); }

// ---------------------------------------------------------------------------------------------------------------------
// v4 (16-bit galleries, C = 256, SMALL shards - the 8-GPU shard shapes of BASELINE configs[2], 256..512 x 12.5k - and few queries
// against up to ~130k rows): TWO launches and LOCAL thresholds instead of prep -> sample scan -> tau -> append scan -> final.
//   sim_block_scan: a block = 32 * QB queries x one gallery slice of 256 * T rows. Every wave owns ALL the block's queries (their
//     K-fragments in registers) and 32 * T rows of its own, which reach its PRIVATE 16-KiB LDS buffer by LDS-DMA in K-half tiles
//     (no block barrier inside the scan); the 16 * T * QB scores of a lane STAY IN REGISTERS. The block then knows, per query, 64
//     disjoint row classes' maxima; their k-th largest is a lower bound of the query's k-th best score over the whole shard (k
//     classes each hold a row at least that good), so rows below it minus delta_q cannot be in the answer: the lanes append the
//     few registers that pass (~k per query and slice) to per-(query, slice) lists. No sample pass, no global threshold, no
//     second scan, no atomics on global memory.
//   sim_final_wave: ONE WAVE per query gathers its lists, finds the k-th best MFMA score by a counting binary search, re-scores
//     the short list with the exact fp32 fmaf chain (rows staged by LDS-DMA, all in flight at once) and ranks it.
// Exactness (same argument as v3, with the slice's own threshold): let T_b be the k-th best MFMA score inside slice b. The k best
// rows of slice b have chain scores >= T_b - eps, so the shard's k-th best chain score is >= T_b - eps for EVERY b; a row g of the
// exact answer therefore has MFMA score >= T_b(g) - 2 eps >= tau_b(g) - delta and is appended by its block. Every row of the MFMA
// top-k is appended too (global k-th best >= local k-th best), so the final's T is the shard's k-th best MFMA score and the short
// list {MFMA score >= T - delta} holds the exact answer. A kernel boundary between the two costs ~1.5 us; keeping the selection in
// the scan launch would need an agent-scope release + counter + acquire (~3.4 us by the MI355X guide's price list) and one block
// ranking 32-64 queries: measured choice, see DESIGN 3.4.
constexpr int SB_NC = 4096;                            // candidates per query held in LDS by sim_final_wave (32 KiB)
constexpr int SB_SL = 64;                              // short list (one entry per lane)
constexpr int SB_MAXSL = 192;                          // slices per query the wave final can gather (make_small keeps nslices below)

struct SmallPlan {
  bool ok;
  int qb, T, nqg, nslices, cap, grid, xcd_map;
  size_t off_flags, off_ovf, off_cnt, off_cand, bytes;
};
inline SmallPlan make_small(int Bq, int Ng, int k) {
  SmallPlan p{};
  p.qb = Bq > 32 ? 2 : 1;
  p.nqg = cdiv(Bq, 32 * p.qb);
  const int tmax = p.qb == 2 ? 2 : 4;                  // accumulators: 16 * T * QB <= 64 registers
  // A block's time is a LATENCY chain (~11 us: query conversion, two DMA round trips, threshold, append), not throughput, and the
  // selection kernel's time grows with the candidates (~12 per slice and query): the fewest, largest slices that still fit one
  // round of blocks. Shapes that need a second round (512 x 32 000: 55 us here against 48 on the global-threshold pipeline) or more
  // than 32 slices per query stay on the global-threshold pipeline.
  int t = cdiv(Ng, 256);
  p.T = t <= 1 ? 1 : (t == 2 ? 2 : tmax);              // instantiated: 1, 2, (4 for QB = 1)
  if (p.T > tmax) p.T = tmax;
  p.nslices = cdiv(Ng, 256 * p.T);
  p.cap = k <= 12 ? 128 : 256;                         // entries per (query, slice) list: ~k + 2 expected; a sparse last slice: all its rows
  p.xcd_map = p.nslices >= 8 ? 1 : 0;                  // blocks that share a gallery slice share an XCD (its L2)
  p.grid = p.nqg * (p.xcd_map ? ((p.nslices + 7) & ~7) : p.nslices);
  // k <= 16: the threshold is the k-th largest of 32 class maxima; near k = 32 it is their MINIMUM, a weak and volatile bound (one query
  // of 300 overflowed a 256-entry list at 300 x 5 000, k = 32): such searches keep the global threshold
  p.ok = k <= 16 && p.nslices <= 32 && p.nqg * p.nslices <= device_cus() && (long)p.nslices * (k + 8) * 13 / 10 <= 3072 && p.nslices <= SB_MAXSL;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 255) & ~(size_t)255; return at; };
  p.off_flags = take(16);
  p.off_ovf = take((size_t)Bq * 4);
  p.off_cnt = take((size_t)Bq * p.nslices * 4);
  p.off_cand = take((size_t)Bq * p.nslices * p.cap * 8);
  p.bytes = o;
  return p;
}


template <typename TG, int QB, int T>
__global__ void __launch_bounds__(512, 2) sim_block_scan(const float* __restrict__ Q, const TG* __restrict__ G, int Bq, int Ng, int k, int nqg,
                                                         int nslices, int xcd_map, int cap, int* __restrict__ cnt, uint2* __restrict__ cand,
                                                         int* __restrict__ flags, unsigned long long* __restrict__ stamps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef COR_PROBES
  unsigned long long ts_[10]; int nts_ = 0;
#define SB_STAMP() do { __builtin_amdgcn_sched_barrier(0); ts_[nts_++] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define SB_STAMP() do { } while (0)
#endif
  constexpr int QPB = 32 * QB, ZB = QB * 16 * 64 * 16, TPQ = 512 / QPB, FPT = 256 / TPQ, VPT = 64 / TPQ, CS = QPB + 1;
  constexpr int RPW = 32 * T, RPB = 8 * RPW;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, h = lane >> 5;
  int slice, qg;
  if (xcd_map) { const int x = blockIdx.x & 7, j = blockIdx.x >> 3; slice = (j / nqg) * 8 + x; qg = j % nqg; }
  else { slice = blockIdx.x / nqg; qg = blockIdx.x % nqg; }
  if (slice >= nslices) return;                        // padding blocks of the XCD mapping (whole block, before any barrier)
  if (blockIdx.x == 0 && tid == 0) flags[0] = 0;       // per-call overflow flag (the final kernel runs behind this one)
  const int q0 = qg * QPB;
  // A short (last) slice spreads its rows EVENLY over the eight waves (floor(rows / 8) each, the remainder one apiece, instead of 32 T), so
  // that the 32 row classes below stay populated: a wave with >= 8 rows fills its four classes, hence every slice with >= 64 rows has
  // all 32 (k <= 32 of them are needed), and a slice with fewer rows may well declare every row a candidate - the list holds >= 128.
  // (Seen at 32 x 12 500: 212 rows in two waves, 8 classes < k, threshold -inf, 212 candidates per query, every query on the brute-force
  // fallback; and at 300 x 5 000, k = 32: 392 rows in seven waves, 28 classes, the same.)
  const long slice0 = (long)slice * RPB;
  const int rows_here = (int)(Ng - slice0 < RPB ? Ng - slice0 : RPB);
  const int rpw = rows_here >> 3, rem = rows_here & 7; // floor(rows / 8) per wave, the first `rem` waves one more: >= 8 each from 64 rows up
  const long w0 = slice0 + wave * rpw + (wave < rem ? wave : rem);          // this wave's first gallery row
  const int own = rpw + (wave < rem ? 1 : 0);          // rows this wave owns (wave-uniform): 32 T in a full slice
  const int ntw = (own + 31) >> 5;                     // 32-row tiles this wave scans (<= T)
  const int nsteps = 2 * ntw;                          // K-half tiles

  char* Z = smem;                                      // query image (prologue), then class maxima / thresholds / list counters
  char* Aw = smem + ZB + wave * 16384;                 // this wave's two 8-KiB K-half buffers (32 rows x 256 B)
  const unsigned ldsA = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((__attribute__((address_space(3))) char*)Aw));
  const int rowl = lane >> 4, sl = lane & 15;
  auto issue = [&](int s) {                            // K-half tile s = 2 t + p -> buffer p. LDS image lane-linear: 4 rows x 256 B per
    const int t = s >> 1, p = s & 1;                   // wave-instruction; slot sl of row `row` holds source chunk sl ^ (row & 15)
    const long g0 = w0 + 32 * t;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = 4 * i + rowl;
      long gr = g0 + row;
      gr = gr < Ng ? gr : (long)Ng - 1;                // clamped duplicates are masked to -inf below
      glds16(G + gr * 256 + ((sl ^ (row & 15)) + 16 * p) * 8, __builtin_amdgcn_readfirstlane(ldsA + p * 8192 + 1024 * i));
    }
  };
  SB_STAMP();                                          // 0: start
  if (nsteps > 0) issue(0);
  if (nsteps > 1) issue(1);

  // queries -> gallery dtype, MFMA-fragment order in Z: image[(qblk * 16 + c) * 64 + lane'] = q[qblk*32 + (lane'&31)][16c + 8(lane'>>5) ..+8]
  // thread (query qq, part pp) converts FPT consecutive values: whole 16-value K-steps c = pp * FPT / 16 ...
  const int qq = tid / TPQ, pp = tid % TPQ;
  float nrm2 = 0.f;
  {
    const float* qrow = Q + (long)min(q0 + qq, Bq - 1) * 256 + pp * FPT;
#pragma unroll
    for (int j = 0; j < FPT / 8; ++j) {                // one 16-byte fragment piece = 8 values
      const f32x4 lo = *(const f32x4*)(qrow + 8 * j), hi = *(const f32x4*)(qrow + 8 * j + 4);
      const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float x = round_to<TG>(v[i]); nrm2 = fmaf(x, x, nrm2); }
      const int kpos = pp * FPT + 8 * j, c = kpos >> 4, hh = (kpos >> 3) & 1;
      ((uint4*)Z)[((qq >> 5) * 16 + c) * 64 + hh * 32 + (qq & 31)] = q_frag16_vals<TG>(lo, hi);
    }
#pragma unroll
    for (int o = 1; o < TPQ; o <<= 1) nrm2 += __shfl_xor(nrm2, o, 64);   // the TPQ threads of a query are adjacent lanes: every one holds |q|^2
  }
  __syncthreads();
  uint4 qf[QB][16];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int c = 0; c < 16; ++c) qf[qb][c] = ((const uint4*)Z)[(qb * 16 + c) * 64 + lane];
  __syncthreads();                                     // Z is free from here on
  SB_STAMP();                                          // 1: queries converted, fragments in registers
  float* cmx = (float*)Z;                              // [32 classes][CS]: class = (wave * 2 + h) * 2 + j ; padded stride: conflict-free both ways
  float* thr = cmx + 32 * CS;                          // [QPB]
  int* lcnt = (int*)(thr + QPB);                       // [QPB]
  float* dlt = (float*)(lcnt + QPB);                   // [QPB] delta_q
  float* smx = dlt + QPB;                              // [QPB] kth: the k-th largest class maximum (the level an overflowing list is re-cut ABOVE)
  int* lcnt2 = (int*)(smx + QPB);                      // [QPB] entries of the re-cut list
  if (pp == 0) dlt[qq] = SIM_DELTA * fmaxf(1.f, sqrtf(nrm2));

  f32x16 acc[QB][T];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[qb][t][e] = 0.f;
  const int rd_base = r * 256 + (((h ^ r) & 1) << 4), rd_x = (r >> 1) & 7;     // chunk (2c' + h) ^ (r & 15) of row r
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t < ntw) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int s = 2 * t + p;
        // K-half tile s has landed once at most the 8 copies of tile s + 1 are outstanding (VMEM retires in order)
        if (s + 1 < nsteps) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const char* buf = Aw + p * 8192;
        uint4 af[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) af[c] = *(const uint4*)(buf + rd_base + ((c ^ rd_x) << 5));
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const uint4 av = af[c & 3];
          if (c + 4 < 8) af[c & 3] = *(const uint4*)(buf + rd_base + (((c + 4) ^ rd_x) << 5));
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) {
            if (__is_same(TG, bf16_t))
              acc[qb][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, qf[qb][8 * p + c]), acc[qb][t], 0, 0, 0);
            else
              acc[qb][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, qf[qb][8 * p + c]), acc[qb][t], 0, 0, 0);
          }
        }
        if (s + 2 < nsteps) {                          // buffer p is consumed (its reads fed the MFMAs above): refill it two steps ahead
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          issue(s + 2);
        }
      }
    }
  }
  SB_STAMP();                                          // 2: scan done
  // rows beyond the wave's share (the next wave's rows, clamped duplicates, absent tiles) never count: only a short slice has any
  if (own < RPW) {                                     // (a full slice: own == 32 T)
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (32 * t + (e & 3) + 8 * (e >> 2) + 4 * h >= own) acc[qb][t][e] = -INFINITY;
  }
  // class maxima: 32 disjoint row classes per query and block = (wave, lane half, register parity); their k-th largest is a lower
  // bound of the query's k-th best score in the shard (k classes each hold a row at least that good)
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    float c0 = -INFINITY, c1 = -INFINITY;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int e = 0; e < 16; e += 2) { c0 = fmaxf(c0, acc[qb][t][e]); c1 = fmaxf(c1, acc[qb][t][e + 1]); }
    cmx[((wave * 2 + h) * 2 + 0) * CS + qb * 32 + r] = c0;
    cmx[((wave * 2 + h) * 2 + 1) * CS + qb * 32 + r] = c1;
  }
  __syncthreads();
  SB_STAMP();                                          // 3: class maxima exchanged
  // tau_q = k-th largest of the 32 class maxima: lane <-> query, a 32-element bitonic network in registers (the K-fragments are dead),
  // 240 compare-exchanges for all 64 queries at once. (First forms: TPQ lanes per query with ds_bpermute count reductions, ~3 us;
  // one scalar counting search per query, 130 cycles per step of a serial v_cmp -> s_bcnt1 -> s_cselect chain: 8 us.)
  if (wave == 0 && lane < QPB) {
    float v[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) v[c] = cmx[c * CS + lane];
#pragma unroll
    for (int kk = 2; kk <= 32; kk <<= 1)
#pragma unroll
      for (int j = kk >> 1; j > 0; j >>= 1)
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          const int l = i ^ j;
          if (l > i) {
            const float x = v[i], y = v[l];
            if ((i & kk) == 0) { v[i] = fmaxf(x, y); v[l] = fminf(x, y); }      // descending
            else               { v[i] = fminf(x, y); v[l] = fmaxf(x, y); }
          }
        }
    float kth = v[0];
#pragma unroll
    for (int c = 1; c < 32; ++c) kth = (c == k - 1) ? v[c] : kth;
    smx[lane] = kth;
    lcnt2[lane] = 0;
    // (fewer than k classes hold a row: -inf, every real row is a candidate; the floor keeps masked -inf scores out with ONE compare)
    thr[lane] = fmaxf(kth - dlt[lane], -3.0e38f);
    lcnt[lane] = 0;
  }
  __syncthreads();
  SB_STAMP();                                          // 4: thresholds
  // append the registers that pass to the block's per-query lists (the A buffers are free: every wave is past its scan). One LDS
  // atomic per lane and query block reserves room for the lane's passing registers; the stores are EXEC-masked, not branched: hipcc
  // turned `if (pass) store` into 64 taken branches per wave (9 000 cycles of a 45 000-cycle block), so each register is one
  // v_cmp -> s_and_saveexec -> ds_write2_b32 (score, row) -> address += 8 -> restore exec, in inline asm.
  uint2* lst = (uint2*)(smem + ZB);                    // [QPB][cap]
  const unsigned lds_lst = (unsigned)(size_t)((__attribute__((address_space(3))) char*)(smem + ZB));
  // pass 0: everything >= kth - delta. pass 1 (round 5), only for queries whose pass-0 list overflowed: a slice of duplicates ties
  // hundreds of rows AT its own k-th class maximum for every query; the list is re-cut to the rows strictly ABOVE kth (few: they sit in
  // fewer than k of the 32 row classes), and kth stays behind as the level of what was left out. sim_final_wave skips the left-out
  // rows when that level is below the query's short-list cut (exact: every row of the answer has an MFMA score >= the cut), so only a
  // query the duplicated row is really close to still takes the brute-force path (rounds 1-4: every query of the call did).
  auto append = [&](const int pass) __attribute__((always_inline)) {
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      const int ql = qb * 32 + r;
      float tq = (q0 + ql < Bq) ? thr[ql] : INFINITY;              // padding queries never append
      if (pass == 1) tq = (q0 + ql < Bq && lcnt[ql] > cap) ? __uint_as_float(__float_as_uint(smx[ql]) + (smx[ql] >= 0.f ? 1u : -1u)) : INFINITY;   // next float above kth
      int* counter = pass == 0 ? lcnt : lcnt2;
      int np = 0;
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) np += acc[qb][t][e] >= tq ? 1 : 0;
      const int pos0 = np > 0 ? atomicAdd(&counter[ql], np) : 0;
      if (pos0 + np > cap - pass) tq = INFINITY;                   // the list is full: this lane stores nothing; the count flags the query
      unsigned addr = lds_lst + (unsigned)(ql * cap + pos0) * 8u;
      const unsigned rowb = (unsigned)w0 + 4u * h;
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const unsigned rowv = rowb + (unsigned)(32 * t + (e & 3) + 8 * (e >> 2));
          unsigned long long sv;
          asm volatile("v_cmp_ge_f32 vcc, %2, %3\n\ts_and_saveexec_b64 %1, vcc\n\tds_write2_b32 %0, %2, %4 offset1:1\n\tv_add_u32 %0, 8, %0\n\ts_mov_b64 exec, %1"
                       : "+v"(addr), "=&s"(sv) : "v"(acc[qb][t][e]), "v"(tq), "v"(rowv) : "vcc", "memory");
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // the asm stores are invisible to hipcc's counter bookkeeping
    __syncthreads();
  };
  append(0);
  {
    bool over = false;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) over = over || (q0 + qb * 32 + r < Bq && lcnt[qb * 32 + r] > cap);
    int* any_over = lcnt2 + QPB;                                   // (inside Z: the kernel's LDS is allocated to the last byte at QB = 2)
    if (tid == 0) *any_over = 0;
    __syncthreads();
    if (over) *any_over = 1;
    __syncthreads();
    if (*any_over) append(1);                                      // (block-uniform)
  }
  SB_STAMP();                                          // 5: lists filled
  if (q0 + qq < Bq) {
    const int n_raw = lcnt[qq], n = min(n_raw, cap);
    const long li = (long)(q0 + qq) * nslices + slice;
    if (n_raw > cap) {
      // overflow: cnt = cap + 1 + n2 (n2 <= cap - 1 entries strictly above kth follow entry 0 = {kth, marker}); 2 cap + 1: even the re-cut
      // list overflowed (nothing usable: the query takes the brute-force path)
      const int n2 = lcnt2[qq];
      const bool hard = n2 > cap - 1;
      if (pp == 0) { cnt[li] = hard ? 2 * cap + 1 : cap + 1 + n2; cand[li * cap] = make_uint2(__float_as_uint(smx[qq]), 0xFFFFFFFFu); }
      if (!hard)
        for (int j = pp; j < n2; j += TPQ) cand[li * cap + 1 + j] = lst[qq * cap + j];
    } else {
      if (pp == 0) cnt[li] = n_raw;
      for (int j = pp; j < n; j += TPQ) cand[li * cap + j] = lst[qq * cap + j];
    }
  }
#ifdef COR_PROBES
  SB_STAMP();                                          // 6: written out
  if (stamps && lane == 0) {
    for (int i = 0; i < nts_; ++i) stamps[((long)blockIdx.x * 8 + wave) * 8 + i] = ts_[i];
  }
#endif
#undef SB_STAMP
}

// ONE WAVE per query: gather the candidates, select, re-score exactly, rank. Two gather front ends: RECORDS = false: the
// per-(query, slice) entry lists of sim_block_scan (cnt / cand; nl = slices); RECORDS = true: the per-(query, stream) records of
// sim_scan<APPEND> (cnt / rec_s / rec_g; nl = streams; a record = the 8 scores of one lane's accumulator column + the tile's
// first row; the scores >= tau_q are kept).
template <typename TG, bool RECORDS>
__global__ void __launch_bounds__(64) sim_final_wave(const float* __restrict__ Q, const TG* __restrict__ G, const int* __restrict__ cnt,
                                                     const uint2* __restrict__ cand, const float* __restrict__ rec_s, const int* __restrict__ rec_g,
                                                     const float* __restrict__ tau, int nslices, int cap, int Ng, int k, long long g_offset,
                                                     float* out_s, long long* out_i, int* flags, int* ovf_q, int no_fallback) {
  __shared__ __attribute__((aligned(16))) float cs[SB_NC];
  __shared__ __attribute__((aligned(16))) int ci[SB_NC];
  __shared__ __attribute__((aligned(16))) char rows[32 * 512];
  __shared__ __attribute__((aligned(16))) float qs[256];
  __shared__ float sl_s[SB_SL];
  __shared__ int sl_i[SB_SL];
  const int q = blockIdx.x, lane = threadIdx.x;
  // (the first 64 list lengths are requested together with the query row: one global round trip instead of two)
  const int c_first = (!RECORDS && lane < nslices) ? cnt[(long)q * nslices + lane] : 0;
  {
    const f32x4 v = *(const f32x4*)(Q + (long)q * 256 + 4 * lane);
    float n2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float x = round_to<TG>(v[i]); qs[4 * lane + i] = x; n2 = fmaf(x, x, n2); }
    n2 = wave_sum(n2);
    sl_s[lane] = n2;                                   // (parked: read back as delta below, after the barrier)
  }
  int n = 0;
  bool ovf = false, lists_over = false;
  __shared__ bool sovf[SB_MAXSL];
  if (RECORDS) {
    // 1r. lane <-> stream; record 0 of every stream is fetched TOGETHER with the stream's count (most streams hold 0 or 1 records):
    // one global round trip instead of three dependent ones. Score [g][i] of lane quarter r4 / 4 is row g0 + 16 g + r4 + i.
    __shared__ int total;
    if (lane == 0) total = 0;
    __syncthreads();
    const float tq = tau[q];
    auto take = [&](const f32x4 (&v)[2], int g0, int r4) {          // one LDS atomic per record (not per score), then predicated stores
      int np = 0;
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) np += (v[g][i] >= tq && v[g][i] > -INFINITY) ? 1 : 0;
      if (np == 0) return;
      int pos = atomicAdd(&total, np);
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (v[g][i] >= tq && v[g][i] > -INFINITY) {
            if (pos < SB_NC) { cs[pos] = v[g][i]; ci[pos] = g0 + i + 16 * g + r4; }
            ++pos;
          }
    };
    // the loads of up to 8 streams per lane (512 of up to 1024 streams) are issued together: one global round trip, not one per 64 streams
    constexpr int RS = 8;
    for (int sb = 0; sb < nslices; sb += 64 * RS) {
      f32x4 v0[RS][2]; int g00[RS], cc[RS];
#pragma unroll
      for (int u = 0; u < RS; ++u) {
        const int st = sb + 64 * u + lane;
        const long rec0 = ((long)q * nslices + (st < nslices ? st : 0)) * cap;
        const f32x4* src = (const f32x4*)(rec_s + rec0 * 8);
        v0[u][0] = src[0]; v0[u][1] = src[1];
        g00[u] = rec_g[rec0];
        cc[u] = st < nslices ? cnt[(long)q * nslices + st] : 0;
      }
#pragma unroll
      for (int u = 0; u < RS; ++u) {
        const int st = sb + 64 * u + lane;
        if (cc[u] > cap) ovf = true;
        const int nrec = min(cc[u], cap), r4 = 4 * (st & 3);
        if (nrec > 0) take(v0[u], g00[u], r4);
        if (nrec > 1) {
          const long rec0 = ((long)q * nslices + st) * cap;
          for (int j = 1; j < nrec; ++j) {
            const f32x4* sj = (const f32x4*)(rec_s + (rec0 + j) * 8);
            const f32x4 vj[2] = {sj[0], sj[1]};
            take(vj, rec_g[rec0 + j], r4);
          }
        }
      }
    }
    __syncthreads();
    n = total;
  }
  // 1. gather. Pass 1: lane <-> slice, list lengths and their exclusive prefix (soff). Pass 2: lane <-> ENTRY of the flattened
  // list (its slice by a binary search over soff): four independent loads per lane and round, so the whole gather is about one
  // global round trip (a first form walked entry j of every slice per round: one dependent round trip per entry, ~12 us)
  if (!RECORDS) {
    __shared__ int soff[SB_MAXSL + 1];
    for (int s0 = 0; s0 < nslices; s0 += 64) {
      const int s = s0 + lane;
      int c = s0 == 0 ? c_first : (s < nslices ? cnt[(long)q * nslices + s] : 0);
      // an overflowing list was re-cut by sim_block_scan to the rows strictly above its k-th class maximum (entries 1 ..); entry 0 holds
      // that level, judged against the cut below
      if (s < nslices) sovf[s] = c > cap;
      if (c > cap) { lists_over = true; if (c > 2 * cap) ovf = true; c = c > 2 * cap ? 0 : c - cap - 1; }   // the re-cut list (entries 1 ..), or nothing
      int incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
      if (s < nslices) soff[s] = n + incl - c;
      n += __builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) soff[nslices] = n;
    __syncthreads();
    const uint2* qc = cand + (long)q * nslices * cap;
    const int nn = min(n, SB_NC);
    for (int i0 = 0; i0 < nn; i0 += 256) {
      uint2 e[4]; int idx[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        idx[u] = i0 + 64 * u + lane;
        const int i = min(idx[u], nn - 1);
        int lo = 0, hi = nslices;                          // largest s with soff[s] <= i (empty slices repeat an offset: the search skips them)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (soff[mid] <= i) lo = mid; else hi = mid; }
        e[u] = qc[(long)lo * cap + (i - soff[lo]) + (sovf[lo] ? 1 : 0)];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (idx[u] < nn) { cs[idx[u]] = __uint_as_float(e[u].x); ci[idx[u]] = (int)e[u].y; }
    }
    __syncthreads();
  }
  n = __builtin_amdgcn_readfirstlane(n);
  if (__builtin_amdgcn_ballot_w64(ovf) != 0 || n > SB_NC) ovf = true; else ovf = false;
  __syncthreads();
  const float delta = SIM_DELTA * fmaxf(1.f, sqrtf(sl_s[0]));
  __syncthreads();
  // 2. T_lo <= T = k-th best MFMA score: counting binary search over the top 16 key bits (n <= k: every candidate is in)
  float T = -INFINITY;
  int m = 0;
  if (!ovf) {
    if (n > k) {
      // keys of the first 512 candidates in registers (8 per lane; typical n: a few hundred), the rest re-read from LDS; every
      // step of the search is compares + ballots + scalar bit counts (no cross-lane reduction, no LDS round trip)
      unsigned kr[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kr[j] = lane + 64 * j < n ? f2key(cs[lane + 64 * j]) >> 16 : 0u;
      unsigned lo = 0x007Fu, hi = 0x10000u;
#pragma unroll 1
      for (int it = 0; it < 16; ++it) {
        const unsigned mid = (lo + hi) >> 1;
        int c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(kr[j] >= mid));
        for (int i0 = 512; i0 < n; i0 += 64)
          c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(i0 + lane < n && (f2key(cs[min(i0 + lane, n - 1)]) >> 16) >= mid));
        if (c >= k) lo = mid; else hi = mid;
      }
      // T_lo = the smallest float whose key starts with the k-th best score's 16 bits (within 2^-7 relative below T): the short list
      // cut T_lo - delta admits a superset of what T - delta would; exactness is unaffected
      T = lo == 0x007Fu ? -INFINITY : key2f_floor(lo << 16);
    }
    // 3. short list: MFMA score >= T - delta (ballot compaction; order irrelevant: the ranking below is total)
    const float cut = T - delta;
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const bool pass = i < n && cs[i] >= cut && cs[i] > -INFINITY;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(pass);
      const int pos = m + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
      if (pass && pos < SB_SL) sl_i[pos] = ci[i];
      m += __builtin_popcountll(bal);
    }
    if (m > SB_SL) ovf = true;
    // slices whose lists overflowed: the rows left out of the re-cut list score at most the level in entry 0; they can hold a row of
    // the answer only if that level reaches the cut (every row of the exact answer has an MFMA score >= cut: the short list's own
    // criterion). Below it they are skipped - exact; at or above it the query takes the brute-force path as before.
    if (!RECORDS && __builtin_amdgcn_ballot_w64(lists_over) != 0) {
      for (int s0 = 0; s0 < nslices; s0 += 64) {
        const int s = s0 + lane;
        const bool bad = s < nslices && sovf[s] && !(__uint_as_float(cand[((long)q * nslices + s) * cap].x) < cut);
        if (__builtin_amdgcn_ballot_w64(bad) != 0) ovf = true;
      }
    }
  }
  __syncthreads();
  if (ovf) {
    if (lane == 0) { ovf_q[q] = 1; atomicOr(flags, 1); }
    if (no_fallback) {
      for (int j = lane; j < k; j += 64) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -2LL; }
      return;
    }
    brute_force_topk<TG, 64>(G, Ng, qs, cs, ci, k, g_offset, out_s + (long)q * k, out_i + (long)q * k);
    return;
  }
  if (lane == 0) ovf_q[q] = 0;
  // 4. exact re-scoring, 32 rows per round: the rows arrive by LDS-DMA (2 rows per wave-instruction, all in flight at once;
  // slot (lane & 31) of row j is fed from source chunk (lane & 31) ^ j), then lane j runs the chain over its row
  const unsigned ldsR = __builtin_amdgcn_readfirstlane((unsigned)(size_t)((__attribute__((address_space(3))) char*)rows));
  for (int base = 0; base < m; base += 32) {
    const int nr = min(32, m - base);
#pragma unroll 1
    for (int i = 0; 2 * i < nr; ++i) {
      const int jj = 2 * i + (lane >> 5);
      const long idx = sl_i[base + min(jj, nr - 1)];
      glds16(G + idx * 256 + (((lane & 31) ^ jj) << 3), __builtin_amdgcn_readfirstlane(ldsR + 1024 * i));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (lane < nr) sl_s[base + lane] = chain_score_lds<TG>(rows + lane * 512, lane, qs);
    __syncthreads();
  }
  // 5. rank by (chain score desc, index asc); entries beyond the short list (Ng < k) are (-inf, -1)
  if (lane < m) {
    const float s = sl_s[lane]; const int idx = sl_i[lane];
    int rank = 0;
    for (int i = 0; i < m; ++i) rank += (sl_s[i] > s || (sl_s[i] == s && sl_i[i] < idx)) ? 1 : 0;
    if (rank < k) { out_s[(long)q * k + rank] = s; out_i[(long)q * k + rank] = (long long)idx + g_offset; }
  }
  for (int j = m + lane; j < k; j += 64) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -1LL; }
}


// plan of the threshold-and-append pipeline (host; shared by the launcher and cor_topk_workspace_bytes)
struct V3Plan {
  int qb, nqg;                       // query blocks per wave (1 | 2), query groups of 256 * qb
  int tiles, nsplit, tiles_per_split, nstreams, cap;                 // APPEND pass
  int s_stride, s_tiles, s_nsplit, s_tiles_per_split, ngroups;       // SAMPLE pass (ngroups == 0: no sample, tau = -inf)
  size_t off_img, off_sg, off_dq, off_tau, off_flags, off_ovf, off_cnt, off_recs, off_recg, off_lists, bytes;
};
inline V3Plan make_v3(int Bq, int Ng, int k) {
  V3Plan p{};
  p.qb = Bq > 256 ? 2 : 1;
  p.nqg = cdiv(Bq, 256 * p.qb);
  p.tiles = cdiv(Ng, 64);                              // 64-row super-tiles
  int want = device_cus() / p.nqg;                     // one resident block per CU
  if (want > 256) want = 256;                          // nstreams <= 1024
  if (want > p.tiles) want = p.tiles;
  if (want < 1) want = 1;
  p.tiles_per_split = cdiv(p.tiles, want);
  p.nsplit = cdiv(p.tiles, p.tiles_per_split);
  p.nstreams = 4 * p.nsplit;                           // (query, slice, lane quarter)
  long expect;                                         // expected accepted scores per query over the whole shard
  if (Ng <= 4096) {                                    // tiny shard: no sample pass, every row is a candidate (<= FS_MAX)
    p.ngroups = 0; p.s_tiles = 0; p.s_stride = 1; p.s_nsplit = 0; p.s_tiles_per_split = 0;
    p.cap = 2 * p.tiles_per_split;                     // records (32-row tiles) per (slice, lane quarter) stream: every tile is one
  } else {
    // every 16th super-tile, at least ~128 of them: the sample pass costs 1/stride of the full scan plus a fixed ~8 us; the
    // candidates it admits (~2 k stride per query) must stay rare per wave and tile (the append path is divergent)
    p.s_stride = p.tiles / 16 >= 128 ? 16 : (p.tiles / 128 > 1 ? p.tiles / 128 : 1);
    p.s_tiles = cdiv(p.tiles, p.s_stride);
    int sw = device_cus() / p.nqg;
    if (sw > 256) sw = 256;
    if (sw > p.s_tiles) sw = p.s_tiles;
    if (sw < 1) sw = 1;
    p.s_tiles_per_split = cdiv(p.s_tiles, sw);
    p.s_nsplit = cdiv(p.s_tiles, p.s_tiles_per_split);
    p.ngroups = 4 * p.s_nsplit;
    expect = 3L * k * p.s_stride;                      // ~ k * Ng / sample rows, x3 for group-maximum slack
    // k > 16: tau is the k-th largest of only 32 super-group maxima - near k = 32 their MINIMUM, which admits ~4x the candidates of the
    // tighter bound the factor 3 was sized for: without this most searches overflow some stream and fall back (exact, slow)
    if (k > 16) expect *= 4;
    // records per stream: Poisson with mean ~ expect / nstreams (< 1 on large shards); +10 keeps P(overflow) per search < 1e-4
    p.cap = (int)(2 * expect / p.nstreams) + 10;
  }
  const TopkPlan2 p2 = make_plan2(Bq, Ng, k, device_cus());
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 255) & ~(size_t)255; return at; };
  p.off_img = take((size_t)p.nqg * 8 * p.qb * 16 * 64 * 16);        // whole query blocks of every group (rows past Bq: copies)
  p.off_sg = take((size_t)32 * p.nqg * 256 * p.qb * 4);               // 32 super-group maxima per query slot (whole query blocks)
  p.off_dq = take((size_t)Bq * 4);
  p.off_tau = take((size_t)Bq * 4);
  p.off_flags = take(16);
  p.off_ovf = take((size_t)Bq * 4);
  p.off_cnt = take((size_t)Bq * p.nstreams * 4);
  p.off_recs = take((size_t)Bq * p.nstreams * p.cap * 32);            // a record = 8 scores
  p.off_recg = take((size_t)Bq * p.nstreams * p.cap * 4);
  p.off_lists = take((size_t)Bq * p2.nparts * p2.kmax * 8);          // fallback list kernels
  p.bytes = o;
  return p;
}

int launch_merge(const float* ws_s, const int* ws_i, int Bq, int n, int k, long long g_offset, float* out_s, long long* out_i,
                 const int* gate_q, hipStream_t s) {
  static DevOnce once;
  cor_max_dyn_lds((const void*)sim_topk_merge, 8192 * 8, once);
  hipLaunchKernelGGL(sim_topk_merge, dim3(Bq), dim3(256), (size_t)n * 8, s, ws_s, ws_i, n, k, g_offset, out_s, out_i, gate_q);
  COR_CHECK_LAUNCH();
  return 0;
}

template <typename TG>
int launch_lists_v2(const float* Q, const TG* G, int Bq, int Ng, int k, long long g_offset, float* out_s, long long* out_i, float* ws_s,
                    const int* gate, const int* gate_q, hipStream_t s) {
  const TopkPlan2 p = make_plan2(Bq, Ng, k, device_cus());
  int* ws_i = (int*)(ws_s + (long)Bq * p.nparts * p.kmax);
  const dim3 grid(p.nqg * p.nsplit), block(256);
  const size_t lds = 2 * 32 * 256 * 2;
#define SIM_V2(KM) hipLaunchKernelGGL((sim_topk_v2<TG, KM>), grid, block, lds, s, Q, G, Bq, Ng, p, ws_s, ws_i, gate)
  if (p.kmax == 8) SIM_V2(8); else if (p.kmax == 16) SIM_V2(16); else SIM_V2(32);
#undef SIM_V2
  COR_CHECK_LAUNCH();
  return launch_merge(ws_s, ws_i, Bq, p.nparts * p.kmax, k, g_offset, out_s, out_i, gate_q, s);
}

template <typename TG, int QB>
int launch_v3(const float* Q, const TG* G, int Bq, int Ng, int k, long long g_offset, float* out_s, long long* out_i, char* w,
              const V3Plan& p, int flags, hipStream_t s) {
  constexpr size_t lds = (size_t)SCAN_NS * 64 * 256 * 2;
  static DevOnce once_s, once_a, once_f;
  cor_max_dyn_lds((const void*)sim_scan<TG, QB, true>, (int)lds, once_s);
  cor_max_dyn_lds((const void*)sim_scan<TG, QB, false>, (int)lds, once_a);
  constexpr size_t fs_lds = (size_t)FS_MAX * 8 + SL_MAX * 8 + 256 * 4 + 256 * 4;
  cor_max_dyn_lds((const void*)sim_final<TG>, (int)fs_lds, once_f);
  unsigned* sg = (unsigned*)(w + p.off_sg); float* dq = (float*)(w + p.off_dq); float* tau = (float*)(w + p.off_tau);
  const int Bqp = p.nqg * 256 * QB;
  int* dflags = (int*)(w + p.off_flags); int* ovf_q = (int*)(w + p.off_ovf); int* cnt = (int*)(w + p.off_cnt);
  float* rec_s = (float*)(w + p.off_recs); int* rec_g = (int*)(w + p.off_recg);
  uint4* qimg = (uint4*)(w + p.off_img);
  // 0. queries -> gallery dtype, fragment-major; clears the per-call overflow flags. (Folding this conversion into the SAMPLE pass -
  // every wave converting its own 64 fp32 rows, the blocks of slice 0 publishing the image - was built and measured in round 4: the
  // SAMPLE pass grew from 8-10 to 21.6 us at 125k rows and from 22.7 to 37 us at 1M, against the 5.6-us launch it replaced: reverted. A
  // second form - COALESCED 1-KiB row loads, transposed into fragments through the wave's 16 KiB of the idle gallery ring - costs the
  // SAMPLE pass +4.5 us (every block still pulls 512 KiB of fp32 rows through its CU's L2 port against 256 KiB of the image) and saves
  // the 5-us launch + its boundary: NO difference in a same-box A/B (three alternating rounds: 512 x 125k 84.6-88.4 vs 86.7-87.9 us,
  // 512 x 1M 319-321 vs 316-327, 256 x 100k 56.3-56.9 vs 55.6-56.1). The launch stays: it is the simpler code.)
  hipLaunchKernelGGL((sim_prep<TG>), dim3(p.nqg * 8 * QB), dim3(256), 0, s, Q, Bq, qimg, dflags, ovf_q, sg, Bqp, dq);
  COR_CHECK_LAUNCH();
  ScanArgs a{};
  a.Bq = Bq; a.Ng = Ng; a.nqg = p.nqg; a.qimg = qimg; a.sg = sg; a.Bqp = Bqp;
  if (p.ngroups > 0) {                                  // A. group maxima of the strided sample
    a.nsplit = p.s_nsplit; a.tiles_per_split = p.s_tiles_per_split; a.ntiles = p.s_tiles; a.tile_stride = p.s_stride;
    hipLaunchKernelGGL((sim_scan<TG, QB, true>), dim3(p.nqg * p.s_nsplit), dim3(512), lds, s, G, a);
    COR_CHECK_LAUNCH();
  }
  // B. (round 4: no sim_tau launch - the APPEND pass ranks the 32 super-group maxima in its prologue; no sample pass: all empty, tau = -inf)
  // C. full scan
  a.nsplit = p.nsplit; a.tiles_per_split = p.tiles_per_split; a.ntiles = p.tiles; a.tile_stride = 1;
  a.dq = dq; a.k = k;
  a.tau = tau; a.cnt = cnt; a.rec_s = rec_s; a.rec_g = rec_g; a.cap = p.cap; a.tau_add = (flags & 4) ? 1e30f : 0.f;
#ifdef COR_PROBES
  a.stamps = (flags & 32) ? (unsigned long long*)(w + cor_topk_workspace_bytes(Bq, Ng, k)) : nullptr;   // tools/sim_stamps.py: 2 MiB behind the workspace
  a.probe_same = ((flags & 64) ? 1 : 0) | ((flags & 128) ? 2 : 0) | ((flags & 256) ? 4 : 0);
#endif
  hipLaunchKernelGGL((sim_scan<TG, QB, false>), dim3(p.nqg * p.nsplit), dim3(512), lds, s, G, a);
  COR_CHECK_LAUNCH();
  // D. exact selection: one 256-thread block per query. (COR_TOPK_WAVE_FINAL: the one-wave-per-query kernel of the small-shard path fed
  // from the records - measured 52-59 us against 25 here: 512 streams are eight dependent gather rounds for one wave. A/B partner only.)
  if (flags & COR_TOPK_WAVE_FINAL)
    hipLaunchKernelGGL((sim_final_wave<TG, true>), dim3(Bq), dim3(64), 0, s, Q, G, cnt, nullptr, rec_s, rec_g, tau, p.nstreams, p.cap, Ng, k, g_offset,
                       out_s, out_i, dflags, ovf_q, (flags & COR_TOPK_NO_FALLBACK) ? 1 : 0);
  else
    hipLaunchKernelGGL((sim_final<TG>), dim3(Bq), dim3(256), fs_lds, s, Q, G, rec_s, rec_g, tau, cnt, p.nstreams, p.cap, Ng, k, g_offset, out_s, out_i,
                       dflags, ovf_q, (flags & COR_TOPK_NO_FALLBACK) ? 1 : 0);
  COR_CHECK_LAUNCH();
  return 0;                                             // (an overflowed query was ranked exactly inside sim_final: no second launch)
}

template <typename TG, int QB, int T>
int launch_small_t(const float* Q, const TG* G, int Bq, int Ng, int k, long long g_offset, float* out_s, long long* out_i, char* w,
                   const SmallPlan& p, int flags, hipStream_t s) {
  constexpr size_t lds = (size_t)QB * 16 * 64 * 16 + 8 * 16384;
  static DevOnce once;
  cor_max_dyn_lds((const void*)sim_block_scan<TG, QB, T>, (int)lds, once);
  int* dflags = (int*)(w + p.off_flags); int* ovf_q = (int*)(w + p.off_ovf); int* cnt = (int*)(w + p.off_cnt);
  uint2* cand = (uint2*)(w + p.off_cand);
#ifdef COR_PROBES
  unsigned long long* stamps = (flags & 32) ? (unsigned long long*)(w + cor_topk_workspace_bytes(Bq, Ng, k)) : nullptr;   // tools/sim_stamps.py: 2 MiB behind the workspace
#else
  unsigned long long* stamps = nullptr;
#endif
  hipLaunchKernelGGL((sim_block_scan<TG, QB, T>), dim3(p.grid), dim3(512), lds, s, Q, G, Bq, Ng, k, p.nqg, p.nslices, p.xcd_map, p.cap, cnt, cand, dflags, stamps);
  COR_CHECK_LAUNCH();
  hipLaunchKernelGGL((sim_final_wave<TG, false>), dim3(Bq), dim3(64), 0, s, Q, G, cnt, cand, nullptr, nullptr, nullptr, p.nslices, p.cap, Ng, k, g_offset,
                     out_s, out_i, dflags, ovf_q, (flags & COR_TOPK_NO_FALLBACK) ? 1 : 0);
  COR_CHECK_LAUNCH();
  return 0;
}
template <typename TG>
int launch_small(const float* Q, const TG* G, int Bq, int Ng, int k, long long g_offset, float* out_s, long long* out_i, char* w,
                 const SmallPlan& p, int flags, hipStream_t s) {
#define SB_GO(QB_, T_) return launch_small_t<TG, QB_, T_>(Q, G, Bq, Ng, k, g_offset, out_s, out_i, w, p, flags, s)
  if (p.qb == 1) { if (p.T == 1) SB_GO(1, 1); if (p.T == 2) SB_GO(1, 2); SB_GO(1, 4); }
  if (p.T == 1) SB_GO(2, 1);
  SB_GO(2, 2);
#undef SB_GO
}

// ---------------------------------------------------------------------------------------------------------------------
// WIDE k (33 <= k <= COR_TOPK_KMAX = 256): Recall@50/100 and two-stage re-ranking. The k <= 32 kernels above keep sorted lists in
// registers (KMAX <= 32) and bound the k-th best score by 32 super-group maxima; neither scales to k = 256. This route keeps the
// threshold-and-append shape with more groups and a block-wide selection:
//   scan: 16-bit galleries with C = 256 run sim_prep + sim_scan<.., WIDE> (the production scan; SAMPLE stores >= 2k group maxima per
//     query instead of folding them into 32); fp32 galleries and 16-bit ones with C != 256 run sim_wide_scan, the tile loop of
//     sim_topk_partial with a SAMPLE and an APPEND epilogue ((score, row) entries instead of register lists).
//   sim_tau_wide: tau_q = k-th largest group maximum - delta_q (block radix select over the group keys; delta_q = 0 for fp32, whose
//     MFMA scores ARE the chain; fewer than k groups: -inf, every row is a candidate).
//   sim_final_wide: per query, the candidates >= tau_q are compacted into LDS, the EXACT k-th best scan score T is found by a 4-pass radix
//     select, the short list {score >= T - delta_q} is re-scored with the chain of oracle/c/sim_chain.c over C / 8 chunks (16-bit only)
//     and ranked by one bitonic sort of 64-bit keys (inverted order-preserving score bits, index). Exactness: the argument of v3 above,
//     for any C <= 256 (C - 1 roundings per score either way).
// Overflow (a stream list, the candidate buffer or the short list) is detected and repaired in the same block: an exact radix select
// over the chain scores of the whole shard (wide_brute_force). Every wide call is bitwise the chain oracle, whatever the dtype and C.
constexpr int FSW = 8192;                              // candidates per query in LDS (64 KiB)
constexpr int SLW = 2048;                              // short list (>= 2 k_max, room for ties within delta)
constexpr size_t FINAL_WIDE_LDS = (size_t)FSW * 8 + SLW * 8 + 256 * 4 + 256 * 4;

// k-th largest (1-based, 1 <= k <= n) of the order-preserving keys key_at(i), i < n: a 4-pass radix select, 8 bits per pass, over the
// NT = 256 threads of the block (wave 0 scans the histogram as sim_final does). *k_rem ends as the k-th key's rank among the keys EQUAL
// to it (k - *k_rem keys are larger). key_at may be expensive (the brute-force path re-scores a row per call): it runs 4 n times.
template <typename F>
__device__ unsigned block_kth_key(F key_at, int n, int k, int* hist, int* sel_bin, int* k_rem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned prefix = 0;
  if (tid == 0) *k_rem = k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const unsigned key = key_at(i);
      if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1);
    }
    __syncthreads();
    if (wave == 0) {                                   // bins 4*lane .. 4*lane+3; suffix sums from the top bin down
      const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const int mine = h0 + h1 + h2 + h3;
      int above = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(above, o, 64); if (lane + o < 64) above += t; }
      above -= mine;
      const int kr = *k_rem;
      if (above < kr && kr <= above + mine) {          // exactly one lane
        int a3 = above, b = 3;
        if (kr <= a3 + h3) b = 3; else { a3 += h3; if (kr <= a3 + h2) b = 2; else { a3 += h2; if (kr <= a3 + h1) b = 1; else { a3 += h1; b = 0; } } }
        *sel_bin = 4 * lane + b; *k_rem = kr - a3;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | (unsigned)*sel_bin;
    __syncthreads();
  }
  return prefix;
}

// ascending bitonic sort of n (a power of two, <= 256 * 64) 64-bit keys in LDS by the block's 256 threads
__device__ void block_sort_u64(unsigned long long* key, int n) {
  for (int kk = 2; kk <= n; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long x = key[i], y = key[l];
          if ((x > y) == ((i & kk) == 0)) { key[i] = y; key[l] = x; }
        }
      }
      __syncthreads();
    }
}
// (score desc, index asc) as one ascending 64-bit key, and back
__device__ __forceinline__ unsigned long long rank_key(float s, int idx) { return ((unsigned long long)~f2key(s) << 32) | (unsigned)idx; }
__device__ __forceinline__ float rank_key_score(unsigned long long key) { return key2f_floor(~(unsigned)(key >> 32)); }

// chain score of gallery row idx (C values, C % 16 == 0) against qs: the order of oracle/c/sim_chain.c for any C (chunks of 8:
// k = 8c+i then 8c+4+i); fp32 rows as stored, 16-bit rows widened exactly
template <typename TG>
__device__ __forceinline__ float chain_score_c(const TG* __restrict__ G, long idx, int C, const float* qs) {
  float acc = 0.f;
  if constexpr (sizeof(TG) == 4) {
    const f32x4* row = (const f32x4*)(G + idx * C);
#pragma unroll 4
    for (int c = 0; c < C / 8; ++c) {
      const f32x4 a = row[2 * c], b = row[2 * c + 1];
#pragma unroll
      for (int i = 0; i < 4; ++i) { acc = fmaf(a[i], qs[8 * c + i], acc); acc = fmaf(b[i], qs[8 * c + 4 + i], acc); }
    }
  } else {
    const uint4* row = (const uint4*)(G + idx * C);
#pragma unroll 4
    for (int c = 0; c < C / 8; ++c) {
      const uint4 v = row[c];
      float g[8];
      if (__is_same(TG, bf16_t)) {
        g[0] = __uint_as_float(v.x << 16); g[1] = __uint_as_float(v.x & 0xffff0000u); g[2] = __uint_as_float(v.y << 16); g[3] = __uint_as_float(v.y & 0xffff0000u);
        g[4] = __uint_as_float(v.z << 16); g[5] = __uint_as_float(v.z & 0xffff0000u); g[6] = __uint_as_float(v.w << 16); g[7] = __uint_as_float(v.w & 0xffff0000u);
      } else {
        const f16x8 hv = __builtin_bit_cast(f16x8, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = (float)hv[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) { acc = fmaf(g[i], qs[8 * c + i], acc); acc = fmaf(g[4 + i], qs[8 * c + 4 + i], acc); }
    }
  }
  return acc;
}

// Exact top-k of ONE query over the whole shard (block of 256 threads), for overflowed queries: the k-th largest chain-score key by
// block_kth_key (four passes, every row re-scored per pass), then one more pass collects the rows above it (fewer than k, any order)
// and the first k_rem rows EQUAL to it in index order (a block-wide prefix count per 256 rows), and a bitonic sort ranks them.
// Five chain passes over the shard: slow, exact, rare (DESIGN 3.4 gives the measured cost).
// FILTER: only the rows allowed for the query (label ql, COR_FILTER_NE if ne) are ranked: a disallowed row has key 0, below every score's
// key, and a query with nA <= k allowed rows gets all of them followed by the (-inf, -1) tail.
// The body takes the score of a row and the allow predicate as callables (brute_force_by): the chain over a float / 16-bit gallery here,
// the integer score of the int8 route in sim_i8_repair.
template <bool FILTER, typename ScoreAt, typename Allowed>
__device__ __forceinline__ void brute_force_by(const ScoreAt score_at, const Allowed allowed, int Ng, int k, long long g_offset, float* sl_s,
                                               int* sl_i, unsigned long long* keys, int* hist, float* out_s, long long* out_i) {
  __shared__ int sel_bin, k_rem, n_above, wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nA = Ng;                                         // rows that may be ranked (block-uniform)
  if constexpr (FILTER) {
    __shared__ int n_allowed;
    if (tid == 0) n_allowed = 0;
    __syncthreads();
    int mine = 0;
    for (int g = tid; g < Ng; g += 256) mine += allowed(g) ? 1 : 0;
    atomicAdd(&n_allowed, mine);
    __syncthreads();
    nA = n_allowed;
  }
  const int kk = min(k, nA);
  auto key_at = [&](int g) { return allowed(g) ? f2key(score_at(g)) : 0u; };
  unsigned kth = 0u;                                   // nA <= k: every allowed row is above "key 0"
  int above = kk, need = 0;
  if (nA > k) { kth = block_kth_key(key_at, Ng, k, hist, &sel_bin, &k_rem); need = k_rem; above = k - need; }
  if (tid == 0) n_above = 0;
  __syncthreads();
  int taken = 0;                                       // rows equal to kth already collected (block-uniform)
  for (int g0 = 0; g0 < Ng; g0 += 256) {
    const int g = g0 + tid;
    float s = -INFINITY; unsigned key = 0u;
    if (g < Ng && allowed(g)) { s = score_at(g); key = f2key(s); }
    const bool up = g < Ng && key > kth, tie = g < Ng && key == kth && nA > k;
    if (up) { const int p = atomicAdd(&n_above, 1); sl_s[p] = s; sl_i[p] = g; }
    const unsigned long long b = __builtin_amdgcn_ballot_w64(tie);
    if (lane == 0) wcnt[wave] = __builtin_popcountll(b);
    __syncthreads();
    int before = taken, tot = 0;
    for (int w = 0; w < 4; ++w) { before += w < wave ? wcnt[w] : 0; tot += wcnt[w]; }
    if (tie) {
      const int pos = before + __builtin_popcountll(b & ((1ull << lane) - 1ull));
      if (pos < need) { sl_s[above + pos] = s; sl_i[above + pos] = g; }
    }
    taken += tot;
    __syncthreads();
  }
  int P = 1;
  while (P < kk) P <<= 1;
  for (int j = tid; j < P; j += 256) keys[j] = j < kk ? rank_key(sl_s[j], sl_i[j]) : ~0ull;
  __syncthreads();
  block_sort_u64(keys, P);
  for (int j = tid; j < k; j += 256) {
    out_s[j] = j < kk ? rank_key_score(keys[j]) : -INFINITY;
    out_i[j] = j < kk ? (long long)(unsigned)keys[j] + g_offset : -1LL;
  }
}
template <typename TG, bool FILTER = false>
__device__ void wide_brute_force(const TG* __restrict__ G, int Ng, int C, const float* qs, int k, long long g_offset, float* sl_s, int* sl_i,
                                 unsigned long long* keys, int* hist, float* out_s, long long* out_i, const int* rlab = nullptr, int ql = -1,
                                 int ne = 0) {
  brute_force_by<FILTER>([&](int g) { return chain_score_c<TG>(G, g, C, qs); },
                         [&](int g) { return !FILTER || row_allowed(rlab, g, ql, ne); }, Ng, k, g_offset, sl_s, sl_i, keys, hist,
                         out_s, out_i);
}
// The fallback of cor_similarity_range for one query: a chain pass over the shard counts the rows at or above the floor, wide_brute_force
// ranks into LDS (tmp_s / tmp_i [k], outside the buffers it works in), and the ranked rows below the floor leave as tail. Six chain passes.
// FILTER (cor_similarity_range_filtered): only the rows allowed for the query (label ql, COR_FILTER_NE if ne) are counted and ranked.
template <typename TG, bool FILTER = false>
__device__ void range_brute_force(const TG* __restrict__ G, int Ng, int C, const float* qs, int k, long long g_offset, float thr, float* sl_s,
                                  int* sl_i, unsigned long long* keys, int* hist, float* tmp_s, long long* tmp_i, float* out_s, long long* out_i,
                                  int* out_count, const int* rlab = nullptr, int ql = -1, int ne = 0) {
  __shared__ int members;
  const int tid = threadIdx.x;
  if (tid == 0) members = 0;
  __syncthreads();
  int mine = 0;
  if constexpr (FILTER) {
    for (int g = tid; g < Ng; g += 256) mine += row_allowed(rlab, g, ql, ne) && chain_score_c<TG>(G, g, C, qs) >= thr ? 1 : 0;
  } else {
    for (int g = tid; g < Ng; g += 256) mine += chain_score_c<TG>(G, g, C, qs) >= thr ? 1 : 0;
  }
  if (mine) atomicAdd(&members, mine);
  if constexpr (FILTER) wide_brute_force<TG, true>(G, Ng, C, qs, k, g_offset, sl_s, sl_i, keys, hist, tmp_s, tmp_i, rlab, ql, ne);
  else wide_brute_force<TG>(G, Ng, C, qs, k, g_offset, sl_s, sl_i, keys, hist, tmp_s, tmp_i);
  __syncthreads();
  for (int j = tid; j < k; j += 256) {
    const bool in = j < Ng && tmp_s[j] >= thr;         // (the first min(k, Ng, allowed rows) slots hold rows; the others are (-inf, -1) already)
    out_s[j] = in ? tmp_s[j] : -INFINITY;
    out_i[j] = in ? tmp_i[j] : -1LL;
  }
  if (tid == 0) *out_count = members;
}

// The tile loop of sim_topk_partial (fp32 galleries: the chain on the f32 MFMA; 16-bit: the 16-bit MFMA; any C <= 256, C % 16 == 0)
// with the epilogues of the wide route. One wave = 32 queries x a slice of 32-row tiles; lane (r, h) holds 16 scores of query r per tile.
//   SAMPLE: tiles t * tile_stride of the slice; the group (slice, lane half h) keeps its maximum: sg[q * ngroups + split * 2 + h].
//   APPEND: every tile of the slice; scores >= tau_q go to the private list of stream (q, slice, h) as (score bits, row) entries.
//   FILTER: disallowed scores are -inf (never a group's best, never >= tau_q), slice `split` walks the tiles split, split + nsplit, ... and
//   SAMPLE keeps the group's four best allowed scores (Best4), sg[q * ngroups + (split * 2 + h) * 4 + j] (ngroups counts the four).
struct WideScanArgs {
  int Bq, Ng, C, nqt, nsplit, tiles_per_split, ntiles, tile_stride;
  unsigned* sg; int ngroups;
  const float* tau; int* cnt; uint2* lst; int cap;
  const int* rlab; const int* qlab; int ne;          // FILTER: row / query labels, COR_FILTER_NE
  int* sgrow;                                        // GROUP SAMPLE: the shard row behind every stored sample value
  const float* rng_a; const float* rng_h; int* sure; // RANGE APPEND: A_q and H_q (sim_range_bounds; tau holds B_q), the sure counts per stream
};
//   GROUP (distinct-group route, SAMPLE only): NV = 1 (4 with FILTER) best allowed scores per group WITH their rows (BestRows, a.sgrow).
//   RANGE (cor_similarity_range, APPEND only): tau holds B_q = thr_q - delta_q; behind one test of the tile maximum against it a lane counts
//   its scores >= H_q (sure members, a register counter) and appends the list candidates (>= A_q) and the band rows (B_q <= s < H_q).
template <typename TG, bool SAMPLE, bool FILTER = false, bool GROUP = false, bool RANGE = false>
__global__ void __launch_bounds__(256) sim_wide_scan(const float* __restrict__ Q, const TG* __restrict__ G, const WideScanArgs a) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= a.nqt * a.nsplit) return;
  const int qt = wid % a.nqt, split = wid / a.nqt;
  const int q = qt * 32 + r, Ng = a.Ng, C = a.C;
  const float* qrow = Q + (long)min(q, a.Bq - 1) * C;

  constexpr bool F32 = sizeof(TG) == 4;
  constexpr int CH = F32 ? 8 : 16;
  constexpr int NCH = 256 / CH;
  const int nch = C / CH;
  uint4 qf[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c < nch) {
      if constexpr (F32) qf[c] = *(const uint4*)(qrow + c * 8 + 4 * h);
      else qf[c] = q_frag16<TG>(qrow, c, h);
    }
  }
  const float tq = SAMPLE ? 0.f : append_threshold(q < a.Bq, a.tau, q);
  const int stream = split * 2 + h, nstreams = 2 * a.nsplit;
  float gmax = -INFINITY;
  int n = 0, nsure = 0;
  const float ra = RANGE ? a.rng_a[min(q, a.Bq - 1)] : 0.f, rh = RANGE ? a.rng_h[min(q, a.Bq - 1)] : 0.f;
  const int ql = FILTER ? a.qlab[min(q, a.Bq - 1)] : 0;
  Best4 top4;
  top4.clear();
  constexpr int NV = GROUP && FILTER ? 4 : 1;
  BestRows<NV> best;
  if constexpr (GROUP) best.clear();
  const SliceWalk<FILTER> walk(split, a.nsplit, a.tiles_per_split, a.ntiles);
  for (int t = walk.t0; t < walk.t1; ++t) {
    const int g0 = walk.tile(t) * a.tile_stride * 32;
    const char* grow = (const char*)(G + (long)min(g0 + r, Ng - 1) * C) + 16 * h;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c < nch) {
        const uint4 av = *(const uint4*)(grow + c * 32);
        if (F32) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(av.x), __uint_as_float(qf[c].x), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(av.y), __uint_as_float(qf[c].y), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(av.z), __uint_as_float(qf[c].z), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(av.w), __uint_as_float(qf[c].w), acc, 0, 0, 0);
        } else if (__is_same(TG, bf16_t)) {
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, qf[c]), acc, 0, 0, 0);
        } else {
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, qf[c]), acc, 0, 0, 0);
        }
      }
    }
    float sc[16], tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      sc[e] = g0 + (e & 3) + 8 * (e >> 2) + 4 * h < Ng ? acc[e] : -INFINITY;
      tmax = fmaxf(tmax, sc[e]);
    }
    if constexpr (FILTER) {                            // labels of rows g0 + 8 j + 4 h + i (score e = 4 j + i). load4_or_zero and label_allows,
                                                       // spelled out: the shared forms cost the FILTER instantiations four more VGPRs
      tmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = g0 + 8 * j + 4 * h;
        int4 l;
        if constexpr (RANGE) {                         // branch-free (a row past the shard is -inf already, whatever label it reads): the two-way
          l.x = a.rlab[min(row, Ng - 1)]; l.y = a.rlab[min(row + 1, Ng - 1)];      // load held exec masks in SGPRs the fp32 RANGE form lacks
          l.z = a.rlab[min(row + 2, Ng - 1)]; l.w = a.rlab[min(row + 3, Ng - 1)];
        } else if (row + 4 <= Ng) l = *(const int4*)(a.rlab + row);
        else { l.x = row < Ng ? a.rlab[row] : 0; l.y = row + 1 < Ng ? a.rlab[row + 1] : 0; l.z = row + 2 < Ng ? a.rlab[row + 2] : 0; l.w = 0; }
        const int lv[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (!(ql < 0 || ((lv[i] == ql) != (a.ne != 0)))) sc[4 * j + i] = -INFINITY;
          tmax = fmaxf(tmax, sc[4 * j + i]);
        }
      }
    }
    if constexpr (SAMPLE && GROUP) {
      if (__builtin_amdgcn_ballot_w64(tmax > best.v[NV - 1]) != 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) best.offer(sc[e], g0 + (e & 3) + 8 * (e >> 2) + 4 * h);
      }
    } else if (SAMPLE && FILTER) {
#pragma unroll
      for (int e = 0; e < 16; ++e) top4.offer(sc[e]);
    } else if (SAMPLE) {
      gmax = fmaxf(gmax, tmax);
    } else if (__builtin_amdgcn_ballot_w64(tmax >= tq) != 0) {
      uint2* dst = a.lst + ((long)q * nstreams + stream) * a.cap;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if constexpr (RANGE) {                         // tq = B_q (a padding lane: +inf, nothing passes)
          if (sc[e] >= tq) {
            nsure += sc[e] >= rh ? 1 : 0;
            if (sc[e] >= ra || sc[e] < rh) append_entry(dst, n, a.cap, sc[e], g0 + (e & 3) + 8 * (e >> 2) + 4 * h);
          }
        } else if (sc[e] >= tq) append_entry(dst, n, a.cap, sc[e], g0 + (e & 3) + 8 * (e >> 2) + 4 * h);
      }
    }
  }
  if (q < a.Bq) {
    if constexpr (SAMPLE && GROUP) best.store(a.sg, a.sgrow, (long)q * a.ngroups + stream * NV);
    else if (SAMPLE && FILTER) top4.store(a.sg + (long)q * a.ngroups + stream * 4);
    else if (SAMPLE) a.sg[(long)q * a.ngroups + stream] = f2key(gmax);
    else {
      a.cnt[(long)q * nstreams + stream] = n;
      if constexpr (RANGE) a.sure[(long)q * nstreams + stream] = nsure;
    }
  }
}

// tau_q for the wide route: one block per query ranks its ngroups group-maximum keys (sg[q * ngroups + g]; 0 or key(-inf) = a group
// without a finite score). delta_q bounds |scan score - chain score| for 16-bit galleries (sim_prep's form, any C <= 256); fp32: 0.
template <typename TG>
__global__ void __launch_bounds__(256) sim_tau_wide(const float* __restrict__ Q, int C, const unsigned* __restrict__ sg, int ngroups, int k,
                                                    float* tau) {
  __shared__ int hist[256], sel_bin, k_rem;
  __shared__ float part[4];
  const int q = blockIdx.x, tid = threadIdx.x;
  float n2 = 0.f;
  if (sizeof(TG) != 4 && tid < C) { const float x = round_to<TG>(Q[(long)q * C + tid]); n2 = x * x; }
  n2 = wave_sum(n2);
  if ((tid & 63) == 0) part[tid >> 6] = n2;
  __syncthreads();
  const float delta = sizeof(TG) == 4 ? 0.f : SIM_DELTA * fmaxf(1.f, sqrtf(part[0] + part[1] + part[2] + part[3]));
  float t = -INFINITY;                                 // fewer than k groups: every row is a candidate
  if (ngroups >= k) {
    const unsigned* g = sg + (long)q * ngroups;
    const unsigned kth = block_kth_key([&](int i) { return g[i]; }, ngroups, k, hist, &sel_bin, &k_rem);
    if (kth > f2key(-INFINITY)) t = key2f_floor(kth) - delta;
  }
  if (tid == 0) tau[q] = t;
}

// Exact selection of the wide route, one block of 256 threads per query. RECORDS: the 8-score records of sim_scan<APPEND> (rec_s /
// rec_g, the scores >= tau_q are kept); otherwise the (score, row) entry lists of sim_wide_scan<APPEND> (lst). fp32 galleries: the scan
// scores are the chain, nothing is re-scored and delta = 0. FILTER: the scans stored allowed scores only (masked record slots are -inf and
// skipped); an overflowed query's brute force ranks its allowed rows (row labels rlab, query labels qlab, ne = COR_FILTER_NE).
template <typename TG, bool RECORDS, bool FILTER = false>
__global__ void __launch_bounds__(256) sim_final_wide(const float* __restrict__ Q, const TG* __restrict__ G, int Ng, int C, int k, long long g_offset,
                                                      const float* __restrict__ tau, const int* __restrict__ cnt, int nstreams, int cap,
                                                      const float* __restrict__ rec_s, const int* __restrict__ rec_g, const uint2* __restrict__ lst,
                                                      float* out_s, long long* out_i, int no_fallback, const int* __restrict__ rlab,
                                                      const int* __restrict__ qlab, int ne) {
  extern __shared__ __attribute__((aligned(16))) char fwraw[];
  float* cs = (float*)fwraw; int* ci = (int*)(cs + FSW);
  float* sl_s = (float*)(ci + FSW); int* sl_i = (int*)(sl_s + SLW);
  float* qs = (float*)(sl_i + SLW); int* hist = (int*)(qs + 256);
  unsigned long long* keys = (unsigned long long*)fwraw;   // the candidate buffer, dead once the short list is built (SLW * 8 B <= 64 KiB)
  __shared__ int ovf, total, nsl, sel_bin, k_rem;
  __shared__ float qn2[4];
  constexpr bool F32 = sizeof(TG) == 4;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { ovf = 0; total = 0; nsl = 0; }
  const float qv = tid < C ? round_to<TG>(Q[(long)q * C + tid]) : 0.f;   // the query as the scan saw it
  if (tid < C) qs[tid] = qv;
  const float part = wave_sum(qv * qv);
  if (lane == 0) qn2[wave] = part;
  __syncthreads();
  const float delta = F32 ? 0.f : SIM_DELTA * fmaxf(1.f, sqrtf(qn2[0] + qn2[1] + qn2[2] + qn2[3]));
  // 1. gather the candidates into LDS (thread <-> stream)
  const float tq = tau[q];
  for (int st = tid; st < nstreams; st += 256) {
    const int c = cnt[(long)q * nstreams + st];
    if (c > cap) ovf = 1;
    const int nrec = min(c, cap);
    const long rec0 = ((long)q * nstreams + st) * cap;
    for (int j = 0; j < nrec; ++j) {
      if (RECORDS) {                                   // score [g][i] of lane quarter st & 3 is row g0 + 16 g + 4 (st & 3) + i
        const f32x4* sj = (const f32x4*)(rec_s + (rec0 + j) * 8);
        const f32x4 v[2] = {sj[0], sj[1]};
        const int g0 = rec_g[rec0 + j], r4 = 4 * (st & 3);
        int np = 0;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i) np += (v[g][i] >= tq && v[g][i] > -INFINITY) ? 1 : 0;
        if (np == 0) continue;
        int p = atomicAdd(&total, np);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (v[g][i] >= tq && v[g][i] > -INFINITY) {
              if (p < FSW) { cs[p] = v[g][i]; ci[p] = g0 + i + 16 * g + r4; }
              ++p;
            }
      } else {
        const uint2 e = lst[rec0 + j];
        const int p = atomicAdd(&total, 1);
        if (p < FSW) { cs[p] = __uint_as_float(e.x); ci[p] = (int)e.y; }
      }
    }
  }
  __syncthreads();
  if (total > FSW) ovf = 1;
  const int n = min(total, FSW);
  __syncthreads();
  // 2. T = the k-th best scan score, exactly (every row of the scan's top-k is a candidate); n <= k: every candidate is in
  float T = -INFINITY;
  if (!ovf && n > k) T = key2f_floor(block_kth_key([&](int i) { return f2key(cs[i]); }, n, k, hist, &sel_bin, &k_rem));
  // 3. short list: scan score >= T - delta (fp32: the rows >= T, ties at T included)
  if (!ovf) {
    const float cut = T - delta;
    for (int i = tid; i < n; i += 256) {
      if (cs[i] >= cut) {
        const int p = atomicAdd(&nsl, 1);
        if (p < SLW) { sl_s[p] = cs[i]; sl_i[p] = ci[i]; }
      }
    }
  }
  __syncthreads();
  if (nsl > SLW) ovf = 1;
  __syncthreads();
  if (ovf) {
    if (no_fallback) {                                 // tests: expose the raw overflow marker
      for (int j = tid; j < k; j += 256) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -2LL; }
      return;
    }
    if constexpr (FILTER)
      wide_brute_force<TG, true>(G, Ng, C, qs, k, g_offset, sl_s, sl_i, keys, hist, out_s + (long)q * k, out_i + (long)q * k, rlab, qlab[q], ne);
    else
      wide_brute_force<TG>(G, Ng, C, qs, k, g_offset, sl_s, sl_i, keys, hist, out_s + (long)q * k, out_i + (long)q * k);
    return;
  }
  const int m = nsl;
  // 4. exact re-scoring (16-bit): the chain of oracle/c/sim_chain.c over the stored values
  if (!F32)
    for (int j = tid; j < m; j += 256) sl_s[j] = chain_score_c<TG>(G, sl_i[j], C, qs);
  __syncthreads();
  // 5. rank by (chain score desc, index asc): one bitonic sort; entries beyond the short list (Ng < k) are (-inf, -1)
  int P = 1;
  while (P < m) P <<= 1;
  for (int j = tid; j < P; j += 256) keys[j] = j < m ? rank_key(sl_s[j], sl_i[j]) : ~0ull;
  __syncthreads();
  block_sort_u64(keys, P);
  for (int j = tid; j < k; j += 256) {
    out_s[(long)q * k + j] = j < m ? rank_key_score(keys[j]) : -INFINITY;
    out_i[(long)q * k + j] = j < m ? (long long)(unsigned)keys[j] + g_offset : -1LL;
  }
}

// The selection of cor_similarity_range: sim_final_wide without a filter, with the floor. (A kernel of its own: as one body shared with
// sim_final_wide the existing instantiations compiled to a different instruction order.) r carries the floors, the bounds the APPEND pass
// used and its sure counts. The candidates are the scores >= A_q; the rows of the band scores (B_q <= s < H_q) are collected in LDS
// (band_i, BAND_MAX rows) and re-scored by the chain, one row per thread, and counted if at or above the floor (re-scored where the gather
// met them, one lane of a wave at a time, 830 band rows per query cost 1.2 ms at 512 x 1M); count = the streams' sure counts + those band
// rows; ranked rows below the floor become tail. An overflow (of the lists, as before: a stream that lost records may have lost band
// rows; or more band rows than band_i holds) sends the query to range_brute_force, which ranks AND counts over the chain; with
// no_fallback it leaves index -2 in every slot and count -2.
constexpr int BAND_MAX = 16384;                        // band rows per query held in LDS (64 KiB: still one block per CU, as sim_final_wide)
constexpr size_t FINAL_RANGE_LDS = FINAL_WIDE_LDS + (size_t)BAND_MAX * 4;
struct RangeFinal {
  const float* thr; const float* ra; const float* rb; const float* rh; const int* sure; int* out_count;
  const int* rlab; const int* qlab; int ne;            // FILTER: the labels, for the fallback
};
// FILTER (cor_similarity_range_filtered): the scans stored and counted allowed scores only (a masked record slot is -inf: below A_q and
// B_q, neither candidate nor band row), so only the fallback differs: it counts and ranks the rows r.rlab / r.qlab / r.ne allow.
template <typename TG, bool RECORDS, bool FILTER = false>
__global__ void __launch_bounds__(256) sim_final_range(const float* __restrict__ Q, const TG* __restrict__ G, int Ng, int C, int k, long long g_offset,
                                                       const int* __restrict__ cnt, int nstreams, int cap, const float* __restrict__ rec_s,
                                                       const int* __restrict__ rec_g, const uint2* __restrict__ lst, float* out_s, long long* out_i,
                                                       int no_fallback, const RangeFinal r) {
  extern __shared__ __attribute__((aligned(16))) char fwraw[];
  float* cs = (float*)fwraw; int* ci = (int*)(cs + FSW);
  float* sl_s = (float*)(ci + FSW); int* sl_i = (int*)(sl_s + SLW);
  float* qs = (float*)(sl_i + SLW); int* hist = (int*)(qs + 256);
  int* band_i = hist + 256;                            // rows of the band scores
  unsigned long long* keys = (unsigned long long*)fwraw;   // the candidate buffer, dead once the short list is built (SLW * 8 B <= 64 KiB)
  __shared__ int ovf, total, nsl, sel_bin, k_rem;
  __shared__ float qn2[4];
  constexpr bool F32 = sizeof(TG) == 4;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ int rcount, nband;                        // sure counts + band rows at or above the floor; band rows met
  const float thr = r.thr[q], rb = r.rb[q], rh = r.rh[q];
  if ((__float_as_uint(thr) & 0x7fffffffu) > 0x7f800000u) {        // a NaN floor (by its bits: the file is built with -fno-honor-nans): the empty set
    for (int j = tid; j < k; j += 256) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -1LL; }
    if (tid == 0) r.out_count[q] = 0;
    return;
  }
  if (tid == 0) { ovf = 0; total = 0; nsl = 0; rcount = 0; nband = 0; }
  const float qv = tid < C ? round_to<TG>(Q[(long)q * C + tid]) : 0.f;   // the query as the scan saw it
  if (tid < C) qs[tid] = qv;
  const float part = wave_sum(qv * qv);
  if (lane == 0) qn2[wave] = part;
  __syncthreads();
  const float delta = F32 ? 0.f : SIM_DELTA * fmaxf(1.f, sqrtf(qn2[0] + qn2[1] + qn2[2] + qn2[3]));
  // 1. gather the candidates into LDS (thread <-> stream)
  const float tq = r.ra[q];                            // A_q
  int mine = 0;                                        // this thread's share of the count
  auto band = [&](float s, int row) {                  // 16-bit rows: the chain decides a band row, below (fp32: B_q = H_q, no band)
    if constexpr (!F32) {
      if (s >= rb && s < rh) {
        const int p = atomicAdd(&nband, 1);
        if (p < BAND_MAX) band_i[p] = row;
      }
    }
  };
  for (int st = tid; st < nstreams; st += 256) {
    const int c = cnt[(long)q * nstreams + st];
    if (c > cap) ovf = 1;
    mine += r.sure[(long)q * nstreams + st];
    const int nrec = min(c, cap);
    const long rec0 = ((long)q * nstreams + st) * cap;
    for (int j = 0; j < nrec; ++j) {
      if (RECORDS) {                                   // score [g][i] of lane quarter st & 3 is row g0 + 16 g + 4 (st & 3) + i
        const f32x4* sj = (const f32x4*)(rec_s + (rec0 + j) * 8);
        const f32x4 v[2] = {sj[0], sj[1]};
        const int g0 = rec_g[rec0 + j], r4 = 4 * (st & 3);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i) band(v[g][i], g0 + i + 16 * g + r4);
        int np = 0;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i) np += (v[g][i] >= tq && v[g][i] > -INFINITY) ? 1 : 0;
        if (np == 0) continue;
        int p = atomicAdd(&total, np);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (v[g][i] >= tq && v[g][i] > -INFINITY) {
              if (p < FSW) { cs[p] = v[g][i]; ci[p] = g0 + i + 16 * g + r4; }
              ++p;
            }
      } else {
        const uint2 e = lst[rec0 + j];
        band(__uint_as_float(e.x), (int)e.y);
        if (__uint_as_float(e.x) < tq) continue;       // a band row below A_q: counted above, no list candidate
        const int p = atomicAdd(&total, 1);
        if (p < FSW) { cs[p] = __uint_as_float(e.x); ci[p] = (int)e.y; }
      }
    }
  }
  __syncthreads();
  if (total > FSW || nband > BAND_MAX) ovf = 1;
  const int n = min(total, FSW);
  if constexpr (!F32) {
    if (nband <= BAND_MAX)
      for (int j = tid; j < nband; j += 256) mine += chain_score_c<TG>(G, band_i[j], C, qs) >= thr ? 1 : 0;
  }
  if (mine) atomicAdd(&rcount, mine);
  __syncthreads();
  // 2. T = the k-th best scan score, exactly (every row of the scan's top-k is a candidate); n <= k: every candidate is in
  float T = -INFINITY;
  if (!ovf && n > k) T = key2f_floor(block_kth_key([&](int i) { return f2key(cs[i]); }, n, k, hist, &sel_bin, &k_rem));
  // 3. short list: scan score >= T - delta (fp32: the rows >= T, ties at T included)
  if (!ovf) {
    const float cut = T - delta;
    for (int i = tid; i < n; i += 256) {
      if (cs[i] >= cut) {
        const int p = atomicAdd(&nsl, 1);
        if (p < SLW) { sl_s[p] = cs[i]; sl_i[p] = ci[i]; }
      }
    }
  }
  __syncthreads();
  if (nsl > SLW) ovf = 1;
  __syncthreads();
  if (ovf) {
    if (no_fallback) {                                 // tests: expose the raw overflow marker
      for (int j = tid; j < k; j += 256) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -2LL; }
      if (tid == 0) r.out_count[q] = -2;
      return;
    }
    if constexpr (FILTER)
      range_brute_force<TG, true>(G, Ng, C, qs, k, g_offset, thr, sl_s, sl_i, keys, hist, (float*)ci, (long long*)(ci + 256), out_s + (long)q * k,
                                  out_i + (long)q * k, r.out_count + q, r.rlab, r.qlab[q], r.ne);
    else
      range_brute_force<TG>(G, Ng, C, qs, k, g_offset, thr, sl_s, sl_i, keys, hist, (float*)ci, (long long*)(ci + 256), out_s + (long)q * k,
                            out_i + (long)q * k, r.out_count + q);
    return;
  }
  if (tid == 0) r.out_count[q] = rcount;
  const int m = nsl;
  // 4. exact re-scoring (16-bit): the chain of oracle/c/sim_chain.c over the stored values
  if (!F32)
    for (int j = tid; j < m; j += 256) sl_s[j] = chain_score_c<TG>(G, sl_i[j], C, qs);
  __syncthreads();
  // 5. rank by (chain score desc, index asc): one bitonic sort; entries beyond the short list (Ng < k) are (-inf, -1)
  int P = 1;
  while (P < m) P <<= 1;
  for (int j = tid; j < P; j += 256) keys[j] = j < m ? rank_key(sl_s[j], sl_i[j]) : ~0ull;
  __syncthreads();
  block_sort_u64(keys, P);
  for (int j = tid; j < k; j += 256) {
    const bool in = j < m && rank_key_score(keys[j]) >= thr;   // below the floor: tail (a suffix of the ranked rows)
    out_s[(long)q * k + j] = in ? rank_key_score(keys[j]) : -INFINITY;
    out_i[(long)q * k + j] = in ? (long long)(unsigned)keys[j] + g_offset : -1LL;
  }
}

// The floors of cor_similarity_range as the APPEND pass and the selection use them, one block per query behind sim_tau_wide:
//   B_q = thr_q - delta_q, H_q = thr_q + delta_q, A_q = max(tau_q, B_q), each floored at -3e38 so that a masked -inf score never passes.
// delta_q is sim_tau_wide's (0 for fp32 rows: no band). SIM_DELTA is twice the bound of |scan - chain|, so scan >= H_q implies chain >= thr_q
// and scan < B_q implies chain < thr_q, the rounding of the two sums included. A NaN floor (told by its bits) gives +inf three times:
// nothing counts, nothing is appended.
template <typename TG>
__global__ void __launch_bounds__(256) sim_range_bounds(const float* __restrict__ Q, int C, const float* __restrict__ thr, const float* __restrict__ tau,
                                                        float* ra, float* rb, float* rh) {
  __shared__ float part[4];
  const int q = blockIdx.x, tid = threadIdx.x;
  float n2 = 0.f;
  if (sizeof(TG) != 4 && tid < C) { const float x = round_to<TG>(Q[(long)q * C + tid]); n2 = x * x; }
  n2 = wave_sum(n2);
  if ((tid & 63) == 0) part[tid >> 6] = n2;
  __syncthreads();
  if (tid != 0) return;
  const float delta = sizeof(TG) == 4 ? 0.f : SIM_DELTA * fmaxf(1.f, sqrtf(part[0] + part[1] + part[2] + part[3]));
  const float t = thr[q];
  float b = INFINITY, h = INFINITY, a = INFINITY;
  if ((__float_as_uint(t) & 0x7fffffffu) <= 0x7f800000u) {
    b = fmaxf(t - delta, -3.0e38f); h = fmaxf(t + delta, -3.0e38f); a = fmaxf(tau[q], b);
  }
  ra[q] = a; rb[q] = b; rh[q] = h;
}

// ---------------------------------------------------------------------------------------------------------------------
// DISTINCT GROUPS (cor_similarity_topk_distinct): every row has an int32 group id grp[row] (the source image of a region; a negative id
// makes the row a group of its own); per query the k best group REPRESENTATIVES (a group's best allowed row by (chain score desc, index
// asc)), ordered the same way. The wide route with three changes: the sample keeps rows (sim_scan / sim_wide_scan GROUP), the threshold
// counts distinct groups (sim_tau_distinct), the selection reduces to one row per group (sim_final_distinct). The APPEND scans are the
// wide / filtered instantiations unchanged: they append scores >= tau_q whatever the groups are.
// one unsigned per group: the id, or for a negative id the row itself behind a set top bit (rows < 2^31: never equal to an id or another row)
__device__ __forceinline__ unsigned group_key(const int* __restrict__ grp, int row) {
  const int g = grp[row];
  return g >= 0 ? (unsigned)g : (0x80000000u | (unsigned)row);
}

// tau_q of the distinct route, one block per query. The sample pass stored n values (order-preserving keys, sg) and the row of each
// (sgrow); the values are reduced to ONE PER GROUP ID (the best kept; a sort of (group key, inverted score key) puts a group's best
// first) and tau_q = the k-th largest of those - delta_q. Validity: the k values at or above it belong to k DIFFERENT groups, each with an
// allowed row whose scan score is >= tau_q + delta_q, so at least k groups have a representative that good: the k-th best representative's
// scan score is >= tau_q + delta_q and every row of the answer passes tau_q (the argument of sim_final_distinct). The k-th largest sampled
// value itself proves nothing here: two sampled rows may be regions of one image. Fewer than k distinct sampled groups: -inf.
// The sort runs in a fixed LDS array of TAU_DISTINCT_MAX keys. make_wide's group plan keeps ngroups within it for every Ng (it widens the
// sample stride, see there), cor_similarity_topk_distinct refuses a plan that does not, and the kernel itself never touches more: it
// ranks the FIRST TAU_DISTINCT_MAX stored values only, which is still a valid bound (any subset of the sampled rows proves the same
// thing, with a lower threshold).
constexpr int TAU_DISTINCT_MAX = 4096;
template <typename TG>
__global__ void __launch_bounds__(256) sim_tau_distinct(const float* __restrict__ Q, int C, const unsigned* __restrict__ sg, const int* __restrict__ sgrow,
                                                        int nstored, int k, const int* __restrict__ grp, float* tau) {
  __shared__ unsigned long long keys[TAU_DISTINCT_MAX];
  const int n = nstored < TAU_DISTINCT_MAX ? nstored : TAU_DISTINCT_MAX;   // values ranked; nstored = the row stride of sg / sgrow
  __shared__ int hist[256], sel_bin, k_rem, nheads;
  __shared__ float part[4];
  const int q = blockIdx.x, tid = threadIdx.x;
  float n2 = 0.f;
  if (sizeof(TG) != 4 && tid < C) { const float x = round_to<TG>(Q[(long)q * C + tid]); n2 = x * x; }
  n2 = wave_sum(n2);
  if ((tid & 63) == 0) part[tid >> 6] = n2;
  if (tid == 0) nheads = 0;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += 256) {
    unsigned long long key = ~0ull;                    // padding and groups without a finite allowed score: behind everything
    if (i < n) {
      const unsigned v = sg[(long)q * nstored + i];
      if (v > f2key(-INFINITY)) key = ((unsigned long long)group_key(grp, sgrow[(long)q * nstored + i]) << 32) | (unsigned)~v;
    }
    keys[i] = key;
  }
  __syncthreads();
  const float delta = sizeof(TG) == 4 ? 0.f : SIM_DELTA * fmaxf(1.f, sqrtf(part[0] + part[1] + part[2] + part[3]));
  block_sort_u64(keys, P);
  auto head = [&](int i) { return keys[i] != ~0ull && (i == 0 || (keys[i - 1] >> 32) != (keys[i] >> 32)); };
  int mine = 0;
  for (int i = tid; i < P; i += 256) mine += head(i) ? 1 : 0;
  if (mine) atomicAdd(&nheads, mine);
  __syncthreads();
  float t = -INFINITY;
  if (nheads >= k) {                                   // (block-uniform)
    const unsigned kth = block_kth_key([&](int i) { return head(i) ? ~(unsigned)keys[i] : 0u; }, P, k, hist, &sel_bin, &k_rem);
    t = key2f_floor(kth) - delta;
  }
  if (tid == 0) tau[q] = t;
}

// flag[j] = 1 iff entry j of rk[0 .. m) is the FIRST of its group there (rk: rank keys, low word = row, in rank order), else 0:
// sort (group key, position) and mark the head of every group run. k2: scratch for the next power of two >= m keys. 256 threads.
__device__ void first_of_group(const unsigned long long* rk, int m, const int* __restrict__ grp, unsigned long long* k2, int* flag) {
  int P = 1;
  while (P < m) P <<= 1;
  for (int j = threadIdx.x; j < P; j += 256)
    k2[j] = j < m ? (((unsigned long long)group_key(grp, (int)(unsigned)rk[j]) << 32) | (unsigned)j) : ~0ull;
  __syncthreads();
  block_sort_u64(k2, P);
  for (int j = threadIdx.x; j < m; j += 256) {
    const unsigned long long x = k2[j];
    flag[(unsigned)x] = (j == 0 || (k2[j - 1] >> 32) != (x >> 32)) ? 1 : 0;
  }
  __syncthreads();
}
// exclusive prefix of flag[0 .. m) (m <= 8 * 256) at position 8 * tid (thread tid owns entries 8 tid .. 8 tid + 7); *total = the sum
__device__ int block_prefix8(const int* flag, int m, int* wtot, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int local = 0;
  for (int u = 0; u < 8; ++u) { const int j = 8 * tid + u; local += j < m ? flag[j] : 0; }
  int incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
  __syncthreads();                                     // wtot of an earlier call is no longer read
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int base = incl - local, tot = 0;
  for (int w = 0; w < 4; ++w) { base += w < wave ? wtot[w] : 0; tot += wtot[w]; }
  *total = tot;
  return base;
}

// Exact fallback of ONE overflowed query of the distinct route (block of 256 threads): the shard is paged through IN RANK ORDER. A page =
// the next <= SLW allowed rows behind the last page's last rank key (score desc, index asc): the page's lowest score key by
// block_kth_key over the chain scores of the rows not yet paged, one pass collects the rows above it and the first ties at it in index
// order (wide_brute_force's scheme), a bitonic sort ranks the page. Each page is folded into a table of the <= k groups found so far:
// first_of_group marks the page's first row of every group, the marks of groups already in the table are dropped, and the survivors -
// representatives, in rank order - go straight to the output. Stops at k groups or when the rows run out. Every page consumes SLW rows,
// so it terminates; five chain passes over the shard per page: slow only for inputs that are pathological anyway (thousands of rows of
// one group ahead of everything else).
// The body takes the score of a row and the allow predicate as callables (distinct_brute_force_by, as brute_force_by does): the chain over a
// float / 16-bit gallery in distinct_brute_force (rlab == nullptr: unfiltered), the integer score of the int8 route in sim_i8_repair_distinct.
template <typename ScoreAt, typename Allowed>
__device__ __forceinline__ void distinct_brute_force_by(const ScoreAt score_at, const Allowed allowed, int Ng, int k, long long g_offset,
                                                        const int* __restrict__ grp, float* sl_s, int* sl_i, int* flag, unsigned long long* keys,
                                                        unsigned long long* k2, unsigned* found, int* hist, float* out_s, long long* out_i) {
  __shared__ int sel_bin, k_rem, n_above, n_allowed, wcnt[4], wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) n_allowed = 0;
  __syncthreads();
  {
    int mine = 0;
    for (int g = tid; g < Ng; g += 256) mine += allowed(g) ? 1 : 0;
    atomicAdd(&n_allowed, mine);
  }
  __syncthreads();
  int remaining = n_allowed, nfound = 0;               // allowed rows not yet paged; groups written (both block-uniform)
  bool first = true;
  unsigned long long last = 0ull;                      // rank key of the last row of the last page
  while (remaining > 0 && nfound < k) {
    const int P = min(SLW, remaining);
    // score and eligibility of row g: allowed and behind `last` in rank order; key 0 = not eligible (below every score's key)
    auto score_of = [&](int g, float& s) {
      if (!allowed(g)) return 0u;
      s = score_at(g);
      return (first || rank_key(s, g) > last) ? f2key(s) : 0u;
    };
    unsigned kth = 0u;
    int need = 0, above = P;
    if (remaining > P) {
      kth = block_kth_key([&](int g) { float s; return score_of(g, s); }, Ng, P, hist, &sel_bin, &k_rem);
      need = k_rem; above = P - need;
    }
    if (tid == 0) n_above = 0;
    __syncthreads();
    int taken = 0;
    for (int g0 = 0; g0 < Ng; g0 += 256) {
      const int g = g0 + tid;
      float s = -INFINITY; unsigned key = 0u;
      if (g < Ng) key = score_of(g, s);
      const bool up = key > kth, tie = key != 0u && key == kth;
      if (up) { const int p = atomicAdd(&n_above, 1); sl_s[p] = s; sl_i[p] = g; }
      const unsigned long long b = __builtin_amdgcn_ballot_w64(tie);
      if (lane == 0) wcnt[wave] = __builtin_popcountll(b);
      __syncthreads();
      int before = taken, tot = 0;
      for (int w = 0; w < 4; ++w) { before += w < wave ? wcnt[w] : 0; tot += wcnt[w]; }
      if (tie) {
        const int pos = before + __builtin_popcountll(b & ((1ull << lane) - 1ull));
        if (pos < need) { sl_s[above + pos] = s; sl_i[above + pos] = g; }
      }
      taken += tot;
      __syncthreads();
    }
    int P2 = 1;
    while (P2 < P) P2 <<= 1;
    for (int j = tid; j < P2; j += 256) keys[j] = j < P ? rank_key(sl_s[j], sl_i[j]) : ~0ull;
    __syncthreads();
    block_sort_u64(keys, P2);
    __syncthreads();
    first_of_group(keys, P, grp, k2, flag);
    for (int j = tid; j < P; j += 256) {
      if (flag[j]) {
        const unsigned gk = group_key(grp, (int)(unsigned)keys[j]);
        for (int t = 0; t < nfound; ++t) if (found[t] == gk) { flag[j] = 0; break; }
      }
    }
    __syncthreads();
    int tot;
    int slot = nfound + block_prefix8(flag, P, wtot, &tot);
    for (int u = 0; u < 8; ++u) {
      const int j = 8 * tid + u;
      if (j < P && flag[j]) {
        if (slot < k) {
          const int row = (int)(unsigned)keys[j];
          out_s[slot] = rank_key_score(keys[j]); out_i[slot] = (long long)row + g_offset;
          found[slot] = group_key(grp, row);
        }
        ++slot;
      }
    }
    last = keys[P - 1];
    __syncthreads();
    nfound = min(k, nfound + tot);
    remaining -= P;
    first = false;
  }
  for (int j = nfound + tid; j < k; j += 256) { out_s[j] = -INFINITY; out_i[j] = -1LL; }
}
template <typename TG>
__device__ void distinct_brute_force(const TG* __restrict__ G, int Ng, int C, const float* qs, int k, long long g_offset, const int* __restrict__ grp,
                                     float* sl_s, int* sl_i, int* flag, unsigned long long* keys, unsigned long long* k2, unsigned* found, int* hist,
                                     float* out_s, long long* out_i, const int* __restrict__ rlab, int ql, int ne) {
  distinct_brute_force_by([&](int g) { return chain_score_c<TG>(G, g, C, qs); },
                          [&](int g) { return rlab == nullptr || row_allowed(rlab, g, ql, ne); }, Ng, k, g_offset, grp, sl_s, sl_i, flag,
                          keys, k2, found, hist, out_s, out_i);
}

// Exact selection of the distinct route, one block of 256 threads per query; the gather front ends of sim_final_wide (RECORDS / entry
// lists). LDS: cs/ci [FSW] | keys [FSW] | sl_s/sl_i/flag [SLW] | qs[256] | hist[256] = 154 KiB.
//   2. the candidates are reduced to one per group by SCAN score (sort of (group key, inverted score key): a group's best comes first)
//      and T = the k-th best of those, exactly: k groups have a candidate row with scan score >= T. Fewer than k groups: T = -inf.
//   3. the short list holds EVERY candidate row with scan score >= T - delta_q, not one per group: within delta_q another row of the group
//      can win the chain re-score, and a row with exactly the same chain score and a lower index must win.
//      Exactness. SIM_DELTA is twice the bound of |scan - chain| per score. k groups have a row that scans >= T, hence a representative with
//      chain score >= T - delta_q / 2, so the k-th best representative has a chain score >= T - delta_q / 2 and every representative of the
//      answer scans >= T - delta_q: it is in the short list (T - delta_q >= tau_q: the k sampled rows behind tau_q are candidates of k
//      groups). It is the best row of its whole group, so the best of its group's short-listed rows too. A group whose representative is
//      NOT short-listed has every chain score < T - delta_q / 2: whatever row of it is short-listed ranks behind the k-th representative.
//   4. chain re-score (16-bit), one sort by (chain score desc, index asc): rank order; first_of_group keeps the first row of every group;
//      a prefix count over the kept rows gives the output slots; the first k are written, then the (-inf, -1) tail.
// Group ids are read from global memory by row (grp). Overflow (a stream list, the candidate buffer, the short list): distinct_brute_force.
template <typename TG, bool RECORDS>
__global__ void __launch_bounds__(256) sim_final_distinct(const float* __restrict__ Q, const TG* __restrict__ G, int Ng, int C, int k, long long g_offset,
                                                          const float* __restrict__ tau, const int* __restrict__ cnt, int nstreams, int cap,
                                                          const float* __restrict__ rec_s, const int* __restrict__ rec_g, const uint2* __restrict__ lst,
                                                          const int* __restrict__ grp, float* out_s, long long* out_i, int no_fallback,
                                                          const int* __restrict__ rlab, const int* __restrict__ qlab, int ne) {
  extern __shared__ __attribute__((aligned(16))) char fdraw[];
  float* cs = (float*)fdraw; int* ci = (int*)(cs + FSW);
  unsigned long long* keys = (unsigned long long*)(ci + FSW);
  float* sl_s = (float*)(keys + FSW); int* sl_i = (int*)(sl_s + SLW); int* flag = sl_i + SLW;
  float* qs = (float*)(flag + SLW); int* hist = (int*)(qs + 256);
  unsigned long long* k2 = (unsigned long long*)fdraw;   // the candidate buffer, dead once the short list is built (SLW * 8 B <= 64 KiB)
  __shared__ int ovf, total, nsl, sel_bin, k_rem, nheads, wtot[4];
  __shared__ float qn2[4];
  constexpr bool F32 = sizeof(TG) == 4;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { ovf = 0; total = 0; nsl = 0; nheads = 0; }
  const float qv = tid < C ? round_to<TG>(Q[(long)q * C + tid]) : 0.f;   // the query as the scan saw it
  if (tid < C) qs[tid] = qv;
  const float part = wave_sum(qv * qv);
  if (lane == 0) qn2[wave] = part;
  __syncthreads();
  const float delta = F32 ? 0.f : SIM_DELTA * fmaxf(1.f, sqrtf(qn2[0] + qn2[1] + qn2[2] + qn2[3]));
  // 1. gather the candidates into LDS (thread <-> stream), as sim_final_wide does
  const float tq = tau[q];
  for (int st = tid; st < nstreams; st += 256) {
    const int c = cnt[(long)q * nstreams + st];
    if (c > cap) ovf = 1;
    const int nrec = min(c, cap);
    const long rec0 = ((long)q * nstreams + st) * cap;
    for (int j = 0; j < nrec; ++j) {
      if (RECORDS) {                                   // score [g][i] of lane quarter st & 3 is row g0 + 16 g + 4 (st & 3) + i
        const f32x4* sj = (const f32x4*)(rec_s + (rec0 + j) * 8);
        const f32x4 v[2] = {sj[0], sj[1]};
        const int g0 = rec_g[rec0 + j], r4 = 4 * (st & 3);
        int np = 0;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i) np += (v[g][i] >= tq && v[g][i] > -INFINITY) ? 1 : 0;
        if (np == 0) continue;
        int p = atomicAdd(&total, np);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (v[g][i] >= tq && v[g][i] > -INFINITY) {
              if (p < FSW) { cs[p] = v[g][i]; ci[p] = g0 + i + 16 * g + r4; }
              ++p;
            }
      } else {
        const uint2 e = lst[rec0 + j];
        const int p = atomicAdd(&total, 1);
        if (p < FSW) { cs[p] = __uint_as_float(e.x); ci[p] = (int)e.y; }
      }
    }
  }
  __syncthreads();
  if (total > FSW) ovf = 1;
  const int n = min(total, FSW);
  __syncthreads();
  // 2. T = the k-th best per-group scan score (n <= k candidates: at most k groups, every candidate is in)
  float T = -INFINITY;
  if (!ovf && n > k) {
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += 256) keys[i] = i < n ? (((unsigned long long)group_key(grp, ci[i]) << 32) | (unsigned)~f2key(cs[i])) : ~0ull;
    __syncthreads();
    block_sort_u64(keys, P);
    auto head = [&](int i) { return i < n && (i == 0 || (keys[i - 1] >> 32) != (keys[i] >> 32)); };
    int mine = 0;
    for (int i = tid; i < n; i += 256) mine += head(i) ? 1 : 0;
    if (mine) atomicAdd(&nheads, mine);
    __syncthreads();
    if (nheads >= k) T = key2f_floor(block_kth_key([&](int i) { return head(i) ? ~(unsigned)keys[i] : 0u; }, n, k, hist, &sel_bin, &k_rem));
  }
  // 3. short list: every candidate with scan score >= T - delta (fp32: the rows >= T, ties at T included)
  if (!ovf) {
    const float cut = T - delta;
    for (int i = tid; i < n; i += 256) {
      if (cs[i] >= cut) {
        const int p = atomicAdd(&nsl, 1);
        if (p < SLW) { sl_s[p] = cs[i]; sl_i[p] = ci[i]; }
      }
    }
  }
  __syncthreads();
  if (nsl > SLW) ovf = 1;
  __syncthreads();
  if (ovf) {
    if (no_fallback) {                                 // tests: expose the raw overflow marker
      for (int j = tid; j < k; j += 256) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -2LL; }
      return;
    }
    // scratch: the found-group table in front of the candidate buffer, the page's group keys behind it
    distinct_brute_force<TG>(G, Ng, C, qs, k, g_offset, grp, sl_s, sl_i, flag, keys, (unsigned long long*)(fdraw + 4096), (unsigned*)fdraw, hist,
                             out_s + (long)q * k, out_i + (long)q * k, rlab, rlab ? qlab[q] : -1, ne);
    return;
  }
  const int m = nsl;
  // 4. exact re-scoring (16-bit), rank order, first row of every group, output slots
  if (!F32)
    for (int j = tid; j < m; j += 256) sl_s[j] = chain_score_c<TG>(G, sl_i[j], C, qs);
  __syncthreads();
  int P = 1;
  while (P < m) P <<= 1;
  for (int j = tid; j < P; j += 256) keys[j] = j < m ? rank_key(sl_s[j], sl_i[j]) : ~0ull;
  __syncthreads();
  block_sort_u64(keys, P);
  __syncthreads();
  first_of_group(keys, m, grp, k2, flag);
  int ng;
  int slot = block_prefix8(flag, m, wtot, &ng);
  for (int u = 0; u < 8; ++u) {
    const int j = 8 * tid + u;
    if (j < m && flag[j]) {
      if (slot < k) { out_s[(long)q * k + slot] = rank_key_score(keys[j]); out_i[(long)q * k + slot] = (long long)(unsigned)keys[j] + g_offset; }
      ++slot;
    }
  }
  for (int j = ng + tid; j < k; j += 256) { out_s[(long)q * k + j] = -INFINITY; out_i[(long)q * k + j] = -1LL; }
}
constexpr size_t FINAL_DISTINCT_LDS = (size_t)FSW * 16 + SLW * 12 + 256 * 4 + 256 * 4;

// plan of the wide route (host; shared by the launcher and cor_topk_workspace_bytes). scan = the sim_scan form (16-bit, C = 256).
// filter = the filtered route (any k): four sample values per group; the scan form's slices walk <= 128 super-tiles (their labels fill
// the 32 KiB behind sim_scan's 4-slot ring).
struct WidePlan {
  bool scan;
  int qb, nqg, nqt;                  // scan form: query blocks per wave, query groups of 256 * qb; tile form: 32-query tiles
  int nsplit, tiles_per_split, ntiles, nstreams, cap;                // APPEND
  int s_stride, s_tiles, s_nsplit, s_tiles_per_split, ngroups;       // SAMPLE (ngroups == 0: no sample, tau = -inf)
  size_t off_img, off_sg, off_dq, off_tau, off_flags, off_ovf, off_cnt, off_recs, off_recg, bytes;
  size_t off_sgrow;                  // group: the rows of the sample values
  size_t off_rng, off_sure;          // range: A_q, B_q, H_q (three f32 [Bq]) and the sure counts per stream
};
// group = the distinct-group route (any k): the sample keeps NV = 1 (filter: 4) values WITH rows per group, and the capacity plan below.
// i8 = the int8 route (cor_similarity_topk_i8; scan must be set): the scan form's 64-row tiles and lane-quarter streams, query groups of
// 512 (sim_i8_scan: 8 waves x 64 queries), and entry lists as the tile form keeps them. i8 + filter (cor_similarity_topk_i8_filtered): four
// sample values per group like every filtered plan, but no 128 clamp: sim_i8_scan carries a tile's labels with the tile.
// i8 + group (cor_similarity_topk_i8_distinct): the group capacity numbers as they are (stride <= 1024 / k, expect = 6 k stride: the sampled
// values are maxima of the same disjoint row classes, rows 4 rq .. 4 rq + 3 of every 16 of a slice). Without the clamp the sample has at
// most 256 slices for every Ng, so ngroups <= 4 streams x 256 x 4 values = TAU_DISTINCT_MAX with the filter and the stride never widens.
// range = cor_similarity_range (any k, no filter, no groups): the streams also take the band rows (scan within delta_q of the floor: about
// 2 delta_q * Ng * the score density at the floor per query, some 830 rows over ~1000 streams at 1M unit rows of C = 256 and a floor of 0), so
// every stream gets 6 more places; the bounds and the sure counts sit behind the other buffers.
// filter + range = cor_similarity_range_filtered: the filtered plan (interleaved slices, four sample values per group, the 128 clamp, which
// satisfies the 4095 bound) with the range plan's extra places and buffers; the scan form always with qb = 1 (query groups of 256).
inline WidePlan make_wide(int Bq, int Ng, int k, bool scan, bool filter = false, bool group = false, bool i8 = false, bool range = false) {
  WidePlan p{};
  p.scan = scan;
  const int rows = scan ? 64 : 32;                     // rows per tile of the scan kernel
  p.ntiles = cdiv(Ng, rows);
  int want;
  if (scan) {
    p.qb = (i8 || Bq > 256) && !(filter && range) ? 2 : 1;   // (filter + range: sim_scan<QB = 2> cannot hold labels and range state, see there)
    p.nqg = cdiv(Bq, 256 * p.qb);
    want = device_cus() / p.nqg;                       // one resident block per CU
    if (want > 256) want = 256;
  } else {
    p.nqt = cdiv(Bq, 32);
    want = cdiv(4096, p.nqt);                          // ~16 waves per CU
  }
  if (want > p.ntiles) want = p.ntiles;
  if (want < 1) want = 1;
  p.tiles_per_split = cdiv(p.ntiles, want);
  if (filter && scan && !i8 && p.tiles_per_split > 128) p.tiles_per_split = 128;
  if (range && scan && p.tiles_per_split > 4095) p.tiles_per_split = 4095;   // sim_scan RANGE counts a lane's sure rows in 16 bits
  p.nsplit = cdiv(p.ntiles, p.tiles_per_split);
  const int per_tile = scan ? 4 : 2;                   // streams per slice: lane quarters (scan) / lane halves (tiles)
  p.nstreams = per_tile * p.nsplit;
  const int stream_max = scan && !i8 ? 2 * p.tiles_per_split : 16 * p.tiles_per_split;   // records / entries a stream can hold at most
  if (Ng <= 4096) {                                    // tiny shard: no sample pass, every row is a candidate (<= FSW)
    p.s_stride = 1;
    p.cap = stream_max;
  } else {
    // Sample groups: >= 2 k per query keep tau near the k-th best score (k-th largest of G group maxima: the top ~G ln(G / (G - k))
    // sampled rows, 1.4 k at G = 2 k), so the full scan admits ~1.4 k * stride candidates per query; the stride keeps that below
    // FSW / 2. Groups: 4 per slice (scan form, up to 256 slices: 1024) or 2 (tile form, up to 512 slices); Ng > 4096 gives >= 260.
    if (scan) p.s_stride = p.ntiles / 16 >= 128 ? 16 : (p.ntiles / 128 > 1 ? p.ntiles / 128 : 1);
    else p.s_stride = p.ntiles / 512 > 1 ? p.ntiles / 512 : 1;
    // group: tau_q is the k-th largest sampled value AFTER the reduction to one per group id, i.e. sample rank k' = c k, where c = the
    // sampled values per group among the best. The sampled values are maxima of disjoint row sets (a slice's rows of one lane quarter:
    // rows 4 rq .. 4 rq + 3 of every 16), so a run of R <= 8 consecutive rows of one image reaches at most 3 of them, and only if its
    // rows score alike; independent scores give c ~ 1 (a collision needs two of the ~k best sampled rows in one of Ng / 4.5 images).
    // Planned for c = 2: the scan admits the rows above the sample's 2k-th value, ~1.4 * 2 k * stride of them (the 1.4 of the comment
    // above), and the stride keeps that below FSW / 2: stride <= 1024 / k, expect = 6 k stride (the same 2x slack). More correlated
    // galleries overflow into the paging fallback: exact, slower.
    const int smax = group ? (1024 / k > 1 ? 1024 / k : 1) : (2048 / k > 1 ? 2048 / k : 1);
    if (p.s_stride > smax) p.s_stride = smax;
    if (group && filter && scan && !i8) {
      // sim_tau_distinct sorts at most TAU_DISTINCT_MAX = 4096 sample values per query in LDS. With a filter the scan form's sample slices
      // walk <= 128 super-tiles (the label ring), so the slice count, and with it ngroups = 16 per slice, grows with Ng: beyond
      // 128 * 256 sample super-tiles the stride widens to keep 256 slices. That trades candidates for the bound: ~2.8 k * stride rows pass
      // tau_q, within FSW while stride <= 2900 / k, i.e. up to ~23M rows at k = 256, ~60M at k = 100 (128 * 256 * 64 rows per unit of
      // stride); larger shards than that overflow into the paging fallback (exact, slow) rather than into memory they do not own.
      const int need = cdiv(p.ntiles, 128 * 256);
      if (p.s_stride < need) p.s_stride = need;
    }
    p.s_tiles = cdiv(p.ntiles, p.s_stride);
    int sw = scan ? 256 : 512;
    if (sw > p.s_tiles) sw = p.s_tiles;
    p.s_tiles_per_split = cdiv(p.s_tiles, sw);
    if (filter && scan && !i8 && p.s_tiles_per_split > 128) p.s_tiles_per_split = 128;
    p.s_nsplit = cdiv(p.s_tiles, p.s_tiles_per_split);
    p.ngroups = per_tile * p.s_nsplit * (filter ? 4 : 1);
    const long expect = (group ? 6L : 3L) * k * p.s_stride;   // candidates per query, ~2x slack
    // per stream: Poisson with mean ~ expect / nstreams; +10 keeps P(overflow) per search small
    p.cap = (int)(2 * expect / p.nstreams) + 10 + (range ? 6 : 0);
    if (p.cap > stream_max) p.cap = stream_max;
  }
  const int Bqp = scan && !i8 ? p.nqg * 256 * p.qb : 0;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += (n + 255) & ~(size_t)255; return at; };
  p.off_img = take(i8 ? (size_t)Bq * 256 : scan ? (size_t)p.nqg * 8 * p.qb * 16 * 64 * 16 : 0);   // (i8: the quantised queries, scales in off_dq)
  const size_t sg_n = (size_t)Bq * p.ngroups > (size_t)32 * Bqp ? (size_t)Bq * p.ngroups : (size_t)32 * Bqp;   // (sim_prep clears 32 x Bqp)
  p.off_sg = take(sg_n * 4 + 4);
  p.off_dq = take((size_t)Bq * 4);
  p.off_tau = take((size_t)Bq * 4);
  p.off_flags = take(16);
  p.off_ovf = take((size_t)Bq * 4);
  p.off_cnt = take((size_t)Bq * p.nstreams * 4);
  p.off_recs = take((size_t)Bq * p.nstreams * p.cap * (scan && !i8 ? 32 : 8));   // a record = 8 scores; an entry = (score, row)
  p.off_recg = take(scan && !i8 ? (size_t)Bq * p.nstreams * p.cap * 4 : 0);
  p.off_sgrow = take(group ? (size_t)Bq * p.ngroups * 4 + 4 : 0);
  p.off_rng = take(range ? (size_t)Bq * 12 : 0);
  p.off_sure = take(range ? (size_t)Bq * p.nstreams * 4 : 0);
  p.bytes = o;
  return p;
}

// One call of the wide family, as the entry points hand it to the launchers. grp: the distinct route's group ids (GROUP); rlab / qlab / ne:
// the row labels, query labels and COR_FILTER_NE of the filtered route (FILTER); null / 0 where the route has none.
struct WideCall {
  const float* Q; int Bq, Ng, C, k; long long g_offset;
  const int* grp; const int* rlab; const int* qlab; int ne;
  float* out_s; long long* out_i; char* w; int flags; hipStream_t s;
  const float* gscale;                               // the int8 route: the gallery rows' scales
  const float* thr; int* out_count;                  // the range call: the floors and the member counts
};

// tau_q from the sample values. GROUP: reduced to one value per group first (sim_tau_distinct, with the rows behind the values).
template <typename TG, bool GROUP, bool RANGE = false>
int launch_wide_tau(const WideCall& c, const WidePlan& p) {
  const unsigned* sg = (const unsigned*)(c.w + p.off_sg); float* tau = (float*)(c.w + p.off_tau);
  if constexpr (GROUP)
    hipLaunchKernelGGL((sim_tau_distinct<TG>), dim3(c.Bq), dim3(256), 0, c.s, c.Q, c.C, sg, (const int*)(c.w + p.off_sgrow), p.ngroups, c.k, c.grp, tau);
  else
    hipLaunchKernelGGL((sim_tau_wide<TG>), dim3(c.Bq), dim3(256), 0, c.s, c.Q, c.C, sg, p.ngroups, c.k, tau);
  COR_CHECK_LAUNCH();
  if constexpr (RANGE) {                               // the floors beside tau_q: A_q, B_q, H_q
    float* rng = (float*)(c.w + p.off_rng);
    hipLaunchKernelGGL((sim_range_bounds<TG>), dim3(c.Bq), dim3(256), 0, c.s, c.Q, c.C, c.thr, tau, rng, rng + c.Bq, rng + 2 * (size_t)c.Bq);
    COR_CHECK_LAUNCH();
  }
  return 0;
}

// the selection over the APPEND pass's streams: records (scan form) or entry lists (tile form). GROUP: one row per group (sim_final_distinct).
template <typename TG, bool RECORDS, bool FILTER, bool GROUP, bool RANGE = false>
int launch_wide_final(const TG* G, const WideCall& c, const WidePlan& p) {
  static DevOnce once;
  const float* tau = (const float*)(c.w + p.off_tau); const int* cnt = (const int*)(c.w + p.off_cnt);
  const float* rec_s = RECORDS ? (const float*)(c.w + p.off_recs) : nullptr; const int* rec_g = RECORDS ? (const int*)(c.w + p.off_recg) : nullptr;
  const uint2* lst = RECORDS ? nullptr : (const uint2*)(c.w + p.off_recs);
  const int no_fallback = (c.flags & COR_TOPK_NO_FALLBACK) ? 1 : 0;
  if constexpr (RANGE) {
    const float* rng = (const float*)(c.w + p.off_rng);
    const RangeFinal r{c.thr, rng, rng + c.Bq, rng + 2 * (size_t)c.Bq, (const int*)(c.w + p.off_sure), c.out_count, c.rlab, c.qlab, c.ne};
    cor_max_dyn_lds((const void*)sim_final_range<TG, RECORDS, FILTER>, (int)FINAL_RANGE_LDS, once);
    hipLaunchKernelGGL((sim_final_range<TG, RECORDS, FILTER>), dim3(c.Bq), dim3(256), FINAL_RANGE_LDS, c.s, c.Q, G, c.Ng, c.C, c.k, c.g_offset, cnt,
                       p.nstreams, p.cap, rec_s, rec_g, lst, c.out_s, c.out_i, no_fallback, r);
  } else if constexpr (GROUP) {
    cor_max_dyn_lds((const void*)sim_final_distinct<TG, RECORDS>, (int)FINAL_DISTINCT_LDS, once);
    hipLaunchKernelGGL((sim_final_distinct<TG, RECORDS>), dim3(c.Bq), dim3(256), FINAL_DISTINCT_LDS, c.s, c.Q, G, c.Ng, c.C, c.k, c.g_offset, tau, cnt,
                       p.nstreams, p.cap, rec_s, rec_g, lst, c.grp, c.out_s, c.out_i, no_fallback, c.rlab, c.qlab, c.ne);
  } else {
    cor_max_dyn_lds((const void*)sim_final_wide<TG, RECORDS, FILTER>, (int)FINAL_WIDE_LDS, once);
    hipLaunchKernelGGL((sim_final_wide<TG, RECORDS, FILTER>), dim3(c.Bq), dim3(256), FINAL_WIDE_LDS, c.s, c.Q, G, c.Ng, c.C, c.k, c.g_offset, tau, cnt,
                       p.nstreams, p.cap, rec_s, rec_g, lst, c.out_s, c.out_i, no_fallback, c.rlab, c.qlab, c.ne);
  }
  COR_CHECK_LAUNCH();
  return 0;
}

// The scan form (16-bit, C = 256): sim_prep, SAMPLE, tau, APPEND, selection. GROUP changes the sample (it keeps the rows, sgrow), the
// threshold and the selection; the APPEND scan is the wide / filtered instantiation unchanged (it appends scores >= tau_q whatever the
// groups are).
// RANGE: the APPEND scan takes B_q for tau_q, counts and keeps the band (sim_scan RANGE); the selection is sim_final_range.
template <typename TG, int QB, bool FILTER, bool GROUP, bool RANGE = false>
int launch_wide_scan(const TG* G, const WideCall& c, const WidePlan& p) {
  constexpr size_t lds = (size_t)SCAN_NS * 64 * 256 * 2;
  static DevOnce once_s, once_a;
  cor_max_dyn_lds((const void*)sim_scan<TG, QB, true, true, FILTER, GROUP>, (int)lds, once_s);
  cor_max_dyn_lds((const void*)sim_scan<TG, QB, false, true, FILTER, false, RANGE>, (int)lds, once_a);
  unsigned* sg = (unsigned*)(c.w + p.off_sg);
  uint4* qimg = (uint4*)(c.w + p.off_img);
  const int Bqp = p.nqg * 256 * QB;
  hipLaunchKernelGGL((sim_prep<TG>), dim3(p.nqg * 8 * QB), dim3(256), 0, c.s, c.Q, c.Bq, qimg, (int*)(c.w + p.off_flags), (int*)(c.w + p.off_ovf), sg,
                     Bqp, (float*)(c.w + p.off_dq));
  COR_CHECK_LAUNCH();
  ScanArgs a{};
  a.Bq = c.Bq; a.Ng = c.Ng; a.nqg = p.nqg; a.qimg = qimg; a.sg = sg; a.Bqp = p.ngroups;
  if constexpr (GROUP) a.sgrow = (int*)(c.w + p.off_sgrow);
  a.rlab = c.rlab; a.qlab = c.qlab; a.ne = c.ne;
  if (p.ngroups > 0) {
    a.nsplit = p.s_nsplit; a.tiles_per_split = p.s_tiles_per_split; a.ntiles = p.s_tiles; a.tile_stride = p.s_stride;
    hipLaunchKernelGGL((sim_scan<TG, QB, true, true, FILTER, GROUP>), dim3(p.nqg * p.s_nsplit), dim3(512), lds, c.s, G, a);
    COR_CHECK_LAUNCH();
  }
  if (const int e = launch_wide_tau<TG, GROUP, RANGE>(c, p)) return e;
  a.nsplit = p.nsplit; a.tiles_per_split = p.tiles_per_split; a.ntiles = p.ntiles; a.tile_stride = 1;
  a.k = c.k; a.tau = (float*)(c.w + p.off_tau); a.cnt = (int*)(c.w + p.off_cnt); a.rec_s = (float*)(c.w + p.off_recs);
  a.rec_g = (int*)(c.w + p.off_recg); a.cap = p.cap; a.tau_add = 0.f;
  if constexpr (RANGE) {
    float* rng = (float*)(c.w + p.off_rng);
    a.rng_a = rng; a.tau = rng + c.Bq; a.rng_h = rng + 2 * (size_t)c.Bq; a.sure = (int*)(c.w + p.off_sure);
  }
  hipLaunchKernelGGL((sim_scan<TG, QB, false, true, FILTER, false, RANGE>), dim3(p.nqg * p.nsplit), dim3(512), lds, c.s, G, a);
  COR_CHECK_LAUNCH();
  return launch_wide_final<TG, true, FILTER, GROUP, RANGE>(G, c, p);
}

// the tile form (fp32, or C != 256): the same steps on sim_wide_scan and its entry lists, without a query image
template <typename TG, bool FILTER, bool GROUP, bool RANGE = false>
int launch_wide_tiles(const TG* G, const WideCall& c, const WidePlan& p) {
  WideScanArgs a{};
  a.Bq = c.Bq; a.Ng = c.Ng; a.C = c.C; a.nqt = p.nqt; a.sg = (unsigned*)(c.w + p.off_sg); a.ngroups = p.ngroups;
  if constexpr (GROUP) a.sgrow = (int*)(c.w + p.off_sgrow);
  a.rlab = c.rlab; a.qlab = c.qlab; a.ne = c.ne;
  if (p.ngroups > 0) {
    a.nsplit = p.s_nsplit; a.tiles_per_split = p.s_tiles_per_split; a.ntiles = p.s_tiles; a.tile_stride = p.s_stride;
    hipLaunchKernelGGL((sim_wide_scan<TG, true, FILTER, GROUP>), dim3(cdiv((long)p.nqt * p.s_nsplit, 4)), dim3(256), 0, c.s, c.Q, G, a);
    COR_CHECK_LAUNCH();
  }
  if (const int e = launch_wide_tau<TG, GROUP, RANGE>(c, p)) return e;
  a.nsplit = p.nsplit; a.tiles_per_split = p.tiles_per_split; a.ntiles = p.ntiles; a.tile_stride = 1;
  a.tau = (float*)(c.w + p.off_tau); a.cnt = (int*)(c.w + p.off_cnt); a.lst = (uint2*)(c.w + p.off_recs); a.cap = p.cap;
  if constexpr (RANGE) {
    float* rng = (float*)(c.w + p.off_rng);
    a.rng_a = rng; a.tau = rng + c.Bq; a.rng_h = rng + 2 * (size_t)c.Bq; a.sure = (int*)(c.w + p.off_sure);
  }
  hipLaunchKernelGGL((sim_wide_scan<TG, false, FILTER, false, RANGE>), dim3(cdiv((long)p.nqt * p.nsplit, 4)), dim3(256), 0, c.s, c.Q, G, a);
  COR_CHECK_LAUNCH();
  return launch_wide_final<TG, false, FILTER, GROUP, RANGE>(G, c, p);
}

// The three routes of the wide family: wide (33 <= k <= COR_TOPK_KMAX), filtered (FILTER, every k) and distinct groups (GROUP, every k,
// with or without a filter). 16-bit galleries with C = 256 take the scan form, everything else the tile form.
template <bool FILTER, bool GROUP, typename TG>
int launch_wide(const TG* G, const WideCall& c) {
  if constexpr (sizeof(TG) == 2) {
    if (c.C == 256) {
      const WidePlan p = make_wide(c.Bq, c.Ng, c.k, true, FILTER, GROUP);
      if (p.qb == 2) return launch_wide_scan<TG, 2, FILTER, GROUP>(G, c, p);
      return launch_wide_scan<TG, 1, FILTER, GROUP>(G, c, p);
    }
  }
  return launch_wide_tiles<TG, FILTER, GROUP>(G, c, make_wide(c.Bq, c.Ng, c.k, false, FILTER, GROUP));
}
// cor_similarity_range: the wide route's two forms with the RANGE scan and selection, for every k. FILTER: cor_similarity_range_filtered,
// the filtered plan and sample with the RANGE scan behind the label mask.
template <bool FILTER, typename TG>
int launch_range(const TG* G, const WideCall& c) {
  if constexpr (sizeof(TG) == 2) {
    if (c.C == 256) {
      const WidePlan p = make_wide(c.Bq, c.Ng, c.k, true, FILTER, false, false, true);
      if constexpr (!FILTER)                           // (the filtered range plan has qb = 1 for every Bq)
        if (p.qb == 2) return launch_wide_scan<TG, 2, false, false, true>(G, c, p);
      return launch_wide_scan<TG, 1, FILTER, false, true>(G, c, p);
    }
  }
  return launch_wide_tiles<TG, FILTER, false, true>(G, c, make_wide(c.Bq, c.Ng, c.k, false, FILTER, false, false, true));
}

template <typename TG>
int launch_topk(const float* Q, const TG* G, int Bq, int Ng, int C, int k, long long g_offset, float* out_s, long long* out_i,
                void* workspace, int flags, hipStream_t s) {
  if (k > 32)                                          // 33 <= k <= COR_TOPK_KMAX
    return launch_wide<false, false>(G, WideCall{Q, Bq, Ng, C, k, g_offset, nullptr, nullptr, nullptr, 0, out_s, out_i, (char*)workspace, flags, s});
  float* ws_s = (float*)workspace;
  const bool force_lists = (flags & COR_TOPK_FORCE_LISTS) != 0;
  if constexpr (sizeof(TG) == 2) {
    if (C == 256 && !force_lists && !(flags & COR_TOPK_FORCE_GLOBAL_THRESHOLD)) {   // small shards: two launches, local thresholds
      const SmallPlan sp = make_small(Bq, Ng, k);
      if (sp.ok) return launch_small<TG>(Q, G, Bq, Ng, k, g_offset, out_s, out_i, (char*)workspace, sp, flags, s);
    }
    if (C == 256 && !force_lists) {                     // threshold-and-append + exact re-scoring
      const V3Plan p = make_v3(Bq, Ng, k);
      if (p.qb == 2) return launch_v3<TG, 2>(Q, G, Bq, Ng, k, g_offset, out_s, out_i, (char*)workspace, p, flags, s);
      return launch_v3<TG, 1>(Q, G, Bq, Ng, k, g_offset, out_s, out_i, (char*)workspace, p, flags, s);
    }
    if (C == 256) return launch_lists_v2<TG>(Q, G, Bq, Ng, k, g_offset, out_s, out_i, ws_s, nullptr, nullptr, s);
  }
  const TopkPlan p = make_plan(Bq, Ng, k);
  int* ws_i = (int*)(ws_s + (long)Bq * p.nparts * p.kmax);
  const int nwaves = p.nqt * p.nsplit;
  if (p.kmax == 8) hipLaunchKernelGGL((sim_topk_partial<TG, 8>), dim3(cdiv(nwaves, 4)), dim3(256), 0, s, Q, G, Bq, Ng, C, p, ws_s, ws_i);
  else hipLaunchKernelGGL((sim_topk_partial<TG, 32>), dim3(cdiv(nwaves, 4)), dim3(256), 0, s, Q, G, Bq, Ng, C, p, ws_s, ws_i);
  COR_CHECK_LAUNCH();
  return launch_merge(ws_s, ws_i, Bq, p.nparts * p.kmax, k, g_offset, out_s, out_i, nullptr, s);
}

// ---------------------------------------------------------------------------------------------------------------------
// INT8 GALLERIES (cor_similarity_topk_i8): rows quantised per row by cor_quantize_rows_i8 (Gq int8 [Ng,C], gscale f32 [Ng]), the query
// quantised the same way inside the call. score = ((float)d * qscale) * gscale with d the int32 dot product: integer arithmetic, exact in
// any summation order, so the scan's score IS the score: delta = 0, nothing is re-scored (include/cor_amd.h has the definition). Every k
// takes the wide route's steps with the fp32 gallery's selection: sim_i8_scan<SAMPLE>, sim_tau_wide<float>, sim_i8_scan<APPEND>,
// sim_final_wide<float> on the entry lists, and for an overflowed query sim_i8_repair (brute_force_by over the int8 scores).
// cor_similarity_topk_i8_filtered takes the same steps with a label filter inside them (sim_i8_scan<.., FILTER>, sim_i8_repair_filtered).
// cor_similarity_topk_i8_distinct takes them with the distinct route's sample rows, threshold and selection (sim_i8_scan<true, .., GROUP>,
// sim_tau_distinct<float>, sim_final_distinct<float>, sim_i8_repair_distinct), with or without the filter.
//
// sim_i8_scan: v_mfma_i32_16x16x64_i8, gallery rows as the A operand, queries as B. A block is 8 waves; wave w keeps the fragments of ITS 64
// queries (4 column blocks x C/64 K steps x 16 B per lane = 64 VGPRs at C = 256) for the whole slice, and all 8 waves share every 64-row
// gallery tile through LDS: 512 queries read the gallery from memory once. Lane (c = lane & 15, rq = lane >> 4) supplies bytes
// [64 ks + 16 rq, +16) of gallery row / query c to K step ks; the K order inside the instruction does not matter as long as both operands
// use the same one, and the C/D map is the dtype-independent one: lane holds column c (the query), rows 4 rq + reg (the gallery rows).
// So lane quarter rq of slice `split` is the private stream split * 4 + rq of each of the lane's four queries: no atomics.
// Tiles are double-buffered in LDS (global -> registers during the previous tile's MFMAs -> LDS, one barrier per tile), the 64 row scales
// with them: the tile loop issues no global load but the prefetch, so nothing waits behind it on the in-order load counter. LDS image of a
// tile: row r at r * stride 16-B slots, chunk ch at slot ch ^ (r & 15) for C = 256 (stride 16: the four 16-lane groups of a ds_read_b128
// see 16 different slots) and at slot ch with an odd stride (C / 16) | 1 otherwise (consecutive rows start one slot apart).
// Edges: rows >= Ng score -inf (their bytes are read as zero, never from beyond the gallery), padding queries (q >= Bq) carry tau = +inf
// and never append, chunks beyond C (C % 64 != 0) are zero in both fragments.
typedef int i32x4 __attribute__((ext_vector_type(4)));
struct I8ScanArgs {
  const signed char* qq; const float* qscale; const float* gscale;
  int Bq, Ng, C, nqg, nsplit, tiles_per_split, ntiles, tile_stride;
  unsigned* sg; int ngroups;
  const float* tau; int* cnt; uint2* lst; int cap;
  const int* rlab; const int* qlab; int ne;          // FILTER: row / query labels, COR_FILTER_NE
  int* sgrow;                                        // GROUP SAMPLE: the shard row behind every stored sample value
};
constexpr int I8_TILE_SLOTS = 64 * 17;                 // 64 rows x the largest stride
// FULL: C = 256, every chunk and K step present (no tail tests in the loop). APPEND tests a cheap upper bound first: rounding is monotone and
// qscale, gscale >= 0, so ((float)max(d_0..d_3, 0) * qscale) * max(gscale_0..3) is >= each of the lane's four scores of a query; only
// where some lane's bound reaches tau_q are the four scores formed and compared (a few rows in 10^4 pass tau_q).
// FILTER (cor_similarity_topk_i8_filtered): the tile's 64 row labels travel with its scales (threads 16..31 fetch them, four each, into the
// same prefetch register; tile_gs[.][16 + i] holds labels 4 i .. 4 i + 3, 0 beyond Ng where the row test already masks), each lane keeps the
// labels of its four queries, and a disallowed score is -inf: never among a group's best, never appended. The bound test needs no label
// (it is >= every score of the four rows, allowed or not). SAMPLE keeps the group's four best allowed scores (Best4's insertion;
// sg[q * ngroups + stream * 4 + j], ngroups counts the four), and slice `split` walks the tiles split, split + nsplit, ...: the allowed rows
// of a class-sorted gallery spread over every stream and every sample group.
// GROUP (cor_similarity_topk_i8_distinct, SAMPLE only): every stored sample value travels with the ROW that produced it (a.sgrow, parallel
// to sg): the lane-quarter group's maximum and its row, with FILTER its four best allowed scores and their rows through one insertion
// network (BestRows's, written out here with Best4's: the structs cost these instantiations a VGPR). Invariant: every sgrow entry written is a row in [0, Ng): a row is kept only behind `gr + e < Ng` (the ragged
// last tile's rows beyond Ng never are), and a slot that no score reached holds (-inf, row 0); sim_tau_distinct dereferences only the
// rows behind values above key(-inf).
template <bool SAMPLE, bool FULL, bool FILTER = false, bool GROUP = false>
__global__ void __launch_bounds__(512) sim_i8_scan(const signed char* __restrict__ G, const I8ScanArgs a) {
#pragma clang fp contract(off)
  __shared__ uint4 tile[2][I8_TILE_SLOTS];
  __shared__ f32x4 tile_gs[2][FILTER ? 32 : 16];       // the tile's 64 row scales (0 beyond Ng), fetched with it; FILTER: and its 64 labels
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, rq = lane >> 4;
  const int qg = blockIdx.x % a.nqg, split = blockIdx.x / a.nqg;
  const int Ng = a.Ng, C = FULL ? 256 : a.C, nch = C >> 4, nks = (C + 63) >> 6;
  const int stride = nch == 16 ? 16 : (nch | 1), xmask = nch == 16 ? 15 : 0;
  const int q0 = (qg * 8 + wave) * 64;
  const bool active = q0 < a.Bq;                       // wave-uniform: a wave without queries only helps to load
  // the lane's four queries (column block j: q0 + 16 j + c16) and their fragments
  i32x4 qf[4][4];
  float qs[4], tq[4], gmax[4];
  int n[4];
  int ql[4];                                           // FILTER: the queries' labels (< 0: unrestricted)
  float top4[4][4];                                    // FILTER SAMPLE: the group's four best allowed scores, descending
  int grow[4][GROUP && FILTER ? 4 : 1];                // GROUP SAMPLE: the rows behind gmax (FILTER: behind top4)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = q0 + 16 * j + c16;
    const signed char* qrow = a.qq + (long)min(q, a.Bq - 1) * C;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[j][ks] = i32x4{0, 0, 0, 0};
      if (active && (FULL || ks * 4 + rq < nch)) qf[j][ks] = *(const i32x4*)(qrow + ks * 64 + rq * 16);
    }
    qs[j] = active ? a.qscale[min(q, a.Bq - 1)] : 0.f;
    tq[j] = SAMPLE ? 0.f : append_threshold(active && q < a.Bq, a.tau, q);
    gmax[j] = -INFINITY;
    n[j] = 0;
    if constexpr (GROUP) {
#pragma unroll
      for (int i = 0; i < (FILTER ? 4 : 1); ++i) grow[j][i] = 0;
    }
    if constexpr (FILTER) {
      ql[j] = active ? a.qlab[min(q, a.Bq - 1)] : -1;
#pragma unroll
      for (int i = 0; i < 4; ++i) top4[j][i] = -INFINITY;
    }
  }
  const int stream = split * 4 + rq, nstreams = 4 * a.nsplit;
  // the thread's two 16-B pieces of a tile: piece i = tid + 512 p is chunk i % nch of row i / nch (a tile is contiguous in the gallery)
  const long gbytes = (long)Ng * C;
  int slot[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int i = tid + 512 * p, r = i / nch, ch = i - r * nch;
    slot[p] = r < 64 ? r * stride + (ch ^ (r & xmask)) : -1;
  }
  const SliceWalk<FILTER> walk(split, a.nsplit, a.tiles_per_split, a.ntiles);
  const int t0 = walk.t0, t1 = walk.t1;
  uint4 pre[2];
  f32x4 pre_gs = {0.f, 0.f, 0.f, 0.f};
  auto fetch = [&](int t) {
    t = walk.tile(t);
    const long base = (long)t * a.tile_stride * 64 * C;
    if (tid < 16) pre_gs = load4_or_zero<f32x4>(a.gscale, t * a.tile_stride * 64 + 4 * tid, Ng);
    else if (FILTER && tid < 32) pre_gs = load4_or_zero<f32x4>(a.rlab, t * a.tile_stride * 64 + 4 * (tid - 16), Ng);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const long off = base + 16L * (tid + 512 * p);
      pre[p] = make_uint4(0u, 0u, 0u, 0u);
      if (slot[p] >= 0 && off < gbytes) pre[p] = *(const uint4*)(G + off);
    }
  };
  if (t0 < t1) fetch(t0);
  for (int t = t0; t < t1; ++t) {
    uint4* buf = tile[(t - t0) & 1];
    const f32x4* buf_gs = tile_gs[(t - t0) & 1];
#pragma unroll
    for (int p = 0; p < 2; ++p)
      if (slot[p] >= 0) buf[slot[p]] = pre[p];
    if (tid < (FILTER ? 32 : 16)) tile_gs[(t - t0) & 1][tid] = pre_gs;
    __syncthreads();                                   // the other buffer was last read before this barrier: the next stores are safe
    if (t + 1 < t1) fetch(t + 1);
    if (!active) continue;
    const int g0 = walk.tile(t) * a.tile_stride * 64;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const int gr = g0 + 16 * sub + 4 * rq;           // the lane's rows gr .. gr + 3 of this 16-row block
      if (g0 + 16 * sub >= Ng) break;                  // block-uniform
      const f32x4 gs = buf_gs[4 * sub + rq];
      const int r = 16 * sub + c16;
      i32x4 af[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        af[ks] = i32x4{0, 0, 0, 0};
        if (FULL || ks * 4 + rq < nch) af[ks] = __builtin_bit_cast(i32x4, buf[r * stride + ((ks * 4 + rq) ^ (r & xmask))]);
      }
      i32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[0], qf[j][0], (i32x4{0, 0, 0, 0}), 0, 0, 0);
#pragma unroll
        for (int ks = 1; ks < 4; ++ks)
          if (FULL || ks < nks) acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[ks], qf[j][ks], acc[j], 0, 0, 0);
      }
      const float gsmax = fmaxf(fmaxf(gs[0], gs[1]), fmaxf(gs[2], gs[3]));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (SAMPLE && FILTER && GROUP) {
          const i32x4 lab = __builtin_bit_cast(i32x4, buf_gs[16 + 4 * sub + rq]);
          float s[4], smax = -INFINITY;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = gr + e < Ng && label_allows(lab[e], ql[j], a.ne);
            s[e] = ok ? ((float)acc[j][e] * qs[j]) * gs[e] : -INFINITY;
            smax = fmaxf(smax, s[e]);
          }
          if (__builtin_amdgcn_ballot_w64(smax > top4[j][3]) != 0) {   // (a masked score is -inf: never > a slot, its row never kept)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (s[e] > top4[j][3]) { top4[j][3] = s[e]; grow[j][3] = gr + e; }
#pragma unroll
              for (int i = 3; i > 0; --i) {
                const float s0 = top4[j][i - 1], s1 = top4[j][i];
                const int i0 = grow[j][i - 1], i1 = grow[j][i];
                const bool up = s1 > s0;
                top4[j][i - 1] = up ? s1 : s0; top4[j][i] = up ? s0 : s1;
                grow[j][i - 1] = up ? i1 : i0; grow[j][i] = up ? i0 : i1;
              }
            }
          }
        } else if constexpr (SAMPLE && GROUP) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float s = ((float)acc[j][e] * qs[j]) * gs[e];
            if (gr + e < Ng && s > gmax[j]) { gmax[j] = s; grow[j][0] = gr + e; }
          }
        } else if constexpr (SAMPLE && FILTER) {
          const i32x4 lab = __builtin_bit_cast(i32x4, buf_gs[16 + 4 * sub + rq]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = gr + e < Ng && label_allows(lab[e], ql[j], a.ne);
            const float s = ok ? ((float)acc[j][e] * qs[j]) * gs[e] : -INFINITY;
            top4[j][3] = fmaxf(top4[j][3], fminf(top4[j][2], s));
            top4[j][2] = fmaxf(top4[j][2], fminf(top4[j][1], s));
            top4[j][1] = fmaxf(top4[j][1], fminf(top4[j][0], s));
            top4[j][0] = fmaxf(top4[j][0], s);
          }
        } else if constexpr (SAMPLE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float s = ((float)acc[j][e] * qs[j]) * gs[e];
            gmax[j] = fmaxf(gmax[j], gr + e < Ng ? s : -INFINITY);
          }
        } else {
          const int dmax = max(max(max(acc[j][0], acc[j][1]), max(acc[j][2], acc[j][3])), 0);
          const float bound = ((float)dmax * qs[j]) * gsmax;
          if (__builtin_amdgcn_ballot_w64(bound >= tq[j]) != 0) {
            uint2* dst = a.lst + ((long)min(q0 + 16 * j + c16, a.Bq - 1) * nstreams + stream) * a.cap;
            i32x4 lab = {0, 0, 0, 0};
            if constexpr (FILTER) lab = __builtin_bit_cast(i32x4, buf_gs[16 + 4 * sub + rq]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float s = ((float)acc[j][e] * qs[j]) * gs[e];
              const bool ok = !FILTER || label_allows(lab[e], ql[j], a.ne);
              if (gr + e < Ng && ok && s >= tq[j]) append_entry(dst, n[j], a.cap, s, gr + e);
            }
          }
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = q0 + 16 * j + c16;
    if (q < a.Bq) {
      if constexpr (SAMPLE && GROUP) {
        if constexpr (FILTER) {
          *(uint4*)(a.sg + (long)q * a.ngroups + stream * 4) = make_uint4(f2key(top4[j][0]), f2key(top4[j][1]), f2key(top4[j][2]), f2key(top4[j][3]));
          *(i32x4*)(a.sgrow + (long)q * a.ngroups + stream * 4) = i32x4{grow[j][0], grow[j][1], grow[j][2], grow[j][3]};
        } else {
          a.sg[(long)q * a.ngroups + stream] = f2key(gmax[j]);
          a.sgrow[(long)q * a.ngroups + stream] = grow[j][0];
        }
      } else if constexpr (SAMPLE && FILTER)
        *(uint4*)(a.sg + (long)q * a.ngroups + stream * 4) = make_uint4(f2key(top4[j][0]), f2key(top4[j][1]), f2key(top4[j][2]), f2key(top4[j][3]));
      else if (SAMPLE) a.sg[(long)q * a.ngroups + stream] = f2key(gmax[j]);
      else a.cnt[(long)q * nstreams + stream] = n[j];
    }
  }
}

// Overflowed queries of the int8 route (sim_final_wide ran with the marker on: slot 0 is (-inf, -2), which no ranked query carries):
// the exact top-k by brute force over the int8 scores, one block of 256 threads per query; every other block leaves at once.
// FILTER (sim_i8_repair_filtered, a kernel of its own so that the unfiltered one stays as compiled): only the rows allowed for the query
// are ranked, and a query with at most k allowed rows gets them followed by the (-inf, -1) tail (brute_force_by<true>).
// the int8 score of gallery row g against the quantised query qv (C bytes in LDS), scale qs: the definition, one row per call
__device__ __forceinline__ float i8_score_at(const signed char* __restrict__ G, const float* __restrict__ gscale, const uint4* qv, float qs, int C,
                                             int g) {
#pragma clang fp contract(off)
  const uint4* row = (const uint4*)(G + (long)g * C);
  int d = 0;
  for (int c = 0; c < C / 16; ++c) {
    const uint4 x = row[c], y = qv[c];
    const unsigned xw[4] = {x.x, x.y, x.z, x.w}, yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int b = 0; b < 4; ++b) d += (int)(signed char)(xw[i] >> (8 * b)) * (int)(signed char)(yw[i] >> (8 * b));
  }
  return ((float)d * qs) * gscale[g];
}
template <bool FILTER>
__device__ __forceinline__ void i8_repair_body(const signed char* __restrict__ qq, const float* __restrict__ qscale,
                                               const signed char* __restrict__ G, const float* __restrict__ gscale, int Ng, int C, int k,
                                               long long g_offset, float* out_s, long long* out_i, const int* __restrict__ rlab,
                                               const int* __restrict__ qlab, int ne) {
#pragma clang fp contract(off)
  __shared__ float sl_s[COR_TOPK_KMAX];
  __shared__ int sl_i[COR_TOPK_KMAX], hist[256];
  __shared__ unsigned long long keys[COR_TOPK_KMAX];
  __shared__ uint4 qv[16];
  const int q = blockIdx.x, tid = threadIdx.x;
  if (out_i[(long)q * k] != -2LL) return;              // block-uniform: read before any thread of the block writes
  if (tid < C / 16) qv[tid] = *(const uint4*)(qq + (long)q * C + 16 * tid);
  __syncthreads();
  const float qs = qscale[q];
  auto score_at = [&](int g) { return i8_score_at(G, gscale, qv, qs, C, g); };
  if constexpr (FILTER) {
    const int ql = qlab[q];
    brute_force_by<true>(score_at, [&](int g) { return row_allowed(rlab, g, ql, ne); }, Ng, k, g_offset, sl_s, sl_i, keys, hist,
                         out_s + (long)q * k, out_i + (long)q * k);
  } else {
    brute_force_by<false>(score_at, [](int) { return true; }, Ng, k, g_offset, sl_s, sl_i, keys, hist, out_s + (long)q * k, out_i + (long)q * k);
  }
}
__global__ void __launch_bounds__(256) sim_i8_repair(const signed char* __restrict__ qq, const float* __restrict__ qscale,
                                                     const signed char* __restrict__ G, const float* __restrict__ gscale, int Ng, int C, int k,
                                                     long long g_offset, float* out_s, long long* out_i) {
  i8_repair_body<false>(qq, qscale, G, gscale, Ng, C, k, g_offset, out_s, out_i, nullptr, nullptr, 0);
}
__global__ void __launch_bounds__(256) sim_i8_repair_filtered(const signed char* __restrict__ qq, const float* __restrict__ qscale,
                                                              const signed char* __restrict__ G, const float* __restrict__ gscale, int Ng, int C,
                                                              int k, long long g_offset, float* out_s, long long* out_i,
                                                              const int* __restrict__ rlab, const int* __restrict__ qlab, int ne) {
  i8_repair_body<true>(qq, qscale, G, gscale, Ng, C, k, g_offset, out_s, out_i, rlab, qlab, ne);
}

// Overflowed queries of the int8 distinct route (sim_final_distinct<float> ran with the marker on): the paging fallback of the distinct
// route (distinct_brute_force_by) over the int8 scores of the allowed rows; rlab == nullptr: unfiltered. One block of 256 threads per
// query, every other block leaves at once. Static LDS: sl_s / sl_i / flag [SLW] 24 KiB, keys and k2 [SLW] 32 KiB, the found-group table
// and the histogram 1 KiB each, the query 256 B: 58.3 KiB.
__global__ void __launch_bounds__(256) sim_i8_repair_distinct(const signed char* __restrict__ qq, const float* __restrict__ qscale,
                                                              const signed char* __restrict__ G, const float* __restrict__ gscale, int Ng, int C,
                                                              int k, long long g_offset, const int* __restrict__ grp, float* out_s, long long* out_i,
                                                              const int* __restrict__ rlab, const int* __restrict__ qlab, int ne) {
#pragma clang fp contract(off)
  __shared__ float sl_s[SLW];
  __shared__ int sl_i[SLW], flag[SLW], hist[256];
  __shared__ unsigned long long keys[SLW], k2[SLW];
  __shared__ unsigned found[COR_TOPK_KMAX];
  __shared__ uint4 qv[16];
  const int q = blockIdx.x, tid = threadIdx.x;
  if (out_i[(long)q * k] != -2LL) return;              // block-uniform: read before any thread of the block writes
  if (tid < C / 16) qv[tid] = *(const uint4*)(qq + (long)q * C + 16 * tid);
  __syncthreads();
  const float qs = qscale[q];
  const int ql = rlab ? qlab[q] : -1;
  distinct_brute_force_by([&](int g) { return i8_score_at(G, gscale, qv, qs, C, g); },
                          [&](int g) { return row_allowed(rlab, g, ql, ne); }, Ng, k, g_offset, grp, sl_s, sl_i, flag, keys, k2, found,
                          hist, out_s + (long)q * k, out_i + (long)q * k);
}

// FILTER: cor_similarity_topk_i8_filtered, the same steps with the filter inside them (c.rlab / c.qlab / c.ne).
// GROUP: cor_similarity_topk_i8_distinct (c.grp): the distinct route's three changes. The SAMPLE scan keeps the rows behind its values
// (sgrow), tau_q is sim_tau_distinct<float> (delta = 0), the APPEND scan is the unchanged <false, FULL, FILTER> instantiation (it appends
// scores >= tau_q whatever the groups are), the selection is sim_final_distinct<float> over the entry lists (delta = 0: nothing is
// re-scored, G is never dereferenced) and marked queries go to sim_i8_repair_distinct.
template <bool FILTER, bool GROUP = false>
int launch_topk_i8(const signed char* Gq, const WideCall& c) {
  const WidePlan p = make_wide(c.Bq, c.Ng, c.k, true, FILTER, GROUP, true);
  signed char* qq = (signed char*)(c.w + p.off_img); float* qscale = (float*)(c.w + p.off_dq);
  if (const int e = cor_quantize_rows_i8(c.Q, COR_F32, c.Bq, c.C, qq, qscale, c.s)) return e;
  I8ScanArgs a{};
  a.qq = qq; a.qscale = qscale; a.gscale = c.gscale; a.Bq = c.Bq; a.Ng = c.Ng; a.C = c.C; a.nqg = p.nqg;
  a.sg = (unsigned*)(c.w + p.off_sg); a.ngroups = p.ngroups;
  a.rlab = c.rlab; a.qlab = c.qlab; a.ne = c.ne;
  if (p.ngroups > 0) {
    a.nsplit = p.s_nsplit; a.tiles_per_split = p.s_tiles_per_split; a.ntiles = p.s_tiles; a.tile_stride = p.s_stride;
    if constexpr (GROUP) a.sgrow = (int*)(c.w + p.off_sgrow);
    if (c.C == 256) hipLaunchKernelGGL((sim_i8_scan<true, true, FILTER, GROUP>), dim3(p.nqg * p.s_nsplit), dim3(512), 0, c.s, Gq, a);
    else hipLaunchKernelGGL((sim_i8_scan<true, false, FILTER, GROUP>), dim3(p.nqg * p.s_nsplit), dim3(512), 0, c.s, Gq, a);
    COR_CHECK_LAUNCH();
  }
  if (const int e = launch_wide_tau<float, GROUP>(c, p)) return e;
  a.nsplit = p.nsplit; a.tiles_per_split = p.tiles_per_split; a.ntiles = p.ntiles; a.tile_stride = 1;
  a.tau = (const float*)(c.w + p.off_tau); a.cnt = (int*)(c.w + p.off_cnt); a.lst = (uint2*)(c.w + p.off_recs); a.cap = p.cap;
  if (c.C == 256) hipLaunchKernelGGL((sim_i8_scan<false, true, FILTER>), dim3(p.nqg * p.nsplit), dim3(512), 0, c.s, Gq, a);
  else hipLaunchKernelGGL((sim_i8_scan<false, false, FILTER>), dim3(p.nqg * p.nsplit), dim3(512), 0, c.s, Gq, a);
  COR_CHECK_LAUNCH();
  // the fp32 gallery's selection over the entry lists (allowed rows only with FILTER); an overflow leaves the marker and never touches
  // the (absent) float rows
  WideCall sel = c;
  sel.flags |= COR_TOPK_NO_FALLBACK;
  if (const int e = launch_wide_final<float, false, false, GROUP>((const float*)nullptr, sel, p)) return e;
  if (!(c.flags & COR_TOPK_NO_FALLBACK)) {
    if constexpr (GROUP)
      hipLaunchKernelGGL(sim_i8_repair_distinct, dim3(c.Bq), dim3(256), 0, c.s, qq, qscale, Gq, c.gscale, c.Ng, c.C, c.k, c.g_offset, c.grp, c.out_s,
                         c.out_i, c.rlab, c.qlab, c.ne);
    else if constexpr (FILTER)
      hipLaunchKernelGGL(sim_i8_repair_filtered, dim3(c.Bq), dim3(256), 0, c.s, qq, qscale, Gq, c.gscale, c.Ng, c.C, c.k, c.g_offset, c.out_s, c.out_i,
                         c.rlab, c.qlab, c.ne);
    else
      hipLaunchKernelGGL(sim_i8_repair, dim3(c.Bq), dim3(256), 0, c.s, qq, qscale, Gq, c.gscale, c.Ng, c.C, c.k, c.g_offset, c.out_s, c.out_i);
    COR_CHECK_LAUNCH();
  }
  return 0;
}

// the largest value of a plan field over the two forms of a route (the gallery's dtype and C choose the form at call time)
template <typename T>
long wide_max(int Bq, int Ng, int k, bool filter, bool group, T WidePlan::*field) {
  const long a = (long)(make_wide(Bq, Ng, k, true, filter, group).*field), b = (long)(make_wide(Bq, Ng, k, false, filter, group).*field);
  return a > b ? a : b;
}
inline long wide_bytes(int Bq, int Ng, int k, bool filter, bool group) { return wide_max(Bq, Ng, k, filter, group, &WidePlan::bytes); }
// the most sample values per query any plan of a distinct call hands sim_tau_distinct
inline int distinct_sample_values(int Bq, int Ng, int k) {
  return (int)std::max(wide_max(Bq, Ng, k, false, true, &WidePlan::ngroups), wide_max(Bq, Ng, k, true, true, &WidePlan::ngroups));
}
// the same for an int8 distinct call (one form; the filtered plan has the most)
inline int i8_distinct_sample_values(int Bq, int Ng, int k) {
  return std::max(make_wide(Bq, Ng, k, true, false, true, true).ngroups, make_wide(Bq, Ng, k, true, true, true, true).ngroups);
}
// Its workspace. A plan depends on Bq through the number of 512-query groups only (more groups: fewer slices, fewer streams), and within
// one group count every buffer grows with Bq; the maximum over the smaller group counts makes the size monotone in Bq, so a workspace
// sized for the largest batch serves every smaller one. Beyond device_cus() groups every plan has one slice: nothing more to look at.
inline long i8_distinct_bytes(int Bq, int Ng, int k) {
  auto at = [&](int b) { return (long)std::max(make_wide(b, Ng, k, true, false, true, true).bytes, make_wide(b, Ng, k, true, true, true, true).bytes); };
  long m = at(Bq);
  const int top = std::min(cdiv(Bq, 512) - 1, device_cus() + 1);
  for (int g = 1; g <= top; ++g) m = std::max(m, at(512 * g));
  return m;
}
inline bool topk_shape_ok(int Bq, int Ng, int k) { return Bq > 0 && Ng > 0 && k > 0 && k <= COR_TOPK_KMAX; }

constexpr int K32_ONLY_FLAGS = COR_TOPK_FORCE_LISTS | COR_TOPK_WAVE_FINAL;   // the register-list / one-wave kernels: k <= 32, never the wide family
enum Route { ROUTE_TOPK, ROUTE_FILTERED, ROUTE_DISTINCT, ROUTE_I8, ROUTE_I8_FILTERED, ROUTE_I8_DISTINCT, ROUTE_RANGE, ROUTE_RANGE_FILTERED };

// The argument checks of the search entry points, in the order (and with the codes) of the ABI. What differs by route: the
// pointers it needs (filtered: both label vectors; distinct: the group ids, and the labels both or neither; int8: the row scales, and
// filtered int8 both label vectors as well, distinct int8 the group ids and the labels both or neither), the A/B flags it refuses
// (the plain call only at k > 32) and the distinct routes' sample bound.
int check_topk_call(Route route, const WideCall& c, const void* G, int filter_mode) {
  const bool own_ptrs = route == ROUTE_TOPK       ? true
                        : route == ROUTE_RANGE    ? c.thr && c.out_count
                        : route == ROUTE_RANGE_FILTERED ? c.thr && c.out_count && c.rlab && c.qlab
                        : route == ROUTE_I8       ? c.gscale != nullptr
                        : route == ROUTE_I8_FILTERED ? c.gscale && c.rlab && c.qlab
                        : route == ROUTE_I8_DISTINCT ? c.gscale && c.grp && (c.rlab == nullptr) == (c.qlab == nullptr)
                        : route == ROUTE_FILTERED ? c.rlab && c.qlab
                                                  : c.grp && (c.rlab == nullptr) == (c.qlab == nullptr);
  if (!c.Q || !G || !own_ptrs || !c.out_s || !c.out_i || !c.w || c.Bq <= 0 || c.Ng <= 0 || c.k <= 0) return COR_EINVAL;
  if (filter_mode != COR_FILTER_EQ && filter_mode != COR_FILTER_NE) return COR_EINVAL;
  if (c.k > COR_TOPK_KMAX || c.C > 256 || (c.C & 15)) return COR_ENOSUPPORT;
  if ((route != ROUTE_TOPK || c.k > 32) && (c.flags & K32_ONLY_FLAGS)) return COR_ENOSUPPORT;
  if ((route == ROUTE_I8 || route == ROUTE_I8_FILTERED || route == ROUTE_I8_DISTINCT || route == ROUTE_RANGE || route == ROUTE_RANGE_FILTERED) &&
      (c.flags & ~COR_TOPK_NO_FALLBACK))
    return COR_ENOSUPPORT;                             // one route: no A/B partner
  if (route == ROUTE_DISTINCT && distinct_sample_values(c.Bq, c.Ng, c.k) > TAU_DISTINCT_MAX) return COR_ENOSUPPORT;   // (the plan keeps it: sim_tau_distinct's LDS sort)
  if (route == ROUTE_I8_DISTINCT && i8_distinct_sample_values(c.Bq, c.Ng, c.k) > TAU_DISTINCT_MAX) return COR_ENOSUPPORT;
  if ((((uintptr_t)c.Q | (uintptr_t)G | (uintptr_t)c.grp | (uintptr_t)c.rlab | (uintptr_t)c.gscale) & 15) || ((uintptr_t)c.w & 255)) return COR_EINVAL;
  return 0;
}

// f(typed gallery pointer) for the gallery's dtype
template <typename F>
int by_dtype(int g_dtype, const void* G, F f) {
  switch (g_dtype) {
    case COR_F32: return f((const float*)G);
    case COR_BF16: return f((const bf16_t*)G);
    case COR_F16: return f((const _Float16*)G);
    default: return COR_ENOSUPPORT;
  }
}
}  // namespace

extern "C" long cor_topk_workspace_bytes(int Bq, int Ng, int k) {
  if (!topk_shape_ok(Bq, Ng, k)) return COR_EINVAL;
  if (k > 32) return wide_bytes(Bq, Ng, k, false, false);   // the wide route: whichever form the gallery's dtype and C select
  const TopkPlan p = make_plan(Bq, Ng, k);
  const TopkPlan2 p2 = make_plan2(Bq, Ng, k, device_cus());
  const long a = (long)Bq * p.nparts * p.kmax * 8, b = (long)Bq * p2.nparts * p2.kmax * 8;
  long m = a > b ? a : b;
  const long c = (long)make_v3(Bq, Ng, k).bytes;
  if (c > m) m = c;
  const long d = (long)make_small(Bq, Ng, k).bytes;
  return d > m ? d : m;
}

extern "C" int cor_similarity_topk(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, int k, long long g_offset,
                                   float* out_scores, long long* out_idx, void* workspace, int flags, void* stream) {
  const WideCall c{Q, Bq, Ng, C, k, g_offset, nullptr, nullptr, nullptr, 0, out_scores, out_idx, (char*)workspace, flags, (hipStream_t)stream};
  if (const int e = check_topk_call(ROUTE_TOPK, c, G, COR_FILTER_EQ)) return e;
  return by_dtype(g_dtype, G, [&](auto* g) { return launch_topk(Q, g, Bq, Ng, C, k, g_offset, out_scores, out_idx, workspace, flags, c.s); });
}

extern "C" long cor_range_workspace_bytes(int Bq, int Ng, int k) {
  if (!topk_shape_ok(Bq, Ng, k)) return COR_EINVAL;
  return (long)std::max(make_wide(Bq, Ng, k, true, false, false, false, true).bytes, make_wide(Bq, Ng, k, false, false, false, false, true).bytes);
}

// range calls always take the wide route (every k): rows at or above a per-query floor, and how many there are (include/cor_amd.h)
extern "C" int cor_similarity_range(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, const float* thresholds, int k,
                                    long long g_offset, float* out_scores, long long* out_idx, int* out_count, void* workspace, int flags,
                                    void* stream) {
  const WideCall c{Q, Bq, Ng, C, k, g_offset, nullptr, nullptr, nullptr, 0, out_scores, out_idx, (char*)workspace, flags, (hipStream_t)stream, nullptr,
                   thresholds, out_count};
  if (const int e = check_topk_call(ROUTE_RANGE, c, G, COR_FILTER_EQ)) return e;
  return by_dtype(g_dtype, G, [&](auto* g) { return launch_range<false>(g, c); });
}

extern "C" long cor_range_filtered_workspace_bytes(int Bq, int Ng, int k) {
  if (!topk_shape_ok(Bq, Ng, k)) return COR_EINVAL;
  // (the scan form's plan has qb = 1 where the filtered top-k's has 2, so fewer slices and streams: not below that call's size all the same)
  return std::max(wide_bytes(Bq, Ng, k, true, false), (long)std::max(make_wide(Bq, Ng, k, true, true, false, false, true).bytes,
                                                                     make_wide(Bq, Ng, k, false, true, false, false, true).bytes));
}

// filtered range calls: the range route with the filter inside its sample, scan and fallback (launch_range<true>)
extern "C" int cor_similarity_range_filtered(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, const float* thresholds, int k,
                                             long long g_offset, const int* row_labels, const int* query_labels, int filter_mode,
                                             float* out_scores, long long* out_idx, int* out_count, void* workspace, int flags, void* stream) {
  const WideCall c{Q, Bq, Ng, C, k, g_offset, nullptr, row_labels, query_labels, filter_mode == COR_FILTER_NE ? 1 : 0, out_scores, out_idx,
                   (char*)workspace, flags, (hipStream_t)stream, nullptr, thresholds, out_count};
  if (const int e = check_topk_call(ROUTE_RANGE_FILTERED, c, G, filter_mode)) return e;
  return by_dtype(g_dtype, G, [&](auto* g) { return launch_range<true>(g, c); });
}

extern "C" long cor_topk_filtered_workspace_bytes(int Bq, int Ng, int k) {
  return topk_shape_ok(Bq, Ng, k) ? wide_bytes(Bq, Ng, k, true, false) : COR_EINVAL;
}

// filtered calls always take the wide route (every k)
extern "C" int cor_similarity_topk_filtered(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, int k, long long g_offset,
                                            const int* row_labels, const int* query_labels, int filter_mode, float* out_scores,
                                            long long* out_idx, void* workspace, int flags, void* stream) {
  const WideCall c{Q, Bq, Ng, C, k, g_offset, nullptr, row_labels, query_labels, filter_mode == COR_FILTER_NE ? 1 : 0, out_scores, out_idx,
                   (char*)workspace, flags, (hipStream_t)stream};
  if (const int e = check_topk_call(ROUTE_FILTERED, c, G, filter_mode)) return e;
  return by_dtype(g_dtype, G, [&](auto* g) { return launch_wide<true, false>(g, c); });
}

extern "C" long cor_topk_distinct_workspace_bytes(int Bq, int Ng, int k) {
  return topk_shape_ok(Bq, Ng, k) ? std::max(wide_bytes(Bq, Ng, k, false, true), wide_bytes(Bq, Ng, k, true, true)) : COR_EINVAL;
}

extern "C" int cor_topk_distinct_sample_values(int Bq, int Ng, int k) {
  return topk_shape_ok(Bq, Ng, k) ? distinct_sample_values(Bq, Ng, k) : COR_EINVAL;
}

// distinct calls always take the wide route (every k); the labels are optional: both or neither
extern "C" int cor_similarity_topk_distinct(const float* Q, const void* G, int g_dtype, int Bq, int Ng, int C, int k, long long g_offset,
                                            const int* row_groups, const int* row_labels, const int* query_labels, int filter_mode,
                                            float* out_scores, long long* out_idx, void* workspace, int flags, void* stream) {
  const bool filter = row_labels != nullptr;
  const WideCall c{Q, Bq, Ng, C, k, g_offset, row_groups, row_labels, query_labels, filter && filter_mode == COR_FILTER_NE ? 1 : 0, out_scores,
                   out_idx, (char*)workspace, flags, (hipStream_t)stream};
  if (const int e = check_topk_call(ROUTE_DISTINCT, c, G, filter_mode)) return e;
  return by_dtype(g_dtype, G, [&](auto* g) { return filter ? launch_wide<true, true>(g, c) : launch_wide<false, true>(g, c); });
}

extern "C" long cor_topk_i8_workspace_bytes(int Bq, int Ng, int k) {
  return topk_shape_ok(Bq, Ng, k) ? (long)make_wide(Bq, Ng, k, true, false, false, true).bytes : COR_EINVAL;
}

// int8 calls take one route for every k (launch_topk_i8)
extern "C" int cor_similarity_topk_i8(const float* Q, const signed char* Gq, const float* gscale, int Bq, int Ng, int C, int k, long long g_offset,
                                      float* out_scores, long long* out_idx, void* workspace, int flags, void* stream) {
  const WideCall c{Q, Bq, Ng, C, k, g_offset, nullptr, nullptr, nullptr, 0, out_scores, out_idx, (char*)workspace, flags, (hipStream_t)stream, gscale};
  if (const int e = check_topk_call(ROUTE_I8, c, Gq, COR_FILTER_EQ)) return e;
  return launch_topk_i8<false>(Gq, c);
}

extern "C" long cor_topk_i8_filtered_workspace_bytes(int Bq, int Ng, int k) {
  return topk_shape_ok(Bq, Ng, k) ? (long)make_wide(Bq, Ng, k, true, true, false, true).bytes : COR_EINVAL;
}

// filtered int8 calls: the int8 route with the filter inside its scans (launch_topk_i8<true>)
extern "C" int cor_similarity_topk_i8_filtered(const float* Q, const signed char* Gq, const float* gscale, int Bq, int Ng, int C, int k,
                                               long long g_offset, const int* row_labels, const int* query_labels, int filter_mode,
                                               float* out_scores, long long* out_idx, void* workspace, int flags, void* stream) {
  const WideCall c{Q, Bq, Ng, C, k, g_offset, nullptr, row_labels, query_labels, filter_mode == COR_FILTER_NE ? 1 : 0, out_scores, out_idx,
                   (char*)workspace, flags, (hipStream_t)stream, gscale};
  if (const int e = check_topk_call(ROUTE_I8_FILTERED, c, Gq, filter_mode)) return e;
  return launch_topk_i8<true>(Gq, c);
}

extern "C" long cor_topk_i8_distinct_workspace_bytes(int Bq, int Ng, int k) {
  return topk_shape_ok(Bq, Ng, k) ? i8_distinct_bytes(Bq, Ng, k) : COR_EINVAL;
}

extern "C" int cor_topk_i8_distinct_sample_values(int Bq, int Ng, int k) {
  return topk_shape_ok(Bq, Ng, k) ? i8_distinct_sample_values(Bq, Ng, k) : COR_EINVAL;
}

// distinct int8 calls: the int8 route with the distinct route's sample rows, threshold, selection and repair (launch_topk_i8<.., true>);
// the labels are optional: both or neither
extern "C" int cor_similarity_topk_i8_distinct(const float* Q, const signed char* Gq, const float* gscale, int Bq, int Ng, int C, int k,
                                               long long g_offset, const int* row_groups, const int* row_labels, const int* query_labels,
                                               int filter_mode, float* out_scores, long long* out_idx, void* workspace, int flags, void* stream) {
  const bool filter = row_labels != nullptr;
  const WideCall c{Q, Bq, Ng, C, k, g_offset, row_groups, row_labels, query_labels, filter && filter_mode == COR_FILTER_NE ? 1 : 0, out_scores,
                   out_idx, (char*)workspace, flags, (hipStream_t)stream, gscale};
  if (const int e = check_topk_call(ROUTE_I8_DISTINCT, c, Gq, filter_mode)) return e;
  return filter ? launch_topk_i8<true, true>(Gq, c) : launch_topk_i8<false, true>(Gq, c);
}
