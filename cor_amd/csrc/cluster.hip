// cor_amd — clustering of a gallery: farthest-point seeding (cor_kmeans_seed) and the centre step of spherical k-means (cor_kmeans_update).
// Contract and both definitions, fixed to the bit: include/cor_amd.h. The assignment step is the existing search and is not in this file.
//
// Rows. Both calls take the by-value segment table of segrows.h (SegRowsAssign; its row address, loaders and norm tree too) through the
// flat positions of member_sort.h (km_locate). The order of
// the flat positions: table order for the seeding (its tie rule reads the global id), ASCENDING SEGMENT OFFSET for the update, so that
// there ascending p is ascending global id. n_total < 2^31.
//
// cor_kmeans_seed: 2K launches (init, then K steps and K - 1 picks), the chosen row stays on the device (KmCur in the workspace).
//   init    best[p] = -inf, NaN at the first row (NaN marks CHOSEN: `s > NaN` and `NaN < x` are false, so a chosen row is never
//           updated and never picked); cur = the first row.
//   step t  every block widens row c_t into 1 KiB of LDS (block 0 also writes out_ids[t] and out_centroids[t]); a thread owns rows
//           p, p + grid, ...: the fmaf chain of oracle/c/sim_chain.c against the LDS row, 16 channels of loads in flight, best[p] raised,
//           and the thread's smallest (best, id) kept; wave butterfly, the block's four waves through LDS, one partial per block.
//   pick t  one block reduces the <= KM_SEED_BLOCKS partials, marks the winner chosen and writes cur for step t + 1.
//   The comparison (best by IEEE <, then the smaller global id) is a total order on the rows, so neither the grid nor the segmentation
//   changes the winner. The last step has no scoring and no pick.
// cor_kmeans_update: 6 launches.
//   keys, columns, scan, place: the member lists by the stable counting sort of member_sort.h, shared with cor_ivf_build. No atomics.
//   chunks  one WAVE per (cluster, chunk of 256 members), found by binary search in the chunk bases; segrows.h's lane layout: lane l owns
//           channels [4l, 4l + 4), a member row is ONE coalesced wave load, 64 members are looked up at a time (lane j: member j) and
//           walked in member order 8 rows at a time, all 8 loads issued before the first add. p_j = +0, then p_j = p_j + x. The members'
//           scores are summed the same way from the lane that looked the member up. Partial rows go to the workspace.
//   finish  one wave per cluster: v = +0, v = v + p_j for j ascending, the norm tree (seg_lane_norm), v / d; an empty cluster
//           copies its row of prev (or writes +0).
// Arithmetic: `#pragma clang fp contract(off)` holds for the whole file: every + * / is one separately rounded fp32 operation, the
// chain's explicit fmaf stays an fma; a / b and __builtin_sqrtf are correctly rounded (no fast-math flag for this file in the Makefile).
#include "member_sort.h"

#pragma clang fp contract(off)

namespace {

constexpr int KM_SEED_BLOCKS = 4096;           // most blocks (and partials) of a seeding step
constexpr int KM_WPB = 4;                      // waves per block of the chunk and finish kernels
constexpr unsigned KM_CHOSEN = 0x7fc00000u;    // best[] of a chosen row: a NaN

// ---------------------------------------------------------------------------------------------------------------- seeding

struct KmCur {                                 // the chosen row of the current step, in the workspace
  u64 row;
  long long id;
  float rs;
  int dt;
};
struct KmPart {                                // a block's smallest (best, id); flat < 0: the block saw no row that is not chosen
  long long id;
  float v;
  int flat;
};

// does (av, aid) come before (bv, bid)? A flat position < 0 is no entry
__device__ __forceinline__ bool km_before(float av, long long aid, int af, float bv, long long bid, int bf) {
  if (af < 0) return false;
  if (bf < 0) return true;
  if (av < bv) return true;
  if (bv < av) return false;
  return aid < bid;
}

// The seeding kernels keep their own spelling of segrows.h's seg_row and seg_load8 (here the 16-bit load is shared by bf16 and fp16).
// With seg_load8 as the header has it, and seg_row in km_set_cur, all three compiled to other code and cor_kmeans_seed measured 2.0 %
// slower at 98 304 bf16 rows, K = 8, against a parent spread of 0.2 % (profiles/row_tables_ab_shared.jsonl); with seg_row in
// km_seed_step and this loader, 2.2 % (profiles/row_tables_ab_common16.jsonl). DESIGN.md has both runs
__device__ __forceinline__ void km_load8(u64 row, int dt, float rs, int c, float (&g)[8]) {
  if (dt == COR_F32) {
    const u32x4 x = *(const SEG_GLOBAL u32x4*)(row + 32u * c), y = *(const SEG_GLOBAL u32x4*)(row + 32u * c + 16u);
#pragma unroll
    for (int e = 0; e < 4; ++e) { g[e] = __uint_as_float(x[e]); g[4 + e] = __uint_as_float(y[e]); }
  } else if (dt == COR_I8) {
    const u32x2 x = *(const SEG_GLOBAL u32x2*)(row + 8u * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = (float)(int)(signed char)(x[e >> 2] >> (8 * (e & 3))) * rs;
  } else {
    const u32x4 x = *(const SEG_GLOBAL u32x4*)(row + 16u * c);
    if (dt == COR_BF16) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { g[2 * e] = __uint_as_float(x[e] << 16); g[2 * e + 1] = __uint_as_float(x[e] & 0xffff0000u); }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = (float)__builtin_bit_cast(_Float16, (unsigned short)(e & 1 ? x[e >> 1] >> 16 : x[e >> 1] & 0xffffu));
    }
  }
}

__device__ __forceinline__ void km_set_cur(const SegRowsAssign& segs, int nseg, int C, long long p, KmCur* cur) {
  km_locate(segs, nseg, p, [&](int s, int local) {
    const int dt = segs.dt[s];
    KmCur c;
    c.row = (u64)segs.rows[s] + (u64)local * (u64)(C * seg_esize(dt));
    c.id = segs.off[s] + local;
    c.rs = dt == COR_I8 ? segs.scale[s][local] : 0.f;
    c.dt = dt;
    *cur = c;
  });
}

__global__ __launch_bounds__(256) void km_seed_init(const SegRowsAssign segs, int nseg, long long n, int C, long long first, unsigned* __restrict__ best,
                                                    KmCur* __restrict__ cur) {
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256)
    best[p] = p == first ? KM_CHOSEN : RANK_NEG_INF;
  if (blockIdx.x == 0 && threadIdx.x == 0) km_set_cur(segs, nseg, C, first, cur);
}

__global__ __launch_bounds__(256) void km_seed_step(const SegRowsAssign segs, int nseg, long long n, int C, float* __restrict__ best,
                                                    const KmCur* __restrict__ cur, KmPart* __restrict__ part, int t, int score,
                                                    long long* __restrict__ out_ids, float* __restrict__ out_centroids) {
  __shared__ __align__(16) float s_q[KM_CMAX];
  __shared__ KmPart s_part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const KmCur c = *cur;
  if (tid < C / 8) {
    float g[8];
    km_load8(c.row, c.dt, c.rs, tid, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) s_q[8 * tid + e] = g[e];
    if (blockIdx.x == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) out_centroids[(long long)t * C + 8 * tid + e] = g[e];
    }
  }
  if (blockIdx.x == 0 && tid == 0) out_ids[t] = c.id;
  if (!score) return;                                                    // (uniform) the last step: nothing is picked after it
  __syncthreads();

  float bv = 0.f;
  long long bid = 0;
  int bf = -1;
  for (long long p = (long long)blockIdx.x * 256 + tid; p < n; p += (long long)gridDim.x * 256) {
    u64 row = 0;
    float rs = 0.f;
    int dt = COR_F32;
    long long id = 0;
    const bool hit = km_locate(segs, nseg, p, [&](int s, int local) {    // the only place a row address is formed
      dt = segs.dt[s];
      row = (u64)segs.rows[s] + (u64)local * (u64)(C * seg_esize(dt));
      id = segs.off[s] + local;
      if (dt == COR_I8) rs = segs.scale[s][local];
    });
    if (!hit) continue;                                                  // (p < n: never)
    float a = 0.f;
    for (int ch = 0; ch < C / 8; ch += 2) {                              // C % 16 == 0: two chunks of loads in flight
      float g0[8], g1[8];
      km_load8(row, dt, rs, ch, g0);
      km_load8(row, dt, rs, ch + 1, g1);
      const f32x4 q0 = ((const f32x4*)s_q)[2 * ch], q1 = ((const f32x4*)s_q)[2 * ch + 1];
      const f32x4 q2 = ((const f32x4*)s_q)[2 * ch + 2], q3 = ((const f32x4*)s_q)[2 * ch + 3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a = fmaf(g0[i], q0[i], a);
        a = fmaf(g0[4 + i], q1[i], a);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a = fmaf(g1[i], q2[i], a);
        a = fmaf(g1[4 + i], q3[i], a);
      }
    }
    float b = best[p];
    if (a > b) {                                                         // false for a chosen row (NaN) and for a NaN score
      b = a;
      best[p] = b;
    }
    if (b == b && km_before(b, id, (int)p, bv, bid, bf)) { bv = b; bid = id; bf = (int)p; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const long long oid = __shfl_xor(bid, o, 64);
    const int of = __shfl_xor(bf, o, 64);
    if (km_before(ov, oid, of, bv, bid, bf)) { bv = ov; bid = oid; bf = of; }
  }
  if (lane == 0) { s_part[wave].v = bv; s_part[wave].id = bid; s_part[wave].flat = bf; }
  __syncthreads();
  if (tid == 0) {
    KmPart w = s_part[0];
    for (int k = 1; k < 4; ++k)
      if (km_before(s_part[k].v, s_part[k].id, s_part[k].flat, w.v, w.id, w.flat)) w = s_part[k];
    part[blockIdx.x] = w;
  }
}

__global__ __launch_bounds__(256) void km_seed_pick(const SegRowsAssign segs, int nseg, int C, const KmPart* __restrict__ part, int nparts,
                                                    unsigned* __restrict__ best, KmCur* __restrict__ cur) {
  __shared__ KmPart s_part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float bv = 0.f;
  long long bid = 0;
  int bf = -1;
  for (int k = tid; k < nparts; k += 256) {
    const KmPart w = part[k];
    if (km_before(w.v, w.id, w.flat, bv, bid, bf)) { bv = w.v; bid = w.id; bf = w.flat; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const long long oid = __shfl_xor(bid, o, 64);
    const int of = __shfl_xor(bf, o, 64);
    if (km_before(ov, oid, of, bv, bid, bf)) { bv = ov; bid = oid; bf = of; }
  }
  if (lane == 0) { s_part[wave].v = bv; s_part[wave].id = bid; s_part[wave].flat = bf; }
  __syncthreads();
  if (tid == 0) {
    KmPart w = s_part[0];
    for (int k = 1; k < 4; ++k)
      if (km_before(s_part[k].v, s_part[k].id, s_part[k].flat, w.v, w.id, w.flat)) w = s_part[k];
    if (w.flat >= 0) {                                                   // (K <= n_total: a row that is not chosen exists)
      best[w.flat] = KM_CHOSEN;
      km_set_cur(segs, nseg, C, w.flat, cur);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- update

template <int ESZ>
__global__ __launch_bounds__(64 * KM_WPB) void km_chunk_sum(const SegRowsAssign segs, int nseg, int K, int C, int with_scores, const int* __restrict__ base,
                                                            const int* __restrict__ cb, const int* __restrict__ mem, float* __restrict__ P,
                                                            float* __restrict__ PS) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * KM_WPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= cb[K]) return;                                                // the whole wave leaves; no barrier follows
  int lo = 0, hi = K - 1;                                                // the cluster: the last c with cb[c] <= w
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cb[mid] <= w) lo = mid; else hi = mid - 1;
  }
  const int c = lo;
  const int m0 = base[c] + KM_CHUNK * (int)(w - cb[c]), m1 = min(m0 + KM_CHUNK, base[c + 1]);
  const bool active = 4 * lane < C;
  const int c0 = active ? 4 * lane : 0;                                  // a lane past the row reads channels 0..3 again: in bounds, unused

  float v[4] = {0.f, 0.f, 0.f, 0.f};
  float ps = 0.f;
  for (int j0 = m0; j0 < m1; j0 += 64) {
    // lane j: member j0 + j
    u64 row = 0;
    float sc = 0.f, rs = 0.f;
    int dt = COR_F32;
    bool present = false;
    if (j0 + lane < m1)
      present = km_locate(segs, nseg, mem[j0 + lane], [&](int s, int local) {   // the only place a row address is formed
        seg_row(segs, s, local, C, dt, row, rs);
        if (with_scores) sc = segs.score[s][local];
      });
    // the members in member order, 8 rows at a time: p = p + x, and the member's score from the lane that looked it up
    seg_lane_walk<ESZ>(present, row, sc, rs, dt, c0, [&](float scj, const float (&x)[4]) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] + x[e];
      ps = ps + scj;
    });
  }
  if (active) {
    f32x4 y;
    y[0] = v[0]; y[1] = v[1]; y[2] = v[2]; y[3] = v[3];
    *(f32x4*)(P + w * C + 4 * lane) = y;
  }
  if (lane == 0) PS[w] = ps;
}

__global__ __launch_bounds__(64 * KM_WPB) void km_finish(int K, int C, const int* __restrict__ count, const int* __restrict__ cb,
                                                         const float* __restrict__ P, const float* __restrict__ PS, const float* __restrict__ prev,
                                                         float* __restrict__ out_centroids, float* __restrict__ out_score_sum) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * KM_WPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (c >= K) return;
  const bool active = 4 * lane < C;
  const int c0 = active ? 4 * lane : 0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  float ss = 0.f;
  if (count[c] == 0) {                                                   // an empty cluster keeps its previous centre, bit for bit
    if (prev) {
      const f32x4 x = *(const f32x4*)(prev + (long long)c * C + c0);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = x[e];
    }
  } else {
    const long long j0 = cb[c], j1 = cb[c + 1];
    for (long long j = j0; j < j1; ++j) {
      const f32x4 x = *(const f32x4*)(P + j * C + c0);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] + x[e];
      ss = ss + PS[j];
    }
    const float d = seg_lane_norm(v, active);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] / d;
  }
  if (active) {
    f32x4 y;
    y[0] = v[0]; y[1] = v[1]; y[2] = v[2]; y[3] = v[3];
    *(f32x4*)(out_centroids + (long long)c * C + 4 * lane) = y;
  }
  if (out_score_sum && lane == 0) out_score_sum[c] = ss;
}

// ---------------------------------------------------------------------------------------------------------------- host

struct KmLayout {                                                        // byte offsets into the workspace; the two calls share it from 0
  size_t keys, cnt, base, cb, mem, P, PS, update_end;
  size_t best, part, cur, seed_end;
  long long tiles, chunks;
};
inline KmLayout km_layout(long long n, int K, int C) {
  KmLayout L;
  L.tiles = (n + KM_TILE - 1) / KM_TILE;
  L.chunks = n / KM_CHUNK + K;                                           // sum of ceil(count / 256) <= n / 256 + K
  size_t o = 0;
  L.keys = o; o += km_up((size_t)L.tiles * KM_TILE * 4);
  L.cnt = o; o += km_up((size_t)L.tiles * K * 4);
  L.base = o; o += km_up((size_t)(K + 1) * 4);
  L.cb = o; o += km_up((size_t)(K + 1) * 4);
  L.mem = o; o += km_up((size_t)n * 4);
  L.P = o; o += km_up((size_t)L.chunks * C * 4);
  L.PS = o; o += km_up((size_t)L.chunks * 4);
  L.update_end = o;
  o = 0;
  L.best = o; o += km_up((size_t)n * 4);
  L.part = o; o += km_up((size_t)KM_SEED_BLOCKS * sizeof(KmPart));
  L.cur = o; o += km_up(sizeof(KmCur));
  L.seed_end = o;
  return L;
}

}  // namespace

extern "C" long cor_kmeans_workspace_bytes(long n_total, int K, int C) {
  if (const int rc = km_shape_check(n_total, K, C)) return rc;
  const KmLayout L = km_layout(n_total, K, C);
  return (long)(L.update_end > L.seed_end ? L.update_end : L.seed_end);
}

extern "C" int cor_kmeans_seed(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                               const int* seg_dtype, int nseg, int C, int K, long long first_id, long long* out_ids, float* out_centroids,
                               void* workspace, void* stream) {
  if (!out_ids || !out_centroids || !workspace) return COR_EINVAL;
  SegRowsAssign segs;
  int live = 0, seen = 0;
  long long n = 0;
  if (const int rc = km_table({seg_rows, seg_scale, seg_offset, seg_n, seg_dtype, nseg, true}, K, C, segs, live, n, seen)) return rc;
  if (K > n) return COR_EINVAL;
  long long first = -1, base = 0;
  for (int s = 0; s < live; ++s) {
    if (first < 0 && first_id >= segs.off[s] && (u64)first_id - (u64)segs.off[s] < (u64)segs.n[s]) first = base + (first_id - segs.off[s]);
    base += segs.n[s];
  }
  if (first < 0) return COR_EINVAL;                                      // first_id is held by no segment

  const KmLayout L = km_layout(n, K, C);
  unsigned char* ws = (unsigned char*)workspace;
  float* best = (float*)(ws + L.best);
  KmPart* part = (KmPart*)(ws + L.part);
  KmCur* cur = (KmCur*)(ws + L.cur);
  const long long want = (n + 255) / 256;
  const int blocks = (int)(want < KM_SEED_BLOCKS ? want : KM_SEED_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(km_seed_init, dim3(blocks), dim3(256), 0, st, segs, live, n, C, first, (unsigned*)best, cur);
  for (int t = 0; t < K; ++t) {
    const int score = t + 1 < K;
    hipLaunchKernelGGL(km_seed_step, dim3(score ? blocks : 1), dim3(256), 0, st, segs, live, n, C, best, cur, part, t, score, out_ids, out_centroids);
    if (score) hipLaunchKernelGGL(km_seed_pick, dim3(1), dim3(256), 0, st, segs, live, C, part, blocks, (unsigned*)best, cur);
  }
  COR_CHECK_LAUNCH();
  return 0;
}

extern "C" int cor_kmeans_update(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                                 const int* seg_dtype, int nseg, const int* const* seg_assign, const float* const* seg_score, int C, int K,
                                 const float* prev, float* out_centroids, int* out_count, float* out_score_sum, void* workspace, void* stream) {
  if (!out_centroids || !out_count || !workspace || (seg_score != nullptr) != (out_score_sum != nullptr)) return COR_EINVAL;
  SegRowsAssign t;
  int live = 0, seen = 0;
  long long n = 0;
  if (const int rc = km_table({seg_rows, seg_scale, seg_offset, seg_n, seg_dtype, nseg, true, seg_assign, true, seg_score}, K, C, t, live, n, seen)) return rc;
  const SegRowsAssign segs = km_by_offset(t, live);                             // ascending flat position is ascending global id

  const KmLayout L = km_layout(n, K, C);
  unsigned char* ws = (unsigned char*)workspace;
  unsigned* keys = (unsigned*)(ws + L.keys);
  int* cnt = (int*)(ws + L.cnt);
  int* base = (int*)(ws + L.base);
  int* cb = (int*)(ws + L.cb);
  int* mem = (int*)(ws + L.mem);
  float* P = (float*)(ws + L.P);
  float* PS = (float*)(ws + L.PS);
  const int tiles = (int)L.tiles;
  hipStream_t st = (hipStream_t)stream;
  km_member_lists(segs, live, n, K, keys, cnt, out_count, base, cb, mem, st);
  if (tiles > 0) {
    const dim3 grid((unsigned)((L.chunks + KM_WPB - 1) / KM_WPB)), block(64 * KM_WPB);
    const int with_scores = seg_score != nullptr;
#define KM_CHUNKS(ESZ) hipLaunchKernelGGL(km_chunk_sum<ESZ>, grid, block, 0, st, segs, live, K, C, with_scores, base, cb, mem, P, PS)
    if (seen == 1 << COR_F32) KM_CHUNKS(4);
    else if (seen == 1 << COR_I8) KM_CHUNKS(1);
    else if ((seen & ~((1 << COR_BF16) | (1 << COR_F16))) == 0) KM_CHUNKS(2);
    else KM_CHUNKS(-1);
#undef KM_CHUNKS
  }
  hipLaunchKernelGGL(km_finish, dim3((K + KM_WPB - 1) / KM_WPB), dim3(64 * KM_WPB), 0, st, K, C, out_count, cb, P, PS, prev, out_centroids, out_score_sum);
  COR_CHECK_LAUNCH();
  return 0;
}
