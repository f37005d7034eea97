// cor_amd — cell-probing search ("IVF-flat"): cor_ivf_build lays the rows of a gallery out cell by cell, cor_ivf_search returns the exact
// top-k over the rows of the cells a query probes. Contract and both definitions, fixed to the bit: include/cor_amd.h.
//
// cor_ivf_build: 5 launches. The four of member_sort.h's stable counting sort (the sort of cor_kmeans_update: tile keys, column scan, scan,
//   place; no atomics) leave slot -> flat position in the workspace and write the members-before-cell table straight into out_cell_start.
//   copy    one WAVE per IVF_CPW = 4 consecutive slots: the slot's flat position is looked up in the segment table (km_locate: the range
//           test first, an address from a hit alone), lane l moves bytes [16 l, 16 l + 16) of the row: ONE coalesced wave load and store per
//           row, the four loads issued before the first store. Lane 0 writes the global id and the scale. Rows are never converted.
// cor_ivf_search: 2 launches.
//   scan    P blocks of 256 threads per query. The block keeps the query in LDS (rounded to the row dtype and widened back; int8: quantised
//           by the rule of quant_i8.h with its scale). Thread j < nprobe range-tests probe j BEFORE anything is derived from it, drops it
//           if a probe j' < j names the same cell, and publishes the cell's slot range (a dropped probe: an empty range). The work units
//           (probe j, slice s < S of its cell) are dealt round-robin: block p takes units p, p + P, ...; slice s walks the tiles s, s + S,
//           ... of IVF_TILE = 512 slots to the END of the cell, so S (from the max_cell hint) only deals work out. A thread scores two
//           rows of a tile, chains interleaved, and reads a row in pieces of 128 bytes (a cache line), the piece's eight 16-byte loads
//           issued together, so that a line is fetched once; plain fmaf chains (int8: four v_dot4 per 16 bytes).
//           Running top-k: 64-bit keys [score key, ascending as the score descends | -0.0 flag: bit 31 | slot: 31 bits] in an LDS buffer of
//           IVF_CAP = 2048. A row is appended only if its score key is at or below the threshold, the score key of the k-th entry after
//           the last sort (none before the first k rows). When a tile might not fit, the buffer is sorted (ranklist.h's bitonic network,
//           ties by the global id read through the slot) and cut to k. One partial list of k (score, id) per block goes to the workspace.
//   finish  one block per query ranks the P partial lists by the same order and writes k entries, then the (-inf, -1) tail.
//   (score, id) is a total order on a query's candidates (distinct ids), so neither P, S nor the order of the appends shows in the result.
// Order. Float rows: cor_similarity_topk's (score desc as floats, -0.0 ties with +0.0, id asc), the bits of a -0.0 carried by the flag.
// Int8 rows: cor_similarity_topk_i8's (order-preserving key of the score BITS desc, +0.0 above -0.0, id asc).
// LDS: scan 16 KiB keys + 1 KiB query + 2 KiB ranges; finish 8 B per entry (<= 32 KiB). No scratch memory in global.
#include "member_sort.h"
#include "quant_i8.h"

#pragma clang fp contract(off)

namespace {

constexpr int IVF_T = 256;                     // threads of a scan block
constexpr int IVF_NI = 2;                      // rows per thread and tile, a 128-byte piece of each in flight
constexpr int IVF_TILE = IVF_T * IVF_NI;       // slots per tile
constexpr int IVF_CAP = 2048;                  // keys in LDS: the k kept ones and at least one tile of appends
constexpr int IVF_SMAX = 1 << 12;              // most slices per cell (a hint beyond 2M rows deals no finer)
constexpr int IVF_FILL = 1024;                 // blocks the automatic P aims at: 256 CUs four times over
constexpr int IVF_CPW = 4;                     // slots per wave of the copy
constexpr unsigned IVF_SLOT_MASK = 0x7fffffffu, IVF_NEGZERO = 0x80000000u;
static_assert(COR_TOPK_KMAX + IVF_TILE <= IVF_CAP, "k kept entries and a whole tile fit the key buffer");
static_assert(COR_IVF_NPROBE_MAX <= IVF_T, "thread j owns probe j");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------------- build

__global__ __launch_bounds__(256) void ivf_copy(const SegRowsAssign segs, int nseg, int rowbytes, int K, const int* __restrict__ cell_start,
                                                const int* __restrict__ mem, unsigned char* __restrict__ out_rows,
                                                float* __restrict__ out_scale, long long* __restrict__ out_ids) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long total = cell_start[K], s0 = w * IVF_CPW;
  if (s0 >= total) return;                                               // the whole wave leaves; no barrier follows
  const bool active = 16 * lane < rowbytes;
  u32x4 v[IVF_CPW];
  long long id[IVF_CPW];
  float sc[IVF_CPW];
  bool has[IVF_CPW];
#pragma unroll
  for (int u = 0; u < IVF_CPW; ++u) {
    v[u] = u32x4{0u, 0u, 0u, 0u};
    id[u] = 0;
    sc[u] = 0.f;
    has[u] = false;
    if (s0 + u < total)
      has[u] = km_locate(segs, nseg, mem[s0 + u], [&](int s, int local) {   // the only place a source address is formed
        if (active) v[u] = *(const u32x4*)(segs.rows[s] + (u64)local * (u64)rowbytes + 16u * lane);
        id[u] = segs.off[s] + local;
        if (segs.dt[s] == COR_I8) sc[u] = segs.scale[s][local];
      });
  }
#pragma unroll
  for (int u = 0; u < IVF_CPW; ++u)
    if (has[u]) {
      const u64 slot = (u64)(s0 + u);
      if (active) *(u32x4*)(out_rows + slot * (u64)rowbytes + 16u * lane) = v[u];
      if (lane == 0) {
        out_ids[slot] = id[u];
        if (out_scale) out_scale[slot] = sc[u];
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------- search

// the score key of a dtype's order: BITS (int8 rows) orders by the score's bits, else -0.0 keys as +0.0 (ranklist.h)
template <bool BITS> __device__ __forceinline__ unsigned ivf_score_key(unsigned u) {
  if (!BITS) return rank_score_key(u);
  return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
// and back: the score bits of a present entry's key
template <bool BITS> __device__ __forceinline__ unsigned ivf_key_score(u64 key) {
  if (!BITS && ((unsigned)key & IVF_NEGZERO)) return 0x80000000u;
  const unsigned asc = ~(unsigned)(key >> 32);
  return (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
}
// ranklist.h's tie rule with the global id read through the slot; padding (RANK_MISSING) never reads an id
struct IvfBefore {
  const long long* ids;
  __device__ __forceinline__ bool operator()(u64 a, u64 b) const {
    const unsigned ha = (unsigned)(a >> 32), hb = (unsigned)(b >> 32);
    if (ha == hb && ha != RANK_MISSING) {
      const long long ia = ids[(unsigned)a & IVF_SLOT_MASK], ib = ids[(unsigned)b & IVF_SLOT_MASK];
      if (ia != ib) return ia < ib;
    }
    return a < b;
  }
};

// elements [8 g, 8 g + 8) of the 128-byte piece x of a float row, widened exactly to fp32
template <typename TG> __device__ __forceinline__ void ivf_widen8(const uint4 (&x)[8], int g, float (&f)[8]) {
  if constexpr (sizeof(TG) == 4) {
    const uint4 a = x[2 * g], b = x[2 * g + 1];
    f[0] = __uint_as_float(a.x); f[1] = __uint_as_float(a.y); f[2] = __uint_as_float(a.z); f[3] = __uint_as_float(a.w);
    f[4] = __uint_as_float(b.x); f[5] = __uint_as_float(b.y); f[6] = __uint_as_float(b.z); f[7] = __uint_as_float(b.w);
  } else if constexpr (__is_same(TG, bf16_t)) {
    const unsigned w[4] = {x[g].x, x[g].y, x[g].z, x[g].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[2 * e] = __uint_as_float(w[e] << 16); f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
  } else {
    const f16x8 h = __builtin_bit_cast(f16x8, x[g]);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)h[e];
  }
}

// sort the first s_cnt keys, keep the k best: -> the new threshold (the score key of the k-th entry, RANK_MISSING while fewer are held).
// Called by the whole block behind a barrier that published s_cnt and the keys
__device__ __forceinline__ unsigned ivf_compact(u64* key, int* s_cnt, int k, const long long* __restrict__ ids) {
  const int tid = threadIdx.x;
  const int n = *s_cnt;
  int npad = 2;
  while (npad < n) npad <<= 1;
  for (int i = n + tid; i < npad; i += IVF_T) key[i] = ~0ull;
  __syncthreads();
  block_bitonic_sort(key, npad, IvfBefore{ids});
  const unsigned thr = n >= k ? (unsigned)(key[k - 1] >> 32) : RANK_MISSING;
  if (tid == 0) *s_cnt = n < k ? n : k;
  __syncthreads();
  return thr;
}

template <typename TG>
__global__ __launch_bounds__(IVF_T) void ivf_scan_kernel(const float* __restrict__ Q, const TG* __restrict__ rows, const float* __restrict__ scale,
                                                         const long long* __restrict__ ids, const int* __restrict__ cell_start, int K, int C,
                                                         const long long* __restrict__ probes, int nprobe, int k, int S, int P,
                                                         unsigned* __restrict__ part_scores, long long* __restrict__ part_ids,
                                                         int* __restrict__ part_cnt, int* __restrict__ out_scanned) {
  constexpr bool I8 = sizeof(TG) == 1;
  __shared__ u64 key[IVF_CAP];
  __shared__ __align__(16) float qs[256];                                // int8: the first 64 words hold the quantised query
  __shared__ int s_lo[IVF_T], s_hi[IVF_T];                               // s_lo doubles as the cell table while the probes are screened
  __shared__ int s_cnt, s_scanned;
  __shared__ float s_qscale;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x / (unsigned)P;
  const int p = (int)(blockIdx.x - (unsigned)b * (unsigned)P);

  // the query
  if constexpr (I8) {
    if (tid < 64) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (4 * tid < C) {
        const f32x4 x = *(const f32x4*)(Q + b * C + 4 * tid);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
      }
      float amax = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fabsf(v[i]));
      amax = wave_max(amax);
      const float inv = q8_inv(amax);
      unsigned w = 0u;
      if (amax != 0.f) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w |= ((unsigned)q8_value(v[i], inv) & 0xffu) << (8 * i);
      }
      ((unsigned*)qs)[tid] = w;
      if (tid == 0) s_qscale = q8_scale(amax);
    }
  } else {
    for (int c = tid; c < C; c += IVF_T) qs[c] = round_to<TG>(Q[b * C + c]);
  }

  // the probes: range test, then the first occurrence of every cell
  int cell = -1;
  if (tid < nprobe) {
    const long long v = probes[b * nprobe + tid];
    if (v >= 0 && v < (long long)K) cell = (int)v;                       // nothing is derived from a value that failed
  }
  s_lo[tid] = cell;
  if (tid == 0) { s_cnt = 0; s_scanned = 0; }
  __syncthreads();
  bool live = cell >= 0;
  for (int j = 0; j < tid && live; ++j) live = s_lo[j] != cell;
  int lo = 0, hi = 0;
  if (live) { lo = cell_start[cell]; hi = cell_start[cell + 1]; }
  __syncthreads();
  s_lo[tid] = lo;
  s_hi[tid] = hi;
  if (p == 0 && out_scanned != nullptr && hi > lo) atomicAdd(&s_scanned, hi - lo);
  __syncthreads();
  if (p == 0 && out_scanned != nullptr && tid == 0) out_scanned[b] = s_scanned;
  const float qscale = I8 ? s_qscale : 0.f;

  unsigned thr = RANK_MISSING;
  const int units = nprobe * S;
  for (int u = p; u < units; u += P) {
    const int j = u / S, s = u - j * S;
    const int c_lo = s_lo[j], len = s_hi[j] - c_lo;
    for (long long t0 = (long long)s * IVF_TILE; t0 < len; t0 += (long long)S * IVF_TILE) {
      const int held = s_cnt;                                            // published by the barrier that ended the tile before
      __syncthreads();                                                   // ... and read by every thread before this tile's first append
      if (held + IVF_TILE > IVF_CAP) thr = ivf_compact(key, &s_cnt, k, ids);
      int slot[IVF_NI];
      unsigned bits[IVF_NI];
#pragma unroll
      for (int i = 0; i < IVF_NI; ++i) {
        const long long r = t0 + tid + i * IVF_T;
        slot[i] = r < len ? c_lo + (int)r : -1;
      }
      // a row is walked in pieces of 128 bytes (a cache line: 8 loads of 16 bytes, all issued before the first use), nv 16-byte words in all
      const int nv = C * (int)sizeof(TG) / 16;
      const uint4* row[IVF_NI];
#pragma unroll
      for (int i = 0; i < IVF_NI; ++i) row[i] = slot[i] >= 0 ? (const uint4*)((const unsigned char*)rows + (u64)slot[i] * (u64)(C * (int)sizeof(TG))) : nullptr;
      float acc[IVF_NI];
      int d[IVF_NI];
#pragma unroll
      for (int i = 0; i < IVF_NI; ++i) { acc[i] = 0.f; d[i] = 0; }
      for (int v0 = 0; v0 < nv; v0 += 8) {
        uint4 x[IVF_NI][8];
#pragma unroll
        for (int i = 0; i < IVF_NI; ++i)
#pragma unroll
          for (int v = 0; v < 8; ++v) x[i][v] = (row[i] && v0 + v < nv) ? row[i][v0 + v] : make_uint4(0u, 0u, 0u, 0u);
        if constexpr (I8) {
#pragma unroll
          for (int v = 0; v < 8; ++v)
            if (v0 + v < nv) {                                           // (uniform) 16 channels: four v_dot4 against the query's words
              const uint4 q = ((const uint4*)qs)[v0 + v];
#pragma unroll
              for (int i = 0; i < IVF_NI; ++i) {
                d[i] = __builtin_amdgcn_sdot4((int)x[i][v].x, (int)q.x, d[i], false);
                d[i] = __builtin_amdgcn_sdot4((int)x[i][v].y, (int)q.y, d[i], false);
                d[i] = __builtin_amdgcn_sdot4((int)x[i][v].z, (int)q.z, d[i], false);
                d[i] = __builtin_amdgcn_sdot4((int)x[i][v].w, (int)q.w, d[i], false);
              }
            }
        } else {
          constexpr int G = 16 / (int)sizeof(TG);                        // groups of 8 channels in a piece
          const int c0 = v0 * G / 8;                                     // the piece's first group (chunk c of oracle/c/sim_chain.c)
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (8 * (c0 + g) < C) {                                      // (uniform)
              const f32x4 qa = ((const f32x4*)qs)[2 * (c0 + g)], qb = ((const f32x4*)qs)[2 * (c0 + g) + 1];
              float f[IVF_NI][8];
#pragma unroll
              for (int i = 0; i < IVF_NI; ++i) ivf_widen8<TG>(x[i], g, f[i]);
#pragma unroll
              for (int e = 0; e < 4; ++e) {                              // k = 8c + e, then 8c + 4 + e
#pragma unroll
                for (int i = 0; i < IVF_NI; ++i) acc[i] = fmaf(f[i][e], qa[e], acc[i]);
#pragma unroll
                for (int i = 0; i < IVF_NI; ++i) acc[i] = fmaf(f[i][4 + e], qb[e], acc[i]);
              }
            }
        }
      }
#pragma unroll
      for (int i = 0; i < IVF_NI; ++i) {
        if constexpr (I8) bits[i] = __float_as_uint(((float)d[i] * qscale) * (slot[i] >= 0 ? scale[slot[i]] : 0.f));
        else bits[i] = __float_as_uint(acc[i]);
      }
#pragma unroll
      for (int i = 0; i < IVF_NI; ++i)
        if (slot[i] >= 0) {
          const unsigned h = ivf_score_key<I8>(bits[i]);
          if (h <= thr) {                                                // at most IVF_TILE appends: the buffer had room for them
            unsigned l = (unsigned)slot[i];
            if (!I8 && bits[i] == 0x80000000u) l |= IVF_NEGZERO;
            key[atomicAdd(&s_cnt, 1)] = ((u64)h << 32) | l;
          }
        }
      __syncthreads();
    }
  }
  __syncthreads();
  thr = ivf_compact(key, &s_cnt, k, ids);
  const int cnt = s_cnt;
  const long long out0 = ((long long)b * P + p) * k;
  for (int r = tid; r < k; r += IVF_T) {
    if (r < cnt) {
      part_scores[out0 + r] = ivf_key_score<I8>(key[r]);
      part_ids[out0 + r] = ids[(unsigned)key[r] & IVF_SLOT_MASK];
    } else {
      part_scores[out0 + r] = RANK_NEG_INF;
      part_ids[out0 + r] = -1;
    }
  }
  if (tid == 0) part_cnt[(long long)b * P + p] = cnt;
}

// the ids of one query's partial lists, by position (the finish kernel's tie rule)
struct IvfPartIds {
  const long long* ids;
  __device__ __forceinline__ long long operator()(unsigned pos) const { return ids[pos]; }
};

template <bool BITS>
__global__ __launch_bounds__(1024) void ivf_finish_kernel(const unsigned* __restrict__ part_scores, const long long* __restrict__ part_ids,
                                                          const int* __restrict__ part_cnt, int P, int k, int npad,
                                                          unsigned* __restrict__ out_scores, long long* __restrict__ out_idx) {
  extern __shared__ __align__(16) unsigned char ivf_lds[];
  __shared__ int s_present;
  u64* key = (u64*)ivf_lds;
  const int tid = threadIdx.x, T = blockDim.x, n = P * k;
  const long long in0 = (long long)blockIdx.x * n, out0 = (long long)blockIdx.x * k;
  if (tid == 0) s_present = 0;
  __syncthreads();
  int mine = 0;
  for (int pos = tid; pos < npad; pos += T) {
    unsigned h = RANK_MISSING;
    if (pos < n) {
      const int pl = pos / k;
      if (pos - pl * k < part_cnt[(long long)blockIdx.x * P + pl]) h = ivf_score_key<BITS>(part_scores[in0 + pos]);
    }
    mine += h != RANK_MISSING;                     // counted by the KEY: the first `present` ranks are exactly the keys below MISSING
    key[pos] = ((u64)h << 32) | (unsigned)pos;
  }
  if (mine) atomicAdd(&s_present, mine);
  __syncthreads();
  block_bitonic_sort(key, npad, RankBefore<IvfPartIds>{IvfPartIds{part_ids + in0}});
  const int present = s_present;
  for (int r = tid; r < k; r += T) {
    if (r < present) {
      const long long at = in0 + ((unsigned)key[r] & RANK_POS_MASK);
      out_scores[out0 + r] = part_scores[at];
      out_idx[out0 + r] = part_ids[at];
    } else {
      out_scores[out0 + r] = RANK_NEG_INF;
      out_idx[out0 + r] = -1;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host

struct IvfBuildLayout { size_t keys, cnt, count, cb, mem, end; };
inline IvfBuildLayout ivf_build_layout(long long n, int K) {
  IvfBuildLayout L;
  const size_t tiles = (size_t)((n + KM_TILE - 1) / KM_TILE);
  size_t o = 0;
  L.keys = o; o += km_up(tiles * KM_TILE * 4);
  L.cnt = o; o += km_up(tiles * K * 4);
  L.count = o; o += km_up((size_t)K * 4);
  L.cb = o; o += km_up((size_t)(K + 1) * 4);
  L.mem = o; o += km_up((size_t)n * 4);
  L.end = o;
  return L;
}

inline bool ivf_dtype_ok(int dt) { return dt == COR_F32 || dt == COR_BF16 || dt == COR_F16 || dt == COR_I8; }

// the shape checks of cor_ivf_search and its workspace query, in the header's order
inline int ivf_search_shape_check(int Bq, int K, int C, int nprobe, int k, int max_cell, int split) {
  if (Bq < 0 || K < 1 || C < 1 || k < 1 || nprobe < 1 || max_cell < 1 || split < 0) return COR_EINVAL;
  if (k > COR_TOPK_KMAX || nprobe > COR_IVF_NPROBE_MAX || K > COR_KMEANS_KMAX || C > KM_CMAX || C % 16 != 0) return COR_ENOSUPPORT;
  if (split > 0 && (long long)split * k > COR_MERGE_NMAX) return COR_ENOSUPPORT;
  return 0;
}
// the most partial lists per query the automatic choice makes (it also never exceeds the number of work units)
inline int ivf_auto_lists(int Bq, int k) {
  const int want = (IVF_FILL + (Bq > 0 ? Bq : 1) - 1) / (Bq > 0 ? Bq : 1), most = COR_MERGE_NMAX / k;
  return want < most ? want : most;
}
inline size_t ivf_search_bytes(int Bq, int P, int k) {
  const size_t lists = (size_t)Bq * P;
  return km_up(lists * k * 4) + km_up(lists * k * 8) + km_up(lists * 4);
}

template <typename TG>
void ivf_launch_scan(const float* Q, const void* rows, const float* scale, const long long* ids, const int* cell_start, int K, int C, int Bq,
                     const long long* probes, int nprobe, int k, int S, int P, unsigned* ps, long long* pi, int* pc, int* out_scanned,
                     hipStream_t st) {
  hipLaunchKernelGGL(ivf_scan_kernel<TG>, dim3((unsigned)Bq * (unsigned)P), dim3(IVF_T), 0, st, Q, (const TG*)rows, scale, ids, cell_start, K, C,
                     probes, nprobe, k, S, P, ps, pi, pc, out_scanned);
}

}  // namespace

extern "C" long cor_ivf_build_workspace_bytes(long n_total, int K, int C) {
  if (const int rc = km_shape_check(n_total, K, C)) return rc;
  return (long)ivf_build_layout(n_total, K).end;
}

extern "C" int cor_ivf_build(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                             const int* seg_dtype, int nseg, const int* const* seg_assign, int C, int K, int dtype, void* out_rows,
                             float* out_scale, long long* out_ids, int* out_cell_start, void* workspace, void* stream) {
  if (!out_rows || !out_ids || !out_cell_start || !workspace || (dtype == COR_I8 && !out_scale)) return COR_EINVAL;
  SegRowsAssign t;
  int live = 0, seen = 0;
  long long n = 0;
  if (const int rc = km_table({seg_rows, seg_scale, seg_offset, seg_n, seg_dtype, nseg, true, seg_assign, true}, K, C, t, live, n, seen)) return rc;
  if (!ivf_dtype_ok(dtype)) return COR_ENOSUPPORT;
  for (int s = 0; s < nseg; ++s)
    if (seg_dtype[s] != dtype) return COR_ENOSUPPORT;                    // rows are copied, never converted
  if (((uintptr_t)out_rows & 15) || ((uintptr_t)workspace & 255)) return COR_EINVAL;
  for (int s = 0; s < live; ++s)
    if ((uintptr_t)t.rows[s] & 15) return COR_EINVAL;
  const SegRowsAssign segs = km_by_offset(t, live);                             // ascending flat position is ascending global id

  const IvfBuildLayout L = ivf_build_layout(n, K);
  unsigned char* ws = (unsigned char*)workspace;
  int* mem = (int*)(ws + L.mem);
  hipStream_t st = (hipStream_t)stream;
  km_member_lists(segs, live, n, K, (unsigned*)(ws + L.keys), (int*)(ws + L.cnt), (int*)(ws + L.count), out_cell_start, (int*)(ws + L.cb), mem, st);
  if (n > 0) {
    const int rowbytes = C * seg_esize(dtype);
    const long long waves = (n + IVF_CPW - 1) / IVF_CPW;
    hipLaunchKernelGGL(ivf_copy, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, segs, live, rowbytes, K, out_cell_start, mem,
                       (unsigned char*)out_rows, dtype == COR_I8 ? out_scale : nullptr, out_ids);
  }
  COR_CHECK_LAUNCH();
  return 0;
}

extern "C" long cor_ivf_search_workspace_bytes(int Bq, int K, int C, int nprobe, int k, int split) {
  if (const int rc = ivf_search_shape_check(Bq, K, C, nprobe, k, 1, split)) return rc;
  return (long)ivf_search_bytes(Bq, split > 0 ? split : ivf_auto_lists(Bq, k), k);
}

extern "C" int cor_ivf_search(const float* Q, const void* rows, const float* scale, int dtype, const long long* ids, const int* cell_start, int K,
                              int C, int Bq, const long long* probes, int nprobe, int k, int max_cell, int split, float* out_scores,
                              long long* out_idx, int* out_scanned, void* workspace, void* stream) {
  if (!Q || !rows || !ids || !cell_start || !probes || !out_scores || !out_idx || !workspace || (dtype == COR_I8 && !scale)) return COR_EINVAL;
  if (const int rc = ivf_search_shape_check(Bq, K, C, nprobe, k, max_cell, split)) return rc;
  if (!ivf_dtype_ok(dtype)) return COR_ENOSUPPORT;
  if (((uintptr_t)Q & 15) || ((uintptr_t)rows & 15) || ((uintptr_t)workspace & 255)) return COR_EINVAL;
  if (Bq == 0) return 0;

  long long S = ((long long)max_cell + IVF_TILE - 1) / IVF_TILE;         // slices per cell: a dealing-out of work, not part of the result
  if (S > IVF_SMAX) S = IVF_SMAX;
  const long long units = (long long)nprobe * S;
  int P = split;
  if (P == 0) {
    P = ivf_auto_lists(Bq, k);
    if (P > units) P = (int)units;
  }
  if ((long long)Bq * P > 0x7fffffffll) return COR_ENOSUPPORT;           // the scan's grid
  unsigned char* ws = (unsigned char*)workspace;
  const size_t lists = (size_t)Bq * P;
  unsigned* ps = (unsigned*)ws;
  long long* pi = (long long*)(ws + km_up(lists * k * 4));
  int* pc = (int*)(ws + km_up(lists * k * 4) + km_up(lists * k * 8));
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case COR_F32: ivf_launch_scan<float>(Q, rows, scale, ids, cell_start, K, C, Bq, probes, nprobe, k, (int)S, P, ps, pi, pc, out_scanned, st); break;
    case COR_BF16: ivf_launch_scan<bf16_t>(Q, rows, scale, ids, cell_start, K, C, Bq, probes, nprobe, k, (int)S, P, ps, pi, pc, out_scanned, st); break;
    case COR_F16: ivf_launch_scan<_Float16>(Q, rows, scale, ids, cell_start, K, C, Bq, probes, nprobe, k, (int)S, P, ps, pi, pc, out_scanned, st); break;
    default: ivf_launch_scan<signed char>(Q, rows, scale, ids, cell_start, K, C, Bq, probes, nprobe, k, (int)S, P, ps, pi, pc, out_scanned, st); break;
  }
  const int npad = next_pow2(P * k);
  const int threads = npad / 2 < 64 ? 64 : (npad / 2 > 1024 ? 1024 : npad / 2);
  if (dtype == COR_I8)
    hipLaunchKernelGGL(ivf_finish_kernel<true>, dim3((unsigned)Bq), dim3(threads), 8 * (size_t)npad, st, ps, pi, pc, P, k, npad, (unsigned*)out_scores, out_idx);
  else
    hipLaunchKernelGGL(ivf_finish_kernel<false>, dim3((unsigned)Bq), dim3(threads), 8 * (size_t)npad, st, ps, pi, pc, P, k, npad, (unsigned*)out_scores, out_idx);
  COR_CHECK_LAUNCH();
  return 0;
}
