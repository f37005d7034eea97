// cor_amd — the flat positions of the clustering calls' segment table (segrows.h: SegRowsAssign) and the stable counting sort that turns a
// per-row cell id into member lists, shared by cluster.hip (cor_kmeans_update: the members of a cluster) and ivf.hip (cor_ivf_build: the
// rows of a cell). The code of this file is integer code only; segrows.h, included for the table, also holds the floating-point row
// loaders: forced-inline templates that set their own fp contract pragma and are used only by files that set it for the whole file.
//
// Rows. A FLAT position p in [0, n_total) numbers the rows of the table's non-empty segments in the order the launcher hands them to the
// kernels; with the segments in ASCENDING OFFSET (km_by_offset) ascending p is ascending global id. km_locate turns p into (segment, local
// row) with a uniform walk over the table; the range test comes first and only a hit forms an address. n_total < 2^31.
// The sort, four launches, no atomics:
//   keys    one block per tile of KM_TILE = 2048 flat positions: a 32-bit key [cluster: 14 bits | position in the tile: 11 bits] per row with
//           an assign value in [0, K) (every other row: 0xffffffff, behind all keys), bitonic sort in LDS (ranklist.h), the sorted keys go
//           to the workspace; the head of every run of one cluster finds the run's end by binary search and writes the tile's count for
//           that cluster into the tiles x K table (the block zeroed its row of the table before).
//   columns one thread per cluster walks its column of the table: exclusive prefix over the tiles in place, the total is out_count.
//   scan    one block: exclusive scans over the K counts (member-list base) and over the K chunk counts ceil(count / 256) (chunk base).
//   place   one block per tile: member slot = base[cluster] + the tile's prefix + the key's rank inside its run (binary search for the run's
//           head). The lists come out ascending by flat position inside every cluster: a stable counting sort.
#pragma once
#include "segrows.h"

namespace {

constexpr int KM_CMAX = 256;                   // 64 lanes x 4 channels
constexpr int KM_TILE_BITS = 11, KM_TILE = 1 << KM_TILE_BITS;   // rows per tile of the member-list build
constexpr int KM_CHUNK = 256;                  // members per chunk sum (part of cor_kmeans_update's definition)
constexpr unsigned KM_NOKEY = 0xffffffffu;
static_assert(COR_KMEANS_KMAX <= (1 << 14) && COR_KMEANS_KMAX * (1ll << KM_TILE_BITS) < (1ll << 32) - 1, "a key is [cluster | position in the tile] in 32 bits");

// flat position -> on_hit(segment, local row) and true, or false: p lies past the table. Every segment is visited (uniform trip count, the
// table in scalar registers); the callers form their addresses inside on_hit, from a hit alone
template <typename OnHit> __device__ __forceinline__ bool km_locate(const SegRowsAssign& segs, int nseg, long long p, const OnHit on_hit) {
  bool hit = false;
  long long base = 0;
  for (int s = 0; s < nseg; ++s) {
    const long long n = segs.n[s];
    if (!hit && p >= base && p - base < n) {
      hit = true;
      on_hit(s, (int)(p - base));
    }
    base += n;
  }
  return hit;
}

__global__ __launch_bounds__(256) void km_tile_keys(const SegRowsAssign segs, int nseg, long long n, int K, unsigned* __restrict__ keys,
                                                    int* __restrict__ cnt) {
  __shared__ unsigned key[KM_TILE];
  const int tid = threadIdx.x;
  const long long tile = blockIdx.x;
  int* row = cnt + tile * K;
  for (int c = tid; c < K; c += 256) row[c] = 0;
  for (int i = tid; i < KM_TILE; i += 256) {
    const long long p = tile * KM_TILE + i;
    unsigned k = KM_NOKEY;
    if (p < n)
      km_locate(segs, nseg, p, [&](int s, int local) {
        const int a = segs.assign[s][local];
        if ((unsigned)a < (unsigned)K) k = ((unsigned)a << KM_TILE_BITS) | (unsigned)i;   // any other value: the row belongs to no cluster
      });
    key[i] = k;
  }
  __syncthreads();
  block_bitonic_sort(key, KM_TILE, PlainBefore{});                       // ends with a barrier (the zeroes above are ordered by it too)
  for (int i = tid; i < KM_TILE; i += 256) {
    const unsigned k = key[i];
    keys[tile * KM_TILE + i] = k;
    if (k == KM_NOKEY) continue;
    const unsigned c = k >> KM_TILE_BITS;
    if (i > 0 && (key[i - 1] >> KM_TILE_BITS) == c) continue;
    const unsigned lim = (c + 1) << KM_TILE_BITS;                        // the run of cluster c ends at the first key >= lim
    int lo = i + 1, hi = KM_TILE;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (key[mid] < lim) lo = mid + 1; else hi = mid;
    }
    row[c] = lo - i;
  }
}

__global__ __launch_bounds__(256) void km_columns(int* __restrict__ cnt, int tiles, int K, int* __restrict__ out_count) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= K) return;
  int run = 0;
  for (long long t = 0; t < tiles; ++t) {
    const int v = cnt[t * K + c];
    cnt[t * K + c] = run;
    run += v;
  }
  out_count[c] = run;
}

// base[c] = the members before cluster c, cb[c] = the chunks before it, both with a K-th entry (the totals)
__global__ __launch_bounds__(1024) void km_scan(const int* __restrict__ count, int K, int* __restrict__ base, int* __restrict__ cb) {
  __shared__ int s_m[1024], s_c[1024];
  const int tid = threadIdx.x;
  const int per = (K + 1023) / 1024, c0 = tid * per, c1 = min(c0 + per, K);
  int m = 0, ch = 0;
  for (int c = c0; c < c1; ++c) {
    const int v = count[c];
    m += v;
    ch += (v + KM_CHUNK - 1) / KM_CHUNK;
  }
  s_m[tid] = m;
  s_c[tid] = ch;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int xm = tid >= o ? s_m[tid - o] : 0, xc = tid >= o ? s_c[tid - o] : 0;
    __syncthreads();
    s_m[tid] += xm;
    s_c[tid] += xc;
    __syncthreads();
  }
  int rm = s_m[tid] - m, rc = s_c[tid] - ch;
  for (int c = c0; c < c1; ++c) {
    base[c] = rm;
    cb[c] = rc;
    const int v = count[c];
    rm += v;
    rc += (v + KM_CHUNK - 1) / KM_CHUNK;
  }
  if (tid == 1023) {
    base[K] = s_m[1023];
    cb[K] = s_c[1023];
  }
}

__global__ __launch_bounds__(256) void km_place(const unsigned* __restrict__ keys, const int* __restrict__ cnt, const int* __restrict__ base,
                                                int K, long long n, int* __restrict__ mem) {
  __shared__ unsigned key[KM_TILE];
  const int tid = threadIdx.x;
  const long long tile = blockIdx.x;
  for (int i = tid; i < KM_TILE; i += 256) key[i] = keys[tile * KM_TILE + i];
  __syncthreads();
  for (int i = tid; i < KM_TILE; i += 256) {
    const unsigned k = key[i];
    if (k == KM_NOKEY) continue;
    const unsigned c = k >> KM_TILE_BITS, lim = c << KM_TILE_BITS;       // (c < K: km_tile_keys made the key)
    int lo = 0, hi = i;                                                  // the run's head: the first key >= lim
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (key[mid] < lim) lo = mid + 1; else hi = mid;
    }
    const long long slot = (long long)base[c] + cnt[tile * K + c] + (i - lo);
    if (slot < n) mem[slot] = (int)(tile * KM_TILE + (k & (KM_TILE - 1)));   // (always: the counts sum to at most n)
  }
}

// ---------------------------------------------------------------------------------------------------------------- host

inline size_t km_up(size_t b) { return (b + 255) & ~(size_t)255; }

inline int km_shape_check(long long n, int K, int C) {
  if (n < 0 || K < 1 || C < 1) return COR_EINVAL;
  if (K > COR_KMEANS_KMAX || C > KM_CMAX || C % 16 != 0 || n > 0x7fffffffll) return COR_ENOSUPPORT;
  return 0;
}

// the checks of the table the calls share, in the header's order; fills `segs` with the NON-EMPTY segments in table order
inline int km_table(const SegArrays& t, int K, int C, SegRowsAssign& segs, int& live, long long& n_total, int& seen) {
  if (t.nseg < 0 || K < 1 || C < 1) return COR_EINVAL;
  if (const int rc = seg_table_check(t)) return rc;
  n_total = 0;
  for (int s = 0; s < t.nseg; ++s) n_total += t.n[s];
  if (const int rc = km_shape_check(n_total, K, C)) return rc;
  return seg_table_fill(t, true, segs, live, seen);
}

// the table in ascending offset: ascending flat position is ascending global id (the ranges are disjoint)
inline SegRowsAssign km_by_offset(const SegRowsAssign& t, int live) {
  int order[SEG_MAX];
  for (int s = 0; s < live; ++s) order[s] = s;
  for (int a = 1; a < live; ++a)
    for (int b = a; b > 0 && t.off[order[b]] < t.off[order[b - 1]]; --b) { const int x = order[b]; order[b] = order[b - 1]; order[b - 1] = x; }
  SegRowsAssign segs = {};
  for (int s = 0; s < live; ++s) {
    const int o = order[s];
    segs.rows[s] = t.rows[o]; segs.off[s] = t.off[o]; segs.n[s] = t.n[o]; segs.dt[s] = t.dt[o]; segs.scale[s] = t.scale[o];
    segs.assign[s] = t.assign[o]; segs.score[s] = t.score[o];
  }
  return segs;
}

// the four launches: keys / cnt / mem are workspace (tiles * KM_TILE keys, tiles * K counts, n positions), count [K], base and cb [K + 1]
inline void km_member_lists(const SegRowsAssign& segs, int live, long long n, int K, unsigned* keys, int* cnt, int* count, int* base, int* cb, int* mem,
                            hipStream_t st) {
  const int tiles = (int)((n + KM_TILE - 1) / KM_TILE);
  if (tiles > 0) hipLaunchKernelGGL(km_tile_keys, dim3(tiles), dim3(256), 0, st, segs, live, n, K, keys, cnt);
  hipLaunchKernelGGL(km_columns, dim3((K + 255) / 256), dim3(256), 0, st, cnt, tiles, K, count);
  hipLaunchKernelGGL(km_scan, dim3(1), dim3(1024), 0, st, count, K, base, cb);
  if (tiles > 0) hipLaunchKernelGGL(km_place, dim3(tiles), dim3(256), 0, st, keys, cnt, base, K, n, mem);
}

}  // namespace
