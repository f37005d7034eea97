// cor_amd — result diversification of candidate lists (cor_diversify_mmr): greedy maximal marginal relevance with optional near-duplicate
// suppression. Per query k dependent steps: the alive entry with the greatest f = lam * score - (1 - lam) * (its largest similarity to a
// winner so far) wins, then every alive entry's penalty is raised by its chain similarity to the winner's row and an entry at or above
// max_sim leaves for good. Contract and the definition, fixed to the bit: include/cor_amd.h.
//
// One block per query, T = max(64, min(npad, 256), npad / 4) threads (npad = kin rounded up to a power of two): one candidate per thread
// up to kin = 256, then up to four, thread t owning the positions t, t + T, t + 2T, t + 3T (rescore.hip's layout). A candidate's state
// stays in registers: row address, row scale, score, penalty, four dtype bytes in one register and four alive bits in another. No
// global workspace, no Gram matrix: k * kin chains per query at most.
//   0. Presence. Every id is looked up in the segment table (ranklist.h's seg_lookup: the range test comes first); only a hit forms a
//      row address and reads its score. The table is a by-value kernel argument.
//   Step t:
//   1. Argmax. Every thread's best alive candidate (f, position), a 6-step wave butterfly, the wave's best taken from lane 0; the lane
//      that OWNS that position writes (f, position, row address, scale, dtype) into the wave's LDS slot, so the slot always holds a real
//      row of this query (or position -1: nothing alive in the wave). Barrier. Every thread walks the <= 16 slots in the same order
//      and finds the same winner. The comparator is (f desc as floats, id asc, position asc); the ids are read on a tie only.
//   2. Output by thread 0: the winner's INPUT score bits, id, position, f. The owner clears the winner's alive bit. t + 1 == k: done.
//   3. The winner's row is widened into 1 KiB of LDS by the first C / 8 threads (8 channels each). Barrier. (The slots of step 1 are
//      next written behind this barrier, after every thread has read them.)
//   4. Similarity pass: the chain of every alive candidate against the LDS row; the order inside a chain is that of
//      oracle/c/sim_chain.c: chunk c of 8, k = 8c+i then 8c+4+i. v > m raises the penalty, v >= max_sim clears the alive bit. The rows
//      are re-read every step; they stay in L2 (kin * C * esize <= 4 MiB). Two forms:
//      STAGED (every non-empty segment has the same dtype, a compile-time constant): a wave copies its 64 rows of slot j into its own
//      LDS image 128 bytes at a time, one wave load = 8 rows x 128 B, whole cache lines, each fetched once; then every lane reads its
//      row's 128 bytes back (conflict-free 16-byte reads) and advances its chain. No block barrier inside.
//      DIRECT (segments of different dtypes; the dtype is read per candidate): thread-per-candidate gather from global memory, one
//      chunk of 8 elements at a time, up to four chains interleaved. A lane uses 16 bytes of a cache line per load, and lines are
//      fetched again once the waves of a CU have more rows in flight than its 32 KiB L1 holds: at kin = 1024 this form ran 8 times
//      slower than the staged one, which is why tables of one dtype do not use it.
//   The loop leaves (uniformly) when no slot holds an entry; the rest of the k outputs get (-inf, -1, -1, -inf).
// Arithmetic: `#pragma clang fp contract(off)` holds for the whole file, so f is four separately rounded operations and an int8 value's
// (float)q * scale is never fused into the chain; the chain's explicit fmaf stays an fma.
#include "segrows.h"

#pragma clang fp contract(off)

namespace {

constexpr int DV_CMAX = 256;                   // embedding width limit of the searches
constexpr int DV_NI = 4;                       // most candidates per thread (the direct form interleaves their chains)

// the staged similarity pass (every table of ONE storage dtype): per wave an LDS image of 64 rows x 128 bytes, rows 144 bytes apart
constexpr int DV_TILE_ROWB = 128, DV_TILE_STRIDE = 144, DV_TILE_BYTES = 64 * DV_TILE_STRIDE;
constexpr int DV_WIDE_THREADS = 256;           // up to that many threads a block has one thread per candidate

// seg_load8 for this file: a table of one dtype takes the shared loader (same code); the mixed kernel keeps its own spelling, one load per
// element size and then seg_widen8. With seg_load8 as the header has it the kernel compiled to shorter code (1913 against 2132 lines)
// that measured 31 % slower, 1181 -> 1544 us at kin = 256, k = 50 (profiles/row_tables_ab_shared.jsonl); with the 16-bit load shared by
// bf16 and fp16, 30 % (profiles/row_tables_ab_common16.jsonl). DESIGN.md has both runs
template <int DT> __device__ __forceinline__ void dv_load8(u64 row, int dt, float rs, int s, float (&g)[8]) {
  if constexpr (DT >= 0) return seg_load8<DT>(row, dt, rs, s, g);
  unsigned w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (dt == COR_F32) {
    const u32x4 x = *(const SEG_GLOBAL u32x4*)(row + 32u * s), y = *(const SEG_GLOBAL u32x4*)(row + 32u * s + 16u);
    w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = x[3]; w[4] = y[0]; w[5] = y[1]; w[6] = y[2]; w[7] = y[3];
  } else if (dt == COR_I8) {
    const u32x2 x = *(const SEG_GLOBAL u32x2*)(row + 8u * s);
    w[0] = x[0]; w[1] = x[1];
  } else {
    const u32x4 x = *(const SEG_GLOBAL u32x4*)(row + 16u * s);
    w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = x[3];
  }
  seg_widen8<DT>(w, dt, rs, g);
}

// does entry a (value fa at position pa) win against entry b? A position < 0 is no entry. Equal values (-0.0 == +0.0): the smaller id,
// then the smaller position; the ids are read only then, and only at positions of this query's list
__device__ __forceinline__ bool dv_wins(float fa, int pa, float fb, int pb, const long long* __restrict__ ids) {
  if (pa < 0) return false;
  if (pb < 0) return true;
  if (fa > fb) return true;
  if (fb > fa) return false;
  const long long ia = ids[pa], ib = ids[pb];
  if (ia != ib) return ia < ib;
  return pa < pb;
}

template <int DT>
__global__ __launch_bounds__(1024) void diversify_mmr_kernel(const SegRowsSq segs, int nseg, const float* __restrict__ scores,
                                                             const long long* __restrict__ idx, int kin, int C, float lam, float max_sim, int k,
                                                             unsigned* __restrict__ out_scores, long long* __restrict__ out_idx,
                                                             int* __restrict__ out_pos, float* __restrict__ out_value) {
  constexpr bool STAGED = DT >= 0;                                 // one storage dtype: the rows go through LDS in step 4
  extern __shared__ __align__(16) unsigned char dv_tiles[];        // STAGED: DV_TILE_BYTES per wave
  __shared__ __align__(16) float s_wrow[DV_CMAX];                  // the winner's row, widened
  __shared__ u64 s_row[16];                                        // per wave: its best alive entry
  __shared__ float s_f[16], s_rs[16];
  __shared__ int s_p[16], s_dt[16];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, nwaves = T >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long* ids = idx + (long long)blockIdx.x * kin;
  const float* sc = scores + (long long)blockIdx.x * kin;
  const long long out0 = (long long)blockIdx.x * k;

  // 0. presence and state: positions tid + j T, j < DV_NI (host: DV_NI * T >= kin)
  u64 row[DV_NI];
  float rs[DV_NI], s[DV_NI], m[DV_NI];
  int dts = 0, alive = 0;                                          // byte j: the dtype of candidate j; bit j: candidate j is alive
#pragma unroll
  for (int j = 0; j < DV_NI; ++j) {
    const int pos = tid + j * T;
    row[j] = 0; rs[j] = 0.f; s[j] = 0.f; m[j] = 0.f;
    if (pos < kin) {
      int dt = COR_F32;
      u64 r = 0;
      float sr = 0.f;
      // the only place a row address is formed
      const bool present = seg_lookup(segs, nseg, ids[pos], [&](int sg, u64 local) { seg_row(segs, sg, local, C, dt, r, sr); });
      if (present) {                                               // a missing entry's score is never read
        row[j] = r; rs[j] = sr; s[j] = sc[pos];
        dts |= dt << (8 * j);
        alive |= 1 << j;
      }
    }
  }
  const float oml = 1.0f - lam;

  int t = 0;
  while (t < k) {
    // 1. the best alive entry: thread, wave, block
    float bf = 0.f;
    int bp = -1;
#pragma unroll
    for (int j = 0; j < DV_NI; ++j)
      if (alive >> j & 1) {
        const float f = (lam * s[j]) - (oml * m[j]);
        if (dv_wins(f, tid + j * T, bf, bp, ids)) { bf = f; bp = tid + j * T; }
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float of = __shfl_xor(bf, o, 64);
      const int op = __shfl_xor(bp, o, 64);
      if (dv_wins(of, op, bf, bp, ids)) { bf = of; bp = op; }
    }
    bf = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(bf)));   // ONE answer per wave, whatever the values were
    bp = __builtin_amdgcn_readfirstlane(bp);
    if (bp < 0) {
      if (lane == 0) s_p[wave] = -1;
    } else if ((bp & (T - 1)) == tid) {                            // the owner: position bp = tid + j T is one of its alive candidates
      const int j = bp / T;
      s_f[wave] = bf;
      s_p[wave] = bp;
      s_row[wave] = j == 0 ? row[0] : j == 1 ? row[1] : j == 2 ? row[2] : row[3];
      s_rs[wave] = j == 0 ? rs[0] : j == 1 ? rs[1] : j == 2 ? rs[2] : rs[3];
      s_dt[wave] = dts >> (8 * j) & 0xff;
    }
    __syncthreads();
    float wf = 0.f;
    int wp = -1, ww = 0;
    for (int w = 0; w < nwaves; ++w) {
      const int p = s_p[w];
      const float f = p < 0 ? 0.f : s_f[w];
      if (dv_wins(f, p, wf, wp, ids)) { wf = f; wp = p; ww = w; }
    }
    if (wp < 0) break;                                             // nothing is alive (every thread sees the same slots)

    // 2. the winner goes out and leaves the alive set
    if (tid == 0) {
      out_scores[out0 + t] = ((const unsigned*)sc)[wp];            // the input score's bits
      out_idx[out0 + t] = ids[wp];
      if (out_pos) out_pos[out0 + t] = wp;
      if (out_value) out_value[out0 + t] = wf;
    }
    if ((wp & (T - 1)) == tid) alive &= ~(1 << (wp / T));
    ++t;
    if (t == k) break;

    // 3. its row, widened, into LDS
    if (tid < C / 8) {
      float g[8];
      dv_load8<DT>(s_row[ww], s_dt[ww], s_rs[ww], tid, g);
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        f32x4 x;
        x[0] = g[4 * v]; x[1] = g[4 * v + 1]; x[2] = g[4 * v + 2]; x[3] = g[4 * v + 3];
        ((f32x4*)s_wrow)[2 * tid + v] = x;
      }
    }
    __syncthreads();

    // 4. the similarity of every alive entry to the winner
    if constexpr (STAGED) {
      // Rows through LDS, the wave on its own (no block barrier): for candidate slot j the wave's 64 rows are copied 128 bytes at a
      // time, one wave load = 8 rows x 128 B (8 lanes x 16 B per row: whole cache lines, each fetched once), into a [64][144 B] image
      // (the 16 B of padding make the 16-byte reads below conflict-free); then every lane reads ITS row's 128 bytes back and advances its
      // chain. Every lane takes part in the copy, alive or not; a row that is not alive, and bytes past the row's end, are stored as 0.
      constexpr int ESZ = DT == COR_F32 ? 4 : DT == COR_I8 ? 1 : 2;
      constexpr int CB = 8 * ESZ;                                    // bytes of one chunk of the chain (8 elements)
      unsigned char* tile = dv_tiles + wave * DV_TILE_BYTES;
      const int RB = C * ESZ;                                        // bytes of a row (a multiple of 16)
      const int sub = lane & 7, grp = lane >> 3;
#pragma unroll
      for (int j = 0; j < DV_NI; ++j) {
        const bool mine = alive >> j & 1;
        if (__ballot(mine) == 0) continue;                           // (wave-uniform) nobody's slot j is alive
        const u64 send = mine ? row[j] : 0;
        const unsigned slo = (unsigned)send, shi = (unsigned)(send >> 32);
        float a = 0.f;
        for (int o = 0; o < RB; o += DV_TILE_ROWB) {
          u32x4 v[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int src = 8 * i + grp;
            const u64 rp = ((u64)(unsigned)__shfl((int)shi, src, 64) << 32) | (unsigned)__shfl((int)slo, src, 64);
            const int off = o + 16 * sub;
            v[i] = u32x4{0u, 0u, 0u, 0u};
            if (rp != 0 && off < RB) v[i] = *(const SEG_GLOBAL u32x4*)(rp + (unsigned)off);   // inside the row: off + 16 <= RB
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) *(u32x4*)(tile + (8 * i + grp) * DV_TILE_STRIDE + 16 * sub) = v[i];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          const unsigned char* mine_row = tile + lane * DV_TILE_STRIDE;
#pragma unroll
          for (int u = 0; u < DV_TILE_ROWB / CB; ++u) {
            if (o + u * CB < RB) {                                   // (wave-uniform) chunk o / CB + u of the chain exists
              unsigned w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
              if constexpr (ESZ == 1) {
                const uint2 x = *(const uint2*)(mine_row + u * CB);
                w[0] = x.x; w[1] = x.y;
              } else {
#pragma unroll
                for (int h = 0; h < CB / 16; ++h) {
                  const u32x4 x = *(const u32x4*)(mine_row + u * CB + 16 * h);
                  w[4 * h] = x[0]; w[4 * h + 1] = x[1]; w[4 * h + 2] = x[2]; w[4 * h + 3] = x[3];
                }
              }
              float g[8];
              seg_widen8<DT>(w, DT, rs[j], g);
              const int c = o / CB + u;
              const f32x4 q0 = ((const f32x4*)s_wrow)[2 * c], q1 = ((const f32x4*)s_wrow)[2 * c + 1];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                a = fmaf(g[i], q0[i], a);
                a = fmaf(g[4 + i], q1[i], a);
              }
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // the reads are done before the next copy overwrites the image
          __builtin_amdgcn_wave_barrier();
        }
        if (mine) {
          if (a > m[j]) m[j] = a;
          if (a >= max_sim) alive &= ~(1 << j);
        }
      }
    } else if (alive) {
      float acc[DV_NI] = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < C / 8; ++c) {
        float g[DV_NI][8];
#pragma unroll
        for (int j = 0; j < DV_NI; ++j) {
          if (alive >> j & 1) dv_load8<DT>(row[j], dts >> (8 * j) & 0xff, rs[j], c, g[j]);
          else {
#pragma unroll
            for (int e = 0; e < 8; ++e) g[j][e] = 0.f;
          }
        }
        const f32x4 q0 = ((const f32x4*)s_wrow)[2 * c], q1 = ((const f32x4*)s_wrow)[2 * c + 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int j = 0; j < DV_NI; ++j) acc[j] = fmaf(g[j][i], q0[i], acc[j]);
#pragma unroll
          for (int j = 0; j < DV_NI; ++j) acc[j] = fmaf(g[j][4 + i], q1[i], acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < DV_NI; ++j)
        if (alive >> j & 1) {
          if (acc[j] > m[j]) m[j] = acc[j];                        // strict: the penalty is never negative, no +-0 ambiguity
          if (acc[j] >= max_sim) alive &= ~(1 << j);               // suppressed for good
        }
    }
  }

  // the tail: slots past the last winner
  for (int u = t + tid; u < k; u += T) {
    out_scores[out0 + u] = RANK_NEG_INF;
    out_idx[out0 + u] = -1;
    if (out_pos) out_pos[out0 + u] = -1;
    if (out_value) out_value[out0 + u] = __uint_as_float(RANK_NEG_INF);
  }
}

template <int DT>
int launch_diversify(const SegRowsSq& segs, int nseg, const float* scores, const long long* idx, int Bq, int kin, int C, float lam, float max_sim,
                     int k, float* out_scores, long long* out_idx, int* out_pos, float* out_value, hipStream_t st) {
  const int npad = next_pow2(kin);
  const int wide = npad < DV_WIDE_THREADS ? npad : DV_WIDE_THREADS;  // one candidate per thread up to DV_WIDE_THREADS threads
  const int threads = npad / DV_NI > wide ? npad / DV_NI : wide < 64 ? 64 : wide;   // a power of two in [64, 1024]; DV_NI * threads >= kin
  const size_t lds = DT >= 0 ? (size_t)(threads / 64) * DV_TILE_BYTES : 0;   // 9 KiB (64 threads) .. 144 KiB (1024) of dynamic LDS
  if (DT >= 0) {
    static DevOnce once;
    cor_max_dyn_lds((const void*)diversify_mmr_kernel<DT>, 16 * DV_TILE_BYTES, once);
  }
  hipLaunchKernelGGL(diversify_mmr_kernel<DT>, dim3((unsigned)Bq), dim3(threads), lds, st, segs, nseg, scores, idx, kin, C, lam, max_sim, k,
                     (unsigned*)out_scores, out_idx, out_pos, out_value);
  COR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int cor_diversify_mmr(const void* const* seg_rows, const float* const* seg_scale, const long long* seg_offset, const int* seg_n,
                                 const int* seg_dtype, int nseg, const float* scores, const long long* idx, int Bq, int kin, int C, float lam,
                                 float max_sim, int k, float* out_scores, long long* out_idx, int* out_pos, float* out_value, void* stream) {
  if (!scores || !idx || !out_scores || !out_idx || Bq < 0 || kin < 1 || k < 1 || nseg < 0 || C < 1) return COR_EINVAL;
  if (!(lam >= 0.f && lam <= 1.f) || max_sim != max_sim) return COR_EINVAL;   // (a NaN lam fails both comparisons)
  const SegArrays t = {seg_rows, seg_scale, seg_offset, seg_n, seg_dtype, nseg, true};
  if (const int rc = seg_table_check(t)) return rc;
  if (kin > COR_MERGE_NMAX || k > COR_TOPK_KMAX || C > DV_CMAX || C % 16 != 0) return COR_ENOSUPPORT;
  SegRowsSq segs;
  int seen = 0;
  if (const int rc = seg_table_fill(t, false, segs, nseg, seen)) return rc;
  if (Bq == 0) return 0;
  return seg_dispatch_dtype(seen, [&](auto dt) {
    return launch_diversify<decltype(dt)::value>(segs, nseg, scores, idx, Bq, kin, C, lam, max_sim, k, out_scores, out_idx, out_pos, out_value,
                                                 (hipStream_t)stream);
  });
}
